// The sparse power-flow plan (powerflow_plan.cpp builds it on the host, powerflow_sparse.hip reads it on the device,
// tests/powerflow_sparse_ref.py interprets it in numpy): ONE relocatable blob of int32 words, no pointers.  A header of PFP_HEADER_WORDS
// words, then the sections it names by BYTE offset from the start of the blob, each 16-byte aligned:
//   order   int32 [n - 1]        the non-slack buses in elimination order (minimum degree of the bus graph, ties to the lowest id)
//   ua, uv  int32 [n] each       unknown number of theta_i / Vm_i, -1 where it is none; a bus's theta sits directly before its Vm
//   colptr  int32 [m + 1]        column j of the filled pattern is the slab segment [colptr[j], colptr[j + 1])
//   diag    int32 [m]            slab position of the diagonal of column j: U part before it, L part behind it
//   rowidx  uint16 or int32 [nnz]  row of every slab position, ascending inside a column (16-bit where the header says so)
//   adjptr  int32 [n + 1]        bus i's line ends are adj[adjptr[i] .. adjptr[i + 1]), in stored order (line k side 0, then side 1)
//   adj     int32 [n_adj][2]     (2 * line + side, the bus at the other end); side 1: the stored line read backwards
//   adjpos  int32 [n_adj][4]     slab positions of the entries that line end adds to: (theta_i, theta_j), (theta_i, Vm_j),
//                                (Vm_i, theta_j), (Vm_i, Vm_j) as (row, column); -1 where a row or a column is no unknown
//   buspos  int32 [n][4]         the same for the bus's own 2 x 2 diagonal block
#pragma once
#include <stdint.h>

namespace pfn {

constexpr int32_t PFP_MAGIC = 0x50465350;          // "PSFP"
constexpr int32_t PFP_VERSION = 1;
constexpr int PFP_HEADER_WORDS = 32;
enum {
    PFP_H_MAGIC = 0, PFP_H_VERSION, PFP_H_N, PFP_H_E, PFP_H_M, PFP_H_MODE,
    PFP_H_NNZ,                                      // slab positions per sample: U parts, diagonals and L parts
    PFP_H_NNZ_L,                                    // strictly-lower positions: nnz(L) without its unit diagonal
    PFP_H_MADDS_LO, PFP_H_MADDS_HI,                 // sum over the columns of (L length)^2: multiply-adds of one factorisation (int64)
    PFP_H_IDX16, PFP_H_MAX_COL,                     // rowidx is uint16; the longest L part
    PFP_H_N_ADJ, PFP_H_BYTES, PFP_H_SLACK,
    PFP_H_OFF_ORDER = 16, PFP_H_OFF_UA, PFP_H_OFF_UV, PFP_H_OFF_COLPTR, PFP_H_OFF_DIAG, PFP_H_OFF_ROWIDX, PFP_H_OFF_ADJPTR,
    PFP_H_OFF_ADJ, PFP_H_OFF_ADJPOS, PFP_H_OFF_BUSPOS
};

}  // namespace pfn
