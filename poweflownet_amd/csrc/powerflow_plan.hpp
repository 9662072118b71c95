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
//
// The fast-decoupled plan (pfn_powerflow_sparse_fd_plan, read by powerflow_sparse_fd.hip and tests/powerflow_sparse_fd_ref.py) is ONE blob too:
// an OUTER header of PFP_HEADER_WORDS words in the positions above with PFD_MAGIC, mode PFD_MODE, n, e, slack and n_adj as above,
// M = m_p = n - 1 (the order of B'), PFD_H_M_Q = m_q = the number of PQ buses (the order of B''), NNZ / NNZ_L / MADDS / BYTES
// totals over both halves (BYTES: the whole blob), MAX_COL the larger half's, IDX16 set when both halves have 16-bit rows; its
// section-offset words are unused but for PFD_H_OFF_P and PFD_H_OFF_Q, the BYTE offsets of two embedded sub-plans.  Each sub-plan
// is a complete plan as described above -- its own header (PFP_MAGIC, mode 1, its own M, NNZ, ... and BYTES), then its sections at
// offsets FROM THE SUB-PLAN'S START -- for a matrix with one unknown per bus: uv is all -1 and only the first of the four adjpos /
// buspos positions is used.
//   P  B' over the n - 1 non-slack buses: byte for byte the mode-1 plan of the grid;
//   Q  B'' over the PQ buses: the bus graph induced on them (the slack and the PV buses left out), its own minimum-degree order
//      (`order` has m_q entries), ua[i] = -1 at every bus that is not PQ.  m_q = 0 is valid: empty sections.
// The launch and the workspace are sized from the outer header alone.
#pragma once
#include <stdint.h>

namespace pfn {

constexpr int32_t PFP_MAGIC = 0x50465350;          // "PSFP"
constexpr int32_t PFP_VERSION = 1;
constexpr int PFP_HEADER_WORDS = 32;
constexpr int32_t PFD_MAGIC = 0x44465350;          // "PSFD"
constexpr int32_t PFD_MODE = 2;
enum { PFD_H_M_Q = 15, PFD_H_OFF_P = 16, PFD_H_OFF_Q = 17 };
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
