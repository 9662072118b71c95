// The host side of the sparse fast-decoupled solve (powerflow_sparse_fd.hip owns and exports it, the way contingency_sparse.hip
// exports cs_launch_base): the check of a fast-decoupled plan header and the whole call -- its argument checks and the ONE launch of
// powerflow_sparse_fd_kernel -- under the name of the entry that makes it.  pfn_powerflow_solve_sparse_fd(_masked) is this call; the
// AC N-1 screen of the sparse route (contingency_ac_sparse.hip) makes it for its base launch, so its base table, status and
// residual are the solver's bits because they are the solver's kernel, and every sample's slab of `ws` (pf_sample_bytes' layout:
// fp64 vm, th, sp, sq [n], F [max(m_p, m_q)], then the fp32 factors of B' and B'') holds what the outage launch reads.
#pragma once
#include "powerflow_common.hpp"

namespace pfn {

int pfd_check_header(const int32_t* h, const char* who);
// `ws` needs n_samples * pf_sample_bytes(n, max(m_p, m_q), nnz) bytes (more is fine: the samples' slabs come first)
int pfd_solve(const char* who, const int64_t* edge_index, int64_t n_lines, const double* rx, const uint8_t* line_mask, const int32_t* unplaced,
              const int32_t* bus_type, const double* spec, const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
              const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status, double* residual, int32_t* flags, void* ws,
              size_t ws_bytes, void* stream);

}  // namespace pfn
