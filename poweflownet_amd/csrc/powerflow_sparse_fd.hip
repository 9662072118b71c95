// The fast-decoupled modes on the sparse route (gfx950): pfn_powerflow_solve_sparse_fd, ONE launch, one workgroup per sample.  The
// semantics are the dense fast-decoupled route's (powerflow.hip, tests/powerflow_fd_ref.py): B' over the angle buses and B'' over the
// PQ buses are constant -- XB: B' from 1 / x, B'' from x / (r^2 + x^2); BX the other way round --, half-iterations alternate
// theta -= B'^-1 (dP / Vm) and Vm -= B''^-1 (dQ / Vm), the P half first, the fp64 mismatch is re-formed and tested after each, and
// the count is of half-iterations.  Where the dense route inverts the two matrices, this one keeps their sparse fp32 factors: the
// fast-decoupled plan (powerflow_plan.hpp) holds one symbolic factorisation per matrix, each is assembled and factored ONCE per
// sample (powerflow_sparse_core.hpp: the Newton kernel's left-looking column factorisation), and a half-iteration is one mismatch
// walk over the bus's line ends (one fp64 sincos per end, line sums in stored order) and one pair of fp64 substitutions.
//
// Every loop bound comes from the plan, so every barrier is reached by the whole workgroup; what fails a sample (a pivot, a
// non-finite mismatch) is a value all threads read behind a barrier, and they leave together.  One owner per target per step, no
// float atomics, only the max crosses threads: a sample's bits depend neither on its batch nor on the workgroup size.
#include "powerflow_plan.hpp"
#include "powerflow_sparse_core.hpp"

namespace pfn {

constexpr double PFD_RAD = 3.14159265358979323846 / 180.0;
constexpr int PFD_F_LDS_BYTES = 80 * 1024;         // w + the right-hand side in LDS up to here (powerflow_sparse.hip's rule)
enum { PFD_NOT_CONVERGED = -1, PFD_SINGULAR = -2, PFD_NON_FINITE = -3, PFD_BAD_TYPES = -5, PFD_STALE_PLAN = -6 };

struct PfdArgs {
    const int64_t* edge_index;
    const double* rx;
    const int32_t* bus_type;
    const double* spec;
    const double* init;
    const int32_t* plan;
    double* table;
    int32_t* status;
    double* residual;
    int32_t* flags;
    unsigned char* ws;
    size_t ws_stride;
    double tol;
    int n, e, m_p, m_q, nnz, bx, max_iter, f_in_lds;
};

// per sample: double vm, th, sp, sq [n], F [max(m_p, m_q)]; then the two fp32 slabs, P's first ([nnz] together); rounded to 16 bytes
__host__ __device__ inline size_t pfd_sample_bytes(int n, int mmax, int nnz) {
    return (((size_t)8 * (4 * (size_t)n + mmax) + (size_t)4 * nnz) + 15) & ~(size_t)15;
}
__host__ __device__ inline bool pfd_f_in_lds(int mmax) { return (size_t)12 * mmax <= (size_t)PFD_F_LDS_BYTES; }
__host__ __device__ inline size_t pfd_w_bytes(int mmax) { return ((size_t)4 * mmax + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pfd_lds_bytes(int mmax) { return pfd_w_bytes(mmax) + (pfd_f_in_lds(mmax) ? (size_t)8 * mmax : 0) + 16; }

// the sections of one embedded sub-plan
struct PfdHalf {
    const int32_t* ua;
    const int32_t* adjptr;
    const int2* adj;
    const int4* adjpos;
    const int4* buspos;
    PfcMatrix A;
    int nnz;
};

__device__ __forceinline__ PfdHalf pfd_half(const unsigned char* pb) {
    const int32_t* H = reinterpret_cast<const int32_t*>(pb);
    PfdHalf h;
    h.ua = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_UA]);
    h.adjptr = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_ADJPTR]);
    h.adj = reinterpret_cast<const int2*>(pb + H[PFP_H_OFF_ADJ]);
    h.adjpos = reinterpret_cast<const int4*>(pb + H[PFP_H_OFF_ADJPOS]);
    h.buspos = reinterpret_cast<const int4*>(pb + H[PFP_H_OFF_BUSPOS]);
    h.A.colptr = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_COLPTR]);
    h.A.diag = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_DIAG]);
    h.A.row = reinterpret_cast<const uint16_t*>(pb + H[PFP_H_OFF_ROWIDX]);      // (the launcher refuses 32-bit ids)
    h.A.m = H[PFP_H_M];
    h.nnz = H[PFP_H_NNZ];
    return h;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void powerflow_sparse_fd_kernel(const PfdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfd_smem[];
    __shared__ double s_red[THREADS / 64];
    const int t = threadIdx.x;
    constexpr int nt = THREADS;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, nnz = a.nnz;
    const int mmax = max(a.m_p, a.m_q);
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(a.plan);
    const int32_t* H = a.plan;
    const PfdHalf hp = pfd_half(pb + H[PFD_H_OFF_P]), hq = pfd_half(pb + H[PFD_H_OFF_Q]);
    const int slack = H[PFP_H_SLACK];

    double* vm = reinterpret_cast<double*>(a.ws + (size_t)s * a.ws_stride);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* Fg = sq + n;
    float* slab_p = reinterpret_cast<float*>(Fg + mmax);
    float* slab_q = slab_p + hp.nnz;
    float* w = reinterpret_cast<float*>(pfd_smem);
    double* F = a.f_in_lds ? reinterpret_cast<double*>(pfd_smem + pfd_w_bytes(mmax)) : Fg;
    const double* init = a.init ? a.init + (int64_t)s * 2 * n : nullptr;
    const double* rx = a.rx + (int64_t)s * 2 * e;
    const double* spec = a.spec + (int64_t)s * 4 * n;
    double* out = a.table + (int64_t)s * 4 * n;
    const double nanv = __builtin_nan("");
    int code = 0;                                   // (uniform over the workgroup wherever it is tested)
    double res = nanv;

    // ---- the device arrays against the plan, both halves: the bus types decide who has an unknown in B' and in B'' (a PV bus the
    // plan took for PQ is noticed here), the line list the line ends.  A plan whose sizes disagree with the outer header (it cannot
    // come from the builder) is refused before anything is indexed with them.
    int odd = 0, stale = hp.A.m != a.m_p || hq.A.m != a.m_q || hp.nnz + hq.nnz != nnz;
    if (!stale) {
        for (int i = t; i < n; i += nt) {
            const int ty = a.bus_type[i];
            odd |= (unsigned)ty > 2u || (ty != 0) != (hp.ua[i] >= 0) || (ty == 2) != (hq.ua[i] >= 0);
            stale |= hp.adjptr[i] != hq.adjptr[i] || hp.adjptr[i + 1] != hq.adjptr[i + 1];
            for (int q = hp.adjptr[i]; q < hp.adjptr[i + 1]; ++q) {
                const int2 lj = hp.adj[q];
                const int k = lj.x >> 1, side = lj.x & 1;
                if ((unsigned)k >= (unsigned)e) { stale = 1; continue; }
                stale |= a.edge_index[side ? e + k : k] != (int64_t)i || a.edge_index[side ? k : e + k] != (int64_t)lj.y;
            }
        }
    }
    odd = __syncthreads_or(odd);
    stale = __syncthreads_or(stale);
    if (odd) {
        code = PFD_BAD_TYPES;
        if (t == 0) a.flags[0] = a.flags[0] | 1;    // (every writer stores the same bit over the same word)
    } else if (stale) {
        code = PFD_STALE_PLAN;
    }
    if (code == 0) {
        // (the two halves were built from one line list: their line ends agree where that list is the device's; checked all the same)
        int differ = 0;
        for (int q = t; q < 2 * e; q += nt) {
            const int2 x = hp.adj[q], y = hq.adj[q];
            differ |= x.x != y.x || x.y != y.y;
        }
        if (__syncthreads_or(differ)) code = PFD_STALE_PLAN;
    }

    int it = 0;
    if (code == 0) {
        // ---- flat start, or the caller's: Va at the non-slack buses, Vm at the PQ buses
        const double th0 = spec[4 * slack + 1] * PFD_RAD;
        int wild = 0;
        for (int i = t; i < n; i += nt) {
            const int ty = a.bus_type[i];
            double v = ty == 2 ? 1.0 : spec[4 * i], ang = th0;
            if (init) {
                if (ty == 2) v = init[2 * i];
                if (ty != 0) ang = init[2 * i + 1] * PFD_RAD;
                wild |= !(fabs(v) < __builtin_inf()) || !(fabs(ang) < __builtin_inf());
            }
            vm[i] = v;
            th[i] = ang;
        }
        if (__syncthreads_or(wild)) code = PFD_NON_FINITE;
    }
    if (code == 0) {
        // ---- B' and B'': bus i's owner adds the off-diagonals of its row at their planned positions, line ends in stored order
        // (parallel lines add), and the diagonal -- summed in fp64 -- last
        for (int k = t; k < nnz; k += nt) slab_p[k] = 0.f;
        __syncthreads();
        for (int i = t; i < n; i += nt) {
            double dp = 0.0, dq = 0.0;
            const int q1 = hp.adjptr[i + 1];
            for (int q = hp.adjptr[i]; q < q1; ++q) {
                const int k = hp.adj[q].x >> 1;
                const int pp = hp.adjpos[q].x, pq = hq.adjpos[q].x;
                const double r = rx[2 * k], x = rx[2 * k + 1];
                const double w_x = 1.0 / x, w_b = x / (r * r + x * x);
                const double wp = a.bx ? w_b : w_x, wq = a.bx ? w_x : w_b;
                dp += wp;
                dq += wq;
                if (pp >= 0) slab_p[pp] += (float)(-wp);
                if (pq >= 0) slab_q[pq] += (float)(-wq);
            }
            const int bp = hp.buspos[i].x, bq = hq.buspos[i].x;
            if (bp >= 0) slab_p[bp] += (float)dp;
            if (bq >= 0) slab_q[bq] += (float)dq;
        }
        __syncthreads();
        // ---- both factors, once
        if (!pfc_factor<THREADS>(hp.A, slab_p, w)) code = PFD_SINGULAR;
        __syncthreads();
        if (code == 0 && !pfc_factor<THREADS>(hq.A, slab_q, w)) code = PFD_SINGULAR;
        __syncthreads();
    }
    if (code == 0) {
        int half = 0;
        for (;; ++it) {
            // ---- line sums of bus i, its line ends in stored order; the mismatch; the right-hand side of the coming half
            double mx = 0.0;
            for (int i = t; i < n; i += nt) {
                const double vi = vm[i], ti = th[i];
                double sP = 0.0, sQ = 0.0;
                const int q1 = hp.adjptr[i + 1];
                for (int q = hp.adjptr[i]; q < q1; ++q) {
                    const int2 lj = hp.adj[q];
                    const int k = lj.x >> 1, j = lj.y;
                    const double r = rx[2 * k], x = rx[2 * k + 1];
                    const double d = r * r + x * x, g = r / d, b = -x / d;
                    const double vv = vi * vm[j];
                    double sn, cs;
                    sincos(ti - th[j], &sn, &cs);
                    const double t1 = vv * cs - vi * vi, t2 = vv * sn;
                    sP += g * t1 + b * t2;
                    sQ += g * t2 - b * t1;
                }
                sp[i] = sP;
                sq[i] = sQ;
                const int ra = hp.ua[i], rv = hq.ua[i];
                if (ra >= 0) {
                    const double f = spec[4 * i + 2] - sP, af = fabs(f);
                    mx = fmax(mx, af < __builtin_inf() ? af : __builtin_inf());
                    if (half == 0) F[ra] = f / vi;
                }
                if (rv >= 0) {
                    const double f = spec[4 * i + 3] - sQ, af = fabs(f);
                    mx = fmax(mx, af < __builtin_inf() ? af : __builtin_inf());
                    if (half == 1) F[rv] = f / vi;
                }
            }
            res = pfc_block_max<THREADS>(mx, s_red);
            if (!(res < __builtin_inf())) { code = PFD_NON_FINITE; break; }
            if (res < a.tol) break;
            if (it >= a.max_iter) { code = PFD_NOT_CONVERGED; break; }
            // ---- the half-iteration: fp64 substitutions through the half's factor, then theta -= dx or Vm -= dx
            if (half == 0) {
                pfc_substitute<THREADS>(hp.A, slab_p, F);
                for (int i = t; i < n; i += nt) {
                    const int ra = hp.ua[i];
                    if (ra >= 0) th[i] -= pfc_solution(hp.A, slab_p, F, ra);
                }
            } else {
                pfc_substitute<THREADS>(hq.A, slab_q, F);
                for (int i = t; i < n; i += nt) {
                    const int rv = hq.ua[i];
                    if (rv >= 0) vm[i] -= pfc_solution(hq.A, slab_q, F, rv);
                }
            }
            half = a.m_q ? 1 - half : 0;
            __syncthreads();
        }
    }

    // ---- the table: slack P, Q and PV Q are the aggregated line sums of the last pass; a failed sample's rows are NaN
    for (int i = t; i < n; i += nt) {
        double4 row = make_double4(nanv, nanv, nanv, nanv);
        if (code == 0) {
            const int ty = a.bus_type[i];
            row.x = vm[i];
            row.y = ty == 0 ? spec[4 * i + 1] : th[i] * (1.0 / PFD_RAD);
            row.z = ty == 0 ? sp[i] : spec[4 * i + 2];
            row.w = ty == 2 ? spec[4 * i + 3] : sq[i];
        }
        *reinterpret_cast<double4*>(out + 4 * i) = row;
    }
    if (t == 0) {
        a.status[s] = code ? code : it;
        a.residual[s] = res;
    }
}

static int pfd_check_header(const int32_t* h, const char* who) {
    PFN_CHECK_ARG(h, "%s: null plan header", who);
    PFN_CHECK_ARG(h[PFP_H_MAGIC] == PFD_MAGIC && h[PFP_H_VERSION] == PFP_VERSION && h[PFP_H_MODE] == PFD_MODE,
                  "%s: not a fast-decoupled sparse power-flow plan (magic %08x, version %d)", who, (unsigned)h[PFP_H_MAGIC], (int)h[PFP_H_VERSION]);
    PFN_CHECK_ARG(h[PFP_H_N] >= 1 && h[PFP_H_E] >= 0 && h[PFP_H_M] >= 0 && h[PFD_H_M_Q] >= 0 && h[PFD_H_M_Q] <= h[PFP_H_M] &&
                      h[PFP_H_M] < h[PFP_H_N] && h[PFP_H_NNZ] >= h[PFP_H_M] + h[PFD_H_M_Q] && h[PFD_H_OFF_P] >= 4 * PFP_HEADER_WORDS &&
                      h[PFD_H_OFF_Q] > h[PFD_H_OFF_P] && h[PFD_H_OFF_Q] < h[PFP_H_BYTES] && ((h[PFD_H_OFF_P] | h[PFD_H_OFF_Q]) & 15) == 0,
                  "%s: the plan header is inconsistent", who);
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_sparse_fd_workspace_bytes(int64_t n_samples, const void* plan_header) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || pfd_check_header(h, "pfn_powerflow_sparse_fd_workspace_bytes") != PFN_OK) return 0;
    return (size_t)n_samples * pfd_sample_bytes(h[PFP_H_N], std::max(h[PFP_H_M], h[PFD_H_M_Q]), h[PFP_H_NNZ]);
}

int pfn_powerflow_solve_sparse_fd(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                                  const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
                                  const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status,
                                  double* residual, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "pfn_powerflow_solve_sparse_fd";
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PFN_TRY(pfd_check_header(h, who));
    PFN_CHECK_ARG(n_samples >= 0 && n_samples < (1ll << 29), "%s: bad sample count %lld", who, (long long)n_samples);
    PFN_CHECK_ARG(mode == 2 || mode == 3, "%s: mode must be 2 (fdxb) or 3 (fdbx); modes 0 and 1 are pfn_powerflow_solve_sparse's", who);
    PFN_CHECK_ARG(h[PFP_H_N] == n_bus && h[PFP_H_E] == n_lines, "%s: the plan is for %d buses, %d lines; the call has %lld, %lld", who,
                  (int)h[PFP_H_N], (int)h[PFP_H_E], (long long)n_bus, (long long)n_lines);
    PFN_CHECK_ARG(max_iter >= 0 && tol > 0.0, "%s: max_iter must be >= 0 and tol > 0", who);
    PFN_CHECK_ARG(threads == 0 || threads == 64 || threads == 256, "%s: threads must be 0 (the default), 64 or 256", who);
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(rx || n_lines == 0, "%s: null rx", who);
    PFN_CHECK_ARG(edge_index || n_lines == 0, "%s: null edge_index", who);
    PFN_CHECK_ARG(bus_type && spec && table && status && residual && flags && plan_dev, "%s: null pointer", who);
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 31) == 0 && ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(plan_dev)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(edge_index) |
                        reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(init)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(bus_type) | reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(flags)) & 3) == 0,
                  "%s: table must be 32-byte aligned, the workspace and the plan 16-byte, fp64 and int64 inputs 8-byte, int32 arrays 4-byte", who);
    const int n = h[PFP_H_N], m_p = h[PFP_H_M], m_q = h[PFD_H_M_Q], nnz = h[PFP_H_NNZ], mmax = std::max(m_p, m_q);
    PFN_CHECK_ARG(h[PFP_H_IDX16] != 0, "%s: %d unknowns: the kernel takes plans with 16-bit row ids (m <= 65535) only", who, mmax);
    const size_t lds = pfd_lds_bytes(mmax);
    PFN_CHECK_ARG(lds <= (size_t)(kLdsCuBytes - kLdsReserve), "%s: a work vector of %d unknowns needs %zu bytes of LDS, %d are there", who, mmax, lds,
                  kLdsCuBytes - kLdsReserve);
    const size_t stride = pfd_sample_bytes(n, mmax, nnz), need = (size_t)n_samples * stride;
    if (!ws || ws_bytes < need) {
        set_error("%s: the workspace must hold %zu bytes (got %zu)", who, need, ws ? ws_bytes : (size_t)0);
        return PFN_ENOSPACE;
    }
    PfdArgs a;
    a.edge_index = edge_index;
    a.rx = rx;
    a.bus_type = bus_type;
    a.spec = spec;
    a.init = init;
    a.plan = static_cast<const int32_t*>(plan_dev);
    a.table = table;
    a.status = status;
    a.residual = residual;
    a.flags = flags;
    a.ws = static_cast<unsigned char*>(ws);
    a.ws_stride = stride;
    a.tol = tol;
    a.n = n;
    a.e = h[PFP_H_E];
    a.m_p = m_p;
    a.m_q = m_q;
    a.nnz = nnz;
    a.bx = mode == 3;
    a.max_iter = max_iter;
    a.f_in_lds = pfd_f_in_lds(mmax);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double madds = (double)(((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]);
    // (the model: one factor of each half, and some twenty half-iterations of one pair of substitutions and one mismatch walk)
    ProfScope ps(mode == 3 ? "powerflow_sparse_fdbx" : "powerflow_sparse_fdxb",
                 (double)n_samples * ((double)n_lines * 16.0 + (double)n * 64.0 + (init ? (double)n * 16.0 : 0.0)) + (double)h[PFP_H_BYTES],
                 (double)n_samples * 2.0 * (madds + 20.0 * (double)h[PFP_H_NNZ]), s);
    // powerflow_sparse.hip's rule: one wave per sample until the longest column exceeds 128 (DESIGN 7l has this kernel's numbers)
    const int use = threads ? threads : (h[PFP_H_MAX_COL] > 128 ? 256 : 64);
    static std::atomic<uint64_t> raised64{0}, raised256{0};
    if (use == 64) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_sparse_fd_kernel<64>), kLdsCuBytes - kLdsReserve, raised64));
        powerflow_sparse_fd_kernel<64><<<(int)n_samples, 64, lds, s>>>(a);
    } else {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_sparse_fd_kernel<256>), kLdsCuBytes - kLdsReserve, raised256));
        powerflow_sparse_fd_kernel<256><<<(int)n_samples, 256, lds, s>>>(a);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
