// The sparse route of the batched power-flow solver (gfx950): pfn_powerflow_solve_sparse, ONE launch, one workgroup per sample, for
// grids beyond the dense cap of powerflow.hip (6470 buses: 10782 unknowns).  The same Newton loop -- fp64 state, mismatch and
// convergence test, an fp32 factor that "only has to point downhill", the right-hand side kept in fp64 -- on a factor that is sparse:
// the elimination order, the filled pattern and the place of every Jacobian entry come from the host plan (powerflow_plan.cpp,
// powerflow_plan.hpp), one per grid, shared by the samples.  No pivoting: the order is static; a pivot that is tiny or NaN fails the
// sample (-2) exactly as a zero pivot column does on the dense route.
//
// One pass:  (1) bus i's owner walks the plan's list of its line ends (O(degree): the dense kernel's scan of the whole line list would
// be 58 M loads at 6470), one fp64 sincos per end, and ADDS the end's Jacobian entries at their planned slab positions -- the slab is
// zeroed first, a (row, column) entry belongs to the row's bus alone, parallel lines add in stored order, the diagonal block is summed
// in fp64 registers and added last;  (2) max |F|, the dense route's stopping rule;  (3) left-looking factorisation by columns: column j
// is scattered into a dense fp32 work vector w [m] in LDS, then for every k of its U part, ascending, U_kj = w[k] is final and the
// lanes subtract L(:, k) U_kj at w[row] -- the pattern is closed under elimination, so every such row is a row of column j -- then the
// pivot test, and the column goes back to the slab with its L part times 1 / pivot;  (4) forward and backward substitution by columns
// on the fp64 right-hand side (in LDS while w and it take at most 80 KiB, else in the workspace);
// (5) x += dx.
//
// Every loop bound comes from the plan, so every barrier is reached by the whole workgroup; what fails a sample (a pivot, a
// non-finite mismatch) is a value all threads read after a barrier, and they leave the loop together.  No float atomics; only the max
// crosses threads.  The metadata of up to 64 columns (where their L parts begin and end) is loaded by the lanes at once and handed
// round with wave shuffles, and a thread's first element of the next L column is requested before the current step's barrier (an
// LDS-only barrier, device_prims.hpp): a k-step then waits for an LDS round trip and a barrier, not for three dependent loads.
// Steps (3) and (4) are powerflow_sparse_core.hpp's, shared with the fast-decoupled kernel (powerflow_sparse_fd.hip).
#include "pfn_internal.hpp"
#include "powerflow_plan.hpp"
#include "powerflow_sparse_core.hpp"

namespace pfn {

constexpr double PFS_RAD = 3.14159265358979323846 / 180.0;
constexpr int PFS_F_LDS_BYTES = 80 * 1024;         // w + F in LDS up to here (two workgroups per compute unit at least)
enum { PFS_NOT_CONVERGED = -1, PFS_SINGULAR = -2, PFS_NON_FINITE = -3, PFS_BAD_TYPES = -5, PFS_STALE_PLAN = -6 };

struct PfsArgs {
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
    int n, e, m, nnz, mode, max_iter, f_in_lds;
};

// per sample: double vm, th, sp, sq [n], F [m]; then the fp32 slab [nnz]; rounded to 16 bytes
__host__ __device__ inline size_t pfs_sample_bytes(int n, int m, int nnz) {
    return (((size_t)8 * (4 * (size_t)n + m) + (size_t)4 * nnz) + 15) & ~(size_t)15;
}
__host__ __device__ inline bool pfs_f_in_lds(int m) { return (size_t)12 * m <= (size_t)PFS_F_LDS_BYTES; }
__host__ __device__ inline size_t pfs_w_bytes(int m) { return ((size_t)4 * m + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pfs_lds_bytes(int m) { return pfs_w_bytes(m) + (pfs_f_in_lds(m) ? (size_t)8 * m : 0) + 16; }

template <int THREADS>
__global__ __launch_bounds__(THREADS) void powerflow_sparse_kernel(const PfsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfs_smem[];
    __shared__ double s_red[THREADS / 64];
    const int t = threadIdx.x;
    constexpr int nt = THREADS;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, m = a.m, nnz = a.nnz;
    const bool dc = a.mode == 1;
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(a.plan);
    const int32_t* H = a.plan;
    const int32_t* ua = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_UA]);
    const int32_t* uv = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_UV]);
    const int32_t* colptr = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_COLPTR]);
    const int32_t* diag = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_DIAG]);
    const uint16_t* row16 = reinterpret_cast<const uint16_t*>(pb + H[PFP_H_OFF_ROWIDX]);      // (the launcher refuses 32-bit ids)
    const int32_t* adjptr = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_ADJPTR]);
    const int2* adj = reinterpret_cast<const int2*>(pb + H[PFP_H_OFF_ADJ]);
    const int4* adjpos = reinterpret_cast<const int4*>(pb + H[PFP_H_OFF_ADJPOS]);
    const int4* buspos = reinterpret_cast<const int4*>(pb + H[PFP_H_OFF_BUSPOS]);
    const int slack = H[PFP_H_SLACK];
    const PfcMatrix A{colptr, diag, row16, m};

    double* vm = reinterpret_cast<double*>(a.ws + (size_t)s * a.ws_stride);
    double* th = vm + n;
    double* sp = th + n;
    double* sq = sp + n;
    double* Fg = sq + n;
    float* slab = reinterpret_cast<float*>(Fg + m);
    float* w = reinterpret_cast<float*>(pfs_smem);
    double* F = a.f_in_lds ? reinterpret_cast<double*>(pfs_smem + pfs_w_bytes(m)) : Fg;
    const double* init = a.init ? a.init + (int64_t)s * 2 * n : nullptr;
    const double* rx = a.rx + (int64_t)s * 2 * e;
    const double* spec = a.spec + (int64_t)s * 4 * n;
    double* out = a.table + (int64_t)s * 4 * n;
    const double nanv = __builtin_nan("");
    int code = 0;                                   // (uniform over the workgroup wherever it is tested)
    double res = nanv;

    // ---- the device arrays against the plan: the bus types decide the unknowns, the line list the line ends
    int odd = 0, stale = 0;
    for (int i = t; i < n; i += nt) {
        const int ty = a.bus_type[i];
        odd |= (unsigned)ty > 2u || (ty != 0) != (ua[i] >= 0) || (ty == 2 && !dc) != (uv[i] >= 0);
        for (int q = adjptr[i]; q < adjptr[i + 1]; ++q) {
            const int2 lj = adj[q];
            const int k = lj.x >> 1, side = lj.x & 1;
            stale |= a.edge_index[side ? e + k : k] != (int64_t)i || a.edge_index[side ? k : e + k] != (int64_t)lj.y;
        }
    }
    odd = __syncthreads_or(odd);
    stale = __syncthreads_or(stale);
    if (odd) {
        code = PFS_BAD_TYPES;
        if (t == 0) a.flags[0] = a.flags[0] | 1;    // (every writer stores the same bit over the same word)
    } else if (stale) {
        code = PFS_STALE_PLAN;
    }

    int it = 0;
    if (code == 0) {
        // ---- flat start, or the caller's: Va at the non-slack buses, Vm at the PQ buses (mode 1: Va only)
        const double th0 = spec[4 * slack + 1] * PFS_RAD;
        int wild = 0;
        for (int i = t; i < n; i += nt) {
            const int ty = a.bus_type[i];
            double v = ty == 2 ? 1.0 : spec[4 * i], ang = th0;
            if (init) {
                if (ty == 2 && !dc) v = init[2 * i];
                if (ty != 0) ang = init[2 * i + 1] * PFS_RAD;
                wild |= !(fabs(v) < __builtin_inf()) || !(fabs(ang) < __builtin_inf());
            }
            vm[i] = v;
            th[i] = ang;
        }
        if (__syncthreads_or(wild)) code = PFS_NON_FINITE;
    }
    if (code == 0) {
        for (;; ++it) {
            for (int k = t; k < nnz; k += nt) slab[k] = 0.f;
            __syncthreads();
            // ---- (1) line sums, mismatch and Jacobian entries of bus i, its line ends in stored order
            for (int i = t; i < n; i += nt) {
                const int ra = ua[i], rv = uv[i];
                const double vi = vm[i], ti = th[i];
                double sP = 0.0, sQ = 0.0, dPt = 0.0, dPv = 0.0, dQt = 0.0, dQv = 0.0;
                const int q1 = adjptr[i + 1];
                for (int q = adjptr[i]; q < q1; ++q) {
                    const int2 lj = adj[q];
                    const int4 pos = adjpos[q];
                    const int k = lj.x >> 1, j = lj.y;
                    const double r = rx[2 * k], x = rx[2 * k + 1];
                    if (dc) {
                        const double b = -1.0 / x;
                        sP += b * (ti - th[j]);
                        dPt += b;
                        if (pos.x >= 0) slab[pos.x] += (float)(-b);
                        continue;
                    }
                    const double d = r * r + x * x, g = r / d, b = -x / d;
                    const double vj = vm[j], vv = vi * vj;
                    double sn, cs;
                    sincos(ti - th[j], &sn, &cs);
                    const double t1 = vv * cs - vi * vi, t2 = vv * sn;
                    sP += g * t1 + b * t2;
                    sQ += g * t2 - b * t1;
                    const double pti = vv * (b * cs - g * sn), qti = vv * (g * cs + b * sn);
                    dPt += pti;
                    dPv += g * (vj * cs - 2.0 * vi) + b * vj * sn;
                    dQt += qti;
                    dQv += g * vj * sn - b * (vj * cs - 2.0 * vi);
                    if (pos.x >= 0) slab[pos.x] += (float)(-pti);
                    if (pos.y >= 0) slab[pos.y] += (float)(vi * (g * cs + b * sn));
                    if (pos.z >= 0) slab[pos.z] += (float)(-qti);
                    if (pos.w >= 0) slab[pos.w] += (float)(vi * (g * sn - b * cs));
                }
                sp[i] = sP;
                sq[i] = sQ;
                const int4 bp = buspos[i];
                if (ra >= 0) {
                    F[ra] = spec[4 * i + 2] - sP;
                    slab[bp.x] += (float)dPt;
                    if (rv >= 0) slab[bp.y] += (float)dPv;
                }
                if (rv >= 0) {
                    F[rv] = spec[4 * i + 3] - sQ;
                    slab[bp.z] += (float)dQt;
                    slab[bp.w] += (float)dQv;
                }
            }
            __syncthreads();
            // ---- (2) max |F| in fp64; a non-finite entry counts as +inf
            double mx = 0.0;
            for (int k = t; k < m; k += nt) {
                const double f = fabs(F[k]);
                mx = fmax(mx, f < __builtin_inf() ? f : __builtin_inf());
            }
            res = pfc_block_max<THREADS>(mx, s_red);
            if (!(res < __builtin_inf())) { code = PFS_NON_FINITE; break; }
            if (res < a.tol) break;
            if (it >= a.max_iter) { code = PFS_NOT_CONVERGED; break; }
            // ---- (3) left-looking factorisation in plan order (powerflow_sparse_core.hpp)
            if (!pfc_factor<THREADS>(A, slab, w)) { code = PFS_SINGULAR; break; }
            // ---- (4) L y = F, then U dx = y, by columns: after its step F[j] is final (the backward one leaves U_jj dx_j)
            pfc_substitute<THREADS>(A, slab, F);
            // ---- (5) x += dx
            for (int i = t; i < n; i += nt) {
                const int ia = ua[i], iv = uv[i];
                if (ia >= 0) th[i] += F[ia] / (double)slab[diag[ia]];
                if (iv >= 0) vm[i] += F[iv] / (double)slab[diag[iv]];
            }
            __syncthreads();
        }
    }

    // ---- the table: slack P, Q and PV Q are the aggregated line sums of the last pass; a failed sample's rows are NaN
    for (int i = t; i < n; i += nt) {
        double4 row = make_double4(nanv, nanv, nanv, nanv);
        if (code == 0) {
            const int ty = a.bus_type[i];
            row.x = vm[i];
            row.y = ty == 0 ? spec[4 * i + 1] : th[i] * (1.0 / PFS_RAD);
            row.z = ty == 0 ? sp[i] : spec[4 * i + 2];
            row.w = dc ? nanv : (ty == 2 ? spec[4 * i + 3] : sq[i]);
        }
        *reinterpret_cast<double4*>(out + 4 * i) = row;
    }
    if (t == 0) {
        a.status[s] = code ? code : it;
        a.residual[s] = res;
    }
}

static int pfs_check_header(const int32_t* h, const char* who) {
    PFN_CHECK_ARG(h, "%s: null plan header", who);
    PFN_CHECK_ARG(h[PFP_H_MAGIC] == PFP_MAGIC && h[PFP_H_VERSION] == PFP_VERSION, "%s: not a sparse power-flow plan (magic %08x, version %d)",
                  who, (unsigned)h[PFP_H_MAGIC], (int)h[PFP_H_VERSION]);
    PFN_CHECK_ARG(h[PFP_H_N] >= 1 && h[PFP_H_E] >= 0 && h[PFP_H_M] >= 0 && h[PFP_H_NNZ] >= h[PFP_H_M] && (h[PFP_H_MODE] == 0 || h[PFP_H_MODE] == 1),
                  "%s: the plan header is inconsistent", who);
    return PFN_OK;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_powerflow_sparse_workspace_bytes(int64_t n_samples, const void* plan_header) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    if (n_samples <= 0 || pfs_check_header(h, "pfn_powerflow_sparse_workspace_bytes") != PFN_OK) return 0;
    return (size_t)n_samples * pfs_sample_bytes(h[PFP_H_N], h[PFP_H_M], h[PFP_H_NNZ]);
}

int pfn_powerflow_solve_sparse(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                               const double* init, int64_t n_samples, int64_t n_bus, int mode, double tol, int max_iter,
                               const void* plan_header, const void* plan_dev, int threads, double* table, int32_t* status,
                               double* residual, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const int32_t* h = static_cast<const int32_t*>(plan_header);
    PFN_TRY(pfs_check_header(h, "pfn_powerflow_solve_sparse"));
    PFN_CHECK_ARG(n_samples >= 0 && n_samples < (1ll << 29), "pfn_powerflow_solve_sparse: bad sample count %lld", (long long)n_samples);
    PFN_CHECK_ARG(mode == 0 || mode == 1, "pfn_powerflow_solve_sparse: mode must be 0 (AC) or 1 (DC); the fast-decoupled modes 2 and 3 are pfn_powerflow_solve_sparse_fd's");
    PFN_CHECK_ARG(h[PFP_H_N] == n_bus && h[PFP_H_E] == n_lines && h[PFP_H_MODE] == mode,
                  "pfn_powerflow_solve_sparse: the plan is for %d buses, %d lines, mode %d; the call has %lld, %lld, mode %d", (int)h[PFP_H_N],
                  (int)h[PFP_H_E], (int)h[PFP_H_MODE], (long long)n_bus, (long long)n_lines, mode);
    PFN_CHECK_ARG(max_iter >= 0 && tol > 0.0, "pfn_powerflow_solve_sparse: max_iter must be >= 0 and tol > 0");
    PFN_CHECK_ARG(threads == 0 || threads == 64 || threads == 256, "pfn_powerflow_solve_sparse: threads must be 0 (the default), 64 or 256");
    if (n_samples == 0) return PFN_OK;
    PFN_CHECK_ARG(rx || n_lines == 0, "pfn_powerflow_solve_sparse: null rx");
    PFN_CHECK_ARG(edge_index || n_lines == 0, "pfn_powerflow_solve_sparse: null edge_index");
    PFN_CHECK_ARG(bus_type && spec && table && status && residual && flags && plan_dev, "pfn_powerflow_solve_sparse: null pointer");
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(table) & 31) == 0 && ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(plan_dev)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(rx) | reinterpret_cast<uintptr_t>(edge_index) |
                        reinterpret_cast<uintptr_t>(residual) | reinterpret_cast<uintptr_t>(init)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(bus_type) | reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(flags)) & 3) == 0,
                  "pfn_powerflow_solve_sparse: table must be 32-byte aligned, the workspace and the plan 16-byte, fp64 and int64 inputs 8-byte, "
                  "int32 arrays 4-byte");
    const int n = h[PFP_H_N], m = h[PFP_H_M], nnz = h[PFP_H_NNZ];
    // (a plan with 32-bit row ids has more than 65535 unknowns: its work vector would not fit LDS either; the kernel reads 16-bit ids only)
    PFN_CHECK_ARG(h[PFP_H_IDX16] != 0, "pfn_powerflow_solve_sparse: %d unknowns: the kernel takes plans with 16-bit row ids (m <= 65535) only", m);
    const size_t lds = pfs_lds_bytes(m);
    PFN_CHECK_ARG(lds <= (size_t)(kLdsCuBytes - kLdsReserve), "pfn_powerflow_solve_sparse: a work vector of %d unknowns needs %zu bytes of LDS, %d are there",
                  m, lds, kLdsCuBytes - kLdsReserve);
    const size_t stride = pfs_sample_bytes(n, m, nnz), need = (size_t)n_samples * stride;
    if (!ws || ws_bytes < need) {
        set_error("pfn_powerflow_solve_sparse: the workspace must hold %zu bytes (got %zu)", need, ws ? ws_bytes : (size_t)0);
        return PFN_ENOSPACE;
    }
    PfsArgs a;
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
    a.m = m;
    a.nnz = nnz;
    a.mode = mode;
    a.max_iter = max_iter;
    a.f_in_lds = pfs_f_in_lds(m);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double madds = (double)(((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]);
    ProfScope ps(mode ? "powerflow_sparse_dc" : "powerflow_sparse_ac",
                 (double)n_samples * ((double)n_lines * 16.0 + (double)n * 64.0 + (init ? (double)n * 16.0 : 0.0)) + (double)h[PFP_H_BYTES],
                 (double)n_samples * 5.0 * 2.0 * (madds + 2.0 * (double)h[PFP_H_NNZ_L]), s);
    // one wave per sample: a k-step costs its load latency, not a barrier, and many samples share a compute unit; four waves once
    // the long columns of the dense tail carry the multiply-adds (DESIGN 7k has the measurements behind the threshold)
    const int use = threads ? threads : (h[PFP_H_MAX_COL] > 128 ? 256 : 64);
    static std::atomic<uint64_t> raised64{0}, raised256{0};
    if (use == 64) {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_sparse_kernel<64>), kLdsCuBytes - kLdsReserve, raised64));
        powerflow_sparse_kernel<64><<<(int)n_samples, 64, lds, s>>>(a);
    } else {
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(powerflow_sparse_kernel<256>), kLdsCuBytes - kLdsReserve, raised256));
        powerflow_sparse_kernel<256><<<(int)n_samples, 256, lds, s>>>(a);
    }
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // extern "C"
