// What every power-flow kernel (powerflow.hip, powerflow_sparse.hip, powerflow_sparse_fd.hip) does to its sample, spelled once:
// the status codes and constants, the problem as the launch passes it, the start state, the AC and DC line-end terms with the
// Jacobian derivatives of an end, the max |F| and the stopping rule, the table write-back, the view of a sparse (sub-)plan with its
// check against the device arrays, and -- host side -- the sizes of the sparse routes' sample, the argument checks every entry
// makes, those the sparse entries make (plan header, launch arguments, workspace) and the launch of a sparse kernel.  The kernels
// keep what differs between them: their matrix and how it is solved (the dense one: powerflow_dense.hpp; what the Q-limit kernels
// add: powerflow_qlim.hpp).
//
// Every device function here is called by ALL threads of the workgroup with the same arguments (`nt` is the workgroup size: a
// compile-time constant on the sparse routes, blockDim.x on the dense one).  The expressions of the line-end terms keep the shape
// the fp64 results were validated in: hipcc contracts a product into the sum that uses it wherever the two end up in one basic block,
// so regrouping a term or moving a statement into or out of one of these functions may move the last bit of a line sum or a
// Jacobian entry (compare the fp64 instructions of the kernels and their results with the parent's after any such change).
#pragma once
#include "pfn_internal.hpp"
#include "powerflow_plan.hpp"

namespace pfn {

// status[s] < 0; >= 0 it is the count of solves.  (utils/powerflow.py STATUS has the texts; topology.hip's TP_BAD_LINE is PF_BAD_LINE)
enum { PF_NOT_CONVERGED = -1, PF_SINGULAR = -2, PF_NON_FINITE = -3, PF_BAD_LINE = -4, PF_BAD_TYPES = -5, PF_STALE_PLAN = -6,
       PF_QLIM_ROUNDS = -7 };                      // (powerflow_qlim.hip only: limits still violated after max_rounds re-solves)
constexpr double PF_RAD = 3.14159265358979323846 / 180.0;
constexpr float PF_TINY_PIVOT = 1e-30f;            // |pivot| <= this (or NaN): singular
constexpr int PF_F_LDS_BYTES = 80 * 1024;          // sparse routes: w + the right-hand side in LDS up to here (two workgroups per compute unit at least)

// the problem as every route's launch passes it; a kernel's argument struct embeds it as `p`
struct PfProblem {
    const int64_t* edge_index;
    const double* rx;
    const int32_t* bus_type;
    const double* spec;
    const double* init;                             // [S, n, 2] = (Vm, Va in degrees) or null: the flat start
    double* table;
    int32_t* status;
    double* residual;
    int32_t* flags;
    void* ws;                                       // dense: the global route's fp32 slabs or null; sparse: the samples' vectors and slabs
    double tol;
    int n, e, max_iter;
    // the cover route (powerflow_cover.hip) only, null elsewhere: which lines of the shared list sample s has, and whether one of
    // its own lines found no place in that list
    const uint8_t* line_mask;                       // [S, e] or null: every line is there
    const int32_t* unplaced;                        // [S] or null
};

// sample s's rows of the per-sample arrays
struct PfSample {
    const double* init;
    const double* rx;
    const double* spec;
    double* out;
};

__device__ __forceinline__ PfSample pf_sample(const PfProblem& p, int s) {
    return {p.init ? p.init + (int64_t)s * 2 * p.n : nullptr, p.rx + (int64_t)s * 2 * p.e, p.spec + (int64_t)s * 4 * p.n,
            p.table + (int64_t)s * 4 * p.n};
}

// sample s's row of the line mask, or null (uniform); and what it holds against the plan before anything is indexed (uniform)
__device__ __forceinline__ const uint8_t* pf_line_mask(const PfProblem& p, int s) {
    return p.line_mask ? p.line_mask + (int64_t)s * p.e : nullptr;
}
__device__ __forceinline__ int pf_unplaced(const PfProblem& p, int s) { return p.unplaced ? p.unplaced[s] != 0 : 0; }

// ---- the start state: flat, or the caller's -- Va at the non-slack buses, Vm at the PQ buses (dc: Va only, its Vm is no unknown).
// True, for all threads alike, when the caller's start holds a non-finite value.  `types` is the row that decides: p.bus_type, or
// the Q-limit kernels' live copy of the sample's own row in LDS (int or byte; they pass dc = false).
template <typename Ty>
__device__ __forceinline__ bool pf_start_state(const PfProblem& p, const PfSample& sm, const Ty* types, int slack, bool dc, int nt, double* vm,
                                               double* th) {
    const double th0 = sm.spec[4 * slack + 1] * PF_RAD;
    int wild = 0;
    for (int i = threadIdx.x; i < p.n; i += nt) {
        const int ty = types[i];
        double v = ty == 2 ? 1.0 : sm.spec[4 * i], ang = th0;
        if (sm.init) {
            if (ty == 2 && !dc) v = sm.init[2 * i];
            if (ty != 0) ang = sm.init[2 * i + 1] * PF_RAD;
            wild |= !(fabs(v) < __builtin_inf()) || !(fabs(ang) < __builtin_inf());
        }
        vm[i] = v;
        th[i] = ang;
    }
    return __syncthreads_or(wild);
}

// ---- one line end seen from bus i (the other end is j): its term is added to bus i's sums, one fp64 sincos per end
struct PfEnd {
    double g, b, vj, vv, sn, cs;
};

__device__ __forceinline__ PfEnd pf_ac_end(double r, double x, double vi, double ti, double vj, double tj, double& sP, double& sQ) {
    const double d = r * r + x * x, g = r / d, b = -x / d;
    const double vv = vi * vj;
    double sn, cs;
    sincos(ti - tj, &sn, &cs);
    const double t1 = vv * cs - vi * vi, t2 = vv * sn;
    sP += g * t1 + b * t2;
    sQ += g * t2 - b * t1;
    return {g, b, vj, vv, sn, cs};
}

// the derivatives of that term: by bus i's own theta and Vm (the diagonal block sums them in fp64) and by Vm_j; by theta_j they
// are -pti and -qti.  The caller scatters them where its matrix keeps them.
struct PfEndJac {
    double pti, pvi, qti, qvi, pvj, qvj;
};

__device__ __forceinline__ PfEndJac pf_ac_end_jac(const PfEnd& t, double vi) {
    const double g = t.g, b = t.b, vj = t.vj, vv = t.vv, sn = t.sn, cs = t.cs;
    PfEndJac J;
    J.pti = vv * (b * cs - g * sn);
    J.qti = vv * (g * cs + b * sn);
    J.pvi = g * (vj * cs - 2.0 * vi) + b * vj * sn;
    J.qvi = g * vj * sn - b * (vj * cs - 2.0 * vi);
    J.pvj = vi * (g * cs + b * sn);
    J.qvj = vi * (g * sn - b * cs);
    return J;
}

// the DC end: b (theta_i - theta_j) with b = -1 / x; returns b, which the caller adds to its diagonal sum and whose negative is the
// (theta_i, theta_j) entry.  (`dPt += b` stays with the caller: with it in here the dense kernel contracts the line sum differently.)
__device__ __forceinline__ double pf_dc_end(double x, double ti, double tj, double& sP) {
    const double b = -1.0 / x;
    sP += b * (ti - tj);
    return b;
}

// ---- max |F| in fp64: a non-finite entry counts as +inf
__device__ __forceinline__ double pf_abs_clamped(double f) {
    const double af = fabs(f);
    return af < __builtin_inf() ? af : __builtin_inf();
}

// max over the workgroup's nw waves (max is exact: the order does not matter); red: nw doubles of LDS
__device__ __forceinline__ double pf_block_max(double v, double* red, int nw) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int w = 1; w < nw; ++w) r = fmax(r, red[w]);
    __syncthreads();
    return r;
}

// ---- the stopping rule on res = max |F| after `it` solves: 0 go on, PF_CONVERGED, or the failure code.  The callers leave their
// loop on two edges -- `if (stop < 0) { code = stop; break; }  if (stop) break;` --: one merged exit costs the sparse Newton kernel
// two VGPRs.
constexpr int PF_CONVERGED = 1;
__device__ __forceinline__ int pf_stop(double res, double tol, int it, int max_iter) {
    if (!(res < __builtin_inf())) return PF_NON_FINITE;
    if (res < tol) return PF_CONVERGED;
    if (it >= max_iter) return PF_NOT_CONVERGED;
    return 0;
}

// ---- the table and the sample's status / residual: slack P, Q and PV Q are the aggregated line sums of the last pass (dc: Q is
// NaN); a failed sample's rows are NaN
__device__ __forceinline__ void pf_write_back(const PfProblem& p, const PfSample& sm, int s, bool dc, int nt, int code, int it, double res,
                                              const double* vm, const double* th, const double* sp, const double* sq) {
    const double nanv = __builtin_nan("");
    for (int i = threadIdx.x; i < p.n; i += nt) {
        double4 row = make_double4(nanv, nanv, nanv, nanv);
        if (code == 0) {
            const int ty = p.bus_type[i];
            row.x = vm[i];
            row.y = ty == 0 ? sm.spec[4 * i + 1] : th[i] * (1.0 / PF_RAD);
            row.z = ty == 0 ? sp[i] : sm.spec[4 * i + 2];
            row.w = dc ? nanv : (ty == 2 ? sm.spec[4 * i + 3] : sq[i]);
        }
        *reinterpret_cast<double4*>(sm.out + 4 * i) = row;
    }
    if (threadIdx.x == 0) {
        p.status[s] = code ? code : it;
        p.residual[s] = res;
    }
}

// ---- one planned matrix: the sections of a (sub-)plan the numeric loops of powerflow_sparse_core.hpp read, and its order
struct PfcMatrix {
    const int32_t* colptr;
    const int32_t* diag;
    const uint16_t* row;                            // (the launchers refuse plans with 32-bit ids)
    int m;
};

// the sections of one (sub-)plan, from its start
struct PfPlanView {
    const int32_t* ua;
    const int32_t* uv;
    const int32_t* adjptr;
    const int2* adj;
    const int4* adjpos;
    const int4* buspos;
    PfcMatrix A;
    int nnz;
};

__device__ __forceinline__ PfPlanView pf_plan_view(const unsigned char* pb) {
    const int32_t* H = reinterpret_cast<const int32_t*>(pb);
    PfPlanView v;
    v.ua = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_UA]);
    v.uv = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_UV]);
    v.adjptr = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_ADJPTR]);
    v.adj = reinterpret_cast<const int2*>(pb + H[PFP_H_OFF_ADJ]);
    v.adjpos = reinterpret_cast<const int4*>(pb + H[PFP_H_OFF_ADJPOS]);
    v.buspos = reinterpret_cast<const int4*>(pb + H[PFP_H_OFF_BUSPOS]);
    v.A.colptr = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_COLPTR]);
    v.A.diag = reinterpret_cast<const int32_t*>(pb + H[PFP_H_OFF_DIAG]);
    v.A.row = reinterpret_cast<const uint16_t*>(pb + H[PFP_H_OFF_ROWIDX]);
    v.A.m = H[PFP_H_M];
    v.nnz = H[PFP_H_NNZ];
    return v;
}

// ---- the device arrays against the plan: the bus types decide the unknowns, the line list the line ends.  `stale` (uniform) is
// what the caller already holds against the plan: nothing is indexed then.  contradicts(i, ty, stale) says whether bus i's type
// disagrees with the kernel's unknowns and may raise `stale` itself.  A line number outside the list is stale, never followed.
// Returns 0, PF_BAD_TYPES (flags bit 0 is set with it) or PF_STALE_PLAN, for all threads alike.  A sample that comes in stale -- the
// fast-decoupled plan's size test, an unplaced line of the cover route -- skips the bus-type scan with everything else: it reports
// PF_STALE_PLAN, and flags bit 0 is set only by the samples that do scan (a batch of nothing but such samples leaves it clear).
template <typename Contradicts>
__device__ __forceinline__ int pf_check_plan(const PfProblem& p, const PfPlanView& v, int nt, int stale, Contradicts contradicts) {
    const int e = p.e;
    int odd = 0;
    if (!stale) {
        for (int i = threadIdx.x; i < p.n; i += nt) {
            const int ty = p.bus_type[i];
            odd |= (unsigned)ty > 2u || contradicts(i, ty, stale);
            for (int q = v.adjptr[i]; q < v.adjptr[i + 1]; ++q) {
                const int2 lj = v.adj[q];
                const int k = lj.x >> 1, side = lj.x & 1;
                if ((unsigned)k >= (unsigned)e) { stale = 1; continue; }
                stale |= p.edge_index[side ? e + k : k] != (int64_t)i || p.edge_index[side ? k : e + k] != (int64_t)lj.y;
            }
        }
    }
    odd = __syncthreads_or(odd);
    stale = __syncthreads_or(stale);
    if (odd) {
        if (threadIdx.x == 0) p.flags[0] = p.flags[0] | 1;      // (every writer stores the same bit over the same word)
        return PF_BAD_TYPES;
    }
    return stale ? PF_STALE_PLAN : 0;
}

// ---- host side.  A sparse route's sample in the workspace: double vm, th, sp, sq [n], F [rhs]; then its fp32 slab(s) [nnz]; rounded
// to 16 bytes.  rhs is the length of the right-hand side: m, or the larger of the fast-decoupled halves.
__host__ __device__ inline size_t pf_sample_bytes(int n, int rhs, int nnz) {
    return (((size_t)8 * (4 * (size_t)n + rhs) + (size_t)4 * nnz) + 15) & ~(size_t)15;
}
__host__ __device__ inline bool pf_f_in_lds(int rhs) { return (size_t)12 * rhs <= (size_t)PF_F_LDS_BYTES; }
__host__ __device__ inline size_t pf_w_bytes(int rhs) { return ((size_t)4 * rhs + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pf_lds_bytes(int rhs) { return pf_w_bytes(rhs) + (pf_f_in_lds(rhs) ? (size_t)8 * rhs : 0) + 16; }

// what every solve entry asks of its arguments.  plan_dev: where the route's device plan pointer stands, null on the dense route;
// sixteen: the words of the alignment message about the 16-byte pointers.  The pointers are looked at only when there are samples.
static inline int pf_check_call(const char* who, const PfProblem& p, int64_t n_samples, const void* const* plan_dev, const char* sixteen) {
    PFN_CHECK_ARG(n_samples >= 0 && n_samples < (1ll << 29), "%s: bad sample count %lld", who, (long long)n_samples);
    PFN_CHECK_ARG(p.max_iter >= 0 && p.tol > 0.0, "%s: max_iter must be >= 0 and tol > 0", who);
    if (n_samples == 0) return PFN_OK;
    const void* plan = plan_dev ? *plan_dev : nullptr;
    PFN_CHECK_ARG(p.rx || p.e == 0, "%s: null rx", who);
    PFN_CHECK_ARG(p.edge_index || p.e == 0, "%s: null edge_index", who);
    PFN_CHECK_ARG(p.bus_type && p.spec && p.table && p.status && p.residual && p.flags && (plan || !plan_dev), "%s: null pointer", who);
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(p.table) & 31) == 0 && ((reinterpret_cast<uintptr_t>(p.ws) | reinterpret_cast<uintptr_t>(plan)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(p.spec) | reinterpret_cast<uintptr_t>(p.rx) | reinterpret_cast<uintptr_t>(p.edge_index) |
                        reinterpret_cast<uintptr_t>(p.residual) | reinterpret_cast<uintptr_t>(p.init)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(p.bus_type) | reinterpret_cast<uintptr_t>(p.status) | reinterpret_cast<uintptr_t>(p.flags)) & 3) == 0,
                  "%s: table must be 32-byte aligned, %s, fp64 and int64 inputs 8-byte, int32 arrays 4-byte", who, sixteen);
    return PFN_OK;
}

// what the sparse entries ask of their plan header before they read sizes from it (the entry adds its own mode and size conditions)
// and of their launch arguments; the row ids are looked at only when there are samples
static inline int pf_check_plan_header(const char* who, const int32_t* h) {
    PFN_CHECK_ARG(h, "%s: null plan header", who);
    PFN_CHECK_ARG(h[PFP_H_MAGIC] == PFP_MAGIC && h[PFP_H_VERSION] == PFP_VERSION, "%s: not a sparse power-flow plan (magic %08x, version %d)",
                  who, (unsigned)h[PFP_H_MAGIC], (int)h[PFP_H_VERSION]);
    PFN_CHECK_ARG(h[PFP_H_N] >= 1 && h[PFP_H_E] >= 0 && h[PFP_H_M] >= 0 && h[PFP_H_NNZ] >= h[PFP_H_M], "%s: the plan header is inconsistent", who);
    return PFN_OK;
}

static inline int pf_check_sparse_launch(const char* who, int threads, const int32_t* unplaced, int64_t n_samples, const int32_t* h, int m) {
    PFN_CHECK_ARG(threads == 0 || threads == 64 || threads == 256, "%s: threads must be 0 (the default), 64 or 256", who);
    PFN_CHECK_ARG((reinterpret_cast<uintptr_t>(unplaced) & 3) == 0, "%s: unplaced must be 4-byte aligned", who);
    // (a plan with 32-bit row ids has more than 65535 unknowns: its work vector would not fit LDS either; the kernels read 16-bit ids only)
    PFN_CHECK_ARG(n_samples <= 0 || h[PFP_H_IDX16] != 0, "%s: %d unknowns: the kernel takes plans with 16-bit row ids (m <= 65535) only", who, m);
    return PFN_OK;
}

static inline int pf_check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need) {
        set_error("%s: the workspace must hold %zu bytes (got %zu)", who, need, ws ? ws_bytes : (size_t)0);
        return PFN_ENOSPACE;
    }
    return PFN_OK;
}

// the launch of a sparse route's kernel, one workgroup per sample: one wave until the longest column of the plan exceeds 128 -- a
// k-step then costs its load latency, not a barrier, and many samples share a compute unit --, four waves once the long columns
// of the dense tail carry the multiply-adds (DESIGN 7k and 7l have the measurements behind the threshold); `threads` overrides.
// Pair tells kernel pairs with one argument struct apart: each needs its own dynamic-LDS attribute raised.
template <int Pair = 0, typename Args>
static int pf_launch_sparse(void (*k64)(Args), void (*k256)(Args), int threads, int max_col, int64_t n_samples, size_t lds, hipStream_t s,
                            const Args& a) {
    static std::atomic<uint64_t> raised64{0}, raised256{0};      // (per Pair and Args: per kernel pair)
    const int use = threads ? threads : (max_col > 128 ? 256 : 64);
    PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(use == 64 ? k64 : k256), kLdsCuBytes - kLdsReserve, use == 64 ? raised64 : raised256));
    (use == 64 ? k64 : k256)<<<(int)n_samples, use, lds, s>>>(a);
    PFN_CHECK_LAUNCH();
    return PFN_OK;
}

}  // namespace pfn
