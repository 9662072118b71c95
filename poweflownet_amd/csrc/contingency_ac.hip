// AC N-1 line-outage screening on the device (gfx950): compensated 1P1Q on the dense route.  For every scenario and every single
// line outage, `halves` half-iterations of the fast-decoupled power flow from the scenario's AC base solution, the inverses of B' and
// B'' corrected for the missing line by a rank-1 update instead of being rebuilt.  pfn_contingency_ac: two launches behind
// pfn_contingency_islands (contingency.hip), which decides the islanding outages combinatorially.
//
// BASE launch, one workgroup per scenario: the fast-decoupled solve of the full grid, which IS powerflow.hip's FD instantiation
// (powerflow_dense.hpp pf_solve_sample<true>, the global placement: same text, same bits) -- base table, status, residual.  It leaves
// in the scenario's slab of the workspace: X' = B'^-1 and X'' = B''^-1 (fp32, ld = m | 1), the fp64 base state, the unknown of every
// bus in both matrices, a per-bus list of incident line ends (offsets plus (line, other end), stored order: the stored direction, then
// the reverse) and the scenario's code.  A scenario whose start is converged already has run no half: its inverses are built here.
//
// OUTAGE launch, one workgroup per (scenario, group of consecutive outages), one WAVE per outage k = (i -> j).  The wave owns its
// vectors in LDS -- theta, Vm, the scaled mismatch g, w', w'' (fp64 [n]) and one fp32 phasor per bus -- and steps through
//     w' = X' a', w'' = X'' a''         a = e_i - e_j restricted to the matrix's buses; the fp32 entries widened, fp64 differences
//     for h = 0 .. halves - 1:          the fp64 mismatch F of the grid WITHOUT line k at the current state (pf_ac_end's terms, a bus's
//                                       sum over its incident ends in stored order, lanes own buses), g = F / Vm;
//         even h (or no PQ bus):        theta -= X' g + w' (w' . g) / (1 / c'_k - a'^T w')      over the angle buses
//         odd h:                        Vm    -= X'' g + w'' (w'' . g) / (1 / c''_k - a''^T w'')  over the PQ buses
//                                       (lanes own matrix rows, an fp64 sum in column order; the row walk has stride ld, odd: no bank
//                                       conflict; the dot product is a lane's strided partial sum and a fixed xor butterfly)
//     mismatch = max |F| once more; the fp32 (Vm, Va in degrees) of the final state; phasors by branch_line.hpp bf_phasor_of, the
//     current of every line l != k by bf_line(...).x (lanes own lines), loading I_l / rating_l; severity, worst line and overloads by
//     contingency_monitor.hpp's tail; vm_min, vm_min_bus, v_violations over the PQ buses.
// A bus's mismatch, the line weights and 1 / c_k - a^T w, the per-bus and per-line tails, the stores and the fill values of a skipped
// outage are contingency_ac_core.hpp's, one text with the sparse route (contingency_ac_sparse.hip); this file keeps the half step by
// rows of the inverses, the butterfly and the wave's merges.
// Only wave-level fences stand between the steps; the one workgroup barrier is behind the copy of both inverses into LDS on the LDS
// placement (the global placement reads the slab: same code, same bits).  Every cross-lane reduction is a max, a min, an integer sum
// or that fixed-order dot product: a result's bits are a pure function of the scenario's inputs, whatever the batch, the waves per
// workgroup or the placement.  No float atomics, no host read, no allocation: capturable.
#include <algorithm>

#include "contingency_ac_core.hpp"
#include "powerflow_dense.hpp"

namespace pfn {

constexpr int CA_MAX_WAVES = 16;

__host__ __device__ inline size_t ca_up16(size_t v) { return (v + 15) & ~(size_t)15; }

// a scenario's slab of the workspace (byte offsets; every section 16-byte aligned)
struct CaSlab {
    size_t vm, th, aidx, qidx, adjptr, adj, code, bytes;      // (the two inverses stand at offset 0)
};
__host__ __device__ inline CaSlab ca_slab(int n, int e, int mq) {
    CaSlab l;
    size_t off = ca_up16((pf_mat_floats(n - 1) + pf_mat_floats(mq)) * sizeof(float));
    l.vm = off;       off += ca_up16((size_t)8 * n);
    l.th = off;       off += ca_up16((size_t)8 * n);
    l.aidx = off;     off += ca_up16((size_t)4 * n);
    l.qidx = off;     off += ca_up16((size_t)4 * n);
    l.adjptr = off;   off += ca_up16((size_t)4 * (n + 1));
    l.adj = off;      off += ca_up16((size_t)8 * 2 * e);
    l.code = off;     off += 16;
    l.bytes = off;
    return l;
}
// a wave's vectors in LDS: double th, vm, g, wp, wq [n]; float2 ph [n]
__host__ __device__ inline size_t ca_wave_bytes(int n) { return ca_up16((size_t)48 * n); }
__host__ __device__ inline size_t ca_mat_bytes(int n, int mq) { return (pf_mat_floats(n - 1) + pf_mat_floats(mq)) * sizeof(float); }

struct CaArgs {
    PfArgs pf;                                      // the base solve as powerflow.hip's kernel takes it (pf.p.ws is not used)
    const double* ratings;                          // [e], [S, e] or null (1.0 everywhere)
    const int32_t* islands;                         // [e]
    CaOut out;                                      // (where its nine pointers always stood: the argument layout does not move)
    unsigned char* slabs;
    float v_lo, v_hi;
    int halves, ratings_per_sample;
};

// ------------------------------------------------------------------------------------------------------------ base
__global__ __launch_bounds__(PF_BIG_THREADS) void contingency_ac_base_kernel(const CaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ca_smem[];
    const int t = threadIdx.x, nt = blockDim.x;
    const int s = blockIdx.x;
    const PfProblem& p = a.pf.p;
    const int n = p.n, e = p.e, m = a.pf.m, mp = n - 1, mq = a.pf.n_pq;
    const CaSlab lay = ca_slab(n, e, mq);
    unsigned char* slab = a.slabs + (size_t)s * lay.bytes;
    float* A = reinterpret_cast<float*>(slab);
    int code = pf_solve_sample<true>(a.pf, s, ca_smem, A);
    __syncthreads();                                // (thread 0's status word; the write-back has read the vectors)
    double* vm = reinterpret_cast<double*>(ca_smem);
    double* th = vm + n;
    double* F = th + 3 * (size_t)n;
    int* aidx = reinterpret_cast<int*>(F + m);
    int* vidx = aidx + n;
    const int64_t* ei = p.edge_index;
    if (code == 0 && p.status[s] == 0) {
        // the start was converged: no half-iteration ran, so the inverses are not there yet -- the outages need them.  Should they
        // turn out singular, the base outputs stay the solver's and the scenario's outages are reported as failed.
        const PfSample sm = pf_sample(p, s);
        const PfDense d{ei, sm.rx, sm.spec, sm.spec + 3, 4, n, e, aidx, vidx, vm, th, th + n, th + 2 * (size_t)n, F};
        if (!pf_fd_inverses(d, a.pf.mode == 2, A, mp, mq)) code = PF_SINGULAR;
    }
    if (t == 0) *reinterpret_cast<int*>(slab + lay.code) = code;
    if (code != 0) return;
    double* svm = reinterpret_cast<double*>(slab + lay.vm);
    double* sth = reinterpret_cast<double*>(slab + lay.th);
    int* saidx = reinterpret_cast<int*>(slab + lay.aidx);
    int* sqidx = reinterpret_cast<int*>(slab + lay.qidx);
    int* adjptr = reinterpret_cast<int*>(slab + lay.adjptr);
    int2* adj = reinterpret_cast<int2*>(slab + lay.adj);
    // ---- the state, the unknowns, and the line ends of every bus: counted, offset by one thread, filled in stored order
    for (int i = t; i < n; i += nt) {
        svm[i] = vm[i];
        sth[i] = th[i];
        saidx[i] = aidx[i];
        sqidx[i] = vidx[i] >= 0 ? vidx[i] - mp : -1;
        int cnt = 0;
        for (int k = 0; k < e; ++k) cnt += ((int)ei[k] == i) + ((int)ei[e + k] == i);
        adjptr[i + 1] = cnt;
    }
    __syncthreads();
    if (t == 0) {
        int run = 0;
        adjptr[0] = 0;
        for (int i = 1; i <= n; ++i) {
            run += adjptr[i];
            adjptr[i] = run;
        }
    }
    __syncthreads();
    for (int i = t; i < n; i += nt) {
        int q = adjptr[i];
        for (int k = 0; k < e; ++k) {
            const int la = (int)ei[k], lb = (int)ei[e + k];
            if (la == i) adj[q++] = make_int2(k, lb);
            if (lb == i) adj[q++] = make_int2(k, la);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- outages
// what one wave reads of its scenario and owns in LDS
struct CaWave {
    const double* spec;                             // [n, 4]
    const double* rx;                               // [e, 2]
    const int* aidx;
    const int* qidx;
    const int* adjptr;
    const int2* adj;
    double* th;
    double* vm;
    double* g;
    int n, k, lane;
};

// the fp64 mismatch of the grid without line k at the wave's state: lanes own buses, a bus sums its ends in stored order.  mode 0:
// g = dP / Vm over the angle buses; mode 1: g = dQ / Vm over the PQ buses; mode 2: nothing stored.  Returns the lane's max |F| over
// both kinds of equation (a non-finite entry counts as +inf).
__device__ __forceinline__ double ca_mismatch(const CaWave& v, const int mode) {
    double mx = 0.0;
    for (int i = v.lane; i < v.n; i += 64) {
        const int ra = v.aidx[i], rq = v.qidx[i];
        if (ra < 0) continue;                       // the slack: no equation
        mx = ca_bus_mismatch<1, 0>(mx, v.th, v.vm, v.g, v.adj, v.adjptr[i], v.adjptr[i + 1], v.rx, v.spec, i, ra, rq, v.k, mode);
    }
    return mx;
}

template <bool LDS>
__global__ __launch_bounds__(CA_MAX_WAVES * 64) void contingency_ac_outage_kernel(const CaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ca_smem[];
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const PfProblem& p = a.pf.p;
    const int n = p.n, e = p.e, mp = n - 1, mq = a.pf.n_pq, ldp = pf_ld(mp), ldq = pf_ld(mq);
    const int groups = (e + nw - 1) / nw;
    const int s = blockIdx.x / groups;
    const int k = (blockIdx.x - s * groups) * nw + wave;
    const CaSlab lay = ca_slab(n, e, mq);
    const unsigned char* slab = a.slabs + (size_t)s * lay.bytes;
    const int code = *reinterpret_cast<const int*>(slab + lay.code);
    const float* Xp = reinterpret_cast<const float*>(slab);
    const float* Xq = Xp + pf_mat_floats(mp);
    unsigned char* vecs = ca_smem;
    if constexpr (LDS) {
        float* lds = reinterpret_cast<float*>(ca_smem);
        const int total = (int)(pf_mat_floats(mp) + pf_mat_floats(mq));
        if (code == 0)
            for (int q = t; q < total; q += nt) lds[q] = Xp[q];
        __syncthreads();                            // (the one workgroup barrier: every wave is still here)
        Xp = lds;
        Xq = lds + pf_mat_floats(mp);
        vecs += ca_mat_bytes(n, mq);
    }
    if (k >= e) return;

    const int64_t o = (int64_t)s * e + k;
    float* crow = a.out.post_current ? a.out.post_current + o * e : nullptr;
    float* srow = a.out.post_state ? a.out.post_state + o * 2 * n : nullptr;
    if (code != 0 || a.islands[k] != 0) {           // a failed scenario, an islanding outage
        ca_skip(code != 0, a.out, o, crow, srow, e, n, lane, 64);
        return;
    }

    const PfSample sm = pf_sample(p, s);
    const int64_t* ei = p.edge_index;
    double* th = reinterpret_cast<double*>(vecs + (size_t)wave * ca_wave_bytes(n));
    double* vm = th + n;
    double* g = vm + n;
    double* wp = g + n;
    double* wq = wp + n;
    float2* ph = reinterpret_cast<float2*>(wq + n);
    const double* svm = reinterpret_cast<const double*>(slab + lay.vm);
    const double* sth = reinterpret_cast<const double*>(slab + lay.th);
    const int* aidx = reinterpret_cast<const int*>(slab + lay.aidx);
    const int* qidx = reinterpret_cast<const int*>(slab + lay.qidx);
    const CaWave v{sm.spec, sm.rx, aidx, qidx, reinterpret_cast<const int*>(slab + lay.adjptr), reinterpret_cast<const int2*>(slab + lay.adj),
                   th, vm, g, n, k, lane};

    // ---- the start is the base state; w' = X' a', w'' = X'' a'' (zero at the buses outside the matrix)
    const int bi = (int)ei[k], bj = (int)ei[e + k];
    const int pi = aidx[bi], pj = aidx[bj], qi = qidx[bi], qj = qidx[bj];
    for (int b = lane; b < n; b += 64) {
        th[b] = sth[b];
        vm[b] = svm[b];
        const int rp = aidx[b], rq = qidx[b];
        double up = 0.0, uq = 0.0;
        if (rp >= 0) up = (pi >= 0 ? (double)Xp[rp * ldp + pi] : 0.0) - (pj >= 0 ? (double)Xp[rp * ldp + pj] : 0.0);
        if (rq >= 0) uq = (qi >= 0 ? (double)Xq[rq * ldq + qi] : 0.0) - (qj >= 0 ? (double)Xq[rq * ldq + qj] : 0.0);
        wp[b] = up;
        wq[b] = uq;
    }
    __syncwarp();
    // ---- 1 / c_k - a^T w of both matrices (c: the line's weight in the matrix)
    const double2 ck = ca_weights(sm.rx[2 * k], sm.rx[2 * k + 1]);
    const bool bx = a.pf.mode != 2;
    const double denp = ca_den(ck, bx, false, wp[bi] - wp[bj]);
    const double denq = ca_den(ck, bx, true, wq[bi] - wq[bj]);

    for (int h = 0; h < a.halves; ++h) {
        const bool qhalf = mq != 0 && (h & 1);
        ca_mismatch(v, qhalf ? 1 : 0);
        __syncwarp();
        const int* idx = qhalf ? qidx : aidx;
        const double* w = qhalf ? wq : wp;
        const float* X = qhalf ? Xq : Xp;
        const int cols = qhalf ? mq : mp, ld = qhalf ? ldq : ldp;
        double* x = qhalf ? vm : th;
        // ---- w . g: a lane's buses in ascending order, then the butterfly (a + b = b + a: every lane ends with the same bits)
        double dot = 0.0;
        for (int b = lane; b < n; b += 64) {
            const int r = idx[b];
            if (r >= 0) dot += w[b] * g[r];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
        const double scale = dot / (qhalf ? denq : denp);
        // ---- x -= X g + w (w . g) / den: a row by its owner, fp64 sum in column order
        for (int b = lane; b < n; b += 64) {
            const int r = idx[b];
            if (r < 0) continue;
            const float* row = X + r * ld;
            double acc = 0.0;
            for (int c = 0; c < cols; ++c) acc += (double)row[c] * g[c];
            x[b] -= acc + w[b] * scale;
        }
        __syncwarp();
    }

    // ---- how far from converged the estimate is
    double mx = ca_mismatch(v, 2);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));

    // ---- the fp32 state, the phasors and the voltage figures over the PQ buses
    CaLow low = ca_low_none();
    for (int b = lane; b < n; b += 64) ca_bus_tail<1>(low, th, vm, ph, srow, sm.spec, b, aidx[b] < 0, qidx[b] >= 0, a.v_lo, a.v_hi);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        ca_low_merge(low, CaLow{__shfl_xor(low.best, off), __shfl_xor(low.arg, off), __shfl_xor(low.cnt, off), __shfl_xor(low.wild, off)});
    __syncwarp();

    // ---- the currents of the lines l != k, their loadings, the wave's worst (contingency_monitor.hpp)
    const double* rat = a.ratings ? a.ratings + (a.ratings_per_sample ? (int64_t)s * e : 0) : nullptr;
    CtWorst worst = ct_worst_none();
    for (int l = lane; l < e; l += 64) ca_line_tail<1>(worst, ph, ei, sm.rx, rat, crow, e, l, k);
    worst = ct_worst_wave(worst);
    if (lane == 0) ca_store(a.out, o, worst, low, mx);
}

// the waves per workgroup and the placement of a call: 0 where it is refused.  route 0: both inverses in LDS beside 16, 8 or 4
// waves' vectors, the first that fits -- else the slab, with as many waves as there is LDS for (16 at most); route 1: LDS, down to
// one wave; route 2: the slab.  group > 0 names the waves.
static int ca_plan(int n, int n_pq, int route, int group, bool* lds) {
    const size_t budget = (size_t)(kLdsCuBytes - kLdsReserve), vec = ca_wave_bytes(n), mats = ca_mat_bytes(n, n_pq);
    const int maxw = (int)std::min<size_t>(CA_MAX_WAVES, budget / vec);
    *lds = false;
    if (maxw < 1 || group > maxw) return 0;
    if (group > 0) {
        const bool fits = mats + (size_t)group * vec <= budget;
        if (route == 1 && !fits) return 0;
        *lds = route != 2 && fits;
        return group;
    }
    if (route != 2) {
        for (int w = CA_MAX_WAVES; w >= (route == 1 ? 1 : 4); w >>= 1)
            if (w <= maxw && mats + (size_t)w * vec <= budget) {
                *lds = true;
                return w;
            }
        if (route == 1) return 0;
    }
    return maxw;
}

static bool ca_sizes_ok(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq) {
    return n_samples >= 0 && n_samples < (1ll << 29) && n_bus >= 2 && n_bus - 1 <= PF_MAX_UNKNOWNS && n_lines >= 0 && n_lines < (1ll << 24) &&
           n_pq >= 0 && n_pq < n_bus;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_contingency_ac_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_pq) {
    if (!ca_sizes_ok(n_samples, n_bus, n_lines, n_pq) || n_samples == 0) return 0;
    return (size_t)n_samples * ca_slab((int)n_bus, (int)n_lines, (int)n_pq).bytes;
}

int pfn_contingency_ac_waves(int64_t n_bus, int64_t n_pq, int route, int group, int* in_lds) {
    if (!ca_sizes_ok(1, n_bus, 0, n_pq) || route < 0 || route > 2 || group < 0 || group > CA_MAX_WAVES) return 0;
    bool lds = false;
    const int w = ca_plan((int)n_bus, (int)n_pq, route, group, &lds);
    if (in_lds) *in_lds = lds;
    return w;
}

int pfn_contingency_ac(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                       const double* init, const double* ratings, int ratings_per_sample, const int32_t* islands, int64_t n_samples,
                       int64_t n_bus, int64_t n_pv, int64_t n_pq, int variant, int halves, float v_lo, float v_hi, double tol, int max_iter,
                       int route, int group, float* severity, int32_t* worst_line, int32_t* overloads, float* vm_min, int32_t* vm_min_bus,
                       int32_t* v_violations, double* mismatch, double* base_table, int32_t* status, double* residual, float* post_current,
                       float* post_state, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "pfn_contingency_ac";
    PFN_CHECK_ARG(n_samples >= 0 && n_bus >= 2 && n_lines >= 0 && n_samples < (1ll << 29) && n_lines < (1ll << 24) && n_bus < (1ll << 24),
                  "%s: bad sizes (%lld scenarios of %lld buses and %lld lines)", who, (long long)n_samples, (long long)n_bus, (long long)n_lines);
    PFN_TRY(ca_check_options(who, n_bus, n_pv, n_pq, variant, halves, v_lo, v_hi, tol, max_iter));
    PFN_CHECK_ARG(route >= 0 && route <= 2, "%s: route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(group >= 0 && group <= CA_MAX_WAVES, "%s: group must be 0 (auto) or the waves per workgroup, 1 .. %d", who, CA_MAX_WAVES);
    PFN_CHECK_ARG(n_bus - 1 <= PF_MAX_UNKNOWNS, "%s: %lld unknowns per scenario exceed the dense screen's %d; beyond it: pfn_contingency_ac_sparse", who,
                  (long long)(n_bus - 1), PF_MAX_UNKNOWNS);
    const int n = (int)n_bus, e = (int)n_lines, mq = (int)n_pq, m = (n - 1) + mq;
    bool lds = false;
    const int waves = ca_plan(n, mq, route, group, &lds);
    PFN_CHECK_ARG(waves > 0, "%s: route %d with %d waves per workgroup: both inverses of %d buses (%zu bytes) and %zu bytes per wave need more than the %d bytes of LDS",
                  who, route, group, n, ca_mat_bytes(n, mq), ca_wave_bytes(n), kLdsCuBytes - kLdsReserve);
    if (n_samples == 0 || n_lines == 0) return PFN_OK;
    const CaOut out{severity, worst_line, overloads, vm_min, vm_min_bus, v_violations, mismatch, post_current, post_state};
    PFN_TRY(ca_check_pointers(who, edge_index, rx, bus_type, spec, init, ratings, islands, out, base_table, status, residual, flags, ws, false, nullptr));
    const CaSlab lay = ca_slab(n, e, mq);
    PFN_TRY(pf_check_workspace(who, ws, ws_bytes, (size_t)n_samples * lay.bytes));
    const size_t base_lds = pf_vec_bytes(n, m) + pf_fd_extra_bytes(m);
    CaArgs a{{{edge_index, rx, bus_type, spec, init, base_table, status, residual, flags, nullptr, tol, n, e, max_iter}, m, (int)n_pv, mq, 2 + variant, 0},
             ratings, islands, out, static_cast<unsigned char*>(ws), v_lo, v_hi, halves, ratings_per_sample != 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double mm = (double)(n - 1), qq = (double)mq, ee = (double)e, hh = (double)halves;
    {
        const int threads = std::max(n - 1, mq) > PF_BIG_M ? PF_BIG_THREADS : PF_SMALL_THREADS;       // the solver's rule
        ProfScope ps("contingency_ac_base", (double)n_samples * (ee * 16.0 + (double)n * 64.0 + (double)lay.bytes),
                     (double)n_samples * (2.0 * (mm * mm * mm + qq * qq * qq) + 20.0 * (mm * mm + qq * qq)), s);
        static std::atomic<uint64_t> raised{0};
        PFN_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(contingency_ac_base_kernel), kLdsCuBytes - kLdsReserve, raised));
        contingency_ac_base_kernel<<<(int)n_samples, threads, base_lds, s>>>(a);
        PFN_CHECK_LAUNCH();
    }
    const int64_t grid = n_samples * ((e + waves - 1) / waves);
    PFN_CHECK_ARG(grid < (1ll << 31), "%s: %lld workgroups exceed the launch grid", who, (long long)grid);
    ProfScope ps("contingency_ac_outages", (double)n_samples * ee * (28.0 + (post_current ? 4.0 * ee : 0.0) + (post_state ? 8.0 * (double)n : 0.0)),
                 (double)n_samples * ee * (hh * (mm * mm + qq * qq + 60.0 * ee) + 60.0 * ee), s);
    const size_t vec = (size_t)waves * ca_wave_bytes(n);
    return launch_either<contingency_ac_outage_kernel<true>, contingency_ac_outage_kernel<false>>(lds, (int)grid, waves * 64, vec + ca_mat_bytes(n, mq), vec, s, a);
}

}  // extern "C"
