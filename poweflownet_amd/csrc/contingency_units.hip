// Generator-outage screening on the device (gfx950), the dense DC route: which unit outages -- alone, and followed by a line outage --
// overload the grid?  One launch, pfn_contingency_units, one workgroup per scenario, behind pfn_contingency_islands where lines are
// asked for.
//
// A unit outage in the DC model changes the right-hand side only.  With X = B'^-1 (zeros at the slack), c_g = X[:, b_g] the column of
// the unit's bus, a_h >= 0 the participation factors, A = sum_h a_h and rest_g = A - a_g (fp64), the outage of unit g takes p_g off
// bus b_g and hands p_g a_h / rest_g to every other unit h (rest_g > 0; else the slack absorbs it).  With u = sum_h a_h c_h:
//     d_g = alpha_g u - beta_g c_g      alpha_g = p_g / rest_g,  beta_g = p_g (a_g / rest_g + 1)     (rest_g > 0)
//     d_g = -p_g c_g                    alpha_g = 0,             beta_g = p_g                        (otherwise)
//     f_l^(g) = f_l + (d_g[a] - d_g[b]) / x_l   for the stored line l = (a -> b); all e lines stay monitored.
// Unit x line (g, k): line k goes out of the post-unit state, by contingency.hip's distribution factors on f^(g):
//     f_l^(g,k) = f_l^(g) + phi_{l,k} / den_k * f_k^(g)   (l != k),   0 at k.
//   PHASE A, the whole workgroup: contingency_base.hpp ct_base_solve, the N-1 screen's: base_flow and status are its bits.
//   PHASE A2, the whole workgroup: the units, their outputs and factors are staged in LDS and checked (a unit id outside [0, n) is
//   never followed: -4; a non-finite p, a factor that is not finite and >= 0: -3; an LDS flag word), a barrier; then thread 0 sums A in fp64 in stored
//   order while the row owners form u [n] in fp32 (bus b by thread b, b + nt, ...: the units in stored order, a row walk of X, ld odd,
//   so the threads' rows fall into different banks), a barrier.
//   PHASE B, no workgroup barrier: wave w takes the units w, w + nw, ...  Its lanes form alpha and beta in fp64, round each once, walk
//   the column c_g into the wave's own fp32 vector [n] (ct_column) and turn it into d_g in place, each lane its own entries; then the
//   lanes stride over the lines: post-outage flow, loading, the one tail of all screens (contingency_monitor.hpp).
//   PHASE C, with candidate lines only, unit g outer at workgroup level: all threads form d_g [n] and then f^(g) [e] in LDS (the same
//   two expressions as PHASE B: the same bits), a barrier each; then wave w takes the candidates w, w + nw, ...: w_k, den_k and the
//   post-outage flows by contingency_line.hpp over f^(g).  (The k-outer order would form every w_k once but needs all G vectors d_g
//   resident: 4 n G bytes, which at case118 would leave one workgroup per compute unit where two fit; the column walk is the cheap part of an item.)
// Every per-line and per-bus expression is compiled without contraction, every cross-thread reduction is a max or an integer sum, one
// owner per output: a scenario's bits are a pure function of its own inputs, whatever the batch, the workgroup size, the placement of
// X, the table or the candidate lines; the unit figures are the same bits with and without PHASE C.  No host sync, no allocation
// (capturable), no float atomics.
#include "contingency_base.hpp"
#include "contingency_line.hpp"
#include "contingency_monitor.hpp"

namespace pfn {

// the kernel's argument block: CtCommon's names (ct_base_in and ct_check_aligned take it by them) and the unit screen's own
struct CuArgs {
    const int64_t* edge_index;                      // [2, e]
    const double* rx;                               // [S, e, 2]
    const int32_t* bus_type;                        // [n]
    const double* spec;                             // [S, n, 4]
    const double* ratings;                          // [e], [S, e] or null
    const int32_t* islands;                         // [e], the islands launch's output, or null without candidate lines
    float* severity;                                // [S, G]
    int32_t* worst_line;                            // [S, G]
    int32_t* overloads;                             // [S, G]
    double* base_flow;                              // [S, e]
    int32_t* status;                                // [S]
    float* post_flow;                               // [S, G, e] or null
    int32_t* flags;
    void* ws;                                       // the global route's fp32 slabs or null
    double tol;
    int n, e, max_iter, n_pv, n_pq, ratings_per_sample;
    const int32_t* units;                           // [G]
    const double* unit_p;                           // [G] or [S, G]
    const double* part;                             // [G], [S, G] or null (all zero)
    const int32_t* lines;                           // [c] or null
    float* line_severity;                           // [S, G, c]
    int32_t* line_worst_line;                       // [S, G, c]
    int32_t* line_overloads;                        // [S, G, c]
    float* line_post_flow;                          // [S, G, c, e] or null
    int G, c, p_per_sample, part_per_sample;
};

// the unit screen's own vectors behind ct_vec_bytes: double up [G], ua [G]; float a32 [G], u [n], dg [n], fg [e]; int ub [G];
// rounded to 16 bytes
__host__ __device__ inline size_t cu_extra_bytes(int n, int e, int G) {
    return ((size_t)24 * G + (size_t)8 * n + (size_t)4 * e + 15) & ~(size_t)15;
}
static inline size_t cu_vec_bytes(int n, int e, int G) { return ct_vec_bytes(n, e, ct_threads(n - 1) >> 6) + cu_extra_bytes(n, e, G); }
static inline size_t cu_lds_bytes(int n, int e, int G) { return cu_vec_bytes(n, e, G) + pf_mat_floats(n - 1) * 4; }
static inline bool cu_fits_lds(int n, int e, int G) { return cu_lds_bytes(n, e, G) <= (size_t)(kLdsCuBytes - kLdsReserve); }

// the two coefficients of d_g = alpha u - beta c_g: fp64, each rounded once
__device__ __forceinline__ void cu_coefficients(double p, double a, double A, float* alpha, float* beta) {
    const double rest = A - a;
    const bool shared = rest > 0.0;
    *alpha = shared ? (float)(p / rest) : 0.f;
    *beta = shared ? (float)(p * (a / rest + 1.0)) : (float)p;
}
// an entry of d_g and the post-outage flow of line l, every operation rounded on its own (as contingency_line.hpp's): PHASE B and
// PHASE C form the same bits from them
__device__ __forceinline__ float cu_delta(float alpha, float beta, float u, float cg) {
#pragma clang fp contract(off)
    const float t1 = alpha != 0.f ? alpha * u : 0.f;
    const float t2 = beta * cg;
    return t1 - t2;
}
__device__ __forceinline__ float cu_post(float da, float db, float x, float fl) {
#pragma clang fp contract(off)
    const float dd = da - db;
    const float q = dd / x;
    return fl + q;
}

template <bool LDS>
__global__ __launch_bounds__(PF_BIG_THREADS) void contingency_units_kernel(const CuArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_smem[];
    __shared__ double s_A;
    __shared__ int s_bad;
    const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, wave = t >> 6, nw = nt >> 6;
    const int s = blockIdx.x;
    const int n = a.n, e = a.e, m = n - 1, ld = pf_ld(m), G = a.G, c = a.c;
    const CtVecs v = ct_vecs(ct_smem, n, e, nw);
    const double* flow = v.flow;
    const float* x32 = v.x32;
    const float* rat = v.rat;
    const int* aidx = v.aidx;
    const uint16_t* la = v.la;
    const uint16_t* lb = v.lb;
    unsigned char* extra = ct_smem + ct_vec_bytes(n, e, nw);
    double* up = reinterpret_cast<double*>(extra);
    double* ua = up + G;
    float* a32 = reinterpret_cast<float*>(ua + G);
    float* u = a32 + G;
    float* dg = u + n;
    float* fg = dg + n;
    int* ub = reinterpret_cast<int*>(fg + e);
    float* X;
    if constexpr (LDS) X = reinterpret_cast<float*>(extra + cu_extra_bytes(n, e, G));
    else X = static_cast<float*>(a.ws) + (size_t)s * pf_mat_floats(m);

    // ================================================================================================ PHASE A
    if (threadIdx.x == 0) s_bad = 0;                // (PHASE A2's flag: ct_base_solve's barriers stand between this and its first use)
    int code = ct_base_solve(ct_base_in(a, s), v, X);

    // ================================================================================================ PHASE A2
    {
        const double* p_in = a.unit_p + (a.p_per_sample ? (int64_t)s * G : 0);
        const double* a_in = a.part ? a.part + (a.part_per_sample ? (int64_t)s * G : 0) : nullptr;
        int bad = 0;
        for (int g = t; g < G; g += nt) {
            const int b = a.units[g];
            const double p = p_in[g], w = a_in ? a_in[g] : 0.0;
            const bool id_ok = (unsigned)b < (unsigned)n;
            bad |= id_ok ? 0 : 1;
            bad |= (fabs(p) < __builtin_inf() && w >= 0.0 && w < __builtin_inf()) ? 0 : 2;
            ub[g] = id_ok ? b : 0;                  // (an id outside [0, n) is never followed)
            up[g] = p;
            ua[g] = w;
            a32[g] = (float)w;
        }
        if (bad) atomicOr(&s_bad, bad);             // (an integer OR on an LDS word: bit 0 a bad id, bit 1 a bad value)
        __syncthreads();
        bad = s_bad;
        if (code == 0 && bad) {
            // the scenario fails on its unit inputs: what ct_base_solve stored for it is taken back
            code = (bad & 1) ? PF_BAD_LINE : PF_NON_FINITE;
            for (int k = t; k < e; k += nt) a.base_flow[(int64_t)s * e + k] = __builtin_nan("");
            if (t == 0) a.status[s] = code;
        }
        if (code == 0) {
            if (t == 0) {
                double A = 0.0;
                for (int g = 0; g < G; ++g) A += ua[g];
                s_A = A;
            }
            for (int b = t; b < n; b += nt) {
                const int r = aidx[b];
                float acc = 0.f;
                if (r >= 0) {
                    const float* row = X + r * ld;
                    for (int g = 0; g < G; ++g) {
                        const int cg = aidx[ub[g]];
                        if (cg >= 0) acc = fmaf(a32[g], row[cg], acc);
                    }
                }
                u[b] = acc;
            }
        }
        __syncthreads();
    }
    const double A = code == 0 ? s_A : 0.0;

    // ================================================================================================ PHASE B
    float* w = v.wk + (size_t)wave * n;
    for (int g = wave; g < G; g += nw) {
        const int64_t o = (int64_t)s * G + g;
        float* row = a.post_flow ? a.post_flow + o * e : nullptr;
        if (code != 0) {
            ct_skip(true, row, e, lane, 64, a.severity[o], a.worst_line[o], a.overloads[o]);
            continue;
        }
        float alpha, beta;
        cu_coefficients(up[g], ua[g], A, &alpha, &beta);
        ct_column<false>(w, X, ld, aidx, n, aidx[ub[g]], -1, lane, 64);
        for (int b = lane; b < n; b += 64) w[b] = cu_delta(alpha, beta, u[b], w[b]);      // (a lane's own entries: no sync between)
        __syncwarp();                               // (the wave's own LDS vector: written by its lanes, gathered by its lanes)
        CtWorst worst = ct_worst_none();
        for (int l = lane; l < e; l += 64) {
            const float post = cu_post(w[la[l]], w[lb[l]], x32[l], (float)flow[l]);
            if (row) row[l] = post;
            const float r = rat[l];
            if (r > 0.f) ct_worst_add(worst, l, ct_loading(post, r));
        }
        worst = ct_worst_wave(worst);
        if (lane == 0) ct_store(ct_figures(worst), a.severity[o], a.worst_line[o], a.overloads[o]);
        __syncwarp();                               // (the next unit overwrites the vector)
    }
    if (c == 0) return;

    // ================================================================================================ PHASE C
    for (int g = 0; g < G; ++g) {
        if (code == 0) {
            float alpha, beta;
            cu_coefficients(up[g], ua[g], A, &alpha, &beta);
            const int cg = aidx[ub[g]];
            for (int b = t; b < n; b += nt) {
                const int r = aidx[b];
                const float xv = (r >= 0 && cg >= 0) ? X[r * ld + cg] : 0.f;               // (ct_column's element, whole workgroup)
                dg[b] = cu_delta(alpha, beta, u[b], xv);
            }
            __syncthreads();
            for (int l = t; l < e; l += nt) fg[l] = cu_post(dg[la[l]], dg[lb[l]], x32[l], (float)flow[l]);
            __syncthreads();
        }
        for (int j = wave; j < c; j += nw) {
            const int64_t o = ((int64_t)s * G + g) * c + j;
            float* row = a.line_post_flow ? a.line_post_flow + o * e : nullptr;
            const int k = a.lines[j];
            const bool line_ok = (unsigned)k < (unsigned)e;                                 // (a candidate that is no line is never followed)
            if (code != 0 || !line_ok || a.islands[k] != 0) {
                ct_skip(code != 0 || !line_ok, row, e, lane, 64, a.line_severity[o], a.line_worst_line[o], a.line_overloads[o]);
                continue;
            }
            const int bi = la[k], bj = lb[k];
            ct_column<false>(w, X, ld, aidx, n, aidx[bi], aidx[bj], lane, 64);
            __syncwarp();
            const float den = ct_den(w[bi], w[bj], x32[k]);
            const float fk = fg[k];
            CtWorst worst = ct_worst_none();
            for (int l = lane; l < e; l += 64) {
                const float post = l == k ? 0.f : ct_post(w[la[l]], w[lb[l]], x32[l], den, fg[l], fk);
                if (row) row[l] = post;
                const float r = rat[l];
                if (l != k && r > 0.f) ct_worst_add(worst, l, ct_loading(post, r));
            }
            worst = ct_worst_wave(worst);
            if (lane == 0) ct_store(ct_figures(worst), a.line_severity[o], a.line_worst_line[o], a.line_overloads[o]);
            __syncwarp();                           // (the next candidate overwrites the vector)
        }
        if (code == 0) __syncthreads();             // (the next unit overwrites dg and fg)
    }
}

static bool cu_sizes_ok(int64_t S, int64_t n, int64_t e, int64_t G, int64_t c) {
    return S >= 0 && n >= 2 && e >= 0 && G >= 1 && c >= 0 && S < (1ll << 29) && e < (1ll << 24) && n < (1ll << 24) && G < (1ll << 24) && c <= e;
}

}  // namespace pfn

using namespace pfn;

extern "C" {

size_t pfn_contingency_units_workspace_bytes(int64_t n_samples, int64_t n_bus, int64_t n_lines, int64_t n_units, int route) {
    if (n_samples <= 0 || !cu_sizes_ok(n_samples, n_bus, n_lines, n_units, 0) || n_bus > PF_MAX_UNKNOWNS + 1) return 0;
    if (route == 1 || (route != 2 && cu_fits_lds((int)n_bus, (int)n_lines, (int)n_units))) return 0;
    return (size_t)n_samples * pf_mat_floats((int)n_bus - 1) * sizeof(float);
}

int pfn_contingency_units(const int64_t* edge_index, int64_t n_lines, const double* rx, const int32_t* bus_type, const double* spec,
                          const double* ratings, int ratings_per_sample, const int32_t* units, int64_t n_units, const double* unit_p,
                          int unit_p_per_sample, const double* participation, int participation_per_sample, const int32_t* lines,
                          int64_t n_candidates, const int32_t* islands, int64_t n_samples, int64_t n_bus, int64_t n_pv, int64_t n_pq,
                          double tol, int max_iter, int route, float* severity, int32_t* worst_line, int32_t* overloads, double* base_flow,
                          int32_t* status, float* post_flow, float* line_severity, int32_t* line_worst_line, int32_t* line_overloads,
                          float* line_post_flow, int32_t* flags, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "pfn_contingency_units";
    PFN_CHECK_ARG(cu_sizes_ok(n_samples, n_bus, n_lines, n_units, n_candidates),
                  "%s: bad sizes (%lld scenarios of %lld buses and %lld lines, %lld units, %lld candidate lines)", who, (long long)n_samples,
                  (long long)n_bus, (long long)n_lines, (long long)n_units, (long long)n_candidates);
    PFN_CHECK_ARG(n_pv >= 0 && n_pq >= 0 && n_pv + n_pq == n_bus - 1, "%s: %lld PV and %lld PQ buses do not leave exactly one slack among %lld buses",
                  who, (long long)n_pv, (long long)n_pq, (long long)n_bus);
    PFN_CHECK_ARG(route >= 0 && route <= 2, "%s: route must be 0 (auto), 1 (LDS) or 2 (global)", who);
    PFN_CHECK_ARG(max_iter >= 0 && tol > 0.0, "%s: max_iter must be >= 0 and tol > 0", who);
    PFN_CHECK_ARG(n_bus - 1 <= PF_MAX_UNKNOWNS,
                  "%s: %lld unknowns per scenario exceed the dense screen's %d; the sparse route is not built", who, (long long)(n_bus - 1),
                  PF_MAX_UNKNOWNS);
    const int n = (int)n_bus, e = (int)n_lines, G = (int)n_units, c = (int)n_candidates, m = n - 1;
    const int threads = ct_threads(m);
    const size_t lds_max = (size_t)(kLdsCuBytes - kLdsReserve);
    const size_t vec = cu_vec_bytes(n, e, G), mat = pf_mat_floats(m) * 4;
    PFN_CHECK_ARG(vec <= lds_max, "%s: the vectors of %d buses, %d lines and %d units need %zu bytes of LDS, %zu are there", who, n, e, G, vec, lds_max);
    const bool fits = cu_fits_lds(n, e, G);
    PFN_CHECK_ARG(route != 1 || fits, "%s: route 1 (LDS): %d unknowns of %d buses, %d lines and %d units need %zu bytes of LDS, %zu are there", who, m,
                  n, e, G, cu_lds_bytes(n, e, G), lds_max);
    PFN_CHECK_ARG(n_samples * n_units < (1ll << 31) && n_samples * n_units * (c > 0 ? c : 1) < (1ll << 40),
                  "%s: %lld scenarios of %lld units and %lld candidate lines are too many items", who, (long long)n_samples, (long long)n_units,
                  (long long)n_candidates);
    if (n_samples == 0 || n_lines == 0) return PFN_OK;          // (nothing to screen: no launch, no output is written -- pfn_contingency_dc's rule)
    PFN_CHECK_ARG(edge_index && rx && bus_type && spec && units && unit_p && severity && worst_line && overloads && base_flow && status && flags,
                  "%s: null pointer", who);
    PFN_CHECK_ARG(c == 0 || (lines && islands && line_severity && line_worst_line && line_overloads),
                  "%s: null pointer (candidate lines need lines, islands and the three line figures)", who);
    const CuArgs a{edge_index, rx, bus_type, spec, ratings, islands, severity, worst_line, overloads, base_flow, status, post_flow, flags, ws, tol, n, e,
                   max_iter, (int)n_pv, (int)n_pq, ratings_per_sample != 0, units, unit_p, participation, lines, line_severity, line_worst_line,
                   line_overloads, line_post_flow, G, c, unit_p_per_sample != 0, participation_per_sample != 0};
    PFN_TRY(ct_check_aligned(who, a, lines));
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    PFN_CHECK_ARG(((at(unit_p) | at(participation)) & 7) == 0 &&
                      ((at(units) | at(line_severity) | at(line_worst_line) | at(line_overloads) | at(line_post_flow)) & 3) == 0,
                  "%s: unit_p and participation must be 8-byte aligned, units and the line figures 4-byte", who);
    const bool lds = route == 1 || (route == 0 && fits);
    if (!lds) {
        const size_t need = (size_t)n_samples * mat;
        if (!ws || ws_bytes < need) {
            set_error("%s: the global route needs a workspace of %zu bytes (got %zu)", who, need, ws ? ws_bytes : (size_t)0);
            return PFN_ENOSPACE;
        }
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double mm = (double)m, ee = (double)e, gg = (double)G, items = gg * (1.0 + (double)c);
    ProfScope ps("contingency_units",
                 (double)n_samples * (ee * 44.0 + (double)n * 32.0 + gg * 20.0 + items * 12.0 + (post_flow ? 4.0 * gg * ee : 0.0) +
                                      (line_post_flow ? 4.0 * gg * (double)c * ee : 0.0)),
                 (double)n_samples * (2.0 * mm * mm * mm + 6.0 * mm * mm + 2.0 * mm * gg + items * (2.0 * mm + 8.0 * ee)), s);
    return launch_either<contingency_units_kernel<true>, contingency_units_kernel<false>>(lds, (int)n_samples, threads, vec + mat, vec, s, a);
}

}  // extern "C"
