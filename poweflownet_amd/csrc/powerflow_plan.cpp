// The symbolic half of the sparse power-flow route (powerflow_sparse.hip), on the host: pfn_powerflow_sparse_plan turns one grid
// (bus types + stored lines) into the blob powerflow_plan.hpp describes -- the elimination order, the filled pattern of the Jacobian
// under that order, a per-bus list of line ends and the slab position of every Jacobian entry.  No device code, no GPU; plain C++ so
// that it can be linked into a stand-alone program as well.
//
// Order: explicit-elimination minimum degree on the BUS graph (parallel lines collapse, self-pairs vanish, the slack is left out: it
// has no unknown), ties to the lowest bus id -- the plan is a pure function of its inputs.  Eliminating a bus makes its neighbours a
// clique; the neighbour set at that moment is the L structure of its block column.  Every (bus, bus) block of the filled pattern is
// taken full (a PV bus has one unknown, a PQ bus two), which keeps the scalar pattern structurally symmetric and closed under
// elimination.  Cost: the sum of the squared column lengths, 83 M set operations at (6470, 9005).
#include <algorithm>
#include <cstring>
#include <iterator>
#include <set>
#include <utility>
#include <vector>

#include "../../include/pfn_hip.h"
#include "powerflow_plan.hpp"

namespace pfn {
void set_error(const char* fmt, ...);
}
using namespace pfn;

namespace {

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// plan null: nothing is written, *bytes_out gets the size.  Returns PFN_OK or PFN_EINVAL (text set).
// mode 0 / 1: the public plans.  PLAN_PQ (internal, the Q half of a fast-decoupled plan): the PQ buses alone carry an unknown, one
// each; the slack AND the PV buses are left out of the bus graph; the header says mode 1 (one unknown per bus) and `order` has m entries.
constexpr int PLAN_PQ = 2;
int build_plan(const char* who, const int64_t* ei, int64_t e, const int32_t* bt, int64_t n, int mode, void* plan, size_t plan_bytes,
               size_t* bytes_out) {
    if (!(n >= 1 && e >= 0 && n < (1ll << 24) && e < (1ll << 24))) {
        set_error("%s: bad sizes (%lld buses, %lld lines)", who, (long long)n, (long long)e);
        return PFN_EINVAL;
    }
    if (mode != 0 && mode != 1 && mode != PLAN_PQ) {
        set_error("%s: mode must be 0 (AC) or 1 (DC)", who);
        return PFN_EINVAL;
    }
    if (!bt || (!ei && e)) {
        set_error("%s: null pointer", who);
        return PFN_EINVAL;
    }
    int64_t n_slack = 0, slack = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (bt[i] < 0 || bt[i] > 2) {
            set_error("%s: bus %lld has type %d; only 0 (slack), 1 (PV) and 2 (PQ) exist", who, (long long)i, (int)bt[i]);
            return PFN_EINVAL;
        }
        if (bt[i] == 0) { ++n_slack; slack = i; }
    }
    if (n_slack != 1) {
        set_error("%s: %lld slack buses; exactly one is needed", who, (long long)n_slack);
        return PFN_EINVAL;
    }
    for (int64_t k = 0; k < e; ++k) {
        if ((uint64_t)ei[k] >= (uint64_t)n || (uint64_t)ei[e + k] >= (uint64_t)n) {
            set_error("%s: line %lld names a bus outside [0, %lld)", who, (long long)k, (long long)n);
            return PFN_EINVAL;
        }
    }
    const int N = (int)n, E = (int)e;
    const bool dc = mode != 0;
    // the buses that carry an unknown: all but the slack; PLAN_PQ: the PQ buses alone
    auto in_graph = [&](int i) { return mode == PLAN_PQ ? bt[i] == 2 : i != slack; };

    // ---- minimum degree on the bus graph induced on those buses
    std::vector<std::vector<int>> nb(N);
    for (int k = 0; k < E; ++k) {
        const int a = (int)ei[k], b = (int)ei[e + k];
        if (a == b || !in_graph(a) || !in_graph(b)) continue;
        nb[a].push_back(b);
        nb[b].push_back(a);
    }
    std::set<std::pair<int, int>> heap;             // (degree, bus)
    for (int i = 0; i < N; ++i) {
        std::sort(nb[i].begin(), nb[i].end());
        nb[i].erase(std::unique(nb[i].begin(), nb[i].end()), nb[i].end());
        if (in_graph(i)) heap.insert({(int)nb[i].size(), i});
    }
    std::vector<int> order, where(N, -1);           // where[bus] = its place in the order
    order.reserve(N);
    std::vector<std::vector<int>> lower(N);          // by place: the buses (ids) of the L structure of that block column
    std::vector<int> merged;
    while (!heap.empty()) {
        const int v = heap.begin()->second;
        heap.erase(heap.begin());
        where[v] = (int)order.size();
        order.push_back(v);
        std::vector<int>& nv = nb[v];                // all still to be eliminated: v is taken out of their lists below
        for (int u : nv) {
            std::vector<int>& nu = nb[u];
            heap.erase({(int)nu.size(), u});
            merged.clear();
            std::set_union(nu.begin(), nu.end(), nv.begin(), nv.end(), std::back_inserter(merged));
            merged.erase(std::remove_if(merged.begin(), merged.end(), [&](int w) { return w == u || w == v; }), merged.end());
            nu.swap(merged);
            heap.insert({(int)nu.size(), u});
        }
        lower[where[v]].swap(nv);
    }
    const int NB = (int)order.size();                // N - 1; PLAN_PQ: the number of PQ buses
    // ---- unknown numbering in that order; upper[place] = earlier places whose L structure holds this bus (ascending by construction)
    std::vector<int> ua(N, -1), uv(N, -1);
    int64_t m64 = 0;
    for (int p = 0; p < NB; ++p) {
        const int v = order[p];
        ua[v] = (int)m64++;
        if (bt[v] == 2 && !dc) uv[v] = (int)m64++;
    }
    const int M = (int)m64;
    std::vector<std::vector<int>> upper(NB);
    for (int p = 0; p < NB; ++p) {
        std::vector<int>& lo = lower[p];
        for (int& b : lo) b = where[b];              // ids -> places
        std::sort(lo.begin(), lo.end());
        for (int q : lo) upper[q].push_back(p);
    }
    auto width = [&](int place) { return uv[order[place]] >= 0 ? 2 : 1; };
    // ---- the filled pattern by columns
    std::vector<int64_t> colptr(M + 1, 0), diag(M, 0);
    int64_t nnz = 0, nnz_l = 0, madds = 0, max_col = 0;
    for (int p = 0; p < NB; ++p) {
        int64_t up = 0, lo = 0;
        for (int q : upper[p]) up += width(q);
        for (int q : lower[p]) lo += width(q);
        const int w = width(p), c0 = ua[order[p]];
        for (int c = 0; c < w; ++c) {
            colptr[c0 + c] = nnz;
            diag[c0 + c] = nnz + up + c;
            const int64_t l = lo + (w - 1 - c);
            nnz += up + w + lo;
            nnz_l += l;
            madds += l * l;
            max_col = std::max(max_col, l);
        }
    }
    colptr[M] = nnz;
    const bool idx16 = M <= 65535;
    const int64_t n_adj = 2ll * E;
    // ---- sizes and offsets
    int64_t off = (int64_t)PFP_HEADER_WORDS * 4;
    auto place_section = [&](int64_t bytes) {
        const int64_t at = off;
        off = align16(off + bytes);
        return at;
    };
    const int64_t o_order = place_section(4ll * NB), o_ua = place_section(4ll * N), o_uv = place_section(4ll * N);
    const int64_t o_colptr = place_section(4ll * (M + 1)), o_diag = place_section(4ll * M);
    const int64_t o_rowidx = place_section((idx16 ? 2ll : 4ll) * nnz), o_adjptr = place_section(4ll * (N + 1));
    const int64_t o_adj = place_section(8ll * n_adj), o_adjpos = place_section(16ll * n_adj), o_buspos = place_section(16ll * N);
    const int64_t total = off;
    if (total >= (1ll << 31) || nnz >= (1ll << 31)) {
        set_error("%s: a filled pattern of %lld entries (a plan of %lld bytes) does not fit 32-bit offsets", who,
                  (long long)nnz, (long long)total);
        return PFN_EINVAL;
    }
    if (bytes_out) *bytes_out = (size_t)total;
    if (!plan) return PFN_OK;
    if (plan_bytes < (size_t)total) {
        set_error("%s: the plan needs %lld bytes (got %zu)", who, (long long)total, plan_bytes);
        return PFN_EINVAL;
    }
    unsigned char* base = static_cast<unsigned char*>(plan);
    std::memset(base, 0, (size_t)total);
    int32_t* H = reinterpret_cast<int32_t*>(base);
    H[PFP_H_MAGIC] = PFP_MAGIC;
    H[PFP_H_VERSION] = PFP_VERSION;
    H[PFP_H_N] = N;
    H[PFP_H_E] = E;
    H[PFP_H_M] = M;
    H[PFP_H_MODE] = dc ? 1 : 0;
    H[PFP_H_NNZ] = (int32_t)nnz;
    H[PFP_H_NNZ_L] = (int32_t)nnz_l;
    H[PFP_H_MADDS_LO] = (int32_t)(uint32_t)(madds & 0xffffffffll);
    H[PFP_H_MADDS_HI] = (int32_t)(madds >> 32);
    H[PFP_H_IDX16] = idx16;
    H[PFP_H_MAX_COL] = (int32_t)max_col;
    H[PFP_H_N_ADJ] = (int32_t)n_adj;
    H[PFP_H_BYTES] = (int32_t)total;
    H[PFP_H_SLACK] = (int32_t)slack;
    H[PFP_H_OFF_ORDER] = (int32_t)o_order;
    H[PFP_H_OFF_UA] = (int32_t)o_ua;
    H[PFP_H_OFF_UV] = (int32_t)o_uv;
    H[PFP_H_OFF_COLPTR] = (int32_t)o_colptr;
    H[PFP_H_OFF_DIAG] = (int32_t)o_diag;
    H[PFP_H_OFF_ROWIDX] = (int32_t)o_rowidx;
    H[PFP_H_OFF_ADJPTR] = (int32_t)o_adjptr;
    H[PFP_H_OFF_ADJ] = (int32_t)o_adj;
    H[PFP_H_OFF_ADJPOS] = (int32_t)o_adjpos;
    H[PFP_H_OFF_BUSPOS] = (int32_t)o_buspos;
    auto words = [&](int64_t o) { return reinterpret_cast<int32_t*>(base + o); };
    for (int p = 0; p < NB; ++p) words(o_order)[p] = order[p];
    for (int i = 0; i < N; ++i) {
        words(o_ua)[i] = ua[i];
        words(o_uv)[i] = uv[i];
    }
    for (int j = 0; j <= M; ++j) words(o_colptr)[j] = (int32_t)colptr[j];
    for (int j = 0; j < M; ++j) words(o_diag)[j] = (int32_t)diag[j];
    // rows of a block column: the unknowns of the upper places, its own, the lower places -- ascending, since places are
    std::vector<int> rows;
    uint16_t* r16 = reinterpret_cast<uint16_t*>(base + o_rowidx);
    int32_t* r32 = words(o_rowidx);
    auto push_bus = [&](int place) {
        const int b = order[place];
        rows.push_back(ua[b]);
        if (uv[b] >= 0) rows.push_back(uv[b]);
    };
    for (int p = 0; p < NB; ++p) {
        rows.clear();
        for (int q : upper[p]) push_bus(q);
        push_bus(p);
        for (int q : lower[p]) push_bus(q);
        for (int c = 0; c < width(p); ++c) {
            const int64_t at = colptr[ua[order[p]] + c];
            for (size_t k = 0; k < rows.size(); ++k) {
                if (idx16) r16[at + (int64_t)k] = (uint16_t)rows[k];
                else r32[at + (int64_t)k] = rows[k];
            }
        }
    }
    auto row_at = [&](int64_t pos) { return idx16 ? (int)r16[pos] : r32[pos]; };
    auto position = [&](int row, int col) -> int32_t {          // slab position of (row, col), -1 where either is no unknown
        if (row < 0 || col < 0) return -1;
        int64_t lo = colptr[col], hi = colptr[col + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (row_at(mid) < row) lo = mid + 1;
            else hi = mid;
        }
        return (lo < colptr[col + 1] && row_at(lo) == row) ? (int32_t)lo : -2;
    };
    // ---- line ends by bus, stored order
    int32_t* adjptr = words(o_adjptr);
    int32_t* adj = words(o_adj);
    int32_t* adjpos = words(o_adjpos);
    int32_t* buspos = words(o_buspos);
    std::vector<int32_t> fill(N, 0);
    for (int k = 0; k < E; ++k) {
        ++fill[(int)ei[k]];
        ++fill[(int)ei[e + k]];
    }
    adjptr[0] = 0;
    for (int i = 0; i < N; ++i) {
        adjptr[i + 1] = adjptr[i] + fill[i];
        fill[i] = adjptr[i];
    }
    bool missing = false;
    for (int k = 0; k < E; ++k) {
        for (int side = 0; side < 2; ++side) {
            const int i = (int)(side ? ei[e + k] : ei[k]), j = (int)(side ? ei[k] : ei[e + k]);
            const int q = fill[i]++;
            adj[2 * q] = 2 * k + side;
            adj[2 * q + 1] = j;
            const int32_t pos[4] = {position(ua[i], ua[j]), position(ua[i], uv[j]), position(uv[i], ua[j]), position(uv[i], uv[j])};
            for (int c = 0; c < 4; ++c) {
                adjpos[4 * q + c] = pos[c];
                missing |= pos[c] == -2;
            }
        }
    }
    for (int i = 0; i < N; ++i) {
        const int32_t pos[4] = {position(ua[i], ua[i]), position(ua[i], uv[i]), position(uv[i], ua[i]), position(uv[i], uv[i])};
        for (int c = 0; c < 4; ++c) {
            buspos[4 * i + c] = pos[c];
            missing |= pos[c] == -2;
        }
    }
    if (missing) {                                   // (cannot happen: every line's block is in the pattern by construction)
        set_error("%s: internal error, a Jacobian entry has no place in the filled pattern", who);
        std::memset(base, 0, (size_t)total);
        return PFN_EINVAL;
    }
    return PFN_OK;
}

}  // namespace

extern "C" {

// (the size is known only once the elimination has run: the sizing call and the build call each run it -- 0.35 s apiece at 6470
//  buses, once per grid -- and neither keeps anything behind; pfn_powerflow_sparse_plan_into below runs it once)
size_t pfn_powerflow_sparse_plan_bytes(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, int mode) {
    size_t bytes = 0;
    if (mode != 0 && mode != 1) mode = -1;          // (the internal kinds are not reachable from here)
    return build_plan("pfn_powerflow_sparse_plan", edge_index, n_lines, bus_type, n_bus, mode, nullptr, 0, &bytes) == PFN_OK ? bytes : 0;
}

int pfn_powerflow_sparse_plan(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, int mode, void* plan,
                              size_t plan_bytes) {
    if (!plan) {
        set_error("pfn_powerflow_sparse_plan: null plan");
        return PFN_EINVAL;
    }
    if (mode != 0 && mode != 1) mode = -1;
    return build_plan("pfn_powerflow_sparse_plan", edge_index, n_lines, bus_type, n_bus, mode, plan, plan_bytes, nullptr);
}

// the outer header of a fast-decoupled plan whose two sub-plans stand at off_p and off_q of `base`
static int finish_fd_plan(const char* who, unsigned char* base, int64_t off_p, int64_t off_q, int64_t total) {
    int32_t* H = reinterpret_cast<int32_t*>(base);
    const int32_t* P = reinterpret_cast<const int32_t*>(base + off_p);
    const int32_t* Q = reinterpret_cast<const int32_t*>(base + off_q);
    auto madds_of = [](const int32_t* h) { return ((int64_t)h[PFP_H_MADDS_HI] << 32) | (uint32_t)h[PFP_H_MADDS_LO]; };
    const int64_t madds = madds_of(P) + madds_of(Q), nnz = (int64_t)P[PFP_H_NNZ] + Q[PFP_H_NNZ];
    if (nnz >= (1ll << 31)) {
        set_error("%s: filled patterns of %lld entries do not fit 32-bit offsets", who, (long long)nnz);
        std::memset(base, 0, (size_t)total);
        return PFN_EINVAL;
    }
    H[PFP_H_MAGIC] = PFD_MAGIC;
    H[PFP_H_VERSION] = PFP_VERSION;
    H[PFP_H_N] = P[PFP_H_N];
    H[PFP_H_E] = P[PFP_H_E];
    H[PFP_H_M] = P[PFP_H_M];
    H[PFP_H_MODE] = PFD_MODE;
    H[PFP_H_NNZ] = (int32_t)nnz;
    H[PFP_H_NNZ_L] = P[PFP_H_NNZ_L] + Q[PFP_H_NNZ_L];
    H[PFP_H_MADDS_LO] = (int32_t)(uint32_t)(madds & 0xffffffffll);
    H[PFP_H_MADDS_HI] = (int32_t)(madds >> 32);
    H[PFP_H_IDX16] = P[PFP_H_IDX16] && Q[PFP_H_IDX16];
    H[PFP_H_MAX_COL] = std::max(P[PFP_H_MAX_COL], Q[PFP_H_MAX_COL]);
    H[PFP_H_N_ADJ] = P[PFP_H_N_ADJ];
    H[PFP_H_BYTES] = (int32_t)total;
    H[PFP_H_SLACK] = P[PFP_H_SLACK];
    H[PFD_H_M_Q] = Q[PFP_H_M];
    H[PFD_H_OFF_P] = (int32_t)off_p;
    H[PFD_H_OFF_Q] = (int32_t)off_q;
    return PFN_OK;
}

// The fast-decoupled plan (layout: powerflow_plan.hpp): an outer header, then two complete sub-plans -- P, B' over the angle buses
// (byte for byte the mode-1 plan), and Q, B'' over the PQ buses.  Each sizing call runs both eliminations.
static int build_fd_plan(const int64_t* ei, int64_t e, const int32_t* bt, int64_t n, void* plan, size_t plan_bytes, size_t* bytes_out) {
    const char* who = "pfn_powerflow_sparse_fd_plan";
    size_t bytes_p = 0, bytes_q = 0;
    if (build_plan(who, ei, e, bt, n, 1, nullptr, 0, &bytes_p) != PFN_OK) return PFN_EINVAL;
    if (build_plan(who, ei, e, bt, n, PLAN_PQ, nullptr, 0, &bytes_q) != PFN_OK) return PFN_EINVAL;
    const int64_t off_p = (int64_t)PFP_HEADER_WORDS * 4, off_q = off_p + align16((int64_t)bytes_p), total = off_q + align16((int64_t)bytes_q);
    if (total >= (1ll << 31)) {
        set_error("%s: a plan of %lld bytes does not fit 32-bit offsets", who, (long long)total);
        return PFN_EINVAL;
    }
    if (bytes_out) *bytes_out = (size_t)total;
    if (!plan) return PFN_OK;
    if (plan_bytes < (size_t)total) {
        set_error("%s: the plan needs %lld bytes (got %zu)", who, (long long)total, plan_bytes);
        return PFN_EINVAL;
    }
    unsigned char* base = static_cast<unsigned char*>(plan);
    std::memset(base, 0, (size_t)total);
    if (build_plan(who, ei, e, bt, n, 1, base + off_p, bytes_p, nullptr) != PFN_OK ||
        build_plan(who, ei, e, bt, n, PLAN_PQ, base + off_q, bytes_q, nullptr) != PFN_OK) {
        std::memset(base, 0, (size_t)total);
        return PFN_EINVAL;
    }
    return finish_fd_plan(who, base, off_p, off_q, total);
}

size_t pfn_powerflow_sparse_fd_plan_bytes(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus) {
    size_t bytes = 0;
    return build_fd_plan(edge_index, n_lines, bus_type, n_bus, nullptr, 0, &bytes) == PFN_OK ? bytes : 0;
}

int pfn_powerflow_sparse_fd_plan(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, void* plan,
                                 size_t plan_bytes) {
    if (!plan) {
        set_error("pfn_powerflow_sparse_fd_plan: null plan");
        return PFN_EINVAL;
    }
    return build_fd_plan(edge_index, n_lines, bus_type, n_bus, plan, plan_bytes, nullptr);
}

// One elimination per matrix where the two calls above run two (the fast-decoupled pair: six): the plan is built straight into a
// buffer the caller sized by a guess -- a plan of the same grid with a few lines more or fewer is a good one.  *needed gets the
// plan's size whenever the inputs are valid; a buffer that is too small (or null) is PFN_ENOSPACE, nothing usable is written, and
// the caller comes again with `needed` bytes.  mode 0, 1, or 2: the fast-decoupled plan.  The blob is the two-call path's, byte for byte.
int pfn_powerflow_sparse_plan_into(const int64_t* edge_index, int64_t n_lines, const int32_t* bus_type, int64_t n_bus, int mode, void* plan,
                                   size_t plan_bytes, size_t* needed) {
    const char* who = "pfn_powerflow_sparse_plan_into";
    if (!needed) {
        set_error("%s: null needed", who);
        return PFN_EINVAL;
    }
    *needed = 0;
    if (!plan) plan_bytes = 0;
    unsigned char* base = static_cast<unsigned char*>(plan);
    if (mode == 0 || mode == 1) {
        size_t bytes = 0;
        const int rc = build_plan(who, edge_index, n_lines, bus_type, n_bus, mode, plan_bytes ? plan : nullptr, plan_bytes, &bytes);
        *needed = bytes;
        if (bytes == 0) return PFN_EINVAL;              // (the inputs were refused: the text is set)
        if (bytes > plan_bytes) {
            set_error("%s: the plan needs %zu bytes (got %zu)", who, bytes, plan_bytes);
            return PFN_ENOSPACE;
        }
        return rc;
    }
    if (mode != PFD_MODE) {
        set_error("%s: mode must be 0 (AC), 1 (DC) or 2 (the fast-decoupled plan)", who);
        return PFN_EINVAL;
    }
    // each half goes where it belongs if the room behind it suffices; a half that does not fit is sized only
    const int64_t off_p = (int64_t)PFP_HEADER_WORDS * 4;
    size_t bytes_p = 0, bytes_q = 0;
    const size_t room_p = plan_bytes > (size_t)off_p ? plan_bytes - (size_t)off_p : 0;
    const int rc_p = build_plan(who, edge_index, n_lines, bus_type, n_bus, 1, room_p ? base + off_p : nullptr, room_p, &bytes_p);
    if (bytes_p == 0) return PFN_EINVAL;
    const int64_t off_q = off_p + align16((int64_t)bytes_p);
    const size_t room_q = bytes_p <= room_p && plan_bytes > (size_t)off_q ? plan_bytes - (size_t)off_q : 0;
    const int rc_q = build_plan(who, edge_index, n_lines, bus_type, n_bus, PLAN_PQ, room_q ? base + off_q : nullptr, room_q, &bytes_q);
    if (bytes_q == 0) return PFN_EINVAL;
    const int64_t total = off_q + align16((int64_t)bytes_q);
    if (total >= (1ll << 31)) {
        set_error("%s: a plan of %lld bytes does not fit 32-bit offsets", who, (long long)total);
        return PFN_EINVAL;
    }
    *needed = (size_t)total;
    if ((size_t)total > plan_bytes || bytes_p > room_p || bytes_q > room_q) {
        set_error("%s: the plan needs %lld bytes (got %zu)", who, (long long)total, plan_bytes);
        return PFN_ENOSPACE;
    }
    if (rc_p != PFN_OK || rc_q != PFN_OK) return PFN_EINVAL;
    std::memset(base, 0, (size_t)off_p);
    std::memset(base + off_p + bytes_p, 0, (size_t)(off_q - off_p) - bytes_p);
    std::memset(base + off_q + bytes_q, 0, (size_t)(total - off_q) - bytes_q);
    return finish_fd_plan(who, base, off_p, off_q, total);
}

}  // extern "C"
