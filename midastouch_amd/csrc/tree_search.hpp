// tree_search.hpp - exact search of the static 8-ary box trees on the device (tree.hip builds them): eight lanes per query.
//
// The search is latency-bound pointer chasing over a tree that lives in L2 (K=50k: 128 KB of nodes + 1.6 MB of points);
// the traversal keeps its state in registers and one LDS column per level, so it needs no scratch.
#pragma once
#include "midas_internal.hpp"
#include "midas_math.hpp"

namespace midas {

template <class KD>
static TreeView<KD> view_of(const midas_tree* t) {
    TreeView<KD> v;
    v.boxes = (const typename KD::Box*)t->boxes;
    v.pts = (const typename KD::Point*)t->pts;
    v.inv_perm = t->inv_perm;
    v.nbrs = (const Nbr6*)t->nbrs;
    v.rho_out = t->rho_out;
    v.twin = t->twin;
    v.levels = t->levels;
    v.K = t->K;
    return v;
}

// =================================================================================================
// KD-tree: device traversal
// =================================================================================================
MD float dist2(const float* q, const Point6& p) {
    float d0 = q[0] - p.c[0], d1 = q[1] - p.c[1], d2 = q[2] - p.c[2];
    float d3 = q[3] - p.c[3], d4 = q[4] - p.c[4], d5 = q[5] - p.c[5];
    float d = d0 * d0;
    d = fmaf_(d1, d1, d);
    d = fmaf_(d2, d2, d);
    d = fmaf_(d3, d3, d);
    d = fmaf_(d4, d4, d);
    d = fmaf_(d5, d5, d);
    return d;
}
MD double dist2(const double* q, const Point3& p) {
    double d0 = q[0] - p.c[0], d1 = q[1] - p.c[1], d2 = q[2] - p.c[2];
    double d = d0 * d0;
    d = fma_(d1, d1, d);
    d = fma_(d2, d2, d);
    return d;
}

// Lower bound of dist2(q, p) over every p inside the box, IN THE COMPUTED ARITHMETIC: each per-axis
// offset is <= |q_j - p_j| after rounding (subtraction and max are monotone) and the fma chain has the
// same shape as dist2, so monotonicity of rounding carries the bound through.
MD float box_dist2(const float* q, const Box6& b) {
    float t[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float a = b.lo[j] - q[j], c = q[j] - b.hi[j];
        float m = a > c ? a : c;
        t[j] = m > 0.0f ? m : 0.0f;
    }
    float d = t[0] * t[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) d = fmaf_(t[j], t[j], d);
    return d;
}
MD double box_dist2(const double* q, const Box3& b) {
    double t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double a = b.lo[j] - q[j], c = q[j] - b.hi[j];
        double m = a > c ? a : c;
        t[j] = m > 0.0 ? m : 0.0;
    }
    double d = t[0] * t[0];
    d = fma_(t[1], t[1], d);
    d = fma_(t[2], t[2], d);
    return d;
}

MD int64_t level_offset_dev(int l) { return (((int64_t)1 << (3 * l)) - 1) / 7; }

// ---- octet-cooperative exact search ------------------------------------------------------------
// Eight lanes (an octet) serve ONE query: at a node each lane tests one child box, at a leaf two point
// slots.  The child distances of every level on the current path stay in an LDS column (cd[level][lane]),
// so backtracking touches no memory; each loop iteration issues one round of global loads (a 48-byte box
// or two 32-byte points per lane).  A wave therefore advances eight queries at a time and finishes a query
// in ~(levels + a few) rounds instead of the ~13-level descents of a binary tree walked per lane.
//
// All state below is octet-uniform except the lane's own child distance.  `cand` packs, per level, the
// 8-bit set of children still worth visiting.  Children are visited in order of box distance (3 low
// mantissa bits replaced by the child number: that only orders the visits, pruning uses exact values).
MD uint32_t octet_bits(bool pred, int octet) { return (uint32_t)((__ballot(pred) >> (8 * octet)) & 0xffull); }

// Cross-lane moves inside an octet as DPP modifiers (no LDS round trip): lane^1, lane^2 (quad permutes)
// and lane <-> 7-lane (row_half_mirror); applied in that order they form an 8-lane all-reduce butterfly.
template <int CTRL>
MD uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;

MD uint32_t octet_min(uint32_t v) {
    uint32_t t = dpp_u32<DPP_XOR1>(v); v = t < v ? t : v;
    t = dpp_u32<DPP_XOR2>(v); v = t < v ? t : v;
    t = dpp_u32<DPP_HALF_MIRROR>(v); v = t < v ? t : v;
    return v;
}

MD uint32_t order_key(float d, int j) { return (__float_as_uint(d) & ~7u) | (uint32_t)j; }
MD uint32_t order_key(double d, int j) { return (__float_as_uint(__double2float_rd(d)) & ~7u) | (uint32_t)j; }

// one butterfly step of a (distance, index) minimum, ties to the smaller index: the lane takes its DPP partner's pair if that is
// better.  Selects, no branches; NaN never wins.  (wave_best, row_best, group_best; left as they were, their instructions change
// with this form: the int64 step of octet_best below and the `if` step of particle_nn_prune_wg's group scan, front.hip)
template <int CTRL>
MD void best_step(float& d, int& i) {
    const float od = __uint_as_float(dpp_u32<CTRL>(__float_as_uint(d)));
    const int oi = (int)dpp_u32<CTRL>((uint32_t)i);
    const bool ob = (od < d) | ((od == d) & (oi < i));
    d = ob ? od : d;
    i = ob ? oi : i;
}
template <int CTRL>
MD void best_step(float& d, int64_t& i) {
    const float od = __uint_as_float(dpp_u32<CTRL>(__float_as_uint(d)));
    const int oi = (int)dpp_u32<CTRL>((uint32_t)(int)i);
    if (od < d || (od == d && (int64_t)oi < i)) { d = od; i = oi; }
}
template <int CTRL>
MD void best_step(double& d, int64_t& i) {  // mesh search: only the distance matters
    const uint64_t b = (uint64_t)__double_as_longlong(d);
    const uint64_t ob = ((uint64_t)dpp_u32<CTRL>((uint32_t)(b >> 32)) << 32) | dpp_u32<CTRL>((uint32_t)b);
    const double od = __longlong_as_double((long long)ob);
    if (od < d) d = od;
    (void)i;
}
// butterfly minimum over the octet; for the 6-d tree with the tie rule (smaller index wins)
template <typename T>
MD void octet_best(T& d, int64_t& i) {
    best_step<DPP_XOR1>(d, i);
    best_step<DPP_XOR2>(d, i);
    best_step<DPP_HALF_MIRROR>(d, i);
}

// One octet, one query.  `run` is octet-uniform; inactive octets fall through.  On entry (best, bi) is a
// valid candidate or (+inf, 0); on exit the exact minimum of the spec distance, ties to the smallest index.
// EXISTS: stop at the first point with d <= best (the entry bound); returns whether one was found.
template <class KD, bool EXISTS, bool STATS = false>
MD bool octet_search(const TreeView<KD>& tv, const typename KD::T* q, typename KD::T& best, int64_t& bi, bool run,
                     typename KD::T* cd, int* n_leaves = nullptr, int* n_nodes = nullptr) {
    using T = typename KD::T;
    static_assert(sizeof(typename KD::Box) == 48 && sizeof(typename KD::Point) == 32, "64-byte unified fetch");
    const int lane = threadIdx.x & 63, octet = lane >> 3, j = lane & 7;
    const int L = tv.levels;
    const int64_t leaf0 = level_offset_dev(L);
    int l = 0;
    int64_t n = 0;
    uint64_t cand = 0;
    bool found = false;
    bool enter = run && L > 0;   // fetch + test the children of n (level l)
    bool leaf = run && L == 0;   // fetch + scan leaf n
    while (__any(run)) {
        // one fetch per iteration whatever the octet is doing: this lane's child box (48 B) or its two
        // point slots (2 x 32 B) - 64 bytes from one base address, so a single wait covers both cases
        const uint4* src = reinterpret_cast<const uint4*>(tv.boxes);
        if (enter) src = reinterpret_cast<const uint4*>(tv.boxes + (8 * n + 1 + j));
        if (leaf) src = reinterpret_cast<const uint4*>(tv.pts + (size_t)(n - leaf0) * LEAF_CAP + 2 * j);
        uint4 r[4];
        if (run && (enter || leaf)) { r[0] = src[0]; r[1] = src[1]; r[2] = src[2]; r[3] = src[3]; }
        if (run) {
            if (enter) {
                typename KD::Box bx;
                __builtin_memcpy(&bx, r, sizeof(bx));
                const T d = box_dist2(q, bx);
                cd[l * 64] = d;
                if (STATS) ++*n_nodes;
                const uint32_t m = octet_bits(d <= best, octet);
                cand = (cand & ~(0xffull << (8 * l))) | ((uint64_t)m << (8 * l));
                enter = false;
            } else if (leaf) {
                typename KD::Point p0, p1;
                __builtin_memcpy(&p0, r, sizeof(p0));
                __builtin_memcpy(&p1, r + 2, sizeof(p1));
                if (STATS) ++*n_leaves;
                T d0 = dist2(q, p0), d1 = dist2(q, p1);
                int64_t i0 = p0.idx, i1 = p1.idx;
                if (d1 < d0 || (d1 == d0 && i1 < i0)) { d0 = d1; i0 = i1; }
                if (!(d0 == d0)) { d0 = INFINITY; i0 = 0x7fffffff; }  // NaN never wins
                octet_best(d0, i0);
                if (EXISTS) {
                    if (d0 <= best) { best = d0; bi = i0; found = true; run = false; }
                } else if (d0 < best || (d0 == best && i0 < bi)) {
                    best = d0;
                    bi = i0;
                }
                leaf = false;
                if (L == 0) run = false;
                else n = (n - 1) >> 3;  // back to the parent; l already points at it
            }
        }
        if (run) {
            // next child at level l: the nearest still-alive candidate
            const T d = cd[l * 64];
            const bool alive = ((cand >> (8 * l + j)) & 1ull) && (d <= best);
            const uint32_t m = octet_bits(alive, octet);
            if (m == 0) {
                if (l == 0) run = false;
                else { --l; n = (n - 1) >> 3; }
            } else {
                const uint32_t jm = octet_min(alive ? order_key(d, j) : 0xffffffffu) & 7u;
                cand = (cand & ~(0xffull << (8 * l))) | ((uint64_t)(m & ~(1u << jm)) << (8 * l));
                n = 8 * n + 1 + jm;
                if (l + 1 == L) leaf = true;
                else { ++l; enter = true; }
            }
        }
    }
    return found;
}

// Wave-level driver: lanes with `need` set get their query served by an octet, eight queries per round.
template <class KD, bool EXISTS, bool STATS = false>
MD bool wave_search(const TreeView<KD>& tv, const typename KD::T* q, typename KD::T& best, int64_t& bi, bool need,
                    typename KD::T* cd_base, int* n_leaves = nullptr, int* n_nodes = nullptr) {
    using T = typename KD::T;
    constexpr int DIM = KD::DIM;
    const int lane = threadIdx.x & 63, octet = lane >> 3;
    uint64_t todo = __ballot(need);
    bool found = false;
    while (todo) {
        // owner of this octet = the octet-th set bit of todo
        uint64_t t = todo;
        int owner = -1;
        for (int k = 0; k <= octet && t; ++k) {
            owner = k == octet ? (int)__builtin_ctzll(t) : -1;
            t &= t - 1;
        }
        const bool active = owner >= 0;
        const int src = active ? owner : lane;
        T qq[DIM];
#pragma unroll
        for (int d = 0; d < DIM; ++d) qq[d] = __shfl(q[d], src);
        T b = __shfl(best, src);
        int64_t i = (int64_t)__shfl((long long)bi, src);
        int nl = 0, nn = 0;
        const bool f = octet_search<KD, EXISTS, STATS>(tv, qq, b, i, active, cd_base + lane, &nl, &nn);
        // hand the result back to the owner lanes
        const int rank = (int)__builtin_popcountll(todo & ((1ull << lane) - 1ull));
        const bool served = ((todo >> lane) & 1ull) && rank < 8;
        const int from = 8 * (rank < 8 ? rank : 0);
        const T rb = __shfl(b, from);
        const int64_t ri = (int64_t)__shfl((long long)i, from);
        const int rf = __shfl((int)f, from);
        const int rl = __shfl(nl, from), rn = __shfl(nn, from);
        if (served) {
            best = rb;
            bi = ri;
            found = rf != 0;
            if (STATS) { *n_leaves += rl; *n_nodes += rn; }
        }
        for (int k = 0; k < 8 && todo; ++k) todo &= todo - 1;
    }
    return found;
}

}  // namespace midas
