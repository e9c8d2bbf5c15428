// tree.hip - the spatial indices: host build of the 8-ary box trees (with the host neighbour-graph and vertex-list builders, the
// checkers of index_build.hip), upload, the mesh's distance field, and the stand-alone search operators (nn6, nn3, knn6).
#include <algorithm>
#include <cmath>
#include <numeric>
#include <thread>
#include <vector>

#include "midas_internal.hpp"
#include "midas_math.hpp"
#include "list_scan.hpp"

namespace midas {

// =================================================================================================
// spatial index: host build (balanced median splits, three binary splits per 8-ary level)
// =================================================================================================
template <class KD>
struct HostTree {
    std::vector<typename KD::Box> boxes;
    std::vector<typename KD::Point> pts;
    std::vector<int32_t> inv_perm;
    std::vector<Nbr6> nbrs;      // dim 6 only
    std::vector<float> rho_out;  // dim 6 only
    std::vector<int32_t> twin;   // dim 6 only
    int levels = 0;              // 8-ary levels
};

static inline int64_t level_offset(int l) { return (((int64_t)1 << (3 * l)) - 1) / 7; }

// binary node `b` (1-based heap) at binary depth `depth`; every third depth is an 8-ary node
template <class KD>
static void build_rec(HostTree<KD>& t, const typename KD::T* P, std::vector<int32_t>& perm, uint64_t b, int64_t lo,
                      int64_t hi, int depth) {
    using T = typename KD::T;
    constexpr int DIM = KD::DIM;
    typename KD::Box bx;
    for (int d = 0; d < DIM; ++d) { bx.lo[d] = INFINITY; bx.hi[d] = -INFINITY; }
    for (int64_t i = lo; i < hi; ++i)
        for (int d = 0; d < DIM; ++d) {
            T v = P[(int64_t)perm[i] * DIM + d];
            bx.lo[d] = v < bx.lo[d] ? v : bx.lo[d];
            bx.hi[d] = v > bx.hi[d] ? v : bx.hi[d];
        }
    if (depth % 3 == 0) {
        const int l = depth / 3;
        const int64_t local = (int64_t)b - ((int64_t)1 << depth);
        t.boxes[level_offset(l) + local] = bx;
        if (l == t.levels) {
            std::sort(perm.begin() + lo, perm.begin() + hi);
            for (int64_t i = lo; i < hi; ++i) {
                typename KD::Point p;
                for (int d = 0; d < DIM; ++d) p.c[d] = P[(int64_t)perm[i] * DIM + d];
                p.idx = perm[i];
                if constexpr (DIM == 6) p.pad = 0;
                const int64_t slot = local * LEAF_CAP + (i - lo);
                t.pts[slot] = p;
                t.inv_perm[perm[i]] = (int32_t)slot;
            }
            return;
        }
    }
    int best_dim = 0;
    T best_spread = -1;
    for (int d = 0; d < DIM; ++d)
        if (bx.hi[d] - bx.lo[d] > best_spread) { best_spread = bx.hi[d] - bx.lo[d]; best_dim = d; }
    const int64_t mid = lo + (hi - lo + 1) / 2;
    auto cmp = [&](int32_t a, int32_t c) {
        T va = P[(int64_t)a * DIM + best_dim], vc = P[(int64_t)c * DIM + best_dim];
        return va < vc || (va == vc && a < c);
    };
    if (mid < hi) std::nth_element(perm.begin() + lo, perm.begin() + mid, perm.begin() + hi, cmp);
    build_rec(t, P, perm, 2 * b, lo, mid, depth + 1);
    build_rec(t, P, perm, 2 * b + 1, mid, hi, depth + 1);
}

template <class KD>
static HostTree<KD> build_tree(const typename KD::T* P, int64_t K) {
    HostTree<KD> t;
    int levels = 0;
    while ((((int64_t)LEAF_CAP) << (3 * levels)) < K) ++levels;
    t.levels = levels;
    const int64_t nleaves = (int64_t)1 << (3 * levels);
    t.boxes.resize(level_offset(levels + 1) + 1);  // +1: the 64-byte unified fetch reads 16 bytes past a box
    typename KD::Point pad;
    for (int d = 0; d < KD::DIM; ++d) pad.c[d] = INFINITY;
    pad.idx = 0x7fffffff;
    if constexpr (KD::DIM == 6) pad.pad = 0;
    t.pts.assign(nleaves * LEAF_CAP, pad);
    t.inv_perm.resize(K);
    std::vector<int32_t> perm(K);
    std::iota(perm.begin(), perm.end(), 0);
    build_rec(t, P, perm, 1u, 0, K, 0);
    return t;
}

// ---- neighbour graph of the codebook features (hint fast path) ---------------------------------
// For every entry k: its NBR_M nearest other entries sorted by (distance, index), float64 distances,
// rho rounded DOWN to float32 so that it never over-states a true distance.
namespace {
struct HeapItem { double d; int64_t idx; };
inline bool heap_less(const HeapItem& a, const HeapItem& b) { return a.d < b.d || (a.d == b.d && a.idx < b.idx); }

template <class KD>
double host_box_d2(const double* q, const typename KD::Box& b) {
    double d = 0.0;
    for (int j = 0; j < KD::DIM; ++j) {
        double a = (double)b.lo[j] - q[j], c = q[j] - (double)b.hi[j];
        double m = a > c ? a : c;
        if (m > 0) d += m * m;
    }
    return d;
}

// k nearest points of q (float64 distances), excluding original index `self` (-1: none)
template <class KD>
void knn_rec(const HostTree<KD>& t, const double* q, int64_t self, int64_t node, int level, std::vector<HeapItem>& heap,
             size_t k) {
    if (level == t.levels) {
        const typename KD::Point* lp = t.pts.data() + (size_t)(node - level_offset(level)) * LEAF_CAP;
        for (int j = 0; j < LEAF_CAP; ++j) {
            if (lp[j].idx == 0x7fffffff || (int64_t)lp[j].idx == self) continue;
            double d = 0.0;
            for (int a = 0; a < KD::DIM; ++a) { double x = q[a] - (double)lp[j].c[a]; d += x * x; }
            HeapItem it{d, (int64_t)lp[j].idx};
            if (heap.size() < k) {
                heap.push_back(it);
                std::push_heap(heap.begin(), heap.end(), heap_less);
            } else if (heap_less(it, heap.front())) {
                std::pop_heap(heap.begin(), heap.end(), heap_less);
                heap.back() = it;
                std::push_heap(heap.begin(), heap.end(), heap_less);
            }
        }
        return;
    }
    std::pair<double, int> order[8];
    for (int j = 0; j < 8; ++j) order[j] = {host_box_d2<KD>(q, t.boxes[8 * node + 1 + j]), j};
    std::sort(order, order + 8);
    for (int j = 0; j < 8; ++j)
        if (heap.size() < k || order[j].first <= heap.front().d)
            knn_rec<KD>(t, q, self, 8 * node + 1 + order[j].second, level + 1, heap, k);
}

template <class F>
void parallel_for(int64_t n, F&& work) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > 32 ? 32 : nt);
    if (n < 4096) nt = 1;
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nt; ++i) th.emplace_back(work, n * i / nt, n * (i + 1) / nt);
    for (auto& x : th) x.join();
}

inline float round_down_f32(double v) {
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, 0.0f);
    return f;
}
}  // namespace

static void build_neighbour_graph(HostTree<Kd6>& t, const float* P, int64_t K) {
    t.nbrs.resize((size_t)K * NBR_REC);
    t.rho_out.resize(K);
    t.twin.resize(K);
    parallel_for(K, [&](int64_t k0, int64_t k1) {
        std::vector<HeapItem> heap;
        for (int64_t k = k0; k < k1; ++k) {
            heap.clear();
            double q[6];
            for (int a = 0; a < 6; ++a) q[a] = (double)P[k * 6 + a];
            knn_rec<Kd6>(t, q, k, 0, 0, heap, (size_t)NBR_M + 1);
            std::sort(heap.begin(), heap.end(), heap_less);
            {   // record 0 = the entry itself (rho 0): the scan needs no other lookup
                Nbr6 r;
                for (int a = 0; a < 6; ++a) r.c[a] = P[k * 6 + a];
                r.idx = (int32_t)k;
                r.rho = 0.0f;
                t.nbrs[(size_t)k * NBR_REC] = r;
            }
            for (int s2 = 0; s2 < NBR_M; ++s2) {
                Nbr6 r;
                if ((size_t)s2 < heap.size()) {
                    const int64_t j = heap[s2].idx;
                    for (int a = 0; a < 6; ++a) r.c[a] = P[j * 6 + a];
                    r.idx = (int32_t)j;
                    r.rho = round_down_f32(std::sqrt(heap[s2].d));
                } else {
                    for (int a = 0; a < 6; ++a) r.c[a] = INFINITY;
                    r.idx = 0x7fffffff;
                    r.rho = INFINITY;
                }
                t.nbrs[(size_t)k * NBR_REC + 1 + s2] = r;
            }
            t.rho_out[k] = heap.size() > (size_t)NBR_M ? round_down_f32(std::sqrt(heap[NBR_M].d)) : INFINITY;
            // twin across the rotation-angle-pi cut: the feature's rotation part is w = 0.01 log(R); a pose whose
            // angle crosses pi reappears at w - 2 pi 0.01 w/|w|.  The entry nearest to that image is the right
            // second hint for a particle whose own feature has just flipped.
            const double wn = std::sqrt(q[3] * q[3] + q[4] * q[4] + q[5] * q[5]);
            t.twin[k] = -1;
            if (wn > 0.01 * (M_PI - 0.6)) {
                double qf[6] = {q[0], q[1], q[2], 0, 0, 0};
                const double sc = (wn - 0.01 * 2.0 * M_PI) / wn;
                for (int a = 3; a < 6; ++a) qf[a] = q[a] * sc;
                heap.clear();
                knn_rec<Kd6>(t, qf, -1, 0, 0, heap, 1);
                if (!heap.empty() && heap[0].idx != k) t.twin[k] = (int32_t)heap[0].idx;
            }
        }
    });
}

// ---- mesh-vertex lists anchored at the codebook entries (prune fast path) --------------------------
// For entry k: the MESH_M mesh vertices nearest to its translation t_k, sorted by rho = |v - t_k|
// (rounded down), and rho_out = distance of the next vertex.  A particle whose NN entry is k can only be
// within thr of a vertex v if rho_v <= thr + |t_q - t_k|, so scanning the list in order decides the prune
// exactly unless the list runs out first.
int attach_mesh_impl(midas_ctx* ctx, midas_tree* t6, const midas_tree* t3, const float* cb_poses_dev) {
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (!index_build_on_host()) return build_vertex_lists_device(ctx, t6, t3, cb_poses_dev);
    const HostTree<Kd3>* mesh = reinterpret_cast<const HostTree<Kd3>*>(t3->host);
    if (!mesh) return midas_set_error(ctx, MIDAS_ERR_INVALID, "attach_mesh", "mesh tree has no host copy");
    const int64_t K = t6->K;
    std::vector<float> poses((size_t)K * 16);
    MIDAS_HIP_CHECK(ctx, hipMemcpy(poses.data(), cb_poses_dev, poses.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<MeshRec> recs((size_t)K * MESH_REC);
    parallel_for(K, [&](int64_t k0, int64_t k1) {
        std::vector<HeapItem> heap;
        for (int64_t k = k0; k < k1; ++k) {
            heap.clear();
            const double q[3] = {(double)poses[k * 16 + 3], (double)poses[k * 16 + 7], (double)poses[k * 16 + 11]};
            knn_rec<Kd3>(*mesh, q, -1, 0, 0, heap, (size_t)MESH_M + 1);
            std::sort(heap.begin(), heap.end(), heap_less);
            for (int s2 = 0; s2 < MESH_M; ++s2) {
                MeshRec r;
                if ((size_t)s2 < heap.size()) {
                    const typename Kd3::Point& p = mesh->pts[mesh->inv_perm[heap[s2].idx]];
                    r.c[0] = p.c[0]; r.c[1] = p.c[1]; r.c[2] = p.c[2];
                    r.rho = round_down_f32(std::sqrt(heap[s2].d));
                } else {
                    r.c[0] = r.c[1] = r.c[2] = INFINITY;
                    r.rho = INFINITY;
                }
                r.pad = 0;
                recs[(size_t)k * MESH_REC + 1 + s2] = r;
            }
            MeshRec hd;
            hd.c[0] = q[0]; hd.c[1] = q[1]; hd.c[2] = q[2];
            hd.rho = heap.size() > (size_t)MESH_M ? round_down_f32(std::sqrt(heap[MESH_M].d)) : INFINITY;
            hd.pad = 0;
            recs[(size_t)k * MESH_REC] = hd;
        }
    });
    if (t6->vlist) { (void)hipFree(t6->vlist); t6->vlist = nullptr; }
    MIDAS_HIP_CHECK(ctx, hipMalloc(&t6->vlist, recs.size() * sizeof(MeshRec)));
    MIDAS_HIP_CHECK(ctx, hipMemcpy(t6->vlist, recs.data(), recs.size() * sizeof(MeshRec), hipMemcpyHostToDevice));
    t6->vlist_mesh = t3;
    return build_vertex_screen(ctx, t6);
}

template <class KD>
static int upload_tree(midas_ctx* ctx, const HostTree<KD>& h, int64_t K, midas_tree* out) {
    auto up = [&](const void* src, size_t bytes, void** dst) -> int {
        MIDAS_HIP_CHECK(ctx, hipMalloc(dst, bytes ? bytes : 16));
        if (bytes) MIDAS_HIP_CHECK(ctx, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return MIDAS_OK;
    };
    int rc;
    if ((rc = up(h.boxes.data(), h.boxes.size() * sizeof(typename KD::Box), &out->boxes))) return rc;
    if ((rc = up(h.pts.data(), h.pts.size() * sizeof(typename KD::Point), &out->pts))) return rc;
    if ((rc = up(h.inv_perm.data(), h.inv_perm.size() * sizeof(int32_t), (void**)&out->inv_perm))) return rc;
    if (!h.nbrs.empty()) {
        if ((rc = up(h.nbrs.data(), h.nbrs.size() * sizeof(Nbr6), &out->nbrs))) return rc;
        if ((rc = up(h.rho_out.data(), h.rho_out.size() * sizeof(float), (void**)&out->rho_out))) return rc;
        if ((rc = up(h.twin.data(), h.twin.size() * sizeof(int32_t), (void**)&out->twin))) return rc;
    }
    out->levels = h.levels;
    out->K = K;
    return MIDAS_OK;
}

// The distance field of a dim-3 tree's vertices (MeshField): the bounding box grown by FIELD_EXPAND, cubic cells sized so that the
// grid has at most FIELD_MAX_CELLS of them, every cell's value by the exact search (k_field_build).  MIDAS_MESH_FIELD=0: none.
constexpr double FIELD_EXPAND = 0.0025;            // m: decides "outside the grid = pruned" for thresholds below it (the reference's is 0.002)
constexpr double FIELD_MIN_CELL = 2.5e-5;          // m: cells no finer than this (shell half-width < 0.022 mm)
constexpr int64_t FIELD_MAX_CELLS = (int64_t)1 << 26;  // 256 MB of float32 (c4's mug: 0.23 mm cells; with 2^22 cells of 0.59 mm the undecided shell held 1700 particles a frame)
static int build_mesh_field(midas_ctx* ctx, midas_tree* t, const double* pts, int64_t K);

int tree_build_impl(midas_ctx* ctx, int32_t dim, int64_t K, const void* points_dev, midas_tree* out) {
    MIDAS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (dim == 6) {
        std::vector<float> host((size_t)K * 6);
        MIDAS_HIP_CHECK(ctx, hipMemcpy(host.data(), points_dev, host.size() * sizeof(float), hipMemcpyDeviceToHost));
        HostTree<Kd6> h = build_tree<Kd6>(host.data(), K);
        if (index_build_on_host()) {
            build_neighbour_graph(h, host.data(), K);
            return upload_tree<Kd6>(ctx, h, K, out);
        }
        // the box tree (K log K) on the host, the neighbour graph (K x K) on the device (index_build.hip)
        int rc = upload_tree<Kd6>(ctx, h, K, out);
        if (rc) return rc;
        return build_neighbour_graph_device(ctx, out);
    }
    std::vector<double> host((size_t)K * 3);
    MIDAS_HIP_CHECK(ctx, hipMemcpy(host.data(), points_dev, host.size() * sizeof(double), hipMemcpyDeviceToHost));
    HostTree<Kd3>* h = new HostTree<Kd3>(build_tree<Kd3>(host.data(), K));
    out->host = h;  // kept for attach_mesh (host k-NN over the mesh vertices)
    int rc = upload_tree<Kd3>(ctx, *h, K, out);
    if (rc) return rc;
    return build_mesh_field(ctx, out, host.data(), K);
}

void tree_free_host(midas_tree* t) {
    if (t->host) {
        if (t->dim == 3) delete reinterpret_cast<HostTree<Kd3>*>(t->host);
        t->host = nullptr;
    }
}

__global__ __launch_bounds__(64) void k_nn6(TreeView<Kd6> tv, int64_t N, const float* __restrict__ feat,
                                            const int32_t* __restrict__ hint, int32_t* __restrict__ idx,
                                            float* __restrict__ d2out) {
    __shared__ float s_cd[KD_MAX_LEVELS * 64];
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = n < N;
    float q[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
        for (int j = 0; j < 6; ++j) q[j] = feat[n * 6 + j];
    }
    int32_t bi;
    float bd;
    nn6_wave(tv, q, live, (live && hint) ? hint[n] : -1, bi, bd, s_cd);
    if (live) {
        idx[n] = bi;
        if (d2out) d2out[n] = bd;
    }
}

// diagnostic twin: per query, leaves / nodes visited by the octet search (0 / -(1 + records scanned) when the
// hint scan certified the answer)
__global__ __launch_bounds__(64) void k_nn6_stats(TreeView<Kd6> tv, int64_t N, const float* __restrict__ feat,
                                                  const int32_t* __restrict__ hint, int32_t* __restrict__ leaves,
                                                  int32_t* __restrict__ nodes) {
    __shared__ float s_cd[KD_MAX_LEVELS * 64];
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = n < N;
    float q[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
        for (int j = 0; j < 6; ++j) q[j] = feat[n * 6 + j];
    }
    int32_t bi;
    float bd;
    int nl = 0, nn = 0, ns = -1;
    nn6_wave<true>(tv, q, live, (live && hint) ? hint[n] : -1, bi, bd, s_cd, &nl, &nn, &ns);
    if (live) {
        leaves[n] = nl;
        nodes[n] = (nl == 0 && nn == 0 && ns >= 0) ? -(ns + 1) : nn;
    }
}

// builder: exact distance (float64 search of the 3-d tree, as k_nn3) from every cell centre of a slab of the grid
__global__ __launch_bounds__(64) void k_field_build(TreeView<Kd3> tv, MeshField f, int64_t c0, int64_t ncells, float* __restrict__ out) {
    __shared__ double s_cd[KD_MAX_LEVELS * 64];
    const int64_t n = c0 + (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = n < ncells;
    double q[3] = {0.0, 0.0, 0.0};
    if (live) {
        const int ix = (int)(n % f.n[0]), iy = (int)((n / f.n[0]) % f.n[1]), iz = (int)(n / ((int64_t)f.n[0] * f.n[1]));
        q[0] = (double)field_centre(f, 0, ix); q[1] = (double)field_centre(f, 1, iy); q[2] = (double)field_centre(f, 2, iz);
    }
    double best = INFINITY;
    int64_t bi = 0;
    wave_search<Kd3, false>(tv, q, best, bi, live, s_cd);
    if (live) out[n] = (float)__builtin_sqrt(best);
}

__global__ __launch_bounds__(64) void k_nn3(TreeView<Kd3> tv, int64_t N, const float* __restrict__ poses,
                                            double* __restrict__ dist) {
    __shared__ double s_cd[KD_MAX_LEVELS * 64];
    const int64_t n = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool live = n < N;
    double q[3] = {0.0, 0.0, 0.0};
    if (live) { q[0] = (double)poses[n * 16 + 3]; q[1] = (double)poses[n * 16 + 7]; q[2] = (double)poses[n * 16 + 11]; }
    double best = INFINITY;
    int64_t bi = 0;
    wave_search<Kd3, false>(tv, q, best, bi, live, s_cd);
    if (live) dist[n] = __builtin_sqrt(best);
}

int launch_nn6(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* feat6, const int32_t* hint, int32_t* idx,
               float* d2) {
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_nn6, dim3((unsigned)ceil_div(N, 64)), dim3(64), 0, ctx->stream, view_of<Kd6>(t), N, feat6, hint,
                       idx, d2);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

// ---- exact k nearest codebook entries (tactile_tree.py:43-58 with n_neighbors > 1) --------------------------------------
// One wave per query, brute force over the tree's leaf slots (empty slots carry +inf coordinates): every lane keeps the k
// best of the slots it visits in its own LDS column, sorted by (distance, index); the wave then merges the 64 columns,
// taking the smallest head k times.  Distances are the spec's dist2 chain, ties go to the smaller index, so column 0 of
// the result is what midas_nn6 returns.  Not on the filter's path (it uses nn = 1): a query costs one pass over the codebook.
__global__ __launch_bounds__(64) void k_knn6(TreeView<Kd6> tv, int64_t N, const float* __restrict__ feat, int k,
                                            int32_t* __restrict__ idx_out, float* __restrict__ d2_out) {
    extern __shared__ unsigned char s_knn[];
    float* s_d = reinterpret_cast<float*>(s_knn);
    int* s_i = reinterpret_cast<int*>(s_d + (size_t)k * 64);
    const int lane = threadIdx.x & 63;
    const int64_t n = blockIdx.x;
    float q[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) q[a] = feat[n * 6 + a];
    for (int s = 0; s < k; ++s) { s_d[s * 64 + lane] = INFINITY; s_i[s * 64 + lane] = 0x7fffffff; }
    const int64_t nslots = ((int64_t)LEAF_CAP) << (3 * tv.levels);
    float worst_d = INFINITY;
    int worst_i = 0x7fffffff;
    for (int64_t slot = lane; slot < nslots; slot += 64) {
        const Point6 p = tv.pts[slot];
        const float d = dist2(q, p);
        const int id = p.idx;
        if (d < worst_d || (d == worst_d && id < worst_i)) {  // NaN never enters
            int pos = k - 1;
            while (pos > 0) {
                const float pd = s_d[(pos - 1) * 64 + lane];
                const int pi = s_i[(pos - 1) * 64 + lane];
                if (pd < d || (pd == d && pi < id)) break;
                s_d[pos * 64 + lane] = pd;
                s_i[pos * 64 + lane] = pi;
                --pos;
            }
            s_d[pos * 64 + lane] = d;
            s_i[pos * 64 + lane] = id;
            worst_d = s_d[(k - 1) * 64 + lane];
            worst_i = s_i[(k - 1) * 64 + lane];
        }
    }
    int ptr = 0;
    for (int r = 0; r < k; ++r) {
        const float hd = ptr < k ? s_d[ptr * 64 + lane] : INFINITY;
        const int hi = ptr < k ? s_i[ptr * 64 + lane] : 0x7fffffff;
        float bd = hd;
        int bi = hi;
        wave_best(bd, bi);
        if (lane == 0) {
            idx_out[n * k + r] = bi;
            if (d2_out) d2_out[n * k + r] = bd;
        }
        if (hi == bi && bi != 0x7fffffff) ++ptr;  // an entry sits in exactly one column
    }
}

int launch_knn6(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* feat6, int32_t k, int32_t* idx, float* d2) {
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_knn6, dim3((unsigned)N), dim3(64), (size_t)k * 64 * 8, ctx->stream, view_of<Kd6>(t), N, feat6, (int)k,
                       idx, d2);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

int launch_nn6_stats(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* feat6, const int32_t* hint,
                     int32_t* leaves, int32_t* nodes) {
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_nn6_stats, dim3((unsigned)ceil_div(N, 64)), dim3(64), 0, ctx->stream, view_of<Kd6>(t), N, feat6,
                       hint, leaves, nodes);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

static int build_mesh_field(midas_ctx* ctx, midas_tree* t, const double* pts, int64_t K) {
    const char* env = getenv("MIDAS_MESH_FIELD");
    if ((env && env[0] == '0') || K <= 0) return MIDAS_OK;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t k = 0; k < K; ++k)
        for (int d = 0; d < 3; ++d) {
            const double v = pts[3 * k + d];
            if (!(v == v) || std::isinf(v)) return MIDAS_OK;  // non-finite vertices: no field (the exact paths deal with them as before)
            lo[d] = v < lo[d] ? v : lo[d];
            hi[d] = v > hi[d] ? v : hi[d];
        }
    double ext[3], vol = 1.0;
    for (int d = 0; d < 3; ++d) { ext[d] = (hi[d] - lo[d]) + 2.0 * FIELD_EXPAND * 1.01; vol *= ext[d]; }
    double h = std::cbrt(vol / (double)FIELD_MAX_CELLS);
    if (h < FIELD_MIN_CELL) h = FIELD_MIN_CELL;  // (a small mesh does not need the whole budget: the shell is thin enough)
    MeshField f;
    for (int iter = 0; iter < 8; ++iter) {  // (rounding the counts up can exceed the budget: grow the cells a little)
        int64_t cells = 1;
        for (int d = 0; d < 3; ++d) { f.n[d] = (int32_t)std::ceil(ext[d] / h) + 1; cells *= f.n[d]; }
        if (cells <= FIELD_MAX_CELLS) break;
        h *= 1.03;
    }
    f.h = (float)h;
    f.inv_h = 1.0f / f.h;
    // the grid's corner: at or below lo - 1.01 expand as a float32 (a point "outside" must really be beyond the grown box)
    for (int d = 0; d < 3; ++d) f.lo[d] = std::nextafter((float)(lo[d] - FIELD_EXPAND * 1.01), -INFINITY);
    // ... and the far faces: n cells of f.h must reach hi + expand (the counts were taken with the double h: check with the float)
    for (int d = 0; d < 3; ++d)
        while ((double)f.lo[d] + (double)f.n[d] * (double)f.h < hi[d] + FIELD_EXPAND * 1.005) ++f.n[d];
    f.expand = (float)FIELD_EXPAND;
    const int64_t cells = (int64_t)f.n[0] * f.n[1] * f.n[2];
    float* dev = nullptr;
    if (hipMalloc((void**)&dev, (size_t)cells * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return MIDAS_OK; }  // no memory: no field
    f.d = dev;
    const TreeView<Kd3> tv = view_of<Kd3>(t);
    const int64_t SLAB = (int64_t)1 << 24;  // cells per launch
    for (int64_t c0 = 0; c0 < cells; c0 += SLAB) {
        const int64_t n = cells - c0 < SLAB ? cells - c0 : SLAB;
        hipLaunchKernelGGL(k_field_build, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, ctx->stream, tv, f, c0, cells, dev);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(dev);
        return midas_set_error(ctx, MIDAS_ERR_HIP, "k_field_build", "building the mesh's distance field failed");
    }
    t->field = f;
    return MIDAS_OK;
}

int launch_nn3(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* poses, double* dist) {
    if (N == 0) return MIDAS_OK;
    hipLaunchKernelGGL(k_nn3, dim3((unsigned)ceil_div(N, 64)), dim3(64), 0, ctx->stream, view_of<Kd3>(t), N, poses, dist);
    MIDAS_HIP_CHECK(ctx, hipGetLastError());
    return MIDAS_OK;
}

MIDAS_WARM_TU(tree, k_nn6)

}  // namespace midas
