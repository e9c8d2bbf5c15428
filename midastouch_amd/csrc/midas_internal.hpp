// midas_internal.hpp - shared declarations of the libmidas_hip.so translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/midas_hip.h"

namespace midas {

// ---- spatial index layouts (shared host/device) ------------------------------------------------
// Complete 8-ary tree of axis-aligned boxes in 0-based heap order: node n has children 8n+1 .. 8n+8,
// level l starts at id (8^l - 1)/7; the 8^L nodes of level L are leaves.  Every node stores the box of
// its points, so the eight child boxes of a node are 384 contiguous bytes (one 48-byte box per lane of
// an octet).  Leaf i owns the LEAF_CAP fixed point slots pts[i*LEAF_CAP ..); unused slots hold +inf
// coordinates.  Built from balanced median splits (three binary splits per 8-ary level).
struct alignas(16) Box6 { float lo[6], hi[6]; };
struct alignas(16) Point6 { float c[6]; int32_t idx; int32_t pad; };
struct alignas(16) Box3 { double lo[3], hi[3]; };
struct alignas(16) Point3 { double c[3]; int64_t idx; };

struct Kd6 {
    using T = float;
    using Box = Box6;
    using Point = Point6;
    static constexpr int DIM = 6;
};
struct Kd3 {
    using T = double;
    using Box = Box3;
    using Point = Point3;
    static constexpr int DIM = 3;
};

constexpr int LEAF_CAP = 16;      // point slots per leaf (two per lane of an octet)
constexpr int KD_MAX_LEVELS = 10; // 8-ary levels (8^10 leaves x 16 slots is far beyond any codebook)

// Neighbour record of the hint fast path (dim 6 only): entry k owns NBR_M records sorted by the
// distance rho from F_k to that neighbour (rounded down), coordinates inlined so that one 32-byte
// read is one candidate.  Unused records are sentinels (+inf coordinates, rho = +inf).
struct alignas(16) Nbr6 { float c[6]; int32_t idx; float rho; };
#ifndef MIDAS_NBR_M
#define MIDAS_NBR_M 512
#endif
constexpr int NBR_M = MIDAS_NBR_M;
constexpr int NBR_REC = NBR_M + 1;  // record 0 = the entry itself

// Mesh-vertex record of the prune fast path: the vertices nearest to a codebook entry's translation.
struct alignas(16) MeshRec { double c[3]; float rho; int32_t pad; };
// float32 screening copy of a MeshRec (vertex rounded to nearest; the header's translation is a float32 value already):
// half the bytes and float32 arithmetic for the decisions that are not within rounding of the threshold (mesh_screen_check)
struct alignas(16) MeshScr { float c[3]; float rho; };
constexpr int MESH_M = 256;
constexpr int MESH_REC = MESH_M + 1;  // record 0 = header: c = the entry's translation, rho = distance of the
                                      // first vertex NOT in the list

// Distance field of a mesh (dim-3 trees): the exact distance from the CENTRE of every cell of a uniform grid to its nearest mesh
// vertex, as float32.  The distance to the nearest vertex is 1-Lipschitz, so a particle at distance rho from its cell's centre has
// d in [v - rho, v + rho]: the prune ("some vertex within thr", modules/particle_filter.py:386-391) is DECIDED for every particle
// outside a shell of half-width rho (< 0.87 cells) around the threshold surface - by one 4-byte read requested before the
// nearest-neighbour search - and only the shell goes on to the vertex lists / the tree, which remain the exact decision.
// A point outside the grid (the vertices' bounding box grown by `expand`) is farther than `expand` from every vertex.
struct MeshField {
    const float* d = nullptr;  // [n[2]][n[1]][n[0]]
    float lo[3] = {0.f, 0.f, 0.f};
    float h = 0.f, inv_h = 0.f;
    int32_t n[3] = {0, 0, 0};
    float expand = 0.f;
};

template <class KD>
struct TreeView {
    const typename KD::Box* boxes;  // [(8^(L+1) - 1)/7]
    const typename KD::Point* pts;  // [8^L * LEAF_CAP]
    const int32_t* inv_perm;        // [K] original index -> slot in pts
    const Nbr6* nbrs;               // [K * NBR_REC] (dim 6) or nullptr
    const float* rho_out;           // [K] distance from F_k to its (NBR_M+1)-th neighbour, rounded down
    const int32_t* twin;            // [K] entry across the |log R| = pi cut (or -1) - second hint of the scan
    int32_t levels;                 // L: number of 8-ary levels above the leaves
    int64_t K;
};


}  // namespace midas

// ---- opaque handles ---------------------------------------------------------------------------
struct midas_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // growable scratch
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    std::string last_error;
    // profiling
    bool prof = false;
    int prof_only = -1;
    hipEvent_t ev[MIDAS_PROF_SLOTS + 1] = {};
    bool ev_ready = false;
    double prof_ms[MIDAS_PROF_SLOTS] = {};
    int64_t prof_calls = 0;
    bool overlap = true;  // MIDAS_OVERLAP=0: separate scoring and particle-update launches (the pre-fusion path)
    // side stream of the batch step: the matrix-core scoring of the B codes runs there, concurrently with the particle
    // update (created on first use, non-blocking, forked from / joined into `stream` by the two events)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // hand-over records of the grouped tail (tail_group.hpp): [tail_rec_blocks x TG_BLOCK_WORDS] words, zeroed at allocation
    // (midas_ctx_create); tail_tag numbers its launches (a record is current when its pairs carry the launch's key)
    unsigned long long* tail_rec = nullptr;
    int tail_rec_blocks = 0;
    uint32_t tail_tag = 0;
};

struct midas_codebook {
    midas_ctx* ctx;
    int64_t K;
    int32_t D;
    int32_t dtype;
    const void* emb;  // caller-owned
    double* norms;    // [K] max(|C_k|, 1e-8), library-owned
    int32_t batch_precision = MIDAS_F32;  // the dense batch pass of midas_filter_step_batch: MIDAS_F32 k_score_mfma, MIDAS_F64 k_score_mfma_f64
};

struct midas_tree {
    midas_ctx* ctx;
    int32_t dim;
    int64_t K;
    int32_t levels;
    void* boxes;
    void* pts;
    int32_t* inv_perm;
    void* nbrs;      // Nbr6[K * NBR_REC] (dim 6)
    float* rho_out;  // [K] (dim 6)
    int32_t* twin;   // [K] (dim 6)
    void* vlist;     // MeshRec[K * MESH_REC] (dim 6, after midas_tree_attach_mesh)
    void* vscr;      // MeshScr[K * MESH_REC]: float32 screening copy of vlist (nullable)
    const midas_tree* vlist_mesh;  // the mesh tree the lists were built from
    void* host;      // host copy of the tree (dim 3: used to build the lists)
    midas::MeshField field;  // dim 3: distance field of the vertices (d == nullptr: none); library-owned
};

// One object of a midas_object_set as the front of a batch frame reads it (k_front_small_objects): everything
// launch_front_small_batch and fill_particle_update take from the codebook and the two tree handles, and the poses the drift
// re-projection gathers from.  Lives in device memory; a workgroup reads its row's record through a uniform address.
namespace midas {
struct ObjectRecord {
    TreeView<Kd6> t6;
    TreeView<Kd3> t3;
    const MeshRec* vlist;   // nullable, as ParticleUpdateArgs::vlist
    const MeshScr* vscr;
    MeshField field;
    const float* emb;
    const double* norms;
    int64_t K;
    const float* cb_poses;  // [K x 16]
};
}  // namespace midas

struct midas_object_set {
    midas_ctx* ctx;
    int32_t n_obj, B, D;
    int64_t K_max;
    void* dev;                           // one allocation: the records, the poses table, the row map
    const midas::ObjectRecord* recs;     // [n_obj]
    const float* const* cb_poses_rows;   // [B] row b's codebook poses
    const int32_t* row_object;           // [B]
    const float* cb_poses_row0;          // (host copy of cb_poses_rows[0])
};

// ---- error helpers ----------------------------------------------------------------------------
int midas_set_error(midas_ctx* ctx, int code, const char* what, const char* detail);

#define MIDAS_HIP_CHECK(ctx, expr)                                                     \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) return midas_set_error((ctx), MIDAS_ERR_HIP, #expr, hipGetErrorString(_e)); \
    } while (0)

#define LAUNCH_CHECK(ctx) MIDAS_HIP_CHECK(ctx, hipGetLastError())

#define MIDAS_REQUIRE(ctx, cond)                                                       \
    do {                                                                               \
        if (!(cond)) return midas_set_error((ctx), MIDAS_ERR_INVALID, #cond, "invalid argument"); \
    } while (0)

// Code objects load lazily, per translation unit, at the first launch of one of its kernels (tens of ms for the large ones, in
// the middle of whatever frame happens to be the first to need them: the "cold frame" of a run).  Every unit exports a function
// that makes the runtime load it now - hipFuncGetAttributes resolves a kernel without launching it - and midas_ctx_create calls
// them all (MIDAS_LAZY_MODULES=1 keeps the lazy behaviour).
#define MIDAS_WARM_TU(name, kernel)                                                          \
    int warm_##name() {                                                                      \
        hipFuncAttributes attr;                                                              \
        return (int)hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(&kernel));     \
    }
#define MIDAS_WARM_DECL(name) int warm_##name();
// (warm_particles also loads the units cut out of particles.hip - tree, front, front_folded, front_batch -, warm_resample those
// cut out of resample.hip - tail, shard_route - and warm_loop the phases of a loop frame - loop_weights, anneal, anneal_small,
// loop_resample: their warm functions are declared and chained in particles.hip, resample.hip and loop.hip, so midas_ctx_create's
// list of units stays as it is)
namespace midas {
MIDAS_WARM_DECL(score) MIDAS_WARM_DECL(particles) MIDAS_WARM_DECL(resample) MIDAS_WARM_DECL(cluster) MIDAS_WARM_DECL(topn)
MIDAS_WARM_DECL(selfsim) MIDAS_WARM_DECL(loop) MIDAS_WARM_DECL(dbscan) MIDAS_WARM_DECL(dbscan_nd) MIDAS_WARM_DECL(index_build)
MIDAS_WARM_DECL(mt19937) MIDAS_WARM_DECL(topk_aten) MIDAS_WARM_DECL(score_f64) MIDAS_WARM_DECL(selfsim_f64)
MIDAS_WARM_DECL(tsne)
}  // namespace midas

// scratch carve-out (stream-ordered reuse; one stream per context)
int midas_scratch(midas_ctx* ctx, size_t bytes, void** out);
// where the carve-out stands / back to there: passes that follow each other on the stream take the same bytes (the DBSCAN passes of
// midas_loop_step_batch share one set of cell tables)
struct midas_scratch_pos { size_t cur, used, total; };
midas_scratch_pos midas_scratch_mark(midas_ctx* ctx);
void midas_scratch_rewind(midas_ctx* ctx, const midas_scratch_pos& pos);

namespace midas {

// control block of the loop engine (midas_loop_args.ctl_i_dev / ctl_d_dev; include/midas_hip.h MIDAS_LOOP_*)
enum : int {
    LOOP_I_N = MIDAS_LOOP_I_N, LOOP_I_NSET = MIDAS_LOOP_I_NSET, LOOP_I_MODE = MIDAS_LOOP_I_MODE, LOOP_I_K = MIDAS_LOOP_I_K,
    LOOP_I_INIT = MIDAS_LOOP_I_INIT, LOOP_I_VARSET = MIDAS_LOOP_I_VARSET, LOOP_I_KEPT = MIDAS_LOOP_I_KEPT,
    LOOP_I_DRIFT = MIDAS_LOOP_I_DRIFT, LOOP_I_STATUS = MIDAS_LOOP_I_STATUS, LOOP_I_RAW = MIDAS_LOOP_I_RAW,
    LOOP_I_NCL = MIDAS_LOOP_I_NCL, LOOP_I_NPRES = MIDAS_LOOP_I_NPRES, LOOP_I_FRAME = MIDAS_LOOP_I_FRAME,
    LOOP_I_NAN = MIDAS_LOOP_I_NAN, LOOP_I_ERR = MIDAS_LOOP_I_ERR, LOOP_I_NDRAW = MIDAS_LOOP_I_NDRAW,
    LOOP_D_S = MIDAS_LOOP_D_S, LOOP_D_VARPREV = MIDAS_LOOP_D_VARPREV, LOOP_D_VAR = MIDAS_LOOP_D_VAR,
    LOOP_D_RMSE_T = MIDAS_LOOP_D_RMSE_T, LOOP_D_RMSE_R = MIDAS_LOOP_D_RMSE_R, LOOP_D_XMAX = MIDAS_LOOP_D_XMAX,
    LOOP_D_XMIN = MIDAS_LOOP_D_XMIN, LOOP_D_TOTAL = MIDAS_LOOP_D_TOTAL,
    LOOP_MAX_CLUSTERS = MIDAS_LOOP_MAX_CLUSTERS,
    LOOP_CTL_I = 32, LOOP_CTL_D = 16,  // entries of one trajectory's control blocks (midas_loop_step_batch: (B, 32) / (B, 16))
};

// blocked-scan spec constants (DESIGN.md "Summation order")
constexpr int SCAN_CHUNK = 16;
constexpr int SCAN_TPB = 256;
constexpr int SCAN_BLOCK = SCAN_CHUNK * SCAN_TPB;  // 4096 values per block
// Guide table of a summation block (single-trajectory pipelined step, optional): GUIDE_BINS equal bins over the block's masked
// total W, edge k at fl(k * (W / GUIDE_BINS)) (a power of two: the bin width is exact).  The block's slots are taken in units of
// GUIDE_UNIT (16: the chunks of the summation spec; 8 / 4: halves / quarters of them); entry k = min(number of the block's unit
// ends < edge k, units of the block - 1), entry GUIDE_BINS = units of the block - 1.  A draw whose block-local target lies in
// bin k finds its slot in unit entry[k] .. entry[k + 1]: one entry pair and GUIDE_UNIT (or twice that) prefix values instead of
// the group-end, chunk-end and slot lines of search_in_block (a hint: the exact fix-up behind it decides).
#ifndef MIDAS_GUIDE_BINS
#define MIDAS_GUIDE_BINS 2048
#endif
#ifndef MIDAS_GUIDE_UNIT
#define MIDAS_GUIDE_UNIT 8
#endif
typedef uint16_t guide_t;
constexpr int GUIDE_BINS = MIDAS_GUIDE_BINS, GUIDE_STRIDE = GUIDE_BINS + 16, GUIDE_UNIT = MIDAS_GUIDE_UNIT;  // (stride in entries)
constexpr double GUIDE_WIDTH = 1.0 / GUIDE_BINS;
constexpr int TAIL_GUIDE_LDS = GUIDE_BINS / 2 + 8;  // 32-bit words of LDS the tail's guide pass takes: the edge histogram (16-bit counters) + 4 wave totals
static_assert((GUIDE_BINS & (GUIDE_BINS - 1)) == 0 && GUIDE_BINS >= 2048, "bins: a power of two, eight or more per chunk");
static_assert(GUIDE_UNIT == 16 || GUIDE_UNIT == 8 || GUIDE_UNIT == 4, "units: whole chunks, halves or quarters");

// grouped tail (tail_group.hpp): one wave per 256-slot group while the whole grid is resident - up to this many 4096-slot blocks
// (128 four-wave workgroups a 32 blocks: 512 workgroups on 256 CUs); larger sets keep one workgroup per block (they fill the chip)
constexpr int TAIL_GROUP_MAX_BLOCKS = 128;
constexpr size_t TAIL_GROUP_BLOCK_BYTES = 2 * 16 * 16 * 8;  // TG_ROUNDS x 16 groups x one 128-byte record

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- launchers (each enqueues on ctx->stream and returns a status) --------------------------------
// score.hip
int launch_row_norms(midas_ctx* ctx, int64_t K, int32_t D, const void* emb, int32_t dtype, double* norms);
int launch_score(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores);
int launch_score_batch(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores);
int launch_score_batch_f64(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores);
int launch_score_dense_batch(midas_ctx* ctx, const midas_codebook* cb, int32_t B, const double* codes, double* scores);

// particles.hip (launch_nn6, launch_nn3, launch_nn6_stats, launch_knn6: tree.hip)
int launch_se3_feature(midas_ctx* ctx, int64_t N, const float* poses, float w, float* feat6);
int launch_propagate(midas_ctx* ctx, int64_t N, const float* in, float* out, const float* odom,
                     const float* tn, const float* rot, float std_t, float std_r, uint64_t seed, uint64_t step);
int launch_check_poses(midas_ctx* ctx, int64_t N, const float* poses, uint8_t* flag, int32_t* count);
int launch_nn6(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* feat6, const int32_t* hint,
               int32_t* idx, float* d2);
int launch_nn3(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* poses, double* dist);
int launch_nn6_stats(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* feat6, const int32_t* hint,
                     int32_t* leaves, int32_t* nodes);
int launch_rmse(midas_ctx* ctx, int64_t N, const float* poses, const float* gt16, double* out2);
// Resample of the PREVIOUS frame folded into the front kernel (k_frame_front): slot n of this frame is particle
// src(n) of the previous one - a per-slot dependence - so the search and the gather of the resampler run as a
// prologue of the particle update and the resampled poses never travel through HBM.  The tables are the ones
// k_tail_a2 wrote for the previous frame; src is exactly what k_tail_b2 computes (same predicates).
constexpr int LAZY_MAX_BLOCKS = 256;  // 1 M particles
struct LazyResample {
    bool enabled = false;
    const double *e, *x_raw, *lp, *lp_raw, *gend, *gend_raw;       // [N] x4, [ng] x2
    const double *ggend, *ggend_raw;                                // [16 nb] x2
    const guide_t *guide = nullptr, *guide_raw = nullptr;           // nullable [nb x GUIDE_STRIDE] x2 (see GUIDE_BINS)
    const double *bsum_e, *btot, *btot_raw, *bmax, *bmin;           // [nb] each
    const float* poses_prev;                                         // [N x 16] propagated poses of the previous frame
    const int32_t* nn_prev;                                          // [N]
    const int32_t* status_prev;                                      // [2]
    int32_t* ridx_out;                                               // nullable [N]
    int nb, ng;
    int32_t softmax, mode;
    const double* u;                                                 // nullable: the previous frame's uniforms
    float u32;
    uint64_t seed, step;                                             // Philox key / counter of the previous frame's draws
    int64_t tstride = 0;      // batch of trajectories: doubles between two trajectories' table blocks
    int64_t key_base = 0;     // Philox key of this trajectory's slot 0 (trajectory * N), set per trajectory in the kernel
    int32_t traj = 0;         // trajectory (the systematic draw's key is seed + trajectory, as in k_tail_b2)
};

// sparse scoring inside the particle kernels (score_body.hpp score_claimed_rows)
struct SparseScore {
    uint32_t* stamps = nullptr;   // [K] epoch of the last frame that scored row k (nullptr: dense scoring)
    uint32_t epoch = 0;
    const float* emb = nullptr;
    const double* norms = nullptr;
    const double* code = nullptr;
    double* scores = nullptr;
    int nj = 0;                   // D / 64
    // prediction list (single-trajectory fused front): the rows the previous frame used, listed and stamped `pred_tag`
    // (= epoch - 1) by that frame's tail kernel; scored by streaming waves of the front launch (score_list_wave)
    uint32_t pred_tag = 0;              // 0: no prediction in this launch (every stamp other than `epoch` is stale)
    const int32_t* list = nullptr;      // [list_cap]
    const int32_t* list_count = nullptr;
    int32_t* next_count = nullptr;      // the other list's counter, zeroed by the front for this frame's tail
    int32_t list_cap = 0;
    // dense_thr > 0: a frame whose list holds more rows than this scores ALL rows with the streaming waves instead (K rows in one
    // coalesced stream cost less than a few thousand scattered ones plus the claims of the rows the list missed - the frames after
    // a wide start); the particle waves then only mark the rows they use (for the next frame's list) and score nothing
    int32_t dense_thr = 0;
    int64_t K = 0;
};
// what the tail kernel needs to build the next frame's list: rows whose stamp is `epoch` (claimed or confirmed in this
// frame) are appended to `list` and re-stamped epoch + 1, the next frame's pred_tag (its epoch is epoch + 2).
// Further chances (round 5): a row that was on this frame's list but that nobody needed (stamp still epoch - 1, whatever its age
// bits) is listed again, up to MIDAS_PRED_CHANCES (3) frames in a row, stamped (epoch + 1) | age << 30 - in the frames after a wide start half of the rows a frame needs and the frame before
// did not were in use two frames back (the cloud's fringe flickers: tools/diag_flicker.py), and every such row was a claim: a
// stamp exchange and a cold 2 KB fetch inside a particle wave.  Epochs stay below 2^30 (MIDAS_EPOCH_LIMIT), bits 31:30 count the
// frames a listed row went unused (MIDAS_PRED_CHANCES of them are allowed).
#ifndef MIDAS_PRED_CHANCES
#define MIDAS_PRED_CHANCES 3  // further frames a listed row stays on the list unused (0 .. 3)
#endif
constexpr uint32_t PRED_SECOND = 0xC0000000u;  // bits 31:30 of a listed row's stamp: frames it has been listed without being used
constexpr uint32_t PRED_AGE1 = 0x40000000u;
constexpr uint32_t MIDAS_EPOCH_LIMIT = 0x3FFFFFF0u;
struct ScorePredict {
    uint32_t* stamps = nullptr;
    uint32_t epoch = 0;
    int64_t K = 0;
    int32_t* list = nullptr;
    int32_t* count = nullptr;
};

// Where a front kernel takes its particles from when the unpack of the previous frame is folded into it (midas_shard_run):
// rows == nullptr: the particle arrays.
struct PeerInboxSrc {
    const char* rows = nullptr;        // this rank's inbox
    long long flag_off = 0;            // bytes from the inbox to its flag block
    unsigned long long tag = 0;        // the frame tag the rows must carry
    int G = 0, rank = 0;
    char* const* peers = nullptr;      // non-null: the launch publishes this rank's flag (its first wave) before anybody waits
    int32_t* status = nullptr;         // bit 16 when a flag did not arrive within the bound
};

struct ParticleUpdateArgs {
    int64_t N;
    const float* poses_in;
    float* poses_prop;
    const float* odom16;
    const float* tn;
    const float* rot;
    float std_t, std_r;
    uint64_t seed, step;
    const int32_t* n_live = nullptr;  // nullable: the live particle count in device memory (loop engine); N is then
                                      // the capacity the grid was sized for and slots >= *n_live are skipped
    int64_t slot_base = 0;  // global index of local particle 0 (Philox key)
    int32_t batch = 1;      // trajectories (grid.y); per-trajectory arrays are (batch, ...) contiguous
    int64_t score_stride = 0;  // K: scores are (batch, K)
    const int32_t* hint_in;
    int32_t* nn_idx;
    const double* scores;  // [K]
    double* x;             // [N] gathered score
    double* e;             // [N] exp(x - 1): softmax numerator with the constant shift 1 (scores are cosines)
    uint8_t* valid;        // [N] prune mask
    double t2;             // squared prune threshold (exact: sqrt(d2) > thr  <=>  d2 > t2)
    double thr;            // the threshold itself (triangle-inequality tests of the vertex lists)
    const MeshRec* vlist;  // nullable: per-codebook-entry mesh vertex lists
    const MeshScr* vscr = nullptr;  // nullable: their float32 screening copy (only read when vlist is set)
    MeshField field;                // d != nullptr: the mesh's distance field decides the prune wherever it can (see MeshField)
    double* part_max;      // [nblocks]
    double* part_min;      // [nblocks]
    const float* gt16;     // nullable
    double* part_rmse;     // [2*nblocks] when gt16
    int ablate = 0;        // profiling only (MIDAS_ABLATE)
    unsigned long long* telemetry = nullptr;  // nullable: cumulative [NN tree searches, mesh tree searches]
    int32_t* status_reset = nullptr;          // nullable: status[0..1] zeroed here for the tail kernels' atomics
    double* flags_reset = nullptr;            // nullable: two float64 counters zeroed here (sharded exchange record)
    LazyResample rs;                          // fused front only
    SparseScore sp;                           // stamps != nullptr: only the rows that are some particle's nearest entry are scored
    PeerInboxSrc inbox;                       // rows != nullptr: particles come from the rank's inbox (unpack folded in; forms without folded resample)
    // presorted form of the folded resample (k_presort_search / k_presort_group in front of the launch): the waves take their
    // particles in an order that puts slots with the same nearest-entry hint side by side, and find the slot's source ready
    const int32_t* pre_order = nullptr;       // [batch x N] rank -> slot
    const int32_t* pre_src = nullptr;         // [batch x N] rank -> source particle of that slot (what lazy_source returns)
    double* pre_rmse_terms = nullptr;         // [batch x N x 2] with gt16: the particles' rmse terms BY SLOT - the per-wave sums the tail
                                              // reads are formed from them in slot order (k_rmse_parts), as the unsorted launch forms them
};
int particle_update_blocks(int64_t N);
bool index_build_on_host();  // MIDAS_HOST_INDEX=1: the host builders of round 1 (checkers of the device builders)
int build_neighbour_graph_device(midas_ctx* ctx, midas_tree* t);
int build_vertex_screen(midas_ctx* ctx, midas_tree* t6);  // t6->vscr from t6->vlist (MIDAS_NO_VSCR=1: none)
int build_vertex_lists_device(midas_ctx* ctx, midas_tree* t6, const midas_tree* t3, const float* cb_poses_dev);
int launch_knn6(midas_ctx* ctx, const midas_tree* t, int64_t N, const float* feat6, int32_t k, int32_t* idx, float* d2);
// front.hip
int launch_frame_front(midas_ctx* ctx, const midas_tree* t6, const midas_tree* t3, const ParticleUpdateArgs& a,
                       const midas_codebook* cb, const double* code, double* scores, bool* launched);
int launch_particle_update(midas_ctx* ctx, const midas_tree* t6, const midas_tree* t3, const ParticleUpdateArgs& a);
// the loop step's small-set front (k_front_small) for B trajectories with their live counts (midas_loop_step_batch): a.N = the
// capacity (up to 16 384; wide, midas_loop_step_batch_wide: up to MIDAS_LOOP_BATCH_WIDE_MAX_CAP), a.n_live = trajectory 0's count,
// LOOP_CTL_I entries apart
int launch_front_small_batch(midas_ctx* ctx, const midas_tree* t6, const midas_tree* t3, const ParticleUpdateArgs& a,
                             const midas_codebook* cb, const double* code, double* scores, int32_t B, bool wide = false);
// the same for rows on different objects (midas_loop_step_batch_objects, k_front_small_objects): `a` without the trees, the vertex
// lists, the field and the codebook - every workgroup takes those from its row's record of the set; scores and stamps (B, K_max)
// rows (midas_loop_step_batch_rows): std_t, std_r, thr and t2 of `a` are then not read - k_front_small_rows takes row b's
int launch_front_small_objects(midas_ctx* ctx, const midas_object_set* set, const ParticleUpdateArgs& a, const double* code,
                               double* scores, bool wide, const midas_loop_row_params* rows = nullptr);
// One launch of a front as launch_frame_front hands it to the units that hold the kernels, and the form of k_frame_front it asks
// for (the template's LAZY, FW, SCR, PREF, STATS: front_wave.hpp).  A family's launcher launches the form if it is one of its own
// and says whether it was.
struct FrontForm { int lazy, fw; bool scr, pref, stats; };
struct FrontLaunch {
    midas_ctx* ctx; const midas_tree *t6, *t3; const ParticleUpdateArgs& a; const midas_codebook* cb; const double* code; double* scores;
    dim3 grid; int n_pu, nwaves;  // the launch's grid; its workgroups of particle waves, particle waves per trajectory
};
bool launch_front_plain(const FrontLaunch& L, const FrontForm& f);   // front.hip: no folded resample
bool launch_front_folded(const FrontLaunch& L, const FrontForm& f);  // front_folded.hip: folded resample, one trajectory
bool launch_front_batch(const FrontLaunch& L, const FrontForm& f);   // front_batch.hip: a batch of trajectories (+ k_rmse_parts behind a presorted launch)
int launch_presort(midas_ctx* ctx, ParticleUpdateArgs& a);           // front_batch.hip: fills a.pre_order / a.pre_src

// ---- host: a frame's particle-update arguments ------------------------------------------------------------------------
// largest float64 t2 with sqrt(t2) <= thr, so that  sqrt(d2) > thr  <=>  d2 > t2  exactly
inline double squared_threshold(double thr) {
    if (!(thr >= 0.0)) return -1.0;  // nothing is within a negative / NaN threshold
    if (std::isinf(thr)) return INFINITY;
    double t = thr * thr;
    while (std::sqrt(t) > thr) t = std::nextafter(t, 0.0);
    while (std::sqrt(std::nextafter(t, INFINITY)) <= thr) t = std::nextafter(t, INFINITY);
    return t;
}

// The fields every frame form fills alike from its arguments (midas_step_args, midas_lazy_args, midas_shard_front_args and
// midas_loop_args name them the same): motion and its draws, the nearest-entry search, the prune, telemetry and the score
// stamps (`stamps`: the frame's, or nullptr where the form does not score sparsely).  Where the particles come from and where
// the rmse sums go differ between the forms; every other field of `pa` is the caller's.
template <class FrameArgs>
inline void fill_particle_update(ParticleUpdateArgs& pa, const FrameArgs& s, const midas_tree* t6, const midas_tree* t3, int64_t N,
                                 const float* poses_in, const int32_t* hint_in, uint8_t* valid, uint32_t* stamps, const float* gt16,
                                 double* part_rmse) {
    pa.N = N;
    pa.poses_in = poses_in;
    pa.poses_prop = s.poses_prop_dev;
    pa.odom16 = s.odom16_dev;
    pa.tn = s.tn_dev;
    pa.rot = s.rot_dev;
    pa.std_t = s.std_t;
    pa.std_r = s.std_r;
    pa.seed = s.seed;
    pa.step = s.step;
    pa.hint_in = hint_in;
    pa.nn_idx = s.nn_idx_dev;
    pa.valid = valid;
    pa.t2 = squared_threshold(s.prune_thr);
    pa.thr = s.prune_thr;
    pa.vlist = (t6->vlist && t6->vlist_mesh == t3) ? (const MeshRec*)t6->vlist : nullptr;
    pa.vscr = pa.vlist ? (const MeshScr*)t6->vscr : nullptr;
    pa.field = t3->field;
    pa.telemetry = (unsigned long long*)s.telemetry_dev;
    pa.gt16 = gt16;
    pa.part_rmse = part_rmse;
    if (stamps && s.score_epoch) { pa.sp.stamps = stamps; pa.sp.epoch = s.score_epoch; }
}

// Prediction lists of the sparse scoring (include/midas_hip.h score_list_dev: two counts, then two lists of K rows): the frame
// with epoch e scores list (e >> 1) & 1, which the frame before tagged e - 1, and its tail builds the other one for the next
// frame.  next_score_list: what that tail needs.
inline ScorePredict next_score_list(uint32_t* stamps, uint32_t epoch, int32_t* lists, int64_t K) {
    const int par = (int)((epoch >> 1) & 1u) ^ 1;
    ScorePredict p;
    p.stamps = stamps; p.epoch = epoch; p.K = K;
    p.count = lists + par;
    p.list = lists + 2 + (int64_t)par * K;
    return p;
}
// sp (stamps and epoch set) scores this frame's list -> next_score_list
inline ScorePredict wire_score_list(SparseScore& sp, int32_t* lists, int64_t K) {
    const int par = (int)((sp.epoch >> 1) & 1u);
    sp.pred_tag = sp.epoch - 1u;
    sp.list_count = lists + par;
    sp.list = lists + 2 + (int64_t)par * K;
    sp.list_cap = (int32_t)(K < 0x7fffffff ? K : 0x7fffffff);
    sp.next_count = lists + (par ^ 1);
    return next_score_list(sp.stamps, sp.epoch, lists, K);
}

// resample.hip - the weight and resampling operators on their own, and TA of the eager step tail
int launch_gather_f64(midas_ctx* ctx, int64_t N, const double* table, const int32_t* idx, double* out);
int launch_softmax(midas_ctx* ctx, int64_t N, const double* x, int32_t softmax, double* w);
int launch_prune(midas_ctx* ctx, int64_t N, double* w, const double* dist, double thr, int32_t* nvalid);
int launch_cdf(midas_ctx* ctx, int64_t N, const double* w, double* cdf, int32_t* status);
int launch_search(midas_ctx* ctx, int64_t N, const double* cdf, int64_t M, int32_t mode, const double* u,
                  float u32, uint64_t seed, uint64_t step, int32_t* idx);
int launch_gather_rows(midas_ctx* ctx, int64_t M, const int32_t* idx, const void* src, void* dst, int32_t row_bytes);
int launch_selftest_wave_sums(midas_ctx* ctx, const double* in64, double* out256);
int launch_tail_a(midas_ctx* ctx, int64_t N, const double* x, const uint8_t* valid, int np, int pstride,
                  const double* pmax_all, const double* pmin_all, int32_t softmax, double* e_io, double* lp_out,
                  double* block_sums_e, double* block_totals_em, double* flags_out, int32_t* flag, int32_t* status,
                  int batch = 1);

// tail.hip - the fused tail of the step: x,valid,partials -> weights (masked) -> cdf -> search -> gather
struct StepTailArgs {
    int32_t batch = 1;       // trajectories (grid.y)
    int64_t N;
    int npart;               // number of part_max/part_min entries
    const double* x;
    double* e;               // exp(x - 1) from the particle update (replaced by x when the softmax is skipped)
    const uint8_t* valid;
    const double* part_max;
    const double* part_min;
    int32_t softmax;
    double* weights;         // [N] masked weights (pre-resample)
    double* cdf;             // [N] scratch
    int32_t* status;         // [2]
    int32_t mode;
    const double* u;
    float u32;
    uint64_t seed, step;
    int32_t* ridx;
    const float* poses_prop;
    float* poses_out;
    double* weights_out;
    const int32_t* nn_idx;
    int32_t* hint_out;
    const double* part_rmse;  // nullable
    double* rmse_out;
    // deferred mode (x == nullptr): the particle update ran without the scores (concurrently with the scoring);
    // the tail gathers x = scores[nn_idx], takes the exponentials and decides the isclose guard itself
    const double* scores = nullptr;
    double* x_raw = nullptr;   // [N] scratch: raw scores, written only where the guard may fire
    double* lp_raw = nullptr;  // [N] scratch: block-local prefix of x*valid, likewise
    int64_t score_stride = 0;  // K: scores are (batch, K)
    int64_t tstride = 0;       // pipelined batch: doubles between two trajectories' table blocks (tables_of layout per trajectory)
};
// The fields the eager step and the pipelined flush fill alike from their arguments (midas_step_args and midas_lazy_flush_args
// name them the same), as fill_particle_update does for the front; every other field of `ta` is the caller's.
template <class TailFrameArgs>
inline void fill_step_tail(StepTailArgs& ta, const TailFrameArgs& s) {
    ta.N = s.N;
    ta.softmax = s.softmax;
    ta.weights = s.weights_dev;
    ta.status = s.status_dev;
    ta.mode = s.resample_mode;
    ta.u = s.u_dev;
    ta.u32 = s.u32;
    ta.seed = s.seed;
    ta.step = s.step;
    ta.ridx = s.ridx_dev;
    ta.poses_prop = s.poses_prop_dev;
    ta.poses_out = s.poses_out_dev;
    ta.weights_out = s.weights_out_dev;
    ta.nn_idx = s.nn_idx_dev;
    ta.hint_out = s.hint_out_dev;
    ta.rmse_out = s.rmse_dev;
}
// the deferred tail on explicit tables (what k_tail_a2 writes and k_tail_b2 / the lazy front read)
struct TailTables {
    double *e, *x_raw, *lp, *lp_raw, *gend, *gend_raw;       // [N] x4, [ceil(N/16)] x2
    double *bsum_e, *btot, *btot_raw, *bmax, *bmin;           // [ceil(N/4096)] each
    double *ggend, *ggend_raw;                                // [16 ceil(N/4096)]: block-local prefix at the end of each 256-slot group
    guide_t *guide = nullptr, *guide_raw = nullptr;           // nullable [ceil(N/4096) x GUIDE_STRIDE] each (see GUIDE_BINS)
};
int launch_tail_a2(midas_ctx* ctx, int64_t N, const double* scores, const int32_t* nn_idx, const uint8_t* valid,
                   int32_t softmax, const TailTables& tb, int32_t* status, int batch = 1, int64_t score_stride = 0,
                   bool padded_tables = false, const double* part_rmse = nullptr, double* rmse_out = nullptr, int64_t tstride = 0,
                   const ScorePredict* predict = nullptr);  // padded: per-slot tables hold a multiple of 16 values (tables_of, api_entry.hpp)
int launch_predict_seed(midas_ctx* ctx, int64_t N, const int32_t* idx, const ScorePredict& pr);
int launch_shard_tail_a(midas_ctx* ctx, int64_t N, const double* scores, const int32_t* nn_idx, const uint8_t* valid,
                        int32_t softmax, const TailTables& tb, double* r1, int32_t* status, const double* part_rmse = nullptr,
                        const ScorePredict* predict = nullptr);
int launch_tail_b2(midas_ctx* ctx, const StepTailArgs& a, const TailTables& tb);  // a.x, a.e, a.cdf, a.lp_raw unused
int launch_step_tail(midas_ctx* ctx, const StepTailArgs& a, int prof_slot_base);
int debug_tb2_clocks(long long* out16);
int debug_ta_clocks(long long* out16);
int debug_tg_clocks(long long* io64, int reset);
int debug_tg_waves(long long* out4096);

// shard_route.hip - the sharded engine's exchange behind launch_shard_tail_a
int launch_tail_fin(midas_ctx* ctx, int64_t N, const double* e, const double* x_raw, const double* lp, const double* lp_raw,
                    const uint8_t* valid, double* weights, double* cdf_io, int G, int nb, const double* r1_all, int rank,
                    double n_total, int32_t softmax, double* rmse_out, int32_t* status);
int launch_tail_resample(midas_ctx* ctx, const midas_tail_resample_args& r);
// sync (peer form, C-side frame): the route kernel's last workgroup publishes the frame's completion flag and waits for every
// rank's (the word behind the 64 flags of the own inbox counts the finished workgroups: zero between launches)
struct PeerRouteSync { const char* inbox; long long flag_off; unsigned long long tag; };
int launch_shard_route(midas_ctx* ctx, const midas_shard_route_args& r, const TailTables& tb, bool pack, const PeerRouteSync* sync = nullptr);
int launch_shard_unpack(midas_ctx* ctx, int64_t N, const void* recv, int32_t* ridx, float* poses_out, double* weights_out,
                        int32_t* hint_out, int32_t dest = -1);
int launch_shard_unpack_peer(midas_ctx* ctx, int64_t N, const void* inbox, int32_t* ridx, float* poses_out, double* weights_out,
                             int32_t* hint_out);
int launch_peer_flag_write(midas_ctx* ctx, void* const* peers, int G, int rank, int64_t flag_off, uint64_t tag);
int launch_shard_unpack_peer_wait(midas_ctx* ctx, int64_t N, const void* inbox, int32_t* ridx, float* poses_out, double* weights_out,
                                  int32_t* hint_out, int G, int64_t flag_off, uint64_t tag, int32_t* status, void* const* peers, int rank);
int launch_peer_probe(midas_ctx* ctx, void* const* peers, const void* inbox, int G, int rank, int nonce, int32_t* ok);

// front_folded.hip, front.hip
int debug_ff_clocks(long long* io8192, int reset);
int launch_reduce_partials(midas_ctx* ctx, int np, const double* pmax, const double* pmin, const double* prm,
                           double* extrema2, double* rmse_sums2);

// cluster.hip
int launch_cluster_centers(midas_ctx* ctx, int64_t N, const float* poses, const double* w64, const float* w32,
                           const int64_t* labels, int32_t C, const int64_t* label_values, float* centers, float* stds,
                           int64_t* counts, bool logmap = false);  // logmap: midas_cluster_centers_logmap (cluster_logmap.hpp)
int launch_se3_log(midas_ctx* ctx, int64_t N, const float* poses, double* xi);

// the pose estimate of a fixed-N frame for B trajectories (midas_pose_estimate): weights w64 (B x N), or - nullptr - made from
// the pipelined frame's table blocks tb (trajectory 0's, tstride doubles apart) and the valid mask
int launch_pose_estimate(midas_ctx* ctx, int64_t N, int32_t B, const float* poses, const double* w64, const TailTables* tb,
                         int64_t tstride, const uint8_t* valid, int32_t softmax, float* centers, float* stds);

// the sharded engine's estimate (midas_shard_estimate_*): this rank's ceil(N / 256) x 36 moment partials from its eager weights;
// the finish over the partials of all ranks in rank order (nblocks = G * ceil(N / 256))
constexpr int ESTIMATE_PART_DOUBLES = 36;  // doubles of one 256-particle block's partial (CL_MOM, cluster_rot.hpp)
int launch_shard_estimate_moments(midas_ctx* ctx, int64_t N, const float* poses, const double* w64, double* part);
int launch_shard_estimate_finish(midas_ctx* ctx, int64_t nblocks, const double* part_all, float* center, float* stds);

struct LoopWeightsParamRowsArgs;  // loop_weights.hpp
int launch_loop_cluster(midas_ctx* ctx, int64_t cap, const int32_t* ctl_i, const float* poses, const double* w64,
                        const int32_t* labels, double* part, float* centers, float* stds, int64_t* counts, double* rot,
                        const LoopWeightsParamRowsArgs* weights = nullptr,  // weights: computed at the head of the moment launch (loop_weights.hip)
                        int32_t B = 1,  // trajectories (grid.y): every array (B, ...) contiguous, the scratch ones included
                        bool logmap = false,           // MIDAS_LOOP_CENTERS_LOGMAP: whole centres by the finisher, their rotations
                        float* centers_out = nullptr); //   into the compact rows of centers_out (the frame's cluster_poses)

// loop.hip / dbscan.hip - the reference's whole loop body on a variable-size particle set (midas_loop_step)
int launch_loop_step(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* t6, const midas_tree* t3,
                     const midas_loop_args& a, int32_t phases);
int launch_loop_step_batch(midas_ctx* ctx, const midas_codebook* cb, const midas_tree* t6, const midas_tree* t3,
                           const midas_loop_args& a, int32_t phases, int32_t B, int64_t log_stride,
                           bool wide = false);  // midas_loop_step_batch_wide: capacities beyond the small-set regime
// the same frame with every row on the object the set names for it (midas_loop_step_batch_objects): set->B rows; rows
// (midas_loop_step_batch_rows): the filter's parameters per row, set->B records in device memory
int launch_loop_step_batch_objects(midas_ctx* ctx, const midas_object_set* set, const midas_loop_args& a, int32_t phases,
                                   int64_t log_stride, bool wide, const midas_loop_row_params* rows = nullptr);

// The phases of a loop frame, what launch_loop_step and launch_loop_step_batch launch alike: each is the host launcher of the unit
// that holds its kernels.  What they are launched over - the single call: one trajectory, the slice strides 0 (the kernels' defaults).
struct LoopGrid {
    int64_t cap;               // particles of a trajectory the grids cover
    int32_t B = 1;             // trajectories = the grid's y: every array - the caller's and the scratch - (B, ...) contiguous
    int32_t slice = 0;         // a batch: particles between two trajectories' slices of the (B, ...) arrays,
    int32_t lp_stride = 0;     //          prefix values between their tables,
    int64_t log_stride = 0;    //          doubles between their log rows
    double* clocks = nullptr;  // MIDAS_ANNEAL_CLOCKS (the single call): k_loop_xe's phase clocks
    const midas_loop_row_params* rows = nullptr;  // midas_loop_step_batch_rows: B records, the phases launch the kernels that read them
    bool logmap = false;       // MIDAS_LOOP_CENTERS_LOGMAP: the annealing kernels are launched without their rotation workgroup
    unsigned nbcap() const { return (unsigned)ceil_div(cap, SCAN_BLOCK); }
    unsigned by() const { return (unsigned)B; }
    bool batch() const { return slice != 0; }
};
inline int32_t loop_bound(int64_t n) { return (int32_t)(n < (1 << 30) ? n : (1 << 30)); }  // a particle bound as the kernels take it
// loop_weights.hip - FRONT, second half: k_loop_xe, then the weights - launched, or (merged) left in `wa` for the cluster-moment launch
bool loop_weights_mergeable(int32_t phases);
// (objects: rows on different objects - K is then the set's K_max, the stride of the score rows and k_loop_xe's clamp, and the drift
// re-projection gathers row b's poses from the set's table)
int loop_weights_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t K, bool rmse, bool merged,
                       LoopWeightsParamRowsArgs& wa, const midas_object_set* objects = nullptr);
// anneal.hip - ANNEAL behind the clusters' moments (loop_cluster_phase, loop.hip): the decision and the annealed set as an index list
struct LoopMoments { float *cen, *sd; int64_t* cnt; double* rot; };
enum class LoopAnneal {
    frozen,     // the caller said annealing cannot act: the decision's bookkeeping alone
    aten_walk,  // the decision, then ATen's CPU tie choices (topk_aten.hip)
    small,      // sets up to LOOP_SMALL_MAX (anneal_decide.hpp): decision and selection by one workgroup (anneal_small.hip)
    select      // the decision, then the radix select's ten launches
};
inline LoopAnneal loop_anneal_regime(bool frozen, bool aten, bool small) {
    return frozen ? LoopAnneal::frozen : aten ? LoopAnneal::aten_walk : small ? LoopAnneal::small : LoopAnneal::select;
}
int loop_anneal_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, const LoopMoments& m, LoopAnneal regime);
// anneal_small.hip - the decision alone, for the regimes of anneal.hip (hist / sel_state: the select state it clears, or null)
// (g.rows: every row's floor from its record - k_loop_decide_rows; frozen and aten_order are then 0)
int launch_loop_decide(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, const LoopMoments& m, uint32_t* hist,
                       int32_t* sel_state, int32_t frozen, int32_t aten_order);
// the single-workgroup annealing of B trajectories: with the decision from the moments m (a second workgroup
// writes the centres' rotations), or - m null - on a plan the host left in ctl_i (launch_anneal_select); g.rows (with m): floor_n is
// not read, row b's floor comes from its record (k_loop_anneal_small_rows)
int launch_anneal_small(midas_ctx* ctx, const LoopGrid& g, int32_t* ctl_i, double* ctl_d, const LoopMoments* m, float* centers_out,
                        float* stds_out, int32_t floor_n, const double* w, int32_t* src);
// loop_resample.hip - RESAMPLE over the cap2 slots a trajectory the annealed set may take; stream_draws, a call that ends in front of
// it: ctl_i[NDRAW]
int loop_resample_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t cap2);
int loop_ndraw_phase(midas_ctx* ctx, const midas_loop_args& s, const LoopGrid& g, int64_t cap2);
// src[0 .. n_set): the annealed particle set as indices - mode 1: the N particles minus the k of smallest weight, in
// order; mode 2: all N followed by the k of largest weight, best first; ties to the smaller index
int launch_anneal_select(midas_ctx* ctx, int64_t N, const double* w, int32_t mode, int64_t k, int32_t ties, int32_t* src, int32_t* info);
// B trajectories (grid.y): ci (B, 32), w and src (B, cap); info (the fallback counter) with B == 1 only
int launch_topk_aten(midas_ctx* ctx, int64_t cap, const int32_t* ci, const double* w, int32_t* src, int32_t* info, int32_t B = 1);
// labels_out[i] in [-1, ncl) for the n = *n_dev (or N when n_dev is null) poses; min_samples < 0 -> n / 5 (cluster_particles);
// ncl_out[0] = number of clusters; err_out (nullable) |= 2 when the grid / cluster limits were exceeded
int launch_dbscan_points(midas_ctx* ctx, int64_t N, int32_t dim, const double* pts, double eps, int64_t min_samples, int32_t* labels, int32_t* info);
int launch_dbscan(midas_ctx* ctx, int64_t cap, const int32_t* n_dev, const float* poses, double eps, int64_t min_samples,
                  int32_t* labels_out, int32_t* ncl_out, int32_t* err_out, int32_t max_clusters);  // max_clusters 0: any number
// the same for B clouds in one set of launches (B * cap <= MIDAS_DBSCAN_BATCH_MAX_POINTS): poses (B, cap, 16), labels_out (B, cap),
// row b's count at n_dev[b * n_stride] (n_dev null: cap), its cluster count at ncl_out[b * out_stride], its flags ORed into
// err_out[b * out_stride]
int launch_dbscan_batch(midas_ctx* ctx, int32_t B, int64_t cap, const int32_t* n_dev, int64_t n_stride, const float* poses, double eps,
                        int64_t min_samples, int32_t* labels_out, int32_t* ncl_out, int32_t* err_out, int64_t out_stride, int32_t max_clusters);

// mt19937.hip - torch's CPU generator stream on the device
int launch_mt_seed(midas_ctx* ctx, uint64_t seed, uint32_t* state);
int launch_mt_rand64(midas_ctx* ctx, uint32_t* state, int64_t skip_words, int64_t N, double* out, uint32_t* hist);
int launch_mt_rand64_chunked(midas_ctx* ctx, uint32_t* state, int64_t N, double* out, uint32_t* hist, const uint32_t* polys, int32_t G);
int launch_mt_draws(midas_ctx* ctx, uint32_t* state, int64_t skip_words, int32_t nseg, const midas_mt_segment* segs, const float* R,
                    const float* C, const float* S, uint32_t* hist, const uint32_t* polys, int32_t G);
int launch_mt_normal32(midas_ctx* ctx, uint32_t* state, int64_t skip_words, int64_t numel, float mean, float std, const float* R, const float* C,
                       const float* S, float* out, uint32_t* hist, const uint32_t* polys, int32_t G);
int launch_mt_draws_batch(midas_ctx* ctx, int32_t B, uint32_t* state, int64_t skip_words, int32_t nseg, const midas_mt_segment* segs,
                          const float* R, const float* C, const float* S, uint32_t* hist, const uint32_t* polys, int32_t G);
int launch_mt_draws_counted(midas_ctx* ctx, uint32_t* state, int64_t skip_words, int32_t nseg, const midas_mt_counted_segment* segs,
                            const float* R, const float* C, const float* S, int32_t* status);
int launch_mt_draws_counted_batch(midas_ctx* ctx, int32_t B, uint32_t* state, int64_t skip_words, int32_t nseg,
                                  const midas_mt_counted_segment* segs, int64_t count_stride, const float* R, const float* C, const float* S,
                                  int32_t* status, int64_t status_stride);

// topn.hip
int launch_topn_pose_error(midas_ctx* ctx, int32_t B, int64_t K, const double* scores, int64_t row0, int32_t n,
                           const double* feat, int32_t d, double* err_out, int32_t* idx_out);
int launch_topn_pose_error(midas_ctx* ctx, int32_t B, int64_t K, const double* scores, int64_t ld, int64_t row0, int32_t n,
                           const double* feat, int32_t d, double* err_out, int32_t* idx_out);

int launch_topn_rinv(midas_ctx* ctx, int64_t K, int64_t ld, const double* norms, float* rinv);
int launch_topn_pose_error_dots(midas_ctx* ctx, int32_t B, int64_t K, const float* panel, int64_t ld, const double* norms, const float* rinv,
                                int64_t row0, int32_t n, const double* feat, int32_t d, double* err_out, int32_t* idx_out);
// selfsim.hip
int launch_selfsim_panel(midas_ctx* ctx, const midas_codebook* cb, int64_t i0, int64_t R, float* panel, int64_t ldo);
// selfsim_f64.hip
int launch_selfsim_panel_f64(midas_ctx* ctx, const midas_codebook* cb, int64_t i0, int64_t R, double* panel, int64_t ldo);
// tsne.hip
int launch_tsne_knn(midas_ctx* ctx, const void* X, int32_t dtype, int64_t K, int64_t F, int64_t ld, int32_t ntn, int32_t k,
                    int64_t rows, double* scratch, int32_t* idx_out, double* d2_out);
int launch_tsne_perplexity(midas_ctx* ctx, const float* d2, int64_t K, int32_t k, double desired_entropy, double* P);
size_t tsne_grad_scratch_doubles(int64_t K);
int launch_tsne_objective(midas_ctx* ctx, int64_t K, const float* y, const int64_t* crow, const int32_t* col, const float* val,
                          double* work, double* kl_out);
int launch_tsne_update(midas_ctx* ctx, int64_t K, float* y, double* work, int mode, float* grad_out, float* gains, double* update,
                       double momentum, double lr, float min_gain, double* gsq);
int launch_tsne_reset(midas_ctx* ctx, int64_t K, float* gains, double* update);
int launch_tsne_sum(midas_ctx* ctx, const double* x, int64_t n, double* out);

// profiling hook used by the step: record event `slot` on the stream when profiling is on
void prof_mark(midas_ctx* ctx, int slot);

}  // namespace midas
