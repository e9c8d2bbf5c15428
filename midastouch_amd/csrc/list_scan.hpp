// list_scan.hpp - the list scans in front of the tree search: the hint scan of a codebook entry's neighbour list (per lane,
// screened or whole records), its cooperative continuation by the wave, the prune from the entry's vertex list and from the
// mesh's distance field, and nn6_wave, which strings the nearest-neighbour steps together.
#pragma once
#include "tree_search.hpp"

namespace midas {

// Hint fast path.  h = a codebook entry near q (the NN of the particle's ancestor).  The candidates
// {h} U N(h) are scanned in order of rho = |F_h - F_s|; every entry not yet scanned is at least
// rho - |q - F_h| away from q (triangle inequality), so once that exceeds the best distance found the
// search is certified complete and returns the exact answer of the full search.  The comparison
// carries a 3e-5 relative margin on squared distances, two orders above float32 rounding of the
// six-term sums, so "certified" also holds for the COMPUTED distances and their tie rule.
// Returns true when certified; otherwise (best, bi) is a valid bound for the tree search.
#ifndef MIDAS_NN_BATCH
#define MIDAS_NN_BATCH 8
#endif
#ifndef MIDAS_MESH_BATCH
#define MIDAS_MESH_BATCH 8
#endif
#ifndef MIDAS_NN_SOLO
#define MIDAS_NN_SOLO 32
#endif
#ifndef MIDAS_MESH_SOLO
#define MIDAS_MESH_SOLO 16
#endif
constexpr int NN_BATCH = MIDAS_NN_BATCH, MESH_BATCH = MIDAS_MESH_BATCH;  // records per round trip of the per-lane scans
constexpr int NN_SOLO = MIDAS_NN_SOLO;      // records a lane scans by itself before the wave takes over its list
constexpr int MESH_SOLO = MIDAS_MESH_SOLO;
static_assert(NN_SOLO % NN_BATCH == 0 && NBR_M % NN_BATCH == 0 && MESH_SOLO % MESH_BATCH == 0 && MESH_M % MESH_BATCH == 0,
              "scan batches must tile the solo prefixes and the lists");

// ---- half-record screening ------------------------------------------------------------------------------------------
// A record is two 16-byte pieces: lo = c[0..3], hi = {c[4], c[5], idx, rho}.  dist2 adds the six squared differences
// in order, every step an fma onto the sum so far, so the sum after four terms P4 is a LOWER bound of the finished
// distance in the computed arithmetic (adding a non-negative term and rounding never lowers a sum).  A record whose
// P4 already exceeds the best distance can neither win nor tie: its second piece is not fetched at all.  On the
// bench workloads 1 - 6 of 32 records pass the screen (the lists are sorted by 6-d distance from the entry, and most
// of a neighbour's offset is in the translation), so a scan issues about half the loads - and the particle kernels
// are bound by the number of scattered 16-byte loads a CU's vector cache can look up, not by bytes.
// The certificate needs rho only once per batch: of the batch's last record (the largest; everything behind is farther).
#ifndef MIDAS_SCREEN
#define MIDAS_SCREEN 1
#endif
MD float part4(const float* q, const float4& lo) {
    const float d0 = q[0] - lo.x, d1 = q[1] - lo.y, d2 = q[2] - lo.z, d3 = q[3] - lo.w;
    float d = d0 * d0;
    d = fmaf_(d1, d1, d);
    d = fmaf_(d2, d2, d);
    d = fmaf_(d3, d3, d);
    return d;
}
MD float full_from(const float* q, float p4, const float4& hi) {  // == dist2(q, record), bit for bit
    const float d4 = q[4] - hi.x, d5 = q[5] - hi.y;
    float d = fmaf_(d4, d4, p4);
    d = fmaf_(d5, d5, d);
    return d;
}
// P[j] for a per-lane j as a chain of selects on registers (the empty asm keeps the compiler from turning the chain
// back into an indexed array, which it would put in scratch memory)
template <int B>
MD float pick(const float* P, int j) {
    float v = P[0];
#pragma unroll
    for (int k = 1; k < B; ++k) {
        v = j == k ? P[k] : v;
        asm volatile("" : "+v"(v));
    }
    return v;
}
template <int B>
MD int pick(const int* P, int j) {
    int v = P[0];
#pragma unroll
    for (int k = 1; k < B; ++k) {
        v = j == k ? P[k] : v;
        asm volatile("" : "+v"(v));
    }
    return v;
}

// Scans records [0, NN_SOLO) of entry h's list (record 0 = the entry itself, fetched whole with the first batch so that
// r = |q - F_h| costs no round trip of its own).  Per batch: the first pieces of its records and the second piece of
// its last one in one round trip; then the second pieces of up to two records that pass the screen in another (the
// lines are in the vector cache by then); a lane with more takes them one at a time (rare).
template <bool FIRST>
MD void nn6_hint_batch(const float4* __restrict__ nb4, int s0, const float* q, int32_t h, float& best, int64_t& bi, float& r,
                       float& rslack, int& scanned, bool& certified) {
    float4 lo[NN_BATCH];
#pragma unroll
    for (int j = 0; j < NN_BATCH; ++j) lo[j] = nb4[2 * (s0 + j)];
    const float4 hl = nb4[2 * (s0 + NN_BATCH - 1) + 1];
    float P[NN_BATCH];
#pragma unroll
    for (int j = 0; j < NN_BATCH; ++j) P[j] = part4(q, lo[j]);
    if (FIRST) {  // the entry itself: the starting candidate (a NaN distance stays, as in a serial scan)
        const float4 h0 = nb4[1];
        best = full_from(q, P[0], h0);
        bi = h;
        r = __builtin_sqrtf(best);
        rslack = -8e-7f * r;
    }
    unsigned mask = 0;
#pragma unroll
    for (int j = FIRST ? 1 : 0; j < NN_BATCH; ++j) mask |= (P[j] <= best ? 1u : 0u) << j;
    scanned += __popc(mask);
    const unsigned m1 = mask & ~(1u << (NN_BATCH - 1)), m2 = m1 & (m1 - 1u);
    // two second pieces, unconditionally (a lane without a candidate re-reads a piece it holds: conditional loads would
    // be waited for one at a time)
    const int j1 = m1 ? __builtin_ctz(m1) : NN_BATCH - 1, j2 = m2 ? __builtin_ctz(m2) : NN_BATCH - 1;
    const float4 ha = nb4[2 * (s0 + j1) + 1];
    const float4 hb = nb4[2 * (s0 + j2) + 1];
    // candidate updates as selects (the short-circuit form compiled to exec-mask regions: slower, removed in round 6)
    int b32 = (int)bi;  // list indices are int32
    auto take = [&](float p4, const float4& hi, bool on) {  // no short circuits: selects instead of exec-mask regions
        const float d = full_from(q, p4, hi);
        const int32_t id = __float_as_int(hi.z);
        const bool better = on & ((d < best) | ((d == best) & (id < b32)));
        best = better ? d : best;
        b32 = better ? id : b32;
    };
    take(pick<NN_BATCH>(P, j1), ha, m1 != 0);
    take(pick<NN_BATCH>(P, j2), hb, m2 != 0);
    take(P[NN_BATCH - 1], hl, (mask >> (NN_BATCH - 1)) != 0);
    unsigned rest = m2 & (m2 - 1u);
    while (rest) {  // more than two candidates among the batch's first records
        const int j = __builtin_ctz(rest);
        rest &= rest - 1u;
        take(pick<NN_BATCH>(P, j), nb4[2 * (s0 + j) + 1], true);
    }
    bi = b32;
    // every record behind this batch is at least this far (lower bound of |q - F| with slack for the rounding of r, rho)
    const float g = fmaf_(hl.w - r, 0.9999996f, rslack);
    certified = g > 0.0f && g * g * 0.99997f > best;
}

// Pivot switch across the rotation-angle-pi cut.  The feature's rotation part is 0.01 log(R): a particle whose rotation angle
// passes pi reappears 2 pi 0.01 = 63 mm-equivalents away from its ancestor's nearest entry, and no list of that entry can
// certify anything for it - the lane would walk all NBR_M records (eight cooperative passes of cold fetches) before the
// twin entry gets its turn.  With uniformly distributed yaws about 0.5 % of the particles of a spread cloud cross the cut in a
// frame, i.e. every second wave has such a lane and ends 30 us after the others (phase clocks of the diffuse regime,
// profiles/r03_diffuse_*).  So: a lane that finds itself farther than FLIP_R from the hinted entry (nothing near an entry is:
// codebook spacings are millimetres) continues from the entry's TWIN - the entry nearest to the hinted one's image across the
// cut - whose index travels with the first batch.  Any pivot is a correct pivot (the certificate is relative to the list
// scanned, the continuation and the tree search stay behind it), so this changes which records are read, never the answer.
constexpr float FLIP_R = 0.02f;
MD bool nn6_hint_scan_screened(const TreeView<Kd6>& tv, const float* q, int32_t& h, float& best, int64_t& bi, int* n_scanned,
                               float* r_out = nullptr) {
    const float4* __restrict__ nb4 = reinterpret_cast<const float4*>(tv.nbrs + (size_t)h * NBR_REC);
    float r = 0.f, rslack = 0.f;
    int scanned = 0;
    bool certified = false;
    const int32_t tw = tv.twin[h];  // with the first batch: behind it, it would be a round trip of its own
    nn6_hint_batch<true>(nb4, 0, q, h, best, bi, r, rslack, scanned, certified);
    if (!certified && r > FLIP_R && tw >= 0) {
        h = tw;
        nb4 = reinterpret_cast<const float4*>(tv.nbrs + (size_t)h * NBR_REC);
        scanned = 0;
        nn6_hint_batch<true>(nb4, 0, q, h, best, bi, r, rslack, scanned, certified);
    }
#pragma unroll 1
    for (int s0 = NN_BATCH; s0 < NN_SOLO && !certified; s0 += NN_BATCH)
        nn6_hint_batch<false>(nb4, s0, q, h, best, bi, r, rslack, scanned, certified);
    if (r_out) *r_out = r;
    if (n_scanned) *n_scanned = scanned;
    return certified;
}

// The unscreened form (whole records, one round trip per batch): what the batch step and the largest particle sets run -
// there the waves are many and short of registers, and a batch in two round trips costs more than the loads it saves
// (c5: 353 -> 376 us per batch frame with the screen, c2's front 32.2 -> 30.8 us).
// Scans records [0, NN_SOLO) of entry h's list (record 0 = the entry itself); the first batch is fetched
// together with the entry so that r = |q - F_h| costs no round trip of its own.
// (measured and dropped: a greedy hop to a closer entry's list - no effect at c2, hints are rarely stale; none at c5 either (round 6:
// 278 us per batch frame with and without): there the nearest entry is about as far as the hinted one - the feature's rotation part
// spreads the entries over five dimensions - so no pivot shortens the proof, 47 of a wave's 64 lanes go on to nn6_coop either way)
MD bool nn6_hint_scan(const TreeView<Kd6>& tv, const float* q, int32_t& h, float& best, int64_t& bi, int* n_scanned,
                      float* r_out = nullptr) {
    const Nbr6* nb = tv.nbrs + (size_t)h * NBR_REC;
    float r = 0.f, rslack = 0.f;
    int scanned = 0;
    int b32 = h;  // record 0 overwrites the incoming candidate; list indices are int32
    bool certified = false;
    int32_t tw = tv.twin[h];  // pivot switch across the angle-pi cut (see nn6_hint_scan_screened); once
#pragma unroll 1
    for (int s0 = 0; s0 < NN_SOLO && !certified; s0 += NN_BATCH) {
        if (s0 == NN_BATCH && r > FLIP_R && tw >= 0) {  // far from the hinted entry: its twin's list from the start
            h = tw;
            tw = -1;
            b32 = h;
            nb = tv.nbrs + (size_t)h * NBR_REC;
            s0 = 0;
            scanned = 0;
        }
        Nbr6 e[NN_BATCH];
#pragma unroll
        for (int j = 0; j < NN_BATCH; ++j) e[j] = nb[s0 + j];
#pragma unroll
        for (int j = 0; j < NN_BATCH; ++j) {
            Point6 p;
#pragma unroll
            for (int a = 0; a < 6; ++a) p.c[a] = e[j].c[a];
            const float d = dist2(q, p);
            if (s0 == 0 && j == 0) {  // the entry itself: the starting candidate (a NaN distance stays, as in a serial scan)
                best = d;
                r = __builtin_sqrtf(best);
                rslack = -8e-7f * r;
            } else {
                // Serial semantics without branches (the compiler turned the nested conditions into exec-mask regions, ~25
                // scalar / mask instructions per record): a record counts while no earlier one has certified;
                // lower bound of |q - F| for this and every later record, with slack for the rounding of r and rho
                const float g = fmaf_(e[j].rho - r, 0.9999996f, rslack);
                certified |= (g > 0.0f) & (g * g * 0.99997f > best);
                const bool better = !certified & ((d < best) | ((d == best) & (e[j].idx < b32)));
                best = better ? d : best;
                b32 = better ? e[j].idx : b32;
                scanned += certified ? 0 : 1;
            }
        }
    }
    bi = b32;
    if (r_out) *r_out = r;
    if (n_scanned) *n_scanned = scanned;
    return certified;
}


// ---- wave-cooperative continuation of the list scans ------------------------------------------------
// Most lanes certify inside their first batch of records; the few that do not used to walk the rest of
// their list alone (up to 32 dependent round trips) while 60 lanes idled.  Here the whole wave serves
// them one at a time: 64 records per round trip, one per lane, reduced with the exact (distance, index)
// tie rule.  Any evaluated candidate bounds the answer from above, so after a chunk the proof is the same
// triangle-inequality test on the chunk's LAST record (largest rho): everything beyond it is farther.
MD float rl_f32(float v, int lane) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane)); }
MD int rl_i32(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// minimum over the wave of (d, idx) with ties to the smaller idx; result uniform
MD void wave_best(float& d, int& i) {
    best_step<DPP_XOR1>(d, i);
    best_step<DPP_XOR2>(d, i);
    best_step<DPP_HALF_MIRROR>(d, i);
    best_step<DPP_ROW_MIRROR>(d, i);
    float bd = rl_f32(d, 0);
    int bi = rl_i32(i, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) {
        const float od = rl_f32(d, r);
        const int oi = rl_i32(i, r);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    d = bd;
    i = bi;
}

// one full cooperative scan of entry h's list for the query of lane `owner`, records [first, NBR_M];
// returns certified; (bb, bi) in/out uniform
MD bool coop_scan_list(const TreeView<Kd6>& tv, const float* qq, int h, int first, float rr, float& bb, int& bi) {
    const int lane = threadIdx.x & 63;
    const Nbr6* nb = tv.nbrs + (size_t)h * NBR_REC;
    const float rslack = -8e-7f * rr;
    for (int c0 = first; c0 <= NBR_M; c0 += 64) {
        const int s = c0 + lane;
        float d = INFINITY, rho = INFINITY;
        int id = 0x7fffffff;
        if (s <= NBR_M) {
            const Nbr6 e = nb[s];
            Point6 p;
#pragma unroll
            for (int a = 0; a < 6; ++a) p.c[a] = e.c[a];
            d = dist2(qq, p);
            if (!(d == d)) d = INFINITY;
            id = e.idx;
            rho = e.rho;
        }
        wave_best(d, id);
        if (d < bb || (d == bb && id < bi)) { bb = d; bi = id; }
        const int last = (c0 + 63 <= NBR_M ? c0 + 63 : NBR_M) - c0;
        const float g = fmaf_(rl_f32(rho, last) - rr, 0.9999996f, rslack);
        if (g > 0.0f && g * g * 0.99997f > bb) return true;
    }
    const float g = fmaf_(tv.rho_out[h] - rr, 0.9999996f, rslack);
    return g > 0.0f && g * g * 0.99997f > bb;
}

// serve the lanes in `need`: continue their hint scan after the solo records, then try the twin entry.
// minimum over a 16-lane row of (d, idx), ties to the smaller idx; every lane of the row gets the result
MD void row_best(float& d, int& i) {
    best_step<DPP_XOR1>(d, i);
    best_step<DPP_XOR2>(d, i);
    best_step<DPP_HALF_MIRROR>(d, i);
    best_step<DPP_ROW_MIRROR>(d, i);
}

// COOP_G owners at a time, one per group of 64 / COOP_G lanes: the group walks the next 64 records of its owner's list in
// 64 / L steps of L (all the loads of a lane in flight together) and reduces inside the group with DPP - the owners are
// evaluated by the same instructions, where the whole-wave form spent them once per owner.  The certificate is the
// one of the 64-record chunk (its last record's rho against the final best); an owner it does not settle comes back
// in the next pass with its next 64 records, until its list is exhausted (then: the list's outer radius, the twin).
// A wave of c2 has ~10 open owners (up to ~20): with four per pass (16-lane rows) that was three to five dependent
// round trips, with eight it is two or three.
// (Looking at the stamps only after the prune was measured twice - round 3: front 34 -> 45 us, round 5 with the prediction
// list: 29.7k -> 29.2k steps/s - the particle waves run in lock step, so with the look deferred nearly every wave still
// finds the old stamps and exchanges.  The claim is looked at where it is issued.)
#ifndef MIDAS_COOP_G
#define MIDAS_COOP_G 8
#endif
// records an owner gets per pass (64: eight steps of eight lanes; 32 halves the records fetched past the certificate
// on codebooks where a typical list needs 40 - 60 of them)
#ifndef MIDAS_COOP_CHUNK
#define MIDAS_COOP_CHUNK 64
#endif
// (measured and dropped: piece-contiguous fetches of the group, DESIGN.md notebook "MIDAS_COOP_PIECES")
constexpr int COOP_G = MIDAS_COOP_G, COOP_L = 64 / COOP_G, COOP_CHUNK = MIDAS_COOP_CHUNK, COOP_STEPS = COOP_CHUNK / COOP_L;
static_assert(COOP_G == 4 || COOP_G == 8 || COOP_G == 16, "owners per pass");
static_assert(COOP_STEPS >= 1 && COOP_STEPS * COOP_L == COOP_CHUNK, "a chunk is whole steps of the group");
// minimum over a group of COOP_L lanes of (d, idx), ties to the smaller idx; every lane of the group gets the result
MD void group_best(float& d, int& i) {
    best_step<DPP_XOR1>(d, i);
    best_step<DPP_XOR2>(d, i);
    if (COOP_L >= 8) best_step<DPP_HALF_MIRROR>(d, i);
    if (COOP_L >= 16) best_step<DPP_ROW_MIRROR>(d, i);
}

template <bool SCREEN = false>
MD void nn6_coop(const TreeView<Kd6>& tv, const float* q, int32_t hint, float r_lane, float& best, int64_t& bi, bool need,
                 bool& done) {
    const int lane = threadIdx.x & 63, grp = lane / COOP_L, j = lane % COOP_L;
    int nrec = NN_SOLO;  // next record of this lane's list (owners only)
    // pass after pass: every open owner gets its next 64 records, COOP_G owners per instruction stream
    for (;;) {
        const bool open_lane = need && !done && nrec <= NBR_M;
        unsigned long long todo = __ballot(open_lane);
        if (!todo) break;
        const int my_rank = (int)__builtin_popcountll(todo & ((1ull << lane) - 1ull));  // rank among this pass's owners
        int served = 0;
        while (todo != 0) {
            int mine = -1;
#pragma unroll
            for (int k = 0; k < COOP_G; ++k) {  // (the owners' lane numbers through LDS instead of these scalar steps: no change, dropped)
                const int o = todo ? (int)__builtin_ctzll(todo) : -1;
                todo &= todo - 1;  // 0 & anything stays 0
                mine = grp == k ? o : mine;
            }
            const int src = mine >= 0 ? mine : lane;
            float qq[6];
#pragma unroll
            for (int d = 0; d < 6; ++d) qq[d] = __shfl(q[d], src);
            const float rr = __shfl(r_lane, src);
            float bb = __shfl(best, src);
            int b_i = __shfl((int)bi, src);
            // (shuffles stay unconditional: a lane outside the branch could not serve as a source)
            const int hh_s = __shfl(hint, src), first_s = __shfl(nrec, src);
            const int hh = mine >= 0 ? hh_s : 0;
            const int first = mine >= 0 ? first_s : 0;  // records first .. first+COOP_CHUNK-1, clamped to the list
            float d = INFINITY, rho_last = 0.f;
            int id = 0x7fffffff;
            if (SCREEN) {
            // half-record screening (see part4): first pieces of the lane's records and the second piece of its last one,
            // then the second pieces of the records whose partial distance does not exceed the owner's best
            const float4* __restrict__ nb4 = reinterpret_cast<const float4*>(tv.nbrs + (size_t)hh * NBR_REC);
            float4 lo[COOP_STEPS];
            int sc[COOP_STEPS];
#pragma unroll
            for (int m = 0; m < COOP_STEPS; ++m) {
                const int s = first + COOP_L * m + j;
                sc[m] = s <= NBR_M ? s : NBR_M;
                lo[m] = nb4[2 * sc[m]];
            }
            const float4 hl = nb4[2 * sc[COOP_STEPS - 1] + 1];
            float P[COOP_STEPS];
            unsigned mask = 0;
#pragma unroll
            for (int m = 0; m < COOP_STEPS; ++m) {
                P[m] = part4(qq, lo[m]);
                const bool in = first + COOP_L * m + j <= NBR_M;
                mask |= (in && P[m] <= bb ? 1u : 0u) << m;
            }
            const unsigned m1 = mask & ~(1u << (COOP_STEPS - 1)), m2 = m1 & (m1 - 1u);
            const int k1 = m1 ? __builtin_ctz(m1) : COOP_STEPS - 1, k2 = m2 ? __builtin_ctz(m2) : COOP_STEPS - 1;
            const int s1 = pick<COOP_STEPS>(sc, k1), s2 = pick<COOP_STEPS>(sc, k2);
            const float4 ha = nb4[2 * s1 + 1];
            const float4 hb = nb4[2 * s2 + 1];
            auto take = [&](float p4, const float4& hi, bool on) {
                const float dm = full_from(qq, p4, hi);
                const int im = __float_as_int(hi.z);
                const bool better = on & ((dm < d) | ((dm == d) & (im < id)));  // NaN never wins; selects, no branches
                d = better ? dm : d;
                id = better ? im : id;
            };
            take(pick<COOP_STEPS>(P, k1), ha, m1 != 0);
            take(pick<COOP_STEPS>(P, k2), hb, m2 != 0);
            take(P[COOP_STEPS - 1], hl, (mask >> (COOP_STEPS - 1)) != 0);
            unsigned rest = m2 & (m2 - 1u);
            while (rest) {
                const int k = __builtin_ctz(rest);
                rest &= rest - 1u;
                take(pick<COOP_STEPS>(P, k), nb4[2 * pick<COOP_STEPS>(sc, k) + 1], true);
            }
            rho_last = hl.w;  // of this lane's last record: the group's last lane holds the chunk's last (when the chunk is whole)
            } else {
            const Nbr6* nb = tv.nbrs + (size_t)hh * NBR_REC;
            Nbr6 e[COOP_STEPS];
#pragma unroll
            for (int m = 0; m < COOP_STEPS; ++m) {
                const int s = first + COOP_L * m + j;
                e[m] = nb[s <= NBR_M ? s : NBR_M];
            }
#pragma unroll
            for (int m = 0; m < COOP_STEPS; ++m) {
                Point6 p;
#pragma unroll
                for (int a = 0; a < 6; ++a) p.c[a] = e[m].c[a];
                const float dm = dist2(qq, p);
                const bool in = first + COOP_L * m + j <= NBR_M;
                const bool better = in & ((dm < d) | ((dm == d) & (e[m].idx < id)));  // NaN never wins; no short circuits: no branches
                d = better ? dm : d;
                id = better ? e[m].idx : id;
                rho_last = in ? e[m].rho : rho_last;
            }
            }
            group_best(d, id);
            {
                const bool gb = (d < bb) | ((d == bb) & (id < b_i));
                bb = gb ? d : bb;
                b_i = gb ? id : b_i;
            }
            // largest rho scanned = the last valid record of the chunk (clamped loads repeat the list's last record);
            // once the list is exhausted the bound is the distance of the first entry NOT in it
            rho_last = __shfl(rho_last, lane | (COOP_L - 1));
            const bool at_end = first + COOP_CHUNK - 1 >= NBR_M;
            const float bound = at_end ? tv.rho_out[hh] : rho_last;
            const float gg = fmaf_(bound - rr, 0.9999996f, -8e-7f * rr);
            const bool cert = gg > 0.0f && gg * gg * 0.99997f > bb;
            // hand the groups' results to the owners: the owner with rank r among this pass sits in group r - served
            const int from = COOP_L * ((my_rank - served) & (COOP_G - 1));
            const float rb = __shfl(bb, from);
            const int ri = __shfl(b_i, from);
            const int rc = __shfl((int)cert, from);
            if (open_lane && my_rank >= served && my_rank < served + COOP_G) { best = rb; bi = ri; done = rc != 0; nrec += COOP_CHUNK; }
            served += COOP_G;
        }
    }
    // lists exhausted without a certificate: second chance from the entry across the angle-pi cut, whole wave (rare)
    unsigned long long open = __ballot(need && !done);
    while (open) {
        const int o = (int)__builtin_ctzll(open);
        open &= open - 1;
        const int h1 = rl_i32(hint, o);
        const int tw = tv.twin[h1];
        if (tw < 0) continue;
        float q1[6];
#pragma unroll
        for (int dd = 0; dd < 6; ++dd) q1[dd] = rl_f32(q[dd], o);
        float b1 = rl_f32(best, o);
        int i1 = rl_i32((int)bi, o);
        const Nbr6 ts = tv.nbrs[(size_t)tw * NBR_REC];  // record 0 = the twin itself
        Point6 pt;
#pragma unroll
        for (int a = 0; a < 6; ++a) pt.c[a] = ts.c[a];
        const float r2 = __builtin_sqrtf(dist2(q1, pt));
        const bool c1 = coop_scan_list(tv, q1, tw, 0, r2, b1, i1);
        if (lane == o) { best = b1; bi = i1; done = c1; }
    }
}

// prune: continue the vertex-list scan of the lanes in `need` (mv < 0 after their solo records); owners in
// groups of COOP_G as above, `lim` (the "cannot be within thr" radius) comes from the owner lane
MD double rl_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)rl_i32((int)(unsigned)b, lane), hi = (unsigned)rl_i32((int)(unsigned)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

MD double shfl_f64(double v, int src) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__shfl((int)(unsigned)b, src), hi = (unsigned)__shfl((int)(unsigned)(b >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Four owners at a time, one per 16-lane row, records MESH_SOLO+1 .. MESH_SOLO+64 of each owner's vertex list in four
// steps of 16 (loads in flight together).  Serial semantics inside a row: records in order, the first event decides
// ("provably too far" before "hit" on the same record).  An owner the 64 records do not settle continues with the
// whole wave, 64 records per step.
MD void mesh_coop(const MeshRec* __restrict__ vlist, int32_t h, const double* tq, double t2, double lim_lane, bool need, int& mv) {
    const int lane = threadIdx.x & 63, row = lane >> 4, j = lane & 15;
    unsigned long long todo = __ballot(need);
    const int my_rank = (int)__builtin_popcountll(todo & ((1ull << lane) - 1ull));
    int served = 0;
    while (todo) {
        int owner[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            owner[k] = todo ? (int)__builtin_ctzll(todo) : -1;
            todo &= todo - 1;
        }
        const int mine = row == 0 ? owner[0] : row == 1 ? owner[1] : row == 2 ? owner[2] : owner[3];
        const int src = mine >= 0 ? mine : lane;
        double q3[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) q3[d] = shfl_f64(tq[d], src);
        const double lim = shfl_f64(lim_lane, src);
        const int hh = __shfl(h, src);
        const MeshRec* vl = vlist + (size_t)(mine >= 0 ? hh : 0) * MESH_REC + (1 + MESH_SOLO) + j;
        MeshRec e[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) e[m] = vl[16 * m];
        int res = -1;  // row-uniform
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            Point3 p;
            p.c[0] = e[m].c[0]; p.c[1] = e[m].c[1]; p.c[2] = e[m].c[2];
            const bool hit = dist2(q3, p) <= t2;
            const bool stop = (double)e[m].rho * (1.0 - 1e-7) > lim;
            const unsigned hits = (unsigned)(__ballot(hit) >> (16 * row)) & 0xffffu;
            const unsigned stops = (unsigned)(__ballot(stop) >> (16 * row)) & 0xffffu;
            const int fh = hits ? __builtin_ctz(hits) : 16, fs = stops ? __builtin_ctz(stops) : 16;
            if (res < 0) {
                if (fh < 16 && fh < fs) res = 1;
                else if (fs < 16) res = 0;
            }
        }
        const int from = 16 * ((my_rank - served) & 3);
        const int rres = __shfl(res, from);
        const bool in_group = need && my_rank >= served && my_rank < served + 4;
        if (in_group) mv = rres;
        served += 4;
        // owners the 64 records did not settle (rare): the rest of the list with the whole wave, then the list's outer radius
        unsigned long long open = __ballot(in_group && mv < 0);
        while (open) {
            const int o = (int)__builtin_ctzll(open);
            open &= open - 1;
            double q1[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) q1[d] = rl_f64(tq[d], o);
            const double lim1 = rl_f64(lim_lane, o);
            const MeshRec* v1 = vlist + (size_t)rl_i32(h, o) * MESH_REC;
            int r1 = -1;
            for (int c0 = 1 + MESH_SOLO + 64; c0 <= MESH_M && r1 < 0; c0 += 64) {
                const int s = c0 + lane;
                bool hit = false;
                // (lanes past the end of the list decide nothing: with +inf here they "stopped" the scan, and a list that was
                // merely EXHAUSTED - a dense mesh, the particle 2 mm off its entry - read as "provably too far" instead of going
                // to the tree search; two particles in 640 000 at c5, found by the exhaustive check of round 6)
                float rho = -INFINITY;
                if (s <= MESH_M) {
                    const MeshRec r = v1[s];
                    Point3 p;
                    p.c[0] = r.c[0]; p.c[1] = r.c[1]; p.c[2] = r.c[2];
                    rho = r.rho;
                    hit = dist2(q1, p) <= t2;
                }
                const unsigned long long hits = __ballot(hit);
                const unsigned long long stops = __ballot((double)rho * (1.0 - 1e-7) > lim1);
                const int fh = hits ? (int)__builtin_ctzll(hits) : 64, fs = stops ? (int)__builtin_ctzll(stops) : 64;
                if (fh < 64 && fh < fs) r1 = 1;
                else if (fs < 64) r1 = 0;
            }
            if (r1 < 0) r1 = ((double)v1[0].rho * (1.0 - 1e-7) > lim1) ? 0 : -1;
            if (lane == o) mv = r1;
        }
    }
}


// Prune fast path: decide "some mesh vertex within thr of tq" from the vertex list of the particle's NN
// entry h.  Returns 1 (valid: an actual vertex passes the exact test d2 <= t2), 0 (invalid: every vertex not
// yet scanned is provably farther than thr, triangle inequality with slack far above float64 rounding) or
// -1 (list exhausted: the caller runs the tree search).
// PRE: header and first batch (records 0 .. MESH_BATCH) were fetched by the caller ahead of time (registers: a compile-time
// choice - a pointer that may or may not refer to them would put them in scratch memory)
template <bool PRE = false>
MD int mesh_list_check(const MeshRec* __restrict__ vlist, int32_t h, const double* tq, double t2, double thr,
                       int max_records = MESH_M, double* lim_out = nullptr, const MeshRec* pre = nullptr) {
    const MeshRec* vl = vlist + (size_t)h * MESH_REC;
    const MeshRec hd = PRE ? pre[0] : vl[0];
    Point3 ph;
    ph.c[0] = hd.c[0]; ph.c[1] = hd.c[1]; ph.c[2] = hd.c[2];
    const double delta = __builtin_sqrt(dist2(tq, ph)) * (1.0 + 1e-12);
    const double lim = thr * (1.0 + 1e-9) + delta + 1e-12;  // a vertex with rho*(1-1e-7) > lim cannot be within thr of tq
    if (lim_out) *lim_out = lim;
    // a batch is evaluated branch-free (all its loads in one round trip), then resolved in record order:
    // per record "provably too far" is tested before "hit", so the first event decides
    for (int s0 = 1; s0 <= max_records; s0 += MESH_BATCH) {
        MeshRec e[MESH_BATCH];
        if (PRE && s0 == 1) {
#pragma unroll
            for (int j = 0; j < MESH_BATCH; ++j) e[j] = pre[1 + j];
        } else {
#pragma unroll
            for (int j = 0; j < MESH_BATCH; ++j) e[j] = vl[s0 + j];
        }
        unsigned hits = 0, stops = 0;
#pragma unroll
        for (int j = 0; j < MESH_BATCH; ++j) {
            Point3 p;
            p.c[0] = e[j].c[0]; p.c[1] = e[j].c[1]; p.c[2] = e[j].c[2];
            stops |= ((double)e[j].rho * (1.0 - 1e-7) > lim ? 1u : 0u) << j;
            hits |= (dist2(tq, p) <= t2 ? 1u : 0u) << j;
        }
        if (hits | stops) {
            const int fh = hits ? __builtin_ctz(hits) : 32, fs = stops ? __builtin_ctz(stops) : 32;
            return fh < fs ? 1 : 0;
        }
    }
    if (max_records < MESH_M) return -1;
    return ((double)hd.rho * (1.0 - 1e-7) > lim) ? 0 : -1;
}

// The same decision from the float32 screening copy of the list (half the bytes per record - the particle kernels are bound
// by the bytes their scattered loads move through the vector cache, tools/probes/ta_probe.hip - and float32 instead of
// float64 arithmetic).  tq is a float32 value already (a pose entry) and so is the header; a vertex v was rounded to
// nearest, |v_f - v| <= 2^-24 |v| per coordinate, and |v| <= |tq| + d, so the true distance d and the one between the
// float32 points d~ satisfy |d - d~| <= E + 1.1e-7 d~ with E = 2.5e-7 (|tq_x| + |tq_y| + |tq_z|); the computed squared
// distance is within 4e-7 (relative) of d~^2.  Hence, with 4e-6 of relative slack on the squares:
//   d2f <= (thr - E)^2 (1 - 4e-6)  =>  d <= thr  (a sure hit: the exact test d2 <= t2 holds - t2 is thr^2 to 1e-16),
//   d2f >  (thr + E)^2 (1 + 4e-6)  =>  d >  thr  (a sure miss; strict, for thr = 0 at the origin: see below),
// and anything between (about one record in 10^5; also NaN) is AMBIGUOUS: the lane returns -2 and the caller decides it
// with mesh_list_check on the float64 records.  "Provably too far" uses a bound that is never below the exact path's
// (a later stop is still a correct stop): rho > (thr + |tq - header| (1 + 1e-6)) (1 + 1e-6).  Events in record order,
// stop before hit on the same record, as in mesh_list_check; 1 / 0 / -1 mean the same.
MD float dist2f3(const float* q, const MeshScr& p) {
    const float d0 = q[0] - p.c[0], d1 = q[1] - p.c[1], d2 = q[2] - p.c[2];
    float d = d0 * d0;
    d = fmaf_(d1, d1, d);
    d = fmaf_(d2, d2, d);
    return d;
}
template <bool PRE = false>
MD int mesh_screen_check(const MeshScr* __restrict__ vscr, int32_t h, const float* tqf, double thr, int max_records,
                         double* lim_out, const MeshScr* pre = nullptr) {
    const MeshScr* vs = vscr + (size_t)h * MESH_REC;
    const MeshScr hd = PRE ? pre[0] : vs[0];
    const float thr_up = __double2float_ru(thr), thr_dn = __double2float_rd(thr);
    const float E = 2.5e-7f * (__builtin_fabsf(tqf[0]) + __builtin_fabsf(tqf[1]) + __builtin_fabsf(tqf[2]));
    const float lo = thr_dn - E, hi = thr_up + E;
    const float t2lo = lo > 0.0f ? lo * lo * (1.0f - 4e-6f) : -1.0f;  // no sure hits when the threshold is within E
    const float t2hi = hi * hi * (1.0f + 4e-6f);
    const float delta_up = __builtin_sqrtf(dist2f3(tqf, hd)) * (1.0f + 1e-6f);
    const float limf = (thr_up + delta_up) * (1.0f + 1e-6f) + 1e-30f;
    if (lim_out) *lim_out = (double)limf;
    for (int s0 = 1; s0 <= max_records; s0 += MESH_BATCH) {
        MeshScr e[MESH_BATCH];
        if (PRE && s0 == 1) {
#pragma unroll
            for (int j = 0; j < MESH_BATCH; ++j) e[j] = pre[1 + j];
        } else {
#pragma unroll
            for (int j = 0; j < MESH_BATCH; ++j) e[j] = vs[s0 + j];
        }
        unsigned hits = 0, stops = 0, amb = 0;
#pragma unroll
        for (int j = 0; j < MESH_BATCH; ++j) {
            const float d = dist2f3(tqf, e[j]);
            // (a strict miss: with thr = 0 and a translation of exactly 0, E = 0 and t2hi = 0 - a vertex ON the particle, d2f = 0, is
            // no miss (0 > 0 is false: kept) and goes to the float64 records; d2f > 0 = t2hi there means v_f != 0, hence v != 0, d > 0)
            const bool hit = d <= t2lo, miss = d > t2hi;
            stops |= (e[j].rho > limf ? 1u : 0u) << j;
            hits |= (hit ? 1u : 0u) << j;
            amb |= ((hit | miss) ? 0u : 1u) << j;
        }
        if (hits | stops | amb) {
            const int fh = hits ? __builtin_ctz(hits) : 32, fs = stops ? __builtin_ctz(stops) : 32, fa = amb ? __builtin_ctz(amb) : 32;
            if (fs <= fh && fs <= fa) return 0;
            return fh < fa ? 1 : -2;
        }
    }
    if (max_records < MESH_M) return -1;
    return hd.rho > limf ? 0 : -1;
}

// Wave-level NN: per-lane hint scan, then the octets serve the lanes it could not certify.
// Must be called by every lane of the wave (`live` = this lane holds a query).
template <bool STATS = false, bool SCREEN = false>
MD bool nn6_wave(const TreeView<Kd6>& tv, const float* q, bool live, int32_t hint, int32_t& idx, float& d2, float* cd,
                 int* n_leaves = nullptr, int* n_nodes = nullptr, int* n_scanned = nullptr, long long* t_solo = nullptr) {
    float best = INFINITY;
    int64_t bi = 0;
    bool done = !live;
    const bool hinted = live && hint >= 0 && (int64_t)hint < tv.K;
    float r_lane = 0.f;
    if (hinted)  // records 0 .. NN_SOLO-1, per lane; `hint` comes back as the pivot whose list was scanned
        done = SCREEN ? nn6_hint_scan_screened(tv, q, hint, best, bi, n_scanned, &r_lane)
                      : nn6_hint_scan(tv, q, hint, best, bi, n_scanned, &r_lane);
    if (t_solo) *t_solo = clock64();
    nn6_coop<SCREEN>(tv, q, hint, r_lane, best, bi, hinted && !done, done);  // the rest, whole wave per lane
    wave_search<Kd6, false, STATS>(tv, q, best, bi, !done, cd, n_leaves, n_nodes);
    idx = (int32_t)bi;
    d2 = best;
    return !done;  // this lane needed the tree search
}

// ---- the mesh's distance field (MeshField, midas_internal.hpp) ---------------------------------------------------------------
// The centre of cell (ix, iy, iz) as ONE float32 expression, used by the builder and by the look-up alike (the stored distance
// belongs to exactly this point).
MD float field_centre(const MeshField& f, int axis, int i) { return fmaf_((float)i + 0.5f, f.h, f.lo[axis]); }

// A look-up in two halves: field_fetch requests the cell's value (early: the translation is known once the motion model is done,
// the answer travels under the nearest-neighbour search), field_decide turns it into 1 (some vertex within thr, certain),
// 0 (none, certain) or -1 (the shell around the threshold, NaN, no field: the exact path decides).
struct FieldProbe { float v = 0.f, rho = 0.f; int state = 2; };  // state 0: inside the grid, 1: outside it, 2: unknown
MD FieldProbe field_fetch(const MeshField& f, const float* tq, bool live) {
    FieldProbe pr;
    if (!f.d || !live) return pr;
    const float gx = (tq[0] - f.lo[0]) * f.inv_h, gy = (tq[1] - f.lo[1]) * f.inv_h, gz = (tq[2] - f.lo[2]) * f.inv_h;
    if (!(gx == gx && gy == gy && gz == gz)) return pr;  // NaN: unknown
    if (!(gx >= 0.f && gy >= 0.f && gz >= 0.f && gx < (float)f.n[0] && gy < (float)f.n[1] && gz < (float)f.n[2])) { pr.state = 1; return pr; }
    const int ix = (int)gx, iy = (int)gy, iz = (int)gz;  // (a value that rounding put into the neighbouring cell is served by that cell: rho says how far its centre is)
    const float dx = tq[0] - field_centre(f, 0, ix), dy = tq[1] - field_centre(f, 1, iy), dz = tq[2] - field_centre(f, 2, iz);
    pr.rho = __builtin_sqrtf(fmaf_(dz, dz, fmaf_(dy, dy, dx * dx)));
    pr.v = f.d[((int64_t)iz * f.n[1] + iy) * f.n[0] + ix];
    pr.state = 0;
    return pr;
}
MD int field_decide(const MeshField& f, const FieldProbe& pr, double thr) {
    // the rule is !(dist > thr): under a NaN or +inf threshold no distance compares greater - a NaN translation's (dist = +inf)
    // neither - and every particle is kept, field or no field, before the exact paths (which find no vertex for such a lane) are asked
    if (!(thr < (double)INFINITY)) return 1;
    if (pr.state == 2 || !(thr >= 0.0)) return -1;
    const float thr_up = __double2float_ru(thr), thr_dn = __double2float_rd(thr);
    if (pr.state == 1) return f.expand > thr_up * 1.00001f ? 0 : -1;  // outside the grown bounding box: farther than `expand` from every vertex
    // true distance d, stored v = float(d_centre) (nearest: 6e-8 relative), rho computed to 4e-7 relative on float32 coordinates
    // that are exact: |d - v| <= rho + 1e-6 (v + rho), and the exact path's comparison is d <= thr up to 1e-16
    const float slack = 2e-6f * (pr.v + pr.rho + thr_up) + 1e-30f;
    if (pr.v + pr.rho + slack <= thr_dn) return 1;
    if (pr.v - pr.rho - slack >= thr_up) return 0;
    return -1;
}

}  // namespace midas
