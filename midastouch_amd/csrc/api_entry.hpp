// api_entry.hpp - what the api*.hip units share: the export attribute, the entry guard, the table block of the pipelined step
// and the condition of the sparse scoring.
#pragma once
#include "midas_internal.hpp"

#define MIDAS_EXPORT __attribute__((visibility("default")))

int scratch_reset(midas_ctx* ctx);  // api.hip: rewinds the scratch to its first chunk

// entry guard: bind the device, reset the scratch bump pointer
#define MIDAS_ENTER(ctx)                                                     \
    do {                                                                     \
        if (!(ctx)) return MIDAS_ERR_INVALID;                                \
        MIDAS_HIP_CHECK((ctx), hipSetDevice((ctx)->device));                 \
        int _rc = scratch_reset(ctx);                                        \
        if (_rc) return _rc;                                                 \
    } while (0)

namespace midas {

// Layout of the caller's table block (doubles).  The per-slot and per-chunk arrays are padded to multiples of 16 so
// that the lazy front may fetch whole 16-value lines with aligned 16-byte loads (values past the data are ignored).
// with_blocks = false: the block of one shard, the same layout without the per-block arrays (those live in the exchange record r1)
inline TailTables tables_of(double* t, int64_t N, bool with_blocks = true) {
    const int64_t ng = ceil_div(N, SCAN_CHUNK), nb = ceil_div(N, SCAN_BLOCK);
    const int64_t Np = ceil_div(N, 16) * 16, ngp = ceil_div(ng, 16) * 16;
    TailTables tb;
    tb.e = t; tb.x_raw = tb.e + Np; tb.lp = tb.x_raw + Np; tb.lp_raw = tb.lp + Np;
    tb.gend = tb.lp_raw + Np; tb.gend_raw = tb.gend + ngp;
    tb.ggend = tb.gend_raw + ngp; tb.ggend_raw = tb.ggend + 16 * nb;
    tb.bsum_e = tb.ggend_raw + 16 * nb; tb.btot = tb.bsum_e + nb; tb.btot_raw = tb.btot + nb; tb.bmax = tb.btot_raw + nb; tb.bmin = tb.bmax + nb;
    if (!with_blocks) tb.bsum_e = tb.btot = tb.btot_raw = tb.bmax = tb.bmin = nullptr;
    return tb;
}
// size of one trajectory's table block: the end of the last array, padded to whole 128-byte lines
// (4 Np + 2 ngp + (2 x 16 + 5) nb = ... + 37 nb doubles before the padding)
inline int64_t tables_doubles(int64_t N) {
    const TailTables tb = tables_of(nullptr, N);
    return ceil_div((tb.bmin - tb.e) + ceil_div(N, SCAN_BLOCK), 16) * 16;
}

// a codebook and code the particle waves can score sparsely (float32 rows of 2 - 16 64-value pieces, 16-byte loads)
inline bool sparse_score_ok(const midas_codebook* cb, const double* code_dev) {
    return cb->dtype == MIDAS_F32 && (cb->D == 128 || cb->D == 256 || cb->D == 512 || cb->D == 1024) && (uintptr_t)cb->emb % 16 == 0 &&
           (uintptr_t)code_dev % 16 == 0;
}

}  // namespace midas
