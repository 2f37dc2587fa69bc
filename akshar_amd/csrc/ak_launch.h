// ak_launch.h — what the three tile launchers share (launch_bpe_tiles, launch_spm_tiles, the row
// tiles' launch_ops): each reads "prepare, launch my kernel, fallback waves, tiers, scan, my copy".
#pragma once
#include <stdlib.h>

#include "ak_internal.h"
#include "ak_nfc_wave.h"
#include "ak_tile.h"

namespace ak {

static_assert(TM_SPM == 6, "k_tile_init (ak_tile.h) writes its flag to word 6");
static_assert(CTR_N <= 256, "k_tile_init's first block clears the counters");

// The workspace of a tile launch of n rows: the per-launch words and the per-pass clocks on first
// use, then the lists every launcher's kernels append to or read (fb_list is ws_reserve's slow_list).
inline int tile_ws_prepare(AkWs *w, uint64_t n, hipStream_t st) {
    if (!w->tile_misc) {
        HIP_TRY(hipMalloc(&w->tile_misc, TM_WORDS * 4));
        HIP_TRY(hipMemsetAsync(w->tile_misc, 0, TM_WORDS * 4, st));
    }
    if (g_prof_passes && !w->tile_passprof) {
        HIP_TRY(hipMalloc(&w->tile_passprof, T_NPROF * 8));
        HIP_TRY(hipMemsetAsync(w->tile_passprof, 0, T_NPROF * 8, st));
    }
    const uint64_t nunits = (n + TILE_UNIT - 1) / TILE_UNIT;  // units of the work queue (ak_tile.h tile_first_unit)
    int rc = ws_grow(w->fb2, w->cap_fb2, n, st);
    if (!rc) rc = ws_grow(w->fb3, w->cap_fb3, n, st);
    if (!rc) rc = ws_grow(w->unit_fb, w->cap_unit_fb, nunits, st);
    if (!rc) rc = ws_grow(w->unit_len, w->cap_unit_len, nunits, st);
    return rc;
}

// the TileArgs fields every launcher sets the same way (after tile_ws_prepare)
inline TileArgs tile_args_common(AkWs *w, const RowArgs &a0, uint64_t ntiles) {
    TileArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.ra = a0;
    ta.ra.out_offs = nullptr;
    ta.fb_list = w->slow_list;
    ta.fb_count = w->tile_misc + TM_FB;
    ta.err = w->tile_misc + TM_ERR;
    ta.fb2_list = w->fb2;
    ta.fb2_count = w->tile_misc + TM_FB2;
    ta.next_unit = w->tile_misc + TM_QUEUE;
    ta.unit_fb = w->unit_fb;
    ta.passprof = g_prof_passes ? w->tile_passprof : nullptr;
    ta.ntiles = ntiles;
    return ta;
}

// Grid of a tile kernel: a block per block / 64 units, at most the blocks resident on every CU
// (bpc_env, development aid: fewer blocks per CU than the occupancy limit).
template <class K>
unsigned tile_grid(K kernel, int block, std::atomic<int> &cache, uint64_t ntiles, const char *bpc_env = nullptr) {
    int bpc = blocks_per_cu(kernel, block, cache);
    if (const char *e = bpc_env ? getenv(bpc_env) : nullptr) bpc = std::max(1, std::min(bpc, atoi(e)));
    const uint64_t wpb = (uint64_t)block / 64;
    return (unsigned)std::min<uint64_t>((ntiles + wpb - 1) / wpb, (uint64_t)num_cus() * (uint64_t)bpc);
}

// waves of a fallback-wave kernel's full grid (k_bpe_nfc, k_spm_redo / k_spm_nfc, k_rows_nfc): a
// block of `block` threads per CU
inline uint64_t fallback_waves(int block) { return (uint64_t)num_cus() * (uint64_t)(block / 64); }

// The waves' merge / word pools (tile BPE and SentencePiece share them): per_wave entries for every
// wave slot of the tile grid and of the fallback-wave grid, which a small launch's tile grid may
// not reach (fb_waves 0: the fallback waves use no pool).
inline int tile_pool_reserve(AkWs *w, hipStream_t st, uint64_t tile_waves, uint64_t fb_waves, uint64_t per_wave) {
    return ws_grow(w->bpool, w->cap_bpool, std::max(tile_waves, fb_waves) * per_wave, st);
}

// Before a launcher's fallback-wave kernel: the waves' epoch buffer (bytes_per_wave each), the
// composition hash (built once per workspace, into tfb) and the kernel's grid in *lgrid: no more
// waves than rows, so a small call dispatches a block or two of the 156 KB kernel. Under
// AK_NO_NFC_WAVE (development aid: the one-lane path for every fallback row) *lgrid is 0, the
// launcher skips its kernel, and every fallback row is passed on (ak_ws_fallback_detail).
// hash_build: k_comp_hash_build<>, which the launcher names (a template: its translation unit's copy).
inline int fallback_wave_prepare(AkWs *w, hipStream_t st, uint64_t n, int block, uint64_t bytes_per_wave, uint8_t *&buf,
                                 uint64_t &cap, void (*hash_build)(uint4 *), TileArgs &tfb, unsigned *lgrid) {
    *lgrid = 0;
    if (getenv("AK_NO_NFC_WAVE")) {
        HIP_TRY(hipMemcpyAsync(w->tile_misc + TM_PASSON, w->tile_misc + TM_FB, 4, hipMemcpyDeviceToDevice, st));
        return AK_OK;
    }
    const int rc = ws_grow(buf, cap, fallback_waves(block), st, GROW_EXACT, bytes_per_wave);
    if (rc) return rc;
    if (!w->comp_hash) {
        HIP_TRY(hipMalloc(&w->comp_hash, CH_SLOTS * sizeof(uint4)));
        HIP_TRY(hipMemsetAsync(w->comp_hash, 0, CH_SLOTS * sizeof(uint4), st));
        hash_build<<<(AK_UT_NCOMP + 255) / 256, 256, 0, st>>>(w->comp_hash);
        HIP_TRY(hipGetLastError());
    }
    tfb.comp_hash = w->comp_hash;
    const uint64_t wpb = (uint64_t)block / 64;
    *lgrid = (unsigned)std::min<uint64_t>((uint64_t)num_cus(), (n + wpb - 1) / wpb);
    return AK_OK;
}

// after it: the one-lane kernel takes the rows the waves passed on (fb3)
inline void fallback_wave_passed(AkWs *w, TileArgs &tfb) {
    tfb.fb_list = w->fb3;
    tfb.fb_count = w->tile_misc + TM_PASSON;
}

}  // namespace ak
