// ak_spans.h — the two steps of span corruption (include/akshar.h ak_ids_spans) that
// are arithmetic and selection only, kept apart from the kernel (ak_k_spans.hip) so that the host
// helper shares the counts and a host program can step the selection (AK_HOST_EMU: ak_wave.h's 64
// threads; tests/emu/spans_select.cpp forces the equal keys that real draws never give):
//   spans_counts  a row's noise tokens N, spans S and kept tokens M from its length
//   spans_select  the k smallest (key, index) pairs of one segmentation, wave-cooperative
#pragma once
#ifdef AK_HOST_EMU
#include "ak_host_emu.h"
#endif
#include "ak_wave.h"

namespace ak {

struct SpanCounts {
    uint64_t N, S, M;  // S == 0: a row of fewer than 2 ids, copied whole
};

// density_q32 <= 2^32 and mean_q16 >= 65536 (the callers check): no step leaves 64 bits at any L < 2^32
__host__ __device__ inline SpanCounts spans_counts(uint64_t L, uint64_t density_q32, uint32_t mean_q16) {
    if (L < 2) return SpanCounts{0, 0, L};
    uint64_t N = (L * density_q32 + (1ull << 31)) >> 32;
    N = N < 1 ? 1 : N > L - 1 ? L - 1 : N;
    const uint64_t M = L - N, most = N < M ? N : M;
    uint64_t S = (2 * N * 65536 + mean_q16) / (2 * (uint64_t)mean_q16);
    S = S < 1 ? 1 : S > most ? most : S;
    return SpanCounts{N, S, M};
}

constexpr uint32_t SPANS_SELECT_REGS = 8;  // keys a lane keeps in registers: segmentations of up to 512 items

// One segmentation of P items: keys[j], 1 <= j < P, is boundary j's key, in the wave's LDS; entry j
// is read and written by lane j % 64 alone. The cuts are the k (<= P - 1) smallest (key, j) pairs, equal
// keys going to the smaller j: T, the k-th smallest key, by a 32-step search on its bits (a step counts
// the keys below the candidate: in the lanes' registers up to 64 SPANS_SELECT_REGS items, over the LDS
// keys beyond), then every key < T and the first k - count(key < T) positions with
// key == T in index order. On return keys[j], 0 <= j < P, holds the number of cuts <= j (the part that
// item j lies in), cuts[1 .. k] the cuts in ascending order, cuts[0] = 0 and cuts[k + 1] = P. k == 0
// reads no key. The caller puts a w_sync() between this and its reads of cuts[].
__device__ __forceinline__ void spans_select(uint32_t *keys, uint32_t P, uint32_t k, uint16_t *cuts) {
    const uint32_t lane = (uint32_t)w_lane();
    uint32_t T = 0, need = 0;
    if (k && P <= 64 * SPANS_SELECT_REGS) {
        // the usual sizes: every lane keeps its keys in registers, so a step is compares and counts and
        // no LDS round trip; a slot without a key holds 2^32 - 1, which is below no candidate
        uint32_t mine[SPANS_SELECT_REGS];
#pragma unroll
        for (uint32_t c = 0; c < SPANS_SELECT_REGS; ++c) {
            const uint32_t j = c * 64 + lane;
            mine[c] = j >= 1 && j < P ? keys[j] : 0xFFFFFFFFu;
        }
        for (int bit = 31; bit >= -1; --bit) {
            const uint32_t cand = bit >= 0 ? T | 1u << bit : T;
            uint32_t below = 0;
#pragma unroll
            for (uint32_t c = 0; c < SPANS_SELECT_REGS; ++c) below += (uint32_t)w_popc(w_ballot(mine[c] < cand));
            if (bit < 0) need = k - below;
            else if (below < k) T = cand;
        }
    } else if (k) {
        for (int bit = 31; bit >= -1; --bit) {
            // bit -1: the count below T itself, once T is known
            const uint32_t cand = bit >= 0 ? T | 1u << bit : T;
            uint32_t below = 0;
            for (uint32_t j0 = 0; j0 < P; j0 += 64) {
                const uint32_t j = j0 + lane;
                below += (uint32_t)w_popc(w_ballot(j >= 1 && j < P && keys[j] < cand));
            }
            if (bit < 0) need = k - below;
            else if (below < k) T = cand;
        }
    }
    uint32_t cuts_seen = 0, eq_seen = 0;
    for (uint32_t j0 = 0; j0 < P; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool is_key = k != 0 && j >= 1 && j < P;
        const uint32_t key = is_key ? keys[j] : 0u;
        const uint64_t eq = w_ballot(is_key && key == T);
        const bool cut = is_key && (key < T || (key == T && eq_seen + w_rank(eq) < need));
        const uint64_t cm = w_ballot(cut);
        const uint32_t at = 1 + cuts_seen + w_rank(cm);
        if (cut && at <= k) cuts[at] = (uint16_t)j;
        if (j < P) keys[j] = cuts_seen + w_rank_incl(cm);
        cuts_seen += (uint32_t)w_popc(cm);
        eq_seen += (uint32_t)w_popc(eq);
    }
    if (lane == 0) {
        cuts[k + 1] = (uint16_t)P;
        cuts[0] = 0;
    }
}

}  // namespace ak
