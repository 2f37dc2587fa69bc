// ak_k_dense.hip — model-ready outputs from the engine's ragged (ids, id_offs) result, on the device:
//   ak_ids_pad   rows -> a [n, width] id matrix, truncated and padded, + attention mask + kept lengths
//                (HF tokenizers enable_truncation + enable_padding with a "<s> $A </s>"-style template:
//                keep_head / keep_tail ids survive truncation)
//   ak_ids_pack  rows (+ a separator) concatenated and cut into [n_blocks, block] blocks, + the
//                per-token position inside its document and the document (row) index
// Both kernels are output-driven and write-bound: the output is cut into chunks of 256 consecutive
// elements, a lane owns 4 consecutive elements of a chunk (one 16-byte store per int32 array, two for
// int64 ids, one dword for the byte mask) and gathers their source ids with dword loads (ids + id_offs[r]
// has no alignment). A wave takes a contiguous span of chunks, so what it needs to find its place in the
// rows (a 64-bit division / a binary search over the row starts) is paid once per wave, not per chunk.
// Every element index is 64-bit: n x width passes 2^32 at the corpus workload's sizes. No workspace,
// no read-back, one launch per call.
#include "ak_dense.h"

namespace ak {

constexpr int VEC_OUT = 1;   // out (and pos, doc) are 16-byte aligned: whole-lane vector stores
constexpr int VEC_MASK = 2;  // mask is 4-byte aligned

// total = rows x W output elements. Element (r, c): with L the row's length, kept = min(L, W) ids and
// W - kept pads (left or right); a truncated row (L > W) keeps its first h and last t ids and W - h - t
// of the ids between, the first ones or (AK_TRUNC_LEFT) the last ones, so the source index of kept
// position j is j, or j + (L - W) from where the cut lies: at W - t (default) or at h (AK_TRUNC_LEFT).
template <typename T>
__global__ __launch_bounds__(DENSE_BLOCK) void k_ids_pad(const int32_t *ids, const uint64_t *id_offs, uint64_t total,
                                                         uint32_t W, int32_t pad_id, uint32_t h, uint32_t t, int flags,
                                                         T *out, uint8_t *mask, int32_t *lengths, int vec) {
    const uint32_t lane = (uint32_t)w_lane();
    uint64_t ch, ch_end;
    if (!wave_span(total, &ch, &ch_end)) return;
    const bool pad_left = flags & AK_PAD_LEFT;
    const uint32_t cut = flags & AK_TRUNC_LEFT ? h : W - t;
    // (row, column) of the chunk's first element, and of this lane's first element relative to it
    uint64_t r0 = ch * DENSE_CHUNK / W, c0 = ch * DENSE_CHUNK % W;
    const uint32_t lq = lane * DENSE_VEC / W, lm = lane * DENSE_VEC % W;
    const uint32_t sq = DENSE_CHUNK / W, sm = DENSE_CHUNK % W;
    for (; ch < ch_end; ++ch) {
        const uint64_t e = ch * DENSE_CHUNK + lane * DENSE_VEC;
        uint64_t r = r0 + lq, cc = c0 + lm;
        if (cc >= W) {
            cc -= W;
            ++r;
        }
        uint32_t c = (uint32_t)cc;
        int32_t v[DENSE_VEC], m[DENSE_VEC];
        uint64_t b = 0, L = 0;
        uint32_t kept = 0;
        bool have = false;  // b, L, kept are row r's
#pragma unroll
        for (uint32_t k = 0; k < DENSE_VEC; ++k) {
            v[k] = pad_id;
            m[k] = 0;
            if (e + k < total) {
                if (!have) {
                    b = id_offs[r];
                    L = id_offs[r + 1] - b;
                    kept = L < W ? (uint32_t)L : W;
                    have = true;
                }
                if (c == 0 && lengths) lengths[r] = (int32_t)kept;
                const uint32_t lead = pad_left ? W - kept : 0u;
                if (c >= lead && c - lead < kept) {
                    const uint32_t j = c - lead;
                    const uint64_t skip = L > W && j >= cut ? L - W : 0;
                    v[k] = ids[b + j + skip];
                    m[k] = 1;
                }
            }
            if (++c == W) {
                c = 0;
                ++r;
                have = false;
            }
        }
        put4(out, e, total, v, vec & VEC_OUT);
        if (mask) put4(mask, e, total, m, vec & VEC_MASK);
        r0 += sq;
        c0 += sm;
        if (c0 >= W) {
            c0 -= W;
            ++r0;
        }
    }
}

// Stream position p belongs to the last row r with start(r) <= p, start(r) = id_offs[r] + r S (S = 1
// with a separator): its ids, then the separator at start(r + 1) - 1. A wave finds the row of its
// span's first element with one uniform binary search, then walks: per round the lanes load the 64
// row starts from the wave's row on into an LDS window, and every lane places its elements in the
// window (a binary search for its first, a walk for the rest). An element past the window's last start
// waits for the next round, which begins at that start; empty rows only take window slots.
template <typename T>
__global__ __launch_bounds__(DENSE_BLOCK) void k_ids_pack(const int32_t *ids, const uint64_t *id_offs, uint64_t n,
                                                          uint32_t block, int32_t sep_id, int32_t pad_id, int drop_last,
                                                          T *out, int32_t *pos, int32_t *doc, uint64_t cap_blocks,
                                                          int vec) {
    __shared__ uint64_t s_win[DENSE_WAVES][64];
    uint64_t *win = s_win[threadIdx.x >> 6];
    const int lane = w_lane();
    const uint64_t S = sep_id >= 0 ? 1u : 0u;
    const uint64_t Tn = id_offs[n] + n * S;
    uint64_t nb = drop_last ? Tn / block : (Tn + block - 1) / block;
    if (nb > cap_blocks) nb = cap_blocks;
    const uint64_t total = nb * block;
    uint64_t ch, ch_end;
    if (!wave_span(total, &ch, &ch_end)) return;
    // rb: a row with start(rb) <= the chunk's first element (the last such row of the span's first chunk)
    uint64_t rb = 0;
    for (uint64_t hi = n; hi - rb > 1;) {
        const uint64_t mid = rb + (hi - rb) / 2;
        if (id_offs[mid] + mid * S <= ch * DENSE_CHUNK) rb = mid;
        else hi = mid;
    }
    for (; ch < ch_end; ++ch) {
        const uint64_t e = ch * DENSE_CHUNK + (uint64_t)lane * DENSE_VEC;
        int32_t v[DENSE_VEC], ps[DENSE_VEC], dc[DENSE_VEC];
        bool need[DENSE_VEC];
#pragma unroll
        for (uint32_t k = 0; k < DENSE_VEC; ++k) {
            v[k] = pad_id;
            ps[k] = 0;
            dc[k] = -1;
            need[k] = e + k < total && e + k < Tn;
        }
        uint64_t last = rb;  // row of this lane's last element
        for (uint64_t wb = rb; w_ballot(need[0] || need[1] || need[2] || need[3]); wb += 63) {
            const uint64_t idx = wb + (uint64_t)lane;
            win[lane] = idx <= n ? id_offs[idx] + idx * S : ~0ull;
            w_sync();
            int cnt = -1;  // window starts <= the element: 1..64 (win[0] <= every open element)
#pragma unroll
            for (uint32_t k = 0; k < DENSE_VEC; ++k) {
                if (!need[k]) continue;
                const uint64_t p = e + k;
                if (cnt < 0) {
                    int lo = 1, hi = 64;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (win[mid] <= p) lo = mid + 1;
                        else hi = mid;
                    }
                    cnt = lo;
                } else {
                    while (cnt < 64 && win[cnt] <= p) ++cnt;
                }
                if (cnt < 64) {  // start(row) = win[cnt - 1] <= p < win[cnt] = start(row + 1)
                    const uint64_t row = wb + (uint64_t)(cnt - 1);
                    v[k] = S && p + 1 == win[cnt] ? sep_id : ids[p - row * S];
                    ps[k] = (int32_t)(p - win[cnt - 1]);
                    dc[k] = (int32_t)row;
                    last = row;
                    need[k] = false;
                }
            }
            w_sync();  // every lane is done with the window before the next round overwrites it
        }
        put4(out, e, total, v, vec & VEC_OUT);
        if (pos) put4(pos, e, total, ps, vec & VEC_OUT);
        if (doc) put4(doc, e, total, dc, vec & VEC_OUT);
        rb = w_bcast(last, 63);
    }
}

}  // namespace ak

using namespace ak;

extern "C" int ak_ids_pad(const int32_t *ids, const uint64_t *id_offs, uint64_t n, uint32_t width, int32_t pad_id,
                          uint32_t keep_head, uint32_t keep_tail, int flags, void *out, uint64_t cap_rows,
                          uint8_t *mask, int32_t *lengths, void *stream) {
    if (flags & ~(AK_PAD_LEFT | AK_TRUNC_LEFT | AK_DENSE_I64)) return set_error(AK_ERR_ARG, "ak_ids_pad: unknown flag bits");
    if (!id_offs) return set_error(AK_ERR_ARG, "ak_ids_pad: null id_offs");
    if (!ids && n) return set_error(AK_ERR_ARG, "ak_ids_pad: null ids");
    if (!out) return set_error(AK_ERR_ARG, "ak_ids_pad: null out");
    if (width == 0) return set_error(AK_ERR_ARG, "ak_ids_pad: width is 0");
    if ((uint64_t)keep_head + keep_tail > width)
        return set_error(AK_ERR_ARG, "ak_ids_pad: keep_head + keep_tail exceeds width (nothing left to truncate)");
    const uint64_t rows = std::min(n, cap_rows);
    if (rows > (1ull << 62) / width) return set_error(AK_ERR_ARG, "ak_ids_pad: n x width is out of range");
    if (rows == 0) return AK_OK;
    const uint64_t total = rows * width;
    hipStream_t st = (hipStream_t)stream;
    const int vec = (aligned(out, 16) ? VEC_OUT : 0) | (aligned(mask, 4) ? VEC_MASK : 0);
    const unsigned grid = dense_grid(total);
    if (flags & AK_DENSE_I64)
        k_ids_pad<int64_t><<<grid, DENSE_BLOCK, 0, st>>>(ids, id_offs, total, width, pad_id, keep_head, keep_tail, flags,
                                                         (int64_t *)out, mask, lengths, vec);
    else
        k_ids_pad<int32_t><<<grid, DENSE_BLOCK, 0, st>>>(ids, id_offs, total, width, pad_id, keep_head, keep_tail, flags,
                                                         (int32_t *)out, mask, lengths, vec);
    HIP_TRY(hipGetLastError());
    return AK_OK;
}

extern "C" uint64_t ak_ids_pack_blocks(uint64_t n_ids, uint64_t n, int has_sep, uint32_t block, int flags) {
    if (block == 0) return 0;
    const uint64_t t = n_ids + (has_sep ? n : 0);
    return flags & AK_PACK_DROP_LAST ? t / block : t / block + (t % block != 0);
}

extern "C" int ak_ids_pack(const int32_t *ids, const uint64_t *id_offs, uint64_t n, uint32_t block, int32_t sep_id,
                           int32_t pad_id, int flags, void *out, int32_t *pos, int32_t *doc, uint64_t cap_blocks,
                           void *stream) {
    if (flags & ~(AK_DENSE_I64 | AK_PACK_DROP_LAST)) return set_error(AK_ERR_ARG, "ak_ids_pack: unknown flag bits");
    if (!id_offs) return set_error(AK_ERR_ARG, "ak_ids_pack: null id_offs");
    if (!ids && n) return set_error(AK_ERR_ARG, "ak_ids_pack: null ids");
    if (!out) return set_error(AK_ERR_ARG, "ak_ids_pack: null out");
    if (block == 0) return set_error(AK_ERR_ARG, "ak_ids_pack: block is 0");
    if (n == 0 || cap_blocks == 0) return AK_OK;  // n == 0: T == 0, no block
    cap_blocks = std::min<uint64_t>(cap_blocks, (1ull << 62) / block);
    hipStream_t st = (hipStream_t)stream;
    const int vec = aligned(out, 16) && aligned(pos, 16) && aligned(doc, 16) ? VEC_OUT : 0;
    const unsigned grid = dense_grid(cap_blocks * block);  // the block count itself is id_offs[n]'s: device-side
    const int drop = flags & AK_PACK_DROP_LAST ? 1 : 0;
    if (flags & AK_DENSE_I64)
        k_ids_pack<int64_t><<<grid, DENSE_BLOCK, 0, st>>>(ids, id_offs, n, block, sep_id, pad_id, drop, (int64_t *)out, pos,
                                                          doc, cap_blocks, vec);
    else
        k_ids_pack<int32_t><<<grid, DENSE_BLOCK, 0, st>>>(ids, id_offs, n, block, sep_id, pad_id, drop, (int32_t *)out, pos,
                                                          doc, cap_blocks, vec);
    HIP_TRY(hipGetLastError());
    return AK_OK;
}
