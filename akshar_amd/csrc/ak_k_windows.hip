// ak_k_windows.hip — sliding windows and text pairs from ragged id rows, on the device:
//   ak_ids_window_offs  rows -> win_offs[n+1], the first window of every row (k_window_count writes
//                       the rows' window counts into the workspace, ak::scan_counts sums them)
//   ak_ids_windows      rows (+ one partner row each) -> [n_windows, width] ids, attention mask, token
//                       type ids, and per window its row, its start in the row's body and its length
//                       (HF tokenizers' enable_truncation(max_length, stride) with overflow, for single
//                       sequences and for pairs under only_second / only_first / longest_first)
// k_ids_windows is output-driven and write-bound like the kernels of ak_k_dense.hip, whose chunk
// geometry it shares (ak_dense.h): a lane owns 4 consecutive output elements, a wave a contiguous span
// of 256-element chunks. The wave finds the window of its span's first element with one 64-bit division
// and that window's row with one binary search over win_offs; from there it walks forward with a
// 64-entry LDS window of win_offs, as k_ids_pack walks its row starts (every row has at least one
// window, so win_offs is strictly increasing). What a window holds is ak_windows.h's arithmetic: two
// views of a row, chosen per element with selects. A lane places its 4 elements with a rolled loop
// (one copy of the row arithmetic) and gathers their ids afterwards, 4 loads in flight. Every element
// index is 64-bit. One launch, no read-back: the window total is win_offs[n], read on the device.
#include "ak_dense.h"
#include "ak_windows.h"

namespace ak {

constexpr int WIN_VEC_OUT = 1;   // out is 16-byte aligned: whole-lane vector stores
constexpr int WIN_VEC_MASK = 2;  // mask is 4-byte aligned
constexpr int WIN_VEC_TYPE = 4;  // type_ids is 4-byte aligned

__global__ __launch_bounds__(256) void k_window_count(const uint64_t *s_offs, const uint64_t *f_offs, uint64_t n, WinArgs a,
                                                      uint32_t *counts) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    counts[r] = win_count(a, win_row(s_offs, r, a.h, a.t), win_row(f_offs, r, a.h, a.t));
}

// 5 waves per SIMD: 96 VGPRs without scratch (6 would spill)
template <typename T>
__global__ __launch_bounds__(DENSE_BLOCK, 5) void k_ids_windows(const int32_t *s_ids, const uint64_t *s_offs,
                                                             const int32_t *f_ids, const uint64_t *f_offs, uint64_t n,
                                                             const uint64_t *win_offs, WinArgs a, int32_t pad_id, T *out,
                                                             uint64_t cap_windows, uint8_t *mask, uint8_t *type_ids,
                                                             int32_t *sample, int32_t *start, int32_t *lengths, int vec) {
    __shared__ uint64_t s_win[DENSE_WAVES][64];
    uint64_t *win = s_win[threadIdx.x >> 6];
    const int lane = w_lane();
    const uint32_t W = a.W;
    uint64_t nwin = win_offs[n];
    if (nwin > cap_windows) nwin = cap_windows;
    const uint64_t total = nwin * W;
    uint64_t ch, ch_end;
    if (!wave_span(total, &ch, &ch_end)) return;
    const bool pad_left = a.flags & AK_PAD_LEFT, has_f = f_offs != nullptr;
    // (window, column) of the chunk's first element, and of this lane's first element relative to it
    uint64_t w0 = ch * DENSE_CHUNK / W, c0 = ch * DENSE_CHUNK % W;
    const uint32_t lq = (uint32_t)lane * DENSE_VEC / W, lm = (uint32_t)lane * DENSE_VEC % W;
    const uint32_t sq = DENSE_CHUNK / W, sm = DENSE_CHUNK % W;
    // rb: the row of window w0 (the last row whose first window is at or before it)
    uint64_t rb = 0;
    for (uint64_t hi = n; hi - rb > 1;) {
        const uint64_t mid = rb + (hi - rb) / 2;
        if (win_offs[mid] <= w0) rb = mid;
        else hi = mid;
    }
    const uint64_t *fo = has_f ? f_offs : s_offs;  // one batch of offset loads per row, with or without a fixed stream
    for (; ch < ch_end; ++ch) {
        const uint64_t e = ch * DENSE_CHUNK + (uint64_t)lane * DENSE_VEC;
        // the lane's elements are placed in order by a rolled loop (one copy of the row arithmetic, few
        // registers): it records each element's source index and three flag bits; the ids are gathered
        // afterwards, 4 loads in flight at once
        const uint32_t kend = e >= total ? 0u : (total - e < DENSE_VEC ? (uint32_t)(total - e) : DENSE_VEC);
        uint64_t w = w0 + lq, cc = c0 + lm;
        if (cc >= W) {
            cc -= W;
            ++w;
        }
        uint32_t c = (uint32_t)cc, k = 0;
        uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;  // source element index in its stream
        uint32_t live = 0, from_f = 0, second = 0;  // bit k: element k is an id / reads f_ids / lies in the second view
        uint64_t last = rb;    // row of this lane's last element
        uint64_t cur = ~0ull;  // the window that d, len and lead describe: set before their first use,
        WinDesc d;             // since no element's window is ~0
        uint32_t len = 0, lead = 0;
        for (uint64_t wb = rb; w_ballot(k < kend); wb += 63) {
            const uint64_t idx = wb + (uint64_t)lane;
            win[lane] = idx <= n ? win_offs[idx] : ~0ull;
            w_sync();
            int cnt = -1;  // window starts <= the element's window: 1..64 (win[0] <= every open one)
#pragma unroll 1
            for (; k < kend; ++k) {
                if (cnt < 0) {
                    int lo = 1, hi = 64;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (win[mid] <= w) lo = mid + 1;
                        else hi = mid;
                    }
                    cnt = lo;
                } else {
                    while (cnt < 64 && win[cnt] <= w) ++cnt;
                }
                if (cnt >= 64) break;  // past the window's last start: the next round's, as all after it
                const uint64_t row = wb + (uint64_t)(cnt - 1);  // win[cnt - 1] <= w < win[cnt]
                if (w != cur) {
                    const uint64_t sb = s_offs[row], se = s_offs[row + 1], fb = fo[row], fe = fo[row + 1];
                    d = win_desc(a, win_row_of(sb, (uint32_t)(se - sb), a.h, a.t),
                                 win_row_of(has_f ? fb : 0, has_f ? (uint32_t)(fe - fb) : 0u, a.h, a.t), has_f,
                                 (uint32_t)(w - win[cnt - 1]));
                    len = d.v1.len + d.v2.len;
                    lead = pad_left ? W - len : 0u;
                    cur = w;
                }
                if (c == 0) {
                    if (sample) sample[w] = (int32_t)row;
                    if (start) start[w] = (int32_t)d.start;
                    if (lengths) lengths[w] = (int32_t)len;
                }
                const uint32_t j = c - lead;
                const bool is_id = c >= lead && j < len, sec = j >= d.v1.len;
                const uint64_t at = (sec ? d.v2.b : d.v1.b) + win_src(sec ? d.v2 : d.v1, sec ? j - d.v1.len : j);
                a0 = k == 0 ? at : a0;
                a1 = k == 1 ? at : a1;
                a2 = k == 2 ? at : a2;
                a3 = k == 3 ? at : a3;
                live |= (uint32_t)is_id << k;
                second |= (uint32_t)(is_id && sec) << k;
                from_f |= (uint32_t)(sec != d.f1) << k;
                last = row;
                if (++c == W) {
                    c = 0;
                    ++w;
                }
            }
            w_sync();  // every lane is done with the window before the next round overwrites it
        }
        const uint64_t at[DENSE_VEC] = {a0, a1, a2, a3};
        int32_t v[DENSE_VEC], m[DENSE_VEC], ty[DENSE_VEC];
#pragma unroll
        for (uint32_t i = 0; i < DENSE_VEC; ++i) {
            m[i] = live >> i & 1;
            ty[i] = second >> i & 1;
            v[i] = pad_id;
            if (m[i]) v[i] = (from_f >> i & 1 ? f_ids : s_ids)[at[i]];
        }
        put4(out, e, total, v, vec & WIN_VEC_OUT);
        if (mask) put4(mask, e, total, m, vec & WIN_VEC_MASK);
        if (type_ids) put4(type_ids, e, total, ty, vec & WIN_VEC_TYPE);
        rb = w_bcast(last, 63);
        w0 += sq;
        c0 += sm;
        if (c0 >= W) {
            c0 -= W;
            ++w0;
        }
    }
}

static int win_args(const char *fn, const uint64_t *s_offs, const uint64_t *f_offs, uint32_t width, uint32_t stride,
                    uint32_t keep_head, uint32_t keep_tail, uint32_t fixed_cap, int flags, int allowed, WinArgs *a) {
    char msg[160];
    const char *why = nullptr;
    const uint64_t ht = (uint64_t)keep_head + keep_tail;
    if (flags & ~allowed) why = flags & AK_TRUNC_LEFT & ~allowed ? "AK_TRUNC_LEFT: windows slide rightwards only" : "unknown flag bits";
    else if (!s_offs) why = "null s_offs";
    else if (width == 0) why = "width is 0";
    else if (fixed_cap && !f_offs) why = "fixed_cap without a fixed stream";
    else if ((flags & AK_WIN_LONGEST_FIRST) && (flags & AK_WIN_FIXED_LAST)) why = "AK_WIN_LONGEST_FIRST with AK_WIN_FIXED_LAST";
    else if ((flags & AK_WIN_LONGEST_FIRST) && !f_offs) why = "AK_WIN_LONGEST_FIRST without a fixed stream";
    else if ((flags & AK_WIN_LONGEST_FIRST) && stride) why = "AK_WIN_LONGEST_FIRST with a stride";
    else if ((flags & AK_WIN_LONGEST_FIRST) && width < 2 * ht) why = "AK_WIN_LONGEST_FIRST: width below 2 (keep_head + keep_tail)";
    else if (!(flags & AK_WIN_LONGEST_FIRST) && (uint64_t)width <= (uint64_t)fixed_cap + ht + stride)
        why = "width - fixed_cap - keep_head - keep_tail must exceed stride (no room to slide)";
    if (why) {
        snprintf(msg, sizeof(msg), "%s: %s", fn, why);
        return set_error(AK_ERR_ARG, msg);
    }
    *a = WinArgs{width, stride, keep_head, keep_tail, flags & AK_WIN_LONGEST_FIRST ? 0u : fixed_cap, flags};
    return AK_OK;
}

}  // namespace ak

using namespace ak;

extern "C" int ak_ids_window_offs(ak_ws *ws, const uint64_t *s_offs, const uint64_t *f_offs, uint64_t n, uint32_t width,
                                  uint32_t stride, uint32_t keep_head, uint32_t keep_tail, uint32_t fixed_cap, int flags,
                                  uint64_t *win_offs, void *stream) {
    WinArgs a;
    if (!ws) return set_error(AK_ERR_ARG, "ak_ids_window_offs: null workspace");
    if (!win_offs) return set_error(AK_ERR_ARG, "ak_ids_window_offs: null win_offs");
    if (const int rc = win_args("ak_ids_window_offs", s_offs, f_offs, width, stride, keep_head, keep_tail, fixed_cap, flags,
                                AK_WIN_FIXED_LAST | AK_WIN_LONGEST_FIRST | AK_PAD_LEFT | AK_DENSE_I64, &a))
        return rc;
    if (n >= (1ull << 32) * 256) return set_error(AK_ERR_ARG, "ak_ids_window_offs: n is out of range");
    hipStream_t st = (hipStream_t)stream;
    if (n) {
        if (const int rc = ws_reserve(ws, n, st)) return rc;
        k_window_count<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(s_offs, f_offs, n, a, ws->counts);
        HIP_TRY(hipGetLastError());
    }
    return scan_counts(ws, n, win_offs, st);
}

extern "C" int ak_ids_windows(const int32_t *s_ids, const uint64_t *s_offs, const int32_t *f_ids, const uint64_t *f_offs,
                              uint64_t n, const uint64_t *win_offs, uint32_t width, uint32_t stride, uint32_t keep_head,
                              uint32_t keep_tail, uint32_t fixed_cap, int32_t pad_id, int flags, void *out,
                              uint64_t cap_windows, uint8_t *mask, uint8_t *type_ids, int32_t *sample, int32_t *start,
                              int32_t *lengths, void *stream) {
    WinArgs a;
    if (const int rc = win_args("ak_ids_windows", s_offs, f_offs, width, stride, keep_head, keep_tail, fixed_cap, flags,
                                AK_WIN_FIXED_LAST | AK_WIN_LONGEST_FIRST | AK_PAD_LEFT | AK_DENSE_I64, &a))
        return rc;
    if (!s_ids && n) return set_error(AK_ERR_ARG, "ak_ids_windows: null s_ids");
    if (!f_ids != !f_offs) return set_error(AK_ERR_ARG, "ak_ids_windows: f_ids and f_offs go together");
    if (!win_offs) return set_error(AK_ERR_ARG, "ak_ids_windows: null win_offs");
    if (!out) return set_error(AK_ERR_ARG, "ak_ids_windows: null out");
    if (n == 0 || cap_windows == 0) return AK_OK;
    cap_windows = std::min<uint64_t>(cap_windows, (1ull << 62) / width);
    hipStream_t st = (hipStream_t)stream;
    const int vec = (aligned(out, 16) ? WIN_VEC_OUT : 0) | (aligned(mask, 4) ? WIN_VEC_MASK : 0) |
                    (aligned(type_ids, 4) ? WIN_VEC_TYPE : 0);
    const unsigned grid = dense_grid(cap_windows * width);  // the window total is win_offs[n]'s: device-side
    if (flags & AK_DENSE_I64)
        k_ids_windows<int64_t><<<grid, DENSE_BLOCK, 0, st>>>(s_ids, s_offs, f_ids, f_offs, n, win_offs, a, pad_id,
                                                             (int64_t *)out, cap_windows, mask, type_ids, sample, start,
                                                             lengths, vec);
    else
        k_ids_windows<int32_t><<<grid, DENSE_BLOCK, 0, st>>>(s_ids, s_offs, f_ids, f_offs, n, win_offs, a, pad_id,
                                                             (int32_t *)out, cap_windows, mask, type_ids, sample, start,
                                                             lengths, vec);
    HIP_TRY(hipGetLastError());
    return AK_OK;
}
