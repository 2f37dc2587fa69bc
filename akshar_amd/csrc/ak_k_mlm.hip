// ak_k_mlm.hip — masked-LM batches from a dense id matrix, on the device:
//   ak_ids_mlm   in [rows, width] -> out (masked inputs) and labels, BERT's select / mask / random /
//                keep rule, drawn per element from the counter-based generator Philox4x32-10
// The draw of element e is a pure function of (seed, stream_id, elem_base + e), so a call
// reproduces bit for bit, a batch split into several calls (elem_base) draws what the whole batch
// would, and the kernel needs no state, no workspace and no read-back. With word_start every element
// takes the selection draw (word x0) of its word's leader, so a word is selected whole or not at all;
// what replaces a selected element is always its own draw (x1, x2).
// The kernel shares the chunk geometry of ak_dense.h: a lane owns 4 consecutive elements, a wave a
// contiguous span of 256-element chunks; 16-byte loads and stores where the pointers allow them,
// element accesses otherwise and in the chunk that straddles the capacity. Every element index is
// 64-bit. A lane whose 4 elements are all ineligible (padding) skips the generator altogether.
#include "ak_dense.h"
#include "ak_philox.h"

namespace ak {

constexpr int MLM_VEC_IN = 1;    // in is 16-byte aligned
constexpr int MLM_VEC_OUT = 2;   // out is 16-byte aligned
constexpr int MLM_VEC_LAB = 4;   // labels is 16-byte aligned
constexpr int MLM_VEC_ATTN = 8;  // attn is 4-byte aligned
constexpr uint32_t MLM_NEVER = 8;

struct MlmArgs {
    uint64_t stream_id, elem_base;
    uint64_t t_select, t_mask, t_mask_random;  // thresholds of x0, of x1 for <mask>, of x1 for <mask> or random
    uint32_t k0, k1;                           // the key: lo32(seed), hi32(seed)
    uint32_t W, n_vocab, span, n_never;        // span = rand_hi - rand_lo
    int32_t mask_id, rand_lo, ignore_index;
    int32_t never[MLM_NEVER];
};

// the 4 elements of a lane from a[e..e+3]; those at or past `total` read as 0
template <typename T>
__device__ __forceinline__ void mlm_get4(const T *a, uint64_t e, uint64_t total, T (&v)[DENSE_VEC], bool vec) {
    if (vec && e + DENSE_VEC <= total) {
        if constexpr (sizeof(T) == 4) {
            const int4 q = *reinterpret_cast<const int4 *>(a + e);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            const longlong2 *q = reinterpret_cast<const longlong2 *>(a + e);
            const longlong2 q0 = q[0], q1 = q[1];
            v[0] = q0.x, v[1] = q0.y, v[2] = q1.x, v[3] = q1.y;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < DENSE_VEC; ++k) v[k] = e + k < total ? a[e + k] : (T)0;
    }
}

// ... to a[e..e+3], the values at their full width (ak_dense.h's put4 takes int32 values); nothing at
// or past `total`
template <typename T>
__device__ __forceinline__ void mlm_put4(T *a, uint64_t e, uint64_t total, const T (&v)[DENSE_VEC], bool vec) {
    if (vec && e + DENSE_VEC <= total) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<int4 *>(a + e) = make_int4(v[0], v[1], v[2], v[3]);
        } else {
            longlong2 *q = reinterpret_cast<longlong2 *>(a + e);
            q[0] = make_longlong2(v[0], v[1]);
            q[1] = make_longlong2(v[2], v[3]);
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < DENSE_VEC; ++k)
            if (e + k < total) a[e + k] = v[k];
    }
}

// (x + y) mod W for x, y < W, at any W up to 2^32 - 1
__device__ __forceinline__ uint32_t mlm_add_mod(uint32_t x, uint32_t y, uint32_t W) {
    const uint32_t s = x + y;
    return s >= W || s < x ? s - W : s;
}

template <typename T>
__device__ __forceinline__ bool mlm_never(const MlmArgs &a, T id) {
    bool hit = false;
#pragma unroll
    for (uint32_t k = 0; k < MLM_NEVER; ++k) hit |= k < a.n_never && id == (T)a.never[k];
    return hit;
}

// the id begins a word: flagged in word_start, or outside [0, n_vocab)
template <typename T>
__device__ __forceinline__ bool mlm_flagged(const uint8_t *word_start, uint32_t n_vocab, T id) {
    return (uint64_t)(int64_t)id >= n_vocab || word_start[(uint64_t)id] != 0;
}

// total = min(rows, cap_rows) x W elements
template <typename T>
__global__ __launch_bounds__(DENSE_BLOCK) void k_ids_mlm(const T *in, const uint8_t *attn, uint64_t total, MlmArgs a,
                                                         const uint8_t *word_start, T *out, T *labels, int vec) {
    const uint32_t lane = (uint32_t)w_lane();
    uint64_t ch, ch_end;
    if (!wave_span(total, &ch, &ch_end)) return;
    const uint32_t W = a.W;
    // column of the chunk's first element, and of this lane's first element relative to it
    uint32_t c0 = (uint32_t)(ch * DENSE_CHUNK % W);
    const uint32_t lm = lane * DENSE_VEC % W, sm = DENSE_CHUNK % W;
    for (; ch < ch_end; ++ch) {
        const uint64_t e = ch * DENSE_CHUNK + lane * DENSE_VEC;
        const uint32_t c = mlm_add_mod(c0, lm, W);
        T id[DENSE_VEC], o[DENSE_VEC], lab[DENSE_VEC];
        mlm_get4(in, e, total, id, vec & MLM_VEC_IN);
        uint32_t att = 0x01010101u;
        if (attn) {
            if ((vec & MLM_VEC_ATTN) && e + DENSE_VEC <= total) {
                att = *reinterpret_cast<const uint32_t *>(attn + e);
            } else {
                att = 0;
#pragma unroll
                for (uint32_t k = 0; k < DENSE_VEC; ++k)
                    if (e + k < total) att |= (uint32_t)attn[e + k] << (8 * k);
            }
        }
        bool el[DENSE_VEC];
#pragma unroll
        for (uint32_t k = 0; k < DENSE_VEC; ++k) {
            el[k] = e + k < total && (att >> (8 * k) & 0xffu) != 0 && !mlm_never(a, id[k]);
            o[k] = id[k];
            lab[k] = (T)a.ignore_index;
        }
        if (el[0] || el[1] || el[2] || el[3]) {
            // the selection draw of the lane's first element when its word began in front of the lane:
            // walk left inside the row to the word's leader
            uint32_t lead_x0 = 0;
            bool own = true;  // the element in hand leads its word
            if (word_start && el[0] && c != 0 && !mlm_flagged(word_start, a.n_vocab, id[0])) {
                uint64_t p = e;
                uint32_t cc = c;
                for (;;) {
                    const T q = in[p - 1];
                    if ((attn && attn[p - 1] == 0) || mlm_never(a, q)) break;  // the run of eligible elements begins at p
                    --p;
                    if (--cc == 0 || mlm_flagged(word_start, a.n_vocab, q)) break;
                }
                if (p != e) {
                    own = false;
                    lead_x0 = philox4x32_10(a.elem_base + p, a.stream_id, a.k0, a.k1).x0;
                }
            }
            uint32_t cc = c;
#pragma unroll
            for (uint32_t k = 0; k < DENSE_VEC; ++k) {
                if (k > 0) own = !word_start || cc == 0 || !el[k - 1] || mlm_flagged(word_start, a.n_vocab, id[k]);
                if (el[k]) {
                    const Philox x = philox4x32_10(a.elem_base + e + k, a.stream_id, a.k0, a.k1);
                    if (own) lead_x0 = x.x0;
                    if ((uint64_t)lead_x0 < a.t_select) {
                        lab[k] = id[k];
                        if ((uint64_t)x.x1 < a.t_mask) o[k] = (T)a.mask_id;
                        else if ((uint64_t)x.x1 < a.t_mask_random)
                            o[k] = (T)(int32_t)((uint32_t)a.rand_lo + (uint32_t)(((uint64_t)x.x2 * a.span) >> 32));
                    }
                }
                if (++cc == W) cc = 0;
            }
        }
        mlm_put4(out, e, total, o, vec & MLM_VEC_OUT);
        mlm_put4(labels, e, total, lab, vec & MLM_VEC_LAB);
        c0 = mlm_add_mod(c0, sm, W);
    }
}

}  // namespace ak

using namespace ak;

extern "C" int ak_ids_mlm(const void *in, const uint8_t *attn, uint64_t rows, uint32_t width, uint64_t seed,
                          uint64_t stream_id, uint64_t elem_base, uint64_t t_select, uint64_t t_mask, uint64_t t_random,
                          int32_t mask_id, int32_t rand_lo, int32_t rand_hi, int32_t ignore_index, const int32_t *never,
                          uint32_t n_never, const uint8_t *word_start, uint32_t n_vocab, int flags, void *out,
                          void *labels, uint64_t cap_rows, void *stream) {
    constexpr uint64_t ONE = 1ull << 32;
    if (flags & ~AK_DENSE_I64) return set_error(AK_ERR_ARG, "ak_ids_mlm: unknown flag bits");
    if (rows && !in) return set_error(AK_ERR_ARG, "ak_ids_mlm: null in");
    if (rows && !out) return set_error(AK_ERR_ARG, "ak_ids_mlm: null out");
    if (rows && !labels) return set_error(AK_ERR_ARG, "ak_ids_mlm: null labels");
    if (width == 0) return set_error(AK_ERR_ARG, "ak_ids_mlm: width is 0");
    if (t_select > ONE || t_mask > ONE || t_random > ONE || t_mask + t_random > ONE)
        return set_error(AK_ERR_ARG, "ak_ids_mlm: a threshold, or t_mask + t_random, exceeds 2^32");
    if (t_random && rand_hi <= rand_lo) return set_error(AK_ERR_ARG, "ak_ids_mlm: rand_hi <= rand_lo with t_random > 0");
    if (n_never > MLM_NEVER) return set_error(AK_ERR_ARG, "ak_ids_mlm: more than 8 never ids");
    if (n_never && !never) return set_error(AK_ERR_ARG, "ak_ids_mlm: null never with n_never > 0");
    if (word_start && n_vocab == 0) return set_error(AK_ERR_ARG, "ak_ids_mlm: word_start with n_vocab == 0");
    if ((out && out == in) || (labels && labels == in) || (out && out == labels))
        return set_error(AK_ERR_ARG, "ak_ids_mlm: in, out and labels must be three arrays (the leader search reads neighbours)");
    rows = std::min(rows, cap_rows);
    if (rows > (1ull << 62) / width) return set_error(AK_ERR_ARG, "ak_ids_mlm: rows x width is out of range");
    if (rows == 0) return AK_OK;
    MlmArgs a{};
    a.stream_id = stream_id;
    a.elem_base = elem_base;
    a.t_select = t_select;
    a.t_mask = t_mask;
    a.t_mask_random = t_mask + t_random;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.W = width;
    a.n_vocab = n_vocab;
    a.span = t_random ? (uint32_t)rand_hi - (uint32_t)rand_lo : 0u;
    a.n_never = n_never;
    a.mask_id = mask_id;
    a.rand_lo = rand_lo;
    a.ignore_index = ignore_index;
    for (uint32_t k = 0; k < n_never; ++k) a.never[k] = never[k];
    const uint64_t total = rows * width;
    hipStream_t st = (hipStream_t)stream;
    const int vec = (aligned(in, 16) ? MLM_VEC_IN : 0) | (aligned(out, 16) ? MLM_VEC_OUT : 0) |
                    (aligned(labels, 16) ? MLM_VEC_LAB : 0) | (aligned(attn, 4) ? MLM_VEC_ATTN : 0);
    const unsigned grid = dense_grid(total);
    if (flags & AK_DENSE_I64)
        k_ids_mlm<int64_t><<<grid, DENSE_BLOCK, 0, st>>>((const int64_t *)in, attn, total, a, word_start, (int64_t *)out,
                                                         (int64_t *)labels, vec);
    else
        k_ids_mlm<int32_t><<<grid, DENSE_BLOCK, 0, st>>>((const int32_t *)in, attn, total, a, word_start, (int32_t *)out,
                                                         (int32_t *)labels, vec);
    HIP_TRY(hipGetLastError());
    return AK_OK;
}
