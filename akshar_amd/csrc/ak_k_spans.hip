// ak_k_spans.hip — span-corruption batches (T5's objective) from a dense id matrix, on the device
// (DESIGN.md §4.11):
//   ak_ids_spans   in [rows, width] -> inputs (the kept tokens, every noise span replaced by one
//                  sentinel) and targets (every sentinel followed by its span), + lengths and the mask
// A row's noise token count N and span count S follow from its length alone; which tokens are noise is
// two uniformly random compositions, of the N noise tokens and of the M kept ones into S parts each,
// chosen by the S - 1 smallest of the boundaries' Philox4x32-10 keys (ak_spans.h spans_select). So a
// call reproduces bit for bit and needs no state, workspace or read-back.
// One wave takes one row at a time: keys into LDS (one generator block per boundary gives both
// segmentations' keys), two selections, then the scatter with lanes over consecutive kept items, noise
// items and spans, so a wave's stores run along the row. The LDS is requested per launch for the
// call's width, 6 width + 8 bytes for the wave; AK_SPANS_MAX_WIDTH bounds it.
#include "ak_internal.h"
#include "ak_philox.h"
#include "ak_spans.h"

namespace ak {

constexpr uint64_t SPANS_LDS_MAX = 6ull * AK_SPANS_MAX_WIDTH + 8;
static_assert(SPANS_LDS_MAX <= 65536, "a wave's keys and cut lists must fit the LDS a launch may request");
static_assert(AK_SPANS_MAX_WIDTH <= 65535, "cuts travel as uint16");

struct SpansArgs {
    uint64_t rows, stream_id, elem_base, density_q32;
    uint32_t k0, k1;  // the key: lo32(seed), hi32(seed)
    uint32_t W, mean_q16, in_width, tgt_width;
    int32_t sentinel_first, sentinel_step, eos_id, pad_id, tgt_pad_id;
};

// entries of one cut list: S + 1 <= width / 2 + 1, and spans_select writes cuts[1] even for S == 0
__host__ __device__ inline uint32_t spans_list_cap(uint32_t W) { return W / 2 + 2; }

template <typename T>
__global__ __launch_bounds__(64) void k_ids_spans(const T *in, const int32_t *lengths, SpansArgs a, T *inputs, T *targets,
                                                  int32_t *in_lengths, int32_t *tgt_lengths, uint8_t *noise) {
    extern __shared__ __align__(16) uint32_t spans_lds[];
    const uint32_t lane = (uint32_t)w_lane();
    const uint32_t W = a.W, E = a.eos_id >= 0 ? 1u : 0u;
    uint32_t *keys = spans_lds;  // [W]: the noise segmentation's at [0, N), the other's at [N, L)
    uint16_t *ca = reinterpret_cast<uint16_t *>(spans_lds + W), *cb = ca + spans_list_cap(W);
    for (uint64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const uint64_t base = r * W;
        uint32_t L = W;
        if (lengths) {
            const int32_t l = lengths[r];
            L = l < 0 ? 0u : (uint32_t)l < W ? (uint32_t)l : W;
        }
        const SpanCounts c = spans_counts(L, a.density_q32, a.mean_q16);
        const uint32_t N = (uint32_t)c.N, S = (uint32_t)c.S, M = (uint32_t)c.M;
        uint32_t *ka = keys, *kb = keys + N;
        const uint32_t k = S > 1 ? S - 1 : 0;
        if (k) {
            const uint32_t top = N > M ? N : M;
            for (uint32_t j0 = 0; j0 < top; j0 += 64) {
                const uint32_t j = j0 + lane;
                if (j >= 1 && j < top) {
                    const Philox x = philox4x32_10(a.elem_base + base + j, a.stream_id, a.k0, a.k1);
                    if (j < N) ka[j] = x.x0;
                    if (j < M) kb[j] = x.x1;
                }
            }
        }
        spans_select(ka, N, k, ca);
        spans_select(kb, M, k, cb);
        w_sync();
        const T *src = in + base;
        T *di = inputs + r * a.in_width, *dt = targets + r * a.tgt_width;
        uint8_t *nz = noise ? noise + base : nullptr;
        // kept item v of segment i: column v + a_i -> inputs[v + i]
        for (uint32_t v0 = 0; v0 < M; v0 += 64) {
            const uint32_t v = v0 + lane;
            if (v < M) {
                const uint32_t i = kb[v], col = v + ca[i];
                if (col < L) {  // always: a_i <= N
                    const T x = src[col];
                    if (v + i < a.in_width) di[v + i] = x;
                    if (nz) nz[col] = 0;
                }
            }
        }
        // noise item u of span i: column u + b_(i+1) -> targets[u + i + 1]
        for (uint32_t u0 = 0; u0 < N; u0 += 64) {
            const uint32_t u = u0 + lane;
            if (u < N) {
                const uint32_t i = ka[u], col = u + cb[i + 1];
                if (col < L) {  // always: b_(i+1) <= M
                    const T x = src[col];
                    if (u + i + 1 < a.tgt_width) dt[u + i + 1] = x;
                    if (nz) nz[col] = 1;
                }
            }
        }
        for (uint32_t i0 = 0; i0 < S; i0 += 64) {
            const uint32_t i = i0 + lane;
            if (i < S) {
                const T s = (T)(int32_t)((uint32_t)a.sentinel_first + i * (uint32_t)a.sentinel_step);
                const uint32_t pi = cb[i + 1] + i, pt = ca[i] + i;
                if (pi < a.in_width) di[pi] = s;
                if (pt < a.tgt_width) dt[pt] = s;
            }
        }
        // eos and padding; the mask past the row's length
        for (uint32_t p = M + S + lane; p < a.in_width; p += 64) di[p] = E && p == M + S ? (T)a.eos_id : (T)a.pad_id;
        for (uint32_t p = N + S + lane; p < a.tgt_width; p += 64) dt[p] = E && p == N + S ? (T)a.eos_id : (T)a.tgt_pad_id;
        if (nz)
            for (uint32_t p = L + lane; p < W; p += 64) nz[p] = 0;
        if (lane == 0) {
            if (in_lengths) in_lengths[r] = (int32_t)(M + S + E);
            if (tgt_lengths) tgt_lengths[r] = (int32_t)(N + S + E);
        }
        w_sync();  // the next row's keys and lists overwrite this row's
    }
}

}  // namespace ak

using namespace ak;

extern "C" int ak_ids_spans_lengths(uint32_t L, uint64_t density_q32, uint32_t mean_q16, int has_eos, uint64_t out[4]) {
    if (!out) return set_error(AK_ERR_ARG, "ak_ids_spans_lengths: null out");
    if (density_q32 > 1ull << 32) return set_error(AK_ERR_ARG, "ak_ids_spans_lengths: density_q32 exceeds 2^32");
    if (mean_q16 < 65536) return set_error(AK_ERR_ARG, "ak_ids_spans_lengths: mean_q16 is below 65536 (a mean span of 1)");
    const SpanCounts c = spans_counts(L, density_q32, mean_q16);
    const uint64_t E = has_eos ? 1 : 0;
    out[0] = c.N;
    out[1] = c.S;
    out[2] = c.M + c.S + E;
    out[3] = c.N + c.S + E;
    return AK_OK;
}

extern "C" int ak_ids_spans(const void *in, const int32_t *lengths, uint64_t rows, uint32_t width, uint64_t seed,
                            uint64_t stream_id, uint64_t elem_base, uint64_t density_q32, uint32_t mean_q16,
                            int32_t sentinel_first, int32_t sentinel_step, int32_t eos_id, int32_t pad_id,
                            int32_t tgt_pad_id, int flags, void *inputs, uint32_t in_width, void *targets,
                            uint32_t tgt_width, int32_t *in_lengths, int32_t *tgt_lengths, uint8_t *noise, uint64_t cap_rows,
                            void *stream) {
    if (flags & ~AK_DENSE_I64) return set_error(AK_ERR_ARG, "ak_ids_spans: unknown flag bits");
    if (rows && !in) return set_error(AK_ERR_ARG, "ak_ids_spans: null in");
    if (rows && !inputs) return set_error(AK_ERR_ARG, "ak_ids_spans: null inputs");
    if (rows && !targets) return set_error(AK_ERR_ARG, "ak_ids_spans: null targets");
    if (width == 0 || in_width == 0 || tgt_width == 0) return set_error(AK_ERR_ARG, "ak_ids_spans: width, in_width or tgt_width is 0");
    if (width > AK_SPANS_MAX_WIDTH) return set_error(AK_ERR_ARG, "ak_ids_spans: width exceeds AK_SPANS_MAX_WIDTH");
    if (density_q32 > 1ull << 32) return set_error(AK_ERR_ARG, "ak_ids_spans: density_q32 exceeds 2^32");
    if (mean_q16 < 65536) return set_error(AK_ERR_ARG, "ak_ids_spans: mean_q16 is below 65536 (a mean span of 1)");
    const void *arrays[] = {in, lengths, inputs, targets, in_lengths, tgt_lengths, noise};  // 2 inputs, then the outputs
    for (int i = 2; i < 7; ++i)
        for (int j = 0; j < i; ++j)
            if (arrays[i] && arrays[i] == arrays[j])
                return set_error(AK_ERR_ARG, "ak_ids_spans: an output is in, lengths or another output");
    rows = std::min(rows, cap_rows);
    if (rows > (1ull << 62) / std::max(width, std::max(in_width, tgt_width)))
        return set_error(AK_ERR_ARG, "ak_ids_spans: rows x width is out of range");
    if (rows == 0) return AK_OK;
    SpansArgs a{};
    a.rows = rows;
    a.stream_id = stream_id;
    a.elem_base = elem_base;
    a.density_q32 = density_q32;
    a.k0 = (uint32_t)seed;
    a.k1 = (uint32_t)(seed >> 32);
    a.W = width;
    a.mean_q16 = mean_q16;
    a.in_width = in_width;
    a.tgt_width = tgt_width;
    a.sentinel_first = sentinel_first;
    a.sentinel_step = sentinel_step;
    a.eos_id = eos_id;
    a.pad_id = pad_id;
    a.tgt_pad_id = tgt_pad_id;
    hipStream_t st = (hipStream_t)stream;
    // one wave per block; as many blocks as a CU holds waves, each taking rows in turn
    const unsigned grid = (unsigned)std::min<uint64_t>(rows, (uint64_t)num_cus() * 32);
    const size_t lds = 4 * (size_t)width + 2 * 2 * (size_t)spans_list_cap(width);
    if (flags & AK_DENSE_I64)
        k_ids_spans<int64_t><<<grid, 64, lds, st>>>((const int64_t *)in, lengths, a, (int64_t *)inputs, (int64_t *)targets,
                                                    in_lengths, tgt_lengths, noise);
    else
        k_ids_spans<int32_t><<<grid, 64, lds, st>>>((const int32_t *)in, lengths, a, (int32_t *)inputs, (int32_t *)targets,
                                                    in_lengths, tgt_lengths, noise);
    HIP_TRY(hipGetLastError());
    return AK_OK;
}
