// ak_dense.h — what the output-driven dense kernels (ak_k_dense.hip: ak_ids_pad, ak_ids_pack;
// ak_k_windows.hip: ak_ids_windows) share: the chunk geometry, a lane's 4-element store and a wave's
// span of chunks, and the launchers' grid and alignment rules.
#pragma once
#include "ak_internal.h"
#include "ak_wave.h"

namespace ak {

constexpr int DENSE_BLOCK = 256;
constexpr int DENSE_WAVES = DENSE_BLOCK / 64;
constexpr uint32_t DENSE_VEC = 4;                 // output elements per lane and step
constexpr uint32_t DENSE_CHUNK = 64 * DENSE_VEC;  // output elements per wave and step

// the 4 elements of a lane at a[e..e+3]: one vector store per 16 bytes where the array's alignment
// allows (vec) and all 4 lie below `total`, element stores otherwise; nothing at or past `total`
template <typename T>
__device__ __forceinline__ void put4(T *a, uint64_t e, uint64_t total, const int32_t (&v)[DENSE_VEC], bool vec) {
    if (vec && e + DENSE_VEC <= total) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<int4 *>(a + e) = make_int4(v[0], v[1], v[2], v[3]);
        } else if constexpr (sizeof(T) == 8) {
            longlong2 *q = reinterpret_cast<longlong2 *>(a + e);
            q[0] = make_longlong2(v[0], v[1]);
            q[1] = make_longlong2(v[2], v[3]);
        } else {
            *reinterpret_cast<uint32_t *>(a + e) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < DENSE_VEC; ++k)
            if (e + k < total) a[e + k] = (T)v[k];
    }
}

// the chunks [*ch, *end) of this wave: a contiguous span, the same number for every wave
__device__ __forceinline__ bool wave_span(uint64_t total, uint64_t *ch, uint64_t *end) {
    const uint64_t nw = (uint64_t)gridDim.x * DENSE_WAVES;
    const uint64_t wv = (uint64_t)blockIdx.x * DENSE_WAVES + (threadIdx.x >> 6);
    const uint64_t chunks = (total + DENSE_CHUNK - 1) / DENSE_CHUNK;
    const uint64_t per = (chunks + nw - 1) / nw;
    *ch = wv * per;
    *end = *ch + per < chunks ? *ch + per : chunks;
    return *ch < *end;
}

inline unsigned dense_grid(uint64_t elems) {
    const uint64_t want = (elems + (uint64_t)DENSE_CHUNK * DENSE_WAVES - 1) / ((uint64_t)DENSE_CHUNK * DENSE_WAVES);
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(want, 1), (uint64_t)num_cus() * 8);
}

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace ak
