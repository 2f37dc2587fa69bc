// ak_philox.h — the counter-based generator of the batch kernels that draw (ak_k_mlm.hip: ak_ids_mlm;
// ak_k_spans.hip: ak_ids_spans): one Philox4x32-10 block per element index, so a draw is a pure
// function of (seed, stream_id, element) and needs no state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ak {

struct Philox {
    uint32_t x0, x1, x2, x3;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) of the counter
// (lo32(e), hi32(e), lo32(stream_id), hi32(stream_id)) under the key (k0, k1)
__device__ __forceinline__ Philox philox4x32_10(uint64_t e, uint64_t stream_id, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t c0 = (uint32_t)e, c1 = (uint32_t)(e >> 32), c2 = (uint32_t)stream_id, c3 = (uint32_t)(stream_id >> 32);
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    return Philox{c0, c1, c2, c3};
}

}  // namespace ak
