// Stand-alone host program: ak_spans.h's spans_select, the selection step of ak_ids_spans, on one
// emulated wave (ak_wave.h under AK_HOST_EMU: 64 threads), with keys drawn from a few values only, so
// that the tie rule (equal keys go to the smaller index) decides most cuts; 32-bit Philox keys tie once
// in 2^32 draws, so the device tests cannot reach it. Compared with a stable sort. Built and run by
// tests/test_spans_select.py:
//   g++ -O1 -std=c++20 -pthread -DAK_HOST_EMU -I akshar_amd/csrc -o spans_select tests/emu/spans_select.cpp
#include <stdio.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "ak_spans.h"

namespace ak {
thread_local int t_lane;
thread_local EmuWave *t_wave;
}  // namespace ak

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {  // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int run_case(uint32_t P, uint32_t k, uint32_t n_values, uint32_t spread) {
    std::vector<uint32_t> keys(P + 1, 0xDEADBEEFu), orig;
    for (uint32_t j = 1; j < P; ++j) keys[j] = (next_u32() % n_values) * spread + (spread > 1 ? 0xFFFFFF00u : 0u);
    orig = keys;
    std::vector<uint16_t> cuts(k + 3, 0xABCD);
    ak::EmuWave wave;
    std::vector<std::thread> th;
    for (int lane = 0; lane < 64; ++lane)
        th.emplace_back([&, lane] {
            ak::t_lane = lane;
            ak::t_wave = &wave;
            ak::spans_select(keys.data(), P, k, cuts.data());
        });
    for (auto &t : th) t.join();
    // the reference: boundaries by (key, j), the first k of them, ascending
    std::vector<uint32_t> js;
    for (uint32_t j = 1; j < P; ++j) js.push_back(j);
    std::stable_sort(js.begin(), js.end(), [&](uint32_t x, uint32_t y) { return orig[x] < orig[y]; });
    std::vector<uint32_t> want(js.begin(), js.begin() + k);
    std::sort(want.begin(), want.end());
    int bad = 0;
    if (cuts[0] != 0 || cuts[k + 1] != P || cuts[k + 2] != 0xABCD) bad = 1;
    for (uint32_t i = 0; i < k; ++i) bad |= cuts[1 + i] != want[i];
    uint32_t part = 0, next = 0;
    for (uint32_t j = 0; j < P; ++j) {
        if (next < k && want[next] == j) ++part, ++next;
        bad |= keys[j] != part;
    }
    bad |= keys[P] != 0xDEADBEEFu;
    if (bad) fprintf(stderr, "mismatch: P %u k %u values %u spread %u\n", P, k, n_values, spread);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t sizes[] = {0, 1, 2, 3, 64, 65, 129, 321, 512, 513, 577};  // from 513 on: the search over LDS
    for (uint32_t P : sizes) {
        std::vector<uint32_t> ks = {0};
        if (P >= 2) ks = {0, 1, (P - 1) / 2, P - 1};
        for (uint32_t k : ks)
            for (uint32_t n_values : {1u, 3u, 17u}) {
                // spread 1: keys 0 .. n_values - 1 (T is often 0); 0x55: keys near 2^32 - 1, every bit of T in play
                bad |= run_case(P, k, n_values, 1);
                bad |= run_case(P, k, n_values, n_values <= 3 ? 0x55u : 0x0Fu);
                cases += 2;
            }
    }
    printf("%s %d cases\n", bad ? "FAILED" : "ok", cases);
    return bad;
}
