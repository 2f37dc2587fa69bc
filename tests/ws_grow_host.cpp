// Host program for tests/test_ws_grow.py: akshar_amd/csrc/ak_ws_grow.h with its three runtime calls
// replaced by stubs that record every call and can fail the k-th allocation. `ws_grow_host <case>`
// prints what went wrong and exits non-zero; no GPU, no HIP headers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

namespace ak {
struct Call { char kind; void *p; uint64_t bytes; };  // 'S' synchronize, 'F' free, 'M' allocation (p null: failed)
static std::vector<Call> g_log;
static std::map<void *, uint64_t> g_live;  // allocation -> bytes
static int g_mallocs = 0, g_fail_at = -1, g_bad_free = 0;
constexpr int STUB_ERR = -2;  // AK_ERR_HIP, what set_hip_error returns

inline int ws_rt_sync(int) {
    g_log.push_back({'S', nullptr, 0});
    return 0;
}
inline void ws_rt_free(void *p) {
    g_log.push_back({'F', p, 0});
    if (!p) return;  // (hipFree(nullptr) is a no-op too)
    if (!g_live.erase(p)) ++g_bad_free;  // freed twice, or never allocated
    else free(p);
}
inline int ws_rt_malloc(void **p, uint64_t bytes) {
    *p = nullptr;
    if (g_mallocs++ == g_fail_at) {
        g_log.push_back({'M', nullptr, bytes});
        return STUB_ERR;
    }
    *p = malloc(bytes ? bytes : 1);
    g_live[*p] = bytes;
    g_log.push_back({'M', *p, bytes});
    return 0;
}
}  // namespace ak

#define AK_WS_RT_STUB 1
#include "ak_ws_grow.h"

using namespace ak;

static int g_failed = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            ++g_failed;                                              \
        }                                                            \
    } while (0)

static std::string kinds() {
    std::string s;
    for (const Call &c : g_log) s += c.kind;
    return s;
}
// a pair is sound: null behind capacity 0, or a live allocation that holds the capacity
template <class T>
static bool sound(const T *buf, uint64_t cap, uint64_t elem = sizeof(T)) {
    if (!buf) return cap == 0;
    const auto it = g_live.find((void *)buf);
    return it != g_live.end() && cap > 0 && it->second == cap * elem;
}
// the end of a case: whatever the pairs still hold is freed, and then nothing is live, nothing was freed twice
static void finish(std::vector<void *> held) {
    for (void *p : held) ws_rt_free(p);
    CHECK(g_live.empty());
    CHECK(g_bad_free == 0);
}

static void case_noop() {
    uint32_t *buf = nullptr;
    uint64_t cap = 0;
    CHECK(ws_grow(buf, cap, 10, 0) == 0 && cap == 10);
    g_log.clear();
    for (uint64_t need : {0ull, 1ull, 9ull, 10ull}) CHECK(ws_grow(buf, cap, need, 0, GROW_X2) == 0);
    CHECK(g_log.empty() && cap == 10 && sound(buf, cap));
    finish({buf});
}

static void case_order() {
    uint32_t *buf = nullptr;
    uint64_t cap = 0;
    CHECK(ws_grow(buf, cap, 10, 0) == 0);
    CHECK(kinds() == "SFM" && g_log[1].p == nullptr && g_log[2].bytes == 40);  // first use: nothing to free
    void *old = buf;
    g_log.clear();
    CHECK(ws_grow(buf, cap, 11, 0) == 0);
    CHECK(kinds() == "SFM" && g_log[1].p == old && g_log[2].p == (void *)buf && g_log[2].bytes == 44);
    CHECK(cap == 11 && sound(buf, cap));
    uint8_t *epochs = nullptr;  // capacity in units of `elem` bytes (the fallback waves' epoch buffers)
    uint64_t waves = 0;
    CHECK(ws_grow(epochs, waves, 7, 0, GROW_EXACT, 256) == 0 && waves == 7 && sound(epochs, waves, 256));
    finish({buf, epochs});
}

static void case_fail() {
    uint32_t *buf = nullptr;
    uint64_t cap = 0;
    CHECK(ws_grow(buf, cap, 100, 0) == 0);
    g_fail_at = g_mallocs;  // the next allocation fails
    g_log.clear();
    CHECK(ws_grow(buf, cap, 200, 0) == STUB_ERR);
    CHECK(buf == nullptr && cap == 0 && kinds() == "SFM" && g_live.empty());
    g_log.clear();
    CHECK(ws_grow(buf, cap, 50, 0) == 0);  // fewer rows than the capacity before the failure: allocates again
    CHECK(kinds() == "SFM" && buf != nullptr && cap == 50 && sound(buf, cap));
    finish({buf});
}

struct Rows {  // the fields of AkWs that ws_grow_rows touches
    uint32_t *counts = nullptr, *slow_list = nullptr, *huge_list = nullptr;
    uint64_t cap_counts = 0, cap_slow = 0, cap_huge = 0;
};
static bool rows_sound(const Rows &w) {
    return sound(w.counts, w.cap_counts) && sound(w.slow_list, w.cap_slow) && sound(w.huge_list, w.cap_huge);
}

static void case_rows() {
    for (int k = 0; k < 3; ++k) {  // the 1st, 2nd, 3rd allocation of a growing call fails
        Rows w;
        CHECK(ws_grow_rows(&w, 100, 0) == 0 && rows_sound(w));
        CHECK(w.cap_counts == 100 && w.cap_slow == 100 && w.cap_huge == 100);
        g_fail_at = g_mallocs + k;
        CHECK(ws_grow_rows(&w, 300, 0) == STUB_ERR);
        CHECK(rows_sound(w));  // no pointer null behind a non-zero capacity
        const uint32_t *p[3] = {w.counts, w.slow_list, w.huge_list};
        CHECK(p[k] == nullptr);
        CHECK(ws_grow_rows(&w, 50, 0) == 0 && rows_sound(w));  // a later, smaller call
        CHECK(w.counts && w.slow_list && w.huge_list);
        CHECK(w.cap_counts >= 50 && w.cap_slow >= 50 && w.cap_huge >= 50);
        CHECK(ws_grow_rows(&w, 300, 0) == 0 && rows_sound(w));
        CHECK(w.cap_counts >= 300 && w.cap_slow >= 300 && w.cap_huge >= 300);
        finish({w.counts, w.slow_list, w.huge_list});
    }
}

// The capacities after each need of 1, 64, 65, 64, 1000, 1001, 3, worked out by hand from the code
// this replaced: exact `if (cap < need) cap = need`; x1.5 `max(need, cap + cap / 2)` (stage, stage8);
// x2 `max(need, 2 * cap)` (ws_reserve).
static void case_policy() {
    const uint64_t needs[7] = {1, 64, 65, 64, 1000, 1001, 3};
    const uint64_t want[3][7] = {{1, 64, 65, 65, 1000, 1001, 1001},
                                 {1, 64, 96, 96, 1000, 1500, 1500},
                                 {1, 64, 128, 128, 1000, 2000, 2000}};
    const Growth g[3] = {GROW_EXACT, GROW_X1_5, GROW_X2};
    for (int j = 0; j < 3; ++j) {
        uint64_t *buf = nullptr;
        uint64_t cap = 0;
        for (int i = 0; i < 7; ++i) {
            CHECK(ws_grow(buf, cap, needs[i], 0, g[j]) == 0);
            if (cap != want[j][i]) printf("policy %d need %llu: cap %llu, want %llu\n", j, (unsigned long long)needs[i],
                                          (unsigned long long)cap, (unsigned long long)want[j][i]);
            CHECK(cap == want[j][i] && sound(buf, cap));
        }
        finish({buf});
    }
}

int main(int argc, char **argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    if (c == "noop") case_noop();
    else if (c == "order") case_order();
    else if (c == "fail") case_fail();
    else if (c == "rows") case_rows();
    else if (c == "policy") case_policy();
    else { printf("unknown case '%s'\n", c.c_str()); return 2; }
    printf("%s: %s\n", c.c_str(), g_failed ? "FAILED" : "ok");
    return g_failed ? 1 : 0;
}
