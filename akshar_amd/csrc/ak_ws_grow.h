// ak_ws_grow.h — the one growth rule of a workspace's "device buffer + capacity" pairs (AkWs).
// Its three runtime calls go through ws_rt_sync / ws_rt_free / ws_rt_malloc: the HIP ones below, or
// the recording stubs of a host test (AK_WS_RT_STUB: tests/ws_grow_host.cpp defines them first).
#pragma once
#include <stdint.h>

#include <algorithm>

#ifndef AK_WS_RT_STUB
#include <hip/hip_runtime.h>
namespace ak {
int set_hip_error(const char *expr, hipError_t e);
inline int ws_rt_sync(hipStream_t st) {
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : set_hip_error("hipStreamSynchronize(st)", e);
}
inline void ws_rt_free(void *p) { (void)hipFree(p); }
inline int ws_rt_malloc(void **p, uint64_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? 0 : set_hip_error("hipMalloc(&buf, bytes)", e);
}
}  // namespace ak
#endif

namespace ak {

// the capacity a buffer of capacity `cap` takes when `need` passes it: exactly the need (the per-row
// lists, the pools), or at least 1.5 x / 2 x what it had (buffers that many calls grow step by step)
enum Growth { GROW_EXACT, GROW_X1_5, GROW_X2 };
inline uint64_t grown_cap(uint64_t need, uint64_t cap, Growth g) {
    return std::max<uint64_t>(need, g == GROW_X2 ? 2 * cap : g == GROW_X1_5 ? cap + cap / 2 : 0);
}

// Grow-only reserve of one pair, capacity in elements of `elem` bytes. Nothing happens (no runtime
// call) when need <= cap. Otherwise, in this order: synchronize the stream (queued work may still read
// the old buffer), free the buffer, set the pair to {null, 0}, allocate, and set the capacity only
// once the allocation has succeeded. On failure the error code is returned (ak_last_error holds the
// runtime's message) and the pair stays {null, 0}, so the next call allocates again: a pointer is
// never null behind a capacity that lets a later, smaller call skip the reserve.
template <class T, class Stream>
int ws_grow(T *&buf, uint64_t &cap, uint64_t need, Stream st, Growth g = GROW_EXACT, uint64_t elem = sizeof(T)) {
    if (need <= cap) return 0;
    int rc = ws_rt_sync(st);
    if (rc) return rc;
    const uint64_t c = grown_cap(need, cap, g);
    ws_rt_free(buf);
    buf = nullptr;
    cap = 0;
    void *p = nullptr;
    if ((rc = ws_rt_malloc(&p, c * elem))) return rc;
    buf = (T *)p;
    cap = c;
    return 0;
}

// ws_reserve's per-row lists (counts, the slow and huge lists): a capacity each, so a failure of the
// second or third allocation leaves every pair consistent
template <class W, class Stream>
int ws_grow_rows(W *w, uint64_t n, Stream st) {
    int rc = ws_grow(w->counts, w->cap_counts, n, st, GROW_X2);
    if (!rc) rc = ws_grow(w->slow_list, w->cap_slow, n, st, GROW_X2);
    if (!rc) rc = ws_grow(w->huge_list, w->cap_huge, n, st, GROW_X2);
    return rc;
}

}  // namespace ak
