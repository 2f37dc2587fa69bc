// ak_windows.h — the per-row arithmetic of ak_ids_window_offs / ak_ids_windows (include/akshar.h),
// shared by k_window_count and k_ids_windows. Plain integer code with no device intrinsics.
//
// A window is two segments, each a *view* of one row: the row's first `hh` ids, `nb` ids of its body
// from body index `off` on, and its last ids. Position j of a view reads row index
//   j + (j >= hh ? off : 0) + (j >= hh + nb ? skip : 0),      skip = body length - off - nb,
// which covers the cut fixed row (off = 0), a sliding window (off = k step) and both halves of a
// LONGEST_FIRST pair. A row has fewer than 2^32 ids, so every in-row quantity is 32-bit.
#pragma once
#include <stdint.h>

#include "akshar.h"

#ifndef AK_WIN_HD
#define AK_WIN_HD __host__ __device__ __forceinline__
#endif

namespace ak {

struct WinArgs {
    uint32_t W, stride, h, t, fixed_cap;
    int flags;
};

// one row of a stream: its start in ids, its length, the template ids it carries, its body length
struct WinRow {
    uint64_t b;
    uint32_t L, h, t, B;
};

AK_WIN_HD WinRow win_row_of(uint64_t b, uint32_t L, uint32_t h, uint32_t t) {
    WinRow x;
    x.b = b;
    x.L = L;
    const bool keep = (uint64_t)L >= (uint64_t)h + t;  // a row shorter than h + t carries no template
    x.h = keep ? h : 0u;
    x.t = keep ? t : 0u;
    x.B = L - x.h - x.t;
    return x;
}

// row r of a stream; no stream (offs == NULL): an empty row
AK_WIN_HD WinRow win_row(const uint64_t *offs, uint64_t r, uint32_t h, uint32_t t) {
    return offs ? win_row_of(offs[r], (uint32_t)(offs[r + 1] - offs[r]), h, t) : win_row_of(0, 0, h, t);
}

struct WinView {
    uint64_t b;  // the row's start in its stream
    uint32_t hh, off, nb, skip, len;
};

AK_WIN_HD WinView win_view(const WinRow &x, uint32_t hh, uint32_t tt, uint32_t off, uint32_t nb) {
    return WinView{x.b, hh, off, nb, x.L - hh - tt - off - nb, hh + nb + tt};
}

AK_WIN_HD uint32_t win_src(const WinView &v, uint32_t j) { return j + (j >= v.hh ? v.off : 0u) + (j >= v.hh + v.nb ? v.skip : 0u); }

// the fixed row cut to fixed_cap ids as ak_ids_pad cuts on the right (a cap below h + t cuts plainly)
AK_WIN_HD WinView win_fixed(const WinRow &f, uint32_t fixed_cap) {
    if (f.L <= fixed_cap) return win_view(f, f.h, f.t, 0, f.B);
    const bool keep = fixed_cap >= f.h + f.t;
    const uint32_t hh = keep ? f.h : 0u, tt = keep ? f.t : 0u;
    return win_view(f, hh, tt, 0, fixed_cap - hh - tt);
}

// ids per window body (C) of a sliding row next to a fixed segment of lf ids; step = C - stride >= 1
// by the host's argument rule
AK_WIN_HD uint32_t win_room(const WinArgs &a, const WinRow &s, uint32_t lf) { return a.W - lf - s.h - s.t; }

AK_WIN_HD uint32_t win_count(const WinArgs &a, const WinRow &s, const WinRow &f) {
    if (a.flags & AK_WIN_LONGEST_FIRST) return 1;
    const uint32_t C = win_room(a, s, win_fixed(f, a.fixed_cap).len), step = C - a.stride;
    return s.B <= C ? 1u : 1u + (uint32_t)(((uint64_t)(s.B - C) + step - 1) / step);  // <= B: 32 bits hold it
}

// LONGEST_FIRST: the body ids kept of the fixed (*nf) and the sliding (*ns) row, HF tokenizers' rule
AK_WIN_HD void win_longest(const WinArgs &a, const WinRow &s, const WinRow &f, uint32_t *nf, uint32_t *ns) {
    const uint32_t M = a.W - f.h - f.t - s.h - s.t;
    uint32_t n1 = f.B, n2 = s.B;
    if ((uint64_t)n1 + n2 > M) {
        const bool swap = n1 > n2;  // n1: the shorter body
        if (swap) {
            const uint32_t x = n1;
            n1 = n2;
            n2 = x;
        }
        n2 = n1 > M ? n1 : (n1 > M - n1 ? n1 : M - n1);
        if ((uint64_t)n1 + n2 > M) {
            n1 = M / 2;
            n2 = n1 + M % 2;
        }
        if (swap) {
            const uint32_t x = n1;
            n1 = n2;
            n2 = x;
        }
    }
    *nf = n1;
    *ns = n2;
}

// window k of a row: its two views in output order, the stream of the first one, and `start`
struct WinDesc {
    WinView v1, v2;
    bool f1;  // the first view reads the fixed stream
    uint32_t start;
};

AK_WIN_HD WinDesc win_desc(const WinArgs &a, const WinRow &s, const WinRow &f, bool has_f, uint32_t k) {
    WinDesc d;
    WinView vf, vs;
    if (a.flags & AK_WIN_LONGEST_FIRST) {
        uint32_t nf, ns;
        win_longest(a, s, f, &nf, &ns);
        vf = win_view(f, f.h, f.t, 0, nf);
        vs = win_view(s, s.h, s.t, 0, ns);
        d.start = 0;
    } else {
        vf = win_fixed(f, a.fixed_cap);
        const uint32_t C = win_room(a, s, vf.len), off = k * (C - a.stride);
        const uint32_t rest = s.B - off;  // k < win_count: off < B, or off == 0 == B
        vs = win_view(s, s.h, s.t, off, rest < C ? rest : C);
        d.start = off;
    }
    d.f1 = has_f && !(a.flags & AK_WIN_FIXED_LAST);  // without a fixed stream the sliding view is the first
    d.v1 = d.f1 ? vf : vs;
    d.v2 = d.f1 ? vs : vf;
    return d;
}

}  // namespace ak
