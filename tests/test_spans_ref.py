"""Span-corruption batches (include/akshar.h ak_ids_spans) without a GPU: the definition restated in
numpy on top of tests/test_mlm_ref.py's Philox restatement (pinned there to Random123's known answers).

  - span_counts and np_spans restate the header: the counts, the cuts by np.lexsort over (key, j), the
    layout and the outputs;
  - properties of the reference: inputs and targets reassemble every row, the lengths are the
    formulas', a row starts with a kept token and ends with noise, no span or segment is empty, the
    mask counts N, and the two possible cuts of a 3-token segmentation come up evenly;
  - through the library on the CPU: ak_ids_spans_lengths, T5's known input / target lengths, every
    AK_ERR_ARG case and the Python layer's ValueErrors.

tests/test_gpu_spans.py holds the kernel to np_spans, element for element. There is no golden fixture:
the reference project has no span-corruption collator to record, and T5's draws come from another
generator.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_mlm_ref import M32, ONE, np_philox4x32_10, threshold

MAX_WIDTH = 4096
DENSE_I64 = 4


def mean_q16(mean):
    return int(round(mean * 65536))


# ------------------------------------------------------------------------------------------ restatements
def span_counts(L, density_q32, mq16, has_eos):
    """(N, S, in_len, tgt_len) of a row of L ids, in Python integers."""
    E = int(bool(has_eos))
    if L < 2:
        return 0, 0, L + E, E
    N = min(max((L * density_q32 + (1 << 31)) >> 32, 1), L - 1)
    M = L - N
    S = min(max((2 * N * 65536 + mq16) // (2 * mq16), 1), min(N, M))
    return N, S, M + S + E, N + S + E


def np_cuts(keys, P, S):
    """[c_0 = 0, c_1 < ... < c_(S-1), c_S = P]: the S - 1 boundaries j in 1 .. P-1 with the smallest
    (keys[j], j), sorted."""
    if S < 1:
        return [0]
    js = np.arange(1, P)
    order = np.lexsort((js, keys[1:P]))  # the last key is the primary one
    return [0] + sorted(js[order[:S - 1]].tolist()) + [P]


def wrap32(v):
    return (v + (1 << 31)) % ONE - (1 << 31)


def np_spans(ids, lengths=None, *, seed=0, stream_id=0, elem_base=0, density_q32, mq16, sentinel_first, sentinel_step=-1,
             eos_id=-1, pad_id=0, tgt_pad_id=-100, in_width=None, tgt_width=None):
    """As include/akshar.h defines ak_ids_spans: a dict of inputs [rows, in_width], targets [rows,
    tgt_width] (ids' dtype), in_lengths, tgt_lengths (int32 [rows]) and noise (uint8, ids' shape). The
    default widths are what a full row needs."""
    ids = np.asarray(ids)
    rows, width = ids.shape
    E = int(eos_id >= 0)
    full = span_counts(width, density_q32, mq16, E)
    in_width = full[2] if in_width is None else in_width
    tgt_width = full[3] if tgt_width is None else tgt_width
    e = np.arange(rows * width, dtype=np.uint64) + np.uint64(elem_base)  # wraps modulo 2^64
    x0, x1, _, _ = np_philox4x32_10(e & np.uint64(M32), e >> np.uint64(32), stream_id & M32, stream_id >> 32, seed & M32,
                                    seed >> 32)
    x0, x1 = x0.reshape(rows, width), x1.reshape(rows, width)
    inputs = np.full((rows, in_width), pad_id, dtype=ids.dtype)
    targets = np.full((rows, tgt_width), tgt_pad_id, dtype=ids.dtype)
    in_lengths, tgt_lengths = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32)
    noise = np.zeros((rows, width), dtype=np.uint8)
    for r in range(rows):
        L = width if lengths is None else min(max(int(lengths[r]), 0), width)
        N, S, in_len, tgt_len = span_counts(L, density_q32, mq16, E)
        M = L - N
        a, b = np_cuts(x0[r], N, S), np_cuts(x1[r], M, S)
        row_in, row_tgt = [], []
        for i in range(S):
            row_in += [ids[r, v + a[i]] for v in range(b[i], b[i + 1])] + [wrap32(sentinel_first + i * sentinel_step)]
            cols = [u + b[i + 1] for u in range(a[i], a[i + 1])]
            row_tgt += [wrap32(sentinel_first + i * sentinel_step)] + [ids[r, c] for c in cols]
            noise[r, cols] = 1
        if S == 0:
            row_in = list(ids[r, :L])
        row_in += [eos_id] * E
        row_tgt += [eos_id] * E
        assert len(row_in) == in_len and len(row_tgt) == tgt_len
        k = min(in_len, in_width)
        inputs[r, :k] = row_in[:k]
        k = min(tgt_len, tgt_width)
        targets[r, :k] = row_tgt[:k]
        in_lengths[r], tgt_lengths[r] = in_len, tgt_len
    return {"inputs": inputs, "targets": targets, "in_lengths": in_lengths, "tgt_lengths": tgt_lengths, "noise": noise}


def reassemble(inputs, targets, sentinels, L):
    """The row that (inputs, targets) came from: every sentinel of the inputs replaced by the ids that
    follow it in the targets. `sentinels`: the ids that are sentinels, in order."""
    spans, cur = {}, None
    for t in targets:
        if t in sentinels:
            cur = t
            spans[cur] = []
        else:
            spans[cur].append(t)
    row = []
    for t in inputs:
        row += spans[t] if t in sentinels else [t]
    assert len(row) == L
    return row


# ------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("density,mean", [(0.15, 3.0), (0.5, 1.0), (0.5, 1.5), (0.3, 7.5), (0.0, 3.0), (1.0, 2.0)])
def test_reference_properties(density, mean):
    rng = np.random.default_rng(int(density * 100 + mean))
    width, rows = 97, 60
    ids = rng.integers(0, 1000, size=(rows, width)).astype(np.int64)  # below every sentinel
    lengths = rng.integers(0, width + 1, size=rows)
    lengths[:6] = (0, 1, 2, 3, width, width - 1)
    dq, mq = threshold(density), mean_q16(mean)
    first = 5000
    res = np_spans(ids, lengths, seed=5, stream_id=6, elem_base=ONE - 50, density_q32=dq, mq16=mq, sentinel_first=first,
                   sentinel_step=-1, eos_id=2000, pad_id=-1, tgt_pad_id=-100, in_width=2 * width, tgt_width=2 * width)
    for r in range(rows):
        L = int(lengths[r])
        N, S, in_len, tgt_len = span_counts(L, dq, mq, 1)
        assert res["in_lengths"][r] == in_len == L - N + S + 1 and res["tgt_lengths"][r] == tgt_len == N + S + 1
        inp, tgt = res["inputs"][r], res["targets"][r]
        assert (inp[in_len:] == -1).all() and (tgt[tgt_len:] == -100).all()
        assert inp[in_len - 1] == 2000 and tgt[tgt_len - 1] == 2000
        assert int(res["noise"][r].sum()) == N and not res["noise"][r, L:].any()
        sent = [first - i for i in range(S)]
        assert reassemble(inp[:in_len - 1].tolist(), tgt[:tgt_len - 1].tolist(), sent, L) == ids[r, :L].tolist()
        if L < 2:
            assert N == S == 0
            continue
        assert 1 <= S <= min(N, L - N) and 1 <= N <= L - 1
        # sentinels in order in both, the row starts kept and ends with noise, nothing is empty
        assert [t for t in inp[:in_len - 1] if t >= first - S + 1] == sent == [t for t in tgt[:tgt_len - 1] if t >= first - S + 1]
        assert res["noise"][r, 0] == 0 and res["noise"][r, L - 1] == 1
        edges = np.flatnonzero(np.diff(res["noise"][r, :L].astype(np.int8)))
        assert len(edges) == 2 * S - 1  # S kept segments and S spans alternate, each non-empty
        assert inp[0] == ids[r, 0] and tgt[0] == first and tgt[tgt_len - 2] == ids[r, L - 1]


def test_reference_by_hand():
    """L = 6, density 0.5, mean 1.5: N = 3, S = 2; the one cut of each segmentation is the smaller of two keys."""
    from tests.test_mlm_ref import philox_scalar
    ids = np.array([[10, 11, 12, 13, 14, 15]], dtype=np.int32)
    dq, mq = threshold(0.5), mean_q16(1.5)
    assert span_counts(6, dq, mq, 0) == (3, 2, 5, 5)
    x = [philox_scalar((j, 0, 8, 0), (7, 0)) for j in range(6)]
    a1 = 1 if x[1][0] <= x[2][0] else 2
    b1 = 1 if x[1][1] <= x[2][1] else 2
    res = np_spans(ids, seed=7, stream_id=8, density_q32=dq, mq16=mq, sentinel_first=99, sentinel_step=-1)
    row = ids[0].tolist()
    # segment 0 = b1 kept, span 0 = a1 noise, segment 1, span 1
    seg0, rest = row[:b1], row[b1:]
    span0, rest = rest[:a1], rest[a1:]
    seg1, span1 = rest[:3 - b1], rest[3 - b1:]
    assert res["inputs"][0].tolist() == seg0 + [99] + seg1 + [98]
    assert res["targets"][0].tolist() == [99] + span0 + [98] + span1
    assert res["noise"][0].tolist() == [0] * b1 + [1] * a1 + [0] * (3 - b1) + [1] * (3 - a1)


def test_reference_cuts_are_uniform():
    """4096 rows of L = 6, density 0.5, mean 1.5 (N = 3, S = 2): each segmentation has one cut, at 1 or
    at 2, each with probability 1/2. A count is Binomial(4096, 1/2), sd 32: within 5 sd = 160 of 2048."""
    rows = 4096
    ids = np.tile(np.arange(6, dtype=np.int32), (rows, 1))
    res = np_spans(ids, seed=2024, stream_id=1, density_q32=threshold(0.5), mq16=mean_q16(1.5), sentinel_first=100,
                   sentinel_step=0)
    assert (res["in_lengths"] == 5).all() and (res["tgt_lengths"] == 5).all()
    # the first sentinel of the inputs sits at b_1, the second of the targets at a_1 + 1
    b1 = np.argmax(res["inputs"] == 100, axis=1)
    a1 = np.array([np.flatnonzero(t == 100)[1] - 1 for t in res["targets"]])
    for cut in (a1, b1):
        assert set(np.unique(cut).tolist()) == {1, 2}
        for pos in (1, 2):
            assert abs(int((cut == pos).sum()) - 2048) <= 160, (pos, int((cut == pos).sum()))


def test_reference_ties_go_to_the_smaller_index():
    keys = np.array([0, 7, 3, 7, 3, 9, 3], dtype=np.uint64)
    assert np_cuts(keys, 7, 3) == [0, 2, 4, 7]
    assert np_cuts(keys, 7, 5) == [0, 1, 2, 4, 6, 7]
    assert np_cuts(keys, 7, 1) == [0, 7] and np_cuts(keys, 7, 7) == [0, 1, 2, 3, 4, 5, 6, 7]


# ------------------------------------------------------------------------------------------ C-ABI, host side
@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    return _lib.lib()


def _is_arg_error(L, rc):
    from akshar_amd import _lib
    return rc == _lib.AK_ERR_ARG and len(L.ak_last_error()) > 0


def lib_counts(L, n, dq, mq, has_eos):
    out = (C.c_uint64 * 4)()
    assert L.ak_ids_spans_lengths(n, dq, mq, has_eos, out) == 0
    return tuple(int(v) for v in out)


def test_lengths_helper_equals_the_formulas(L):
    for density in (0.0, 0.01, 0.15, 0.3, 0.5, 0.85, 1.0):
        for mean in (1.0, 1.5, 3.0, 10.0, 1000.0):
            dq, mq = threshold(density), mean_q16(mean)
            for n in range(601):
                for has_eos in (0, 1):
                    assert lib_counts(L, n, dq, mq, has_eos) == span_counts(n, dq, mq, has_eos), (density, mean, n)
    big = (1 << 32) - 1
    assert lib_counts(L, big, ONE, 65536, 1) == span_counts(big, ONE, 65536, 1) == (big - 1, 1, 3, big + 1)
    assert lib_counts(L, big, ONE // 2, (1 << 32) - 1, 0) == span_counts(big, ONE // 2, (1 << 32) - 1, 0)
    out = (C.c_uint64 * 4)()
    assert _is_arg_error(L, L.ak_ids_spans_lengths(10, ONE + 1, 65536, 0, out))
    assert _is_arg_error(L, L.ak_ids_spans_lengths(10, ONE, 65535, 0, out))
    assert _is_arg_error(L, L.ak_ids_spans_lengths(10, ONE, 65536, 0, None))


def test_t5_known_lengths(L):
    """HF's T5 pretraining example: inputs_length 512 at 0.15 / 3.0 takes 568 raw tokens and gives 114
    targets. By hand: N = 85, S = 28, 568 - 85 + 28 + 1 = 512, 85 + 28 + 1 = 114; L = 569 needs 513."""
    from akshar_amd import engine
    dq, mq = threshold(0.15), mean_q16(3.0)
    assert lib_counts(L, 568, dq, mq, 1) == (85, 28, 512, 114)
    assert lib_counts(L, 569, dq, mq, 1)[2] == 513
    assert engine.span_lengths(568, noise_density=0.15, mean_span_length=3.0, eos=True) == (85, 28, 512, 114)
    assert engine.span_raw_length(512, noise_density=0.15, mean_span_length=3.0, eos=True) == (568, 114)
    assert engine.span_raw_length(512, noise_density=0.15, mean_span_length=3.0, eos=False) == (569, 113)
    # the largest L, not the first that fits: no longer row fits either
    assert all(lib_counts(L, n, dq, mq, 1)[2] > 512 for n in range(569, MAX_WIDTH + 1))


def test_spans_argument_errors_cpu(L):
    """Every ak_ids_spans error of the header, raised on the host before any device call (the pointers
    here are host memory: nothing may touch them)."""
    src = (C.c_int32 * 64)()
    bufs = [(C.c_int32 * 128)(*([77] * 128)) for _ in range(4)]
    inp, tgt, il, tl = bufs
    nz = (C.c_uint8 * 64)(*([77] * 64))
    lens = (C.c_int32 * 8)(*([8] * 8))

    def spans(src=src, lengths=None, rows=8, width=8, density=ONE // 4, mean=3 * 65536, flags=0, inp=inp, in_width=9,
              tgt=tgt, tgt_width=5, il=il, tl=tl, nz=nz, cap=8):
        return L.ak_ids_spans(src, lengths, rows, width, 1, 2, 3, density, mean, 100, -1, 1, 0, -100, flags, inp, in_width, tgt,
                              tgt_width, il, tl, nz, cap, None)

    assert _is_arg_error(L, spans(src=None))
    assert _is_arg_error(L, spans(inp=None))
    assert _is_arg_error(L, spans(tgt=None))
    assert _is_arg_error(L, spans(width=0))
    assert _is_arg_error(L, spans(width=0, rows=0))
    assert _is_arg_error(L, spans(in_width=0))
    assert _is_arg_error(L, spans(tgt_width=0))
    assert _is_arg_error(L, spans(width=MAX_WIDTH + 1, rows=1))
    assert _is_arg_error(L, spans(density=ONE + 1))
    assert _is_arg_error(L, spans(mean=65535))
    assert _is_arg_error(L, spans(mean=0))
    assert _is_arg_error(L, spans(flags=1))
    assert _is_arg_error(L, spans(flags=DENSE_I64 | 8))
    assert _is_arg_error(L, spans(flags=-1))
    for kw in (dict(inp=src), dict(tgt=src), dict(il=src), dict(tl=src), dict(nz=C.cast(src, C.POINTER(C.c_uint8))),
               dict(tgt=inp), dict(il=inp), dict(tl=tgt), dict(tl=il), dict(nz=C.cast(il, C.POINTER(C.c_uint8))),
               dict(lengths=lens, il=lens)):
        assert _is_arg_error(L, spans(**kw)), kw
    assert _is_arg_error(L, spans(rows=1 << 62, cap=1 << 62))
    assert _is_arg_error(L, spans(rows=1 << 52, cap=1 << 52, width=8, in_width=1 << 12))
    assert all(list(b) == [77] * 128 for b in bufs) and list(nz) == [77] * 64


def test_spans_empty_calls_are_ok_without_a_device(L):
    src, inp, tgt = (C.c_int32 * 64)(), (C.c_int32 * 64)(*([77] * 64)), (C.c_int32 * 64)(*([77] * 64))

    def spans(src, rows, inp, tgt, cap):
        return L.ak_ids_spans(src, None, rows, 8, 1, 2, 3, ONE // 4, 3 * 65536, 100, -1, 1, 0, -100, 0, inp, 8, tgt, 8, None, None,
                              None, cap, None)

    assert spans(None, 0, None, None, 8) == 0
    assert spans(src, 8, inp, tgt, 0) == 0
    assert list(inp) == [77] * 64 and list(tgt) == [77] * 64


def test_header_states_the_definition():
    import os
    from tests.conftest import ROOT
    from akshar_amd import _lib
    src = open(os.path.join(ROOT, "include", "akshar.h")).read()
    assert "#define AK_SPANS_MAX_WIDTH %d" % MAX_WIDTH in src and _lib.AK_SPANS_MAX_WIDTH == MAX_WIDTH
    assert "round-half-up" in src and "equal keys: the smaller j first" in src


# ------------------------------------------------------------------------------------------ Python layer
def test_span_ids_value_errors_cpu():
    """engine.span_ids checks its numbers before it looks at a device."""
    import torch
    from akshar_amd import engine
    ids = torch.zeros((2, 40), dtype=torch.int32)
    ok = dict(sentinel_first=31999, pad_id=0)
    for bad in (dict(noise_density=1.5), dict(noise_density=-0.1), dict(mean_span_length=0.5), dict(mean_span_length=70000.0),
                dict(sentinel_first=1 << 31), dict(pad_id=-(1 << 31) - 1), dict(label_pad=1 << 40), dict(eos_id=-1),
                dict(sentinel_step=1 << 31), dict(seed=-1), dict(stream_id=1 << 64), dict(in_width=0), dict(tgt_width=-3),
                dict(n_sentinels=1, noise_density=0.5, mean_span_length=1.0)):
        with pytest.raises(ValueError):
            engine.span_ids(ids, **{**ok, **bad})
    with pytest.raises(ValueError, match="4096"):
        engine.span_ids(torch.zeros((1, MAX_WIDTH + 1), dtype=torch.int32), **ok)
    with pytest.raises(TypeError):  # the values pass: the host tensor is what is wrong
        engine.span_ids(ids, **ok)
    with pytest.raises(ValueError):
        engine.span_raw_length(0, eos=True)  # not even the empty row's eos fits
    assert engine.span_raw_length(1, eos=True) == (0, 1) and engine.span_raw_length(2, eos=True) == (1, 1)
    assert engine.span_lengths(0) == (0, 0, 0, 0) and engine.span_lengths(1, eos=True) == (0, 0, 2, 1)
