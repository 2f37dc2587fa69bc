"""Sliding windows and text pairs (include/akshar.h ak_ids_window_offs / ak_ids_windows) without a GPU:
what the two calls compute, restated with Python lists and pinned to HF `tokenizers`.

  - np_windows with keep_head = keep_tail = 1 reproduces every record of tests/golden/windows_hf.json.gz
    (HF enable_truncation(max_length, stride, strategy) with its overflow encodings on models/akshar.json,
    tools/gen_golden_windows.py): the window count, every window's ids, and HF's sequence_ids on the
    non-special positions of the main encoding;
  - without a fixed stream, a row's first window is its row of np_pad, and the whole output is np_pad's
    when no row overflows;
  - the C-ABI's host-side argument errors and empty calls, the flag values, the Python layer's checks.

tests/test_gpu_windows.py holds the kernels to np_windows and to the HF records.
"""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_dense_ref import load_dense_golden, mixed_rows, np_pad, pack_id_rows

WINDOWS_GOLDEN = os.path.join(ROOT, "tests", "golden", "windows_hf.json.gz")
PAD_LEFT, TRUNC_LEFT, DENSE_I64, DROP_LAST, FIXED_LAST, LONGEST_FIRST = 1, 2, 4, 8, 16, 32


def load_windows_golden():
    with gzip.open(WINDOWS_GOLDEN, "rt", encoding="utf-8") as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------ restatement
def _template(row, h, t):
    return (h, t) if len(row) >= h + t else (0, 0)


def _longest_first(n1, n2, m):
    """HF's TruncationStrategy::LongestFirst: the ids kept of two bodies of n1 and n2 ids in m places."""
    if n1 + n2 <= m:
        return n1, n2
    swap = n1 > n2
    if swap:
        n1, n2 = n2, n1
    n2 = n1 if n1 > m else max(n1, m - n1)
    if n1 + n2 > m:
        n1 = m // 2
        n2 = n1 + m % 2
    return (n2, n1) if swap else (n1, n2)


def row_windows(S, F, width, stride, h, t, fixed_cap, fixed_last, longest_first, has_f):
    """The windows of one sliding row S with its fixed row F, as [(first segment, second segment,
    start)] lists of ids, unpadded."""
    S, F = list(S), list(F)
    hs, ts = _template(S, h, t)
    head, body, tail = S[:hs], S[hs:len(S) - ts], S[len(S) - ts:]
    if longest_first:
        hf, tf = _template(F, h, t)
        fbody = F[hf:len(F) - tf]
        n1, n2 = _longest_first(len(fbody), len(body), width - hf - tf - hs - ts)
        return [(F[:hf] + fbody[:n1] + F[len(F) - tf:], head + body[:n2] + tail, 0)]
    if len(F) > fixed_cap:  # ak_ids_pad's right truncation; a cap below h + t cuts plainly
        hf, tf = _template(F, h, t)
        if fixed_cap < hf + tf:
            hf = tf = 0
        F = F[:hf] + F[hf:len(F) - tf][:fixed_cap - hf - tf] + F[len(F) - tf:]
    room = width - len(F) - hs - ts
    step = room - stride
    assert step >= 1
    wins, at = [], 0
    while True:  # HF's loop: windows every `step` ids until one reaches the end of the body
        sl = head + body[at:at + room] + tail
        wins.append((F, sl, at) if has_f and not fixed_last else (sl, F, at))
        if at + room >= len(body):
            return wins
        at += step


def np_windows(ids, offs, width, pad_id, stride=0, h=0, t=0, fixed=None, fixed_cap=0, fixed_last=False,
               longest_first=False, pad_left=False, dtype=np.int32):
    """A dict of out / mask / type_ids [n_windows, width], sample / start / lengths [n_windows] and
    win_offs [n + 1], as include/akshar.h defines ak_ids_window_offs and ak_ids_windows."""
    n = len(offs) - 1
    wins, sample, win_offs = [], [], [0]
    for r in range(n):
        F = fixed[0][fixed[1][r]:fixed[1][r + 1]] if fixed is not None else []
        rw = row_windows(ids[offs[r]:offs[r + 1]], F, width, stride, h, t, fixed_cap, fixed_last, longest_first,
                         fixed is not None)
        wins += rw
        sample += [r] * len(rw)
        win_offs.append(len(wins))
    nw = len(wins)
    out = np.full((nw, width), pad_id, dtype=dtype)
    mask = np.zeros((nw, width), dtype=np.uint8)
    types = np.zeros((nw, width), dtype=np.uint8)
    lens = np.asarray([len(a) + len(b) for a, b, _ in wins], dtype=np.int64)
    first = np.asarray([len(a) for a, _, _ in wins], dtype=np.int64)
    flat = np.asarray([x for a, b, _ in wins for x in a + b], dtype=np.int64)
    row = np.repeat(np.arange(nw), lens)
    j = np.arange(len(flat)) - np.repeat(np.cumsum(lens) - lens, lens)  # the id's index inside its window
    col = j + (np.repeat(width - lens, lens) if pad_left else 0)
    out[row, col] = flat
    mask[row, col] = 1
    types[row, col] = j >= np.repeat(first, lens)
    return {"out": out, "mask": mask, "type_ids": types, "sample": np.asarray(sample, dtype=np.int32),
            "start": np.asarray([s for _, _, s in wins], dtype=np.int32),
            "lengths": lens.astype(np.int32),
            "win_offs": np.asarray(win_offs, dtype=np.int64)}


def largest_fixed_cap(width, stride, h, t):
    return width - h - t - stride - 1


def hf_cases(golden, dense):
    """Every record of the fixture as (key, np_windows keyword arguments, sliding rows, fixed rows | None,
    HF's windows per row, HF's sequence_ids per row); rows are id lists."""
    rows = [dense["rows"][i]["ids"] for i in golden["rows"]]
    for rec in golden["single"]:
        kw = dict(width=rec["max_length"], stride=rec["stride"], h=1, t=1)
        yield ("single", rec["max_length"], rec["stride"]), kw, rows, None, rec["windows"], rec["seq"]
    for rec in golden["pairs"]:
        w, s = rec["max_length"], rec["stride"]
        kw = dict(width=w, stride=s, h=1, t=1, fixed_cap=largest_fixed_cap(w, s, 1, 1), fixed_last=rec["mode"] == "only_first")
        yield (rec["mode"], w, s), kw, rows, [rows[q] for q in rec["partner"]], rec["windows"], rec["seq"]
    for rec in golden["longest_first"]:
        kw = dict(width=rec["max_length"], h=1, t=1, longest_first=True)
        yield (("longest_first", rec["max_length"], 0), kw, rows, [rows[q] for q in rec["partner"]],
               [[x] for x in rec["ids"]], rec["seq"])


def check_against_hf(res, want, seq, key):
    """res (np_windows' dict, right padding) holds exactly HF's windows, and HF's sequence ids."""
    assert res["win_offs"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), key
    flat = [w for row in want for w in row]
    assert res["lengths"].tolist() == [len(w) for w in flat], key
    assert [res["out"][i, :len(w)].tolist() for i, w in enumerate(flat)] == flat, key
    assert res["sample"].tolist() == [r for r, row in enumerate(want) for _ in row], key
    for r, sq in enumerate(seq):  # the main encoding is the row's first window
        sq = np.asarray(sq)
        ty = res["type_ids"][res["win_offs"][r], :len(sq)]
        assert np.array_equal(ty[sq >= 0], sq[sq >= 0]), key
    assert np.array_equal(res["mask"], np.arange(res["out"].shape[1])[None, :] < res["lengths"][:, None]), key


# ------------------------------------------------------------------------------------------ semantics
@pytest.fixture(scope="module")
def golden():
    return load_windows_golden()


@pytest.fixture(scope="module")
def dense():
    return load_dense_golden()


def test_fixture_covers_the_cases(golden, dense):
    lens = [len(dense["rows"][i]["ids"]) for i in golden["rows"]]
    assert dense["rows"][golden["rows"][0]]["text"] == "" and 2 in lens and 3 in lens and sum(n > 70 for n in lens) >= 3
    assert {(r["max_length"], r["stride"]) for r in golden["single"]} == {(3, 0), (4, 1), (6, 2), (8, 3), (64, 16)}
    assert {(r["mode"], r["max_length"], r["stride"]) for r in golden["pairs"]} == {
        (m, w, s) for m in ("only_second", "only_first") for w, s in ((12, 0), (12, 3), (64, 8))}
    assert {r["max_length"] for r in golden["longest_first"]} == {4, 5, 6, 16, 64}
    for rec in golden["pairs"]:
        assert max(lens[q] for q in rec["partner"]) <= 6 and min(lens[q] for q in rec["partner"]) == 2


def test_np_windows_reproduces_every_hf_record(golden, dense):
    seen = 0
    for key, kw, rows, partners, want, seq in hf_cases(golden, dense):
        ids, offs = pack_id_rows(rows)
        res = np_windows(ids, offs, pad_id=0, fixed=pack_id_rows(partners) if partners else None, **kw)
        check_against_hf(res, want, seq, key)
        seen += 1
    assert seen == 16


def test_first_window_is_the_padded_row():
    rows = mixed_rows(130, seed=3)
    ids, offs = pack_id_rows(rows)
    for width, h, t in ((1, 0, 0), (4, 1, 1), (5, 2, 0), (64, 0, 3), (65, 1, 1)):
        for stride in sorted({0, 1, width - h - t - 1}):
            if width - h - t <= stride:
                continue
            for left in (False, True):
                res = np_windows(ids, offs, width, -7, stride, h, t, pad_left=left)
                pad = np_pad(ids, offs, width, -7, h, t, pad_left=left)
                first = res["win_offs"][:-1]
                assert np.array_equal(res["out"][first], pad[0]) and np.array_equal(res["mask"][first], pad[1])
                assert np.array_equal(res["lengths"][first], pad[2]) and not res["type_ids"].any()
                assert (np.diff(res["win_offs"]) >= 1).all() and (res["start"][first] == 0).all()


def test_no_overflow_is_np_pad():
    rows = mixed_rows(60, seed=5, lengths=(0, 1, 2, 3, 9, 10))
    ids, offs = pack_id_rows(rows)
    res = np_windows(ids, offs, 10, 4, 3, 1, 1, pad_left=True)
    pad = np_pad(ids, offs, 10, 4, 1, 1, pad_left=True)
    assert np.array_equal(res["out"], pad[0]) and np.array_equal(res["mask"], pad[1])
    assert np.array_equal(res["lengths"], pad[2]) and res["sample"].tolist() == list(range(60))


def test_np_windows_by_hand():
    ids, offs = pack_id_rows([[1, 10, 11, 12, 13, 14, 2], [], [7]])
    fix = pack_id_rows([[1, 20, 21, 22, 2], [1, 2], [1, 30, 2]])
    res = np_windows(ids, offs, 6, 0, 1, 1, 1)  # room 4, step 3
    assert res["out"].tolist() == [[1, 10, 11, 12, 13, 2], [1, 13, 14, 2, 0, 0], [0] * 6, [7, 0, 0, 0, 0, 0]]
    assert res["start"].tolist() == [0, 3, 0, 0] and res["win_offs"].tolist() == [0, 2, 3, 4]
    res = np_windows(ids, offs, 8, 0, 0, 1, 1, fixed=fix, fixed_cap=4)  # the first fixed row is cut to [1, 20, 21, 2]
    assert res["out"].tolist() == [[1, 20, 21, 2, 1, 10, 11, 2], [1, 20, 21, 2, 1, 12, 13, 2], [1, 20, 21, 2, 1, 14, 2, 0],
                                   [1, 2, 0, 0, 0, 0, 0, 0], [1, 30, 2, 7, 0, 0, 0, 0]]
    assert res["type_ids"].tolist() == [[0] * 4 + [1] * 4] * 2 + [[0] * 4 + [1] * 3 + [0], [0] * 8, [0, 0, 0, 1, 0, 0, 0, 0]]
    res = np_windows(ids, offs, 8, 0, 0, 1, 1, fixed=fix, fixed_cap=1, fixed_last=True, pad_left=True)
    # a cap below h + t keeps the first id only; room 5: one window per row, the fixed id behind it
    assert res["out"].tolist() == [[1, 10, 11, 12, 13, 14, 2, 1], [0] * 7 + [1], [0] * 6 + [7, 1]]
    assert res["type_ids"].tolist() == [[0] * 7 + [1]] * 3
    res = np_windows(ids, offs, 7, 0, 0, 1, 1, fixed=fix, longest_first=True)  # M = 3: bodies 3 and 5 -> 1 and 2
    assert res["out"][0].tolist() == [1, 20, 2, 1, 10, 11, 2] and res["type_ids"][0].tolist() == [0, 0, 0, 1, 1, 1, 1]


# ------------------------------------------------------------------------------------------ C-ABI, host side
@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    return _lib.lib()


def _is_arg_error(L, rc):
    from akshar_amd import _lib
    return rc == _lib.AK_ERR_ARG and len(L.ak_last_error()) > 0


def test_flag_values_match_the_header():
    from akshar_amd import _lib
    src = open(os.path.join(ROOT, "include", "akshar.h")).read()
    for name in ("AK_WIN_FIXED_LAST", "AK_WIN_LONGEST_FIRST"):
        assert ("#define %s %d" % (name, getattr(_lib, name))) in src
    assert (_lib.AK_WIN_FIXED_LAST, _lib.AK_WIN_LONGEST_FIRST) == (FIXED_LAST, LONGEST_FIRST)


def test_window_argument_errors_cpu(L):
    """Every argument error of the header, from both calls where both take the argument, raised on the
    host before any device call (the pointers here are host memory: nothing may touch them)."""
    ids, offs, out = (C.c_int32 * 8)(), (C.c_uint64 * 3)(0, 4, 8), (C.c_int32 * 64)(*([77] * 64))
    wo = (C.c_uint64 * 3)(5, 5, 5)
    ws = C.c_void_p(8)  # never dereferenced: every call below fails before it is used

    def emit(ids=ids, offs=offs, f_ids=None, f_offs=None, n=2, wo=wo, width=8, stride=0, h=1, t=1, cap=0, flags=0, out=out):
        return L.ak_ids_windows(ids, offs, f_ids, f_offs, n, wo, width, stride, h, t, cap, 0, flags, out, 4, None, None,
                                None, None, None, None)

    def count(ws=ws, offs=offs, f_offs=None, n=2, wo=wo, width=8, stride=0, h=1, t=1, cap=0, flags=0):
        return L.ak_ids_window_offs(ws, offs, f_offs, n, width, stride, h, t, cap, flags, wo, None)

    assert _is_arg_error(L, emit(ids=None))
    assert _is_arg_error(L, emit(out=None))
    assert _is_arg_error(L, emit(f_ids=ids))
    assert _is_arg_error(L, emit(f_offs=offs))
    assert _is_arg_error(L, count(ws=None))
    for call in (emit, count):
        assert _is_arg_error(L, call(offs=None))
        assert _is_arg_error(L, call(wo=None))
        assert _is_arg_error(L, call(width=0, h=0, t=0))
        for flags in (TRUNC_LEFT, DROP_LAST, 64, -1):
            assert _is_arg_error(L, call(flags=flags))
        assert _is_arg_error(L, call(cap=2))                          # fixed_cap without a fixed stream
        assert _is_arg_error(L, call(width=2))                        # 2 - 0 - 1 - 1 <= 0
        assert _is_arg_error(L, call(stride=6))                       # 8 - 0 - 1 - 1 <= 6
        assert _is_arg_error(L, call(f_offs=offs, cap=6, **({"f_ids": ids} if call is emit else {})))
        assert _is_arg_error(L, call(h=0xFFFFFFFF, t=0xFFFFFFFF))     # no wrap-around
        assert _is_arg_error(L, call(stride=0xFFFFFFFF, h=9, t=0))
        assert _is_arg_error(L, call(flags=LONGEST_FIRST))            # no fixed stream
        pair = {"f_offs": offs, **({"f_ids": ids} if call is emit else {})}
        assert _is_arg_error(L, call(flags=LONGEST_FIRST, stride=1, **pair))
        assert _is_arg_error(L, call(flags=LONGEST_FIRST, width=3, **pair))   # below 2 (h + t)
        assert _is_arg_error(L, call(flags=LONGEST_FIRST | FIXED_LAST, **pair))
    assert list(out) == [77] * 64 and list(wo) == [5, 5, 5]


def test_empty_calls_are_ok_without_a_device(L):
    """n == 0 and a capacity of 0 store nothing and launch nothing: AK_OK on a machine without a GPU."""
    ids, offs, out = (C.c_int32 * 8)(), (C.c_uint64 * 3)(0, 4, 8), (C.c_int32 * 64)(*([77] * 64))
    wo = (C.c_uint64 * 3)(0, 1, 2)
    args = (8, 2, 1, 1, 0, 0, 0, out)
    assert L.ak_ids_windows(None, offs, None, None, 0, wo, *args, 4, None, None, None, None, None, None) == 0
    assert L.ak_ids_windows(ids, offs, None, None, 2, wo, *args, 0, None, None, None, None, None, None) == 0
    assert L.ak_ids_windows(ids, offs, ids, offs, 2, wo, 8, 0, 1, 1, 0, 0, LONGEST_FIRST, out, 0, None, None, None, None,
                            None, None) == 0
    assert list(out) == [77] * 64


def test_python_layer_errors_cpu():
    import torch
    from akshar_amd import engine
    from akshar_amd.tokenizer import aksharTokenizer
    with pytest.raises(ValueError, match="need model for IDs"):
        aksharTokenizer().encode_windows(["a"], 8)
    ids, offs = torch.zeros(4, dtype=torch.int32), torch.tensor([0, 4])
    with pytest.raises(TypeError):
        engine.window_ids(ids, offs, 8, 0)  # host tensors
    assert "window_ids" in engine.__all__
