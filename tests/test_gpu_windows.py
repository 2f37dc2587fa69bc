"""Sliding windows and text pairs on the device (include/akshar.h ak_ids_window_offs / ak_ids_windows,
akshar_amd/csrc/ak_k_windows.hip), bit-exact against np_windows of tests/test_windows_ref.py (which
that file pins to HF `tokenizers`) and against the HF records themselves.

Every output array of every raw call is allocated for the full result plus a guard band of
BUFFER_GUARD sentinel elements: what lies at or past the capacity must come back untouched.

Shapes: the adversarial length mix of tests/test_gpu_dense.py. The strides 0 and 1 run on all of its
2,002 rows at selected widths and on its first 260 rows (20 of every length, the empty rows, the rows
shorter than h + t and the 1,000-id rows included) in the full cross product; the largest legal
stride makes step 1, one window per body id, so it runs on those 260 rows only, and from width 63 on
on the first 65 (5 of every length).
"""
import numpy as np
import pytest
import torch

from tests.conftest import BPE_PATH, SPM_PATH
from tests.test_dense_ref import LENGTH_MIX, load_dense_golden, mixed_rows, np_pad, pack_id_rows
from tests.test_gpu_buffers import S32, S64
from tests.test_gpu_dense import S8, _dev_rows, _guarded, _split
from tests.test_windows_ref import (DENSE_I64, FIXED_LAST, LONGEST_FIRST, PAD_LEFT, check_against_hf, hf_cases,
                                    largest_fixed_cap, load_windows_golden, np_windows)

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 256)
KEEPS = ((0, 0), (1, 1), (2, 0), (0, 3))
SCAN_TILE = 2048  # ak_internal.h: the single-block scan's limit
NAMES = ("out", "mask", "type_ids", "sample", "start", "lengths")


@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def ws(L):
    from akshar_amd import engine
    return engine.workspace(0)


def run_offs(L, ws, so, fo, n, width, stride, h, t, cap, flags):
    """ak_ids_window_offs into a guarded win_offs; returns the device tensor (n + 1 used)."""
    wo = _guarded(n + 1, torch.int64, S64)
    rc = L.ak_ids_window_offs(ws, so.data_ptr(), fo.data_ptr() if fo is not None else None, n, width, stride, h, t, cap,
                              flags, wo.data_ptr(), None)
    assert rc == 0, L.ak_last_error()
    torch.cuda.synchronize()
    got, clean = _split(wo, n + 1, S64)
    assert clean, "win_offs stored past n + 1"
    return wo, got


def run_windows(L, ws, S, F, n, width, stride, h, t, cap, pad_id, flags, cap_windows=None, skip=None, lead=0):
    """Both calls through the raw C-ABI into guarded outputs sized for every window; returns win_offs and
    the windows below the capacity as a dict like np_windows' (None for the output `skip` names), after
    the guard checks. S, F: (ids, offs) device pairs."""
    fo = F[1] if F is not None else None
    wo, offs = run_offs(L, ws, S[1], fo, n, width, stride, h, t, cap, flags)
    total = int(offs[n])
    cw = total if cap_windows is None else cap_windows
    i64 = bool(flags & DENSE_I64)
    bufs = {"out": _guarded(total * width, torch.int64 if i64 else torch.int32, S64 if i64 else S32, lead),
            "mask": _guarded(total * width, torch.uint8, S8, lead), "type_ids": _guarded(total * width, torch.uint8, S8, lead),
            "sample": _guarded(total, torch.int32, S32, lead), "start": _guarded(total, torch.int32, S32, lead),
            "lengths": _guarded(total, torch.int32, S32, lead)}
    if skip:
        bufs[skip] = None
    ptr = [bufs[k].data_ptr() if bufs[k] is not None else None for k in NAMES]
    rc = L.ak_ids_windows(S[0].data_ptr(), S[1].data_ptr(), F[0].data_ptr() if F is not None else None,
                          fo.data_ptr() if F is not None else None, n, wo.data_ptr(), width, stride, h, t, cap, pad_id,
                          flags, ptr[0], cw, *ptr[1:], None)
    assert rc == 0, L.ak_last_error()
    torch.cuda.synchronize()
    k = min(total, cw)
    res = {"win_offs": offs.astype(np.int64), "windows": k}
    for name in NAMES:
        if bufs[name] is None:
            res[name] = None
            continue
        wide = name in ("out", "mask", "type_ids")
        per = width if wide else 1
        sent = (S64 if i64 else S32) if name == "out" else S8 if name in ("mask", "type_ids") else S32
        got, clean = _split(bufs[name], k * per, sent)
        assert clean, "%s stored at or past the capacity" % name
        res[name] = got.reshape(k, width) if wide else got
    return res


def check_windows(res, ref, key=None):
    k = res["windows"]
    assert np.array_equal(res["win_offs"], ref["win_offs"]), key
    for name in NAMES:
        if res[name] is not None:
            assert np.array_equal(res[name], ref[name][:k]), (name, key)


@pytest.fixture(scope="module")
def mixed():
    """The 2,002 rows of tests/test_gpu_dense.py's mix as the sliding stream, and a fixed stream of the
    same count whose lengths run through the mix at another pace (empty fixed rows, fixed rows shorter
    than h + t, fixed rows under and over every fixed_cap), on the host and on the device at element
    offsets 1 and 3 of larger tensors."""
    rows = mixed_rows(2002, seed=7)
    assert {len(r) for r in rows} == set(LENGTH_MIX)
    rng = np.random.default_rng(11)
    flens = [LENGTH_MIX[(3 * i + i // 7) % 10] for i in range(2002)]  # 0 .. 127 ids
    frows = [rng.integers(30001, 60000, size=ln).tolist() for ln in flens]
    S, F = pack_id_rows(rows), pack_id_rows(frows)
    return {"S": S, "F": F, "n": 2002, "dev": {lead: (_dev_rows(*S, lead), _dev_rows(*F, 4 - lead)) for lead in (1, 3)}}


SUB = 260


def _rows_for(width, step):
    """Rows of the mix a case runs on: at step 1 a wide window costs the reference width elements per body id."""
    return 65 if step == 1 and width >= 63 else SUB


def _strides(width, h, t, cap=0):
    return sorted({s for s in (0, 1, width - cap - h - t - 1) if 0 <= s < width - cap - h - t})


# ------------------------------------------------------------------------------------------ single sequences
@pytest.mark.parametrize("width", WIDTHS)
def test_single_adversarial_shapes(L, ws, mixed, width):
    """Keeps x strides x int32 / int64, each optional output NULL in turn, left padding, a negative pad
    id, unaligned sources; the first window of every row is np_pad's row."""
    case = 0
    for h, t in KEEPS:
        for stride in _strides(width, h, t):
            flags = (PAD_LEFT if case % 2 else 0) | (DENSE_I64 if case % 3 == 1 else 0)
            n = _rows_for(width, width - h - t - stride)
            ref = np_windows(mixed["S"][0], mixed["S"][1][:n + 1], width, -7, stride, h, t, pad_left=bool(flags & PAD_LEFT),
                             dtype=np.int64 if flags & DENSE_I64 else np.int32)
            S, _ = mixed["dev"][(1, 3)[case % 2]]
            res = run_windows(L, ws, S, None, n, width, stride, h, t, 0, -7, flags, skip=((None,) + NAMES[1:])[case % 6])
            check_windows(res, ref, (h, t, stride, flags))
            pad = np_pad(mixed["S"][0], mixed["S"][1][:n + 1], width, -7, h, t, pad_left=bool(flags & PAD_LEFT))
            assert np.array_equal(res["out"][ref["win_offs"][:-1]], pad[0])
            case += 1
    assert case >= (1 if width == 1 else 2)


@pytest.mark.parametrize("width,h,t,stride", [(1, 0, 0, 0), (2, 0, 0, 1), (3, 0, 0, 0), (3, 1, 1, 0), (65, 1, 1, 1), (256, 1, 1, 0)])
def test_single_all_rows(L, ws, mixed, width, h, t, stride):
    """All 2,002 rows: widths 1 to 3 with keep (0, 0) put more than 64 one-window rows into one chunk of
    256 elements (several rounds of the LDS window); 65 makes chunks straddle windows."""
    ref = np_windows(*mixed["S"], width, 0, stride, h, t)
    S, _ = mixed["dev"][1]
    check_windows(run_windows(L, ws, S, None, mixed["n"], width, stride, h, t, 0, 0, 0), ref)
    assert len(ref["out"]) > mixed["n"]


@pytest.mark.parametrize("width", [1, 2, 3])
def test_many_one_window_rows_in_one_chunk(L, ws, width):
    """700 rows of 0 or 1 ids, one window each: 85 to 256 rows share a chunk of 256 elements, so a wave
    needs several rounds of its 64-entry LDS window; with and without a fixed id in front."""
    rows = [[i + 1] if i % 5 else [] for i in range(700)]
    frows = [[9000 + i] if i % 3 else [] for i in range(700)]
    ids, offs = pack_id_rows(rows)
    S, F = _dev_rows(ids, offs, 1), _dev_rows(*pack_id_rows(frows), 3)
    check_windows(run_windows(L, ws, S, None, 700, width, 0, 0, 0, 0, -1, 0), np_windows(ids, offs, width, -1))
    if width > 1:
        ref = np_windows(ids, offs, width, -1, fixed=pack_id_rows(frows), fixed_cap=1)
        check_windows(run_windows(L, ws, S, F, 700, width, 0, 0, 0, 1, -1, 0), ref)
        assert ref["win_offs"].tolist() == list(range(701))


# ------------------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("width", WIDTHS)
def test_pairs_adversarial_shapes(L, ws, mixed, width):
    """only_second / only_first with fixed rows under and over fixed_cap (and a cap below h + t), and
    longest_first, on both unaligned placements."""
    case = 0
    for h, t in KEEPS:
        room = width - h - t
        for cap in sorted({0, 3, room // 2, room - 1}):
            if not 0 <= cap < room:
                continue
            for stride in _strides(width, h, t, cap):
                n = _rows_for(width, width - cap - h - t - stride)
                flags = (FIXED_LAST if case % 2 else 0) | (PAD_LEFT if case % 4 >= 2 else 0) | (DENSE_I64 if case % 3 == 2 else 0)
                S, F = mixed["dev"][(1, 3)[case % 2]]
                ref = np_windows(mixed["S"][0], mixed["S"][1][:n + 1], width, -7, stride, h, t,
                                 fixed=(mixed["F"][0], mixed["F"][1][:n + 1]), fixed_cap=cap,
                                 fixed_last=bool(flags & FIXED_LAST), pad_left=bool(flags & PAD_LEFT),
                                 dtype=np.int64 if flags & DENSE_I64 else np.int32)
                res = run_windows(L, ws, S, F, n, width, stride, h, t, cap, -7, flags, skip=((None,) + NAMES[1:])[case % 6])
                check_windows(res, ref, (h, t, cap, stride, flags))
                case += 1
        if width >= 2 * (h + t):
            for flags in (LONGEST_FIRST, LONGEST_FIRST | PAD_LEFT | DENSE_I64):
                S, F = mixed["dev"][3]
                ref = np_windows(*mixed["S"], width, 5, 0, h, t, fixed=mixed["F"], longest_first=True,
                                 pad_left=bool(flags & PAD_LEFT), dtype=np.int64 if flags & DENSE_I64 else np.int32)
                res = run_windows(L, ws, S, F, mixed["n"], width, 0, h, t, 77, 5, flags)  # fixed_cap is ignored
                check_windows(res, ref, (h, t, flags))
                assert res["win_offs"].tolist() == list(range(mixed["n"] + 1))
                case += 1
    assert case >= 2


@pytest.mark.parametrize("width,h,t,stride,cap,flags", [(65, 1, 1, 1, 9, 0), (3, 0, 0, 0, 1, FIXED_LAST), (65, 1, 1, 8, 40, FIXED_LAST),
                                                        (3, 0, 0, 1, 1, 0)])
def test_pairs_all_rows(L, ws, mixed, width, h, t, stride, cap, flags):
    """only_second and only_first over all 2,002 rows: the search and the LDS walk with a fixed stream
    over many chunks per wave."""
    ref = np_windows(*mixed["S"], width, 0, stride, h, t, fixed=mixed["F"], fixed_cap=cap, fixed_last=bool(flags & FIXED_LAST))
    S, F = mixed["dev"][1]
    check_windows(run_windows(L, ws, S, F, mixed["n"], width, stride, h, t, cap, 0, flags), ref)
    assert len(ref["out"]) > mixed["n"]


# ------------------------------------------------------------------------------------------ capacities, alignment
@pytest.mark.parametrize("width", [3, 8, 65])
def test_short_capacities(L, ws, mixed, width):
    """cap_windows 0, 1, in the middle of a row's windows, and past the total: nothing past it."""
    S, F = mixed["dev"][1]
    ref = np_windows(mixed["S"][0], mixed["S"][1][:SUB + 1], width, 0, 0, 1, 1, fixed=(mixed["F"][0], mixed["F"][1][:SUB + 1]),
                     fixed_cap=0)
    multi = int(np.flatnonzero(np.diff(ref["win_offs"]) >= 3)[0])
    mid = int(ref["win_offs"][multi]) + 1
    assert ref["sample"][mid - 1] == ref["sample"][mid] == multi
    for k, cap in enumerate((0, 1, mid, len(ref["out"]) + 9)):
        res = run_windows(L, ws, S, F, SUB, width, 0, 1, 1, 0, 0, DENSE_I64 if k % 2 else 0, cap_windows=cap)
        assert res["windows"] == min(cap, len(ref["out"]))
        check_windows(res, ref, cap)


@pytest.mark.parametrize("width", [3, 8, 65])
def test_unaligned_outputs(L, ws, mixed, width):
    """Outputs at element offset 1 of their allocations: the element-store path gives the same result."""
    S, F = mixed["dev"][3]
    ref = np_windows(mixed["S"][0], mixed["S"][1][:SUB + 1], width, -7, 0, 0, 0, fixed=(mixed["F"][0], mixed["F"][1][:SUB + 1]),
                     fixed_cap=width // 2, fixed_last=True)
    for i64 in (0, DENSE_I64):
        res = run_windows(L, ws, S, F, SUB, width, 0, 0, 0, width // 2, -7, FIXED_LAST | i64, cap_windows=len(ref["out"]) - 3, lead=1)
        check_windows(res, ref)


# ------------------------------------------------------------------------------------------ win_offs
@pytest.mark.parametrize("n", [0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 5000])
def test_win_offs_is_the_cumsum(L, ws, n):
    """At, below and above the single-block scan's limit; n = 0 writes win_offs[0] = 0."""
    rows = mixed_rows(n, seed=n + 1, lengths=(0, 1, 2, 9, 40, 200))
    ids, offs = pack_id_rows(rows)
    S = _dev_rows(ids, offs, 1)
    lens = np.diff(offs)
    body = np.where(lens >= 2, lens - 2, lens)
    room = 8 - np.where(lens >= 2, 2, 0)
    want = np.where(body <= room, 1, 1 + -(-(body - room) // (room - 3)))
    _, got = run_offs(L, ws, S[1], None, n, 8, 3, 1, 1, 0, 0)
    assert got.tolist() == np.concatenate([[0], np.cumsum(want)]).tolist()


def test_all_rows_empty(L, ws):
    S, F = _dev_rows(*pack_id_rows([[]] * 70)), _dev_rows(*pack_id_rows([[]] * 70))
    for fixed, flags in ((None, PAD_LEFT), (F, 0), (F, LONGEST_FIRST)):
        res = run_windows(L, ws, S, fixed, 70, 5, 0, 1, 1, 0, 9, flags)
        assert res["win_offs"].tolist() == list(range(71)) and (res["out"] == 9).all()
        assert not res["mask"].any() and not res["lengths"].any() and res["sample"].tolist() == list(range(70))


# ------------------------------------------------------------------------------------------ HF records
@pytest.fixture(scope="module")
def golden():
    return load_windows_golden(), load_dense_golden()


def test_kernel_matches_every_hf_record(L, ws, golden):
    seen = 0
    for key, kw, rows, partners, want, seq in hf_cases(*golden):
        S = _dev_rows(*pack_id_rows(rows), 1)
        F = _dev_rows(*pack_id_rows(partners), 3) if partners else None
        flags = (FIXED_LAST if kw.get("fixed_last") else 0) | (LONGEST_FIRST if kw.get("longest_first") else 0)
        res = run_windows(L, ws, S, F, len(rows), kw["width"], kw.get("stride", 0), 1, 1, kw.get("fixed_cap", 0), 0, flags)
        check_against_hf(res, want, seq, key)
        seen += 1
    assert seen == 16


# ------------------------------------------------------------------------------------------ Python layer
@pytest.fixture(scope="module")
def toks():
    from akshar_amd.tokenizer import aksharTokenizer
    return {"bpe": aksharTokenizer(BPE_PATH, "bpe"), "spm": aksharTokenizer(SPM_PATH, "sentencepiece")}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _as_ref(d):
    """encode_windows' dict under np_windows' names."""
    h = _host(d)
    return {"out": h["input_ids"], "mask": h["attention_mask"].astype(np.uint8), "type_ids": h["token_type_ids"],
            "sample": h["overflow_to_sample_mapping"], "start": h["window_start"], "lengths": h["lengths"],
            "win_offs": h["win_offs"], "windows": len(h["input_ids"])}


def _pick(golden):
    """Positions in the fixture's rows that encode quickly (the 2,503-id row among them)."""
    wg, dg = golden
    return [p for p, i in enumerate(wg["rows"]) if len(dg["rows"][i]["ids"]) < 2600]


def test_encode_windows_bpe_equals_hf(toks, golden):
    wg, dg = golden
    pick = _pick(golden)
    texts = [dg["rows"][i]["text"] for i in wg["rows"]]
    assert "" in [texts[p] for p in pick] and max(len(dg["rows"][wg["rows"][p]]["ids"]) for p in pick) > 70
    seen = set()
    for rec in wg["single"]:
        got = _as_ref(toks["bpe"].encode_windows([texts[p] for p in pick], rec["max_length"], stride=rec["stride"]))
        check_against_hf(got, [rec["windows"][p] for p in pick], [rec["seq"][p] for p in pick], rec["max_length"])
        seen.add("single")
    for rec in wg["pairs"]:
        a, b = [texts[p] for p in pick], [texts[rec["partner"][p]] for p in pick]
        first, second = (b, a) if rec["mode"] == "only_second" else (a, b)
        got = _as_ref(toks["bpe"].encode_windows(first, rec["max_length"], stride=rec["stride"], text_pair=second,
                                                 truncation=rec["mode"]))
        check_against_hf(got, [rec["windows"][p] for p in pick], [rec["seq"][p] for p in pick], rec["mode"])
        seen.add(rec["mode"])
    for rec in wg["longest_first"]:
        keep = [p for p in pick if rec["partner"][p] in pick]
        got = _as_ref(toks["bpe"].encode_windows([texts[rec["partner"][p]] for p in keep], rec["max_length"],
                                                 text_pair=[texts[p] for p in keep], truncation="longest_first"))
        check_against_hf(got, [[rec["ids"][p]] for p in keep], [rec["seq"][p] for p in keep], "longest_first")
        seen.add("longest_first")
    assert seen == {"single", "only_second", "only_first", "longest_first"}


def _texts(golden):
    wg, dg = golden
    return [dg["rows"][i]["text"] for i in wg["rows"] if len(dg["rows"][i]["ids"]) < 200]


def test_encode_windows_spm_equals_numpy(toks, golden):
    from akshar_amd import engine
    texts = _texts(golden)
    ids, offs = pack_id_rows(toks["spm"].encode_batch(texts))
    fixed = pack_id_rows(toks["spm"].encode_batch(texts[::-1]))
    for width, stride, side in ((1, 0, "right"), (7, 2, "left"), (16, 5, "right")):
        got = _as_ref(toks["spm"].encode_windows(texts, width, stride=stride, padding_side=side, pad_id=5))
        check_windows(got, np_windows(ids, offs, width, 5, stride, pad_left=side == "left"))
        assert got["out"].dtype == np.int32 and len(got["out"]) > len(texts)
    got = _as_ref(toks["spm"].encode_windows(texts[::-1], 16, stride=2, text_pair=engine.pack(texts), max_fixed_length=6,
                                             pad_id=5))
    check_windows(got, np_windows(ids, offs, 16, 5, 2, fixed=fixed, fixed_cap=6))
    got = _as_ref(toks["spm"].encode_windows(texts, 16, stride=2, text_pair=texts[::-1], truncation="only_first", pad_id=5))
    check_windows(got, np_windows(ids, offs, 16, 5, 2, fixed=fixed, fixed_cap=largest_fixed_cap(16, 2, 0, 0), fixed_last=True))


def test_side_stream_then_default_stream_and_max_windows(toks, golden):
    from akshar_amd import engine
    texts = _texts(golden)
    tok = toks["bpe"]
    want = _host(tok.encode_windows(texts, 12, stride=3, text_pair=texts[::-1], pad_id=1))
    side = torch.cuda.Stream()
    for stream in (side, torch.cuda.default_stream()):
        with torch.cuda.stream(stream):
            got = tok.encode_windows(texts, 12, stride=3, text_pair=texts[::-1], pad_id=1)
        stream.synchronize()
        assert all(np.array_equal(v, want[k]) for k, v in _host(got).items()), stream is side
    ids, oo = tok.encode_packed(*engine.pack(texts))
    sized = _host(engine.window_ids(ids, oo, 9, 0, stride=2, keep_head=1, keep_tail=1, dtype=torch.int64))
    nw = len(sized["input_ids"])
    assert sized["input_ids"].dtype == np.int64 and nw == sized["win_offs"][-1] > len(texts)
    for cap in (nw + 7, nw // 2):
        fixed = _host(engine.window_ids(ids, oo, 9, 0, stride=2, keep_head=1, keep_tail=1, dtype=torch.int64, max_windows=cap))
        k = min(cap, nw)
        assert len(fixed["input_ids"]) == cap and np.array_equal(fixed["win_offs"], sized["win_offs"])
        for name in ("input_ids", "attention_mask", "token_type_ids", "overflow_to_sample_mapping", "window_start", "lengths"):
            assert np.array_equal(fixed[name][:k], sized[name][:k]), name


def test_python_layer_errors(toks):
    from akshar_amd import engine
    with pytest.raises(ValueError, match="pad"):
        toks["spm"].encode_windows(["a"], 4)
    with pytest.raises(ValueError, match="truncation"):
        toks["bpe"].encode_windows(["a"], 8, text_pair=["b"], truncation="do_not_truncate")
    with pytest.raises(ValueError):
        toks["bpe"].encode_windows(["a"], 8, stride=1, text_pair=["b"], truncation="longest_first")
    with pytest.raises(ValueError):
        toks["bpe"].encode_windows(["a"], 2)  # no room for a body id between <s> and </s>
    with pytest.raises(ValueError):
        toks["bpe"].encode_windows(["a"], 8, stride=6)
    with pytest.raises(ValueError):
        toks["bpe"].encode_windows(["a"], 8, padding_side="up")
    with pytest.raises(ValueError):
        toks["bpe"].encode_windows(["a", "b"], 8, text_pair=["c"])
    with pytest.raises(ValueError):
        toks["bpe"].encode_windows(["a"], 8, text_pair=["c"], max_fixed_length=-1)
    big = toks["bpe"].encode_windows(["a b c d e f g h i j"], 8, text_pair=["c"], max_fixed_length=99)  # lowered to 5
    assert torch.equal(big["input_ids"], toks["bpe"].encode_windows(["a b c d e f g h i j"], 8, text_pair=["c"])["input_ids"])
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        engine.window_ids(ids.long(), offs, 4, 0)
    with pytest.raises(TypeError):
        engine.window_ids(ids, offs, 4, 0, fixed=(ids, offs.int()))
    with pytest.raises(TypeError):
        engine.window_ids(ids, offs, 4, 0, dtype=torch.int16)
    for kw in ({"fixed_cap": 2}, {"fixed_last": True}, {"longest_first": True}, {"stride": 4}, {"max_windows": -1},
               {"fixed": (ids, offs), "fixed_cap": 4}, {"fixed": (ids, offs), "longest_first": True, "stride": 1}):
        with pytest.raises(ValueError):
            engine.window_ids(ids, offs, 4, 0, **kw)
