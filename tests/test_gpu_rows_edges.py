"""The row-op tile kernel (ak_tile_rows.h: normalize, segment, switches, analyze at flags 3) and the
SentencePiece tile kernel (ak_tile_spm.h) on the device at their step edges and limits: the rows of
tests/rows_edge_rows.py, replicated so many waves and the unit queue see them, against the
reference's recorded answers (tests/golden/rows_edges.jsonl.gz) and the oracle, with tiles of 1 row,
4 rows and as many as fit (AK_TILE_ROWS). Bit-exact; and every call must have taken the path its
rows were built for: the engine's fallback counters equal the numbers counted from the row list."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import rows_edge_rows as R
from tests.util import ends_to_lens, pack_rows, rows_ints, rows_runs, rows_u8

pytestmark = pytest.mark.gpu
REP = 40
TILE_ROWS = [None, "1", "4"]


@pytest.fixture(scope="module")
def eng():
    from akshar_amd import engine
    assert torch.cuda.is_available()
    return engine


def _tile_rows(monkeypatch, v):
    if v is None:
        monkeypatch.delenv("AK_TILE_ROWS", raising=False)
    else:
        monkeypatch.setenv("AK_TILE_ROWS", v)


def _rep(out, oo, rep):
    """A batch's packed output, the batch repeated `rep` times."""
    oo = np.asarray(oo).astype(np.int64)
    offs = np.concatenate([oo[:-1] + k * oo[-1] for k in range(rep)] + [np.asarray([rep * oo[-1]])])
    return np.tile(np.asarray(out)[:oo[-1]], rep), offs


def _device_rows(eng, rows, rep):
    buf, offs = pack_rows(rows)
    nb = int(offs[-1])
    big, boffs = _rep(buf[:nb], offs, rep)
    pad = np.zeros(((len(big) + 15) // 16) * 16 + 16, dtype=np.uint8)
    pad[:len(big)] = big
    return eng.to_device(pad, boffs)


def _batch(eng, name, rows, rep):
    buf, offs = pack_rows(rows)
    want, _ = R.golden(name)
    assert sorted(want) == [i for i, r in enumerate(rows) if R.is_valid(r)]
    gb, go = _device_rows(eng, rows, rep)
    return {"rows": rows, "n": len(rows), "want": want, "gb": gb, "go": go,
            "norm": O.normalize_batch(buf, offs, 3), "sw": O.switches_batch(buf, offs, 3),
            False: O.segment_batch(buf, offs, 3, False), True: O.segment_batch(buf, offs, 3, True),
            "invalid": np.tile(np.asarray([0 if R.is_valid(r) else 1 for r in rows], dtype=np.uint8), rep),
            "leave": rep * sum(R.leaves_the_tile(r) for r in rows),
            "waves_finish": rep * sum(1 for r in rows if R.leaves_the_tile(r) and R.is_valid(r) and len(r) <= R.R_BCAP)}


@pytest.fixture(scope="module")
def tile_batch(eng):
    return _batch(eng, "rows", R.all_rows(), REP)


@pytest.fixture(scope="module")
def nfc_batch(eng):
    return _batch(eng, "nfc", R.nfc_rows(), REP)


def _cpu(t):
    return t.cpu().numpy()


def _eq(got, ref, rep):
    """Device arrays (values..., offsets) == the oracle's (values..., offsets) repeated."""
    oo = ref[-1]
    ok = True
    for g, r in zip(got[:-1], ref[:-1]):
        want, offs = _rep(r, oo, rep)
        ok = ok and np.array_equal(_cpu(g).astype(np.int64), want.astype(np.int64))
    return ok and np.array_equal(_cpu(got[-1]).astype(np.int64), offs)


def _first(t, oo, n):
    """The first copy of the batch in a device output."""
    o = _cpu(oo)[:n + 1]
    return [_cpu(x)[:o[-1]] for x in t] + [o]


def _path(eng, b):
    """The engine's counters after a tile-path call: the rows that left the tile kernel, and those
    the fallback waves finished."""
    d = eng.fallback_detail()
    assert eng.fallback_rows()[0] == b["leave"] == d["rows"]
    assert d["finished_in_tile_path"] == b["waves_finish"]


def _run_ops(eng, b, monkeypatch, tile_rows):
    _tile_rows(monkeypatch, tile_rows)
    gb, go, n, want = b["gb"], b["go"], b["n"], b["want"]
    st = torch.full((n * REP,), 7, dtype=torch.uint8, device=gb.device)
    norm = eng.normalize_batch(gb, go, flags=3, row_status=st, path=1)
    _path(eng, b)
    assert _eq(norm, b["norm"], REP)
    assert np.array_equal(_cpu(st) & 1, b["invalid"])
    got = rows_u8(*_first(norm[:1], norm[1], n))
    assert [i for i, r in want.items() if got[i] != r["norm"]] == []
    n0 = eng.normalize_batch(gb, go, flags=3, path=0)
    assert torch.equal(n0[0], norm[0]) and torch.equal(n0[1], norm[1])
    sw = eng.switches_batch(gb, go, flags=3, row_status=st, path=1)
    _path(eng, b)
    assert _eq(sw, b["sw"], REP)
    got = rows_runs(*_first(sw[:2], sw[2], n))
    assert [i for i, r in want.items() if got[i] != r["sw"]] == []
    s0 = eng.switches_batch(gb, go, flags=3, path=0)
    assert all(torch.equal(a, c) for a, c in zip(s0, sw))
    for matras, key in ((False, "ak"), (True, "ak_m")):
        st.fill_(7)
        seg = eng.segment_batch(gb, go, flags=3, matras=matras, row_status=st, path=1)
        _path(eng, b)
        assert _eq(seg, b[matras], REP)
        assert np.array_equal(_cpu(st) & 1, b["invalid"])
        got = rows_ints(*_first(seg[:1], seg[1], n))
        assert [i for i, r in want.items() if ends_to_lens(got[i]) != r[key]] == []
        g0 = eng.segment_batch(gb, go, flags=3, matras=matras, path=0)
        assert torch.equal(g0[0], seg[0]) and torch.equal(g0[1], seg[1])
        st.fill_(7)
        an = eng.analyze_batch(gb, go, flags=3, matras=matras, row_status=st, path=1)
        _path(eng, b)
        assert np.array_equal(_cpu(st) & 1, b["invalid"])
        # the fused analyze equals the single ops
        assert torch.equal(an[0], norm[0]) and torch.equal(an[1], norm[1])
        assert torch.equal(an[2], seg[0]) and torch.equal(an[3], seg[1])
        assert torch.equal(an[4], sw[0]) and torch.equal(an[5], sw[1]) and torch.equal(an[6], sw[2])
        a0 = eng.analyze_batch(gb, go, flags=3, matras=matras, path=0)
        assert all(torch.equal(a, c) for a, c in zip(a0, an))


@pytest.mark.parametrize("tile_rows", TILE_ROWS)
def test_tile_rows_at_step_edges(eng, tile_batch, monkeypatch, tile_rows):
    """Only the rows over the tile buffer leave the tile kernel (the one-lane kernel takes them)."""
    assert tile_batch["leave"] == REP * len(R.OVER_BUFFER) and tile_batch["waves_finish"] == 0
    _run_ops(eng, tile_batch, monkeypatch, tile_rows)


@pytest.mark.parametrize("tile_rows", TILE_ROWS)
def test_epoch_text_at_step_edges(eng, nfc_batch, monkeypatch, tile_rows):
    """The same constructs as the fallback waves' epoch text (rows_tile<OPS, NFCD>): every row
    leaves the tile kernel; the waves finish every valid row within the buffer."""
    assert nfc_batch["leave"] == REP * nfc_batch["n"] and nfc_batch["waves_finish"] > 0.85 * nfc_batch["leave"]
    _run_ops(eng, nfc_batch, monkeypatch, tile_rows)


# ---------------------------------------------------------------- SentencePiece
@pytest.fixture(scope="module")
def spm_batch(eng, spm_model):
    rows = R.spm_rows()
    buf, offs = pack_rows(rows)
    want, _ = R.golden("spm")
    assert sorted(want) == [i for i, r in enumerate(rows) if R.is_valid(r)]
    gb, go = _device_rows(eng, rows, REP)
    invalid = [0 if R.is_valid(r) else 1 for r in rows]
    return {"rows": rows, "n": len(rows), "want": want, "gb": gb, "go": go,
            "ref": O.OracleSPM(spm_model).encode_batch(buf, offs), "invalid": invalid,
            "long_word": [i in want and R.has_long_word(want[i]["norm"]) for i in range(len(rows))]}


@pytest.mark.parametrize("tile_rows", TILE_ROWS)
@pytest.mark.parametrize("variant", ["pooled", "tile", "default"])
def test_spm_rows_at_the_limits(eng, spm_model, spm_batch, monkeypatch, variant, tile_rows):
    """Pooled (AK_SPM_POOL_ROWS=0), the tile variant (AK_SPM_POOL=0) and the default (the tile variant
    at this size). Rows that leave the tile kernel: the invalid ones and those over its staged bytes
    (S_BCAP = 480; SP_BCAP = 1,024 pooled: none); the pool sends back exactly the rows with a word
    over SP_MAXL, and the one of those over 480 bytes goes on to the fallback kernels."""
    b = spm_batch
    _tile_rows(monkeypatch, tile_rows)
    if variant == "pooled":
        monkeypatch.setenv("AK_SPM_POOL_ROWS", "0")
    elif variant == "tile":
        monkeypatch.setenv("AK_SPM_POOL", "0")
    pooled = variant == "pooled"
    m = eng.SPM(spm_model)  # (the model reads the two variables when it is built)
    st = torch.full((b["n"] * REP,), 7, dtype=torch.uint8, device=b["gb"].device)
    ids = m.encode_batch(b["gb"], b["go"], row_status=st, path=1)
    fb = [bool(bad) or len(r) > (R.SP_BCAP if pooled and not lw else R.S_BCAP)
          for r, bad, lw in zip(b["rows"], b["invalid"], b["long_word"])]
    redo = sum(b["long_word"]) if pooled else 0
    passed_on = sum(1 for f, lw in zip(fb, b["long_word"]) if f and lw) if pooled else 0
    assert eng.fallback_rows()[0] == REP * sum(fb)
    assert eng.fallback_detail()["rows"] == REP * (sum(fb) + redo - passed_on)
    assert _eq(ids, b["ref"], REP)
    assert np.array_equal(_cpu(st) & 1, np.tile(np.asarray(b["invalid"], dtype=np.uint8), REP))
    got = rows_ints(*_first(ids[:1], ids[1], b["n"]))
    assert [i for i, r in b["want"].items() if got[i] != r["spm"]] == []
    i0 = m.encode_batch(b["gb"], b["go"], path=0)
    assert torch.equal(i0[0], ids[0]) and torch.equal(i0[1], ids[1])
    if variant == "default" and tile_rows is None:  # the one-kernel path with the start-parallel tile
        for i, r in b["want"].items():
            if len(b["rows"][i]) <= R.S_BCAP:
                assert m.encode_host(b["rows"][i]).tolist() == r["spm"], i


def test_spm_word_pool_ring_bound(eng, spm_model, monkeypatch):
    """The word pool's ring at its bound (ak_tile_spm.h SP_RING >= 63 + a tile's words of one length
    class): tests/rows_edge_rows.py spm_ring_texts, 300 units, pooled at this size."""
    texts = R.spm_ring_texts(300)
    monkeypatch.setenv("AK_SPM_POOL_ROWS", "0")
    monkeypatch.delenv("AK_TILE_ROWS", raising=False)
    ids, oo = eng.SPM(spm_model).encode_batch(*eng.pack(texts))
    # every row fits a pooled tile and no tile passes S_WORDS: only rows NFC changes may leave it
    import unicodedata
    assert eng.fallback_rows()[0] <= sum(unicodedata.normalize("NFC", t) != t for t in texts) < 100
    ref, ro = O.OracleSPM(spm_model).encode_batch(*O.pack(texts))
    assert np.array_equal(_cpu(oo).astype(np.uint64), ro) and np.array_equal(_cpu(ids).astype(np.uint32), ref)
