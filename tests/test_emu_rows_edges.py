"""The row-op tile kernel (ak_tile_rows.h rows_tile: normalize, segment, switches and the fused
analyze) and the SentencePiece tile kernel (ak_tile_spm.h) on the host emulator, at their step edges
and limits: the rows of tests/rows_edge_rows.py against the reference's recorded answers
(tests/golden/rows_edges.jsonl.gz) and the oracle, with tiles of 1, 4 and 16 rows on one and on three
waves. Bit-exact. Each call must also have taken the path its rows were built for: the rows sent to
the fallback kernels, finished by the fallback waves or sent back by the word pool are counted from
the row list and compared with the emulator's counters."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import rows_edge_rows as R
from tests.emu import emu
from tests.util import ends_to_lens, pack_rows, rows_ints, rows_runs, rows_u8

SHAPES = [(1, 3), (4, 1), (16, 1), (16, 3)]  # (rows per tile, waves)


def _batch(name, rows):
    buf, offs = pack_rows(rows)
    want, meta = R.golden(name)
    ref = {"norm": rows_u8(*O.normalize_batch(buf, offs, 3)), "sw": rows_runs(*O.switches_batch(buf, offs, 3)),
           False: rows_ints(*O.segment_batch(buf, offs, 3, False)), True: rows_ints(*O.segment_batch(buf, offs, 3, True))}
    return {"rows": rows, "buf": buf, "offs": offs, "want": want, "ref": ref, "meta": meta,
            "invalid": [0 if R.is_valid(r) else 1 for r in rows], "leave": sum(R.leaves_the_tile(r) for r in rows)}


@pytest.fixture(scope="module")
def tile_batch():
    return _batch("rows", R.all_rows())


@pytest.fixture(scope="module")
def nfc_batch():
    return _batch("nfc", R.nfc_rows())


def _check(b, res, ops, matras):
    """The outputs of `ops` equal the oracle's on every row and the reference's on every valid row."""
    want = b["want"]
    if ops & 1:
        got = rows_u8(*res["norm"])
        assert [i for i, g in enumerate(got) if g != b["ref"]["norm"][i]] == []
        assert [i for i, r in want.items() if got[i] != r["norm"]] == []
    if ops & 2:
        got = rows_ints(*res["seg"])
        assert [i for i, g in enumerate(got) if g != b["ref"][matras][i]] == []
        assert [i for i, r in want.items() if ends_to_lens(got[i]) != r["ak_m" if matras else "ak"]] == []
    if ops & 4:
        got = rows_runs(*res["runs"])
        assert [i for i, g in enumerate(got) if g != b["ref"]["sw"][i]] == []
        assert [i for i, r in want.items() if got[i] != r["sw"]] == []
    assert res["status"].tolist() == b["invalid"]


def _same(a, b, key):
    return all(np.array_equal(x, y) for x, y in zip(a[key], b[key]))


def _run_all(b, rows, waves, matras, nfc_rows):
    fused = emu.rows_tiles(7, b["buf"], b["offs"], matras=matras, rows=rows, waves=waves)
    assert (emu.last_fallback_rows(), emu.last_nfc_rows()) == (b["leave"], nfc_rows)
    _check(b, fused, 7, matras)
    for ops, key in ((2, "seg"),) if matras else ((1, "norm"), (2, "seg"), (4, "runs")):  # (ops 1 and 4 take no matras)
        res = emu.rows_tiles(ops, b["buf"], b["offs"], matras=matras, rows=rows, waves=waves)
        assert (emu.last_fallback_rows(), emu.last_nfc_rows()) == (b["leave"], nfc_rows)
        _check(b, res, ops, matras)
        assert _same(res, fused, key)  # the fused analyze equals the single op


def test_row_set_reaches_the_edges(tile_batch, nfc_batch):
    """The reference answered every valid row; the rows hold what they were built to hold: a
    construct's first element at each of POS in a one-row tile, a row of exactly the tile buffer and
    one over it, empty rows, whole units for the tile shapes; only classes the tile implements pass
    the filter (so the second sweep cannot run for the normalize_text defaults)."""
    for b in (tile_batch, nfc_batch):
        assert sorted(b["want"]) == [i for i, bad in enumerate(b["invalid"]) if not bad]
        assert all(r["text"].encode("utf-8") == b["rows"][i] for i, r in b["want"].items())
    assert set(tile_batch["meta"]["gcb_kept"]) <= {"Other", "CR", "LF", "Control", "Extend", "SpacingMark", "ZWJ", "Prepend"}
    assert tile_batch["meta"]["extpict_kept"] == 0
    assert sum(tile_batch["invalid"]) == 0 and tile_batch["leave"] == len(R.OVER_BUFFER) == 2
    lens = {len(r) for r in tile_batch["rows"]}
    assert {0, R.R_BCAP, R.R_BCAP + 1} <= lens and len(R.shape_units()) % 64 == 0
    cons = R.KA + R.VIRAMA + R.SSA
    for k in R.POS:  # V_B, k - 1 fill chars, then the construct at V index k
        row = R.at(k, cons)
        assert row.index(cons) + 1 == k and row in R.gb9c_rows()
    assert {k % 64 for k in R.POS} >= {61, 62, 63, 0, 1, 2}
    # the fallback waves' batch: every valid row is changed by NFC, a few rows are invalid, one is over the buffer
    assert nfc_batch["leave"] == len(nfc_batch["rows"]) and 0 < sum(nfc_batch["invalid"]) < 20
    assert sum(len(r) > R.R_BCAP for r in nfc_batch["rows"]) == 1


@pytest.mark.parametrize("matras", [False, True])
@pytest.mark.parametrize("rows,waves", SHAPES)
def test_tile_rows_at_step_edges(tile_batch, rows, waves, matras):
    """Ops 1, 2, 4 and the fused 7: only the two rows over the tile buffer leave the tile kernel."""
    _run_all(tile_batch, rows, waves, matras, 0)


@pytest.mark.parametrize("matras", [False, True])
@pytest.mark.parametrize("rows,waves", SHAPES)
def test_epoch_text_at_step_edges(nfc_batch, rows, waves, matras):
    """The same constructs as the fallback waves' epoch text (rows_tile<OPS, NFCD>): every row
    leaves the tile kernel, and every valid row within the buffer is finished by the waves."""
    b = nfc_batch
    done = sum(1 for r in b["rows"] if R.is_valid(r) and len(r) <= R.R_BCAP)
    _run_all(b, rows, waves, matras, done)


# ---------------------------------------------------------------- SentencePiece
@pytest.fixture(scope="module")
def spm_batch(spm_model):
    rows = R.spm_rows()
    buf, offs = pack_rows(rows)
    want, _ = R.golden("spm")
    ref, ro = O.OracleSPM(spm_model).encode_batch(buf, offs)
    assert sorted(want) == [i for i, r in enumerate(rows) if R.is_valid(r)]
    return {"rows": rows, "buf": buf, "offs": offs, "want": want, "ref": rows_ints(ref, ro),
            "invalid": [0 if R.is_valid(r) else 1 for r in rows],
            "long_word": [i in want and R.has_long_word(want[i]["norm"]) for i in range(len(rows))]}


@pytest.mark.parametrize("rows", [1, 4, 16])
@pytest.mark.parametrize("variant", ["pooled", "tile", "starts"])
def test_spm_rows_at_the_limits(spm_model, spm_batch, monkeypatch, variant, rows):
    """The pooled variant (the emulator's default), the tile variant (AK_SPM_POOL=0) and the per-call
    path's start-parallel tile (AK_EMU_SPM_STARTS=1). Fallback rows: the invalid ones and those over
    the variant's staged bytes (S_BCAP = 480; SP_BCAP = 1,024 pooled: none). Sent back by the pool:
    exactly the rows with a word over SP_MAXL, which the tile variants solve in the tile; the redo
    pass solves them in one-row tiles of S_BCAP bytes, so the one such row over 480 bytes goes on to
    the fallback kernels from there."""
    b = spm_batch
    if variant != "pooled":
        monkeypatch.setenv("AK_SPM_POOL", "0")
    if variant == "starts":
        monkeypatch.setenv("AK_EMU_SPM_STARTS", "1")
    pooled = variant == "pooled"
    ids, oo, st = emu.spm_tiles(emu.Model(spm=spm_model), b["buf"], b["offs"], rows=rows, waves=3 if rows == 4 else 1)
    got = rows_ints(ids, oo)
    assert [i for i, g in enumerate(got) if g != b["ref"][i]] == []
    assert [i for i, r in b["want"].items() if got[i] != r["spm"]] == []
    assert st.tolist() == b["invalid"]
    fb = [bad or len(r) > (R.SP_BCAP if pooled and not lw else R.S_BCAP)
          for r, bad, lw in zip(b["rows"], b["invalid"], b["long_word"])]
    assert emu.last_fallback_rows() == sum(fb) and sum(b["invalid"]) < sum(fb) < 20
    assert sum(b["long_word"]) >= 8
    assert emu.last_redo_rows() == (sum(b["long_word"]) if pooled else 0)


def test_spm_word_pool_ring_rows(spm_model):
    """The ring-bound rows of the device test (tests/rows_edge_rows.py spm_ring_texts), 8 units on
    one emulated wave, pooled: every row stays in its tile (1,019 bytes of three-char words are 255
    words, under S_WORDS), none is sent back, the ids equal the oracle's."""
    buf, offs = O.pack(R.spm_ring_texts(8))
    ids, oo, _ = emu.spm_tiles(emu.Model(spm=spm_model), buf, offs, rows=16)
    assert (emu.last_fallback_rows(), emu.last_redo_rows()) == (0, 0)
    ref, ro = O.OracleSPM(spm_model).encode_batch(buf, offs)
    assert np.array_equal(oo, ro) and np.array_equal(ids, ref)
