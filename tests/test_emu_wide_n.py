"""Pass N of the BPE tile kernel at 128 V entries per step and pass S folded into it (ak_tile.h
AK_TILE_WIDE bits TW_N = 4 and TW_NS = 16) on the host emulator: rows built to hit every edge of
such a step (tests/wide_n_rows.py) against the oracle, with tiles of one, a few and many rows, for
the 64-wide code (AK_TILE_WIDE=0), the default build, each new bit alone on top of TW_D1 (TW_NS brings the wide pass N with it) and every
bit together; all builds must agree on ids, offsets, row statuses and the rows sent to the
fallback kernels."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import wide_n_rows as R
from tests.emu import emu
from tests.util import pack_rows, rows_ints

TW_D1, TW_N, TW_F, TW_NS = 1, 4, 8, 16
BUILDS = (0, None, TW_D1 | TW_N, TW_D1 | TW_NS, TW_D1 | TW_N | TW_F | TW_NS)


@pytest.fixture(scope="module")
def batch(bpe_model):
    buf, offs = pack_rows(R.all_rows())
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    return buf, offs, rows_ints(ref, ro)


def _emu_build(monkeypatch, wide):
    """The emulator built with AK_TILE_WIDE=wide (None: the default), loaded for this test only."""
    if wide is not None:
        monkeypatch.setenv("AK_EMU_DEFINES", "AK_TILE_WIDE=%d" % wide)
    else:
        monkeypatch.delenv("AK_EMU_DEFINES", raising=False)
    monkeypatch.setattr(emu, "_L", None)


def test_row_set_reaches_the_edges():
    """The row set holds what its docstrings promise, worked out from the rows themselves: V lengths
    126..130 and 254..258 as one-row and as 4-row tiles; </s><s> pairs inside a lane's pair, over two
    lanes and over entries 127 | 128 and 255 | 256; elongation runs starting at odd and even entries
    and straddling 127 | 128; a pre-token start at entry 127 with its second symbol at 128, a
    single-symbol pre-token there and at a row's end; rare chars at odd and even entries and at
    127 and 128; tiles of exactly T_SCAP, T_SCAP + 1 and 256 two-symbol pre-tokens."""
    assert {len(r) + 2 for r in R.length_rows()} == set(R.STEP_LENS)
    groups = R.tile_groups()
    assert set(R.STEP_LENS) <= {R.v_len(g) for g in groups}
    ends = {e for g in groups for e in R.mark_pairs(g)}
    assert any(e % 2 == 0 for e in ends) and any(e % 2 == 1 for e in ends) and {127, 255} <= ends
    flat = R.all_rows()
    assert flat[:len(groups) * R.GROUP] == [r.encode() for g in groups for r in g]  # groups start at row 0: 4-row tiles
    # elongation: the run "zzz" + starts at V entry k + 1 in fill(k) + run
    starts = {r.index("zzz") + 1 for r in R.elongation_rows() if "zzz" in r and r.isascii() and "\n" not in r}
    assert {1, 2, 3, 4, 125, 126, 127, 128, 255, 256} <= starts
    assert any("\n" in r for r in R.elongation_rows()) and any("क" * 4 in r for r in R.elongation_rows())
    # a kept char whose previous kept char is 1 and 2 fully dropped pairs back: runs of 3 and 5 starting
    # at an odd entry (the run's first char is kept at 2l + 1, the pairs after it are dropped)
    assert any(r.index("zzz") % 2 == 0 and "zzzq" in r and "zzzz" not in r for r in R.elongation_rows() if "zzz" in r)
    assert any(r.index("zzz") % 2 == 0 and "zzzzzq" in r and "zzzzzz" not in r for r in R.elongation_rows() if "zzz" in r)
    pt = R.pretoken_rows()
    assert any(r.find(" xy") + 2 == 127 and r.endswith("xy") for r in pt)       # start at 127, second symbol at 128, ends the row
    assert any(r.find(" xy") + 2 == 255 for r in pt)
    assert any(r.find(" x yz") + 2 == 127 for r in pt)                          # one symbol at a step's last entry
    assert any(r.endswith(" x") for r in pt)                                     # ... and as the tile's last
    assert {r.index(" x") % 2 for r in pt if " x" in r} == {0, 1}               # starts at even and odd entries
    assert {0, 1, 126, 127} <= set(R.RARE_AT)                                    # entries 1, 2 (odd, even), 127, 128
    assert any(R.NBSP + R.EMSP in r and r.index(R.NBSP) + 1 == 127 for r in R.dropped_rows())
    assert any(R.CJK in r for r in R.dropped_rows())
    sc = R.scap_rows()
    assert sorted(r.count("ab ") for r in sc if "ab " in r) == [R.T_SCAP, R.T_SCAP + 1, 256]
    assert len(sc[0]) + 3 * R.T_SCAP > 768 and len(sc[9]) == 768


@pytest.mark.parametrize("wide", BUILDS)
@pytest.mark.parametrize("rows", [1, 4, 16])
def test_wide_n_vs_oracle(bpe_model, batch, monkeypatch, rows, wide):
    buf, offs, ref = batch
    _emu_build(monkeypatch, wide)
    ids, oo, st = emu.bpe_tiles(emu.Model(bpe=bpe_model), buf, offs, rows=rows)
    got = rows_ints(ids, oo)
    bad = [i for i, (g, r) in enumerate(zip(got, ref)) if g != r]
    assert bad == []
    assert not st.any()  # every row is valid UTF-8


@pytest.mark.parametrize("rows", [1, 4, 16])
def test_builds_agree(bpe_model, batch, monkeypatch, rows):
    """Same ids, offsets, statuses, and the same number of rows sent to the fallback kernels and
    finished by the fallback waves, whichever passes run wide."""
    buf, offs, _ = batch
    res = []
    for wide in BUILDS:
        _emu_build(monkeypatch, wide)
        ids, oo, st = emu.bpe_tiles(emu.Model(bpe=bpe_model), buf, offs, rows=rows)
        res.append((ids, oo, st, emu.last_fallback_rows(), emu.last_nfc_rows()))
    for r in res[1:]:
        assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1]) and np.array_equal(r[2], res[0][2])
        assert r[3:] == res[0][3:]
    assert 0 < res[0][3] < len(offs) - 1


@pytest.mark.parametrize("wide", BUILDS)
def test_rare_rows_reach_the_fallback_kernels(bpe_model, monkeypatch, wide):
    """Every row that trips pass N's HF-NFC quick check goes to the fallback kernels, wherever in a
    lane's pair and a step the tripping char sits; a tile of more than T_SCAP listed pre-tokens sends
    its rows there and one of exactly T_SCAP does not; all equal the oracle."""
    _emu_build(monkeypatch, wide)
    m = emu.Model(bpe=bpe_model)
    orc = O.OracleBPE(bpe_model)
    for raw, nfb in ((R.hf_trip_rows(), len(R.hf_trip_rows())), (R.scap_rows()[1:5], 0), (R.scap_rows()[5:9], 4),
                     (R.scap_rows()[9:10], 1)):
        buf, offs = pack_rows([r.encode() for r in raw])
        ids, oo, _ = emu.bpe_tiles(m, buf, offs, rows=4)
        assert emu.last_fallback_rows() == nfb
        ref, ro = orc.encode_batch(buf, offs)
        assert rows_ints(ids, oo) == rows_ints(ref, ro)


@pytest.mark.parametrize("kind", [1, 3])
def test_synthetic_rows_vs_oracle(bpe_model, monkeypatch, kind):
    """Bench-like rows (kind 1) and IME-typed Hindi (kind 3) with every bit on: the oracle's ids, no
    fallback row."""
    from akshar_amd import synth
    buf, offs = synth.generate(kind, 400, seed=900 + kind)
    _emu_build(monkeypatch, TW_D1 | TW_N | TW_F | TW_NS)
    ids, oo, _ = emu.bpe_tiles(emu.Model(bpe=bpe_model), buf, offs, rows=16)
    assert emu.last_fallback_rows() == 0
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    assert np.array_equal(oo, ro) and np.array_equal(ids, ref)
