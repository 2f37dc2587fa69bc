"""The 128-element sweep steps of the BPE tile kernel (ak_tile.h AK_TILE_WIDE: pass D1 over the whole
tile, pass F; two adjacent elements per lane) on the host emulator: rows built to hit every edge of
such a step (tests/wide_rows.py) against the oracle, with tiles of one, a few and many rows, for the
default build, the 64-wide code alone (AK_TILE_WIDE=0) and every wide part (AK_TILE_WIDE=9); the
three builds must also agree on the rows sent to the fallback kernels and on the row statuses."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import wide_rows
from tests.emu import emu
from tests.util import pack_rows, rows_ints


@pytest.fixture(scope="module")
def batch(bpe_model):
    buf, offs = pack_rows(wide_rows.all_rows())
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
    """The row set holds, for every edge count, a one-row tile with exactly that many P entries
    (its mark + its chars) and bytes at odd and even positions; marks at odd and even P indices."""
    rows = wide_rows.count_rows()
    chars = {len(r) for r in rows}
    assert all(n - 1 in chars for n in wide_rows.EDGES)
    assert any(len(r.encode()) != len(r) for r in rows)
    marks = wide_rows.mark_rows()
    assert "" in marks and any(len(r.encode()) == 768 for r in marks) and any(len(r.encode()) == 769 for r in marks)
    parity, idx = set(), 0
    for r in marks[:8]:  # P index of each row's mark in one tile: rows before it + their chars
        parity.add(idx & 1)
        idx += 1 + len(r)
    assert parity == {0, 1}


@pytest.mark.parametrize("wide", [None, 0, 9])
@pytest.mark.parametrize("rows", [1, 4, 16])
def test_wide_steps_vs_oracle(bpe_model, batch, monkeypatch, rows, wide):
    buf, offs, ref = batch
    _emu_build(monkeypatch, wide)
    ids, oo, st = emu.bpe_tiles(emu.Model(bpe=bpe_model), buf, offs, rows=rows)
    got = rows_ints(ids, oo)
    bad = [i for i, (g, r) in enumerate(zip(got, ref)) if g != r]
    assert bad == []
    # invalid UTF-8 rows (and only those) are flagged
    raw = wide_rows.all_rows()
    inv = []
    for r in raw:
        try:
            r.decode("utf-8")
            inv.append(0)
        except UnicodeDecodeError:
            inv.append(1)
    assert st.tolist() == inv


@pytest.mark.parametrize("rows", [1, 4, 16])
def test_wide_and_narrow_builds_agree(bpe_model, batch, monkeypatch, rows):
    """Same ids, offsets, statuses and the same number of rows sent to the fallback kernels and
    finished by the fallback waves, whichever sweeps run wide."""
    buf, offs, _ = batch
    res = []
    for wide in (0, 1, 9):
        _emu_build(monkeypatch, wide)
        ids, oo, st = emu.bpe_tiles(emu.Model(bpe=bpe_model), buf, offs, rows=rows)
        res.append((ids, oo, st, emu.last_fallback_rows(), emu.last_nfc_rows()))
    for r in res[1:]:
        assert np.array_equal(r[0], res[0][0]) and np.array_equal(r[1], res[0][1]) and np.array_equal(r[2], res[0][2])
        assert r[3:] == res[0][3:]
    assert 0 < res[0][3] < len(offs) - 1  # the 769-byte row, the invalid rows; most rows stay in the tile


@pytest.mark.parametrize("kind", [1, 3])
def test_synthetic_rows_wide_vs_oracle(bpe_model, monkeypatch, kind):
    """Bench-like rows (kind 1) and IME-typed Hindi (kind 3: the nukta expansion) with every wide
    part on: the oracle's ids, no fallback row."""
    from akshar_amd import synth
    buf, offs = synth.generate(kind, 400, seed=700 + kind)
    _emu_build(monkeypatch, 9)
    ids, oo, _ = emu.bpe_tiles(emu.Model(bpe=bpe_model), buf, offs, rows=16)
    assert emu.last_fallback_rows() == 0
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    assert np.array_equal(oo, ro) and np.array_equal(ids, ref)
