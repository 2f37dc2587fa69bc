"""Pass N of the BPE tile kernel at 128 V entries per step with pass S folded in (ak_tile.h
AK_TILE_WIDE) on the device: the rows of tests/wide_n_rows.py (every edge of such a step under
elongation runs, pre-token starts, dropped and remapped chars, rare code points, row marks, the
T_SCAP limit) with tiles of one row, of four and of as many as fit, and 20 k synthetic rows of each
kind, against the oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import wide_n_rows as R
from tests.util import pack_rows, rows_ints

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from akshar_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.fixture(scope="module")
def bpe(eng, bpe_model):
    return eng.BPE(bpe_model)


@pytest.fixture(scope="module")
def batch(bpe_model):
    buf, offs = pack_rows(R.all_rows())
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    return buf, offs, rows_ints(ref, ro)


def _device_rows(eng, buf, offs):
    pad = np.zeros(((len(buf) + 15) // 16) * 16 + 16, dtype=np.uint8)
    pad[:len(buf)] = buf
    return eng.to_device(pad, np.asarray(offs).astype(np.int64))


@pytest.mark.parametrize("rows", [1, 4, None])
def test_wide_n_rows_vs_oracle(eng, bpe, batch, monkeypatch, rows):
    """Tiles of one row, of four rows (the row set's 4-row groups) and of as many as fit (the
    default); every row is valid UTF-8, so every status is 0; the rows that trip the HF-NFC quick
    check, the tile over T_SCAP and the 768-byte row of 256 pre-tokens take the fallback kernels."""
    buf, offs, ref = batch
    if rows is None:
        monkeypatch.delenv("AK_TILE_ROWS", raising=False)
    else:
        monkeypatch.setenv("AK_TILE_ROWS", str(rows))
    gb, go = _device_rows(eng, buf, offs)
    st = torch.zeros(len(offs) - 1, dtype=torch.uint8, device=gb.device)
    ids, oo = bpe.encode_batch(gb, go, row_status=st, path=1)
    fb = eng.fallback_rows()[0]
    got = rows_ints(ids.cpu().numpy(), oo.cpu().numpy())
    bad = [i for i, (g, r) in enumerate(zip(got, ref)) if g != r]
    assert bad == []
    assert not st.cpu().numpy().any()
    assert len(R.hf_trip_rows()) + 2 <= fb < len(offs) - 1


@pytest.mark.parametrize("kind", [0, 1, 3])
def test_synthetic_rows_vs_oracle(eng, bpe, bpe_model, kind):
    """20 k rows of Devanagari (0), Hinglish (1: the bench's) and IME-typed Hindi (3); kinds 1 and 3
    send no row to the fallback kernels."""
    from akshar_amd import synth
    buf, offs = synth.generate(kind, 20000, seed=1500 + kind)
    gb, go = _device_rows(eng, buf, offs)
    ids, oo = bpe.encode_batch(gb, go, path=1)
    fb = eng.fallback_rows()[0]
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    assert np.array_equal(oo.cpu().numpy().astype(np.uint64), ro) and np.array_equal(ids.cpu().numpy().astype(ref.dtype), ref)
    if kind in (1, 3):
        assert fb == 0
