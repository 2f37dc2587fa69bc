"""The one-lane row pipeline's output contract on the host (the CPU mirror of tests/test_gpu_buffers.py
part A): `emu_run` runs the device row code (count / scan / emit through ak_dev.h's Cursor, the
switch labels beside it) with a caller's capacity. For the batch of tests.util.buffer_batch and every
capacity of tests.util.buffer_capacities: out_offs[0..n] equal the oracle's whatever the capacity
(out_offs[n] is the required total), nothing is stored at or past `cap` (every output lies in a numpy
array with a sentinel-filled guard band), and with the exact capacity the output equals the oracle.
What lies below a short capacity is not asserted (include/akshar.h: "incomplete").

The tile copy kernels live in the .hip files and are not emulated; the GPU module covers them.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests.emu import emu
from tests.util import BUFFER_GUARD as G, buffer_batch, buffer_capacities, pack_rows

S32 = 0x7A7A7A7A           # above any id or code point index, and not STAGE_DEAD
S64 = 0x7A7A7A7A7A7A7A7A
S_TEXT, S_LABEL = 0xFF, 0x77  # 0xFF is no UTF-8 byte; labels are 0, 1, 2 or 255


@pytest.fixture(scope="module")
def batch():
    buf, offs = pack_rows(buffer_batch())
    return emu.pad(buf), buf, offs


# op, flags, matras, model, what the oracle says
CASES = [
    ("normalize-3", 0, 3, False, None, lambda b, o, m: O.normalize_batch(b, o, flags=3)),
    ("normalize-0", 0, 0, False, None, lambda b, o, m: O.normalize_batch(b, o, flags=0)),
    ("segment-3", 1, 3, False, None, lambda b, o, m: O.segment_batch(b, o, flags=3)),
    ("segment-3-matras", 1, 3, True, None, lambda b, o, m: O.segment_batch(b, o, flags=3, matras=True)),
    ("segment-raw", 1, -1, False, None, lambda b, o, m: O.segment_batch(b, o, flags=-1)),
    ("switches-3", 2, 3, False, None, lambda b, o, m: O.switches_batch(b, o, flags=3)),
    ("bpe-3", 3, 3, False, "bpe", lambda b, o, m: O.OracleBPE(m).encode_batch(b, o)),
    ("bpe-1", 3, 1, False, "bpe", lambda b, o, m: O.OracleBPE(m).encode_batch(b, o, flags=1)),
    ("spm-3", 4, 3, False, "spm", lambda b, o, m: O.OracleSPM(m).encode_batch(b, o)),
]


@pytest.mark.parametrize("name,op,flags,matras,model,ref", CASES, ids=[c[0] for c in CASES])
def test_row_pipeline_capacity_and_guard_bands(batch, bpe_model, spm_model, name, op, flags, matras, model, ref):
    padded, buf, offs = batch
    n = len(offs) - 1
    pm = {"bpe": bpe_model, "spm": spm_model}.get(model)
    em = emu.Model(bpe=pm) if model == "bpe" else emu.Model(spm=pm) if model == "spm" else None
    want = ref(buf, offs, pm)
    want, want_labels, want_oo = (want[0], want[1], want[2]) if op == 2 else (want[0], None, want[1])
    total = int(want_oo[-1])
    assert total == len(want) and total > n
    u8 = op == 0
    for cap in buffer_capacities(want_oo, u8):
        out = np.full(cap + G, S_TEXT if u8 else S32, dtype=np.uint8 if u8 else np.uint32)
        labels = np.full(cap + G, S_LABEL, dtype=np.uint8)
        oo = np.full(n + 1 + G, S64, dtype=np.uint64)
        tot = emu.lib().emu_run(op, flags, int(matras), em.h if em else None, padded.ctypes.data, offs.ctypes.data, n,
                                out.ctypes.data, labels.ctypes.data, cap, oo.ctypes.data)
        assert tot == total, (name, cap)
        assert np.array_equal(oo[:n + 1], want_oo), (name, cap)
        assert (oo[n + 1:] == S64).all(), (name, cap)
        assert (out[cap:] == (S_TEXT if u8 else S32)).all(), (name, cap, np.flatnonzero(out[cap:] != out[-1])[:4])
        if op == 2:
            assert (labels[cap:] == S_LABEL).all(), (name, cap)
        else:
            assert (labels == S_LABEL).all(), (name, cap)  # no other op has labels
        if cap == total:
            assert np.array_equal(out[:total], want), name
            if op == 2:
                assert np.array_equal(labels[:total], want_labels), name
