"""ONE workspace through calls of changing size and kind: the tile launchers share its lists
(fb2, fb3, unit_fb, unit_len, the pools, the epoch buffers), each grown by whichever launcher needed
more first, so the later small calls run on buffers the earlier large ones grew and the large ones on
buffers the small ones left. Every batch holds a row for each fallback path; every output is the
oracle's, bit for bit, and ak_ws_check stays AK_OK after each call."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.util import oracle_bad_rows, pack_rows

pytestmark = pytest.mark.gpu

FAST_SEG, FAST_WORD, FAST_VCAP = 8, 32, 48  # akshar_amd/csrc/ak_rows.h: the one-lane kernels' fast buffers
NFC_ROW = "a\u0301\u0323 b \u0928\u094d\u093c\u093e yaar".encode()  # marks out of canonical order: the fallback waves
BAD_ROW = b"kal a\x80b milte"                                       # invalid UTF-8: the one-lane kernel (fb3)
LONG_ROW = ("namaste dost " * 60).encode()                          # 780 bytes: over the 768-byte tile buffer
# past the fast buffers into the slow tier (fb2): an NFC segment of 2 x FAST_SEG marks, and one word of
# more symbols than FAST_WORD and FAST_VCAP, in a row no tile holds
SLOW_ROW = ("e" + "\u0301" * (2 * FAST_SEG) + " " + "abcdefghij" * (2 * FAST_VCAP)).encode()
ALL_ROW = NFC_ROW + b" \xe0\xa4 " + SLOW_ROW                        # all four at once (the 1-row batch)
assert len(LONG_ROW) > 768 and len(SLOW_ROW) > 768 and 10 * 2 * FAST_VCAP > max(FAST_WORD, FAST_VCAP)

# (op, rows) in call order: 65 rows cross a 64-row unit, so unit_fb / unit_len grow
CALLS = (("bpe", 1), ("bpe", 65), ("spm", 200), ("analyze", 130), ("bpe", 3), ("spm", 65))


def _batch(n, seed):
    from akshar_amd import synth
    special = [ALL_ROW, NFC_ROW, BAD_ROW, LONG_ROW, SLOW_ROW][:n]
    rows = [r.encode() for r in synth.lines(synth.KIND_HINGLISH, n - len(special), seed=seed)] if n > len(special) else []
    for k, s in enumerate(special):  # spread over the batch, the first one in the last unit
        rows.insert((len(rows) - 7 * k) % (len(rows) + 1), s)
    assert len(rows) == n
    return rows


def _oracle(op, buf, offs, bpe_model, spm_model):
    if op == "bpe":
        return O.OracleBPE(bpe_model).encode_batch(buf, offs)
    if op == "spm":
        return O.OracleSPM(spm_model).encode_batch(buf, offs)
    norm, no = O.normalize_batch(buf, offs, flags=3)  # analyze: segment / switches of the normalized text
    return (norm, no) + O.segment_batch(norm, no, flags=-1) + O.switches_batch(norm, no, flags=-1)


def test_one_workspace_across_growth(bpe_model, spm_model):
    from akshar_amd import _lib, engine
    assert torch.cuda.is_available()
    bpe, spm = engine.BPE(bpe_model), engine.SPM(spm_model)
    ws = engine.workspace(bpe.dev.index)
    for k, (op, n) in enumerate(CALLS):
        rows = _batch(n, seed=100 + k)
        buf, offs = pack_rows(rows)
        want = _oracle(op, buf, offs, bpe_model, spm_model)
        bad = oracle_bad_rows(buf, offs)
        assert bad.any()
        pad = np.zeros((len(buf) + 15) // 16 * 16 + 16, dtype=np.uint8)
        pad[:int(offs[-1])] = buf[:int(offs[-1])]
        gb, go = engine.to_device(pad, offs.astype(np.int64))
        status = torch.full((n,), 0x77, dtype=torch.uint8, device=gb.device)
        if op == "analyze":
            got = engine.analyze_batch(gb, go, row_status=status)
        else:
            got = (bpe if op == "bpe" else spm).encode_batch(gb, go, row_status=status)
        assert engine.workspace(bpe.dev.index) is ws  # the same ak_ws for every call
        assert _lib.lib().ak_ws_check(ws) == _lib.AK_OK, (k, op, n)
        assert len(got) == len(want)
        for j, (g, r) in enumerate(zip(got, want)):
            g = g.cpu().numpy()
            assert np.array_equal(g.astype(np.int64), np.asarray(r).astype(np.int64)), (k, op, n, "output %d" % j)
        assert np.array_equal(status.cpu().numpy(), bad), (k, op, n, "row_status")
