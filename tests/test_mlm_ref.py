"""Masked-LM batches (include/akshar.h ak_ids_mlm) without a GPU: the definition restated in numpy /
plain Python, pinned to Random123's published known-answer vectors for Philox4x32-10.

  - np_philox4x32_10 (vectorised) and philox_scalar (Python ints) agree with each other and with the
    known answers;
  - np_mlm restates the header's definition; its leader rule is a forward scan that carries the
    current word's first column, not the kernel's walk to the left;
  - the selected / masked / random / kept shares lie where the binomial distribution puts them;
  - the C-ABI's host-side argument errors and the Python layer's ValueErrors.

tests/test_gpu_mlm.py holds the kernel to np_mlm, element for element. There is no golden fixture:
neither the reference project nor HF `tokenizers` has a masking collator to record.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests.conftest import ROOT

M32 = 0xFFFFFFFF
ONE = 1 << 32
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


# ------------------------------------------------------------------------------------------ restatements
def philox_scalar(ctr, key):
    """Philox4x32-10 of one counter (4 words) under one key (2 words), in Python integers."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def np_philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The same over arrays: every argument a uint64 array (or scalar) of 32-bit values; returns the
    four output words as uint64 arrays."""
    m = np.uint64(M32)
    s = np.uint64(32)
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2  # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def np_draws(n, seed, stream_id, elem_base):
    """x0..x3 of the elements elem_base .. elem_base + n - 1 (64-bit, wrapping)."""
    e = np.arange(n, dtype=np.uint64) + np.uint64(elem_base)  # array arithmetic wraps modulo 2^64
    return np_philox4x32_10(e & np.uint64(M32), e >> np.uint64(32), stream_id & M32, stream_id >> 32, seed & M32, seed >> 32)


def np_leaders(ids, elig, word_start):
    """Flat index of every eligible element's leader (-1 for the others): a forward scan of each row
    that remembers where the word in hand began."""
    rows, width = ids.shape
    lead = np.full((rows, width), -1, dtype=np.int64)
    n_vocab = 0 if word_start is None else len(word_start)
    for r in range(rows):
        first = -1  # column at which the current word began; -1: no word is open
        row, ok = ids[r].tolist(), elig[r].tolist()
        for c in range(width):
            if not ok[c]:
                first = -1
                continue
            v = row[c]
            if first < 0 or word_start is None or not 0 <= v < n_vocab or word_start[v]:
                first = c
            lead[r, c] = r * width + first
    return lead


def np_mlm(ids, attn=None, *, seed=0, stream_id=0, elem_base=0, t_select, t_mask, t_random, mask_id, rand_lo=0, rand_hi=1,
           ignore_index=-100, never=(), word_start=None):
    """(out, labels), each of ids' shape and dtype, as include/akshar.h defines ak_ids_mlm."""
    ids = np.asarray(ids)
    rows, width = ids.shape
    x0, x1, x2, _ = np_draws(rows * width, seed, stream_id, elem_base)
    elig = np.ones(ids.shape, dtype=bool) if attn is None else np.asarray(attn).reshape(ids.shape) != 0
    if len(never):
        elig &= ~np.isin(ids, np.asarray(never, dtype=np.int64))
    flat = elig.ravel()
    if word_start is None:
        lead_x0 = x0
    else:
        lead = np_leaders(ids, elig, word_start).ravel()
        lead_x0 = x0[np.where(lead >= 0, lead, 0)]
    sel = flat & (lead_x0 < np.uint64(t_select))
    span = np.uint64((rand_hi - rand_lo) & M32)
    rand = ((x2 * span) >> np.uint64(32)).astype(np.int64) + rand_lo
    rand = (rand + (1 << 31)) % ONE - (1 << 31)  # int32 arithmetic wraps
    src = ids.ravel().astype(np.int64)
    out = np.where(sel & (x1 < np.uint64(t_mask)), mask_id, np.where(sel & (x1 < np.uint64(t_mask + t_random)), rand, src))
    labels = np.where(sel, src, ignore_index)
    return out.astype(ids.dtype).reshape(ids.shape), labels.astype(ids.dtype).reshape(ids.shape)


def threshold(p):
    return min(ONE, int(round(p * ONE)))


# ------------------------------------------------------------------------------------------ Philox
# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key -> output
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    assert philox_scalar(ctr, key) == want
    assert tuple(int(v) for v in np_philox4x32_10(*ctr, *key)) == want


def test_philox_vectorised_equals_scalar():
    rng = np.random.default_rng(2024)
    ctr = rng.integers(0, ONE, size=(1000, 4), dtype=np.uint64)
    key = (int(rng.integers(0, ONE)), int(rng.integers(0, ONE)))
    got = np.stack(np_philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key), axis=1)
    for i in range(1000):
        assert tuple(int(v) for v in got[i]) == philox_scalar(tuple(int(v) for v in ctr[i]), key)


def test_draws_count_in_64_bits():
    """The element index carries into the counter's second word, and wraps at 2^64."""
    x = np_draws(8, 7, 9, ONE - 3)
    assert tuple(int(v[2]) for v in x) == philox_scalar((M32, 0, 9, 0), (7, 0))
    assert tuple(int(v[3]) for v in x) == philox_scalar((0, 1, 9, 0), (7, 0))
    x = np_draws(3, 7 + (5 << 32), 9 + (4 << 32), (1 << 64) - 1)
    assert tuple(int(v[0]) for v in x) == philox_scalar((M32, M32, 9, 4), (7, 5))
    assert tuple(int(v[1]) for v in x) == philox_scalar((0, 0, 9, 4), (7, 5))


# ------------------------------------------------------------------------------------------ np_mlm
BERT = dict(t_select=threshold(0.15), t_mask=threshold(0.8), t_random=threshold(0.1), mask_id=4, rand_lo=5, rand_hi=24000)


def test_mlm_by_hand():
    """Six elements worked through from their draws."""
    ids = np.array([[10, 11, 0, 12, 13, 14]], dtype=np.int32)
    attn = np.array([[1, 1, 1, 1, 1, 0]], dtype=np.uint8)
    x = [philox_scalar((e, 0, 3, 0), (1, 0)) for e in range(6)]
    kw = dict(seed=1, stream_id=3, t_select=ONE // 2, t_mask=ONE // 2, t_random=ONE // 4, mask_id=99, rand_lo=100, rand_hi=200,
              never=[0])
    out, labels = np_mlm(ids, attn, **kw)
    for c in range(6):
        sel = c not in (2, 5) and x[c][0] < ONE // 2
        assert labels[0, c] == (ids[0, c] if sel else -100)
        want = ids[0, c]
        if sel and x[c][1] < ONE // 2:
            want = 99
        elif sel and x[c][1] < ONE // 2 + ONE // 4:
            want = 100 + ((x[c][2] * 100) >> 32)
        assert out[0, c] == want
    # one word over columns 0-1, the never id ends it, the next begins at column 3
    ws = np.zeros(20, dtype=np.uint8)
    out, labels = np_mlm(ids, attn, word_start=ws, **kw)
    picked = [bool(labels[0, c] != -100) for c in range(6)]
    assert picked == [x[0][0] < ONE // 2] * 2 + [False] + [x[3][0] < ONE // 2] * 2 + [False]


def test_mlm_shares_are_binomial():
    """2^20 eligible elements at p = 0.15 with 0.8 / 0.1 / 0.1. Every count is a sum of independent
    Bernoulli draws (the thresholds differ from p by less than 2^-33, which moves a count by less than
    10^-3), so it lies within 5 standard deviations sqrt(n p (1 - p)) of n p but for a chance below
    10^-6: the selected among n = 2^20 at p = 0.15 (sd 366), then the masked / random / kept among the
    n_sel selected at p = 0.8 / 0.1 / 0.1 (sd about 159 / 119 / 119)."""
    n = 1 << 20
    ids = np.arange(n, dtype=np.int32).reshape(1024, 1024) % 20000 + 30000  # no id is mask_id or in the random range
    out, labels = np_mlm(ids, None, seed=12345, stream_id=1, **BERT)
    sel = labels != -100
    n_sel = int(sel.sum())
    assert abs(n_sel - n * 0.15) <= 5 * math.sqrt(n * 0.15 * 0.85)
    assert np.array_equal(labels[sel], ids[sel]) and np.array_equal(out[~sel], ids[~sel])
    masked = int((out[sel] == 4).sum())
    kept = int((out[sel] == ids[sel]).sum())
    rand = n_sel - masked - kept
    assert ((out[sel] == 4) | (out[sel] == ids[sel]) | ((out[sel] >= 5) & (out[sel] < 24000))).all()
    for count, p in ((masked, 0.8), (rand, 0.1), (kept, 0.1)):
        assert abs(count - n_sel * p) <= 5 * math.sqrt(n_sel * p * (1 - p)), (count, p)
    # the random ids spread over the range: their mean lies within 5 sd of the middle (uniform: sd = span / sqrt(12))
    r = out[sel & (out != 4) & (out != ids)]
    assert abs(r.mean() - (5 + 23999) / 2) <= 5 * (23995 / math.sqrt(12)) / math.sqrt(len(r))
    # another stream draws another selection; the same arguments the same one
    out2, labels2 = np_mlm(ids, None, seed=12345, stream_id=2, **BERT)
    both = int(((labels2 != -100) & sel).sum())
    assert abs(both - n * 0.15 * 0.15) <= 5 * math.sqrt(n * 0.0225 * 0.9775)  # independent: p^2
    out3, labels3 = np_mlm(ids, None, seed=12345, stream_id=1, **BERT)
    assert np.array_equal(out3, out) and np.array_equal(labels3, labels)


def test_mlm_parts_equal_the_whole():
    """elem_base continues a batch: rows 40.. masked on their own equal the whole batch's rows 40.."""
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 500, size=(100, 37), dtype=np.int64)
    attn = (rng.random((100, 37)) < 0.8).astype(np.uint8)
    ws = (rng.random(450) < 0.4).astype(np.uint8)
    kw = dict(seed=3, stream_id=4, elem_base=ONE - 1000, never=[1, 2], word_start=ws, **BERT)
    out, labels = np_mlm(ids, attn, **kw)
    kw["elem_base"] += 40 * 37
    out2, labels2 = np_mlm(ids[40:], attn[40:], **kw)
    assert np.array_equal(out[40:], out2) and np.array_equal(labels[40:], labels2)
    assert out.dtype == np.int64 and labels.dtype == np.int64


def test_mlm_words_are_selected_whole():
    rng = np.random.default_rng(6)
    n_vocab = 300
    ids = rng.integers(0, 320, size=(200, 50)).astype(np.int32)  # ids from 300 on lie outside the vocabulary: word starts
    attn = (np.arange(50)[None, :] < rng.integers(0, 51, size=200)[:, None]).astype(np.uint8)
    ws = (rng.random(n_vocab) < 0.3).astype(np.uint8)
    never = [7, 8, 9]
    out, labels = np_mlm(ids, attn, seed=9, t_select=ONE // 3, t_mask=ONE, t_random=0, mask_id=-5, never=never, word_start=ws)
    sel = labels != -100
    words = multi = picked = 0
    for r in range(200):
        c = 0
        while c < 50:
            if not attn[r, c] or ids[r, c] in never:
                assert not sel[r, c]
                c += 1
                continue
            e = c + 1  # the word [c, e): up to the next word start, ineligible element or row end
            while e < 50 and attn[r, e] and ids[r, e] not in never and ids[r, e] < n_vocab and not ws[ids[r, e]]:
                e += 1
            assert sel[r, c:e].all() or not sel[r, c:e].any(), (r, c, e)
            words += 1
            multi += e - c > 1
            picked += bool(sel[r, c])
            c = e
    assert words > 1000 and multi > 300
    # one draw per word (its leader's), p = 1/3: the selected words lie within 5 binomial sd of words / 3
    assert abs(picked - words / 3) <= 5 * math.sqrt(words * (1 / 3) * (2 / 3))
    assert (out[sel] == -5).all() and np.array_equal(out[~sel], ids[~sel])


def test_thresholds():
    assert threshold(0.0) == 0 and threshold(1.0) == ONE and threshold(0.15) == 644245094 and threshold(0.5) == ONE // 2


# ------------------------------------------------------------------------------------------ C-ABI, host side
DENSE_I64 = 4


@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    return _lib.lib()


def _is_arg_error(L, rc):
    from akshar_amd import _lib
    return rc == _lib.AK_ERR_ARG and len(L.ak_last_error()) > 0


def test_mlm_argument_errors_cpu(L):
    """Every ak_ids_mlm error of the header, raised on the host before any device call (the pointers
    here are host memory: nothing may touch them)."""
    src, out, lab = (C.c_int32 * 64)(), (C.c_int32 * 64)(*([77] * 64)), (C.c_int32 * 64)(*([77] * 64))
    nev = (C.c_int32 * 9)(*range(9))
    ws = (C.c_uint8 * 16)()

    def mlm(src=src, rows=8, width=8, t_select=ONE // 4, t_mask=ONE // 2, t_random=ONE // 4, rand_lo=0, rand_hi=10, never=nev,
            n_never=2, word_start=None, n_vocab=0, flags=0, out=out, lab=lab, cap=8):
        return L.ak_ids_mlm(src, None, rows, width, 1, 2, 3, t_select, t_mask, t_random, 4, rand_lo, rand_hi, -100, never,
                            n_never, word_start, n_vocab, flags, out, lab, cap, None)

    assert _is_arg_error(L, mlm(src=None))
    assert _is_arg_error(L, mlm(out=None))
    assert _is_arg_error(L, mlm(lab=None))
    assert _is_arg_error(L, mlm(width=0))
    assert _is_arg_error(L, mlm(width=0, rows=0))
    assert _is_arg_error(L, mlm(t_select=ONE + 1))
    assert _is_arg_error(L, mlm(t_mask=ONE + 1, t_random=0))
    assert _is_arg_error(L, mlm(t_mask=0, t_random=ONE + 1))
    assert _is_arg_error(L, mlm(t_mask=ONE, t_random=1))
    assert _is_arg_error(L, mlm(t_mask=1 << 63, t_random=1 << 63))  # the sum does not wrap
    assert _is_arg_error(L, mlm(rand_lo=10, rand_hi=10))
    assert _is_arg_error(L, mlm(rand_lo=10, rand_hi=-10))
    assert _is_arg_error(L, mlm(n_never=9))
    assert _is_arg_error(L, mlm(never=None, n_never=1))
    assert _is_arg_error(L, mlm(word_start=ws, n_vocab=0))
    assert _is_arg_error(L, mlm(flags=1))
    assert _is_arg_error(L, mlm(flags=DENSE_I64 | 8))
    assert _is_arg_error(L, mlm(flags=-1))
    assert _is_arg_error(L, mlm(out=src))
    assert _is_arg_error(L, mlm(lab=src))
    assert _is_arg_error(L, mlm(lab=out))
    assert list(out) == [77] * 64 and list(lab) == [77] * 64


def test_mlm_empty_calls_are_ok_without_a_device(L):
    """rows == 0 and cap_rows == 0 store nothing and launch nothing: AK_OK on a machine without a GPU;
    so is rand_hi <= rand_lo while t_random is 0, and NULL never with n_never 0."""
    src, out, lab = (C.c_int32 * 64)(), (C.c_int32 * 64)(*([77] * 64)), (C.c_int32 * 64)(*([77] * 64))
    ws = (C.c_uint8 * 16)()
    assert L.ak_ids_mlm(None, None, 0, 8, 1, 2, 3, ONE, ONE, 0, 4, 0, 0, -100, None, 0, None, 0, 0, None, None, 8, None) == 0
    assert L.ak_ids_mlm(src, None, 8, 8, 1, 2, 3, ONE, ONE, 0, 4, 0, 0, -100, None, 0, ws, 16, DENSE_I64, out, lab, 0, None) == 0
    assert list(out) == [77] * 64 and list(lab) == [77] * 64


def test_header_documents_the_known_answer():
    src = open(os.path.join(ROOT, "include", "akshar.h")).read()
    assert "6627e8d5 e169c58d bc57ac4c 9b00dbd8" in src and "0xD2511F53" in src and "0xBB67AE85" in src


# ------------------------------------------------------------------------------------------ Python layer
def test_mask_ids_value_errors_cpu():
    """engine.mask_ids checks its numbers before it looks at a tensor or a device."""
    import torch
    from akshar_amd import engine
    ids = torch.zeros((2, 4), dtype=torch.int32)
    ok = dict(mask_id=4, vocab_range=(0, 100))
    for bad in (dict(mask_fraction=0.8, random_fraction=0.3), dict(mlm_probability=1.5), dict(mlm_probability=-0.1),
                dict(mask_fraction=2.0, random_fraction=0.0), dict(random_fraction=-1.0), dict(never=list(range(9))),
                dict(vocab_range=(5, 5)), dict(mask_id=1 << 31), dict(ignore_index=-(1 << 31) - 1), dict(never=[1, 1 << 32]), dict(vocab_range=(0, 1 << 40)), dict(seed=-1), dict(stream_id=1 << 64)):
        with pytest.raises(ValueError):
            engine.mask_ids(ids, **{**ok, **bad})
    with pytest.raises(TypeError):  # the values pass: the host tensor is what is wrong
        engine.mask_ids(ids, **ok)
    assert engine._threshold("p", 0.15) == threshold(0.15) and engine._threshold("p", 1.0) == ONE


def test_models_know_their_mask_token(bpe_model, spm_model):
    assert bpe_model.mask_id == 4 and bpe_model.unk_token_id == 1
    assert spm_model.mask_id == spm_model.piece_to_id[b"<mask>"] == 3 and spm_model.bos_id == 1
