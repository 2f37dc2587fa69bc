"""Masked-LM batches on the device (include/akshar.h ak_ids_mlm, akshar_amd/csrc/ak_k_mlm.hip), element
for element against np_mlm of tests/test_mlm_ref.py (which that file pins to Random123's known answers
for Philox4x32-10).

Every raw call writes into outputs allocated for all rows plus a guard band of BUFFER_GUARD sentinel
elements: what lies at or past the capacity, the slack between a short capacity and the full size
included, must come back untouched.
"""
import numpy as np
import pytest
import torch

from tests.conftest import BPE_PATH, SPM_PATH
from tests.test_dense_ref import load_dense_golden
from tests.test_gpu_buffers import S32, S64
from tests.test_mlm_ref import BERT, ONE, np_mlm, threshold
from tests.util import BUFFER_GUARD as G

pytestmark = pytest.mark.gpu

DENSE_I64 = 4
N_VOCAB = 900
NEVER8 = [0, 1, 2, 3, 4, 5, 6, 7]
WIDTHS = (1, 3, 4, 5, 255, 256, 257)


@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


@pytest.fixture(scope="module")
def word_start():
    host = (np.random.default_rng(1).random(N_VOCAB) < 0.3).astype(np.uint8)
    host[NEVER8] = 0
    return host, torch.from_numpy(host).cuda()


def make_batch(rows, width, seed, dtype=np.int32):
    """ids in [0, 1000) (those from N_VOCAB on lie outside the vocabulary), one in 12 an id of NEVER8;
    a right-padded attention mask with rows that are all padding and a few holes inside rows."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(8, 1000, size=(rows, width))
    ids = np.where(rng.random((rows, width)) < 1 / 12, rng.integers(0, 8, size=(rows, width)), ids).astype(dtype)
    lens = rng.integers(0, width + 1, size=rows)
    lens[rng.random(rows) < 0.1] = 0
    lens[rng.random(rows) < 0.3] = width
    attn = (np.arange(width)[None, :] < lens[:, None]) & (rng.random((rows, width)) > 0.02)
    return ids, attn.astype(np.uint8)


def run_mlm(L, ids, attn, *, cap=None, lead=0, never=(), word_start=None, seed=0, stream_id=0, elem_base=0, t_select, t_mask,
            t_random, mask_id, rand_lo=0, rand_hi=1, ignore_index=-100):
    """ak_ids_mlm through the raw C-ABI; inputs and guarded outputs lie `lead` elements into their
    allocations (lead 1: no array is 16-byte aligned, the mask not even 4-byte). Returns the rows below
    the capacity as (out, labels), after the guard checks."""
    import ctypes
    rows, width = ids.shape
    cap = rows if cap is None else cap
    i64 = ids.dtype == np.int64
    tdt, sent = (torch.int64, S64) if i64 else (torch.int32, S32)
    n = rows * width
    src = torch.full((lead + n + 8,), -99, dtype=tdt, device="cuda")[lead:]
    src[:n] = torch.from_numpy(ids.ravel()).cuda()
    gm = None
    if attn is not None:
        gm = torch.full((lead + n + 8,), 1, dtype=torch.uint8, device="cuda")[lead:]
        gm[:n] = torch.from_numpy(attn.ravel()).cuda()
    out = torch.full((lead + n + G,), sent, dtype=tdt, device="cuda")[lead:]
    lab = torch.full((lead + n + G,), sent, dtype=tdt, device="cuda")[lead:]
    nev = (ctypes.c_int32 * 8)(*never) if never else None
    rc = L.ak_ids_mlm(src.data_ptr(), gm.data_ptr() if gm is not None else None, rows, width, seed, stream_id, elem_base,
                      t_select, t_mask, t_random, mask_id, rand_lo, rand_hi, ignore_index, nev, len(never),
                      word_start.data_ptr() if word_start is not None else None, N_VOCAB if word_start is not None else 0,
                      DENSE_I64 if i64 else 0, out.data_ptr(), lab.data_ptr(), cap, None)
    assert rc == 0, L.ak_last_error()
    torch.cuda.synchronize()
    k = min(rows, cap)
    res = []
    for t in (out, lab):
        h = t.cpu().numpy()
        assert (h[k * width:] == sent).all(), "stored at or past the capacity"
        res.append(h[:k * width].reshape(k, width))
    assert np.array_equal(src[:n].cpu().numpy(), ids.ravel())  # the input is read only
    return res


def check(got, ref, k=None):
    for g, r in zip(got, ref):
        r = r if k is None else r[:k]
        assert g.dtype == r.dtype and g.shape == r.shape
        bad = np.argwhere(g != r)
        assert len(bad) == 0, (len(bad), bad[:4].tolist())


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("width", WIDTHS)
def test_mlm_shapes(L, word_start, width):
    """1 row, 2 rows and about 70 k elements (some 70 blocks, every wave a span of one chunk) x int32 /
    int64 x aligned / at element offset 1 x with and without word_start, the attention mask and the
    never list left out in turn, the element index crossing 2^32 and 2^64 inside the batch."""
    ws_host, ws_dev = word_start
    case, seen = 0, set()
    for rows in (1, 2, -(-70000 // width)):
        for variant in range(8):
            dtype, lead, use_ws = (np.int32, np.int64)[variant & 1], variant >> 1 & 1, bool(variant >> 2 & 1)
            use_attn, use_never = variant not in (1, 6), variant not in (2, 5)
            ids, attn = make_batch(rows, width, seed=100 + case, dtype=dtype)
            kw = dict(seed=0xDEADBEEF12345678 + case, stream_id=(7 << 32) + case, elem_base=(0, ONE - 5, (1 << 64) - 300)[case % 3],
                      never=NEVER8 if use_never else [], t_select=ONE // 3, t_mask=ONE // 2, t_random=ONE // 4, mask_id=-3,
                      rand_lo=1000, rand_hi=1000000, ignore_index=-100 - case)
            ref = np_mlm(ids, attn if use_attn else None, word_start=ws_host if use_ws else None, **kw)
            got = run_mlm(L, ids, attn if use_attn else None, lead=lead, word_start=ws_dev if use_ws else None, **kw)
            check(got, ref)
            if rows > 2:
                assert (ref[1] != kw["ignore_index"]).any() and (ref[0] == -3).any()
                seen.add((dtype, lead, use_ws))
            case += 1
    assert len(seen) == 8 and {d for d, _, _ in seen} == {np.int32, np.int64}


@pytest.fixture(scope="module")
def span_elems():
    """More elements than the launch's largest grid has chunks for at one per wave (8 blocks per CU, 4
    waves of 256 elements each), so every wave's span is 2 chunks or more and the kernel's chunk loop
    carries its column from one to the next."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(2_500_000, cus * 8 * 1024 * 6 // 5)


@pytest.mark.parametrize("width", [257, 100])
def test_mlm_spans_of_several_chunks(L, word_start, span_elems, width):
    """Whole-word masking over spans of 2+ chunks per wave, int32 aligned and int64 at element offset 1:
    the column a wave carries from chunk to chunk decides where a walk stops at a row's start."""
    ws_host, ws_dev = word_start
    rows = -(-span_elems // width)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert rows * width > cus * 8 * 1024 and 256 % width != 0
    ids, attn = make_batch(rows, width, seed=width)
    kw = dict(seed=21, stream_id=22, elem_base=ONE - 1000, never=NEVER8, t_select=ONE // 3, t_mask=ONE // 2, t_random=ONE // 4,
              mask_id=-3, rand_lo=1000, rand_hi=1000000)
    ref = np_mlm(ids, attn, word_start=ws_host, **kw)  # once: the int64 batch holds the same values
    check(run_mlm(L, ids, attn, lead=0, word_start=ws_dev, **kw), ref)
    check(run_mlm(L, ids.astype(np.int64), attn, lead=1, word_start=ws_dev, **kw), [r.astype(np.int64) for r in ref])


@pytest.mark.parametrize("width,rows,cap", [(3, 200, 85), (5, 103, 51), (257, 9, 3), (256, 5, 2), (1, 700, 255), (4, 100, 0),
                                            (4, 100, 120)])
def test_mlm_short_capacities(L, word_start, width, rows, cap):
    """cap_rows x width = 255 or 771 elements: the last chunk and the last lane's group of 4 straddle the
    capacity; 512: it ends with a chunk; 0 and more than the rows. Nothing is stored at or past it."""
    ws_host, ws_dev = word_start
    for dtype, lead in ((np.int32, 0), (np.int64, 0), (np.int32, 1), (np.int64, 1)):
        ids, attn = make_batch(rows, width, seed=cap + lead, dtype=dtype)
        kw = dict(seed=5, stream_id=6, elem_base=ONE - 100, never=NEVER8, **BERT)
        kw["t_select"] = ONE // 2
        ref = np_mlm(ids, attn, word_start=ws_host, **kw)
        check(run_mlm(L, ids, attn, cap=cap, lead=lead, word_start=ws_dev, **kw), ref, min(rows, cap))


def test_mlm_no_rows(L):
    ids = np.zeros((0, 8), dtype=np.int32)
    out, lab = run_mlm(L, ids, None, **BERT)
    assert out.shape == lab.shape == (0, 8)


# ------------------------------------------------------------------------------------------ thresholds
def test_mlm_thresholds(L):
    ids, attn = make_batch(300, 37, seed=3)
    elig = (attn != 0) & ~np.isin(ids, NEVER8)
    base = dict(never=NEVER8, seed=1, stream_id=2, mask_id=4, rand_lo=2000, rand_hi=2010)
    # every eligible element carries a label; 0.8 / 0.1 / 0.1 of them
    kw = dict(base, t_select=ONE, t_mask=threshold(0.8), t_random=threshold(0.1))
    out, lab = run_mlm(L, ids, attn, **kw)
    check((out, lab), np_mlm(ids, attn, **kw))
    assert np.array_equal(lab != -100, elig) and np.array_equal(lab[elig], ids[elig])
    # nothing selected: out == in, no label
    kw = dict(base, t_select=0, t_mask=ONE, t_random=0)
    out, lab = run_mlm(L, ids, attn, **kw)
    assert np.array_equal(out, ids) and (lab == -100).all()
    # all <mask>; all random, inside [rand_lo, rand_hi) and hitting both ends of it
    kw = dict(base, t_select=ONE, t_mask=ONE, t_random=0)
    out, lab = run_mlm(L, ids, attn, **kw)
    assert (out[elig] == 4).all() and np.array_equal(out[~elig], ids[~elig])
    kw = dict(base, t_select=ONE, t_mask=0, t_random=ONE)
    out, lab = run_mlm(L, ids, attn, **kw)
    check((out, lab), np_mlm(ids, attn, **kw))
    assert set(np.unique(out[elig]).tolist()) == set(range(2000, 2010)) and np.array_equal(out[~elig], ids[~elig])
    # a negative range, and the widest one
    for lo, hi in ((-50, -40), (-(1 << 31), (1 << 31) - 1)):
        kw = dict(base, t_select=ONE, t_mask=0, t_random=ONE, rand_lo=lo, rand_hi=hi)
        out, lab = run_mlm(L, ids, attn, **kw)
        check((out, lab), np_mlm(ids, attn, **kw))
        assert (out[elig] >= lo).all() and (out[elig] < hi).all()


# ------------------------------------------------------------------------------------------ whole words
@pytest.mark.parametrize("dtype,lead", [(np.int32, 0), (np.int64, 1)])
def test_mlm_whole_word_rows(L, dtype, lead):
    """Rows 257 wide, so words cross the lanes' groups of 4 and the 256-element chunks at every offset."""
    W = 257
    flag = np.zeros(N_VOCAB, dtype=np.uint8)
    flag[500:] = 1  # ids 10..499 continue a word, 500..899 begin one
    ids = np.full((6, W), 20, dtype=dtype)
    attn = np.ones((6, W), dtype=np.uint8)
    # row 0: no flagged id at all: one word led by column 0
    ids[1, ::2] = 600                       # row 1: alternating flags
    ids[2, [0, 250, 255]] = 700             # row 2: words over columns 0-249 (past element 512 = row 1's end + 255), 250-254, 255-256
    ids[3, 100] = 3                         # row 3: a never id inside a word ...
    attn[3, 200] = 0                        # ... and a masked-out position inside the next
    ids[4, [10, 11, 40]] = (N_VOCAB, -1, 10 ** 6)  # row 4: ids outside the vocabulary begin words
    attn[5, :] = 0                          # row 5: all padding
    kw = dict(never=NEVER8, seed=77, stream_id=3, elem_base=ONE - 300, t_select=ONE // 2, t_mask=ONE, t_random=0, mask_id=4)
    ws = torch.from_numpy(flag).cuda()
    for s in range(4):  # four draws: most words are seen both selected and not
        kw["stream_id"] = s
        ref = np_mlm(ids, attn, word_start=flag, **kw)
        out, lab = got = run_mlm(L, ids, attn, lead=lead, word_start=ws, **kw)
        check(got, ref)
        sel = lab != -100
        assert sel[0].all() or not sel[0].any()
        assert all(sel[1, c] == sel[1, c + 1] for c in range(0, W - 1, 2))
        for a, b in ((0, 250), (250, 255), (255, 257)):
            assert sel[2, a:b].all() or not sel[2, a:b].any()
        for a, b in ((0, 100), (101, 200), (201, 257)):
            assert sel[3, a:b].all() or not sel[3, a:b].any()
        assert not sel[3, 100] and not sel[3, 200] and not sel[5].any()
        for a, b in ((0, 10), (10, 11), (11, 40), (40, 257)):
            assert sel[4, a:b].all() or not sel[4, a:b].any()


# ------------------------------------------------------------------------------------------ Python layer
@pytest.fixture(scope="module")
def toks():
    from akshar_amd.tokenizer import aksharTokenizer
    return {"bpe": aksharTokenizer(BPE_PATH, "bpe"), "spm": aksharTokenizer(SPM_PATH, "sentencepiece")}


@pytest.fixture(scope="module")
def texts():
    return [r["text"] for r in load_dense_golden()["rows"][:48] if len(r["ids"]) < 200]


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize("name", ["bpe", "spm"])
def test_encode_mlm(toks, texts, name):
    from akshar_amd import engine
    tok = toks[name]
    m = tok.model.model
    pad = None if name == "bpe" else 5
    assert len(texts) >= 30
    plain = _host(tok.encode_padded(texts, 24, pad_id=pad))
    got = _host(tok.encode_mlm(texts, 24, mlm_probability=0.5, seed=11, stream_id=2, pad_id=pad))
    assert set(got) == {"input_ids", "attention_mask", "labels", "lengths"}
    assert np.array_equal(got["attention_mask"], plain["attention_mask"]) and np.array_equal(got["lengths"], plain["lengths"])
    lab, ids = got["labels"], got["input_ids"]
    sel = lab != -100
    assert sel.any() and (ids[sel] == m.mask_id).any()
    assert np.array_equal(lab[sel], plain["input_ids"][sel]) and np.array_equal(ids[~sel], plain["input_ids"][~sel])
    special = [0, 1, 2, 3, 4] if name == "bpe" else [5, 0, 1, 2, 3]  # pad unk bos eos mask
    assert not sel[~plain["attention_mask"]].any() and not np.isin(plain["input_ids"][sel], special).any()
    if name == "bpe":
        assert (plain["input_ids"][:, 0] == m.bos).all() and not sel[:, 0].any()
    # the kernel's definition, from the padded batch
    ref = np_mlm(plain["input_ids"], plain["attention_mask"], seed=11, stream_id=2, t_select=ONE // 2, t_mask=threshold(0.8),
                 t_random=threshold(0.1), mask_id=m.mask_id, rand_lo=0, rand_hi=m.vocab_size, never=special)
    check((ids, lab), ref)
    # reproducible, another stream differs, the (buf, offs) form is the list form
    again = _host(tok.encode_mlm(engine.pack(texts), 24, mlm_probability=0.5, seed=11, stream_id=2, pad_id=pad))
    assert all(np.array_equal(again[k], got[k]) for k in got)
    other = _host(tok.encode_mlm(texts, 24, mlm_probability=0.5, seed=11, stream_id=3, pad_id=pad))
    assert not np.array_equal(other["labels"], lab)
    # int64 matrices through engine.mask_ids
    dev = torch.from_numpy(plain["input_ids"]).cuda().long()
    o64, l64 = engine.mask_ids(dev, torch.from_numpy(plain["attention_mask"]).cuda(), mask_id=m.mask_id,
                               vocab_range=(0, m.vocab_size), never=special, mlm_probability=0.5, seed=11, stream_id=2)
    assert o64.dtype == torch.int64 and np.array_equal(o64.cpu().numpy(), ids) and np.array_equal(l64.cpu().numpy(), lab)


def test_encode_mlm_whole_word(toks, texts):
    tok = toks["spm"]
    m = tok.model.model
    plain = _host(tok.encode_padded(texts, 32, pad_id=5))
    got = _host(tok.encode_mlm(texts, 32, mlm_probability=0.4, seed=3, whole_word=True, pad_id=5))
    flag = np.array([p.startswith("▁".encode()) for p in m.pieces], dtype=np.uint8)
    assert 0 < flag.sum() < len(flag)
    ref = np_mlm(plain["input_ids"], plain["attention_mask"], seed=3, t_select=threshold(0.4), t_mask=threshold(0.8),
                 t_random=threshold(0.1), mask_id=3, rand_lo=0, rand_hi=m.vocab_size, never=[5, 0, 1, 2, 3], word_start=flag)
    check((got["input_ids"], got["labels"]), ref)
    sel, ids = got["labels"] != -100, plain["input_ids"]
    cont = plain["attention_mask"][:, 1:] & plain["attention_mask"][:, :-1] & (flag[ids[:, 1:]] == 0) \
        & ~np.isin(ids[:, 1:], [5, 0, 1, 2, 3]) & ~np.isin(ids[:, :-1], [5, 0, 1, 2, 3])
    assert cont.sum() > 20 and np.array_equal(sel[:, 1:][cont], sel[:, :-1][cont])  # a piece inside a word goes with the one before
    assert tok._word_start(torch.device("cuda", torch.cuda.current_device())) is tok._word_start(
        torch.device("cuda", torch.cuda.current_device()))


def test_encode_mlm_errors(toks):
    from akshar_amd.tokenizer import aksharTokenizer
    with pytest.raises(ValueError, match="need model for IDs"):
        aksharTokenizer().encode_mlm(["a"], 4)
    with pytest.raises(ValueError, match="whole_word"):
        toks["bpe"].encode_mlm(["a"], 4, whole_word=True)
    with pytest.raises(ValueError, match="pad"):
        toks["spm"].encode_mlm(["a"], 4)
    with pytest.raises(ValueError):
        toks["bpe"].encode_mlm(["a"], 4, mask_fraction=0.9, random_fraction=0.2)
    m = toks["bpe"].model.model
    keep, m.mask_id = m.mask_id, None
    try:
        with pytest.raises(ValueError, match="the model has no <mask> token: pass mask_id"):
            toks["bpe"].encode_mlm(["a"], 4)
        got = toks["bpe"].encode_mlm(["a b c"], 8, mask_id=4, mlm_probability=1.0, mask_fraction=1.0, random_fraction=0.0)
        assert (got["input_ids"][got["labels"] != -100] == 4).all()
    finally:
        m.mask_id = keep
