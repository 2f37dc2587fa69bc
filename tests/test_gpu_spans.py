"""Span-corruption batches on the device (include/akshar.h ak_ids_spans, akshar_amd/csrc/ak_k_spans.hip),
element for element against np_spans of tests/test_spans_ref.py.

Every raw call writes into outputs allocated for all rows plus a guard band of BUFFER_GUARD sentinel
elements, every array `lead` = 1 element into its allocation so that nothing is aligned: what lies at
or past the capacity must come back untouched, and the input unchanged.
"""
import numpy as np
import pytest
import torch

from tests.conftest import BPE_PATH, SPM_PATH
from tests.test_dense_ref import load_dense_golden
from tests.test_gpu_buffers import S32, S64
from tests.test_mlm_ref import ONE, threshold
from tests.test_spans_ref import MAX_WIDTH, mean_q16, np_spans, span_counts
from tests.util import BUFFER_GUARD as G

pytestmark = pytest.mark.gpu

DENSE_I64 = 4
WIDTHS = (2, 3, 4, 63, 64, 65, 127, 128, 129, 257)
KEYS = ("inputs", "targets", "in_lengths", "tgt_lengths", "noise")
# (density, mean): T5's; every boundary a cut (S = min(N, M)); N = S = 1; one long span (S = 1, no cuts)
RATES = ((0.15, 3.0), (0.5, 1.0), (1e-9, 3.0), (0.3, 1000.0))


@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


def make_ids(rows, width, seed, dtype=np.int32):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 30000, size=(rows, width)).astype(dtype)
    if dtype == np.int64:  # ids beyond int32, on both sides
        far = rng.random((rows, width))
        ids = np.where(far < 0.2, ids + (1 << 40), np.where(far > 0.9, -ids - (1 << 35), ids))
    return ids


def make_lengths(rows, width, seed):
    lens = np.random.default_rng(seed).integers(0, width + 1, size=rows).astype(np.int32)
    lens[:7] = (0, 1, 2, width, width + 5, -3, width - 1)  # beyond the width and negative: clamped
    return lens


def guarded(n, dtype, sent, lead):
    return torch.full((lead + n + G,), sent, dtype=dtype, device="cuda")[lead:]


def run_spans(L, ids, lengths=None, *, cap=None, lead=1, in_width=None, tgt_width=None, skip=(), seed=0, stream_id=0,
              elem_base=0, density_q32, mq16, sentinel_first, sentinel_step=-1, eos_id=-1, pad_id=0, tgt_pad_id=-100,
              expect_rc=0):
    """ak_ids_spans through the raw C-ABI; returns np_spans' dict for the rows below the capacity (the
    outputs named in `skip` passed as NULL and left out), after the guard checks."""
    rows, width = ids.shape
    cap = rows if cap is None else cap
    i64 = ids.dtype == np.int64
    tdt, sent = (torch.int64, S64) if i64 else (torch.int32, S32)
    full = span_counts(width, density_q32, mq16, eos_id >= 0)
    in_width = full[2] if in_width is None else in_width
    tgt_width = full[3] if tgt_width is None else tgt_width
    n = rows * width
    src = torch.full((lead + n + 8,), -99, dtype=tdt, device="cuda")[lead:]
    src[:n] = torch.from_numpy(ids.ravel()).cuda()
    gl = None
    if lengths is not None:
        gl = torch.full((lead + rows + 8,), 1, dtype=torch.int32, device="cuda")[lead:]
        gl[:rows] = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).cuda()
    outs = {"inputs": (guarded(rows * in_width, tdt, sent, lead), in_width, sent),
            "targets": (guarded(rows * tgt_width, tdt, sent, lead), tgt_width, sent),
            "in_lengths": (guarded(rows, torch.int32, S32, lead), 1, S32),
            "tgt_lengths": (guarded(rows, torch.int32, S32, lead), 1, S32),
            "noise": (guarded(n, torch.uint8, 0xEE, lead), width, 0xEE)}
    ptr = {k: (None if k in skip else t.data_ptr()) for k, (t, _, _) in outs.items()}
    rc = L.ak_ids_spans(src.data_ptr(), gl.data_ptr() if gl is not None else None, rows, width, seed, stream_id, elem_base,
                        density_q32, mq16, sentinel_first, sentinel_step, eos_id, pad_id, tgt_pad_id, DENSE_I64 if i64 else 0,
                        ptr["inputs"], in_width, ptr["targets"], tgt_width, ptr["in_lengths"], ptr["tgt_lengths"], ptr["noise"],
                        cap, None)
    assert rc == expect_rc, L.ak_last_error()
    torch.cuda.synchronize()
    k = min(rows, cap) if rc == 0 else 0
    res = {}
    for key, (t, w, s) in outs.items():
        h = t.cpu().numpy()
        kept = 0 if key in skip else k * w
        assert (h[kept:] == s).all(), "%s: stored at or past the capacity" % key
        if key not in skip:
            res[key] = h[:kept] if key.endswith("lengths") else h[:kept].reshape(k, w)
    assert np.array_equal(src[:n].cpu().numpy(), ids.ravel())  # the input is read only
    return res


def check(got, ref, k=None):
    for key, g in got.items():
        r = ref[key] if k is None else ref[key][:k]
        assert g.dtype == r.dtype and g.shape == r.shape, key
        bad = np.argwhere(g != r)
        assert len(bad) == 0, (key, len(bad), bad[:4].tolist())


def both(L, ids, lengths=None, **kw):
    raw = {k: v for k, v in kw.items() if k not in ("cap", "lead", "skip")}
    ref = np_spans(ids, lengths, **raw)
    got = run_spans(L, ids, lengths, **kw)
    check(got, ref, kw.get("cap"))
    return got, ref


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("width", WIDTHS)
def test_spans_shapes(L, width):
    """37 rows (one wave each) x the four rate settings x int32 / int64, with lengths (0, 1, 2, the width,
    clamped and random ones) or without, eos on and off and the three sentinel steps taking turns."""
    case = 0
    for density, mean in RATES:
        for dtype in (np.int32, np.int64):
            ids = make_ids(37, width, seed=width * 10 + case, dtype=dtype)
            lengths = make_lengths(37, width, seed=case) if case % 2 == 0 else None
            kw = dict(seed=0xDEADBEEF12345678 + case, stream_id=(7 << 32) + case, elem_base=(0, ONE - 5, (1 << 64) - 300)[case % 3],
                      density_q32=threshold(density), mq16=mean_q16(mean), sentinel_first=(31999, -7, (1 << 31) - 2)[case % 3],
                      sentinel_step=(-1, 0, 1)[case % 3], eos_id=1 if case % 4 < 2 else -1, pad_id=-5 - case, tgt_pad_id=-100 - case)
            got, ref = both(L, ids, lengths, **kw)
            full = span_counts(width, kw["density_q32"], kw["mq16"], kw["eos_id"] >= 0)
            if lengths is None:
                assert (got["in_lengths"] == full[2]).all() and (got["tgt_lengths"] == full[3]).all()
            if (density, mean) == (0.5, 1.0) and width >= 4:
                assert full[1] == width // 2  # every boundary of the shorter segmentation is a cut
            if density < 1e-6 or mean > 100:
                assert full[1] == 1
            case += 1


@pytest.mark.parametrize("width", [MAX_WIDTH, MAX_WIDTH - 1])
def test_spans_widest_rows(L, width):
    """One row at the widest the call takes: 64 chunks of keys, and at 0.5 / 1.0 cut lists of 2048 entries."""
    for case, (density, mean) in enumerate(((0.15, 3.0), (0.5, 1.0))):
        dtype = (np.int32, np.int64)[case]
        ids = make_ids(1, width, seed=width + case, dtype=dtype)
        both(L, ids, None, seed=3 + case, stream_id=9, elem_base=ONE - 100, density_q32=threshold(density), mq16=mean_q16(mean),
             sentinel_first=40000, sentinel_step=-1, eos_id=1, pad_id=0)
    two = make_ids(2, width, seed=5)
    both(L, two, np.array([width - 1, 7], dtype=np.int32), seed=1, density_q32=threshold(0.15), mq16=mean_q16(3.0),
         sentinel_first=40000, eos_id=1)


def test_spans_more_rows_than_waves(L):
    """More rows than the launch has waves (32 per CU), so waves take a second row and reuse their
    LDS; rows of differing lengths, so a row's keys and lists are shorter or longer than the last one's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows, width = cus * 32 + 77, 9
    ids = make_ids(rows, width, seed=61)
    lengths = make_lengths(rows, width, seed=62)
    both(L, ids, lengths, seed=4, stream_id=5, elem_base=ONE - 1000, density_q32=threshold(0.4), mq16=mean_q16(1.5),
         sentinel_first=31999, eos_id=1, pad_id=0)


def test_spans_too_wide_is_an_argument_error(L):
    from akshar_amd import _lib
    ids = make_ids(1, MAX_WIDTH + 1, seed=1)
    run_spans(L, ids, None, density_q32=threshold(0.15), mq16=mean_q16(3.0), sentinel_first=40000, expect_rc=_lib.AK_ERR_ARG)


# ------------------------------------------------------------------------------------------ widths, capacities
@pytest.mark.parametrize("eos_id", [1, -1])
def test_spans_output_widths(L, eos_id):
    """in_width / tgt_width exact, larger (padding), short by 1 and by half: the lengths still report what
    a row needs, and an element whose column lies outside is dropped, not moved."""
    width, rows = 129, 37
    ids = make_ids(rows, width, seed=11)
    lengths = make_lengths(rows, width, seed=12)
    kw = dict(seed=5, stream_id=6, density_q32=threshold(0.3), mq16=mean_q16(2.0), sentinel_first=31999, eos_id=eos_id, pad_id=0)
    _, _, in_len, tgt_len = span_counts(width, kw["density_q32"], kw["mq16"], eos_id >= 0)
    whole = np_spans(ids, lengths, **kw)
    for iw, tw in ((in_len, tgt_len), (in_len + 70, tgt_len + 1), (in_len - 1, tgt_len - 1), (in_len // 2, tgt_len // 2), (1, 1)):
        for lens in (lengths, None):
            got, _ = both(L, ids, lens, in_width=iw, tgt_width=tw, **kw)
            if lens is not None:
                assert np.array_equal(got["in_lengths"], whole["in_lengths"]) and np.array_equal(got["tgt_lengths"], whole["tgt_lengths"])
                k = min(iw, in_len)
                assert np.array_equal(got["inputs"][:, :k], whole["inputs"][:, :k])
                k = min(tw, tgt_len)
                assert np.array_equal(got["targets"][:, :k], whole["targets"][:, :k])


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_spans_capacities_and_optional_outputs(L, dtype):
    width, rows = 65, 37
    ids = make_ids(rows, width, seed=21, dtype=dtype)
    lengths = make_lengths(rows, width, seed=22)
    kw = dict(seed=8, stream_id=1, elem_base=ONE - 1000, density_q32=threshold(0.15), mq16=mean_q16(3.0), sentinel_first=31999,
              eos_id=1, pad_id=0)
    for cap in (0, 1, rows - 1, rows + 5):
        both(L, ids, lengths, cap=cap, **kw)
    for skip in (("in_lengths",), ("tgt_lengths",), ("noise",), ("in_lengths", "tgt_lengths", "noise")):
        got, _ = both(L, ids, lengths, skip=skip, **kw)
        assert set(got) == set(KEYS) - set(skip)
    got = run_spans(L, np.zeros((0, 8), dtype=dtype), None, **kw)
    assert got["inputs"].shape[0] == 0


def test_spans_parts_equal_the_whole(L):
    """Rows 10.. and 25.. on their own, elem_base moved to the part's first row x width, equal the whole
    call's rows (the element index crosses 2^32 inside the batch)."""
    width, rows = 127, 37
    ids = make_ids(rows, width, seed=31)
    kw = dict(seed=77, stream_id=3, density_q32=threshold(0.25), mq16=mean_q16(2.5), sentinel_first=31999, eos_id=1, pad_id=0)
    base = ONE - 12 * width
    whole = run_spans(L, ids, None, elem_base=base, **kw)
    check(whole, np_spans(ids, None, elem_base=base, **kw))
    for first in (10, 25):
        part = run_spans(L, ids[first:], None, elem_base=base + first * width, **kw)
        for key in KEYS:
            assert np.array_equal(part[key], whole[key][first:]), key


def test_spans_draws_depend_on_seed_and_stream_only(L):
    width, rows = 128, 37
    ids = make_ids(rows, width, seed=41)
    kw = dict(density_q32=threshold(0.15), mq16=mean_q16(3.0), sentinel_first=31999, eos_id=1, pad_id=0)
    torch.manual_seed(1)
    one = run_spans(L, ids, None, seed=5, stream_id=6, **kw)
    torch.manual_seed(2)
    torch.rand(10, device="cuda")
    again = run_spans(L, ids, None, seed=5, stream_id=6, lead=0, **kw)
    assert all(np.array_equal(one[k], again[k]) for k in KEYS)
    for other in (dict(seed=6, stream_id=6), dict(seed=5, stream_id=7), dict(seed=5 + (1 << 32), stream_id=6),
                  dict(seed=5, stream_id=6 + (1 << 32))):
        res = run_spans(L, ids, None, **other, **kw)
        assert not np.array_equal(res["noise"], one["noise"]), other
        assert np.array_equal(res["in_lengths"], one["in_lengths"])  # the counts do not depend on the draw


# ------------------------------------------------------------------------------------------ Python layers
def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_span_ids(L):
    from akshar_amd import engine
    width, rows = 200, 37
    ids = make_ids(rows, width, seed=51, dtype=np.int64)
    lengths = make_lengths(rows, width, seed=52).clip(0, width)
    dev, dl = torch.from_numpy(ids).cuda(), torch.from_numpy(lengths).cuda()
    got = _host(engine.span_ids(dev, dl, sentinel_first=31999, eos_id=1, pad_id=0, seed=9, stream_id=2, noise_mask=True))
    ref = np_spans(ids, lengths, seed=9, stream_id=2, density_q32=threshold(0.15), mq16=mean_q16(3.0), sentinel_first=31999,
                   sentinel_step=-1, eos_id=1, pad_id=0, tgt_pad_id=-100)
    assert set(got) == {"input_ids", "labels", "input_lengths", "label_lengths", "noise_mask"}
    assert got["input_ids"].shape == (rows, engine.span_lengths(width, eos=True)[2]) and got["input_ids"].dtype == np.int64
    for a, b in (("input_ids", "inputs"), ("labels", "targets"), ("input_lengths", "in_lengths"), ("label_lengths", "tgt_lengths")):
        assert np.array_equal(got[a], ref[b]), a
    assert got["noise_mask"].dtype == np.bool_ and np.array_equal(got["noise_mask"], ref["noise"] != 0)
    # no eos, <mask>-style sentinels, widths given, int32, no mask
    got = _host(engine.span_ids(dev.int(), None, sentinel_first=4, sentinel_step=0, pad_id=0, label_pad=-1, in_width=180,
                                tgt_width=20, noise_density=0.3, mean_span_length=2.0, elem_base=123))
    ref = np_spans(ids.astype(np.int32), None, elem_base=123, density_q32=threshold(0.3), mq16=mean_q16(2.0), sentinel_first=4,
                   sentinel_step=0, eos_id=-1, pad_id=0, tgt_pad_id=-1, in_width=180, tgt_width=20)
    assert set(got) == {"input_ids", "labels", "input_lengths", "label_lengths"}
    assert np.array_equal(got["input_ids"], ref["inputs"]) and np.array_equal(got["labels"], ref["targets"])
    S = engine.span_lengths(width)[1]
    with pytest.raises(ValueError, match="sentinels"):
        engine.span_ids(dev, sentinel_first=31999, pad_id=0, n_sentinels=S - 1)
    assert engine.span_ids(dev, sentinel_first=31999, pad_id=0, n_sentinels=S)["labels"].shape[0] == rows
    empty = engine.span_ids(dev[:0], sentinel_first=31999, pad_id=0)
    assert empty["input_ids"].shape == (0, engine.span_lengths(width)[2])


@pytest.fixture(scope="module")
def toks():
    from akshar_amd.tokenizer import aksharTokenizer
    return {"bpe": aksharTokenizer(BPE_PATH, "bpe"), "spm": aksharTokenizer(SPM_PATH, "sentencepiece")}


@pytest.fixture(scope="module")
def texts():
    return [r["text"] for r in load_dense_golden()["rows"] if len(r["ids"]) < 200]  # 295 rows, some 4,500 ids


@pytest.mark.parametrize("name", ["bpe", "spm"])
def test_encode_spans(toks, texts, name):
    from akshar_amd import engine
    tok = toks[name]
    m = tok.model.model
    pad = None if name == "bpe" else 5
    eos = m.eos if name == "bpe" else m.eos_id
    inputs_length = 64
    block, tgt_len = engine.span_raw_length(inputs_length, eos=True)
    blocks = tok.encode_blocks(texts, block, pad_id=pad, drop_last=True)["input_ids"].cpu().numpy()
    assert blocks.shape[0] >= 4 and blocks.shape[1] == block
    got = _host(tok.encode_spans(texts, inputs_length, seed=11, stream_id=2, pad_id=pad))
    assert set(got) == {"input_ids", "labels", "input_lengths", "label_lengths"}
    assert got["input_ids"].shape == (blocks.shape[0], inputs_length) and got["labels"].shape == (blocks.shape[0], tgt_len)
    ref = np_spans(blocks, None, seed=11, stream_id=2, density_q32=threshold(0.15), mq16=mean_q16(3.0), sentinel_first=m.mask_id,
                   sentinel_step=0, eos_id=eos, pad_id=tok._pad_id(pad), tgt_pad_id=-100, in_width=inputs_length)
    assert np.array_equal(got["input_ids"], ref["inputs"]) and np.array_equal(got["labels"], ref["targets"])
    assert np.array_equal(got["input_lengths"], ref["in_lengths"]) and (got["label_lengths"] == tgt_len).all()
    S = engine.span_lengths(block)[1]
    assert ((got["input_ids"] == m.mask_id).sum(axis=1) >= S).all() and (got["input_ids"][np.arange(len(blocks)), got["input_lengths"] - 1] == eos).all()
    # reproducible, another stream differs, the (buf, offs) form is the list form, int64 on request
    again = _host(tok.encode_spans(engine.pack(texts), inputs_length, seed=11, stream_id=2, pad_id=pad, dtype=torch.int64))
    assert again["input_ids"].dtype == np.int64 and all(np.array_equal(again[k], got[k]) for k in got)
    other = _host(tok.encode_spans(texts, inputs_length, seed=11, stream_id=3, pad_id=pad))
    assert not np.array_equal(other["labels"], got["labels"])
    # numbered sentinels: the range must hold a block's spans
    top = m.vocab_size - 1
    t5 = _host(tok.encode_spans(texts, inputs_length, seed=11, stream_id=2, pad_id=pad, sentinel_first=top))
    ref = np_spans(blocks, None, seed=11, stream_id=2, density_q32=threshold(0.15), mq16=mean_q16(3.0), sentinel_first=top,
                   sentinel_step=-1, eos_id=eos, pad_id=tok._pad_id(pad), tgt_pad_id=-100, in_width=inputs_length)
    assert np.array_equal(t5["input_ids"], ref["inputs"]) and np.array_equal(t5["labels"], ref["targets"])
    with pytest.raises(ValueError, match="sentinels"):
        tok.encode_spans(texts, inputs_length, sentinel_first=S - 2, pad_id=pad)  # ids S-2 .. 0: one too few
    with pytest.raises(ValueError, match="sentinels"):
        tok.encode_spans(texts, inputs_length, sentinel_first=m.vocab_size - S + 1, sentinel_step=1, pad_id=pad)
    with pytest.raises(ValueError, match="sentinel_step"):
        tok.encode_spans(texts, inputs_length, sentinel_step=-1, pad_id=pad)
