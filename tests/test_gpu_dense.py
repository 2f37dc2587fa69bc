"""Padded batches and packed blocks on the device (include/akshar.h ak_ids_pad / ak_ids_pack,
akshar_amd/csrc/ak_k_dense.hip), bit-exact against the numpy restatements of tests/test_dense_ref.py
(which that file pins to HF `tokenizers`) and against the HF records themselves.

Every output array of every raw call (ids, mask, lengths, pos, doc) is allocated for the full result
plus a guard band of BUFFER_GUARD sentinel elements: what lies at or past the capacity, the slack
between a short capacity and the full size included, must come back untouched.
"""
import numpy as np
import pytest
import torch

from tests.conftest import BPE_PATH, SPM_PATH
from tests.test_dense_ref import LENGTH_MIX, load_dense_golden, mixed_rows, np_pack, np_pad, pack_id_rows
from tests.test_gpu_buffers import S32, S64
from tests.util import BUFFER_GUARD as G

pytestmark = pytest.mark.gpu

S8 = 0x77  # mask bytes are 0 / 1
PAD_LEFT, TRUNC_LEFT, DENSE_I64, DROP_LAST = 1, 2, 4, 8
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 256)
KEEPS = ((0, 0), (1, 1), (2, 0), (0, 3))
BLOCKS = (1, 2, 3, 4, 5, 64, 100, 4096)


@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    assert torch.cuda.is_available()
    return _lib.lib()


def _guarded(numel, dtype, sentinel, lead=0):
    """A device tensor of lead + numel + G sentinel elements and its view from `lead` on."""
    t = torch.full((lead + numel + G,), sentinel, dtype=dtype, device="cuda")
    return t[lead:]


def _dev_rows(ids, offs, lead=0):
    """Host id rows on the device; ids as a view `lead` elements into a larger tensor (an unaligned
    source: nothing in front of the view is a row's)."""
    big = torch.full((lead + max(len(ids), 1) + 8,), -123456, dtype=torch.int32, device="cuda")
    big[lead:lead + len(ids)] = torch.from_numpy(ids).cuda()
    return big[lead:lead + len(ids)] if len(ids) else big[lead:lead + 1], torch.from_numpy(offs).cuda()


def _split(t, used, sentinel):
    """Host copy of a guarded output: (the first `used` elements, True if all others are the sentinel)."""
    h = t.cpu().numpy()
    return h[:used], bool((h[used:] == sentinel).all())


def run_pad(L, gi, go, n, width, pad_id, h, t, flags, cap, mask=True, lengths=True, lead=0):
    """ak_ids_pad through the raw C-ABI into guarded outputs sized for all n rows; returns the rows
    below the capacity as (out, mask | None, lengths | None), after the guard checks."""
    i64 = bool(flags & DENSE_I64)
    out = _guarded(n * width, torch.int64 if i64 else torch.int32, S64 if i64 else S32, lead)
    mk = _guarded(n * width, torch.uint8, S8, lead) if mask else None
    ln = _guarded(n, torch.int32, S32, lead) if lengths else None
    rc = L.ak_ids_pad(gi.data_ptr(), go.data_ptr(), n, width, pad_id, h, t, flags, out.data_ptr(), cap,
                      mk.data_ptr() if mask else None, ln.data_ptr() if lengths else None, None)
    assert rc == 0, L.ak_last_error()
    torch.cuda.synchronize()
    rows = min(n, cap)
    res = []
    for arr, used, sent in ((out, rows * width, S64 if i64 else S32), (mk, rows * width, S8), (ln, rows, S32)):
        if arr is None:
            res.append(None)
            continue
        got, clean = _split(arr, used, sent)
        assert clean, "stored at or past the capacity"
        res.append(got)
    return res


def check_pad(res, ref, rows):
    out, mask, lengths = res
    r_out, r_mask, r_len = ref
    width = r_out.shape[1]
    assert np.array_equal(out.reshape(rows, width), r_out[:rows])
    if mask is not None:
        assert np.array_equal(mask.reshape(rows, width), r_mask[:rows])
    if lengths is not None:
        assert np.array_equal(lengths, r_len[:rows])


# ------------------------------------------------------------------------------------------ pad
@pytest.fixture(scope="module")
def dense_golden():
    return load_dense_golden()


def test_pad_matches_every_hf_record(L, dense_golden):
    ids, offs = pack_id_rows([r["ids"] for r in dense_golden["rows"]])
    gi, go = _dev_rows(ids, offs)
    n = len(offs) - 1
    for rec in dense_golden["records"]:
        flags = (PAD_LEFT if rec["padding_side"] == "left" else 0) | (TRUNC_LEFT if rec["truncation_side"] == "left" else 0)
        w = rec["max_length"]
        out, mask, lengths = run_pad(L, gi, go, n, w, dense_golden["pad_id"], 1, 1, flags, n)
        key = (w, rec["truncation_side"], rec["padding_side"])
        assert out.reshape(n, w).tolist() == rec["ids"], key
        assert mask.reshape(n, w).tolist() == rec["attention_mask"], key
        assert lengths.tolist() == [sum(m) for m in rec["attention_mask"]], key


@pytest.fixture(scope="module")
def mixed():
    """About 2,000 rows of the adversarial length mix (rows shorter than keep_head + keep_tail, empty
    rows and rows far over every width next to each other), on the host and on the device at element
    offsets 1 and 3 of a larger tensor."""
    rows = mixed_rows(2002, seed=7)
    assert {len(r) for r in rows} == set(LENGTH_MIX)
    ids, offs = pack_id_rows(rows)
    return {"ids": ids, "offs": offs, "n": len(rows), "dev": {lead: _dev_rows(ids, offs, lead) for lead in (1, 3)}}


@pytest.mark.parametrize("width", WIDTHS)
def test_pad_adversarial_shapes(L, mixed, width):
    """Every keep pair that fits the width x the four side combinations x int32 / int64, the optional
    outputs NULL in turn, an unaligned source, a negative pad id."""
    n, case = mixed["n"], 0
    for h, t in KEEPS:
        if h + t > width:
            continue
        for sides in range(4):
            ref = np_pad(mixed["ids"], mixed["offs"], width, -7, h, t, bool(sides & PAD_LEFT), bool(sides & TRUNC_LEFT))
            for i64 in (0, DENSE_I64):
                gi, go = mixed["dev"][(1, 3)[case % 2]]
                res = run_pad(L, gi, go, n, width, -7, h, t, sides | i64, n, mask=case % 3 != 1, lengths=case % 3 != 2)
                check_pad(res, ref, n)
                case += 1
    assert case >= 8


@pytest.mark.parametrize("width", WIDTHS)
def test_pad_short_capacities(L, mixed, width):
    n = mixed["n"]
    h, t = (1, 1) if width >= 2 else (0, 0)
    gi, go = mixed["dev"][1]
    for k, cap in enumerate((0, n // 2, n, n + 5)):
        flags = (PAD_LEFT, TRUNC_LEFT, DENSE_I64, PAD_LEFT | TRUNC_LEFT)[k]
        ref = np_pad(mixed["ids"], mixed["offs"], width, 0, h, t, bool(flags & PAD_LEFT), bool(flags & TRUNC_LEFT))
        check_pad(run_pad(L, gi, go, n, width, 0, h, t, flags, cap), ref, min(n, cap))


@pytest.mark.parametrize("width", [3, 8, 65])
def test_pad_unaligned_outputs(L, mixed, width):
    """Outputs at element offset 1 of their allocations (4-byte aligned ids, 1-byte aligned mask): the
    element-store path gives the same result and keeps inside the same bounds."""
    n = mixed["n"]
    gi, go = mixed["dev"][3]
    ref = np_pad(mixed["ids"], mixed["offs"], width, -7, 0, 0)
    for i64 in (0, DENSE_I64):
        check_pad(run_pad(L, gi, go, n, width, -7, 0, 0, i64, n - 3, lead=1), ref, n - 3)


def test_pad_all_rows_empty_and_no_rows(L):
    ids, offs = pack_id_rows([[]] * 70)
    gi, go = _dev_rows(ids, offs)
    out, mask, lengths = run_pad(L, gi, go, 70, 5, 9, 1, 1, PAD_LEFT, 70)
    assert (out == 9).all() and not mask.any() and not lengths.any()
    out, mask, lengths = run_pad(L, gi, go, 0, 5, 9, 1, 1, 0, 70)
    assert len(out) == len(mask) == len(lengths) == 0


# ------------------------------------------------------------------------------------------ pack
def run_pack(L, gi, go, n, n_ids, block, sep_id, pad_id, flags, cap=None, pos=True, doc=True, lead=0):
    """ak_ids_pack through the raw C-ABI into guarded outputs sized for every block; returns the blocks
    below the capacity as (out, pos | None, doc | None), after the guard checks."""
    nb = int(L.ak_ids_pack_blocks(n_ids, n, int(sep_id >= 0), block, flags))
    cap = nb if cap is None else cap
    i64 = bool(flags & DENSE_I64)
    out = _guarded(nb * block, torch.int64 if i64 else torch.int32, S64 if i64 else S32, lead)
    ps = _guarded(nb * block, torch.int32, S32, lead) if pos else None
    dc = _guarded(nb * block, torch.int32, S32, lead) if doc else None
    rc = L.ak_ids_pack(gi.data_ptr(), go.data_ptr(), n, block, sep_id, pad_id, flags, out.data_ptr(),
                       ps.data_ptr() if pos else None, dc.data_ptr() if doc else None, cap, None)
    assert rc == 0, L.ak_last_error()
    torch.cuda.synchronize()
    used = min(nb, cap) * block
    res = []
    for arr, sent in ((out, S64 if i64 else S32), (ps, S32), (dc, S32)):
        if arr is None:
            res.append(None)
            continue
        got, clean = _split(arr, used, sent)
        assert clean, "stored at or past the capacity"
        res.append(got)
    return nb, res


PACK_BATCHES = {
    "mixed": lambda: mixed_rows(2002, seed=7),
    "empty": lambda: [[]] * 130,
    "ones": lambda: [[i + 1] for i in range(200)],   # more than 64 documents inside one wave's 256 elements
    "none": lambda: [],
    "long": lambda: [list(range(1, 10001))],          # one document over many blocks and wave spans
}


@pytest.mark.parametrize("batch", sorted(PACK_BATCHES))
def test_pack_matches_numpy(L, batch):
    rows = PACK_BATCHES[batch]()
    ids, offs = pack_id_rows(rows)
    n = len(rows)
    gi, go = _dev_rows(ids, offs, lead=1)
    case, exact = 0, 0
    for block in BLOCKS:
        for sep_id in (3, -1):
            total = len(ids) + (n if sep_id >= 0 else 0)
            exact += total > 0 and total % block == 0
            for drop in (0, DROP_LAST):
                i64 = DENSE_I64 if case % 2 else 0
                ref = np_pack(ids, offs, block, sep_id, -5, bool(drop))
                nb, res = run_pack(L, gi, go, n, len(ids), block, sep_id, -5, drop | i64, pos=case % 3 != 1,
                                   doc=case % 3 != 2)
                assert nb == ref[0].shape[0]
                for got, want in zip(res, ref):
                    if got is not None:
                        assert np.array_equal(got.reshape(nb, block), want), (block, sep_id, drop)
                case += 1
    if batch in ("ones", "long"):
        assert exact >= 4  # stream lengths that are a whole number of blocks


@pytest.mark.parametrize("batch", ["mixed", "ones", "long"])
def test_pack_short_capacities(L, batch):
    rows = PACK_BATCHES[batch]()
    ids, offs = pack_id_rows(rows)
    n = len(rows)
    gi, go = _dev_rows(ids, offs, lead=3)
    for block in (3, 64, 100):
        ref = np_pack(ids, offs, block, 3, 0)
        for cap in (0, 1, ref[0].shape[0] // 2, ref[0].shape[0] + 4):
            for i64 in (0, DENSE_I64):
                nb, res = run_pack(L, gi, go, n, len(ids), block, 3, 0, i64, cap=cap)
                k = min(nb, cap)
                for got, want in zip(res, ref):
                    assert np.array_equal(got.reshape(k, block), want[:k]), (block, cap)


def test_pack_unaligned_outputs(L):
    rows = PACK_BATCHES["mixed"]()
    ids, offs = pack_id_rows(rows)
    gi, go = _dev_rows(ids, offs)
    ref = np_pack(ids, offs, 100, -1, -5)
    for i64 in (0, DENSE_I64):
        nb, res = run_pack(L, gi, go, len(rows), len(ids), 100, -1, -5, i64, lead=1)
        for got, want in zip(res, ref):
            assert np.array_equal(got.reshape(nb, 100), want)


# ------------------------------------------------------------------------------------------ Python layer
@pytest.fixture(scope="module")
def toks():
    from akshar_amd.tokenizer import aksharTokenizer
    return {"bpe": aksharTokenizer(BPE_PATH, "bpe"), "spm": aksharTokenizer(SPM_PATH, "sentencepiece")}


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_encode_padded_bpe_equals_hf(toks, dense_golden):
    """Text in, HF's padded batch out: the first rows of the fixture (the empty string, one-token rows
    and the rows over 70 ids among them) through normalize + encode + pad."""
    rows = dense_golden["rows"]
    pick = [i for i in range(24) if len(rows[i]["ids"]) < 2600]  # one 2,500-id row, not the 18,000-id one (seconds per encode)
    texts = [rows[i]["text"] for i in pick]
    assert "" in texts and len(pick) >= 20 and max(len(rows[i]["ids"]) for i in pick) > 70
    for rec in dense_golden["records"]:
        got = _host(toks["bpe"].encode_padded(texts, rec["max_length"], padding_side=rec["padding_side"],
                                              truncation_side=rec["truncation_side"]))
        assert got["input_ids"].dtype == np.int32 and got["attention_mask"].dtype == np.bool_
        assert got["input_ids"].tolist() == [rec["ids"][i] for i in pick]
        assert got["attention_mask"].astype(np.uint8).tolist() == [rec["attention_mask"][i] for i in pick]
        assert got["lengths"].tolist() == [sum(rec["attention_mask"][i]) for i in pick]


def _texts(dense_golden):
    return [r["text"] for r in dense_golden["rows"][:40] if len(r["ids"]) < 200]


def test_encode_padded_spm_equals_numpy(toks, dense_golden):
    texts = _texts(dense_golden)
    ids, offs = pack_id_rows(toks["spm"].encode_batch(texts))
    for width, pside, tside in ((1, "right", "right"), (7, "left", "right"), (64, "right", "left")):
        got = _host(toks["spm"].encode_padded(texts, width, padding_side=pside, truncation_side=tside, pad_id=5))
        out, mask, lengths = np_pad(ids, offs, width, 5, 0, 0, pside == "left", tside == "left")
        assert np.array_equal(got["input_ids"], out) and np.array_equal(got["lengths"], lengths)
        assert np.array_equal(got["attention_mask"], mask.astype(bool))


def test_encode_blocks_agrees_with_numpy(toks, dense_golden):
    from akshar_amd import engine
    texts = _texts(dense_golden)
    for name, sep in (("spm", toks["spm"].model.model.eos_id), ("bpe", -1)):
        tok = toks[name]
        rows = tok.encode_batch(texts)
        ids, offs = pack_id_rows(rows)
        pad = 5 if name == "spm" else None  # BPE: the model's <pad>
        got = _host(tok.encode_blocks(texts, 16, pad_id=pad))
        out, pos, doc = np_pack(ids, offs, 16, sep, 5 if name == "spm" else 0)
        assert np.array_equal(got["input_ids"], out)
        assert np.array_equal(got["position_ids"], pos) and np.array_equal(got["doc_ids"], doc)
        if name == "spm":  # </s> after every row, the empty ones included
            flat, d = got["input_ids"].ravel(), got["doc_ids"].ravel()
            ends = [np.flatnonzero(d == r)[-1] for r in range(len(texts))]
            assert sep == 2 and all(flat[e] == sep for e in ends)
            assert [int((d == r).sum()) for r in range(len(texts))] == [len(r) + 1 for r in rows]
        # the same from a (buf, offs) device pair, and with the last block dropped
        pair = engine.pack(texts)
        again = _host(tok.encode_blocks(pair, 16, pad_id=pad))
        assert all(np.array_equal(again[k], got[k]) for k in got)
        short = _host(tok.encode_blocks(pair, 16, pad_id=pad, drop_last=True))
        nb = (len(ids) + (len(rows) if sep >= 0 else 0)) // 16
        assert short["input_ids"].shape == (nb, 16) and np.array_equal(short["input_ids"], out[:nb])
        padded = _host(tok.encode_padded(pair, 9, pad_id=5))
        assert np.array_equal(padded["input_ids"], _host(tok.encode_padded(texts, 9, pad_id=5))["input_ids"])


def test_side_stream_then_default_stream(toks, dense_golden):
    texts = _texts(dense_golden)
    want = {}
    for name, tok in toks.items():
        want[name] = (_host(tok.encode_padded(texts, 12, pad_id=1)), _host(tok.encode_blocks(texts, 32, pad_id=1)))
    side = torch.cuda.Stream()
    for stream in (side, torch.cuda.default_stream()):
        for name, tok in toks.items():
            with torch.cuda.stream(stream):
                a, b = tok.encode_padded(texts, 12, pad_id=1), tok.encode_blocks(texts, 32, pad_id=1)
            stream.synchronize()
            for got, ref in zip((_host(a), _host(b)), want[name]):
                assert all(np.array_equal(got[k], ref[k]) for k in ref), (name, stream is side)


def test_engine_outputs_in_place_and_int64(toks, dense_golden):
    from akshar_amd import engine
    texts = _texts(dense_golden)
    ids, oo = toks["bpe"].encode_packed(*engine.pack(texts))
    n = len(texts)
    out = torch.empty(n * 10, dtype=torch.int64, device="cuda")
    mask = torch.empty((n, 10), dtype=torch.uint8, device="cuda")
    lengths = torch.empty(n, dtype=torch.int32, device="cuda")
    a, m, ln = engine.pad_ids(ids, oo, 10, 0, keep_head=1, keep_tail=1, dtype=torch.int64, out=out, mask=mask, lengths=lengths)
    assert a.data_ptr() == out.data_ptr() and a.shape == (n, 10) and m.data_ptr() == mask.data_ptr() and ln is lengths
    ref = np_pad(ids.cpu().numpy(), oo.cpu().numpy(), 10, 0, 1, 1, dtype=np.int64)
    assert np.array_equal(a.cpu().numpy(), ref[0]) and np.array_equal(m.cpu().numpy(), ref[1])
    assert np.array_equal(ln.cpu().numpy(), ref[2])
    blocks, pos, doc = engine.pack_ids(ids, oo, 8, dtype=torch.int64, positions=False)
    assert pos is None and blocks.dtype == torch.int64 and doc.dtype == torch.int32
    assert np.array_equal(blocks.cpu().numpy(), np_pack(ids.cpu().numpy(), oo.cpu().numpy(), 8, -1, 0, dtype=np.int64)[0])


def test_python_layer_errors(toks):
    from akshar_amd import engine
    from akshar_amd.tokenizer import aksharTokenizer
    bare = aksharTokenizer()
    for call in (lambda: bare.encode_padded(["a"], 4), lambda: bare.encode_blocks(["a"], 4)):
        with pytest.raises(ValueError, match="need model for IDs"):
            call()
    for call in (lambda: toks["spm"].encode_padded(["a"], 4), lambda: toks["spm"].encode_blocks(["a"], 4)):
        with pytest.raises(ValueError, match="pad"):
            call()
    with pytest.raises(ValueError):
        toks["bpe"].encode_padded(["a"], 1)  # no room for <s> ... </s>
    with pytest.raises(ValueError):
        toks["bpe"].encode_padded(["a"], 4, padding_side="up")
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        engine.pad_ids(ids.long(), offs, 4, 0)
    with pytest.raises(TypeError):
        engine.pad_ids(ids.cpu(), offs.cpu(), 4, 0)
    with pytest.raises(TypeError):
        engine.pack_ids(ids, offs.int(), 4)
    with pytest.raises(TypeError):
        engine.pad_ids(torch.zeros(8, dtype=torch.int32, device="cuda")[::2], offs, 4, 0)
    with pytest.raises(TypeError):
        engine.pad_ids(ids, offs, 4, 0, out=torch.empty(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        engine.pad_ids(ids, offs, 4, 0, out=torch.empty(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        engine.pack_ids(ids, offs, 0)
