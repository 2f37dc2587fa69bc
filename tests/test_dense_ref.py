"""Padded batches and packed blocks (include/akshar.h ak_ids_pad / ak_ids_pack) without a GPU: what
the two ops compute, restated in plain numpy / Python and pinned to HF `tokenizers`.

  - np_pad with keep_head = keep_tail = 1 reproduces every record of tests/golden/dense_hf.json.gz (HF
    enable_truncation + enable_padding on models/akshar.json, tools/gen_golden_dense.py);
  - np_pack agrees with the obvious Python loop over lists;
  - the C-ABI's host-side argument errors, ak_ids_pack_blocks, and the models' pad / eos / bos ids.

tests/test_gpu_dense.py holds the kernels to np_pad / np_pack.
"""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from tests.conftest import BPE_PATH, ROOT

DENSE_GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_hf.json.gz")
LENGTH_MIX = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000)


def load_dense_golden():
    with gzip.open(DENSE_GOLDEN, "rt", encoding="utf-8") as f:
        return json.load(f)


def pack_id_rows(rows):
    """list[list[int]] -> (int32 ids, int64 offsets)."""
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        np.cumsum([len(r) for r in rows], out=offs[1:])
    return np.asarray([x for r in rows for x in r], dtype=np.int32), offs


def mixed_rows(n, seed, lengths=LENGTH_MIX):
    """n rows whose lengths cycle through `lengths` with a stride, so neighbouring rows (and lanes)
    differ; ids are distinct small positive numbers, so a misplaced id shows."""
    rng = np.random.default_rng(seed)
    lens = [lengths[(5 * i + i // len(lengths)) % len(lengths)] for i in range(n)]
    return [rng.integers(1, 30000, size=ln).tolist() for ln in lens]


# ------------------------------------------------------------------------------------------ restatements
def np_pad(ids, offs, width, pad_id, h=0, t=0, pad_left=False, trunc_left=False, dtype=np.int32):
    """(out [n, width], mask u8 [n, width], lengths int32 [n]) as include/akshar.h defines ak_ids_pad."""
    n = len(offs) - 1
    out = np.full((n, width), pad_id, dtype=dtype)
    mask = np.zeros((n, width), dtype=np.uint8)
    lengths = np.zeros(n, dtype=np.int32)
    for r in range(n):
        row = ids[offs[r]:offs[r + 1]]
        rh, rt = (h, t) if len(row) >= h + t else (0, 0)
        if len(row) > width:
            body = row[rh:len(row) - rt]
            keep = width - rh - rt
            body = body[len(body) - keep:] if trunc_left else body[:keep]
            row = np.concatenate([row[:rh], body, row[len(row) - rt:]])
        k = len(row)
        at = width - k if pad_left else 0
        out[r, at:at + k] = row
        mask[r, at:at + k] = 1
        lengths[r] = k
    return out, mask, lengths


def np_pack(ids, offs, block, sep_id, pad_id, drop_last=False, dtype=np.int32):
    """(out, pos, doc), each [n_blocks, block], as include/akshar.h defines ak_ids_pack (sep_id < 0: no
    separator)."""
    n = len(offs) - 1
    offs = np.asarray(offs, dtype=np.int64)
    s = 1 if sep_id >= 0 else 0
    starts = offs + np.arange(n + 1, dtype=np.int64) * s
    total = int(starts[n])
    nb = total // block if drop_last else -(-total // block)
    p = np.arange(nb * block, dtype=np.int64)
    live = p < total
    row = np.searchsorted(starts, p, side="right") - 1  # the last row starting at or before p
    row[~live] = 0
    pos = np.where(live, p - starts[row], 0)
    is_sep = live & (s == 1) & (p + 1 == starts[np.minimum(row + 1, n)])
    src = np.where(live & ~is_sep, p - row * s, 0)
    flat = np.concatenate([np.asarray(ids, dtype=np.int64), [0]])  # an empty ids still indexes
    out = np.where(is_sep, sep_id, np.where(live, flat[np.minimum(src, len(flat) - 1)], pad_id))
    doc = np.where(live, row, -1)
    shape = (nb, block)
    return out.astype(dtype).reshape(shape), pos.astype(np.int32).reshape(shape), doc.astype(np.int32).reshape(shape)


def loop_pack(rows, block, sep_id, pad_id, drop_last):
    """The same from lists: (ids, pos, doc) of the stream, then cut."""
    ids, pos, doc = [], [], []
    for r, row in enumerate(rows):
        full = list(row) + ([sep_id] if sep_id >= 0 else [])
        ids += full
        pos += list(range(len(full)))
        doc += [r] * len(full)
    if drop_last:
        keep = len(ids) // block * block
        ids, pos, doc = ids[:keep], pos[:keep], doc[:keep]
    else:
        fill = -len(ids) % block
        ids, pos, doc = ids + [pad_id] * fill, pos + [0] * fill, doc + [-1] * fill
    return [np.asarray(x, dtype=np.int64).reshape(-1, block) for x in (ids, pos, doc)]


# ------------------------------------------------------------------------------------------ semantics
@pytest.fixture(scope="module")
def dense_golden():
    return load_dense_golden()


def test_fixture_covers_the_edge_rows(dense_golden):
    lens = [len(r["ids"]) for r in dense_golden["rows"]]
    assert len(lens) >= 250 and dense_golden["rows"][0]["text"] == ""
    assert 2 in lens and 3 in lens and sum(n > 70 for n in lens) >= 3
    got = {(r["max_length"], r["truncation_side"], r["padding_side"]) for r in dense_golden["records"]}
    assert got == {(m, a, b) for m in (2, 3, 6, 64) for a in ("left", "right") for b in ("left", "right")}


def test_np_pad_reproduces_every_hf_record(dense_golden):
    ids, offs = pack_id_rows([r["ids"] for r in dense_golden["rows"]])
    for rec in dense_golden["records"]:
        out, mask, lengths = np_pad(ids, offs, rec["max_length"], dense_golden["pad_id"], 1, 1,
                                    rec["padding_side"] == "left", rec["truncation_side"] == "left")
        key = (rec["max_length"], rec["truncation_side"], rec["padding_side"])
        assert out.tolist() == rec["ids"], key
        assert mask.tolist() == rec["attention_mask"], key
        assert lengths.tolist() == [sum(m) for m in rec["attention_mask"]], key


def test_np_pad_short_rows_and_no_template():
    ids, offs = pack_id_rows([[7], [], [1, 2, 3, 4, 5, 6]])
    out, mask, lengths = np_pad(ids, offs, 4, -9, 2, 1)  # the 1-id row is shorter than h + t: kept whole
    assert out.tolist() == [[7, -9, -9, -9], [-9] * 4, [1, 2, 3, 6]]
    assert mask.tolist() == [[1, 0, 0, 0], [0] * 4, [1] * 4] and lengths.tolist() == [1, 0, 4]
    out, _, _ = np_pad(ids, offs, 4, -9, 2, 1, pad_left=True, trunc_left=True)
    assert out.tolist() == [[-9, -9, -9, 7], [-9] * 4, [1, 2, 5, 6]]
    out, _, _ = np_pad(ids, offs, 4, 0, trunc_left=True)
    assert out[2].tolist() == [3, 4, 5, 6]


@pytest.mark.parametrize("sep_id", [-1, 3])
@pytest.mark.parametrize("drop_last", [False, True])
def test_np_pack_agrees_with_the_list_loop(sep_id, drop_last):
    batches = [mixed_rows(120, seed=11), [[]] * 7, [[5]] * 200, [], [list(range(1, 1001))], [[], [4, 5, 6], [], []]]
    for rows in batches:
        ids, offs = pack_id_rows(rows)
        for block in (1, 2, 3, 4, 5, 64, 100, 4096):
            got = np_pack(ids, offs, block, sep_id, -7, drop_last)
            want = loop_pack(rows, block, sep_id, -7, drop_last)
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g, w), (len(rows), block)


def test_np_pack_positions_cross_block_boundaries():
    ids, offs = pack_id_rows([[10, 11, 12, 13, 14], [], [20]])
    out, pos, doc = np_pack(ids, offs, 4, 3, 0)
    assert out.tolist() == [[10, 11, 12, 13], [14, 3, 3, 20], [3, 0, 0, 0]]
    assert pos.tolist() == [[0, 1, 2, 3], [4, 5, 0, 0], [1, 0, 0, 0]]
    assert doc.tolist() == [[0, 0, 0, 0], [0, 0, 1, 2], [2, -1, -1, -1]]
    out, pos, doc = np_pack(ids, offs, 4, -1, 0)  # no separator: the empty row appears nowhere
    assert out.tolist() == [[10, 11, 12, 13], [14, 20, 0, 0]] and doc.tolist() == [[0, 0, 0, 0], [0, 2, -1, -1]]


# ------------------------------------------------------------------------------------------ C-ABI, host side
PAD_LEFT, TRUNC_LEFT, DENSE_I64, DROP_LAST = 1, 2, 4, 8


@pytest.fixture(scope="module")
def L():
    from akshar_amd import _lib
    return _lib.lib()


def _is_arg_error(L, rc):
    from akshar_amd import _lib
    return rc == _lib.AK_ERR_ARG and len(L.ak_last_error()) > 0


def test_flag_values_match_the_header():
    from akshar_amd import _lib
    src = open(os.path.join(ROOT, "include", "akshar.h")).read()
    for name in ("AK_PAD_LEFT", "AK_TRUNC_LEFT", "AK_DENSE_I64", "AK_PACK_DROP_LAST"):
        assert ("#define %s %d" % (name, getattr(_lib, name))) in src
    assert (_lib.AK_PAD_LEFT, _lib.AK_TRUNC_LEFT, _lib.AK_DENSE_I64, _lib.AK_PACK_DROP_LAST) == (1, 2, 4, 8)


def test_pad_argument_errors_cpu(L):
    """Every ak_ids_pad error of the header, raised on the host before any device call (the pointers
    here are host memory: nothing may touch them)."""
    ids, offs, out = (C.c_int32 * 8)(), (C.c_uint64 * 3)(0, 4, 8), (C.c_int32 * 64)()

    def pad(ids=ids, offs=offs, n=2, width=8, h=1, t=1, flags=0, out=out):
        return L.ak_ids_pad(ids, offs, n, width, 0, h, t, flags, out, n, None, None, None)

    assert _is_arg_error(L, pad(ids=None))
    assert _is_arg_error(L, pad(offs=None))
    assert _is_arg_error(L, pad(offs=None, n=0))
    assert _is_arg_error(L, pad(out=None))
    assert _is_arg_error(L, pad(width=0, h=0, t=0))
    assert _is_arg_error(L, pad(width=1))            # HF leaves max_length 1 untruncated: refused
    assert _is_arg_error(L, pad(width=4, h=2, t=3))
    assert _is_arg_error(L, pad(width=4, h=0xFFFFFFFF, t=2))  # the sum does not wrap
    assert _is_arg_error(L, pad(flags=DROP_LAST))
    assert _is_arg_error(L, pad(flags=16))
    assert _is_arg_error(L, pad(flags=-1))


def test_pack_argument_errors_cpu(L):
    ids, offs, out = (C.c_int32 * 8)(), (C.c_uint64 * 3)(0, 4, 8), (C.c_int32 * 64)()

    def pack(ids=ids, offs=offs, n=2, block=4, flags=0, out=out):
        return L.ak_ids_pack(ids, offs, n, block, -1, 0, flags, out, None, None, 4, None)

    assert _is_arg_error(L, pack(ids=None))
    assert _is_arg_error(L, pack(offs=None))
    assert _is_arg_error(L, pack(offs=None, n=0))
    assert _is_arg_error(L, pack(out=None))
    assert _is_arg_error(L, pack(block=0))
    assert _is_arg_error(L, pack(flags=PAD_LEFT))
    assert _is_arg_error(L, pack(flags=TRUNC_LEFT))
    assert _is_arg_error(L, pack(flags=16))


def test_empty_calls_are_ok_without_a_device(L):
    """n == 0 and a capacity of 0 store nothing and launch nothing: AK_OK on a machine without a GPU."""
    ids, offs, out = (C.c_int32 * 8)(), (C.c_uint64 * 3)(0, 4, 8), (C.c_int32 * 64)(*([77] * 64))
    assert L.ak_ids_pad(None, offs, 0, 8, 0, 1, 1, 0, out, 5, None, None, None) == 0
    assert L.ak_ids_pad(ids, offs, 2, 8, 0, 1, 1, 0, out, 0, None, None, None) == 0
    assert L.ak_ids_pack(None, offs, 0, 4, 3, 0, 0, out, None, None, 5, None) == 0
    assert L.ak_ids_pack(ids, offs, 2, 4, 3, 0, 0, out, None, None, 0, None) == 0
    assert list(out) == [77] * 64


@pytest.mark.parametrize("block", [1, 7, 2048])
def test_pack_blocks_formula(L, block):
    for n in (0, 1, 5):
        for total in sorted({0, 1, block - 1, block, block + 1}):
            for has_sep in (0, 1):
                n_ids = total - n * has_sep  # the call takes the id count; T adds one separator per row
                if n_ids < 0:
                    continue
                assert L.ak_ids_pack_blocks(n_ids, n, has_sep, block, 0) == -(-total // block)
                assert L.ak_ids_pack_blocks(n_ids, n, has_sep, block, DROP_LAST) == total // block
    assert L.ak_ids_pack_blocks(10, 2, 1, 0, 0) == 0
    assert L.ak_ids_pack_blocks(10_000_000 * 512, 10_000_000, 1, 2048, 0) == -(-10_000_000 * 513 // 2048)


# ------------------------------------------------------------------------------------------ models
def test_bpe_model_special_ids(bpe_model):
    assert (bpe_model.pad_id, bpe_model.eos_id, bpe_model.bos) == (0, 3, 2)
    assert bpe_model.eos_id == bpe_model.eos


def test_spm_model_special_ids(spm_model):
    with open(os.path.join(ROOT, "models", "akshar.vocab"), encoding="utf-8") as f:
        vocab = {line.split("\t")[0]: i for i, line in enumerate(f)}
    assert spm_model.pad_id == vocab.get("<pad>")
    assert spm_model.eos_id == vocab["</s>"] and spm_model.eos_id is not None
    assert spm_model.piece_to_id[b"<s>"] == vocab["<s>"]  # bos: a control piece, never emitted by EncodeAsIds


def test_tiny_model_without_pad_or_eos(tmp_path):
    """A vocabulary without the tokens gives None, not an error."""
    from akshar_amd.models import BPEModel
    j = json.load(open(BPE_PATH, encoding="utf-8"))
    j["added_tokens"] = [a for a in j["added_tokens"] if a["content"] != "<pad>"]
    j["model"]["vocab"] = {k: v for k, v in j["model"]["vocab"].items() if k != "<pad>"}
    p = tmp_path / "nopad.json"
    p.write_text(json.dumps(j), encoding="utf-8")
    m = BPEModel(str(p))
    assert m.pad_id is None and m.eos_id == 3
