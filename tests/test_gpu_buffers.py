"""The batch calls' buffer contract (include/akshar.h "Conventions") on the device: WHERE the kernels
read and write, next to tests/test_gpu_parity.py's WHAT they compute.

  A  capacity: every batch entry point through the raw C-ABI with an exact, a short and a zero
     capacity. Every output array (values, out_offs, row_status) is followed by a guard band of
     BUFFER_GUARD sentinel elements inside the same tensor: out_offs[0..n] equal the oracle's whatever
     the capacity, no guard element changes, ak_ws_check stays AK_OK (a caller's short buffer is not
     an engine overflow), the exact capacity gives the oracle's output, and an exact call after a short
     one on the same workspace does too. What lies below a short capacity is not asserted ("incomplete").
  B  engine-level outputs: encode_batch's out= / out_offs= / cap= arguments, success and errors.
  C  input placement: device views at byte offsets 1, 4 and 15 of a larger allocation (no alignment is
     required), and a last row followed by bytes that are not zero (the slack's contents are free).
  D  a side stream: its own workspace, every op, the per-call path; the default stream afterwards.

One 229-row batch (tests.util.buffer_batch) drives every emit path; the reference is always the
oracle (oracle.oracle, oracle.decode_ref), computed once per module. Everything is bit-exact.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import decode_ref
from oracle import oracle as O
from tests.conftest import BPE_PATH, SPM_PATH
from tests.util import (BUFFER_BAD_ROWS, BUFFER_GUARD as G, buffer_batch, buffer_capacities, oracle_bad_rows, pack_rows,
                        rows_ints)

pytestmark = pytest.mark.gpu

S32 = 0x7A7A7A7A               # above any id or code point index, and not STAGE_DEAD (0xFFFFFFFF)
S64 = 0x7A7A7A7A7A7A7A7A
S_TEXT, S_LABEL, S_STATUS = 0xFF, 0x77, 0x77  # 0xFF is no UTF-8 byte; labels are 0, 1, 2, 255; status bits 0 and 2
KINDS = {"text": (torch.uint8, S_TEXT), "label": (torch.uint8, S_LABEL), "u32": (torch.int32, S32)}
FILTER_ELONG = 16 | 4 | 8      # AK_NORM_STAGES | AK_ST_FILTER | AK_ST_ELONG
SMALL_ROWS = ["kal milte hain", "\u0928\u092e\u0938\u094d\u0924\u0947 dost", "aaj ab"]  # the last: a short tile-path row


# ------------------------------------------------------------------------------------------ reference
def _oracle_ops(buf, offs, bpe_model, spm_model):
    """Every op's oracle result for one packed batch, in the engine calls' return order."""
    norm, no = O.normalize_batch(buf, offs, flags=3)
    nb = norm if len(norm) else np.zeros(1, np.uint8)
    return {
        "normalize-3": (norm, no),
        "normalize-0": O.normalize_batch(buf, offs, flags=0),
        "normalize-filter-elong": O.normalize_batch(buf, offs, flags=FILTER_ELONG),
        "segment-3": O.segment_batch(buf, offs, flags=3),
        "segment-3-matras": O.segment_batch(buf, offs, flags=3, matras=True),
        "segment-raw": O.segment_batch(buf, offs, flags=-1),
        "switches-3": O.switches_batch(buf, offs, flags=3),
        # ak_analyze: normalize, then segment / switches of the normalized text (include/akshar.h)
        "analyze-3": (norm, no) + O.segment_batch(nb, no, flags=-1) + O.switches_batch(nb, no, flags=-1),
        "bpe-3": O.OracleBPE(bpe_model).encode_batch(buf, offs),
        "bpe-1": O.OracleBPE(bpe_model).encode_batch(buf, offs, flags=1),
        "spm-3": O.OracleSPM(spm_model).encode_batch(buf, offs),
    }


def _decode_ref(fn, model, rows):
    """Rows of ids and their decoded text, both packed: (ids u32, id_offs, text u8, text_offs)."""
    text = [fn(model, r).encode("utf-8", "surrogatepass") for r in rows]
    ids = np.asarray([x for r in rows for x in r], dtype=np.uint32)
    io = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=io[1:])
    return (ids, io) + pack_rows(text)


@pytest.fixture(scope="module")
def eng():
    from akshar_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.fixture(scope="module")
def host():
    """The batch on the host: rows, packed bytes, u64 offsets."""
    rows = buffer_batch()
    buf, offs = pack_rows(rows)
    return SimpleNamespace(rows=rows, buf=buf, offs=offs, n=len(rows))


@pytest.fixture(scope="module")
def ref(host, bpe_model, spm_model):
    r = _oracle_ops(host.buf, host.offs, bpe_model, spm_model)
    r["spm-3-pooled"] = r["spm-3"]
    r["bad"] = oracle_bad_rows(host.buf, host.offs)
    assert [host.rows[i] for i in np.flatnonzero(r["bad"])] == list(BUFFER_BAD_ROWS)
    r["bpe-decode"] = _decode_ref(decode_ref.bpe_decode, bpe_model, rows_ints(*r["bpe-3"]))
    # SentencePiece: a few byte-piece and <unk> ids after the encoder's own (valid, truncated and split
    # byte runs, <unk> next to a space, a row that is only <unk>), the last on the batch's last row
    m = spm_model
    bid = [int(x) for x in m.byte_ids]
    ws = [i for i, p in enumerate(m.pieces) if p == "\u2581".encode()][0]
    rows = rows_ints(*r["spm-3"])
    rows[0] += [bid[0xE0], bid[0xA4], bid[0x95]]
    rows[5] += [m.unk_id, ws, m.unk_id]
    rows[66] += [m.unk_id]
    rows[70] += [bid[0xF0], bid[0x9F]]
    rows[-1] += [bid[0xC3], 500, bid[0xA9], m.unk_id]
    r["spm-decode"] = _decode_ref(decode_ref.spm_decode, m, rows)
    return r


@pytest.fixture(scope="module")
def small(bpe_model, spm_model):
    """The 3-row batch of the dirty-slack test and its oracle results."""
    buf, offs = pack_rows([t.encode() for t in SMALL_ROWS])
    r = _oracle_ops(buf, offs, bpe_model, spm_model)
    r["spm-3-pooled"] = r["spm-3"]
    return SimpleNamespace(buf=buf, offs=offs, ref=r)


@pytest.fixture(scope="module")
def models(eng, bpe_model, spm_model):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("AK_SPM_POOL_ROWS", "0")  # read at creation: the word pool at this batch size too
        pooled = eng.SPM(spm_model)
    return SimpleNamespace(bpe=eng.BPE(bpe_model), spm=eng.SPM(spm_model), spm_pooled=pooled)


def _place(eng, buf, offs, lead=b"", slack=None):
    """The batch on the device as pack_host sizes it (round_up(nbytes, 16) + 16 bytes), after `lead`
    bytes of the same allocation; the bytes after the last row are zero, or `slack` repeated."""
    nb = int(offs[-1])
    size = (nb + 15) // 16 * 16 + 16
    h = np.zeros(len(lead) + size, dtype=np.uint8)
    h[:len(lead)] = np.frombuffer(lead, dtype=np.uint8)
    h[len(lead):len(lead) + nb] = buf[:nb]
    if slack:
        fill = np.frombuffer(slack * (size // len(slack) + 1), dtype=np.uint8)
        h[len(lead) + nb:] = fill[:size - nb]
    big, go = eng.to_device(h, offs.astype(np.int64))
    return big[len(lead):], go


@pytest.fixture(scope="module")
def gdev(eng, host):
    return _place(eng, host.buf, host.offs)


def _np(t):
    return np.asarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).astype(np.int64)


def _same(got, want, what):
    """Every array of an op's result tuple (values and offsets) equals the oracle's."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = _np(g), _np(w)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        d = np.flatnonzero(g != w)
        assert d.size == 0, (what, k, int(d[0]), g[d[:4]].tolist(), w[d[:4]].tolist())


# ------------------------------------------------------------------------------------------ A: capacity
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class Guarded:
    """A device array of `numel` elements followed by G guard elements, all set to `sentinel`."""

    def __init__(self, numel, dtype, sentinel, dev):
        self.numel, self.sentinel = numel, sentinel
        self.t = torch.full((numel + G,), sentinel, dtype=dtype, device=dev)

    def guard_broken(self):
        return torch.nonzero(self.t[self.numel:] != self.sentinel).flatten()[:4].tolist()

    def head(self, k):
        return _np(self.t[:k])


def _spec(cx, name):
    """One C-ABI op: its output arrays' kinds, which arrays share a capacity (`groups`, one out_offs
    each), the oracle's values and offsets, and the raw call."""
    L, r = cx.L, cx.ref[name]
    inp = (_p(cx.gb), _p(cx.go), cx.n)
    S = SimpleNamespace
    if name.startswith("normalize"):
        flags = {"normalize-3": 3, "normalize-0": 0, "normalize-filter-elong": FILTER_ELONG}[name]
        return S(kinds=["text"], groups=[[0]], want=[r[0]], offs=[r[1]], status=True,
                 call=lambda a, c, oo, st: L.ak_normalize(cx.ws, flags, *inp, _p(a[0]), c[0], _p(oo[0]), _p(st), cx.stream))
    if name.startswith("segment"):
        flags, matras = {"segment-3": (3, 0), "segment-3-matras": (3, 1), "segment-raw": (-1, 0)}[name]
        return S(kinds=["u32"], groups=[[0]], want=[r[0]], offs=[r[1]], status=True,
                 call=lambda a, c, oo, st: L.ak_segment(cx.ws, flags, matras, *inp, _p(a[0]), c[0], _p(oo[0]), _p(st), cx.stream))
    if name == "switches-3":
        return S(kinds=["u32", "label"], groups=[[0, 1]], want=[r[0], r[1]], offs=[r[2]], status=True,
                 call=lambda a, c, oo, st: L.ak_switches(cx.ws, 3, *inp, _p(a[0]), _p(a[1]), c[0], _p(oo[0]), _p(st), cx.stream))
    if name == "analyze-3":
        return S(kinds=["text", "u32", "u32", "label"], groups=[[0], [1], [2, 3]], want=[r[0], r[2], r[4], r[5]],
                 offs=[r[1], r[3], r[6]], status=True,
                 call=lambda a, c, oo, st: L.ak_analyze(cx.ws, 3, 0, *inp, _p(a[0]), c[0], _p(oo[0]), _p(a[1]), c[1], _p(oo[1]),
                                                        _p(a[2]), _p(a[3]), c[2], _p(oo[2]), _p(st), cx.stream))
    if name in ("bpe-3", "bpe-1"):
        flags = int(name[-1])
        return S(kinds=["u32"], groups=[[0]], want=[r[0]], offs=[r[1]], status=True,
                 call=lambda a, c, oo, st: L.ak_bpe_encode(cx.models.bpe.h, cx.ws, flags, *inp, _p(a[0]), c[0], _p(oo[0]), _p(st),
                                                           cx.stream))
    if name in ("spm-3", "spm-3-pooled"):
        h = (cx.models.spm if name == "spm-3" else cx.models.spm_pooled).h
        return S(kinds=["u32"], groups=[[0]], want=[r[0]], offs=[r[1]], status=True,
                 call=lambda a, c, oo, st: L.ak_spm_encode(h, cx.ws, 3, *inp, _p(a[0]), c[0], _p(oo[0]), _p(st), cx.stream))
    assert name in ("bpe-decode", "spm-decode")
    fn, h = (L.ak_bpe_decode, cx.models.bpe.h) if name == "bpe-decode" else (L.ak_spm_decode, cx.models.spm.h)
    dev = cx.gb.device
    ids = torch.from_numpy(r[0].view(np.int32).copy()).to(dev)
    io = torch.from_numpy(r[1].astype(np.int64)).to(dev)
    return S(kinds=["text"], groups=[[0]], want=[r[2]], offs=[r[3]], status=False,
             call=lambda a, c, oo, st: fn(h, cx.ws, _p(ids), _p(io), cx.n, _p(a[0]), c[0], _p(oo[0]), cx.stream))


def _run_caps(cx, sp, caps, what):
    """One raw call with the groups' capacities `caps`, and everything the contract promises of it."""
    dev, n = cx.gb.device, cx.n
    cap_of = {i: caps[g] for g, idx in enumerate(sp.groups) for i in idx}
    arrays = [Guarded(cap_of[i], *KINDS[k], dev) for i, k in enumerate(sp.kinds)]
    oo = [Guarded(n + 1, torch.int64, S64, dev) for _ in sp.groups]
    st = Guarded(n, torch.uint8, S_STATUS, dev)
    rc = sp.call([a.t for a in arrays], caps, [o.t for o in oo], st.t)
    assert rc == 0, (what, cx.L.ak_last_error())
    torch.cuda.synchronize()
    for g, o in enumerate(oo):
        got, want = o.head(n + 1), _np(sp.offs[g])
        d = np.flatnonzero(got != want)
        assert d.size == 0, (what, "out_offs", g, int(d[0]), got[d[:4]].tolist(), want[d[:4]].tolist())
        assert o.guard_broken() == [], (what, "out_offs guard", g)
    for i, a in enumerate(arrays):
        assert a.guard_broken() == [], (what, "store at cap +", a.guard_broken(), "of output array", i)
    assert st.guard_broken() == [], (what, "row_status guard")
    assert cx.L.ak_ws_check(cx.ws) == 0, (what, cx.L.ak_last_error())
    for g, idx in enumerate(sp.groups):
        total = int(sp.offs[g][-1])
        if caps[g] != total:
            continue
        for i in idx:
            got, want = arrays[i].head(total), _np(sp.want[i])
            d = np.flatnonzero(got != want)
            assert d.size == 0, (what, "output array", i, int(d[0]), got[d[:4]].tolist(), want[d[:4]].tolist())
    if sp.status:
        assert np.array_equal(st.head(n), _np(cx.ref["bad"])), (what, "row_status")
    else:
        assert (st.head(n) == S_STATUS).all(), what


A_CASES = [("normalize-3", 1), ("normalize-3", 0), ("normalize-0", 1), ("normalize-filter-elong", 1),
           ("segment-3", 1), ("segment-3", 0), ("segment-3-matras", 1), ("segment-3-matras", 0), ("segment-raw", 1),
           ("switches-3", 1), ("switches-3", 0), ("analyze-3", 1), ("analyze-3", 0),
           ("bpe-3", 1), ("bpe-3", 0), ("bpe-1", 1), ("spm-3", 1), ("spm-3", 0), ("spm-3-pooled", 1),
           ("bpe-decode", 1), ("spm-decode", 1)]


@pytest.mark.parametrize("name,path", A_CASES, ids=["%s-path%d" % c for c in A_CASES])
def test_capacity_and_guard_bands(eng, host, ref, models, gdev, name, path):
    """path 1: the tile kernels and their copy kernels for flags 3; path 0: one lane per row."""
    from akshar_amd import _lib
    gb, go = gdev
    ws = eng.workspace(gb.device.index)
    eng.set_tiling(ws, path)
    cx = SimpleNamespace(L=_lib.lib(), ws=ws, gb=gb, go=go, n=host.n, ref=ref, models=models, stream=eng._stream(gb.device))
    sp = _spec(cx, name)
    exact = [int(o[-1]) for o in sp.offs]
    _run_caps(cx, sp, exact, (name, path, "exact"))
    if name in ("bpe-3", "spm-3") and path == 1:
        # the batch reaches the branches it is built for: fallback rows the tile path finishes (the NFC
        # waves) and rows left to the one-lane pipeline (invalid UTF-8, over the tile buffer, long rows)
        d = eng.fallback_detail(gb.device.index)
        assert d["finished_in_tile_path"] > 0 and d["one_lane"] > 0, d
    for g, idx in enumerate(sp.groups):
        for cap in buffer_capacities(sp.offs[g], sp.kinds[idx[0]] == "text")[1:]:
            caps = list(exact)
            caps[g] = cap
            _run_caps(cx, sp, caps, (name, path, "group", g, "cap", cap, "of", exact[g]))
            _run_caps(cx, sp, exact, (name, path, "exact after group", g, "cap", cap))  # no state left behind


# ------------------------------------------------------------------------------------------ B: engine-level outputs
ENC = [("bpe", "bpe-3", 1), ("bpe", "bpe-3", 0), ("spm", "spm-3", 1), ("spm", "spm-3", 0)]


@pytest.mark.parametrize("which,key,path", ENC)
def test_encode_in_place_exact_size(eng, host, ref, models, gdev, which, key, path):
    gb, go = gdev
    m = getattr(models, which)
    total = int(ref[key][1][-1])
    out = torch.full((total,), S32, dtype=torch.int32, device=gb.device)
    oo = torch.full((host.n + 1,), S64, dtype=torch.int64, device=gb.device)
    ids, o = m.encode_batch(gb, go, path=path, out=out, out_offs=oo)
    assert o is oo and ids.data_ptr() == out.data_ptr() and ids.numel() == total
    _same((out, oo), ref[key], (which, path))


@pytest.mark.parametrize("which,key,path", ENC)
def test_encode_short_out_raises_then_exact_succeeds(eng, host, ref, models, gdev, which, key, path):
    from akshar_amd._lib import AksharError
    gb, go = gdev
    m = getattr(models, which)
    total = int(ref[key][1][-1])
    with pytest.raises(AksharError, match="output buffer too small"):
        m.encode_batch(gb, go, path=path, out=torch.empty(total - 1, dtype=torch.int32, device=gb.device))
    out = torch.full((total,), S32, dtype=torch.int32, device=gb.device)
    _same(m.encode_batch(gb, go, path=path, out=out), ref[key], (which, path))


@pytest.mark.parametrize("which", ["bpe", "spm"])
def test_encode_outputs_rejected_before_any_launch(eng, host, ref, models, gdev, which):
    gb, go = gdev
    m = getattr(models, which)
    dev, n = gb.device, host.n
    total = int(ref[which + "-3"][1][-1])
    oo = torch.full((n + 1,), S64, dtype=torch.int64, device=dev)
    wide = torch.full((2 * total,), S32, dtype=torch.int32, device=dev)
    cases = [
        (TypeError, dict(out=torch.full((total,), S32, dtype=torch.int64, device=dev))),      # wrong dtype
        (TypeError, dict(out=torch.full((total,), S32, dtype=torch.int32))),                  # a CPU tensor
        (TypeError, dict(out=wide[::2])),                                                     # not contiguous
        (TypeError, dict(out=torch.full((total,), S32, dtype=torch.int32, device=dev),
                         out_offs=torch.full((n + 1,), S32, dtype=torch.int32, device=dev))),  # out_offs dtype
        (ValueError, dict(out=torch.full((total,), S32, dtype=torch.int32, device=dev), out_offs=oo[:n])),  # n entries
    ]
    for exc, kw in cases:
        before = {k: t.clone() for k, t in kw.items()}
        with pytest.raises(exc, match="out"):
            m.encode_batch(gb, go, **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(t, before[k]) for k, t in kw.items()), kw
    assert bool((wide == S32).all()) and bool((oo == S64).all())


@pytest.mark.parametrize("which,key,path", ENC)
def test_encode_rerun_branch_from_a_one_element_capacity(eng, ref, models, gdev, which, key, path):
    """cap=1: the first attempt is short, _run reads the total back and runs again with it."""
    gb, go = gdev
    _same(getattr(models, which).encode_batch(gb, go, cap=1, path=path), ref[key], (which, path))


# ------------------------------------------------------------------------------------------ C, D: every op, engine level
def _engine_ops(eng, models, gb, go, path):
    return {
        "normalize-3": eng.normalize_batch(gb, go, flags=3, path=path),
        "normalize-0": eng.normalize_batch(gb, go, flags=0, path=path),
        "normalize-filter-elong": eng.normalize_batch(gb, go, flags=FILTER_ELONG, path=path),
        "segment-3": eng.segment_batch(gb, go, flags=3, path=path),
        "segment-3-matras": eng.segment_batch(gb, go, flags=3, matras=True, path=path),
        "segment-raw": eng.segment_batch(gb, go, flags=eng.AK_RAW, path=path),
        "switches-3": eng.switches_batch(gb, go, flags=3, path=path),
        "analyze-3": eng.analyze_batch(gb, go, flags=3, path=path),
        "bpe-3": models.bpe.encode_batch(gb, go, path=path),
        "bpe-1": models.bpe.encode_batch(gb, go, flags=1, path=path),
        "spm-3": models.spm.encode_batch(gb, go, path=path),
        "spm-3-pooled": models.spm_pooled.encode_batch(gb, go, path=path),
    }


def _check_ops(eng, models, gb, go, want, what):
    for path in (1, 0):
        got = _engine_ops(eng, models, gb, go, path)
        for name, g in got.items():
            _same(g, want[name], what + (name, "path", path))


def _check_decode(eng, models, ref, lead, tail, what):
    """Both decoders on id rows that are a view `lead` elements into a larger tensor of junk ids, with
    `tail` junk ids after the last row."""
    for name, m in (("bpe-decode", models.bpe), ("spm-decode", models.spm)):
        ids, io, text, to = ref[name]
        h = np.full(lead + len(ids) + tail, 7, dtype=np.uint32)  # a small valid id of both vocabularies
        h[lead:lead + len(ids)] = ids
        big = torch.from_numpy(h.view(np.int32)).to(m.dev)
        out, oo = m.decode_batch(big[lead:lead + len(ids)], torch.from_numpy(io.astype(np.int64)).to(m.dev))
        _same((out, oo), (text, to), what + (name,))


@pytest.mark.parametrize("k", [1, 4, 15])
def test_input_as_unaligned_view_of_a_larger_buffer(eng, host, ref, models, k):
    """`in` needs no alignment: the rows start k bytes into an allocation whose first k bytes are the end
    of other text, closing with a dangling lead (E0 A4) that a read from the aligned-down address would
    glue to the first row."""
    junk = ("\u0915\u093c" * 4).encode() + b"\xe0\xa4"
    gb, go = _place(eng, host.buf, host.offs, lead=junk[-k:])
    assert gb.data_ptr() % 16 == k and gb.is_contiguous()
    _check_ops(eng, models, gb, go, ref, ("view", k))
    _check_decode(eng, models, ref, k % 4 or 1, 5, ("view", k))


@pytest.mark.parametrize("fill", ["\u093c".encode(), "\u0301".encode(), b"b", b"\xe0\xa4"],
                         ids=["nukta", "acute", "letter", "lead"])
def test_bytes_after_the_last_row_are_not_read_as_text(eng, host, ref, small, models, fill):
    """The slack after offs[n] may hold anything: a combining mark, a nukta, a letter that would extend
    the last pre-token, a UTF-8 lead. After the 229-row batch (last row: the huge tier, one lane) and
    after a 3-row batch whose last row is a short tile-path row."""
    gb, go = _place(eng, host.buf, host.offs, slack=fill)
    nb = int(host.offs[-1])
    assert gb.numel() == (nb + 15) // 16 * 16 + 16 and int(gb[nb]) == fill[0] and int(gb[-1]) != 0
    _check_ops(eng, models, gb, go, ref, ("slack", fill))
    gb, go = _place(eng, small.buf, small.offs, slack=fill)
    _check_ops(eng, models, gb, go, small.ref, ("slack, 3 rows", fill))
    _check_decode(eng, models, ref, 0, 64, ("slack", fill))


def _single_calls(tokenizers, text):
    """aksharTokenizer.encode(str) per model (the one-kernel per-call path) against the oracle."""
    ob = O.pack([text])
    for tk, orc in tokenizers:
        assert tk.encode(text) == [int(x) for x in orc.encode_batch(*ob)[0]], tk.model_type


def test_side_stream_has_its_own_workspace(eng, host, ref, models, gdev, bpe_model, spm_model):
    """ak_ws is one per stream: engine.workspace keys by (device, current stream). Every op, both
    decoders and the per-call path on a side stream, then the same on the default stream again."""
    gb, go = gdev
    text = host.rows[0].decode()
    from akshar_amd import aksharTokenizer
    tokenizers = ((aksharTokenizer(model_path=BPE_PATH, model_type="bpe"), O.OracleBPE(bpe_model)),
                  (aksharTokenizer(model_path=SPM_PATH, model_type="sentencepiece"), O.OracleSPM(spm_model)))
    ws0 = eng.workspace(gb.device.index)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ws1 = eng.workspace(gb.device.index)
        assert ws1.value != ws0.value
        assert torch.cuda.current_stream().cuda_stream != torch.cuda.default_stream().cuda_stream
        _check_ops(eng, models, gb, go, ref, ("side stream",))
        for name, m, fn, model in (("bpe-decode", models.bpe, decode_ref.bpe_decode, bpe_model),
                                   ("spm-decode", models.spm, decode_ref.spm_decode, spm_model)):
            rows = rows_ints(ref[name][0], ref[name][1])
            assert eng.decode_lists(m, rows) == [fn(model, r) for r in rows], name
        _single_calls(tokenizers, text)
        side.synchronize()
    assert eng.workspace(gb.device.index).value == ws0.value
    _check_ops(eng, models, gb, go, ref, ("default stream again",))
    _single_calls(tokenizers, text)
