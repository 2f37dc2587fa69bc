"""Batch API over device-resident packed rows (the engine's native data layout).

Rows are packed UTF-8 in one uint8 tensor with int64 row offsets (offs[0] == 0), both on the
GPU. Every call returns device tensors: a packed output plus int64 row offsets. Calls are
enqueued on torch's current HIP stream; the capacity check reads out_offs[-1] back (one
stream sync) and re-runs once with the exact size if the first estimate was short.

This is the batched form of the reference's per-string API; the drop-in
per-string classes in tokenizer.py / normalize.py / segment.py are thin wrappers over it.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import AK_NORM_CLEAN, AK_NORM_LOWER, AK_NORM_STAGES, AK_RAW, AK_ST_FILTER, AksharError, check
from .models import BPEModel, SPMModel

_WS = {}


def _device(dev=None):
    if not torch.cuda.is_available():
        raise AksharError("akshar_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device() if dev is None else dev)


def workspace(dev=None):
    d = _device(dev)
    key = (d.index, torch.cuda.current_stream(d).cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        with torch.cuda.device(d):
            h = ctypes.c_void_p()
            check(_lib.lib().ak_ws_create(ctypes.byref(h)), "ak_ws_create")
        ws = h
        _WS[key] = ws
    return ws


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def flags_of(normalize_roman=True, clean_hinglish=True):
    return (AK_NORM_LOWER if normalize_roman else 0) | (AK_NORM_CLEAN if clean_hinglish else 0)


try:  # host plumbing of the list API (csrc/ak_pylist.c): two C loops instead of per-row Python
    from . import _pylist
except ImportError:  # not built: the same results from the Python loops below
    _pylist = None


def id_lists(ids, offs):
    """Host int32 ids + int64 row offsets (numpy) -> list[list[int]]."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    if _pylist is not None:
        return _pylist.split(ids, offs)
    flat, o = ids.tolist(), offs.tolist()
    return [flat[a:b] for a, b in zip(o, o[1:])]


def pack_host(texts):
    """list[str] -> (numpy u8 bytes padded to 16, numpy int64 offsets)."""
    if _pylist is not None:
        buf, offs = _pylist.pack(texts)
        return np.frombuffer(buf, dtype=np.uint8), np.frombuffer(offs, dtype=np.int64)
    enc = [t.encode("utf-8", "surrogatepass") for t in texts]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum([len(e) for e in enc], out=offs[1:])
    raw = b"".join(enc)
    buf = np.zeros(((len(raw) + 15) // 16) * 16 + 16, dtype=np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return buf, offs


def to_device(buf, offs, dev=None):
    d = _device(dev)
    b = torch.from_numpy(np.ascontiguousarray(buf)).to(d, non_blocking=False)
    o = torch.from_numpy(np.ascontiguousarray(offs).astype(np.int64, copy=False)).to(d)
    return b, o


def pack(texts, dev=None):
    """list[str] -> device (bytes uint8, offs int64)."""
    return to_device(*pack_host(texts), dev=dev)


def _check_inputs(buf, offs):
    if buf.dtype != torch.uint8 or offs.dtype != torch.int64:
        raise TypeError("rows must be uint8 bytes with int64 offsets")
    if not (buf.is_cuda and offs.is_cuda):
        raise TypeError("rows must be device tensors")
    if not buf.is_contiguous() or not offs.is_contiguous():
        raise TypeError("rows must be contiguous")
    n = offs.numel() - 1
    if n < 0:
        raise ValueError("offs must have n+1 entries")
    return n


def _check_out(out, out_offs, n, dev):
    """Caller-provided encode outputs: int32 ids and int64 offsets (n + 1), contiguous, on `dev`;
    checked before any launch because the kernels write through them."""
    if out is not None:
        if out.dtype != torch.int32 or out.device != dev or not out.is_contiguous():
            raise TypeError("out must be a contiguous int32 tensor on %s" % dev)
    if out_offs is not None:
        if out_offs.dtype != torch.int64 or out_offs.device != dev or not out_offs.is_contiguous():
            raise TypeError("out_offs must be a contiguous int64 tensor on %s" % dev)
        if out_offs.numel() != n + 1:
            raise ValueError("out_offs must have n + 1 = %d entries, got %d" % (n + 1, out_offs.numel()))


def _decode(fn, h, ids, id_offs):
    if ids.dtype != torch.int32 or id_offs.dtype != torch.int64 or not (ids.is_cuda and id_offs.is_cuda):
        raise TypeError("id rows must be int32 device ids with int64 device offsets")
    ids, id_offs = ids.contiguous(), id_offs.contiguous()
    n = id_offs.numel() - 1
    if n < 0:
        raise ValueError("id_offs must have n+1 entries")
    if ids.numel() == 0:
        ids = torch.zeros(1, dtype=torch.int32, device=ids.device)
    dev = ids.device
    ws = workspace(dev.index)
    cap = 8 * (int(ids.numel()) + n) + 64

    def call(out, c, oo):
        check(fn(h, ws, _ptr(ids), _ptr(id_offs), n, _ptr(out), c, _ptr(oo), _stream(dev)), fn.__name__)

    out, oo, total = _run(call, n, cap, lambda c: torch.empty(max(c, 1), dtype=torch.uint8, device=dev), dev, ws)
    return out[:total], oo


def decode_lists(model, rows, dev=None):
    """list[list[int]] -> list[str] through model.decode_batch on the device."""
    n = len(rows)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    flat = np.fromiter((x for r in rows for x in r), dtype=np.int64, count=int(offs[-1]))
    if (flat < 0).any() or (flat > 0xFFFFFFFF).any():
        raise AksharError("token id out of range")
    d = model.dev
    gi = torch.from_numpy(flat.astype(np.uint32).view(np.int32).copy()).to(d)
    go = torch.from_numpy(offs).to(d)
    out, oo = model.decode_batch(gi, go)
    b = out.cpu().numpy().tobytes()
    o = oo.cpu().numpy()
    return [b[o[i]:o[i + 1]].decode("utf-8", "surrogatepass") for i in range(n)]


_TILING = {}  # workspace handle -> the (path, rows) it was last set to


def set_tiling(ws, path):
    """ak_ws_set_tiling, skipped when the workspace already holds the setting (the per-call path
    runs it on every call)."""
    t = (path, tile_rows())
    if _TILING.get(ws.value) != t:
        check(_lib.lib().ak_ws_set_tiling(ws, t[0], t[1]), "ak_ws_set_tiling")
        _TILING[ws.value] = t


def _encode_host(fn, name, h, dev, raw, flags, cap):
    """One host string -> numpy int32 ids through ak_*_encode_host: a row that fits one tile runs the
    one-kernel path (one launch, the row and its ids in pinned host memory, one synchronize), any
    other the host-staged batch sequence. The per-call Python work is kept to the lookups it needs."""
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _WS.get((dev.index, stream))
    if ws is None:
        ws = workspace(dev.index)
    set_tiling(ws, TILE_PATH)
    out = np.empty(max(cap, 1), dtype=np.int32)
    n = ctypes.c_uint64()
    check(fn(h, ws, flags, raw, len(raw), out.ctypes.data, cap, ctypes.byref(n), ctypes.c_void_p(stream)), name)
    return out[:n.value]


def _run(fn_call, n, cap, make_out, dev, ws, out=None, out_offs=None):
    """Run a capacity-bounded op, re-running once with the exact size if needed. Every row is exact
    at any length (include/akshar.h "Row lengths"); ak_ws_check turns an internal overflow into an
    exception instead of a short row. With a caller-provided `out` (and `out_offs`), the output is
    written in place and a short capacity raises instead of re-running."""
    if out_offs is None:
        out_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    if out is not None:
        fn_call(out, out.numel(), out_offs)
        total = int(out_offs[-1].item())
        if total > out.numel():
            raise AksharError("output buffer too small: %d elements needed, %d given" % (total, out.numel()))
        check(_lib.lib().ak_ws_check(ws), "ak_ws_check")
        return out, out_offs, total
    outs = make_out(cap)
    fn_call(outs, cap, out_offs)
    total = int(out_offs[-1].item())
    if total > cap:
        cap = total
        outs = make_out(cap)
        fn_call(outs, cap, out_offs)
        total = int(out_offs[-1].item())
    check(_lib.lib().ak_ws_check(ws), "ak_ws_check")
    return outs, out_offs, total


def _tiling(ws, path):
    """path 1 = tile-cooperative kernels for flags 3 (default), 0 = the one-lane-per-row kernels."""
    path = TILE_PATH if path is None else path
    set_tiling(ws, path)


def normalize_batch(buf, offs, flags=3, row_status=None, path=None):
    """flags: normalize_text's 0..3, or AK_NORM_STAGES | AK_ST_* for a subset of its steps."""
    n = _check_inputs(buf, offs)
    dev = buf.device
    ws = workspace(dev.index)
    _tiling(ws, path)
    nbytes = int(offs[-1].item()) if n else 0
    filtered = flags & AK_ST_FILTER if flags & AK_NORM_STAGES else flags & AK_NORM_CLEAN
    # filtered text: NFC of the allowlist expands only the precomposed nukta letters (3 -> 6 bytes)
    cap = 2 * nbytes + 64 if filtered else int(_lib.lib().ak_normalize_cap(n, nbytes))

    def call(out, c, oo):
        check(_lib.lib().ak_normalize(ws, flags, _ptr(buf), _ptr(offs), n, _ptr(out), c, _ptr(oo),
                                      _ptr(row_status), _stream(dev)), "ak_normalize")

    out, oo, total = _run(call, n, cap, lambda c: torch.empty(max(c, 1), dtype=torch.uint8, device=dev), dev, ws)
    return out[:total], oo


def segment_batch(buf, offs, flags=3, matras=False, row_status=None, path=None):
    """flags=AK_RAW (-1) segments the raw rows; else normalizes with flags first."""
    n = _check_inputs(buf, offs)
    dev = buf.device
    ws = workspace(dev.index)
    _tiling(ws, path)
    nbytes = int(offs[-1].item()) if n else 0
    cap = int(_lib.lib().ak_segment_cap(n, nbytes))

    def call(out, c, oo):
        check(_lib.lib().ak_segment(ws, flags, int(bool(matras)), _ptr(buf), _ptr(offs), n, _ptr(out), c, _ptr(oo),
                                    _ptr(row_status), _stream(dev)), "ak_segment")

    out, oo, total = _run(call, n, cap, lambda c: torch.empty(max(c, 1), dtype=torch.int32, device=dev), dev, ws)
    return out[:total], oo


def switches_batch(buf, offs, flags=3, row_status=None, path=None):
    n = _check_inputs(buf, offs)
    dev = buf.device
    ws = workspace(dev.index)
    _tiling(ws, path)
    nbytes = int(offs[-1].item()) if n else 0
    cap = int(_lib.lib().ak_segment_cap(n, nbytes))

    def make(c):
        return (torch.empty(max(c, 1), dtype=torch.int32, device=dev),
                torch.empty(max(c, 1), dtype=torch.uint8, device=dev))

    def call(out, c, oo):
        check(_lib.lib().ak_switches(ws, flags, _ptr(buf), _ptr(offs), n, _ptr(out[0]), _ptr(out[1]), c, _ptr(oo),
                                     _ptr(row_status), _stream(dev)), "ak_switches")

    (ends, labels), oo, total = _run(call, n, cap, make, dev, ws)
    return ends[:total], labels[:total], oo


def analyze_batch(buf, offs, flags=3, matras=False, row_status=None, path=None):
    """explain()'s front half in one fused pass (include/akshar.h ak_analyze): returns
    (norm u8, norm_offs, cluster ends i32, cl_offs, run ends i32, run labels u8, run_offs); cluster
    and run ends index the NORMALIZED row's code points, as segment_akshars(norm) /
    detect_code_switches(norm)."""
    n = _check_inputs(buf, offs)
    dev = buf.device
    ws = workspace(dev.index)
    _tiling(ws, path)
    nbytes = int(offs[-1].item()) if n else 0
    L = _lib.lib()
    caps = [2 * nbytes + 64 if flags & AK_NORM_CLEAN else int(L.ak_normalize_cap(n, nbytes)),
            int(L.ak_segment_cap(n, nbytes)), int(L.ak_segment_cap(n, nbytes))]
    oo = [torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(3)]
    for _ in range(2):
        norm = torch.empty(max(caps[0], 1), dtype=torch.uint8, device=dev)
        cl = torch.empty(max(caps[1], 1), dtype=torch.int32, device=dev)
        runs = torch.empty(max(caps[2], 1), dtype=torch.int32, device=dev)
        labels = torch.empty(max(caps[2], 1), dtype=torch.uint8, device=dev)
        check(L.ak_analyze(ws, flags, int(bool(matras)), _ptr(buf), _ptr(offs), n, _ptr(norm), caps[0], _ptr(oo[0]),
                           _ptr(cl), caps[1], _ptr(oo[1]), _ptr(runs), _ptr(labels), caps[2], _ptr(oo[2]),
                           _ptr(row_status), _stream(dev)), "ak_analyze")
        tot = [int(o[-1].item()) for o in oo]
        check(L.ak_ws_check(ws), "ak_ws_check")
        if all(t <= c for t, c in zip(tot, caps)):
            break
        caps = [max(t, c) for t, c in zip(tot, caps)]
    return norm[:tot[0]], oo[0], cl[:tot[1]], oo[1], runs[:tot[2]], labels[:tot[2]], oo[2]


# Kernel choice for every flags-3 op (BPE / SentencePiece encode, normalize, segment, switches,
# analyze): 1 = the tile-cooperative single-pass kernels (default), 0 = one lane per row (the staged
# row kernels). AK_TILE_PATH overrides the default (development aid).
TILE_PATH = int(os.environ.get("AK_TILE_PATH", "1"))


def tile_rows():
    """Rows per tile: tiles pack rows greedily up to their byte buffer, 16 rows at most;
    AK_TILE_ROWS overrides (development aid)."""
    v = os.environ.get("AK_TILE_ROWS")
    return int(v) if v else 16


class BPE:
    """Device-resident HF BPE model (models/akshar.json layout, cli.py:276-299)."""

    def __init__(self, model, dev=None):
        self.model = model if isinstance(model, BPEModel) else BPEModel(model)
        self.dev = _device(dev)
        m = self.model
        h = ctypes.c_void_p()
        merges = np.ascontiguousarray(m.merges, dtype=np.uint32)
        with torch.cuda.device(self.dev):
            check(_lib.lib().ak_bpe_create(len(m.single_cp), m.single_cp.ctypes.data, m.single_id.ctypes.data,
                                           len(merges), merges.ctypes.data, m.bos, m.eos, ctypes.byref(h)),
                  "ak_bpe_create")
        self.h = h
        cps, aoffs, aids = m.added_arrays()
        check(_lib.lib().ak_bpe_set_added(h, len(aids), cps.ctypes.data, aoffs.ctypes.data, aids.ctypes.data),
              "ak_bpe_set_added")
        toks = [m.id_to_token.get(i, "").encode("utf-8", "surrogatepass") for i in range(m.vocab_size)]
        tb = np.frombuffer(b"".join(toks) or b"\0", dtype=np.uint8)
        to = np.zeros(len(toks) + 1, dtype=np.uint64)
        np.cumsum([len(t) for t in toks], out=to[1:])
        sp = np.asarray([1 if (i in m.special_ids or i not in m.id_to_token) else 0 for i in range(m.vocab_size)],
                        dtype=np.uint8)
        check(_lib.lib().ak_bpe_set_vocab(h, len(toks), tb.ctypes.data, to.ctypes.data, sp.ctypes.data),
              "ak_bpe_set_vocab")

    def cache_info(self):
        """The pre-token result cache (include/akshar.h ak_bpe_cache_info): slots, keys found, keys
        stored, merged-token sequences whose merge_all is not one id."""
        info = (ctypes.c_uint64 * 4)()
        check(_lib.lib().ak_bpe_cache_info(self.h, info), "ak_bpe_cache_info")
        return {"slots": info[0], "keys": info[1], "stored": info[2], "multi": info[3]}

    @classmethod
    def load(cls, path, dev=None):
        """The device model read by the library itself (ak_bpe_load: tokenizer.json parsed in C++, as
        a non-Python caller of the C-ABI would load it); `model` still holds the Python reader's
        arrays for the host-side piece strings."""
        self = cls.__new__(cls)
        self.model = BPEModel(path)
        self.dev = _device(dev)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            check(_lib.lib().ak_bpe_load(os.fsencode(path), ctypes.byref(h)), "ak_bpe_load")
        self.h = h
        return self

    def decode_batch(self, ids, id_offs):
        """Device id rows (int32, int64 offsets) -> (uint8 UTF-8 text, int64 row offsets):
        HF Tokenizer.decode per row (tokenizer.py:219), on the device."""
        return _decode(_lib.lib().ak_bpe_decode, self.h, ids, id_offs)

    def encode_host(self, raw, flags=3):
        """One UTF-8 string (bytes) -> numpy int32 ids (ak_bpe_encode_host: the per-call path)."""
        # the library's ids bound for the flags (ak_bpe_encode_host): bytes + 2 with clean_hinglish,
        # 6 x bytes + 2 under HF's full NFKC without it
        mul = 1 if flags & AK_NORM_CLEAN else 6
        return _encode_host(_lib.lib().ak_bpe_encode_host, "ak_bpe_encode_host", self.h, self.dev, raw, flags,
                            mul * len(raw) + 18)

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:  # at interpreter exit the module may already be torn down
            _lib.lib().ak_bpe_free(h)

    def encode_batch(self, buf, offs, flags=3, row_status=None, cap=None, nbytes=None, path=None, out=None,
                     out_offs=None):
        """Device rows -> (int32 ids, int64 row offsets). `out` / `out_offs` (optional, int32 /
        int64 device tensors, the latter n + 1 long) receive the result in place."""
        n = _check_inputs(buf, offs)
        dev = buf.device
        _check_out(out, out_offs, n, dev)
        ws = workspace(dev.index)
        if nbytes is None:
            nbytes = int(offs[-1].item()) if n else 0
        if cap is None:
            cap = nbytes // 2 + 2 * n + 1024
        path = TILE_PATH if path is None else path
        set_tiling(ws, path)

        def call(out, c, oo):
            check(_lib.lib().ak_bpe_encode(self.h, ws, flags, _ptr(buf), _ptr(offs), n, _ptr(out), c, _ptr(oo),
                                           _ptr(row_status), _stream(dev)), "ak_bpe_encode")

        out, oo, total = _run(call, n, cap, lambda c: torch.empty(max(c, 1), dtype=torch.int32, device=dev), dev, ws,
                              out, out_offs)
        return out[:total], oo


class SPM:
    """Device-resident SentencePiece unigram model (cli.py:232-248)."""

    def __init__(self, model, dev=None):
        self.model = model if isinstance(model, SPMModel) else SPMModel(model)
        self.dev = _device(dev)
        m = self.model
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            check(_lib.lib().ak_spm_create(len(m.pieces), m.piece_bytes.ctypes.data, m.piece_offs.ctypes.data,
                                           m.scores.ctypes.data, m.types.ctypes.data, m.unk_id,
                                           m.byte_ids.ctypes.data, ctypes.byref(h)), "ak_spm_create")
        self.h = h

    def encode_host(self, raw, flags=3):
        """One UTF-8 string (bytes) -> numpy int32 ids (ak_spm_encode_host: the per-call path)."""
        return _encode_host(_lib.lib().ak_spm_encode_host, "ak_spm_encode_host", self.h, self.dev, raw, flags,
                            3 * len(raw) + 20)

    def cache_info(self):
        """The word cache (include/akshar.h ak_spm_cache_info): slots, "▁" words found, words
        stored, words whose solution holds an unknown char or more than 6 pieces."""
        info = (ctypes.c_uint64 * 4)()
        check(_lib.lib().ak_spm_cache_info(self.h, info), "ak_spm_cache_info")
        return {"slots": info[0], "words": info[1], "stored": info[2], "skipped": info[3]}

    @classmethod
    def load(cls, path, dev=None):
        """The device model read by the library itself (ak_spm_load: the protobuf parsed in C++)."""
        self = cls.__new__(cls)
        self.model = SPMModel(path)
        self.dev = _device(dev)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            check(_lib.lib().ak_spm_load(os.fsencode(path), ctypes.byref(h)), "ak_spm_load")
        self.h = h
        return self

    def __del__(self):
        h = getattr(self, "h", None)
        if h and _lib is not None:  # at interpreter exit the module may already be torn down
            _lib.lib().ak_spm_free(h)

    def decode_batch(self, ids, id_offs):
        """Device id rows (int32, int64 offsets) -> (uint8 UTF-8 text, int64 row offsets):
        SentencePieceProcessor.DecodeIds per row (tokenizer.py:217), on the device."""
        return _decode(_lib.lib().ak_spm_decode, self.h, ids, id_offs)

    def encode_batch(self, buf, offs, flags=3, row_status=None, cap=None, nbytes=None, out=None, out_offs=None,
                     path=None):
        """Device rows -> (int32 ids, int64 row offsets); `out` / `out_offs` as BPE.encode_batch.
        path 1 = tile-cooperative kernel (flags 3), 0 = the staged row kernel."""
        n = _check_inputs(buf, offs)
        dev = buf.device
        _check_out(out, out_offs, n, dev)
        ws = workspace(dev.index)
        if nbytes is None:
            nbytes = int(offs[-1].item()) if n else 0
        if cap is None:
            cap = nbytes // 2 + 2 * n + 1024
        path = TILE_PATH if path is None else path
        set_tiling(ws, path)

        def call(out, c, oo):
            check(_lib.lib().ak_spm_encode(self.h, ws, flags, _ptr(buf), _ptr(offs), n, _ptr(out), c, _ptr(oo),
                                           _ptr(row_status), _stream(dev)), "ak_spm_encode")

        out, oo, total = _run(call, n, cap, lambda c: torch.empty(max(c, 1), dtype=torch.int32, device=dev), dev, ws,
                              out, out_offs)
        return out[:total], oo


def _check_ids(ids, offs):
    """Ragged id rows as the encode calls return them: int32 ids, int64 offsets (n + 1), contiguous, on
    one device; returns n."""
    if ids.dtype != torch.int32 or offs.dtype != torch.int64:
        raise TypeError("id rows must be int32 ids with int64 offsets")
    if not (ids.is_cuda and offs.is_cuda) or ids.device != offs.device:
        raise TypeError("id rows must be device tensors on one device")
    if not ids.is_contiguous() or not offs.is_contiguous():
        raise TypeError("id rows must be contiguous")
    n = offs.numel() - 1
    if n < 0:
        raise ValueError("offs must have n+1 entries")
    return n


def _check_dense(t, name, dtypes, numel, dev):
    """A caller-provided output of pad_ids: dtype, device, contiguity and size, checked before the
    launch because the kernel writes through it."""
    if t.dtype not in dtypes or t.device != dev or not t.is_contiguous():
        raise TypeError("%s must be a contiguous %s tensor on %s" % (name, " / ".join(str(d) for d in dtypes), dev))
    if t.numel() != numel:
        raise ValueError("%s must have %d elements, got %d" % (name, numel, t.numel()))


def _side(name, v):
    if v not in ("left", "right"):
        raise ValueError("%s must be 'left' or 'right', got %r" % (name, v))
    return v == "left"


def _dense_dtype(dtype):
    if dtype not in (torch.int32, torch.int64):
        raise TypeError("dtype must be torch.int32 or torch.int64")
    return _lib.AK_DENSE_I64 if dtype == torch.int64 else 0


def pad_ids(ids, offs, width, pad_id, *, padding_side="right", truncation_side="right", keep_head=0, keep_tail=0,
            dtype=torch.int32, out=None, mask=None, lengths=None):
    """Ragged device id rows -> (input_ids [n, width], attention_mask bool [n, width], lengths int32 [n])
    on the device, in one launch on the current stream (include/akshar.h ak_ids_pad): rows longer than
    `width` are truncated keeping their first keep_head and last keep_tail ids (a template's special
    tokens) and the first (truncation_side "right") or last ("left") ids between; the others are padded
    with pad_id on padding_side. out / mask / lengths (optional) receive the results in place."""
    n = _check_ids(ids, offs)
    dev = ids.device
    width, keep_head, keep_tail = int(width), int(keep_head), int(keep_tail)
    flags = _dense_dtype(dtype)
    flags |= _lib.AK_PAD_LEFT if _side("padding_side", padding_side) else 0
    flags |= _lib.AK_TRUNC_LEFT if _side("truncation_side", truncation_side) else 0
    if width <= 0:
        raise ValueError("width must be positive")
    if keep_head < 0 or keep_tail < 0 or keep_head + keep_tail > width:
        raise ValueError("keep_head + keep_tail must lie in 0..width")
    if out is not None:
        _check_dense(out, "out", (dtype,), n * width, dev)
    if mask is not None:
        _check_dense(mask, "mask", (torch.bool, torch.uint8), n * width, dev)
    if lengths is not None:
        _check_dense(lengths, "lengths", (torch.int32,), n, dev)
    with torch.cuda.device(dev):
        out = torch.empty((n, width), dtype=dtype, device=dev) if out is None else out
        mask = torch.empty((n, width), dtype=torch.bool, device=dev) if mask is None else mask
        lengths = torch.empty(n, dtype=torch.int32, device=dev) if lengths is None else lengths
        if n:
            src = ids if ids.numel() else torch.zeros(1, dtype=torch.int32, device=dev)  # all rows empty
            check(_lib.lib().ak_ids_pad(_ptr(src), _ptr(offs), n, width, int(pad_id), keep_head, keep_tail, flags,
                                        _ptr(out), n, _ptr(mask), _ptr(lengths), _stream(dev)), "ak_ids_pad")
    return out.view(n, width), mask.view(n, width), lengths


def pack_ids(ids, offs, block, *, sep_id=None, pad_id=0, drop_last=False, dtype=torch.int32, positions=True, docs=True):
    """Ragged device id rows -> (input_ids [n_blocks, block], position_ids | None, doc_ids | None) on the
    device, in one launch on the current stream (include/akshar.h ak_ids_pack): the rows concatenated,
    each followed by sep_id if given, cut into blocks; the last block is padded with pad_id, or dropped
    with drop_last. position_ids restart at every row and count on across blocks, doc_ids hold the row
    index (padding: 0 and -1). `ids` must hold exactly the offs[-1] ids of the rows (as the encode calls
    return them): the block count comes from ids.numel(), with no read-back."""
    n = _check_ids(ids, offs)
    dev = ids.device
    block = int(block)
    if block <= 0:
        raise ValueError("block must be positive")
    if sep_id is not None and int(sep_id) < 0:
        raise ValueError("sep_id must be a token id (or None for no separator)")
    flags = _dense_dtype(dtype) | (_lib.AK_PACK_DROP_LAST if drop_last else 0)
    nb = int(_lib.lib().ak_ids_pack_blocks(ids.numel(), n, int(sep_id is not None), block, flags))
    with torch.cuda.device(dev):
        out = torch.empty((nb, block), dtype=dtype, device=dev)
        pos = torch.empty((nb, block), dtype=torch.int32, device=dev) if positions else None
        doc = torch.empty((nb, block), dtype=torch.int32, device=dev) if docs else None
        if nb:
            src = ids if ids.numel() else torch.zeros(1, dtype=torch.int32, device=dev)  # all rows empty
            check(_lib.lib().ak_ids_pack(_ptr(src), _ptr(offs), n, block, -1 if sep_id is None else int(sep_id),
                                         int(pad_id), flags, _ptr(out), _ptr(pos), _ptr(doc), nb, _stream(dev)),
                  "ak_ids_pack")
    return out, pos, doc


def window_ids(ids, offs, width, pad_id, *, stride=0, keep_head=0, keep_tail=0, fixed=None, fixed_cap=None,
               fixed_last=False, longest_first=False, padding_side="right", dtype=torch.int32, max_windows=None):
    """Ragged device id rows -> sliding windows of `width` ids on the device, on the current stream
    (include/akshar.h ak_ids_window_offs + ak_ids_windows): HF tokenizers' enable_truncation(width, stride)
    with its overflow encodings. A row whose body (the ids between its keep_head and keep_tail template
    ids) does not fit yields further windows that overlap by `stride` body ids, each with the row's head
    and tail ids. fixed = (ids, offs) gives every row a partner row that is repeated in every window: in
    front of the sliding part (HF "only_second"), or behind it with fixed_last ("only_first"); a partner
    longer than fixed_cap is cut to it as pad_ids truncates (None: width - keep_head - keep_tail -
    stride - 1, the largest legal value, so it is cut only when it has to be). longest_first (needs
    fixed, stride 0): one window per row, partner then row, the longer body cut first as HF does.
    Returns a dict of device tensors: input_ids [n_windows, width], attention_mask (bool),
    token_type_ids (uint8: 0 on the first segment, 1 on the second), overflow_to_sample_mapping,
    window_start (the window's first body id's index in the row's body), lengths (int32 [n_windows]) and
    win_offs (int64 [n + 1]: the first window of every row). Sizing the outputs costs one 8-byte
    read-back of win_offs[-1]; with max_windows there is none: the outputs have max_windows rows, those
    from win_offs[-1] on are unwritten, and the caller reads win_offs."""
    n = _check_ids(ids, offs)
    dev = ids.device
    width, stride, keep_head, keep_tail = int(width), int(stride), int(keep_head), int(keep_tail)
    flags = _dense_dtype(dtype) | (_lib.AK_PAD_LEFT if _side("padding_side", padding_side) else 0)
    if width <= 0 or stride < 0 or keep_head < 0 or keep_tail < 0:
        raise ValueError("width must be positive; stride, keep_head and keep_tail must not be negative")
    f_ids = f_offs = None
    if fixed is not None:
        f_ids, f_offs = fixed
        if _check_ids(f_ids, f_offs) != n or f_ids.device != dev:
            raise ValueError("fixed must hold one row per row of ids, on the same device")
    elif fixed_cap or fixed_last or longest_first:
        raise ValueError("fixed_cap, fixed_last and longest_first need the fixed rows")
    if longest_first:
        if stride or fixed_last:
            raise ValueError("longest_first takes neither a stride nor fixed_last")
        if width < 2 * (keep_head + keep_tail):
            raise ValueError("width leaves no room for the two rows' template ids")
        flags |= _lib.AK_WIN_LONGEST_FIRST
        fixed_cap = 0
    else:
        room = width - keep_head - keep_tail - stride - 1  # what the fixed row may take at most
        if room < 0:
            raise ValueError("width - keep_head - keep_tail must exceed stride")
        fixed_cap = (room if fixed is not None else 0) if fixed_cap is None else int(fixed_cap)
        if not 0 <= fixed_cap <= room:
            raise ValueError("fixed_cap must lie in 0..%d (width - keep_head - keep_tail - stride - 1)" % room)
        flags |= _lib.AK_WIN_FIXED_LAST if fixed_last else 0
    if max_windows is not None and int(max_windows) < 0:
        raise ValueError("max_windows must not be negative")
    L = _lib.lib()
    with torch.cuda.device(dev):
        win_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        check(L.ak_ids_window_offs(workspace(dev.index), _ptr(offs), _ptr(f_offs), n, width, stride, keep_head, keep_tail,
                                   fixed_cap, flags, _ptr(win_offs), _stream(dev)), "ak_ids_window_offs")
        nw = int(win_offs[-1].item()) if max_windows is None else int(max_windows)
        out = torch.empty((nw, width), dtype=dtype, device=dev)
        mask = torch.empty((nw, width), dtype=torch.bool, device=dev)
        types = torch.empty((nw, width), dtype=torch.uint8, device=dev)
        sample, start, lengths = (torch.empty(nw, dtype=torch.int32, device=dev) for _ in range(3))
        if n and nw:
            one = torch.zeros(1, dtype=torch.int32, device=dev)  # all rows empty: a pointer nothing is read from
            check(L.ak_ids_windows(_ptr(ids if ids.numel() else one), _ptr(offs),
                                   None if fixed is None else _ptr(f_ids if f_ids.numel() else one), _ptr(f_offs), n,
                                   _ptr(win_offs), width, stride, keep_head, keep_tail, fixed_cap, int(pad_id), flags,
                                   _ptr(out), nw, _ptr(mask), _ptr(types), _ptr(sample), _ptr(start), _ptr(lengths),
                                   _stream(dev)), "ak_ids_windows")
    return {"input_ids": out, "attention_mask": mask, "token_type_ids": types, "overflow_to_sample_mapping": sample,
            "window_start": start, "lengths": lengths, "win_offs": win_offs}


def _threshold(name, p):
    """A probability as the 33-bit threshold a 32-bit draw is compared with: min(2^32, round(p 2^32))."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("%s must lie in 0..1, got %r" % (name, p))
    return min(1 << 32, int(round(p * (1 << 32))))


def mask_ids(ids, attention_mask=None, *, mask_id, vocab_range, never=(), mlm_probability=0.15, mask_fraction=0.8,
             random_fraction=0.1, seed=0, stream_id=0, elem_base=0, word_start=None, ignore_index=-100):
    """A device id matrix [rows, width] (int32 or int64, as pad_ids / pack_ids return it) -> (inputs,
    labels) of the same shape and dtype for masked-LM training, in one launch on the current stream
    (include/akshar.h ak_ids_mlm). Every position where attention_mask (optional, bool / uint8) is set
    and whose id is not in `never` (at most 8 ids: pad, bos, eos, ...) is selected with
    mlm_probability; labels hold the id at the selected positions and ignore_index elsewhere; a selected
    input becomes mask_id with mask_fraction, an id drawn evenly from vocab_range = (lo, hi), hi
    excluded, with random_fraction, and stays otherwise. word_start (optional, a device uint8 tensor
    with one entry per vocabulary id, nonzero where the id begins a word) selects whole words: an id
    that begins none shares the selection of the nearest word start to its left.
    The draws are Philox4x32-10 of (seed, stream_id, elem_base + the element's index): the same
    arguments give the same result on every run, whatever torch's generators hold; another stream_id (an
    epoch, a rank) gives an independent draw; elem_base continues a larger batch's numbering."""
    t_select = _threshold("mlm_probability", mlm_probability)
    t_mask = _threshold("mask_fraction", mask_fraction)
    t_random = _threshold("random_fraction", random_fraction)
    if float(mask_fraction) + float(random_fraction) > 1.0:
        raise ValueError("mask_fraction + random_fraction must not exceed 1")
    t_random = min(t_random, (1 << 32) - t_mask)  # the two roundings may add up to 2^32 + 1
    lo, hi = (int(v) for v in vocab_range)
    if not -(1 << 31) <= lo < hi <= (1 << 31) - 1:
        raise ValueError("vocab_range must be (lo, hi) with lo < hi, both int32")
    never = [int(v) for v in never]
    if len(never) > 8:
        raise ValueError("never takes at most 8 ids, got %d" % len(never))
    mask_id, ignore_index = int(mask_id), int(ignore_index)
    for name, v in [("mask_id", mask_id), ("ignore_index", ignore_index)] + [("never", v) for v in never]:
        if not -(1 << 31) <= v < 1 << 31:
            raise ValueError("%s must be int32, got %d" % (name, v))
    for name, v in (("seed", seed), ("stream_id", stream_id), ("elem_base", elem_base)):
        if not 0 <= int(v) < 1 << 64:
            raise ValueError("%s must lie in 0..2^64-1" % name)
    # the tensors (the values above are checked first: they need no device)
    if ids.dim() != 2 or not ids.is_cuda or not ids.is_contiguous():
        raise TypeError("ids must be a contiguous [rows, width] device tensor")
    flags = _dense_dtype(ids.dtype)
    dev = ids.device
    rows, width = ids.shape
    if width <= 0:
        raise ValueError("width must be positive")
    if attention_mask is not None:
        _check_dense(attention_mask, "attention_mask", (torch.bool, torch.uint8), rows * width, dev)
    n_vocab = 0
    if word_start is not None:
        if word_start.dim() != 1 or word_start.numel() == 0:
            raise ValueError("word_start must hold one entry per vocabulary id")
        _check_dense(word_start, "word_start", (torch.uint8, torch.bool), word_start.numel(), dev)
        n_vocab = word_start.numel()
    nev = (ctypes.c_int32 * max(len(never), 1))(*never)
    with torch.cuda.device(dev):
        out, labels = torch.empty_like(ids), torch.empty_like(ids)
        if rows:
            check(_lib.lib().ak_ids_mlm(_ptr(ids), _ptr(attention_mask), rows, width, int(seed), int(stream_id),
                                        int(elem_base), t_select, t_mask, t_random, mask_id, lo, hi, ignore_index,
                                        nev, len(never), _ptr(word_start), n_vocab, flags, _ptr(out), _ptr(labels), rows,
                                        _stream(dev)), "ak_ids_mlm")
    return out, labels


def _span_rates(noise_density, mean_span_length):
    """(density_q32, mean_q16) as ak_ids_spans takes them."""
    density_q32 = _threshold("noise_density", noise_density)
    mean = float(mean_span_length)
    if not 1.0 <= mean < 65536.0:
        raise ValueError("mean_span_length must lie in 1..65535, got %r" % (mean_span_length,))
    return density_q32, min((1 << 32) - 1, int(round(mean * 65536)))


def span_lengths(L, *, noise_density=0.15, mean_span_length=3.0, eos=False):
    """(N, S, in_len, tgt_len) of a row of L ids under span corruption (include/akshar.h
    ak_ids_spans_lengths, host arithmetic): its noise tokens and spans, and the ids its inputs and its
    targets take, the closing eos included if eos."""
    density_q32, mean_q16 = _span_rates(noise_density, mean_span_length)
    if not 0 <= int(L) < 1 << 32:
        raise ValueError("L must lie in 0..2^32-1")
    out = (ctypes.c_uint64 * 4)()
    check(_lib.lib().ak_ids_spans_lengths(int(L), density_q32, mean_q16, int(bool(eos)), out), "ak_ids_spans_lengths")
    return tuple(int(v) for v in out)


def span_raw_length(inputs_length, *, noise_density=0.15, mean_span_length=3.0, eos=False):
    """(L, tgt_len): the longest row, up to the AK_SPANS_MAX_WIDTH ids span_ids takes, whose corrupted
    inputs fit inputs_length ids, and its targets' length (T5's compute_input_and_target_lengths): pack the
    corpus into blocks of L ids and every batch is [n, inputs_length] and [n, tgt_len] without padding."""
    inputs_length = int(inputs_length)
    for L in range(_lib.AK_SPANS_MAX_WIDTH, -1, -1):
        _, _, in_len, tgt_len = span_lengths(L, noise_density=noise_density, mean_span_length=mean_span_length, eos=eos)
        if in_len <= inputs_length:
            return L, tgt_len
    raise ValueError("no row fits inputs_length = %d" % inputs_length)


def span_ids(ids, lengths=None, *, noise_density=0.15, mean_span_length=3.0, sentinel_first, sentinel_step=-1, eos_id=None,
             pad_id, label_pad=-100, in_width=None, tgt_width=None, seed=0, stream_id=0, elem_base=0, noise_mask=False,
             n_sentinels=None):
    """A device id matrix [rows, width] (int32 or int64, as pack_ids / pad_ids return it; width up to
    4096) -> span-corruption batches for encoder-decoder pretraining (T5's objective), in one launch on
    the current stream (include/akshar.h ak_ids_spans). Of the first lengths[r] ids of row r (lengths:
    optional int32 [rows]; None: all) noise_density are noise, in spans of mean_span_length ids on average;
    the counts depend on the length alone, which spans on the draw. Returns a dict of device tensors:
    input_ids [rows, in_width] (the kept ids, every span replaced by one sentinel, then eos_id if given,
    then pad_id), labels [rows, tgt_width] (every sentinel followed by its span, then eos_id, then
    label_pad), input_lengths and label_lengths (int32 [rows]: what each row needs, whatever the widths)
    and, with noise_mask, noise_mask (bool, ids' shape). Span i's sentinel is sentinel_first + i
    sentinel_step: T5's are the last vocabulary ids counting down; sentinel_step 0 shows one id, such as
    <mask>, for every span. n_sentinels (optional): how many sentinel ids the vocabulary reserves;
    ValueError if a full row has more spans. The widths default to what a full row needs
    (span_lengths(width)); a shorter width cuts the rows that need more, a longer one pads.
    The draws are Philox4x32-10 of (seed, stream_id, elem_base + the element's index), as mask_ids':
    reproducible whatever torch's generators hold; elem_base continues a larger batch's numbering."""
    density_q32, mean_q16 = _span_rates(noise_density, mean_span_length)
    if eos_id is not None and int(eos_id) < 0:
        raise ValueError("eos_id must be a token id (or None for no eos)")
    eos = -1 if eos_id is None else int(eos_id)
    sentinel_first, sentinel_step, pad_id, label_pad = int(sentinel_first), int(sentinel_step), int(pad_id), int(label_pad)
    for name, v in (("sentinel_first", sentinel_first), ("sentinel_step", sentinel_step), ("eos_id", eos), ("pad_id", pad_id),
                    ("label_pad", label_pad)):
        if not -(1 << 31) <= v < 1 << 31:
            raise ValueError("%s must be int32, got %d" % (name, v))
    for name, v in (("seed", seed), ("stream_id", stream_id), ("elem_base", elem_base)):
        if not 0 <= int(v) < 1 << 64:
            raise ValueError("%s must lie in 0..2^64-1" % name)
    if ids.dim() != 2:
        raise TypeError("ids must be a contiguous [rows, width] device tensor")
    rows, width = ids.shape
    if not 0 < width <= _lib.AK_SPANS_MAX_WIDTH:
        raise ValueError("width must lie in 1..%d, got %d" % (_lib.AK_SPANS_MAX_WIDTH, width))
    _, S, in_len, tgt_len = span_lengths(width, noise_density=noise_density, mean_span_length=mean_span_length,
                                         eos=eos_id is not None)
    if n_sentinels is not None and S > int(n_sentinels):
        raise ValueError("a row of %d ids has %d spans, more than the %d sentinels" % (width, S, int(n_sentinels)))
    in_width = in_len if in_width is None else int(in_width)
    tgt_width = tgt_len if tgt_width is None else int(tgt_width)
    if in_width <= 0 or tgt_width <= 0:
        raise ValueError("in_width and tgt_width must be positive")
    # the tensors (the values above are checked first: they need no device)
    if not ids.is_cuda or not ids.is_contiguous():
        raise TypeError("ids must be a contiguous [rows, width] device tensor")
    flags = _dense_dtype(ids.dtype)
    dev = ids.device
    if lengths is not None:
        _check_dense(lengths, "lengths", (torch.int32,), rows, dev)
    with torch.cuda.device(dev):
        inputs = torch.empty((rows, in_width), dtype=ids.dtype, device=dev)
        labels = torch.empty((rows, tgt_width), dtype=ids.dtype, device=dev)
        in_lengths, tgt_lengths = (torch.empty(rows, dtype=torch.int32, device=dev) for _ in range(2))
        noise = torch.empty((rows, width), dtype=torch.bool, device=dev) if noise_mask else None
        if rows:
            check(_lib.lib().ak_ids_spans(_ptr(ids), _ptr(lengths), rows, width, int(seed), int(stream_id), int(elem_base),
                                          density_q32, mean_q16, sentinel_first, sentinel_step, eos, pad_id, label_pad, flags,
                                          _ptr(inputs), in_width, _ptr(labels), tgt_width, _ptr(in_lengths),
                                          _ptr(tgt_lengths), _ptr(noise), rows, _stream(dev)), "ak_ids_spans")
    res = {"input_ids": inputs, "labels": labels, "input_lengths": in_lengths, "label_lengths": tgt_lengths}
    if noise_mask:
        res["noise_mask"] = noise
    return res


__all__ = ["pack", "pack_host", "to_device", "normalize_batch", "segment_batch", "switches_batch", "BPE", "SPM",
           "flags_of", "workspace", "AK_RAW", "pad_ids", "pack_ids", "window_ids", "mask_ids", "span_ids", "span_lengths",
           "span_raw_length"]


def profile_enable(on=True, passes=False):
    """on: HIP events around every launch (profile_read); passes: also the tile kernels' per-pass
    clocks (profile_tile_passes), which instrument the kernels themselves — never for timing."""
    _lib.lib().ak_profile_enable((2 if passes else 1) if on else 0)


def profile_reset():
    _lib.lib().ak_profile_reset()


def profile_read():
    """{kernel class: (total device ms, launches)} since the last reset (synchronizes)."""
    res = {}
    for name, k in _lib.AK_PROF.items():
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        check(_lib.lib().ak_profile_read(k, ctypes.byref(ms), ctypes.byref(n)), "ak_profile_read")
        res[name] = (ms.value, n.value)
    return res


def profile_tile_passes(dev=None, raw=False):
    """{pass name: fraction of tile-kernel wave-cycles} since the last call (profiling enabled);
    raw: the wave-cycles themselves."""
    ws = workspace(dev)
    n = len(_lib.AK_TILE_PASSES)
    buf = (ctypes.c_uint64 * n)()
    k = _lib.lib().ak_profile_tile_passes(ws, buf, n)
    if k < 0:
        check(k, "ak_profile_tile_passes")
    if raw:
        return {name: int(buf[i]) for i, name in enumerate(_lib.AK_TILE_PASSES)} if k else {}
    tot = float(sum(buf)) or 1.0
    return {name: round(buf[i] / tot, 4) for i, name in enumerate(_lib.AK_TILE_PASSES)} if k else {}


def profile_tile_counters(dev=None):
    """Event counters of the instrumented tile launches since the last call (include/akshar.h
    ak_profile_tile_counters): pre-token cache probes / hits, merge batches / rounds / lane-rounds."""
    ws = workspace(dev)
    names = ("ptc_probes", "ptc_hits", "merge_batches", "merge_rounds", "merge_lane_rounds")
    buf = (ctypes.c_uint64 * len(names))()
    k = _lib.lib().ak_profile_tile_counters(ws, buf, len(names))
    if k < 0:
        check(k, "ak_profile_tile_counters")
    return {nm: int(buf[i]) for i, nm in enumerate(names[:k])}


def fallback_rows(dev=None):
    """(rows, pool rows) of the last tile-path BPE encode that took the sequential fallback kernels."""
    ws = workspace(dev)
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    check(_lib.lib().ak_ws_fallback_rows(ws, ctypes.byref(a), ctypes.byref(b)), "ak_ws_fallback_rows")
    return a.value, b.value


def fallback_detail(dev=None):
    """The last tile-path encode's fallback rows in detail (include/akshar.h ak_ws_fallback_detail):
    sent off the tile kernel, finished by the tile path after all (BPE: wave NFC; SentencePiece: the
    word pool's send-backs), left to the one-lane row pipeline, needing its slow tier."""
    ws = workspace(dev)
    d = (ctypes.c_uint64 * 4)()
    check(_lib.lib().ak_ws_fallback_detail(ws, d), "ak_ws_fallback_detail")
    return {"rows": d[0], "finished_in_tile_path": d[1], "one_lane": d[2], "slow_tier": d[3]}
