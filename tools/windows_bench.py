"""Rates of the window kernels (ak_ids_window_offs + ak_ids_windows) next to a same-size device copy.

The cfg4 synthetic Hinglish set (bench.py's generator and seed) at --rows rows (1 M) is encoded once
with the BPE model; then HIP events time, for
  single  width 128, stride 32, keep_head = keep_tail = 1
  pair    width 384, stride 128, every row behind a fixed row of 16 ids (only_second),
  (a) "kernel": engine.window_ids with max_windows (no read-back): the count, the scan and the window
      kernel, allocating all seven outputs; "emit": ak_ids_windows alone (one launch) into preallocated
      outputs, which is how tools/dense_bench.py times ak_ids_pad; "offs": ak_ids_window_offs alone
      (the count and the scan),
  (b) one hipMemcpyAsync device-to-device of exactly the bytes the call writes (the yardstick),
  (c) a straightforward torch composition producing the same tensors (checked equal first).
Each timed window is --inner back-to-back calls between two events; the three are taken in turn
--repeats times after --warmup windows each, and the median window is reported. Rates are bytes
written / time. One JSON document goes to --out (profiles/windows_bench.json).

  python tools/windows_bench.py [--rows 1000000] [--out profiles/windows_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dense_bench import SEED, measure  # noqa: E402

KEYS = ("input_ids", "attention_mask", "token_type_ids", "overflow_to_sample_mapping", "window_start", "lengths", "win_offs")


def torch_windows(ids, offs, width, stride, h, t, pad_id, fixed=None):
    """window_ids(padding right) from index arithmetic; fixed: [n, Lf] ids, rows that need no cut."""
    dev = ids.device
    n = offs.numel() - 1
    lens = offs[1:] - offs[:-1]
    keep = lens >= h + t
    hs, ts = torch.where(keep, h, 0), torch.where(keep, t, 0)
    body = lens - hs - ts
    lf = 0 if fixed is None else fixed.shape[1]
    room = width - lf - hs - ts
    step = room - stride
    nwin = torch.where(body <= room, 1, 1 + (body - room + step - 1) // step)
    win_offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(nwin, 0)])
    sample = torch.repeat_interleave(torch.arange(n, device=dev), nwin)
    start = (torch.arange(sample.numel(), device=dev) - win_offs[sample]) * step[sample]
    nb = torch.minimum(start + room[sample], body[sample]) - start
    hs, ts = hs[sample], ts[sample]
    length = lf + hs + nb + ts
    col = torch.arange(width, device=dev)[None, :]
    j = col - lf
    src = offs[sample][:, None] + j + torch.where(j >= hs[:, None], start[:, None], 0)
    src = src + torch.where(j >= (hs + nb)[:, None], (body[sample] - start - nb)[:, None], 0)
    out = ids[src.clamp(0, ids.numel() - 1)]
    if fixed is not None:
        out = torch.where(col < lf, fixed[sample][:, :width].repeat(1, -(-width // lf))[:, :width], out)
    live = col < length[:, None]
    out = torch.where(live, out, pad_id).to(torch.int32)
    types = (live & (col >= lf)).to(torch.uint8) if fixed is not None else torch.zeros_like(live, dtype=torch.uint8)
    return {"input_ids": out, "attention_mask": live, "token_type_ids": types,
            "overflow_to_sample_mapping": sample.to(torch.int32), "window_start": start.to(torch.int32),
            "lengths": length.to(torch.int32), "win_offs": win_offs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("windows_bench needs a GPU: there is nothing to measure without one")

    from akshar_amd import _lib, engine, synth
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    buf, offs = synth.generate(synth.KIND_HINGLISH, args.rows, seed=SEED)
    nbytes = int(offs[-1])
    host = np.zeros((nbytes + 15) // 16 * 16 + 16, dtype=np.uint8)
    host[:nbytes] = buf
    gb, go = engine.to_device(host, offs.astype(np.int64), dev=0)
    bpe = engine.BPE(os.path.join(ROOT, "models", "akshar.json"), dev=0)
    ids, oo = bpe.encode_batch(gb, go, nbytes=nbytes)
    ids = ids.clone()
    n, pad_id = args.rows, bpe.model.pad_id
    fixed2d = torch.cat([torch.full((n, 1), 2, dtype=torch.int32, device=dev),
                         (torch.arange(n * 14, dtype=torch.int32, device=dev) % 29000 + 4).view(n, 14),
                         torch.full((n, 1), 3, dtype=torch.int32, device=dev)], 1).contiguous()
    f_offs = torch.arange(n + 1, dtype=torch.int64, device=dev) * 16
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    res = {"gpu": torch.cuda.get_device_name(0), "rows": n, "ids": ids.numel(), "input_bytes": nbytes,
           "method": "HIP events around %d back-to-back calls, median of %d windows after %d warm-up windows, "
                     "candidates in turn; rate = bytes written / time. Outputs of this size that are rewritten "
                     "back to back partly stay in the 256 MiB Infinity Cache: these are back-to-back-call rates, "
                     "not HBM rates" % (args.inner, args.repeats, args.warmup), "cases": []}
    for name, width, stride, fixed in (("single", 128, 32, None), ("pair_only_second", 384, 128, fixed2d)):
        kw = dict(stride=stride, keep_head=1, keep_tail=1)
        if fixed is not None:
            kw.update(fixed=(fixed.view(-1), f_offs), fixed_cap=16)
        got = engine.window_ids(ids, oo, width, pad_id, **kw)
        ref = torch_windows(ids, oo, width, stride, 1, 1, pad_id, fixed)
        assert all(torch.equal(got[k], ref[k]) for k in KEYS), "torch composition differs"
        nw = got["input_ids"].shape[0]
        del got, ref
        written = nw * width * 6 + nw * 12 + (n + 1) * 8
        src, dst = (torch.empty(written, dtype=torch.uint8, device=dev) for _ in range(2))
        src.zero_()
        L, buf = _lib.lib(), engine.window_ids(ids, oo, width, pad_id, **kw)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        fixed_ptrs = (ptr(kw["fixed"][0]), ptr(kw["fixed"][1])) if fixed is not None else (None, None)
        cap, ws = kw.get("fixed_cap", 0), engine.workspace(0)

        def emit():
            _lib.check(L.ak_ids_windows(ptr(ids), ptr(oo), *fixed_ptrs, n, ptr(buf["win_offs"]), width, stride, 1, 1, cap, pad_id,
                                        0, ptr(buf["input_ids"]), nw, ptr(buf["attention_mask"]), ptr(buf["token_type_ids"]),
                                        ptr(buf["overflow_to_sample_mapping"]), ptr(buf["window_start"]), ptr(buf["lengths"]),
                                        stream()), "ak_ids_windows")

        def offs_only():
            _lib.check(L.ak_ids_window_offs(ws, ptr(oo), fixed_ptrs[1], n, width, stride, 1, 1, cap, 0, ptr(buf["win_offs"]),
                                            stream()), "ak_ids_window_offs")

        fns = {"emit": emit, "offs": offs_only, "kernel": lambda: engine.window_ids(ids, oo, width, pad_id, max_windows=nw, **kw),
               "torch": lambda: torch_windows(ids, oo, width, stride, 1, 1, pad_id, fixed),
               "copy": lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), written, 3, stream())}  # 3: device to device
        inner = {k: (max(1, args.inner // 10) if k == "torch" else args.inner) for k in fns}
        med, spread = measure(fns, inner, args.warmup, args.repeats)
        case = {"op": "window_ids", "case": name, "width": width, "stride": stride, "n_windows": nw, "bytes_written": written}
        for k in fns:
            case[k] = {"ms": round(med[k], 4), "min_ms": round(spread[k][0], 4), "max_ms": round(spread[k][1], 4),
                       "GB_per_s": round(written / med[k] / 1e6, 1)}
        case["kernel_vs_copy"] = round(med["copy"] / med["kernel"], 3)   # > 1: the kernel is faster than the copy
        case["emit_vs_copy"] = round(med["copy"] / med["emit"], 3)
        case["kernel_vs_torch"] = round(med["torch"] / med["kernel"], 2)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del src, dst, buf
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
