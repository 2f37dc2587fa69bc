"""Rates of the dense-output kernels (ak_ids_pad, ak_ids_pack) next to a same-size device copy.

The cfg4 synthetic Hinglish set (bench.py's generator and seed) at --rows rows (1 M) is encoded once
with the BPE model; then, for width in {32, 128} and block 2048, HIP events time
  (a) ak_ids_pad with mask and lengths (keep_head = keep_tail = 1, the BPE template),
  (b) ak_ids_pack with pos and doc,
  (c) one hipMemcpyAsync device-to-device of exactly the bytes the call writes (the yardstick),
  (d) a straightforward torch composition producing the same tensors (checked equal first).
Each timed window is --inner back-to-back calls between two events; the four are taken in turn
--repeats times after --warmup windows each, and the median window is reported. Rates are bytes
written / time. One JSON document goes to --out (profiles/dense_bench.json).

  python tools/dense_bench.py [--rows 1000000] [--out profiles/dense_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 1234  # bench.py's


def torch_pad(ids, offs, width, pad_id, h, t):
    """pad_ids(padding right, truncation right) from index arithmetic."""
    lens = offs[1:] - offs[:-1]
    col = torch.arange(width, device=ids.device)[None, :]
    kept = lens.clamp(max=width)
    mask = col < kept[:, None]
    src = offs[:-1, None] + col
    tail = (lens > width)[:, None] & (col >= width - t)
    src = torch.where(tail, offs[1:, None] - (width - col), src)
    out = torch.where(mask, ids[src.clamp(max=ids.numel() - 1)], pad_id).to(torch.int32)
    return out, mask, kept.to(torch.int32)


def torch_pack(ids, offs, block, pad_id):
    """pack_ids(no separator, last block padded) from index arithmetic."""
    total = ids.numel()
    nb = -(-total // block)
    p = torch.arange(nb * block, device=ids.device)
    live = p < total
    row = torch.searchsorted(offs, p, right=True) - 1
    row = torch.where(live, row, 0)
    out = torch.where(live, ids[p.clamp(max=total - 1)], pad_id).to(torch.int32)
    pos = torch.where(live, p - offs[row], 0).to(torch.int32)
    doc = torch.where(live, row, -1).to(torch.int32)
    return out.view(nb, block), pos.view(nb, block), doc.view(nb, block)


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(fns, inner, warmup, repeats):
    """{name: median ms per call}; the candidates take turns, so drift hits all alike."""
    for name, fn in fns.items():
        for _ in range(warmup):
            window(fn, inner[name])
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            times[name].append(window(fn, inner[name]))
    return {name: statistics.median(v) for name, v in times.items()}, {name: (min(v), max(v)) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dense_bench needs a GPU: there is nothing to measure without one")

    from akshar_amd import engine, synth
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
    n, n_ids, pad_id = args.rows, ids.numel(), bpe.model.pad_id
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    res = {"gpu": torch.cuda.get_device_name(0), "rows": n, "ids": n_ids, "input_bytes": nbytes,
           "method": "HIP events around %d back-to-back calls, median of %d windows after %d warm-up windows, "
                     "candidates in turn; rate = bytes written / time" % (args.inner, args.repeats, args.warmup),
           "cases": []}

    def add(name, shape, written, fns, slow):
        src, dst = (torch.empty(written, dtype=torch.uint8, device=dev) for _ in range(2))
        src.zero_()
        fns = dict(fns)
        fns["copy"] = lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), written, 3, stream())  # 3: device to device
        inner = {k: (max(1, args.inner // 10) if k == slow else args.inner) for k in fns}
        med, spread = measure(fns, inner, args.warmup, args.repeats)
        case = {"op": name, **shape, "bytes_written": written}
        for k in fns:
            case[k] = {"ms": round(med[k], 4), "min_ms": round(spread[k][0], 4), "max_ms": round(spread[k][1], 4),
                       "GB_per_s": round(written / med[k] / 1e6, 1)}
        case["kernel_vs_copy"] = round(med["copy"] / med["kernel"], 3)   # > 1: the kernel is faster than the copy
        case["kernel_vs_torch"] = round(med["torch"] / med["kernel"], 2)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)

    for width in (32, 128):
        out = torch.empty((n, width), dtype=torch.int32, device=dev)
        mask = torch.empty((n, width), dtype=torch.bool, device=dev)
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        engine.pad_ids(ids, oo, width, pad_id, keep_head=1, keep_tail=1, out=out, mask=mask, lengths=lengths)
        ref = torch_pad(ids, oo, width, pad_id, 1, 1)
        assert all(torch.equal(a, b) for a, b in zip((out, mask, lengths), ref)), "torch composition differs"
        del ref
        add("ak_ids_pad", {"width": width}, n * width * 5 + n * 4,
            {"kernel": lambda: engine.pad_ids(ids, oo, width, pad_id, keep_head=1, keep_tail=1, out=out, mask=mask,
                                              lengths=lengths),
             "torch": lambda: torch_pad(ids, oo, width, pad_id, 1, 1)}, "torch")
        del out, mask, lengths
    block = 2048
    got = engine.pack_ids(ids, oo, block, pad_id=pad_id)
    ref = torch_pack(ids, oo, block, pad_id)
    assert all(torch.equal(a, b) for a, b in zip(got, ref)), "torch composition differs"
    nb = got[0].shape[0]
    del got, ref
    add("ak_ids_pack", {"block": block, "n_blocks": nb}, nb * block * 12,
        {"kernel": lambda: engine.pack_ids(ids, oo, block, pad_id=pad_id),
         "torch": lambda: torch_pack(ids, oo, block, pad_id)}, "torch")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
