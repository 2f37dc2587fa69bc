"""Rate of the span-corruption kernel (ak_ids_spans) next to a same-size device copy and a torch composition.

The cfg4 synthetic Hinglish set (bench.py's generator and seed) at --rows rows (1 M) is encoded once
with the BPE model and packed into full int32 blocks of span_raw_length(--inputs-length = 512) ids (568
at T5's 0.15 / 3.0 with </s>); then HIP events time, in turn,
  (a) "spans": ak_ids_spans on the blocks into preallocated inputs, targets and both length arrays,
  (b) "copy":  one hipMemcpyAsync device-to-device of exactly the bytes a call writes, the yardstick,
  (c) "torch": a torch composition that gives batches of the same distribution (random keys, topk for
               the S - 1 smallest, scatter + cumsum for the part indices, gather / scatter for the
               layout); its draws differ, so it is checked by reassembling rows, not element for element.
Each timed window is --inner back-to-back calls between two events (a tenth as many for torch); the
candidates take turns --repeats times after --warmup windows each, and the median window is reported.
Rates are bytes written / time. One JSON document goes to --out (profiles/spans_bench.json).

  python tools/spans_bench.py [--rows 1000000] [--out profiles/spans_bench.json]
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

DENSITY, MEAN = 0.15, 3.0


def torch_spans(ids, N, S, sentinels, eos_id, pad_id, label_pad):
    """(inputs [rows, M + S + 1], targets [rows, N + S + 1]) of full rows, each with N noise ids in S spans."""
    rows, L = ids.shape
    M, dev = L - N, ids.device
    ones = torch.ones((), dtype=torch.int64, device=dev)

    def composition(P):
        """part index of every item [rows, P], exclusive and inclusive part offsets [rows, S]"""
        cuts = torch.rand((rows, P - 1), device=dev).topk(S - 1, dim=1, largest=False).indices + 1
        part = torch.zeros((rows, P), dtype=torch.int64, device=dev).scatter_(1, cuts, ones.expand_as(cuts)).cumsum(1)
        size = torch.zeros((rows, S), dtype=torch.int64, device=dev).scatter_add_(1, part, ones.expand_as(part))
        end = size.cumsum(1)
        return part, end - size, end

    span, a, _ = composition(N)
    seg, _, b_end = composition(M)
    v, u, i = (torch.arange(n, device=dev)[None, :] for n in (M, N, S))
    inputs = torch.full((rows, M + S + 1), pad_id, dtype=ids.dtype, device=dev)
    inputs.scatter_(1, v + seg, ids.gather(1, v + a.gather(1, seg)))
    inputs.scatter_(1, b_end + i, sentinels.expand(rows, S))
    inputs[:, M + S] = eos_id
    targets = torch.full((rows, N + S + 1), label_pad, dtype=ids.dtype, device=dev)
    targets.scatter_(1, u + span + 1, ids.gather(1, u + b_end.gather(1, span)))
    targets.scatter_(1, a + i, sentinels.expand(rows, S))
    targets[:, N + S] = eos_id
    return inputs, targets


def reassembles(ids, inputs, targets, sentinels, rows=64):
    """the first rows of (inputs, targets), each sentinel replaced by its span, equal ids' rows (eos dropped)"""
    sent = set(sentinels)
    for r in range(min(rows, len(ids))):
        spans, cur = {}, None
        for t in targets[r, :-1].tolist():
            if t in sent:
                cur = t
                spans[cur] = []
            else:
                spans[cur].append(t)
        row = []
        for t in inputs[r, :-1].tolist():
            row += spans[t] if t in sent else [t]
        if row != ids[r].tolist():
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--inputs-length", type=int, default=512)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spans_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spans_bench needs a GPU: there is nothing to measure without one")

    from akshar_amd import _lib, engine, synth
    from akshar_amd.tokenizer import aksharTokenizer
    L = _lib.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda", 0)
    buf, offs = synth.generate(synth.KIND_HINGLISH, args.rows, seed=SEED)
    nbytes = int(offs[-1])
    host = np.zeros((nbytes + 15) // 16 * 16 + 16, dtype=np.uint8)
    host[:nbytes] = buf
    pair = engine.to_device(host, offs.astype(np.int64), dev=0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    tok = aksharTokenizer(os.path.join(ROOT, "models", "akshar.json"), "bpe")
    m = tok.model.model
    block, tgt_len = engine.span_raw_length(args.inputs_length, noise_density=DENSITY, mean_span_length=MEAN, eos=True)
    N, S, in_len, _ = engine.span_lengths(block, noise_density=DENSITY, mean_span_length=MEAN, eos=True)
    ids = tok.encode_blocks(pair, block, drop_last=True)["input_ids"].clone()
    n = ids.shape[0]
    # numbered sentinels above the vocabulary, so that reassembling can tell them from ids
    first = m.vocab_size + S - 1
    sentinels = torch.arange(first, first - S, -1, dtype=torch.int32, device=dev)[None, :]
    density_q32, mean_q16 = engine._span_rates(DENSITY, MEAN)
    inputs = torch.empty((n, in_len), dtype=torch.int32, device=dev)
    targets = torch.empty((n, tgt_len), dtype=torch.int32, device=dev)
    in_lengths, tgt_lengths = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))

    def kernel():
        _lib.check(L.ak_ids_spans(ids.data_ptr(), None, n, block, SEED, 0, 0, density_q32, mean_q16, first, -1, m.eos, m.pad_id,
                                  -100, 0, inputs.data_ptr(), in_len, targets.data_ptr(), tgt_len, in_lengths.data_ptr(),
                                  tgt_lengths.data_ptr(), None, n, stream()), "ak_ids_spans")

    def by_torch():
        return torch_spans(ids, N, S, sentinels, m.eos, m.pad_id, -100)

    written = n * (in_len + tgt_len + 2) * 4
    res = {"gpu": torch.cuda.get_device_name(0), "rows": args.rows, "input_bytes": nbytes, "blocks": n, "block": block,
           "inputs_length": in_len, "targets_length": tgt_len, "noise_tokens_per_block": N, "spans_per_block": S, "noise_density": DENSITY,
           "mean_span_length": MEAN, "bytes_written": written, "bytes_read": n * block * 4,
           "method": "HIP events around %d back-to-back calls (torch: %d), median of %d windows after %d warm-up windows, "
                     "candidates in turn; rate = bytes written / time" % (args.inner, max(1, args.inner // 10), args.repeats,
                                                                         args.warmup)}
    # what each candidate produces, before any timing
    kernel()
    torch.cuda.synchronize()
    host_ids = ids[:64].cpu().numpy()
    sent = sentinels[0].tolist()
    res["spans_reassembles"] = reassembles(host_ids, inputs[:64].cpu().numpy(), targets[:64].cpu().numpy(), sent)
    t_in, t_tgt = by_torch()
    res["torch_reassembles"] = reassembles(host_ids, t_in[:64].cpu().numpy(), t_tgt[:64].cpu().numpy(), sent)
    res["lengths_ok"] = bool((in_lengths == in_len).all() and (tgt_lengths == tgt_len).all())
    del t_in, t_tgt
    src, dst = (torch.empty(written, dtype=torch.uint8, device=dev) for _ in range(2))
    src.zero_()
    fns = {"spans": kernel,
           "copy": lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), written, 3, stream()),  # 3: device to device
           "torch": by_torch}
    inner = {k: (max(1, args.inner // 10) if k == "torch" else args.inner) for k in fns}
    med, spread = measure(fns, inner, args.warmup, args.repeats)
    for k in fns:
        res[k] = {"ms": round(med[k], 4), "min_ms": round(spread[k][0], 4), "max_ms": round(spread[k][1], 4),
                  "GB_per_s": round(written / med[k] / 1e6, 1)}
    res["spans_vs_copy"] = round(med["copy"] / med["spans"], 3)  # > 1: the kernel is faster than the copy
    res["spans_vs_torch"] = round(med["torch"] / med["spans"], 2)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
