"""Rate of the masked-LM kernel (ak_ids_mlm) next to a same-size device copy and a torch composition.

The cfg4 synthetic Hinglish set (bench.py's generator and seed) at --rows rows (1 M) is encoded once
with each model and padded to --width (128); then HIP events time, in turn,
  (a) "token":      ak_ids_mlm on the BPE batch, p = 0.15, 0.8 / 0.1 / 0.1, into preallocated outputs,
  (b) "whole_word": ak_ids_mlm with word_start on the SentencePiece batch,
  (c) "copy":       one hipMemcpyAsync device-to-device of exactly the bytes a call writes (inputs +
                    labels), the yardstick,
  (d) "torch":      the straightforward torch composition giving tensors of the same distribution
                    (rand / isin / where / randint on the BPE batch; its draws differ, so it is checked
                    by its shares, not element for element).
Each timed window is --inner back-to-back calls between two events (a tenth as many for torch); the
candidates take turns --repeats times after --warmup windows each, and the median window is
reported. Rates are bytes written / time. One JSON document goes to --out (profiles/mlm_bench.json).

  python tools/mlm_bench.py [--rows 1000000] [--out profiles/mlm_bench.json]
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

P, P_MASK, P_RANDOM = 0.15, 0.8, 0.1


def torch_mlm(ids, mask, never, mask_id, vocab):
    elig = mask & ~torch.isin(ids, never)
    sel = (torch.rand(ids.shape, device=ids.device) < P) & elig
    labels = torch.where(sel, ids, -100)
    u = torch.rand(ids.shape, device=ids.device)
    rnd = torch.randint(0, vocab, ids.shape, dtype=ids.dtype, device=ids.device)
    out = torch.where(sel & (u < P_MASK), mask_id, torch.where(sel & (u < P_MASK + P_RANDOM), rnd, ids))
    return out, labels


def shares(ids, out, labels, mask_id):
    sel = labels != -100
    n_sel = int(sel.sum())
    masked = int(((out == mask_id) & sel).sum())
    kept = int(((out == ids) & sel).sum())
    return {"selected": n_sel, "masked_share": round(masked / max(n_sel, 1), 4), "kept_share": round(kept / max(n_sel, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mlm_bench needs a GPU: there is nothing to measure without one")

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
    n, width = args.rows, args.width
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    batches = {}
    for name, path, kind in (("token", "akshar.json", "bpe"), ("whole_word", "akshar.model", "sentencepiece")):
        tok = aksharTokenizer(os.path.join(ROOT, "models", path), kind)
        m = tok.model.model
        pad = m.pad_id if m.pad_id is not None else m.unk_id
        enc = tok.encode_padded(pair, width, pad_id=pad)
        special = (pad, m.unk_token_id, m.bos, m.eos, m.mask_id) if kind == "bpe" else (pad, m.unk_id, m.bos_id, m.eos_id, m.mask_id)
        never = sorted({int(v) for v in special if v is not None})
        batches[name] = {"ids": enc["input_ids"].clone(), "mask": enc["attention_mask"].clone(), "never": never,
                         "mask_id": m.mask_id, "vocab": m.vocab_size, "ids_total": int(enc["lengths"].sum()),
                         "word_start": tok._word_start(dev) if name == "whole_word" else None}
        del enc
    out = torch.empty((n, width), dtype=torch.int32, device=dev)
    labels = torch.empty((n, width), dtype=torch.int32, device=dev)
    t_select, t_mask, t_random = (engine._threshold("p", p) for p in (P, P_MASK, P_RANDOM))

    def kernel(b):
        nev = (ctypes.c_int32 * 8)(*b["never"])
        ws = b["word_start"]

        def call():
            _lib.check(L.ak_ids_mlm(b["ids"].data_ptr(), b["mask"].data_ptr(), n, width, SEED, 0, 0, t_select, t_mask, t_random,
                                    b["mask_id"], 0, b["vocab"], -100, nev, len(b["never"]),
                                    ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, 0,
                                    out.data_ptr(), labels.data_ptr(), n, stream()), "ak_ids_mlm")
        return call

    written = 2 * n * width * 4
    res = {"gpu": torch.cuda.get_device_name(0), "rows": n, "width": width, "input_bytes": nbytes, "bytes_written": written,
           "mlm_probability": P, "mask_fraction": P_MASK, "random_fraction": P_RANDOM,
           "method": "HIP events around %d back-to-back calls (torch: %d), median of %d windows after %d warm-up windows, "
                     "candidates in turn; rate = bytes written / time" % (args.inner, max(1, args.inner // 10), args.repeats,
                                                                         args.warmup),
           "batches": {}}
    # what each candidate produces, before any timing
    for name, b in batches.items():
        kernel(b)()
        torch.cuda.synchronize()
        res["batches"][name] = {"ids": b["ids_total"], "eligible_share": round(b["ids_total"] / (n * width), 4),
                                **shares(b["ids"], out, labels, b["mask_id"])}
    tb = batches["token"]
    never_t = torch.tensor(tb["never"], dtype=torch.int32, device=dev)
    t_out, t_lab = torch_mlm(tb["ids"], tb["mask"], never_t, tb["mask_id"], tb["vocab"])
    res["batches"]["torch"] = shares(tb["ids"], t_out, t_lab, tb["mask_id"])
    del t_out, t_lab
    src, dst = (torch.empty(written, dtype=torch.uint8, device=dev) for _ in range(2))
    src.zero_()
    fns = {"token": kernel(batches["token"]), "whole_word": kernel(batches["whole_word"]),
           "copy": lambda: hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), written, 3, stream()),  # 3: device to device
           "torch": lambda: torch_mlm(tb["ids"], tb["mask"], never_t, tb["mask_id"], tb["vocab"])}
    inner = {k: (max(1, args.inner // 10) if k == "torch" else args.inner) for k in fns}
    med, spread = measure(fns, inner, args.warmup, args.repeats)
    for k in fns:
        res[k] = {"ms": round(med[k], 4), "min_ms": round(spread[k][0], 4), "max_ms": round(spread[k][1], 4),
                  "GB_per_s": round(written / med[k] / 1e6, 1)}
    res["token_vs_copy"] = round(med["copy"] / med["token"], 3)  # > 1: the kernel is faster than the copy
    res["whole_word_vs_copy"] = round(med["copy"] / med["whole_word"], 3)
    res["token_vs_torch"] = round(med["torch"] / med["token"], 2)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
