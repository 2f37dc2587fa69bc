"""Generate tests/golden/dense_hf.json.gz: HF `tokenizers` truncation + padding on models/akshar.json.

About 300 rows of tests/golden/golden.jsonl.gz (empty strings, one-token rows and every row over 70
ids included). For each row the unpadded, untruncated ids, and for each (max_length, truncation
direction, padding direction) in {2, 3, 6, 64} x {left, right}^2 what
enable_truncation(max_length, direction) + enable_padding(direction, pad_id=0, length=max_length) give:
ids and attention_mask. HF sees the row's normalized text (golden "norm"), as aksharTokenizer.encode
feeds it; "text" is the raw string, for tests that go through the whole pipeline.

Needs the `tokenizers` package (0.22.2 wrote the committed file). max_length = 1 is left out: HF
cannot fit the <s> ... </s> template into it and leaves the row untruncated.

  python tools/gen_golden_dense.py
"""
import gzip
import itertools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden.jsonl.gz")
OUT = os.path.join(ROOT, "tests", "golden", "dense_hf.json.gz")
LENGTHS = (2, 3, 6, 64)
SIDES = ("left", "right")
N_ROWS = 300


def pick(rows):
    """Empty rows, one-token rows, every row over 70 ids, then an even sample of the rest; one row per text."""
    seen, out = set(), []

    def take(cands, k):
        for r in cands:
            if k <= 0:
                break
            if r["text"] not in seen:
                seen.add(r["text"])
                out.append(r)
                k -= 1

    take([{"text": "", "norm": "", "bpe": [2, 3]}], 1)
    take([r for r in rows if len(r["bpe"]) == 2], 4)
    take([r for r in rows if len(r["bpe"]) == 3], 12)
    take([r for r in rows if len(r["bpe"]) > 70], 24)
    take([r for r in rows if len(r["bpe"]) in (4, 5, 6, 7, 8, 63, 64, 65, 66)], 60)
    rest = [r for r in rows if r["text"] not in seen]
    take(rest[::max(1, len(rest) // (N_ROWS - len(out)))], N_ROWS - len(out))
    return out


def main():
    from tokenizers import Tokenizer
    import tokenizers
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as f:
        rows = pick([json.loads(line) for line in f])
    tok = Tokenizer.from_file(os.path.join(ROOT, "models", "akshar.json"))
    tok.no_truncation()
    tok.no_padding()
    raw = [tok.encode(r["norm"]).ids for r in rows]
    assert all(a == r["bpe"] for a, r in zip(raw, rows)), "HF on the normalized text is not the golden encode"
    records = []
    for ml, tdir, pdir in itertools.product(LENGTHS, SIDES, SIDES):
        tok.enable_truncation(max_length=ml, direction=tdir)
        tok.enable_padding(direction=pdir, pad_id=0, pad_token="<pad>", length=ml)
        encs = tok.encode_batch([r["norm"] for r in rows])
        assert all(len(e.ids) == ml for e in encs)
        records.append({"max_length": ml, "truncation_side": tdir, "padding_side": pdir,
                        "ids": [e.ids for e in encs], "attention_mask": [e.attention_mask for e in encs]})
    doc = {"tokenizers": tokenizers.__version__, "model": "models/akshar.json", "pad_id": 0,
           "rows": [{"text": r["text"], "ids": a} for r, a in zip(rows, raw)], "records": records}
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(doc, ensure_ascii=False, separators=(",", ":")).encode("utf-8"))
    lens = [len(a) for a in raw]
    print("%s: %d rows (ids per row %d..%d, %d over 70), %d records, %d bytes"
          % (OUT, len(rows), min(lens), max(lens), sum(n > 70 for n in lens), len(records), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
