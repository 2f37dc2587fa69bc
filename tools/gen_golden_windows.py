"""Generate tests/golden/windows_hf.json.gz: HF `tokenizers` overflow windows and text pairs on
models/akshar.json, over a subset of the rows of tests/golden/dense_hf.json.gz ("rows": indices into
that file's rows, so texts and plain ids are stored once).

The subset: every row of at most 3 ids (the empty rows, the 2- and 3-id rows), every row over 70 ids
(2,503 to 18,002 ids: thousands of windows per case, which compress well), two rows each of 4, 5 and 6
ids, and an even sample of the rest. For every case the ids of every window (the main encoding,
then its `overflowing` in order) and the main encoding's sequence_ids (-1 for a special token):

  single         enable_truncation(max_length, stride), (max_length, stride) in SINGLE
  only_second    encode(partner, row): the row slides behind a short partner (at most 6 ids with its
  only_first     <s> </s>, so HF never raises "too short"; asserted) / encode(row, partner): the row
                 slides in front of it; (max_length, stride) in PAIR
  longest_first  encode(partner, row), any row as the partner, max_length in LONGEST, stride 0

No padding: a test pads. HF sees the rows' normalized text (golden.jsonl.gz "norm"), as
aksharTokenizer feeds it. Needs the `tokenizers` package (0.22.2 wrote the committed file).

  python tools/gen_golden_windows.py
"""
import gzip
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden.jsonl.gz")
DENSE = os.path.join(ROOT, "tests", "golden", "dense_hf.json.gz")
OUT = os.path.join(ROOT, "tests", "golden", "windows_hf.json.gz")
SINGLE = ((3, 0), (4, 1), (6, 2), (8, 3), (64, 16))
PAIR = ((12, 0), (12, 3), (64, 8))
LONGEST = (4, 5, 6, 16, 64)
N_ROWS = 48


def pick(lens):
    """Positions in dense_hf's rows: all of at most 3 ids, all over 70, two each of 4, 5 and
    6 ids, a sample of the rest."""
    must = [i for i, n in enumerate(lens) if n <= 3 or n > 70]
    must += [[i for i, n in enumerate(lens) if n == k][j] for k in (4, 5, 6) for j in (0, 1)]  # short partners
    rest = [i for i, n in enumerate(lens) if 3 < n <= 70 and i not in must]
    return sorted(must + rest[::max(1, len(rest) // (N_ROWS - len(must)))][:N_ROWS - len(must)])


def windows(enc):
    return [e.ids for e in [enc] + list(enc.overflowing)]


def seq_ids(enc):
    return [-1 if s is None else s for s in enc.sequence_ids]


def main():
    import tokenizers
    from tokenizers import Tokenizer
    with gzip.open(DENSE, "rt", encoding="utf-8") as f:
        dense = json.load(f)["rows"]
    with gzip.open(GOLDEN, "rt", encoding="utf-8") as f:
        norm_of = {r["text"]: r["norm"] for r in map(json.loads, f)}
    norm_of.setdefault("", "")
    rows = pick([len(r["ids"]) for r in dense])
    norms = [norm_of[dense[i]["text"]] for i in rows]
    ids = [dense[i]["ids"] for i in rows]
    tok = Tokenizer.from_file(os.path.join(ROOT, "models", "akshar.json"))
    tok.no_padding()
    tok.no_truncation()
    assert [tok.encode(t).ids for t in norms] == ids, "HF on the normalized text is not the fixture's encode"
    short = [p for p, a in enumerate(ids) if len(a) <= 6]
    assert any(len(ids[p]) == 2 for p in short) and any(len(ids[p]) == 6 for p in short)
    doc = {"tokenizers": tokenizers.__version__, "model": "models/akshar.json", "rows": rows, "single": [], "pairs": [],
           "longest_first": []}
    for ml, stride in SINGLE:
        tok.enable_truncation(max_length=ml, stride=stride)
        encs = [tok.encode(t) for t in norms]
        doc["single"].append({"max_length": ml, "stride": stride, "windows": [windows(e) for e in encs],
                              "seq": [seq_ids(e) for e in encs]})
    for mode in ("only_second", "only_first"):
        for ml, stride in PAIR:
            tok.enable_truncation(max_length=ml, stride=stride, strategy=mode)
            partner = [short[(3 * p + 1) % len(short)] for p in range(len(rows))]
            encs = []
            for t, q in zip(norms, partner):  # an exception here is HF's "sequence too short": none may occur
                encs.append(tok.encode(norms[q], t) if mode == "only_second" else tok.encode(t, norms[q]))
            doc["pairs"].append({"mode": mode, "max_length": ml, "stride": stride, "partner": partner,
                                 "windows": [windows(e) for e in encs], "seq": [seq_ids(e) for e in encs]})
    for ml in LONGEST:
        tok.enable_truncation(max_length=ml, stride=0, strategy="longest_first")
        partner = [(5 * p + 2) % len(rows) for p in range(len(rows))]
        encs = [tok.encode(norms[q], t) for t, q in zip(norms, partner)]
        doc["longest_first"].append({"max_length": ml, "partner": partner, "ids": [e.ids for e in encs],
                                     "seq": [seq_ids(e) for e in encs]})
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode("utf-8"))
    lens = [len(a) for a in ids]
    n_win = sum(len(w) for c in doc["single"] + doc["pairs"] for w in c["windows"])
    print("%s: %d rows (ids per row %d..%d, %d over 70), %d cases, %d windows, %d bytes"
          % (OUT, len(rows), min(lens), max(lens), sum(n > 70 for n in lens),
             len(doc["single"]) + len(doc["pairs"]) + len(doc["longest_first"]), n_win, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
