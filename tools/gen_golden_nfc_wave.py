#!/usr/bin/env python3
"""Record the REFERENCE's answers for the rows of tests/nfc_wave_rows.py (build container only;
modelled on tools/gen_golden_rows_edges.py).

Imports /root/reference/src read-only and writes data only, one JSON record per distinct valid UTF-8
row of the families and of one period of every uniform list (never the replicas):

  text   the row
  norm   normalize_text(text)                                             normalize.py:117-148
  ak / ak_m   segment_akshars(norm[, matras=True]) as code-point lengths   segment.py:40-125
  sw     detect_code_switches(norm) as [cp length, label]                  segment.py:150-201
  spm    aksharTokenizer(models/akshar.model).encode(text)                 tokenizer.py:167-193
  bpe    aksharTokenizer(models/akshar.json).encode(text)

Invalid rows have no reference answer; the oracle stands in for them in the tests. Output:
tests/golden/nfc_wave_edges.jsonl.gz, the same bytes on every run.
"""
import gzip
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/src")

from akshar.normalize import normalize_text  # noqa: E402
from akshar.segment import segment_akshars, detect_code_switches  # noqa: E402
from akshar.tokenizer import aksharTokenizer  # noqa: E402
from tests import nfc_wave_rows as W  # noqa: E402


def lens(parts):
    return [len(p) for p in parts]


def main():
    spm = aksharTokenizer(model_path=os.path.join(ROOT, "models", "akshar.model"), model_type="sentencepiece")
    bpe = aksharTokenizer(model_path=os.path.join(ROOT, "models", "akshar.json"), model_type="bpe")
    assert spm.model is not None and bpe.model is not None
    out_path = os.path.join(ROOT, "tests", "golden", "nfc_wave_edges.jsonl.gz")
    n = 0
    with open(out_path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as gz:
        for row in W.distinct_valid_rows():
            t = row.decode("utf-8")
            norm = normalize_text(t)
            rec = {"text": t, "norm": norm, "ak": lens(segment_akshars(norm)),
                   "ak_m": lens(segment_akshars(norm, matras=True)),
                   "sw": [[len(s), lab] for s, lab in detect_code_switches(norm)],
                   "spm": spm.encode(t), "bpe": bpe.encode(t)}
            gz.write((json.dumps(rec, ensure_ascii=True) + "\n").encode("ascii"))
            n += 1
    print("wrote", n, "records to", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
