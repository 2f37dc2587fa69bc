#!/usr/bin/env python3
"""Record the REFERENCE's answers for the step-edge rows of tests/rows_edge_rows.py (build container
only; modelled on tools/gen_golden.py).

Imports /root/reference/src read-only and writes data only, one JSON record per valid UTF-8 row:

  set    "rows" (all_rows), "nfc" (nfc_rows) or "spm" (spm_rows)
  i      the row's index in that list
  text   the row
  norm   normalize_text(text)                                             normalize.py:117-148
  ak / ak_m   segment_akshars(norm[, matras=True]) as code-point lengths   segment.py:40-125
  sw     detect_code_switches(norm) as [cp length, label]                  segment.py:150-201
  spm    aksharTokenizer(models/akshar.model).encode(text), set "spm" only tokenizer.py:167-193

The first record is {"meta": ...}: the grapheme cluster break classes (and the count of
Extended_Pictographic chars) among the code points normalize_text's filter keeps, found as
tools/gen_tables.py finds the classes. Invalid rows have no reference answer; the oracle stands in
for them in the tests. Output: tests/golden/rows_edges.jsonl.gz, the same bytes on every run.
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

import regex  # noqa: E402

from akshar.normalize import normalize_text, filter_garbage  # noqa: E402
from akshar.segment import segment_akshars, detect_code_switches  # noqa: E402
from akshar.tokenizer import aksharTokenizer  # noqa: E402
from tests import rows_edge_rows as R  # noqa: E402

GCB_NAMES = ["Other", "CR", "LF", "Control", "Extend", "ZWJ", "Regional_Indicator", "Prepend",
             "SpacingMark", "L", "V", "T", "LV", "LVT"]  # as tools/gen_tables.py


def kept_classes():
    kept = "".join(chr(c) for c in range(0x110000) if not 0xD800 <= c < 0xE000 and filter_garbage(chr(c)))
    names = [n for n in GCB_NAMES[1:] if regex.search(r"\p{Grapheme_Cluster_Break=%s}" % n, kept)]
    other = regex.search(r"\p{Grapheme_Cluster_Break=Other}", kept) is not None
    return {"meta": True, "kept_chars": len(kept), "gcb_kept": (["Other"] if other else []) + names,
            "extpict_kept": len(regex.findall(r"\p{Extended_Pictographic}", kept))}


def lens(parts):
    return [len(p) for p in parts]


def main():
    spm = aksharTokenizer(model_path=os.path.join(ROOT, "models", "akshar.model"), model_type="sentencepiece")
    assert spm.model is not None
    sets = (("rows", R.all_rows()), ("nfc", R.nfc_rows()), ("spm", R.spm_rows()))
    out_path = os.path.join(ROOT, "tests", "golden", "rows_edges.jsonl.gz")
    n = 0
    with open(out_path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as gz:
        gz.write((json.dumps(kept_classes(), ensure_ascii=True) + "\n").encode("ascii"))
        for name, rows in sets:
            for i, row in enumerate(rows):
                if not R.is_valid(row):
                    continue
                t = row.decode("utf-8")
                norm = normalize_text(t)
                rec = {"set": name, "i": i, "text": t, "norm": norm, "ak": lens(segment_akshars(norm)),
                       "ak_m": lens(segment_akshars(norm, matras=True)),
                       "sw": [[len(s), lab] for s, lab in detect_code_switches(norm)]}
                if name == "spm":
                    rec["spm"] = spm.encode(t)
                gz.write((json.dumps(rec, ensure_ascii=True) + "\n").encode("ascii"))
                n += 1
    print("wrote", n, "records to", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
