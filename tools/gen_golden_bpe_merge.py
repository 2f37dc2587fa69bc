#!/usr/bin/env python3
"""Record the REFERENCE's answers for the merge-stage rows of tests/bpe_merge_rows.py (build container
only; modelled on tools/gen_golden_rows_edges.py).

Imports /root/reference/src read-only and writes data only (ids, counts and hashes; the rows are
regenerated from the module):

  lists   {list name: [aksharTokenizer(model_path=<deep model>, model_type="bpe").encode(row), ...]}
          for every list of merge_rows(); the deep model is written to a temporary directory by
          deep_bpe_model                                                          tokenizer.py:167-193
  real    {"pairs" / "merges": {"rows": count, "sha256": over the int32 ids of all rows back to back,
          then the int64 row offsets}} for the two exhaustive sets on models/akshar.json

Output: tests/golden/bpe_merge_hf.json.gz, the same bytes on every run.
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference/src")

import numpy as np  # noqa: E402

from akshar.tokenizer import aksharTokenizer  # noqa: E402
from akshar_amd.models import BPEModel  # noqa: E402
from tests import bpe_merge_rows as M  # noqa: E402


def ids_hash(rows_ids):
    """SHA-256 over the int32 ids of all rows back to back, then the int64 row offsets."""
    offs = np.zeros(len(rows_ids) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows_ids], out=offs[1:])
    ids = np.asarray([x for r in rows_ids for x in r], dtype=np.int32)
    return hashlib.sha256(ids.tobytes() + offs.tobytes()).hexdigest()


def main():
    out = {"lists": {}, "real": {}}
    with tempfile.TemporaryDirectory() as d:
        tk = aksharTokenizer(model_path=M.deep_bpe_model(os.path.join(d, "deep.json")), model_type="bpe")
        assert tk.model is not None
        for name, (rows, _, _) in M.merge_rows().items():
            out["lists"][name] = [[int(x) for x in tk.encode(r)] for r in rows]
    path = os.path.join(ROOT, "models", "akshar.json")
    tk = aksharTokenizer(model_path=path, model_type="bpe")
    assert tk.model is not None
    for name, rows in M.real_sets(BPEModel(path)).items():
        ids = [[int(x) for x in tk.encode(" ".join(r))] for r in rows]
        out["real"][name] = {"rows": len(rows), "sha256": ids_hash(ids)}
    out_path = M.GOLDEN
    with open(out_path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as gz:
        gz.write(json.dumps(out, ensure_ascii=True, separators=(",", ":"), sort_keys=True).encode("ascii"))
    print("wrote", sum(len(v) for v in out["lists"].values()), "rows to", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
