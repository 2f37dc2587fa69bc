"""bench.py --gpus N started with no launcher (the way the driver's N = 1 line is started, with a
larger N): the script runs torch.distributed.run itself as a child process, every rank joins one
process group, and rank 0 prints the JSON line with the world size the group saw. CPU only:
--dry-run stops after the rendezvous (gloo), before any GPU call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus2_without_launcher_starts_two_ranks():
    env = dict(os.environ, AK_BENCH_BACKEND="gloo")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "200000", "--no-cpu",
                        "--dry-run"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["world_size"] == 2 and rec["requested_gpus"] == 2
    assert "launching 2 ranks" in p.stderr


def _ragged(n, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return rng.randint(0, 24000, size=int(offs[-1])).astype(np.int32), offs


def _load(d, suffix=""):
    out = {k: np.load(os.path.join(str(d), k + suffix + ".npy")) for k in ("totals", "rows", "offsets", "ids")}
    assert out["ids"].dtype == np.float32 and all(out[k].dtype == np.float64 for k in ("totals", "rows", "offsets"))
    return out


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """bench.dump_outputs on host tensors: a small output is written whole; one over the row or the
    id budget as a seeded sample of rows (the same rows every call), every sampled row's ids intact."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    ids, offs = _ragged(5000, 1)
    t_ids, t_offs = torch.from_numpy(ids), torch.from_numpy(offs)
    bench.dump_outputs(str(tmp_path / "whole"), t_ids, t_offs)
    w = _load(tmp_path / "whole")
    assert w["totals"].tolist() == [5000, len(ids)]
    assert np.array_equal(w["rows"], np.arange(5000)) and np.array_equal(w["offsets"], offs)
    assert np.array_equal(w["ids"], ids)
    for max_rows, max_ids in ((700, 10 ** 9), (10 ** 9, 1500)):
        monkeypatch.setattr(bench, "DUMP_MAX_ROWS", max_rows)
        monkeypatch.setattr(bench, "DUMP_MAX_IDS", max_ids)
        a, b = tmp_path / ("a%d" % max_rows), tmp_path / ("b%d" % max_rows)
        bench.dump_outputs(str(a), t_ids, t_offs, "_rank1")
        bench.dump_outputs(str(b), t_ids, t_offs, "_rank1")
        s, s2 = _load(a, "_rank1"), _load(b, "_rank1")
        assert all(np.array_equal(s[k], s2[k]) for k in s)
        rows = s["rows"].astype(np.int64)
        assert 0 < len(rows) <= max_rows and len(s["ids"]) <= max_ids and np.all(np.diff(rows) > 0)
        assert len(rows) == 700 or len(s["ids"]) > max_ids - 9  # the budget is used
        assert s["totals"].tolist() == [5000, len(ids)] and len(s["offsets"]) == len(rows) + 1
        so = s["offsets"].astype(np.int64)
        assert so[0] == 0 and so[-1] == len(s["ids"])
        for i, r in enumerate(rows):
            assert np.array_equal(s["ids"][so[i]:so[i + 1]], ids[offs[r]:offs[r + 1]])


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path, bpe_model):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times K steps and runs no side measurement;
    --dump-outputs writes the last step's ids and row offsets, equal to the oracle's on the same rows."""
    from akshar_amd import synth
    from oracle import oracle as O
    rows = 20000
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--rows", str(rows), "--dump-outputs", str(tmp_path / "out")], cwd=ROOT, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "MB/s" and rec["higher_is_better"] is True and rec["dtype"] == "u8" and "metric" in rec
    assert p.stderr.count("enqueued") == 3
    assert rec["cpu_baseline"] is None
    assert not {"cfg5", "other_configs", "end_to_end", "single_call_us"} & set(rec)
    assert "tile_pass_cycle_frac" not in rec["roofline"]
    buf, offs = synth.generate(synth.KIND_HINGLISH, rows, seed=1234, first=0)
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    d = _load(tmp_path / "out")
    assert d["totals"].tolist() == [rows, len(ref)] and np.array_equal(d["rows"], np.arange(rows))
    assert np.array_equal(d["offsets"].astype(np.uint64), ro) and np.array_equal(d["ids"].astype(np.uint32), ref)
