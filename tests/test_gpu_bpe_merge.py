"""The BPE tile kernel's merge stage on the device (tests/test_emu_bpe_merge.py is the host mirror): the
deep-merge model and row lists of tests/bpe_merge_rows.py, bit-equal to the reference's recorded ids
(tests/golden/bpe_merge_hf.json.gz) on the tile path and the one-lane path with the pre-token cache at
its default, off (AK_PTC=0) and forced into 4 slots (AK_PTC_BITS=2); the fallback waves, the rows over
the tile buffer and the per-call path on the same words; the kernel's counters against the numbers
counted from the row lists; and the two exhaustive sets of models/akshar.json against the oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import bpe_merge_rows as M

pytestmark = pytest.mark.gpu
REP = 8   # the lists' 2,821 rows, 8 times: 353 units, so many waves and the unit queue see them
CACHE = [None, "off", "bits2"]


@pytest.fixture(scope="module")
def eng():
    from akshar_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    from akshar_amd.models import BPEModel
    return BPEModel(M.deep_bpe_model(tmp_path_factory.mktemp("deep") / "deep.json"))


@pytest.fixture(scope="module")
def lists():
    return M.merge_rows()


@pytest.fixture(scope="module")
def gold():
    return M.golden()["lists"]


def _want(gold_rows, rep=1):
    ids = np.asarray([x for r in gold_rows for x in r], dtype=np.int64)
    oo = np.zeros(rep * len(gold_rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in gold_rows] * rep, out=oo[1:])
    return np.tile(ids, rep), oo


def _cpu(t):
    return t.cpu().numpy().astype(np.int64)


def _same(ids, oo, want):
    wi, wo = want
    assert np.array_equal(_cpu(oo), wo)
    d = np.flatnonzero(_cpu(ids) != wi)
    assert d.size == 0, (int(d[0]), int(np.searchsorted(wo, d[0], side="right")) - 1)


def _model(eng, deep, monkeypatch, cache):
    """The device model under a cache setting (read when the model is built), loaded for the tile path."""
    monkeypatch.delenv("AK_PTC", raising=False)
    monkeypatch.delenv("AK_PTC_BITS", raising=False)
    monkeypatch.delenv("AK_TILE_ROWS", raising=False)
    if cache == "off":
        monkeypatch.setenv("AK_PTC", "0")
    elif cache == "bits2":
        monkeypatch.setenv("AK_PTC_BITS", "2")
    m = eng.BPE(deep)
    info = m.cache_info()
    assert info["slots"] == {None: 1024, "off": 0, "bits2": 4}[cache]
    if cache is None:
        assert info["stored"] == info["keys"] == 65 and info["multi"] == 2
    return m


def _counted(eng, fn):
    """fn() under the instrumented tile kernel -> its event counters."""
    eng.profile_enable(True, passes=True)
    try:
        eng.profile_tile_counters()  # reset
        res = fn()
        torch.cuda.synchronize()
        return res, eng.profile_tile_counters()
    finally:
        eng.profile_enable(False)


@pytest.mark.parametrize("cache", CACHE)
def test_every_list_on_both_paths(eng, deep, lists, gold, monkeypatch, cache):
    """All lists in one batch, repeated: the tile path (with its counters: a model that did not load
    for the tile path would show no probes) and the one-lane path."""
    m = _model(eng, deep, monkeypatch, cache)
    names = sorted(lists)
    rows = [r for n in names for r in lists[n][0]] * REP
    want = _want([g for n in names for g in gold[n]], REP)
    gb, go = eng.pack(rows)
    (ids, oo), ctr = _counted(eng, lambda: m.encode_batch(gb, go, path=1))
    _same(ids, oo, want)
    fb = sum(M.expected_counters(*lists[n][:2])["fallback"] for n in names) + len(lists["nfc"][0])
    assert eng.fallback_rows()[0] == REP * fb
    if cache == "off":
        assert ctr.get("ptc_probes", 0) == 0
    else:
        assert ctr["ptc_probes"] > 0 and ctr["merge_lane_rounds"] > 0
    ids0, oo0 = m.encode_batch(gb, go, path=0)
    _same(ids0, oo0, want)


def test_counters_equal_the_row_lists(eng, deep, lists, gold, monkeypatch):
    """The lists that stay in the tile kernel, repeated, with the default table: probes, hits and pool
    lane-rounds do not depend on which wave takes which unit, so they equal the lists' numbers; the
    batches are at least ceil(misses / 64)."""
    m = _model(eng, deep, monkeypatch, None)
    rows = [r for n in M.TILE_LISTS for r in lists[n][0]] * REP
    want = _want([g for n in M.TILE_LISTS for g in gold[n]], REP)
    gb, go = eng.pack(rows)
    (ids, oo), ctr = _counted(eng, lambda: m.encode_batch(gb, go, path=1))
    _same(ids, oo, want)
    exp = [M.expected_counters(*lists[n][:2]) for n in M.TILE_LISTS]
    tot = {k: REP * sum(e[k] for e in exp) for k in exp[0]}
    assert (ctr["ptc_probes"], ctr["ptc_hits"], ctr["merge_lane_rounds"]) == (tot["probes"], tot["hits"], tot["lane_rounds"])
    assert ctr["merge_batches"] >= -(-tot["misses"] // 64)
    assert eng.fallback_rows()[0] == tot["fallback"] == REP


@pytest.mark.parametrize("name", [n for n in M.TILE_LISTS if n.startswith(("pool", "maxn", "ring"))])
def test_single_unit_batches(eng, deep, lists, gold, monkeypatch, name):
    """At most 64 rows: one unit, so one wave owns the batch and its pool: exactly ceil(misses / 64)
    batches (63 | 64 | 65, 127 | 128 | 129; the ring list wraps the wave's ring inside the unit)."""
    m = _model(eng, deep, monkeypatch, None)
    rows, info, _ = lists[name]
    assert len(rows) <= M.UNIT
    exp = M.expected_counters(rows, info)
    gb, go = eng.pack(rows)
    (ids, oo), ctr = _counted(eng, lambda: m.encode_batch(gb, go, path=1))
    _same(ids, oo, _want(gold[name]))
    assert (ctr["ptc_probes"], ctr["ptc_hits"], ctr["merge_lane_rounds"]) == (exp["probes"], exp["hits"], exp["lane_rounds"])
    assert ctr["merge_batches"] == -(-exp["misses"] // 64)
    assert eng.fallback_rows()[0] == 0


@pytest.mark.parametrize("cache", CACHE)
def test_other_paths(eng, deep, lists, gold, monkeypatch, cache):
    """Rows NFC changes (the fallback waves' tile), rows over 768 bytes (the one-lane kernel's own merge
    loop), and the per-call path (encode_host), on the same words."""
    m = _model(eng, deep, monkeypatch, cache)
    for kind in ("nfc", "over"):
        rows = lists[kind][0]
        ids, oo = m.encode_batch(*eng.pack(rows * 4), path=1)
        _same(ids, oo, _want(gold[kind], 4))
        fb = eng.fallback_rows()[0]
        d = eng.fallback_detail()
        assert fb == 4 * len(rows)
        assert d["finished_in_tile_path"] == (fb if kind == "nfc" else 0)
    for r, g in zip(lists["host"][0][:100], gold["host"]):
        assert m.encode_host(r.encode()).tolist() == g


def test_exact_out_buffer_after_a_short_miss(eng, deep, lists, gold, monkeypatch):
    """The placement list ends in a 2-symbol miss: the ids at the exact capacity, a guard band behind."""
    from tests.test_gpu_buffers import S32, Guarded
    m = _model(eng, deep, monkeypatch, None)
    rows = lists["place"][0]
    assert lists["place"][1][-1][-1] == (2, 2, False)
    want = _want(gold["place"])
    total = int(want[1][-1])
    gb, go = eng.pack(rows)
    g = Guarded(total, torch.int32, S32, gb.device)
    ids, oo = m.encode_batch(gb, go, out=g.t[:total], path=1)
    _same(ids, oo, want)
    assert g.guard_broken() == []


@pytest.mark.parametrize("cache", [None, "off"])
@pytest.mark.parametrize("name", ["pairs", "merges"])
def test_real_model_sets(eng, bpe_model, monkeypatch, name, cache):
    """models/akshar.json: all pairs of its single-character tokens (merge_lookup_c on present and absent
    pairs) and every merge's left + right (every cache key), cache on and off, against the oracle."""
    monkeypatch.delenv("AK_PTC_BITS", raising=False)
    if cache == "off":
        monkeypatch.setenv("AK_PTC", "0")
    else:
        monkeypatch.delenv("AK_PTC", raising=False)
    m = eng.BPE(bpe_model)
    assert (m.cache_info()["slots"] > 0) == (cache is None)
    texts = [" ".join(r) for r in M.real_sets(bpe_model)[name]]
    ref, ro = O.OracleBPE(bpe_model).encode_batch(*O.pack(texts))
    gb, go = eng.pack(texts)
    (ids, oo), ctr = _counted(eng, lambda: m.encode_batch(gb, go, path=1))
    _same(ids, oo, (ref.astype(np.int64), ro.astype(np.int64)))
    if cache is None:
        assert ctr["ptc_probes"] > 0 and ctr["ptc_hits"] > 0
    ids0, oo0 = m.encode_batch(gb, go, path=0)
    assert torch.equal(ids0, ids) and torch.equal(oo0, oo)
