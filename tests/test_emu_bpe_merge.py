"""The BPE tile kernel's merge stage (ak_tile.h: pass C / ptc_probe, pass B / bpe_merge_lds, pass A and
the per-wave pool: pool_flush, merge_rounds, pool_drain; ak_dev.h merge_lookup_c) on the emulated
kernel with the deep-merge model of tests/bpe_merge_rows.py: ids and offsets bit-equal to the
reference's recorded answers under every cache setting, tile height and wave count, and the kernel's
own counters (cache probes and hits, pool batches and lane-rounds, fallback rows) equal to what the
row lists say, so a probe that misses a stored key or a miss that skips the pool cannot hide behind
right ids."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import bpe_merge_rows as M
from tests.emu import emu


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    from akshar_amd.models import BPEModel
    return BPEModel(M.deep_bpe_model(tmp_path_factory.mktemp("deep") / "deep.json"))


@pytest.fixture(scope="module")
def em(deep):
    return emu.Model(bpe=deep)


@pytest.fixture(scope="module")
def lists():
    return M.merge_rows()


@pytest.fixture(scope="module")
def gold():
    return M.golden()["lists"]


def _want(gold_rows):
    oo = np.zeros(len(gold_rows) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in gold_rows], out=oo[1:])
    return np.asarray([x for r in gold_rows for x in r], dtype=np.uint32), oo


def _run(em, rows, gold_rows, tile_rows, waves):
    ids, oo, st = emu.bpe_tiles(em, *O.pack(rows), rows=tile_rows, waves=waves)
    wi, wo = _want(gold_rows)
    assert np.array_equal(oo, wo)
    d = np.flatnonzero(ids != wi)
    assert d.size == 0, (int(d[0]), int(np.searchsorted(wo, d[0], side="right")) - 1)
    assert not st.any()


def test_cache_holds_every_key(em, deep):
    """The table the tile path probes: every key stored, keys of every length 2..14, and the two vocab
    strings that are not their own merge_all (N9, N14) counted and left out."""
    info = em.set_ptc(-1)
    assert info["slots"] > 0 and info["stored"] == info["keys"] and info["multi"] == 2
    tab = em.ptc_table().reshape(-1, 8)
    lens = sorted({(int(e[0]) >> 16) & 15 for e in tab} - {0})
    assert lens == list(range(2, 15))
    # L prefixes, R suffixes, N9 / N14 prefixes of 2..14, the tree's 8 + 4 + 2 blocks, yz, yzyz, 88, 889, and the
    # (n7, n8) / (n12, n13) pairs
    assert info["keys"] == 13 + 13 + 7 + 12 + 14 + 4 + 2


# every list in one batch, the lists in an order that puts each one's first row at a different place
# of a 64-row unit; the cache at its default, off, and forced into 4 slots
@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("tile_rows", [2, 8, 16])
@pytest.mark.parametrize("bits", [-1, None, 2])
def test_every_list_equals_the_golden(em, lists, gold, bits, tile_rows, waves):
    info = em.set_ptc(bits)
    try:
        assert info["slots"] == {-1: 1024, None: 0, 2: 4}[bits]
        names = sorted(lists)
        rows = [r for n in names for r in lists[n][0]]
        _run(em, rows, [g for n in names for g in gold[n]], tile_rows, waves)
        probes, hits = emu.last_counters()
        assert (probes > 0) == (bits is not None) and (hits > 0) == (bits is not None)
    finally:
        em.set_ptc(-1)


@pytest.mark.parametrize("name", M.TILE_LISTS)
def test_counters_equal_the_row_list(em, lists, gold, name):
    """One wave, the default table (every key stored), 8-row tiles. Exact for every list: probes = the
    multi-symbol pre-tokens of rows the tile kernel kept (rows over its buffer and the tile with 241
    of them list none), hits = those that are cache keys, lane-rounds = the sum of n - n_after over the
    pooled misses (each round merges one pair per merging lane), batches = ceil(misses / 64): one wave
    and one class, so the ring flushes 64 at a time and once more for the rest when the wave leaves.
    Rounds are not exact from the list alone (a batch runs as many as its deepest lane): bounded."""
    rows, info, _ = lists[name]
    want = M.expected_counters(rows, info)
    assert em.set_ptc(-1)["stored"] > 0
    _run(em, rows, gold[name], 8, 1)
    probes, hits, batches, rounds, lanes = emu.last_counters_all()[:5]
    assert (probes, hits, lanes) == (want["probes"], want["hits"], want["lane_rounds"])
    assert batches == -(-want["misses"] // 64)
    assert rounds <= 14 * batches and rounds * 64 >= lanes
    assert emu.last_fallback_rows() == want["fallback"]
    if name.startswith("pool"):
        assert want["misses"] == int(name[4:]) and len(rows) <= M.UNIT
    if name == "ring":
        assert want["misses"] > M.POOL_RING and len(rows) == M.UNIT
    if name == "scap":
        assert want["fallback"] == 1 and want["probes"] == M.T_SCAP
    if name == "long":
        assert want["long"] == 50


@pytest.mark.parametrize("kind,fb,nfc", [("nfc", 300, 300), ("over", 300, 0), ("host", 0, 0)])
def test_other_paths(em, lists, gold, kind, fb, nfc):
    """The same words through the fallback waves' bpe_tile<..., NFCD> (rows NFC changes), the row pipeline's
    bpe_merge_word (rows over the tile buffer) and, for the per-call sample, the tile."""
    rows, info, _ = lists[kind]
    em.set_ptc(-1)
    _run(em, rows, gold[kind], 8, 3)
    assert len(rows) >= 280
    assert emu.last_fallback_rows() == (len(rows) if fb else 0)
    assert emu.last_nfc_rows() == (len(rows) if nfc else 0)


def test_hits_with_keys_at_their_second_slot(em, lists, gold):
    """128 slots for the 65 keys: every key still stored, several at their second-choice slot (their
    first-choice slot carries the flag), and the hit count is still the list's number: a probe that
    never looks at the second slot returns right ids and loses these hits."""
    info = em.set_ptc(7)
    try:
        assert info["slots"] == 128 and info["stored"] == info["keys"] == 65
        tab = em.ptc_table().reshape(-1, 8)
        assert int(((tab[:, 0] >> 20) & 1).sum()) >= 3  # akp::PTC_FLAG (bit 20): some key's first choice was taken
        rows, inf, _ = lists["place"]
        _run(em, rows, gold["place"], 8, 1)
        want = M.expected_counters(rows, inf)
        assert emu.last_counters() == (want["probes"], want["hits"])
    finally:
        em.set_ptc(-1)


@pytest.mark.parametrize("name,bits", [("pairs", None), ("merges", None), ("merges", -1)])
def test_real_model_sets(bpe_model, name, bits):
    """models/akshar.json: all pairs of its single-character tokens and every merge's left + right, with
    the cache off (every word through merge_lookup_c: the absent pairs whose first slot is flagged, the
    keys stored at their second choice) and on (every cache key probed), against the oracle."""
    m = emu.Model(bpe=bpe_model)
    m.set_ptc(bits)
    texts = [" ".join(r) for r in M.real_sets(bpe_model)[name]]
    buf, offs = O.pack(texts)
    ids, oo, _ = emu.bpe_tiles(m, buf, offs, rows=16, waves=3)
    ref, ro = O.OracleBPE(bpe_model).encode_batch(buf, offs)
    assert np.array_equal(oo, ro) and np.array_equal(ids, ref)
    probes, hits = emu.last_counters()
    assert (hits > 0.9 * len(bpe_model.merges)) if bits == -1 else probes == 0


@pytest.mark.parametrize("bits", [2, 4])
def test_near_misses_of_long_keys_in_tiny_tables(em, lists, gold, bits):
    """4 and 16 slots: every probe lands on one of a few stored keys. Whatever key of 7..14 symbols a
    slot holds, the list has a word of that length with the same first symbols and another last one
    (tests/bpe_merge_rows.py near_words): accepted on the first half-entry alone, it would take the
    key's id."""
    info = em.set_ptc(bits)
    try:
        tab = em.ptc_table().reshape(-1, 8)
        assert info["stored"] == (1 << bits) and max((int(e[0]) >> 16) & 15 for e in tab) > 6
        for name in ("near", "maxn8", "maxn13"):
            _run(em, lists[name][0], gold[name], 8, 1)
    finally:
        em.set_ptc(-1)
