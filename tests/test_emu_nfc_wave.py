"""The fallback waves' NFC (ak_nfc_wave.h) on the host emulator at the edges of its own loops: the
rows of tests/nfc_wave_rows.py (segments of 14 .. 18 decomposed code points, 63 .. 193 non-trivial
segments per batch, segments over the 64-char step, uniform lists for the block copy, the batch
prefix, the epoch's rows and text reserve, rows that triple, HF rounds) through the BPE,
SentencePiece and row-op kernels on one and on three emulated waves, against the oracle on every
row and the reference's recorded answers (tests/golden/nfc_wave_edges.jsonl.gz) on every valid row.
Bit-exact, row statuses included.

Path accounting: every row leaves the tile kernel, and the number the waves finish equals the number
predicted from the rows by nfc_wave_rows.finishes(): the row's fate ("wave": valid, at most 768 bytes,
no segment past 16 decomposed code points) and the caller's further documented rules: the epoch's
tile takes the NFC text only within its buffer (768 bytes; the SentencePiece tile variant 480), the
result must fit the row's fallback slot (cnt > mul len + 2 goes on), and for BPE a row HF's NFKC
changes must have no HF segment past 16. A row that is passed on never takes a neighbour with it: the
count is exact."""
import unicodedata

import numpy as np
import pytest

from oracle import oracle as O
from tests import nfc_wave_rows as W
from tests.emu import emu
from tests.util import ends_to_lens, pack_rows, rows_ints, rows_runs, rows_u8

FAMILIES = ["dcap", "chunk", "straddle", "uniform", "expand", "hf"]
WAVES = [1, 3]


@pytest.fixture(scope="module")
def fams():
    return W.families()


@pytest.fixture(scope="module")
def want():
    return W.golden()


def _batch(fr, want, bpe_model, spm_model=None):
    """The packed rows, the oracle's answers and the predicted counts (BPE alone without spm_model)."""
    rows = [r for r, _ in fr]
    buf, offs = pack_rows(rows)
    recs = [want.get(r) for r in rows]
    b = {"rows": rows, "buf": buf, "offs": offs, "recs": recs, "invalid": [0 if W.is_valid(r) else 1 for r in rows],
         "bpe": rows_ints(*O.OracleBPE(bpe_model).encode_batch(buf, offs)),
         "done": {k: sum(1 for r, rec in zip(rows, recs) if rec is not None and W.finishes(r, k, rec))
                  for k in ("rows", "spm", "bpe")}}
    if spm_model is not None:
        b.update({"norm": rows_u8(*O.normalize_batch(buf, offs, 3)), "sw": rows_runs(*O.switches_batch(buf, offs, 3)),
                  False: rows_ints(*O.segment_batch(buf, offs, 3, False)), True: rows_ints(*O.segment_batch(buf, offs, 3, True)),
                  "spm": rows_ints(*O.OracleSPM(spm_model).encode_batch(buf, offs))})
    return b


@pytest.fixture(scope="module")
def batches(fams, want, bpe_model, spm_model):
    """Per family, computed once."""
    return {name: _batch(fr, want, bpe_model, spm_model) for name, fr in fams.items()}


def _bad(got, ref):
    return [i for i, (g, r) in enumerate(zip(got, ref)) if g != r]


def _check_ids(b, key, ids, oo, st):
    got = rows_ints(ids, oo)
    assert len(got) == len(b[key]) and _bad(got, b[key]) == []
    assert [i for i, rec in enumerate(b["recs"]) if rec is not None and got[i] != rec[key]] == []
    assert st.tolist() == b["invalid"]


def _check_rows(b, res, ops, matras):
    recs = b["recs"]
    if ops & 1:
        got = rows_u8(*res["norm"])
        assert _bad(got, b["norm"]) == []
        assert [i for i, r in enumerate(recs) if r is not None and got[i] != r["norm"]] == []
    if ops & 2:
        got = rows_ints(*res["seg"])
        assert _bad(got, b[matras]) == []
        assert [i for i, r in enumerate(recs) if r is not None and ends_to_lens(got[i]) != r["ak_m" if matras else "ak"]] == []
    if ops & 4:
        got = rows_runs(*res["runs"])
        assert _bad(got, b["sw"]) == []
        assert [i for i, r in enumerate(recs) if r is not None and got[i] != r["sw"]] == []
    assert res["status"].tolist() == b["invalid"]


def _paths(b, kind, off):
    """Every row left the tile kernel; the waves finished the predicted number (none when off)."""
    assert emu.last_fallback_rows() == len(b["rows"])
    assert emu.last_nfc_rows() == (0 if off else b["done"][kind])


def _run_bpe(b, bpe_model, waves, off=False):
    ids, oo, st = emu.bpe_tiles(emu.Model(bpe=bpe_model), b["buf"], b["offs"], rows=8, waves=waves)
    _paths(b, "bpe", off)
    _check_ids(b, "bpe", ids, oo, st)


def _run_spm(b, spm_model, waves, off=False):
    ids, oo, st = emu.spm_tiles(emu.Model(spm=spm_model), b["buf"], b["offs"], rows=8, waves=waves)
    _paths(b, "spm", off)
    _check_ids(b, "spm", ids, oo, st)


def _run_rows(b, waves, off=False):
    for matras in (False, True):
        fused = emu.rows_tiles(7, b["buf"], b["offs"], matras=matras, rows=16, waves=waves)
        _paths(b, "rows", off)
        _check_rows(b, fused, 7, matras)
        for ops, key in ((2, "seg"),) if matras else ((1, "norm"), (2, "seg"), (4, "runs")):  # (ops 1 and 4 take no matras)
            res = emu.rows_tiles(ops, b["buf"], b["offs"], matras=matras, rows=16, waves=waves)
            _paths(b, "rows", off)
            _check_rows(b, res, ops, matras)
            assert all(np.array_equal(x, y) for x, y in zip(res[key], fused[key]))


@pytest.mark.skipif(unicodedata.unidata_version != "13.0.0", reason="the row set is checked against Unicode 13 data")
def test_row_set_reaches_the_edges(fams, want):
    """Each family holds what it claims; the reference answered every valid row."""
    for name, fr in fams.items():
        for r, fate in fr:
            assert fate == W.fate_of(r), (name, r)
            assert W.is_valid(r) == (r in want) and (r not in want or want[r]["text"].encode("utf-8") == r)
        assert all(W.is_valid(r) for r, _ in fr) or name == "uniform"
    assert [unicodedata.combining(c) for c in W.DESC] == sorted((unicodedata.combining(c) for c in W.DESC), reverse=True)
    assert len({unicodedata.combining(c) for c in W.DESC}) == len(W.DESC) and unicodedata.combining(W.DESC[-1]) > 9
    # dcap: every variant at 14 .. 18 decomposed code points, the input one char shorter for the bases that decompose
    for n in W.DCAP_N:
        segs = (W.seg_desc(n), W.seg_equal(n), W.seg_dbase(n), W.seg_dbase(n - 1, "z" + W.ZA))
        assert [W.dlen(s) for s in segs] == [n] * 4 and [len(s) for s in segs] == [n, n, n - 1, n - 1]
        assert all(len(W.segments("q" + s)) == 2 for s in segs)
        for s in segs:
            assert sum((s.encode(), f) in fams["dcap"] for f in ("wave", "one_lane")) == 1
    for n in (15, 16, 17):
        assert W.dlen(W.seg_marks(n)) == n == max(W.dlen(s) for s in W.segments(W.seg_marks(n) + W.KA))
        assert W.dlen(W.seg_jamo(n)) == n and len(W.segments(W.seg_jamo(n))) == 1
    worst = sorted(W.dlen(s) for r, _ in fams["dcap"] for s in W.segments(r.decode()))
    assert set(W.DCAP_N) <= set(worst) and worst[-1] == 18
    # chunk: N non-trivial segments after k trivial chars, every row within the batch
    for n in W.CHUNK_N:
        for k in W.CHUNK_K:
            row = W.chunk_row(n, k)
            assert W.count_nontrivial(row) == (n, k) and (row.encode(), "wave") in fams["chunk"]
    for gap in (1, 2):
        segs = W.segments(W.chunk_row(128, 0, gap))
        assert [i for i, s in enumerate(segs) if not W.trivial(s)] == list(range(gap, 128 * (gap + 1), gap + 1))
    assert max(len(r) for r, _ in fams["chunk"]) <= W.NW_MAXB and {W.NNNA, "x" + W.QA, W.NA + W.NUKTA} <= {W.chunk_seg(i) for i in range(8)}
    # straddle: the four chars of a segment at char indices k .. k + 3
    for k in W.STRADDLE_AT:
        for s in W.STRADDLE_SEGS:
            row = W.straddle_row(k, s)
            assert row.index(s) == k and s in W.segments(row) and unicodedata.normalize("NFC", s) != s
    # ... at those indices of the batch too: a row of these two families is alone in its batch
    assert all(2 * len(r) > W.NW_MAXB for f in ("straddle", "chunk") for r, _ in fams[f])
    assert all(2 * len(W.hf_elong_row(at, run).encode()) > W.NW_MAXB for at in W.HF_RUN_AT for run in (3, 4, 5, 6))
    for n in (16, 17):  # the m + len check at a segment's end, both sides
        assert all(W.dlen(W.seg_dtail(n, t)) == n and len(W.seg_dtail(n, t)) == n - 1 and W.dlen(t) == 2 for t in W.DTAILS)
        assert all(len(W.segments("q" + W.seg_dtail(n, t))) == 2 for t in W.DTAILS)
    assert all(W.is_stable(chr(c)) for c in (0xAC00, 0xAC01))  # a Hangul syllable always opens its segment: m + 3 at m = 0
    # uniform: equal byte lengths, every start alignment of the block copy, ends on, before and after a block edge
    for L in W.ODD_L + (12, 13, 681, 682, 768):
        assert {len(r) for r, _ in W.uniform(L)} == {L} and len({r for r, _ in W.uniform(L)}) == W.UNIFORM_P
    rows = [r for r, _ in fams["uniform"]]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    assert {int(o) & 15 for o in offs[:-1]} == set(range(16)) and {15, 0, 1} <= {int(o) & 15 for o in offs[1:]}
    assert 64 * 12 == W.NW_MAXB and 3 * 4 * 681 + 16 <= W.NE_TCAP < 3 * 4 * 682 + 16
    assert sum(len(r) == W.NW_MAXB + 1 for r in rows) == 3 and sum(len(r) == W.NW_MAXB for r in rows) == 3
    # the mark-opening rows, a call of their own: 16 chars and 30 bytes each, so every batch is 25 rows and its rows
    # 4, 8, ... open at lane 0 of a step, right after a row that ends at lane 63
    ms = [r for r, _ in W.markstart(5 * max(WAVES))]
    assert all(len(r) == 30 and len(r.decode()) == 16 and unicodedata.combining(r.decode()[0]) for r in ms)
    assert W.NW_MAXB // 30 == 25 and all(len(ms[w::waves]) >= 25 + 5 and len(set(ms[w::waves])) >= 2 for waves in WAVES for w in range(waves))
    for L in (12, 13, 9):
        assert sum(len(r) == L for r in rows) >= W.NE_VMAX + 2
    # expand: the dense rows triple; hf: HF's NFKC changes the normalized rows
    dense = [r for r, _ in fams["expand"] if b"\xf0\x9d\x85\xa0" in r]
    assert max(len(r) for r in dense) == W.NW_MAXB and any(W.nfc_bytes(r) > 2.5 * len(r) for r in dense)
    hf = [r for r, _ in fams["hf"] if W.hf_changes(want[r]["norm"])]
    assert len(hf) >= len(fams["hf"]) - 3
    assert sorted(max(W.dlen(s) for s in W.hf_segments(want[r]["norm"])) for r in hf)[-4:] == [15, 16, 16, 17]
    for at in W.HF_RUN_AT:
        t = want[W.hf_elong_row(at, 3).encode()]["norm"]
        assert len(W.hf_elong_row(at, 3).encode()) > W.NW_MAXB // 2 and "zz" not in t
    # the HF epoch lists: n * waves rows of 7 bytes give each wave (rows w, w + waves, ...) one epoch of n HF rows
    assert set(W.HF_EPOCH_N) == {63, 64, 65, 127, 128} and max(W.HF_EPOCH_N) <= W.NE_VMAX
    for n in W.HF_EPOCH_N:
        for waves in WAVES:
            rows = [r for r, _ in W.hf_short(n * waves)]
            assert all(len(r) == 7 and W.hf_changes(want[r]["norm"]) and W.finishes(r, "bpe", want[r]) for r in rows)
            assert all(len(rows[w::waves]) == n and len(set(rows[w::waves])) == 3 for w in range(waves))
            assert 3 * 7 * n + 16 <= W.NE_TCAP and 64 * 7 <= W.NW_MAXB
    # the HF rounds: 128 rows fit the epoch as raw bytes, their NFC text is over twice a round's reserve,
    # so the first round leaves more than 64 rows for hf_rest_down
    for waves in WAVES:
        rows = [r for r, _ in W.hf_grow(W.NE_VMAX * waves)]
        assert all(len(r) == W.HF_GROW_RAW and W.nfc_bytes(r) == W.HF_GROW_NFC and W.hf_changes(want[r]["norm"]) for r in rows)
        assert all(len(set(rows[w::waves])) == 3 and W.finishes(r, "bpe", want[r]) for w in range(waves) for r in rows[w::waves])
    assert 3 * W.HF_GROW_RAW * W.NE_VMAX + 16 <= W.NE_TCAP
    per_round = (W.NE_TCAP - 16) // 3 // W.HF_GROW_NFC
    assert per_round == 63 and W.NE_VMAX - per_round > 64 and W.HF_GROW_NFC * W.NE_VMAX > 2 * (W.NE_TCAP - 16) // 3
    # (681-byte HF rows: the NFC epoch holds four; their NFC text does not grow, so one HF round takes them)
    assert all(W.nfc_bytes(r) <= len(r) for r, _ in W.hf_long(5))


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("family", FAMILIES)
def test_bpe_through_the_wave_nfc(batches, bpe_model, family, waves):
    _run_bpe(batches[family], bpe_model, waves)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("family", FAMILIES[:-1])  # (the hf rows leave the BPE tile only)
def test_spm_through_the_wave_nfc(batches, spm_model, family, waves):
    _run_spm(batches[family], spm_model, waves)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("family", FAMILIES[:-1])
def test_row_ops_through_the_wave_nfc(batches, family, waves):
    _run_rows(batches[family], waves)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_lane_path_alone_gives_the_same(batches, bpe_model, spm_model, monkeypatch, family):
    """AK_NO_NFC_WAVE=1: nothing is finished by the waves, and every output equals the oracle's and
    the reference's as above."""
    monkeypatch.setenv("AK_NO_NFC_WAVE", "1")
    b = batches[family]
    _run_bpe(b, bpe_model, 1, off=True)
    if family == "hf":  # (its rows leave the BPE tile only)
        return
    _run_spm(b, spm_model, 1, off=True)
    _run_rows(b, 1, off=True)


@pytest.mark.parametrize("waves", WAVES)
def test_mark_opening_rows_at_lane_0(want, bpe_model, spm_model, waves):
    """Rows of 16 chars that open with a mark, alone in the call: in every batch a row ends at lane 63
    and the next opens with its mark at lane 0 of the following step."""
    b = _batch(W.markstart(5 * waves), want, bpe_model, spm_model)
    assert b["done"] == {k: len(b["rows"]) for k in ("rows", "spm", "bpe")}
    _run_bpe(b, bpe_model, waves)
    _run_spm(b, spm_model, waves)
    _run_rows(b, waves)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("n", W.HF_EPOCH_N)
def test_hf_epochs_of_n_rows(want, bpe_model, n, waves):
    """Every wave's one epoch holds exactly n rows HF's NFKC changes (63, 64, 65, 127, 128: the map,
    elongation and segment passes of hf_epoch_gather at their 64-entry steps); all finish in the wave."""
    b = _batch(W.hf_short(n * waves), want, bpe_model)
    assert b["done"]["bpe"] == n * waves
    _run_bpe(b, bpe_model, waves)


@pytest.mark.parametrize("waves", WAVES)
def test_hf_rounds_cut_by_the_text_reserve(want, bpe_model, waves):
    """Every wave's epoch holds 128 HF rows whose NFC text is over twice a round's reserve: three HF
    rounds, hf_rest_down moves 65 rows (two entries in lane 0), then 2; all finish in the wave."""
    b = _batch(W.hf_grow(W.NE_VMAX * waves), want, bpe_model)
    assert b["done"]["bpe"] == W.NE_VMAX * waves
    _run_bpe(b, bpe_model, waves)


def test_predicted_counts(batches):
    """The prediction is not vacuous: in every family the waves finish rows, and the families built to
    pass rows on pass some on, for each kernel."""
    for name, b in batches.items():
        n = len(b["rows"])
        assert all(0 < b["done"][k] <= n for k in ("rows", "spm", "bpe")), (name, b["done"])
    assert all(batches[f]["done"]["rows"] < len(batches[f]["rows"]) for f in ("dcap", "uniform", "expand"))
