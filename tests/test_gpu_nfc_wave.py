"""The fallback waves' NFC (ak_nfc_wave.h) on the device at the edges of its own loops: the rows of
tests/nfc_wave_rows.py through BPE, SentencePiece and the row ops, against the oracle on every row
and the reference's recorded answers (tests/golden/nfc_wave_edges.jsonl.gz) on every valid row, bit
for bit, with the engine's path counts equal to the numbers predicted from the rows
(nfc_wave_rows.finishes; tests/test_emu_nfc_wave.py states the rules).

The self-contained families (dcap, chunk, straddle, expand, hf) run as one batch and replicated 40
times, so many waves take them. A uniform list has rows of one byte length and a short period, so
whichever rows a wave draws (entries wave, + waves, ... of the fallback list) its batches have the
shape the list was built for; a wave sees a full 64-entry prefix or a 128-row epoch only if the call
holds at least 128 rows per fallback wave (one 704-thread block per CU: 11 waves), so each period is
replicated to that size and the expected output is the oracle's answer for one period, tiled."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import nfc_wave_rows as W
from tests.util import ends_to_lens, pack_rows, rows_ints, rows_runs, rows_u8

pytestmark = pytest.mark.gpu
REP = 40
FAMILIES = ["dcap", "chunk", "straddle", "expand", "hf"]
LISTS = sorted(W.device_uniform_lists())


@pytest.fixture(scope="module")
def eng():
    from akshar_amd import engine
    assert torch.cuda.is_available()
    return engine


@pytest.fixture(scope="module")
def want():
    return W.golden()


@pytest.fixture(scope="module")
def oracles(bpe_model, spm_model):
    return O.OracleBPE(bpe_model), O.OracleSPM(spm_model)


def _cpu(t):
    return t.cpu().numpy()


def _rep(out, oo, rep):
    """A batch's packed output, the batch repeated `rep` times."""
    oo = np.asarray(oo).astype(np.int64)
    offs = np.concatenate([oo[:-1] + k * oo[-1] for k in range(rep)] + [np.asarray([rep * oo[-1]])])
    return np.tile(np.asarray(out)[:oo[-1]], rep), offs


def _device_rows(eng, rows, rep):
    buf, offs = pack_rows(rows)
    big, boffs = _rep(buf[:int(offs[-1])], offs, rep)
    pad = np.zeros(((len(big) + 15) // 16) * 16 + 16, dtype=np.uint8)
    pad[:len(big)] = big
    return eng.to_device(pad, boffs)


def _eq(got, ref, rep):
    """Device arrays (values..., offsets) == the oracle's (values..., offsets) repeated."""
    oo = ref[-1]
    ok = True
    for g, r in zip(got[:-1], ref[:-1]):
        w, offs = _rep(r, oo, rep)
        ok = ok and np.array_equal(_cpu(g)[:len(w)].astype(np.int64), w.astype(np.int64))
    return ok and np.array_equal(_cpu(got[-1]).astype(np.int64), offs)


def _first(t, oo, n):
    """The first copy of the batch in a device output."""
    o = _cpu(oo)[:n + 1]
    return [_cpu(x)[:o[-1]] for x in t] + [o]


def _batch(rows, want, oracles):
    """The oracle's answers for one copy of the rows (computed once) and the predicted counts."""
    buf, offs = pack_rows(rows)
    recs = [want.get(r) for r in rows]
    return {"rows": rows, "n": len(rows), "recs": recs, "invalid": np.asarray([0 if W.is_valid(r) else 1 for r in rows], np.uint8),
            "bpe": oracles[0].encode_batch(buf, offs), "spm": oracles[1].encode_batch(buf, offs),
            "norm": O.normalize_batch(buf, offs, 3), "sw": O.switches_batch(buf, offs, 3),
            False: O.segment_batch(buf, offs, 3, False), True: O.segment_batch(buf, offs, 3, True),
            "done": {k: sum(1 for r, rec in zip(rows, recs) if rec is not None and W.finishes(r, k, rec))
                     for k in ("rows", "spm", "bpe")}}


def _paths(eng, b, kind, rep):
    """Every row left the tile kernel; the waves finished the predicted number and passed the rest on."""
    d = eng.fallback_detail()
    assert eng.fallback_rows()[0] == rep * b["n"], (kind, rep, d)
    assert d["one_lane"] == rep * (b["n"] - b["done"][kind]), (kind, rep, d, b["done"])
    assert d["finished_in_tile_path"] == rep * b["done"][kind], (kind, rep, d, b["done"])


def _status(st, b, rep):
    assert np.array_equal(_cpu(st) & 1, np.tile(b["invalid"], rep))


def _run_ids(eng, model, b, key, gb, go, rep):
    st = torch.full((b["n"] * rep,), 7, dtype=torch.uint8, device=gb.device)
    ids = model.encode_batch(gb, go, row_status=st, path=1)
    _paths(eng, b, key, rep)
    assert _eq(ids, b[key], rep)
    _status(st, b, rep)
    got = rows_ints(*_first(ids[:1], ids[1], b["n"]))
    assert [i for i, r in enumerate(b["recs"]) if r is not None and got[i] != r[key]] == []


def _run_analyze(eng, b, gb, go, rep, matras, singles):
    n, recs = b["n"], b["recs"]
    st = torch.full((n * rep,), 7, dtype=torch.uint8, device=gb.device)
    an = eng.analyze_batch(gb, go, flags=3, matras=matras, row_status=st, path=1)
    _paths(eng, b, "rows", rep)
    _status(st, b, rep)
    assert _eq(an[0:2], b["norm"], rep) and _eq(an[2:4], b[matras], rep) and _eq(an[4:7], b["sw"], rep)
    got = rows_u8(*_first(an[:1], an[1], n))
    assert [i for i, r in enumerate(recs) if r is not None and got[i] != r["norm"]] == []
    got = rows_ints(*_first(an[2:3], an[3], n))
    assert [i for i, r in enumerate(recs) if r is not None and ends_to_lens(got[i]) != r["ak_m" if matras else "ak"]] == []
    got = rows_runs(*_first(an[4:6], an[6], n))
    assert [i for i, r in enumerate(recs) if r is not None and got[i] != r["sw"]] == []
    if singles:  # the single ops equal the fused analyze and take the same path
        norm = eng.normalize_batch(gb, go, flags=3, path=1)
        _paths(eng, b, "rows", rep)
        seg = eng.segment_batch(gb, go, flags=3, matras=matras, path=1)
        _paths(eng, b, "rows", rep)
        sw = eng.switches_batch(gb, go, flags=3, path=1)
        _paths(eng, b, "rows", rep)
        assert all(torch.equal(a, c) for a, c in zip(tuple(norm) + tuple(seg) + tuple(sw), an))


def _run_off(eng, monkeypatch, b, gb, go, rep, models, rows_too):
    """AK_NO_NFC_WAVE=1 on the same rows: nothing is finished by the waves, the outputs are equal."""
    monkeypatch.setenv("AK_NO_NFC_WAVE", "1")
    for model, key in models:
        ids = model.encode_batch(gb, go, path=1)
        d = eng.fallback_detail()
        assert d["one_lane"] == rep * b["n"] and d["finished_in_tile_path"] == 0, (key, d)
        assert _eq(ids, b[key], rep)
    if rows_too:
        an = eng.analyze_batch(gb, go, flags=3, matras=False, path=1)
        d = eng.fallback_detail()
        assert d["one_lane"] == rep * b["n"] and d["finished_in_tile_path"] == 0, d
        assert _eq(an[0:2], b["norm"], rep) and _eq(an[2:4], b[False], rep) and _eq(an[4:7], b["sw"], rep)
    monkeypatch.delenv("AK_NO_NFC_WAVE")


@pytest.mark.parametrize("rep", [1, REP])
@pytest.mark.parametrize("family", FAMILIES)
def test_families_through_the_wave_nfc(eng, want, oracles, bpe_model, spm_model, monkeypatch, family, rep):
    """dcap, chunk, straddle, expand and (BPE only) hf: one batch, and 40 copies of it; the single
    batch once more with the one-lane path alone."""
    b = _batch([r for r, _ in W.families()[family]], want, oracles)
    gb, go = _device_rows(eng, b["rows"], rep)
    bpe = eng.BPE(bpe_model)
    _run_ids(eng, bpe, b, "bpe", gb, go, rep)
    if family == "hf":  # (its rows leave the BPE tile only)
        if rep == 1:
            _run_off(eng, monkeypatch, b, gb, go, rep, [(bpe, "bpe")], False)
        return
    spm = eng.SPM(spm_model)
    _run_ids(eng, spm, b, "spm", gb, go, rep)
    for matras in (False, True):
        _run_analyze(eng, b, gb, go, rep, matras, singles=not matras)
    if rep == 1:
        _run_off(eng, monkeypatch, b, gb, go, rep, [(bpe, "bpe"), (spm, "spm")], True)


@pytest.mark.parametrize("name", LISTS)
def test_uniform_lists_through_the_wave_nfc(eng, want, oracles, bpe_model, spm_model, monkeypatch, name):
    """Each uniform list's period replicated until every fallback wave holds the rows its shape needs
    (128 for the batch prefix, the epoch's rows and the HF rounds, 6 for the text reserve and the
    768-byte rows); then the same rows with the one-lane path alone."""
    rows, per_wave = W.device_uniform_lists()[name]
    b = _batch([r for r, _ in rows], want, oracles)
    waves = 11 * torch.cuda.get_device_properties(0).multi_processor_count
    rep = -(-per_wave * waves // b["n"])
    gb, go = _device_rows(eng, b["rows"], rep)
    bpe = eng.BPE(bpe_model)
    _run_ids(eng, bpe, b, "bpe", gb, go, rep)
    if name.startswith("hf"):
        _run_off(eng, monkeypatch, b, gb, go, rep, [(bpe, "bpe")], False)
        return
    spm = eng.SPM(spm_model)
    _run_ids(eng, spm, b, "spm", gb, go, rep)
    _run_analyze(eng, b, gb, go, rep, False, singles=False)
    _run_off(eng, monkeypatch, b, gb, go, rep, [(bpe, "bpe"), (spm, "spm")], True)
