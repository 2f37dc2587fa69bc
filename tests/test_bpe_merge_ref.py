"""The reference chain of the merge-stage rows (tests/bpe_merge_rows.py): the merge_all result of every
constructed word STATED from its construction == an independent Python merge_all == the reference's
recorded ids (tests/golden/bpe_merge_hf.json.gz) == the oracle, on the deep-merge model; and for the
two exhaustive sets on models/akshar.json, Python merge_all == the oracle, and the oracle's hash ==
the reference's recorded one. Everything the emulator and device tests compare against hangs on this."""
import hashlib
import re
import unicodedata
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as O
from tests import bpe_merge_rows as M
from tests.test_emu_ptc import _merge_all


@pytest.fixture(scope="module")
def deep(tmp_path_factory):
    from akshar_amd.models import BPEModel
    return BPEModel(M.deep_bpe_model(tmp_path_factory.mktemp("deep") / "deep.json"))


@pytest.fixture(scope="module")
def lists():
    return M.merge_rows()


def _rank(bm):
    rank = {}
    for r, (a, b, c) in enumerate(bm.merges.tolist()):
        rank.setdefault((a, b), (r, c))
    return rank


def test_model_shape_for_the_tile_path(deep):
    """What ak_engine.hip asks of a model before the tile path takes it: every id below 0x7FFC, new ids
    increasing with merge rank; and the families are all there."""
    new = deep.merges[:, 2].astype(np.int64)
    assert deep.vocab_size < 0x7FFC and np.all(np.diff(new) > 0) and new[0] > deep.single_id.max()
    lens = Counter(len(t) for t in deep.vocab if not t.startswith("<"))
    assert max(lens) == 24 and all(lens[k] >= 2 for k in range(2, 25)) and lens[16] == 3


def test_stated_results_are_merge_all(deep):
    """Every constructed word's stated result is what lowest-rank-leftmost merging gives."""
    rank, v = _rank(deep), deep.vocab
    ws = M.edge_words()
    assert len(ws) >= 400
    for text, toks in ws:
        assert "".join(toks) == text
        assert _merge_all([v[c] for c in text], rank) == [v[t] for t in toks], text
        assert not re.search(r"(.)\1\1", text), text  # the elongation rule leaves it alone


def test_lists_cover_the_edges(lists):
    """The measured coverage the commit message quotes: every length, cache keys at 8..14 symbols, a
    15-symbol miss that runs 14 rounds, long pre-tokens that collapse."""
    pre = [t for name in M.TILE_LISTS for inf in lists[name][1] for t in inf]
    by_n = Counter(n for n, _, _ in pre)
    assert all(by_n[n] >= 8 for n in M.LENGTHS), by_n
    keys = Counter(n for n, _, key in pre if key)
    assert all(keys[n] >= 4 for n in range(2, 15)) and not any(key for n, _, key in pre if n > 14)
    assert max(n - k for n, k, key in pre if not key and n < M.WREG) == 14
    assert any(n == 15 and k == 1 for n, k, _ in pre) and any(n in (16, 17, 24) and k == 1 for n, k, _ in pre)
    assert any(n == 9 and k == 2 for n, k, _ in pre) and any(n == 14 and k == 2 for n, k, _ in pre)  # N9, N14
    print("rows", sum(len(lists[n][0]) for n in lists), "pre-tokens per length", sorted(by_n.items()),
          "cache keys per length", sorted(keys.items()))


def test_stated_equals_golden_equals_oracle(deep, lists):
    gold = M.golden()["lists"]
    assert sorted(gold) == sorted(lists)
    orc = O.OracleBPE(deep)
    v = deep.vocab
    for name, (rows, _, toks) in lists.items():
        ids, oo = orc.encode_batch(*O.pack(rows))
        got = [ids[int(oo[i]):int(oo[i + 1])].tolist() for i in range(len(rows))]
        assert got == gold[name], name
        for i, t in enumerate(toks):
            want = [deep.bos] + [v[x] for x in t if x != M.NFC_TAIL] + [deep.eos]
            assert got[i] == want, (name, i)


def _clean(w, single):
    """One pre-token of known chars (letters, marks and digits: the Whitespace pre-tokenizer's \\w) that
    normalize_text and NFKC leave alone."""
    return (all(c in single and unicodedata.category(c)[0] in "LMN" for c in w) and not re.search(r"(.)\1\1", w)
            and unicodedata.normalize("NFKC", w).lower() == w)


@pytest.mark.parametrize("name", ["pairs", "merges"])
def test_real_model_sets(bpe_model, name):
    """models/akshar.json: all pairs of its single-character tokens, and every merge's left + right."""
    rows = M.real_sets(bpe_model)[name]
    rec = M.golden()["real"][name]
    assert len(rows) == rec["rows"] and sum(len(r) for r in rows) == {"pairs": 112 * 112, "merges": len(bpe_model.merges)}[name]
    ids, oo = O.OracleBPE(bpe_model).encode_batch(*O.pack([" ".join(r) for r in rows]))
    h = hashlib.sha256(ids.astype(np.int32).tobytes() + oo.astype(np.int64).tobytes()).hexdigest()
    assert h == rec["sha256"]
    single = {chr(int(c)): int(i) for c, i in zip(bpe_model.single_cp, bpe_model.single_id)}
    rank = _rank(bpe_model)
    # the words that are one pre-token which normalization leaves alone, 32 per row again
    cw = [w for r in rows for w in r if _clean(w, single)]
    assert len(cw) > 1000, len(cw)  # (not vacuous; the rest hold punctuation, or chars NFKC or the filter change)
    print(name, "words checked against Python merge_all:", len(cw))
    crows = [cw[i:i + 32] for i in range(0, len(cw), 32)]
    ids, oo = O.OracleBPE(bpe_model).encode_batch(*O.pack([" ".join(r) for r in crows]))
    for i, r in enumerate(crows):
        want = [bpe_model.bos] + [x for w in r for x in _merge_all([single[c] for c in w], rank)] + [bpe_model.eos]
        assert ids[int(oo[i]):int(oo[i + 1])].tolist() == want, (name, i)
