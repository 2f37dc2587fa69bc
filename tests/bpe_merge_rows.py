"""A deep-merge BPE model and the rows that take the tile kernel's merge stage (ak_tile.h: pass C /
ptc_probe, pass B / bpe_merge_lds, pass A and the per-wave pool: pool_flush, merge_rounds, pool_drain,
merge_lookup_c, unit_copy_live) to its edges. models/akshar.json has no token over 7 characters and
needs at most 7 merge rounds; this model's chains merge 24 deep, so cache keys of 8..14 symbols,
pooled misses that run 14 rounds, and pre-tokens of 16 and more symbols that collapse all exist.

Every word is a concatenation of PIECES from families with disjoint alphabets, so no merge crosses a
piece boundary and the merge_all result of a word is the concatenation of its pieces' results, each
STATED from the family's construction (never computed by running a merge loop):

  L-chain  c0..c23 (a..x): (c0,c1), (c0c1,c2), ...: a prefix is one id, every merge at position 0;
           an infix that does not start at c0 has no merge
  R-chain  d0..d23 (Devanagari ka..bha): (d22,d23), (d21,d22d23), ...: a suffix is one id, the merges
           walk left from the last pair; an infix that does not end at d23 has no merge
  tree     t0..t15 (Bengali ka..ta): sibling pairs level by level, the ranks inside a level neither
           left-to-right nor right-to-left; an infix [a, b) merges to its maximal aligned blocks
  ties     (y,z), (yz,yz), (8,8), (88,9): "yz" k times has the same rank at every even position
  N9, N14  as "abc" in tests/util.py tiny_bpe_model at 9 and 14 characters: the full string is a vocab
           token (made by (n0..n7, n8)) whose merge_all is [n0..n6, n7n8], because (n7,n8) has the lowest
           rank: never a cache key (ak_bpe_cache_info "multi")
  filler   digits 0..7, Devanagari and Bengali vowels: in no merge

Vocab ids follow merge order (ak_engine.hip accepts the model for the tile path: ids < 0x7FFC, new ids
increasing with rank). Rows are lists of words separated by spaces; "7" is a one-symbol word (never
listed by pass S). Every list returns (rows, info): info[i] = [(n_symbols, n_after_merge,
is_cache_key), ...] for row i's multi-symbol pre-tokens, from which the tests count probes, hits,
pooled misses, lane-rounds and fallback rows."""
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bpe_merge_hf.json.gz")

PTC_MAXN = 14     # ak_ptc.h: the longest cached pre-token
WREG = 16         # ak_tile.h: pre-tokens of >= WREG symbols merge in pass B, shorter misses in the pool
T_BCAP = 768      # staged bytes per tile
T_SCAP = 240      # multi-symbol pre-tokens a tile lists
POOL_RING = 320
UNIT = 64

L = "abcdefghijklmnopqrstuvwx"
R = "कखगघङचछजझञटठडढणतथदधनपफबभ"
T = "কখগঘঙচছজঝঞটঠডঢণত"
N9 = "मयरलळवशषस"
N14 = "থদধনপফবভমযরলশষ"
TIE = "yz89"
FILL = "01234567" + "".join(chr(c) for c in (0x0905, 0x0906, 0x0907, 0x0908, 0x0909, 0x090a, 0x090f, 0x0910, 0x0913, 0x0914,
                                             0x0985, 0x0986, 0x0987, 0x0988, 0x0989, 0x098a, 0x098f, 0x0990, 0x0993, 0x0994))
SPECIALS = ["<pad>", "<unk>", "<s>", "</s>", "<mask>"]
TREE_ORDER = ([5, 2, 7, 0, 3, 6, 1, 4], [2, 0, 3, 1], [1, 0], [0])  # rank order of the sibling pairs per level
assert len(set(L + R + T + N9 + N14 + TIE + FILL)) == 24 + 24 + 16 + 9 + 14 + 4 + 28 and len(R) == 24


def merges():
    """The merges (left, right) in rank order."""
    mg = [("y", "z"), ("yz", "yz"), ("8", "8"), ("88", "9")]
    for A in (N9, N14):
        mg.append((A[-2], A[-1]))
        mg += [(A[:k], A[k]) for k in range(1, len(A))]
    mg += [(L[:k], L[k]) for k in range(1, 24)]
    mg += [(R[k], R[k + 1:]) for k in range(22, -1, -1)]
    for lvl, order in enumerate(TREE_ORDER):
        w = 1 << lvl
        mg += [(T[2 * w * i:2 * w * i + w], T[2 * w * i + w:2 * w * i + 2 * w]) for i in order]
    return mg


def vocab():
    v = {t: i for i, t in enumerate(SPECIALS)}
    for ch in L + R + T + N9 + N14 + TIE + FILL:
        v[ch] = len(v)
    for a, b in merges():
        assert a + b not in v
        v[a + b] = len(v)
    return v


def deep_bpe_model(path):
    """Write the model as a tokenizer.json in the shape of tests/util.py tiny_bpe_model; returns the path."""
    tmpl = [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
            {"SpecialToken": {"id": "</s>", "type_id": 0}}]
    j = {"version": "1.0", "truncation": None, "padding": None,
         "added_tokens": [{"id": i, "content": t, "single_word": False, "lstrip": False, "rstrip": False,
                           "normalized": False, "special": True} for i, t in enumerate(SPECIALS)],
         "normalizer": {"type": "NFKC"}, "pre_tokenizer": {"type": "Whitespace"},
         "post_processor": {"type": "TemplateProcessing", "single": tmpl, "pair": tmpl + tmpl,
                            "special_tokens": {"<s>": {"id": "<s>", "ids": [2], "tokens": ["<s>"]},
                                               "</s>": {"id": "</s>", "ids": [3], "tokens": ["</s>"]}}},
         "decoder": None,
         "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": None,
                   "end_of_word_suffix": None, "fuse_unk": False, "byte_fallback": False, "ignore_merges": False,
                   "vocab": vocab(), "merges": [[a, b] for a, b in merges()]}}
    with open(path, "w", encoding="utf-8") as f:
        json.dump(j, f, ensure_ascii=False)
    return str(path)


# ------------------------------------------------------------------------------------------ pieces
# a piece = (text, [token strings of its merge_all result]), stated from the family's construction


def lp(k):
    """L-chain prefix of k chars: one id."""
    return (L[:k], [L[:k]])


def linf(a, k):
    """L-chain infix c_a.. of k chars, a >= 1: no merge."""
    assert a >= 1 and a + k <= 24
    return (L[a:a + k], list(L[a:a + k]))


def rs(k):
    """R-chain suffix of k chars: one id."""
    return (R[24 - k:], [R[24 - k:]])


def rinf(a, k):
    """R-chain infix of k chars that does not reach d23: no merge."""
    assert a + k <= 23
    return (R[a:a + k], list(R[a:a + k]))


def tree(a, b):
    """Tree leaves [a, b): the maximal aligned blocks, left to right."""
    out = []
    while a < b:
        w = 1
        while a % (2 * w) == 0 and a + 2 * w <= b:
            w *= 2
        out.append(T[a:a + w])
        a += w
    return ("".join(out), out)


def fill(k, off=0):
    """k filler chars from position `off` of the filler cycle: no merge."""
    s = "".join(FILL[(off + i) % len(FILL)] for i in range(k))
    return (s, list(s))


def yz(k):
    """"yz" k times: k // 2 ids "yzyz", then "yz" if k is odd."""
    return ("yz" * k, ["yzyz"] * (k // 2) + ["yz"] * (k % 2))


def n_full(A):
    """The whole N-family string: a vocab token, but merge_all gives two ids."""
    return (A, [A[:-2], A[-2:]])


def n_pre(A, k):
    """An N-family prefix of k < len chars: one id."""
    assert 1 <= k < len(A)
    return (A[:k], [A[:k]])


def word(*pieces):
    """(text, tokens) of the concatenated pieces (empty pieces allowed)."""
    return ("".join(p[0] for p in pieces), [t for p in pieces for t in p[1]])


def info_of(w):
    n, k = len(w[0]), len(w[1])
    return (n, k, k == 1 and 2 <= n <= PTC_MAXN)


def big(n, kinds):
    """n chars from the largest pieces of `kinds` in turn (each collapsing to one id), then filler."""
    pieces, left = [], n
    for k in kinds:
        size = {"L": 24, "R": 24, "T": 16, "N14": 13, "Y": 4, "U": 3, "N9": 8}[k]
        m = min(size, left)
        if m < 2:
            break
        pieces.append({"L": lp, "R": rs, "T": lambda q: tree(0, q), "N14": lambda q: n_pre(N14, q), "Y": lambda q: yz(q // 2),
                       "U": lambda q: ("889"[:q], ["889"] if q == 3 else ["88"]), "N9": lambda q: n_pre(N9, q)}[k](m))
        left -= len(pieces[-1][0])
    pieces.append(fill(left, 3))
    return word(*pieces)


LENGTHS = list(range(2, 18)) + [23, 24, 31, 32, 33, 63, 64, 65, 100]


def form_words():
    """Every length in four forms: (a) fully merging (one id up to 24 chars, beyond that each glued part
    to one id), (b) no merge, (c) merging to several ids with a survivor in each third, (d) a cache key."""
    ws = []
    for n in LENGTHS:
        ws.append(lp(n) if n <= 24 else big(n, ["L", "R", "T", "N14", "Y", "U", "N9"]))
        if n <= 24:
            ws.append(rs(n))
        ws.append(linf(1, n) if n <= 23 else fill(n, n))
        if n >= 3:
            p1 = (n + 2) // 3
            p2 = (n - p1 + 1) // 2
            p3 = n - p1 - p2
            ws.append(word(big(p1, ["L"]), big(p2, ["R"]), tree(0, p3) if p3 <= 15 else big(p3, ["T", "N14"])))
            ws.append(word(big(p1, ["R"]), tree(1, 1 + p2) if p2 <= 15 else big(p2, ["T"]), big(p3, ["L"])))
        if n in (2, 4, 8):
            ws.append(tree(8, 8 + n))
        if n <= 8:
            ws.append(n_pre(N9, n))
        if n <= 13:
            ws.append(n_pre(N14, n))
    ws += [n_full(N9), n_full(N14), tree(0, 16), tree(0, 15), tree(1, 16), tree(3, 14), tree(0, 9), tree(0, 13), tree(0, 14)]
    ws += [word(n_full(N9), fill(3)), word(fill(2), n_full(N14)), word(n_full(N14), lp(2)), word(tree(0, 16), lp(3))]
    return ws


def position_words():
    """For n = 2..15 and every p: a word whose first merge is at position p (one pair between
    fillers, and a chain that goes on merging at p); for n = 15 the last merge at p too (an R-chain
    suffix: the merges walk left from position 13 down to p)."""
    ws = []
    for n in range(2, 16):
        for p in range(n - 1):
            ws.append(word(fill(p), lp(2), fill(n - p - 2, p + 2)))
            if n - p > 2:
                ws.append(word(fill(p, 5), lp(n - p)))
    for p in range(14):
        ws.append(word(fill(p, 9), rs(15 - p)))
        ws.append(word(fill(p, 2), tree(0, 15 - p)))
    return ws


def tie_words():
    """Equal ranks: at every even position (2..8 times "yz", the odd counts leave a remainder), only at
    odd positions, only in the upper half, at the last pair of 15 symbols, "88988" after the doubling."""
    ws = [yz(k) for k in range(1, 9)]
    ws += [word(fill(1), yz(k)) for k in range(1, 8)]             # minima at 1, 3, 5, ...
    ws += [word(yz(k), fill(15 - 2 * k, 1)) for k in (1, 3, 7)]  # even positions, then no merge
    ws += [word(fill(8, 4), yz(3)), word(fill(9, 4), yz(3)), word(fill(13), yz(1)), word(fill(12), yz(1), fill(1, 4))]
    ws += [("889889", ["889", "889"]), ("8898", ["889", "8"]), ("88988", ["889", "88"]), ("98898", ["9", "889", "8"]),
           ("zyzyzy", ["z", "yzyz", "y"]), ("zyzyzyzy", ["z", "yzyz", "yz", "y"]),
           word(yz(2), ("889", ["889"]), yz(3), ("88", ["88"]))]
    return ws


def tail_words():
    """Misses of n = 5, 6, 7, 8 and 13, 14, 15, 12 symbols (the write-back's tail chunk of 1, 2, 3, 4
    dwords), merged at the front, at the end, and nowhere."""
    ws = []
    for n in (5, 6, 7, 8, 12, 13, 14, 15):
        ws += [word(lp(n - 1), fill(1)), word(fill(1, 6), rs(n - 1)), word(fill(n - 2, 1), lp(2)), linf(2, n),
               word(fill(n - 3, 2), tree(0, 3))]
    return ws


def near_words():
    """For every cache key of 7..14 symbols a word of the same length that shares its first 6 (or more)
    symbols and differs only in the last one: in a tiny table it probes the key's own slot, and only
    the second half-entry compare tells the two apart."""
    ws = []
    for n in range(7, 15):
        ws += [word(lp(n - 1), fill(1, n)), word(rinf(24 - n, n - 1), fill(1, n)), word(fill(1, n), rs(n - 1))]
        if n <= 13:
            ws.append(word(n_pre(N14, n - 1), fill(1, n)))
        if n <= 8:
            ws.append(word(n_pre(N9, n - 1), fill(1, n)))
    return ws + [word(tree(0, 7), fill(1)), word(tree(8, 15), fill(1, 3))]


def edge_words():
    return form_words() + position_words() + tie_words() + tail_words() + near_words()


def _row(words):
    return " ".join(w if isinstance(w, str) else w[0] for w in words)


def _info(words):
    return [info_of(w) for w in words if not isinstance(w, str) and len(w[0]) >= 2]


def _toks(words):
    return [t for w in words for t in ([w] if isinstance(w, str) else w[1])]


def _rows(lists):
    """[[word or str, ...], ...] -> (rows, info, tokens per row)."""
    return [_row(r) for r in lists], [_info(r) for r in lists], [_toks(r) for r in lists]


def placement_lists():
    """Every edge word alone in its row at an odd index of W (after the row's <s>) and, after a
    one-symbol word, at an even one; as the first and as the last pre-token of a row with others; a
    2-symbol miss directly before a 15-symbol miss and the reverse. The batch ends in a row whose last
    pre-token is a 2-symbol miss."""
    ws = edge_words()
    rows = []
    for i, w in enumerate(ws):
        rows.append([w])
        rows.append(["7", w])
        o = ws[(7 * i + 3) % len(ws)]
        if len(w[0]) + len(o[0]) <= 120:
            rows.append([w, "7", o] if i % 2 else [o, w])
    m2, m15 = linf(3, 2), word(fill(1), rs(14))
    rows += [[m2, m15], [m15, m2], [m2, m15, m2, m15], ["7", m15, m2], [m15, "7", m2]]
    rows.append(["7", lp(14), linf(5, 2)])
    return rows


def pool_lists(total, seed):
    """One unit (at most 64 rows) whose pooled misses (2..15 symbols, not cache keys) number exactly
    `total`, lengths and merge depths mixed, cache hits and one-symbol words between them."""
    rng = np.random.default_rng(seed)
    miss = [w for w in edge_words() if 2 <= len(w[0]) < WREG and not info_of(w)[2]]
    hits = [w for w in edge_words() if info_of(w)[2]]
    nrows = min(UNIT, max(1, total // 2))
    rows = [[] for _ in range(nrows)]
    for k in range(total):
        r = rows[k % nrows]
        if rng.integers(3) == 0:
            r.append(hits[int(rng.integers(len(hits)))] if rng.integers(2) else "7")
        r.append(miss[int(rng.integers(len(miss)))])
    return rows


def maxn_lists():
    """Single units whose longest miss is 2, 4, 5, 8, 9, 12, 13 symbols (the read-back's chunk skip and
    the wave-uniform lookup skip follow the longest n of a batch): 70 misses each, so one full batch
    and a short one."""
    out = {}
    for mx in (2, 4, 5, 8, 9, 12, 13):
        cyc = [word(fill(mx - 2, 1), lp(2)), linf(2, mx), word(lp(mx - 1), fill(1)) if mx > 2 else linf(7, 2),
               linf(4, 2), word(fill(1, 3), rs(mx - 1)) if mx > 2 else word(fill(1), fill(1, 9))]
        out[mx] = [[cyc[(r + k) % 5] for k in range(7)] for r in range(10)]
    return out


def ring_lists():
    """One unit of 64 rows handing on more than POOL_RING misses (the wave's ring wraps inside the
    unit), lengths 2..15 mixed, every row short enough that a tile holds several."""
    miss = [w for w in edge_words() if 2 <= len(w[0]) < WREG and not info_of(w)[2]]
    rows = [[miss[(11 * r + 5 * k) % len(miss)] for k in range(6)] for r in range(UNIT)]
    assert sum(len(r) for r in rows) > POOL_RING
    return rows


def long_lists():
    """Pass B: tiles whose miss list holds 0, 1, 2 and 40 pre-tokens of >= 16 symbols (40 x 17 bytes: what a
    768-byte tile can hold; 65 cannot fit one), next to cache hits and pooled misses; a long one at
    indices 64 and 65 of a tile's miss list (the second step of pass B's loop); long ones of 65 and
    100 symbols (a length scan capped at 64 would cut them). `pad` rows (80 bytes, no multi-symbol
    pre-token) keep every such row in a tile of its own whatever the tile's row count."""
    pad = ["7"] * 40
    l16, l17, l24 = lp(16), rs(17), lp(24)
    rows = [pad, [lp(5), linf(2, 3), rs(14)], pad, [lp(14), l16, linf(3, 4)], pad, [l17, rs(3), linf(1, 2), l24, lp(2)], pad,
            [l16] * 40, pad, [linf(1 + k % 20, 2) for k in range(64)] + [l16, word(fill(3), rs(17)), lp(7)], pad,
            [big(65, ["R", "L", "T"]), lp(3), big(100, ["T", "L", "R", "N14", "Y"])], pad,
            [word(fill(40, 2), lp(24), fill(36))], pad, [tree(0, 16), word(linf(1, 20), lp(20))], pad]
    return rows


def scap_lists():
    """T_SCAP (240) multi-symbol pre-tokens in one tile, and 241 (the tile's rows go to the fallback
    kernels), lengths 2..7 mixed with deep merges; each such row over 700 bytes between pad rows, so it
    is alone in its tile."""
    pad = ["7"] * 40
    deep = [lp(7), word(fill(1), lp(5)), lp(4), word(lp(3), fill(1)), linf(2, 5), lp(6), yz(2), ("889", ["889"])]
    rows = []
    for cnt in (T_SCAP, T_SCAP + 1):
        r = [deep[k // 24 % len(deep)] if k % 24 == 0 else (lp(2) if k % 3 == 0 else linf(1 + k % 22, 2)) for k in range(cnt)]
        assert 700 < len(_row(r).encode()) <= T_BCAP
        rows += [pad, r]
    return rows + [pad]


NFC_TAIL = "\u0928\u094d\u093c\u093e"   # a nukta after a virama: NFC reorders, the row goes to the fallback waves


def sample_lists(kind, n=300, seed=5):
    """A sample of rows of edge words: "nfc" (NFC changes the row elsewhere: the fallback waves'
    bpe_tile<..., NFCD>), "over" (rows over 768 bytes: the one-lane kernel's bpe_merge_word), "host" (the
    per-call path)."""
    rng = np.random.default_rng(seed)
    ws = edge_words()
    rows = []
    for i in range(n):
        k = {"nfc": 5, "over": 60, "host": 4}[kind]
        r = [ws[int(x)] for x in rng.integers(len(ws), size=k)]
        if kind == "nfc":
            r.insert(int(rng.integers(len(r) + 1)), NFC_TAIL)
        rows.append(r)
    if kind == "over":
        rows = [r for r in rows if len(_row(r).encode()) > T_BCAP]
        assert len(rows) > 0.9 * n
    return rows


def merge_rows():
    """{name: (rows, info, tokens)} of every list; `tokens` are the stated merge_all results as token
    strings per row (without <s> </s>; None for the rows with an NFC tail, whose stray chars the
    vocabulary does not hold)."""
    out = {"place": _rows(placement_lists()), "near": _rows([[w, "7", w] for w in near_words()]), "ring": _rows(ring_lists()), "long": _rows(long_lists()),
           "scap": _rows(scap_lists())}
    for t in (1, 63, 64, 65, 127, 128, 129):
        out["pool%d" % t] = _rows(pool_lists(t, 100 + t))
    for mx, rows in maxn_lists().items():
        out["maxn%d" % mx] = _rows(rows)
    for kind in ("nfc", "over", "host"):
        out[kind] = _rows(sample_lists(kind))
    return out


TILE_LISTS = ["place", "near", "ring", "long", "scap"] + ["pool%d" % t for t in (1, 63, 64, 65, 127, 128, 129)] + \
             ["maxn%d" % m for m in (2, 4, 5, 8, 9, 12, 13)]


def expected_counters(rows, info):
    """What the tile kernel's counters must read for a list with the default cache table (every key
    stored): rows over the tile buffer and the rows of a tile with more than T_SCAP multi-symbol
    pre-tokens (here always alone in their tile) are not probed."""
    probes = hits = misses = lanes = fb = nlong = 0
    for r, inf in zip(rows, info):
        if len(r.encode()) > T_BCAP or len(inf) > T_SCAP:
            fb += 1
            continue
        for n, k, key in inf:
            probes += 1
            hits += key
            if not key and n < WREG:
                misses += 1
                lanes += n - k
            nlong += n >= WREG
    return {"probes": probes, "hits": hits, "misses": misses, "lane_rounds": lanes, "fallback": fb, "long": nlong}


# ------------------------------------------------------------------------------------------ real model
def real_sets(bpe_model):
    """models/akshar.json: "pairs" = every ordered pair of its single-character word tokens as a
    2-character word (present and absent merges: every flagged first slot an absent pair can hit in
    merge_lookup_c); "merges" = for every merge the word left + right (every key at its second choice
    in the compact table, every cache key). 32 words per row. -> {name: list of rows of words}"""
    single = [t for t in bpe_model.vocab if len(t) == 1]
    single.sort(key=lambda t: bpe_model.vocab[t])
    pairs = [a + b for a in single for b in single]
    inv = bpe_model.id_to_token
    mg = [inv[int(a)] + inv[int(b)] for a, b, _ in bpe_model.merges.tolist()]
    return {"pairs": [pairs[i:i + 32] for i in range(0, len(pairs), 32)],
            "merges": [mg[i:i + 32] for i in range(0, len(mg), 32)]}


def golden():
    with gzip.open(GOLDEN, "rt", encoding="ascii") as f:
        return json.load(f)
