"""Rows for the fallback waves' NFC (ak_nfc_wave.h) at the edges of its own loops: the 16-code-point
segment cap of nfc_seg, the 64-segment chunks of nfc_flush_batch, the 64-char steps of the segment
pass, the block copy, batch prefixes and text reserve of nfc_epoch_gather, and the rounds, map and
elongation steps of hf_epoch_gather. Plain data: generators, no tests. Shared by
tests/test_emu_nfc_wave.py (the host emulator) and tests/test_gpu_nfc_wave.py (the device);
tools/gen_golden_nfc_wave.py records the reference's answers for the distinct valid rows in
tests/golden/nfc_wave_edges.jsonl.gz.

A row is (bytes, fate): "wave" = the fallback waves finish its NFC, "one_lane" = they pass it on. The
builder states the fate it intends; fate_of() computes it from the rules ak_nfc_wave.h documents
(invalid UTF-8, over NW_MAXB = 768 bytes, a segment whose full canonical decomposition passes
NW_DCAP = 16 code points), never from a counter, and the self-check compares the two. What a wave
finishes after the NFC depends on the kernel that calls it; those further rules are finishes().

A segment is [stable char, the non-stable chars after it), stable = ccc 0, NFC(c) == c, never the
second of a primary composite, no Hangul V / T (tools/gen_tables.py). So U+0929 (NFC keeps it) opens
a segment, while U+0958 (a composition exclusion: NFC(c) != c) joins the segment before it: the
"becomes two chars" kind below is "x" + U+0958, one segment of two chars that leaves as three. A
segment is trivial when it is one char that does not decompose (and no Hangul syllable); only the
others are listed, chunked and run through nfc_seg.

normalize_text keeps Devanagari, Bengali, ASCII letters and digits, whitespace and .,!?;:'"- only, so
what NFC did is read from Devanagari and Bengali witnesses; other scripts (Hangul jamo, marks of many
combining classes, "x" + U+1D160 which grows from 5 to 13 bytes) serve as pressure only and are
followed by witnesses whose text would shift if an offset were wrong. Every row carries a construct
the tile kernel does not redo itself (rows_edge_rows.NFC_CASES), so every row reaches the waves.

nfc_seg has three cap checks. m + 1 (a char that does not decompose) and m + len (one that does)
are taken to both sides of the cap below, the latter at a segment's start (seg_dbase) and at its end
(seg_dtail: U+095B, and the non-starter U+0344 which decomposes to two marks). The Hangul check
m + 3 > NW_DCAP is conservative for a two-jamo (LV) syllable, but it cannot be met near the cap: a
precomposed syllable is stable, so it always opens its segment and is decomposed at m = 0.

A row over 384 bytes is alone in its batch (two such rows pass NW_MAXB), wherever it stands in the
list and however many waves share it: alone() pads the rows whose constructs are placed by batch
char index (straddle, chunk, the HF elongation runs).
"""
import unicodedata

from tests.wide_rows import fill

NW_MAXB, NW_DCAP, NE_TCAP, NE_VMAX = 768, 16, 8192, 128
S_BCAP = 480  # ak_tile_spm.h: the SentencePiece tile variant's staged bytes (the epoch's NFC text goes through it)

NA, RA, LLA, KA, JA = "\u0928", "\u0930", "\u0933", "\u0915", "\u091c"
NNNA, RRA, LLLA, QA, ZA = "\u0929", "\u0931", "\u0934", "\u0958", "\u095b"
NUKTA, VIRAMA, ANUDATTA, UDATTA, GRAVE, ACUTE = "\u093c", "\u094d", "\u0952", "\u0951", "\u0953", "\u0954"
B_NUKTA, B_VIRAMA, B_E, B_AA, B_AU, B_KA = "\u09bc", "\u09cd", "\u09c7", "\u09be", "\u09d7", "\u0995"
B_EXCL = ("\u09dc", "\u09dd", "\u09df")
LATIN = "a\u0301\u0323"  # a, acute, dot below: reordered and composed (U+1EA1 U+0301), then dropped by the filter
TRIG = NA + VIRAMA + NUKTA  # reordered, then composed to U+0929: 9 bytes -> 6, three chars, one segment
# Heads of one byte length (9) and different results; the second opens with an ASCII letter that
# composes with the mark at the row's second byte (a row-start tag one byte late splits them)
HEADS = (TRIG, LATIN + KA + "q", LLA + VIRAMA + NUKTA)
WIT = (KA, "\u0916", "\u0917", B_KA, "\u0998")

# Marks of strictly descending combining class (230, 220, 216, 202, 36 .. 20), none composing with
# NA: every one moves in the sort. The Devanagari virama (9) and nukta (7) go last, so the visible
# result opens with U+0929.
DESC = ("\u0951", "\u0952", "\u031b", "\u0321", "\u0711", "\u0670", "\u0652", "\u0651", "\u0650", "\u064f",
        "\u064e", "\u064d", "\u064c", "\u064b", "\ufb1e", "\u05c2", "\u05c1", "\u05bf", "\u05bd", "\u05bb")
DCAP_N = (14, 15, 16, 17, 18)


# ---------------------------------------------------------------- the rules
_SECOND = None


def _seconds():
    global _SECOND
    if _SECOND is None:
        s = set(range(0x1161, 0x1176)) | set(range(0x11A8, 0x11C3))
        for c in range(0x110000):
            if 0xAC00 <= c <= 0xD7A3 or 0xD800 <= c <= 0xDFFF:
                continue
            d = unicodedata.decomposition(chr(c))
            if d and not d.startswith("<"):
                p = d.split()
                if len(p) == 2 and unicodedata.normalize("NFC", chr(int(p[0], 16)) + chr(int(p[1], 16))) == chr(c):
                    s.add(int(p[1], 16))
        _SECOND = s
    return _SECOND


def is_stable(ch):
    return unicodedata.combining(ch) == 0 and unicodedata.normalize("NFC", ch) == ch and ord(ch) not in _seconds()


def segments(text):
    """The NFC segments of one row: its first char and every stable char open one."""
    segs = []
    for i, ch in enumerate(text):
        if i == 0 or is_stable(ch):
            segs.append(ch)
        else:
            segs[-1] += ch
    return segs


def dlen(seg):
    """Code points of the segment's full canonical decomposition."""
    return len(unicodedata.normalize("NFD", seg))


def trivial(seg):
    return len(seg) == 1 and dlen(seg) == 1


def is_valid(row):
    try:
        row.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def fate_of(row):
    if not is_valid(row) or len(row) > NW_MAXB:
        return "one_lane"
    return "one_lane" if any(dlen(s) > NW_DCAP for s in segments(row.decode("utf-8"))) else "wave"


def nfc_bytes(row):
    return len(unicodedata.normalize("NFC", row.decode("utf-8")).encode("utf-8"))


def hf_text(norm):
    """normalize_text's output as HF's normalizer takes it before its NFC: compat spaces -> ' '."""
    return "".join(" " if c.isspace() and unicodedata.normalize("NFKC", c) == " " else c for c in norm)


def hf_changes(norm):
    t = hf_text(norm)
    return unicodedata.normalize("NFKC", t) != t


def hf_segments(norm):
    """The HF text's segments (hf_epoch_gather: at ccc 0 chars that are no composition second; over
    the alphabet normalize_text keeps, HF's combining classes are zero where Unicode's are)."""
    segs = []
    for i, ch in enumerate(hf_text(norm)):
        if i == 0 or (unicodedata.combining(ch) == 0 and ord(ch) not in _seconds()):
            segs.append(ch)
        else:
            segs[-1] += ch
    return segs


def finishes(row, kind, rec):
    """Whether the fallback waves finish the row for `kind` ("rows", "spm", "bpe"): its fate is "wave"
    and none of the caller's further documented rules sends it on. `rec` is the reference's record.
      all   the epoch's tile takes the NFC text only within its byte buffer (768; SentencePiece's tile
            variant 480), and the result must fit the row's fallback slot: cnt > mul * len + 2 goes on
            (BPE mul 1, SentencePiece mul 2; the row ops: the normalized bytes within 2 len + 1)
      bpe   a row HF's NFKC changes runs hf_epoch_gather, where a HF segment past 16 fails"""
    if fate_of(row) != "wave":
        return False
    n = len(row)
    if kind == "rows":
        return nfc_bytes(row) <= NW_MAXB and len(rec["norm"].encode("utf-8")) <= 2 * n + 1
    if kind == "spm":
        return nfc_bytes(row) <= S_BCAP and len(rec["spm"]) <= 2 * n + 2
    if nfc_bytes(row) > NW_MAXB or len(rec["bpe"]) > n + 2:
        return False
    return not (hf_changes(rec["norm"]) and any(dlen(s) > NW_DCAP for s in hf_segments(rec["norm"])))


def _rows(texts, fate="wave"):
    return [(t if isinstance(t, bytes) else t.encode("utf-8"), fate) for t in texts]


# ---------------------------------------------------------------- dcap
def seg_desc(n):
    """NA + n - 1 marks of strictly descending class: n decomposed code points."""
    return NA + "".join(DESC[:n - 3]) + VIRAMA + NUKTA


def seg_equal(n):
    """NA + marks of class 230 (their order must stay), then the virama and nukta that pass them all."""
    return NA + "".join((UDATTA, GRAVE, ACUTE)[i % 3] for i in range(n - 3)) + VIRAMA + NUKTA


def seg_dbase(n, base=NNNA):
    """A base that decomposes to two (U+0929; U+095B after the row's first char joins it): n - 1
    chars of input, n decomposed."""
    return base + "".join((UDATTA, ANUDATTA, GRAVE)[i % 3] for i in range(n - 4)) + VIRAMA + B_NUKTA


def seg_dtail(n, tail):
    """NA + marks + a last char that decomposes to two (U+095B, U+0344): the m + len check at the
    segment's end, n decomposed code points from n - 1 chars."""
    return NA + "".join((UDATTA, GRAVE, ACUTE)[i % 3] for i in range(n - 5)) + VIRAMA + NUKTA + tail


DTAILS = (ZA, "\u0344")


def seg_marks(n):
    """n non-starters (for a row's start: a leading non-starter blocks composition)."""
    return "".join((UDATTA, VIRAMA, ANUDATTA, NUKTA)[i % 4] for i in range(n))


def seg_jamo(n):
    """L + V + T, then V / T: n code points, the first three compose."""
    return "\u1100\u1161\u11a8" + "".join("\u1162\u11a9"[i % 2] for i in range(n - 3))


BLOCKED = (NA + B_NUKTA + NUKTA,            # the Devanagari nukta behind one of its own class: blocked
           NA + VIRAMA + NUKTA,             # behind a higher class: sorted in front, composed
           NA + UDATTA + VIRAMA + B_NUKTA + NUKTA + ANUDATTA,  # sorted, then blocked by the Bengali nukta
           B_E + B_VIRAMA + B_AA,           # a starter second behind a mark: blocked
           B_E + B_AA + B_VIRAMA, B_E + B_AU, RA + ACUTE + NUKTA + UDATTA)


def dcap_rows():
    good = [TRIG + " " + KA + VIRAMA + KA, RA + VIRAMA + NUKTA + "ok", LATIN + " " + B_KA + B_E + B_AA]
    out = []
    for n in DCAP_N:
        f = "wave" if n <= NW_DCAP else "one_lane"
        for i, seg in enumerate((seg_desc(n), seg_equal(n), seg_dbase(n), seg_dbase(n - 1, "z" + ZA))):
            assert dlen(seg) == n, (n, i)
            out += _rows([seg], f)                                           # alone in its row
            out += _rows([good[i % 3]]) + _rows([fill(5, n) + " " + WIT[i] + seg], f) + _rows([good[(i + 1) % 3]])
            out += _rows([TRIG + seg + LLA + NUKTA + UDATTA + " " + WIT[i]], f)  # the middle of three
    for n in (15, 16, 17):
        f = "wave" if n <= NW_DCAP else "one_lane"
        out += _rows([seg_marks(n) + KA + " " + TRIG], f)
        out += _rows([good[0]]) + _rows([seg_marks(n) + B_KA + B_E + B_AA + TRIG], f) + _rows([good[1]])
        out += _rows([seg_jamo(n) + " " + TRIG + WIT[2]], f)
        out += _rows([WIT[1] + TRIG + seg_jamo(n)], f) + _rows([good[2]])
        out += _rows([TRIG + seg_jamo(n) + NA + NUKTA + WIT[3]], f)
    for n in (16, 17):
        f = "wave" if n <= NW_DCAP else "one_lane"
        for i, tail in enumerate(DTAILS):
            out += _rows([seg_dtail(n, tail) + " " + WIT[i], WIT[i + 2] + " " + TRIG + seg_dtail(n, tail) + KA + VIRAMA], f)
    out += _rows(["\uac00" + seg_marks(13)[1:] + KA + TRIG, TRIG + "\uac01" + "\u11a9" * 12 + WIT[0]])  # syllables: decomposed at m = 0
    out += _rows(["".join(BLOCKED), " ".join(BLOCKED[::-1]), BLOCKED[2] + BLOCKED[0] + TRIG])
    out += _rows([e + NUKTA + TRIG for e in B_EXCL] + ["".join(chr(c) for c in range(0x958, 0x960)) + TRIG])
    return out


# ---------------------------------------------------------------- chunk
CHUNK_N = (63, 64, 65, 127, 128, 129, 130, 192, 193)
CHUNK_K = (0, 1, 62, 63, 64, 65)


def chunk_seg(i):
    """The i-th non-trivial segment: U+0929 / U+0931 / U+0934 (stay), "x" + U+0958 (two chars leave as
    three) at i = 3 mod 8, NA + nukta (two leave as one) at i = 6 mod 8: a slot off by s shows unless
    24 divides s."""
    return "x" + QA if i % 8 == 3 else NA + NUKTA if i % 8 == 6 else (NNNA, RRA, LLLA)[i % 3]


def alone(t):
    """t padded with ASCII words past 384 bytes: alone in its batch."""
    i = 0
    while len(t.encode("utf-8")) <= NW_MAXB // 2:
        t += " " + fill(7, i)
        i += 1
    return t


def chunk_row(n, k, gap=0):
    """k trivial chars, then n non-trivial segments (the last one TRIG) with `gap` trivial chars
    before each; alone in its batch."""
    segs = [chunk_seg(i) for i in range(n - 1)] + [TRIG]
    return alone(fill(k, n) + "".join(fill(gap, i) + s for i, s in enumerate(segs)))


def chunk_rows():
    out = [chunk_row(n, k) for n in CHUNK_N for k in CHUNK_K]
    out += [chunk_row(n, 0, gap) for gap in (1, 2) for n in (63, 64, 65, 127, 128, 129)]
    assert all(len(r.encode("utf-8")) <= NW_MAXB for r in out)
    return _rows(out)


def count_nontrivial(text):
    return sum(not trivial(s) for s in segments(text)), next(i for i, s in enumerate(segments(text)) if not trivial(s))


# ---------------------------------------------------------------- straddle
STRADDLE_AT = (61, 62, 63, 64)
STRADDLE_SEGS = (NA + UDATTA + VIRAMA + NUKTA, RA + ANUDATTA + VIRAMA + NUKTA, B_KA + UDATTA + B_VIRAMA + B_NUKTA)


def straddle_row(k, seg):
    """The segment's four chars at char indices k .. k + 3 of its batch (the row is alone in it)."""
    return alone(TRIG + fill(k - 3, k) + seg + " " + KA)


def straddle_rows():
    return _rows([straddle_row(k, s) for k in STRADDLE_AT for s in STRADDLE_SEGS])


# ---------------------------------------------------------------- uniform
UNIFORM_P = 3
ODD_L = tuple(range(9, 50, 2))


def uniform_row(L, j):
    """Row j of the list of byte length L: a head of 9 bytes, Devanagari / Bengali witnesses that cycle
    with j, ASCII to the length (words of at most 9 letters)."""
    t = HEADS[j % UNIFORM_P]
    rest = L - 9
    nw = min(rest // 3, 4 + rest // 40)
    t += "".join(WIT[(j + i) % len(WIT)] for i in range(nw))
    rest -= 3 * nw
    while rest > 0:
        w = min(rest, 10)
        t += (" " if w > 1 else "") + fill(w - 1 if w > 1 else 1, j + rest)
        rest -= w
    assert len(t.encode("utf-8")) == L, (L, j)
    return t


def uniform(L, periods=1):
    return _rows([uniform_row(L, j) for j in range(UNIFORM_P)] * periods)


def markstart_row(j):
    """16 chars, 30 bytes, opening with a mark: four rows fill a 64-char step, so every fourth row of
    a batch opens at lane 0 right after a row that ends at lane 63. A list of these rows alone (a call
    of its own) gives every wave batches of 25 such rows (750 bytes), whichever rows it draws."""
    t = (NUKTA, VIRAMA, UDATTA)[j % 3] + WIT[j % 5] + HEADS[2 * (j % 2)] + fill(9, j) + NA + NUKTA
    assert len(t) == 16 and len(t.encode("utf-8")) == 30
    return t


def markstart(periods=1):
    return _rows([markstart_row(j) for j in range(6)] * periods)


def long_among_short(periods=1):
    """A 769-byte row (passed on, no bytes in the batch) after every three 20-byte rows."""
    unit = _rows([uniform_row(20, j) for j in range(3)]) + _rows([TRIG + fill(760)], "one_lane")
    assert len(unit[3][0]) == NW_MAXB + 1
    return unit * periods


def reserve_rows(L, n):
    """n rows of L bytes (681: four rows' 3 B + 16 fit the text reserve; 682: the fourth does not)."""
    return _rows([uniform_row(L, j) for j in range(n)])


# ---------------------------------------------------------------- expand
def expand_rows():
    """"a".."z" + U+1D160 (5 bytes -> 13: every segment triples) at the densest the row allows, then
    witness rows in the same epoch. The NFC text of the dense rows passes every tile buffer, so the
    epoch's tile sends them on; the witnesses must come through untouched."""
    def dense(nbytes, s):
        t = "".join(chr(97 + (i + s) % 26) + "\U0001d160" for i in range(nbytes // 5))
        return t + fill(nbytes - len(t.encode("utf-8")), s)
    out = []
    for i, nb in enumerate((768, 765, 300, 100, 50, 768, 150)):
        out += _rows([dense(nb, i)])
        out += _rows([uniform_row(25, i), TRIG + WIT[i % 5] + " ok"])
    out += _rows([TRIG + dense(45, 1) + WIT[0], WIT[1] + dense(20, 2) + TRIG + dense(20, 3) + WIT[2]])
    return out


# ---------------------------------------------------------------- hf (BPE)
HF_HEADS = (NA + "\x01" + NUKTA, RA + "\x02" + NUKTA, LLA + "\x07" + NUKTA)  # HF's NFKC composes what normalize_text leaves


HF_EPOCH_N = (63, 64, 65, 127, 128)


def hf_head(j):
    """Cycles with period 9, so rows j, j + 3, ... (a wave's share of three) still differ."""
    return HF_HEADS[(j + j // 3) % 3]


def hf_short(n):
    """n rows of 7 bytes whose normalize_text output HF's NFKC changes. A call of n * waves such rows
    gives every wave one epoch of exactly n HF rows (n <= 128; their bytes are far below the text
    reserve), taken 64 list entries at a time."""
    return _rows([hf_head(j) for j in range(n)])


HF_GROW_RAW, HF_GROW_NFC = 19, 43


def hf_grow(n):
    """n rows of 19 bytes that HF's NFKC changes and whose NFC text is 43 bytes (three U+1D160, 4 bytes
    each, leave as 12; normalize_text then drops them). 128 of them fit one epoch's text reserve as
    raw bytes, so a call of 128 * waves rows gives every wave an epoch of 128 HF rows whose NFC text
    (5,504 bytes) is over twice the reserve of a HF round (2,725 bytes): the first round takes 63
    rows and hf_rest_down moves 65 down (both entries of lane 0), the second 63, the third 2."""
    return _rows([hf_head(j) + "\U0001d160" * 3 for j in range(n)])


def hf_long(n, L=681):
    """HF rows of L bytes: the NFC epoch holds four of 681 (nfc_epoch_gather's reserve); their NFC text
    is no longer than the raw text, so the HF round takes all of them at once."""
    return _rows([HF_HEADS[j % 3] + uniform_row(L - 7, j) for j in range(n)])


HF_RUN_AT = (59, 60, 61, 62, 63, 64)


def hf_elong_row(at, run):
    """A run of `run` equal letters, a dropped control char inside, from mapped-char index `at` of
    its HF batch; over 384 bytes, so the row is alone in that batch."""
    body = HF_HEADS[0] + fill(at - 2, at) + "z" + "\x01" + "z" * (run - 1) + " " + KA + " "
    return body + " ".join(fill(7, i) for i in range(50))


def hf_rows():
    """The HF rows that need no epoch of their own (the epoch-count and round lists run as calls of
    their own: hf_short, hf_grow)."""
    out = hf_short(20) + _rows([TRIG + " x"]) + hf_long(4) + hf_long(5)
    out += _rows([hf_elong_row(at, run) for at in HF_RUN_AT for run in (3, 4, 5, 6)])
    marks = "".join((UDATTA, GRAVE, ACUTE)[i % 3] for i in range(16))  # one class, no two neighbours equal: nothing collapses
    # HF segments of 15, 16 and 17 code points (the control char between is dropped); the last one's
    # NFC segments stay short (8 and 10), so only hf_epoch_gather can fail it
    out += _rows([NA + "\x01" + NUKTA + marks[:13] + " " + KA, NA + "\x01" + NUKTA + marks[:14] + " " + KA,
                  NA + marks[:7] + "\x01" + NUKTA + marks[7:15] + " " + KA, NA + marks[:7] + "\x01" + NUKTA + marks[7:14] + KA])
    return out


# ---------------------------------------------------------------- the lists
INVALID = (b"\x80abc", b"ab\xe0\xa4", TRIG.encode() + b"\xc3(")


def emu_uniform_rows():
    """The uniform lists as the emulator runs them, one after the other: six rows of every odd length
    (the block copy's start and end alignments), 130 rows of 12, of 13 and of 9 bytes (the 64-entry
    prefix at exactly 768 bytes and one over; the 128-row epoch), four and
    five rows of 681 and of 682 bytes, the 769-byte row among short ones, rows of exactly 768."""
    out = []
    for L in ODD_L:
        out += uniform(L, 2)
    for L in (12, 13, 9):
        out += uniform(L, 44)[:130]
    out += reserve_rows(681, 5) + reserve_rows(682, 4) + long_among_short(3) + uniform(768, 1)
    for i, bad in enumerate(INVALID):
        out.insert(40 + 97 * i, (bad, "one_lane"))
    return out


def families():
    """name -> rows, as the emulator runs them."""
    return {"dcap": dcap_rows(), "chunk": chunk_rows(), "straddle": straddle_rows(), "uniform": emu_uniform_rows(),
            "expand": expand_rows(), "hf": hf_rows()}


def device_uniform_lists():
    """name -> (one period, rows per wave the list needs) for the device test."""
    lists = {"L%d" % L: (uniform(L), 128) for L in ODD_L + (12, 13)}
    lists["markstart"] = (markstart(), 128)
    lists["long"] = (long_among_short(), 128)
    lists["L681"] = (reserve_rows(681, 3), 6)
    lists["L682"] = (reserve_rows(682, 3), 6)
    lists["L768"] = (uniform(768), 4)
    lists["hf7"] = (hf_short(9), 128)
    lists["hf681"] = (hf_long(3), 6)
    lists["hfgrow"] = (hf_grow(9), 128)
    return lists


def distinct_valid_rows():
    """Every distinct valid row of the families and the device lists, in a fixed order."""
    seen, out = set(), []
    groups = list(families().values()) + [rows for rows, _ in device_uniform_lists().values()]
    for rows in groups:
        for r, _ in rows:
            if r not in seen and is_valid(r):
                seen.add(r)
                out.append(r)
    return out


def golden():
    """The reference's records (tools/gen_golden_nfc_wave.py) by row bytes."""
    import gzip
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nfc_wave_edges.jsonl.gz")
    with gzip.open(path, "rt", encoding="utf-8") as f:
        return {r["text"].encode("utf-8"): r for r in map(json.loads, f)}
