"""Rows that put every construct the row-op tile kernel (ak_tile_rows.h rows_tile: normalize, segment,
switches, the fused analyze) carries across its 64-element sweep steps on the last element of a step,
on the first of the next and mid-step, and rows at the limits of the SentencePiece tile kernel
(ak_tile_spm.h). Plain data: generators, no tests. Shared by tests/test_emu_rows_edges.py (the host
emulator) and tests/test_gpu_rows_edges.py (the device); tools/gen_golden_rows_edges.py records the
reference's answers for the valid rows in tests/golden/rows_edges.jsonl.gz.

V, the array the sweep runs over, holds per row of a tile its V_B, one entry per char normalize_text
keeps (before the elongation collapse; a precomposed nukta letter takes two) and its V_E, the rows
back to back. In a one-row tile the char after fill(k - 1) therefore sits at V index k; at() places a
construct there. Tiles of several rows shift the rows behind the first, so the shape units below,
which need a row mark at a chosen index, are laid out for tiles of 4 and of 16 rows alike.

Alphabet: what normalize_text keeps (U+0900-U+09FF, ASCII letters and digits, \\s, .,!?;:'"-), or
the rows would test the filter, not the sweep. Every char that passes that filter has a grapheme
class the tile implements (Other, CR, LF, Control, Extend, SpacingMark: the fixture's generator lists
them with the table generator's method and the emulator test checks the list), so for the
normalize_text defaults no row can make rows_tile run its second sweep. The fallback waves' epoch
text (NFCD) passes the same filter in the tile's front end before the sweep sees it, so a raw row
with other scripts (Hangul jamo, regional indicators) does not reach that branch either: nothing
the tile path serves can, and no row here is built for it.
"""
import unicodedata

from tests.wide_rows import fill

STEP = 64
POS = (30, 61, 62, 63, 64, 65, 66, 125, 126, 127, 128, 129, 130)  # V index of a construct's first element
POS_FEW = (30, 62, 63, 64, 127, 128)                               # ... for the long constructs
R_BCAP = 768   # ak_tile_rows.h R_BCAP: staged bytes per tile; a row over it takes the fallback kernels
TAIL = "q" + fill(3)

KA, SSA, VIRAMA, NUKTA = "क", "ष", "्", "़"
U, ANUSVARA, AA, I, VISARGA, E = "ु", "ं", "ा", "ि", "ः", "े"
B_KA, B_SSA, B_VIRAMA, B_NYA, B_CA, B_O, B_KHA = "ক", "ষ", "্", "ঞ", "চ", "ো", "খ"


def at(k, construct, tail=TAIL):
    """A row whose construct starts at V index k of a one-row tile."""
    return fill(k - 1, shift=k) + construct + tail


def extends(n):
    """n alternating ccc-0 Extends (no elongation run, nothing for NFC to reorder)."""
    return (U + ANUSVARA) * (n // 2) + (U if n & 1 else "")


def neutrals(n):
    """n chars detect_code_switches treats as neutral (digits, punctuation, spaces), no two equal
    neighbours."""
    return "".join("1 2,3.4;5-"[i % 10] for i in range(n))


def gb9c_rows():
    """Conjuncts over the step edge: consonant | linker | consonant at every split, Extends between,
    a doubled linker, breakers that must break, Bengali; then a linker and a second consonant one
    and two whole steps after the consonant (the carries of steps without a breaker), with and
    without a nukta right after the first consonant."""
    short = [KA + VIRAMA + SSA, KA + VIRAMA + U + ANUSVARA + SSA, KA + U + VIRAMA + SSA, KA + VIRAMA + VIRAMA + SSA,
             KA + VIRAMA + "a" + SSA, KA + VIRAMA + " " + SSA, KA + NUKTA + VIRAMA + SSA,
             B_KA + B_VIRAMA + B_SSA, B_NYA + B_VIRAMA + B_CA, KA + VIRAMA + SSA + VIRAMA + KA + VIRAMA + SSA,
             KA + VIRAMA + "\n" + SSA, KA + AA + VIRAMA + SSA]
    rows = [at(k, c) for k in POS for c in short]
    for k in POS_FEW:
        for n in (70, 134):
            for first in (KA, KA + NUKTA):
                rows.append(at(k, first + extends(n) + VIRAMA + extends(2) + SSA + AA))
                rows.append(at(k, first + extends(n) + SSA))                           # no linker: must break
                rows.append(at(k, first + VIRAMA + extends(n) + SSA))                  # the linker right away
                rows.append(at(k, first + VIRAMA + extends(70) + "a" + extends(n - 64) + SSA))  # a breaker since
    return rows


def mark_rows():
    """GB9 / GB9a and the matras split: base | Extend, base | SpacingMark, two different matras, a
    precomposed two-part vowel, over the edge; rows that end in a matra (V_E one element on: the
    fin rule) and rows of matras only."""
    cons = [KA + U, KA + AA, KA + I, KA + VISARGA, B_KA + B_O, KA + AA + E, KA + I + VISARGA, KA + U + ANUSVARA,
            KA + VIRAMA, "a" + AA, AA + I, "1" + U]
    rows = [at(k, c) for k in POS for c in cons]
    rows += [at(k, c, tail="") for k in POS for c in (KA + AA, KA + AA + I, KA, KA + VIRAMA, "a")]
    rows += [AA, AA + I + E, (AA + I) * 40, (AA + I + VISARGA) * 43, U, VIRAMA + VIRAMA]
    return rows


def control_rows():
    """GB3 - GB5: CR | LF, LF | CR, CR CR LF, a char | LF, LF | Extend, the other controls the filter
    keeps, and four newlines (exempt from the collapse) over the edge."""
    cons = ["\r\n", "\n\r", "\r\r\n", "x\n", "\n" + U, "\r" + AA, "\t", "\x85", "\u2028", "\u2029", "\n\n\n\n",
            "\t\t\t", KA + "\r\n" + U, "\x0b\x0c", "\x1c\x1f"]
    rows = [at(k, c) for k in POS for c in cons]
    rows += [at(k, c, tail="") for k in POS_FEW for c in ("\r\n", "\n", "\r")]
    return rows


def elongation_rows():
    """Runs of 3 .. 6 equal chars and a run of 130 starting at every position (the kept element is
    the last of a step, the first of the next or a whole step behind the next kept char), runs of
    matras and viramas after a consonant (the collapse under GB9c), runs that end the row."""
    runs = ["zzz", "zzzz", "zzzzz", "zzzzzz", "z" * 130, "zzyyy", KA + VIRAMA * 5 + SSA, KA + AA * 4, KA + AA * 4 + I,
            KA * 3 + VIRAMA + SSA, KA + VIRAMA + SSA * 3 + AA, "   ", "111" + KA, KA + "..." + "a", "zz" + "\n" * 3 + "zz"]
    rows = [at(k, c) for k in POS for c in runs]
    rows += [at(k, c, tail="") for k in POS for c in ("zzz", "z" * 66, KA + AA * 3, KA + VIRAMA * 3)]
    rows += [at(k, "z" * 65 + KA + VIRAMA + "z" * 70 + SSA) for k in POS_FEW]
    return rows


SCRIPTS = (("ab", KA + SSA), (KA + SSA, B_KA + B_KHA), (B_KA + B_KHA, "ab"), (KA, "\n"), ("\t", KA))


def script_rows():
    """Script-run boundaries over the edge, and with 1, 63, 64, 65 and 130 neutral chars between (the
    boundary's label comes from a carry one or two steps old); rows of neutrals only (label 255 at
    V_E); rows whose first non-neutral char is in their third step, two of them back to back, so the
    second must not inherit the first's script."""
    rows = [at(k, a + b) for k in POS for a, b in SCRIPTS]
    for k in POS_FEW:
        for n in (1, 63, 64, 65, 130):
            rows += [at(k, a + neutrals(n) + b) for a, b in SCRIPTS[:3]]
    rows += [neutrals(n) for n in (1, 5, 62, 63, 64, 126, 127, 200)]
    rows += [neutrals(140) + KA, neutrals(140) + "a", neutrals(140) + B_KA, neutrals(130), neutrals(129) + "a" + neutrals(70)]
    rows += [at(k, neutrals(70), tail="") for k in POS_FEW]   # a row that ends in a step of neutrals
    return rows


def length_rows():
    """Rows of two and of four steps, one entry either side, and a row of exactly the tile buffer."""
    rows = [fill(c, shift=c) for c in (61, 62, 63, 125, 126, 127, 253, 254, 255)]
    rows += [(KA + VIRAMA + SSA + AA + " ab ") * 48, ("ab " * 256)[:R_BCAP]]
    return rows


OVER_BUFFER = [("cd " * 257)[:R_BCAP + 1], (KA + VIRAMA + SSA + " ") * 80]  # 769 and 800 bytes: the fallback kernels

_SHORT = ["aaj " + KA + VIRAMA + SSA + AA, "ok", KA + I + " 12", "yaar!!", B_KA + B_O + " x", "a\r\nb", "12 " + KA,
          "zzz " + KA + AA, "q", KA + VIRAMA, "hi " + B_NYA + B_VIRAMA + B_CA, "."]


def _unit16(block, last=None):
    """16 rows for one tile: the 4-row block, then short rows (under 768 bytes in all)."""
    rows = list(block) + _SHORT[:16 - len(block)]
    if last is not None:
        rows[15] = last
    assert len(rows) == 16 and sum(len(r.encode()) for r in rows) <= R_BCAP
    return rows


def shape_units():
    """Whole 64-row units, each four 16-row tiles that open with a 4-row block (so tiles of 4 and of
    16 rows both start on it): a row's V_B as the last element of a step with its chars in the next
    one, a row's V_E as the first element of a step, an empty row at both places, a tile whose last
    row is empty; then 16 rows of 48 bytes in one tile (every step holds a V_B, every row's outputs
    start from M.base), and a unit of 64 one-char rows."""
    conj = KA + VIRAMA + SSA + AA
    u1 = (_unit16([fill(61), conj + " ab", "", AA + I]) +              # V_B at 63, chars from 64
          _unit16([fill(63, 1), "", KA + I, ""]) +                      # V_E at 64; then an empty row at 65 / 66
          _unit16([fill(60, 2), "", conj, "x"]) +                       # the empty row's V_B at 62, V_E at 63
          _unit16([fill(61, 3), "", U + conj, "12"], last=""))          # ... V_B at 63, V_E at 64; the tile ends empty
    u2 = (_unit16([fill(125), KA + SSA, "", "a"]) +                     # the same at the second edge
          _unit16([fill(127, 1), "", B_KA + B_O, ""]) +
          _unit16([neutrals(61), KA, "", "b"]) +                        # the row before it ends neutral: no script carried over
          _unit16([fill(62, 4), VIRAMA + SSA, AA, "1"], last=""))      # V_E at 63, V_B at 64: a linker opens the row
    w48 = ["namaste " + conj + " 12 " + KA + I + " ok!!", KA + AA + " " + B_KA + B_O + " abcd 1234 yaar..",
           "zzzz " + conj + VIRAMA + SSA + " q\r\nr 9", "hello   world " + KA + VIRAMA + " " + SSA + U + ANUSVARA]
    u3 = []
    for i in range(16):
        r = w48[i % 4]
        r = (r + fill(48, i))[:48 - (len(r.encode()) - len(r))]
        assert len(r.encode()) <= 48
        u3.append(r)
    assert sum(len(r.encode()) for r in u3) <= R_BCAP
    u3 = u3 * 4
    u4 = [("abcdefg" + KA + "1 ." + SSA + "\n" + AA)[i % 14] for i in range(64)]
    units = u1 + u2 + u3 + u4
    assert len(units) % STEP == 0
    return units


def interleave(groups):
    """Round-robin over the groups, so tiles of several rows mix them."""
    out, i = [], 0
    while any(i < len(g) for g in groups):
        out += [g[i] for g in groups if i < len(g)]
        i += 1
    return out


def tile_rows():
    """Every row built to stay in the tile kernel (valid, NFC already, at most 768 bytes)."""
    return shape_units() + interleave([gb9c_rows(), mark_rows(), control_rows(), elongation_rows(), script_rows(),
                                       length_rows()])


def all_rows():
    """tile_rows() with the rows over the tile buffer spread between them, as UTF-8 bytes."""
    rows = tile_rows()
    for i, r in enumerate(OVER_BUFFER):
        rows.insert(4 * STEP + 7 + 150 * i, r)
    return [r.encode("utf-8") for r in rows]


def leaves_the_tile(row):
    """A row of all_rows() / nfc_rows() the tile kernel must hand on: over its buffer, invalid UTF-8,
    or changed by NFC in a way the tile does not redo itself (every NFC case below is of that kind)."""
    try:
        t = row.decode("utf-8")
    except UnicodeDecodeError:
        return True
    return len(row) > R_BCAP or unicodedata.normalize("NFC", t) != t


def is_valid(row):
    try:
        row.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


# One NFC-changing element per row. The tile kernel redoes the simple cases in place (a decomposed
# nukta letter that composes, a two-part vowel sign typed as its parts, a Latin base + one mark, two
# marks in the wrong order: such rows never leave it), so each case here is one it hands on, and the
# row comes back as the fallback waves' epoch text (rows_tile<OPS, NFCD = true>):
NFC_CASES = ("\u0928\u094d\u093c",              # NA, virama, nukta: reordered, then composed to U+0929
             "\u09a1\u0951\u09cd\u09bc \u0995\u09c7\u09be",  # three marks out of order (ccc 230, 9, 7); a two-part vowel as its parts
             "a\u0301\u0323",                   # a Latin base + two marks: reordered, composed, then dropped by the filter
             "\u0915\u0951\u094d\u093c",        # three marks out of order: beyond the in-tile swap
             "\u00e9\u0323")                    # a precomposed Latin letter + a mark below: recomposed (U+1EB9 U+0301)
INVALID = (b"\x80abc", b"ab\xe0\xa4", b"\xc3(", b"a\x80b " + KA.encode(), b"\xe0\xa4\x95\x80\xe0\xa4\x96")


def nfc_rows():
    """The constructs above with one NFC-changing element in front of or behind them, so the same
    sweep runs over the row as epoch text; a few invalid rows between, and one row past the buffer."""
    cons = [KA + VIRAMA + SSA, KA + extends(70) + VIRAMA + U + SSA, KA + AA + I, "\r\n" + U, "zzzz" + KA + AA * 3,
            "ab" + neutrals(64) + KA + SSA + B_KA, KA + VIRAMA * 4 + SSA, neutrals(66), B_KA + B_VIRAMA + B_SSA + B_O]
    rows = []
    for j, k in enumerate(POS):
        for i, c in enumerate(cons):
            case = NFC_CASES[(i + j) % len(NFC_CASES)]
            body = at(k, c)
            rows.append(((case + " " + body[len(case) + 1:]) if (i + j) & 1 else (body + " " + case)).encode("utf-8"))
        rows.append(INVALID[j % len(INVALID)])
    rows.append((NFC_CASES[0] + " " + "ab " * 260).encode("utf-8"))  # NFC-changing and over the buffer: the one-lane kernel
    return rows


# ---------------------------------------------------------------- the SentencePiece tile kernel
# ak_tile_spm.h: SP_SHORT = 12 (the longest word of the pool's 64-lane batches), SP_MAXL = 24 =
# ak_dev.h SPM_POOL_MAXL (the longest pooled word), both counting the word's "▁"; S_BCAP = 480 staged
# bytes per tile (the tile variant), SP_BCAP = 1024 (the pooled variant); AK_SP_FLUSH_MIN = 64 words
# start a batch; SP_RING = 320 slots per length class and wave.
SP_SHORT, SP_MAXL, S_BCAP, SP_BCAP, SP_FLUSH_MIN = 12, 24, 480, 1024, 64


def word_len_rows():
    """Words of 2, SP_SHORT - 1 .. SP_SHORT + 1 and SP_MAXL - 1 .. SP_MAXL + 1 chars ("▁" counted) in
    Latin, in Devanagari, in Bengali (no piece holds these chars: byte fallback) and mixed, alone and
    between other words."""
    rows = []
    for n in (2, SP_SHORT - 1, SP_SHORT, SP_SHORT + 1, SP_MAXL - 1, SP_MAXL, SP_MAXL + 1):
        c = n - 1
        for w in (fill(c, n), ("कमलनय" * 6)[:c], ("নাকষ" * 7)[:c], ("क१ল२" * 7)[:c]):
            rows += [w, "ab " + w + " cd", w + " " + w]
    return rows


def has_long_word(norm):
    """The normalized row holds a word over SP_MAXL chars, "▁" included (the pooled variant sends
    such a row to k_spm_redo, the tile variant solves it in the tile)."""
    return any(len(w) + 1 > SP_MAXL for w in norm.split(" "))


def row_len_rows():
    """Rows of S_BCAP - 1, S_BCAP and S_BCAP + 1 bytes: one long word, and many two-char words. A tile
    whose rows total 480 bytes of one-letter words holds (480 + 16) / 2 = 248 words at most, under
    S_WORDS = 256, so that limit of the tile variant is not reachable."""
    rows = []
    for n in (S_BCAP - 1, S_BCAP, S_BCAP + 1):
        rows += [fill(n, n), ("ab " * 200)[:n - 1] + "c", ("a " * 300)[:n - 1] + "b"]
    return rows


def w_step_rows():
    """Words that straddle a 64-element step of W (chars, "▁" per word, the row sentinels): "▁" as
    the last element of a step, and a word's last char there; the whitespace shapes at the same
    places."""
    rows = []
    for k in (60, 61, 62, 63, 64, 125, 126, 127):
        rows += [fill(k, k) + " xyz ab", fill(k, k) + "  a  b  ", fill(k, k) + "\t a", fill(k, k) + " a\nb  c",
                 "a " * (k // 2) + "namaste", fill(k, k) + " ", fill(k, k) + "   " + "q" * 30]
    rows += ["", " ", "   ", "a", " a", "a ", "  a  b  ", " " * 70 + "x", ";:" * 10 + " ok"]
    return rows


def spm_rows():
    """The SentencePiece rows as UTF-8 bytes; every row at the byte limit stands between two rows of
    600 bytes, so in the pooled variant too (1,024 staged bytes) it is alone in its tile and no tile
    passes S_WORDS; the invalid rows come last."""
    rows = interleave([word_len_rows(), w_step_rows()])
    for r in row_len_rows():
        rows += ["hello " * 100, r]
    rows.append("world " * 100)
    return [r.encode("utf-8") for r in rows] + list(INVALID)


def golden(name):
    """The reference's records for one row list (tools/gen_golden_rows_edges.py) by row index, and
    the fixture's meta record."""
    import gzip
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rows_edges.jsonl.gz")
    with gzip.open(path, "rt", encoding="utf-8") as f:
        recs = [json.loads(line) for line in f]
    return {r["i"]: r for r in recs[1:] if r["set"] == name}, recs[0]


def spm_ring_texts(units=300):
    """In every 64-row unit one tile adds 63 words of one length class (by itself below
    AK_SP_FLUSH_MIN: with what the rows before left waiting, up to 63 stay behind), and the next tile
    adds the most words of that class a pooled tile holds: 1,019 bytes of three-char words (one
    class: length 4 with "▁") are 255 words, under S_WORDS = 256, so up to 63 + 255 = 318 <= SP_RING
    = 320 entries wait before the drain. The rest of each unit is short synthetic rows; `units`
    units, so every wave's ring wraps."""
    from akshar_amd import synth
    filler = synth.lines(1, units * 62, seed=97)
    texts = []
    for u in range(units):
        texts.append(" ".join(fill(3, u + i) for i in range(63)))      # 251 bytes
        texts.append(" ".join(fill(3, u + i) for i in range(255)))     # 1,019 bytes: its own tile
        texts.extend(filler[62 * u:62 * (u + 1)])
    return texts
