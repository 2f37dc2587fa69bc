"""Rows that put every edge of a 128-entry step of the BPE tile kernel's pass N (ak_tile.h AK_TILE_WIDE
bits TW_N and TW_NS: lane l takes V entries 2l and 2l + 1; the pre-token starts are listed by N
itself) under elongation runs, pre-token starts, dropped and remapped chars, the rare code points and
row marks. V holds, per row, <s>, one entry per char that normalize_text keeps, </s>: char i of a
one-row tile is V entry i + 1, and a tile of rows with c_0, c_1, ... chars has its </s><s> pairs at
entries c_0 + 1, c_0 + c_1 + 3, ... Shared by tests/test_emu_wide_n.py (the host emulator) and
tests/test_gpu_wide_n.py (the device); both compare with the oracle."""
from tests.wide_rows import fill

STEP_LENS = (126, 127, 128, 129, 130, 254, 255, 256, 257, 258)  # V lengths around one and two steps
T_SCAP = 240          # ak_tile.h: pre-tokens of >= 2 symbols one tile may list
GROUP = 4             # tile_groups(): rows per group (= a tile when tiles take 4 rows)

NBSP, EMSP = " ", " "      # HF NFKC maps both to ' '
CJK = "中"                       # kept by normalize_text, outside the vocabulary: it vanishes
GURMUKHI, QUOTE = "ਕ", "’"  # outside the LDS hot table and outside the LDS single-id table
NUKTA = "़"
EMOJI = "\U0001F600"                 # removed by normalize_text's filter: no V entry


def v_len(rows):
    """V entries of a tile of rows of plain one-byte chars (fill() rows)."""
    return sum(len(r) + 2 for r in rows)


def mark_pairs(rows):
    """V index of the </s> of each </s><s> pair of such a tile."""
    out, at = [], 0
    for r in rows[:-1]:
        at += len(r) + 2
        out.append(at - 1)
    return out


def tile_groups():
    """Groups of GROUP rows, first in the row set, so that each is one tile when tiles take 4 rows:
    tiles whose V length is each of STEP_LENS, and tiles whose </s><s> pair sits in one lane's pair
    (</s> at an even entry), in two lanes' (odd), and in two steps' (entries 127 | 128, 255 | 256)."""
    groups = []
    for n in STEP_LENS:
        rest = n - 2 * GROUP - (10 + 11 + 12)
        groups.append([fill(10), fill(11, 1), fill(rest, 2), fill(12, 3)])
    for c in (4, 5, 124, 125, 126, 127, 254):   # </s> at c + 1
        groups.append([fill(c, 1), fill(3), "xy", "z"])
    groups.append([fill(60), fill(64, 2), fill(1), fill(125, 4)])  # pairs at 61|62, 127|128, 130|131
    assert all(len(g) == GROUP and sum(len(r) for r in g) <= 768 for g in groups)
    return groups


def length_rows():
    """One-row tiles whose V length is each of STEP_LENS (c chars list c + 2 entries)."""
    return [fill(n - 2, n) for n in STEP_LENS]


def elongation_rows():
    """Runs of 3 .. 7 equal chars starting at every V entry around a lane's pair and around entries
    127 | 128 and 255 | 256: members in one pair, over two pairs, over two steps; the kept char after
    a run has its previous kept char one and two fully dropped pairs back (runs of 3+ keep their
    first char only). Runs broken by '\\n' (exempt), a run right after the row start, runs of a
    3-byte char, and a run whose chars are dropped at a step's first entries."""
    rows = []
    for k in (0, 1, 2, 3, 122, 123, 124, 125, 126, 127, 128, 250, 252, 253, 254, 255):
        for n in (3, 4, 5, 6, 7):
            rows.append(fill(k) + "z" * n + "q" + fill(3))
    for k in (0, 1, 124, 125, 126):
        for run in ("zz\nzz", "z\n\n\nz", "\n\n\n\n", "zzz\nzzz", "क" * 4 + "z", "zzकककzzz", "zz zz  zzz"):
            rows.append(fill(k) + run + "q")
    return rows


def pretoken_rows():
    """Pre-token starts at even and odd entries; a start at a step's last entry with its second symbol
    in the next step; a single-symbol pre-token at a step's last entry, and as the tile's last entry;
    a pre-token of several symbols that ends with the row; pre-tokens of one and two symbols all
    along two steps at both parities."""
    rows = []
    for k in (123, 124, 125, 126, 127, 251, 252, 253, 254, 255):   # the char after the space is V entry k + 2
        rows += [fill(k) + " xy", fill(k) + " x", fill(k) + " x yz", fill(k) + " xyz wv", fill(k) + " x y"]
    for lead in ("", " ", "q", "q "):
        rows += [lead + "ab " * 70, lead + "a b " * 60, lead + "a bc " * 50 + "d", lead + "ab, cd. " * 30 + "ef"]
    return rows


def dropped_rows():
    """A char outside the vocabulary (it vanishes) between two kept chars of one word and of two
    words, and several in a row; HF compat spaces at both entries of a pair and at entries 127 | 128."""
    rows = []
    for k in (0, 1, 2, 124, 125, 126, 127):
        rows += [fill(k) + "a" + CJK + "b", fill(k) + "a " + CJK + " b", fill(k) + "a" + CJK + " b",
                 fill(k) + "a" + CJK * 2 + "b" + CJK * 3 + "c", fill(k) + " " + CJK + "ab",
                 fill(k) + NBSP + "ab" + EMSP + "c", fill(k) + "a" + NBSP + EMSP + "bc", fill(k) + EMSP + NBSP + "b"]
    return rows


RARE_AT = (0, 1, 2, 3, 125, 126, 127, 128)   # chars before the rare one: it is V entry k + 1


def rare_rows():
    """Code points outside the LDS hot table and the LDS single-id table at even and odd entries and
    on both sides of a step edge; rows whose NFC trips in pass D2 (a singleton, a decomposed pair, the
    in-tile cases)."""
    rows = []
    for k in RARE_AT:
        rows += [fill(k) + GURMUKHI + "ab" + QUOTE + "c", fill(k) + QUOTE + GURMUKHI + GURMUKHI + " d"]
    for k in (0, 1, 125, 126, 127):
        rows += [fill(k) + "Å" + "b", fill(k) + "é" + "b", fill(k) + "क़" + "b", fill(k) + "न" + NUKTA + "b"]
    return rows


def hf_trip_rows():
    """Rows that pass D2's NFC proof and trip pass N's HF-NFC quick check, the tripping char at each of
    RARE_AT: a nukta that meets its letter only after normalize_text removed the char between them
    (HF's NFKC composes the pair). Each goes to the fallback kernels (fb bit 1)."""
    return [fill(k) + "न" + EMOJI + NUKTA + " ab" for k in RARE_AT]


def scap_rows():
    """A tile of exactly T_SCAP pre-tokens of two symbols, one of T_SCAP + 1 and a full 768-byte one
    (256): the rows before and between are too long to share a tile with them, the rows after hold
    no pre-token of two symbols."""
    return [fill(700), "ab " * T_SCAP, "a", "b", "c", "ab " * (T_SCAP + 1), "a", "b", "c", ("ab " * 256)[:768], "d", "e", "f"]


def all_rows():
    """Every row above as UTF-8 bytes: the 4-row groups first, then the rest."""
    rows = [r for g in tile_groups() for r in g]
    rows += scap_rows()
    for g in (length_rows(), elongation_rows(), pretoken_rows(), dropped_rows(), rare_rows(), hf_trip_rows()):
        rows += g
    return [r.encode("utf-8") for r in rows]
