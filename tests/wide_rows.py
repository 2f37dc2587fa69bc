"""Rows that put every edge of the tile kernels' 128-element sweep steps (ak_tile.h AK_TILE_WIDE: two
adjacent elements per lane) and of their 64-element steps under row marks, elongation runs, in-tile
NFC cases, pre-token starts and rare code points. Shared by tests/test_emu_wide_steps.py (the host
emulator) and tests/test_gpu_wide_steps.py (the device); both compare with the oracle."""

EDGES = (63, 64, 65, 127, 128, 129, 255, 256, 257)   # entry counts around one, two and four 64-lane steps
FILL1 = "abcdefg"                                    # 1-byte chars, no char repeated within 7
FILLX = ["a", "क", "b", "é", "c", "खि"]  # 1-, 3-, 1-, 2-, 1-, 3+3-byte chars


def fill(k, shift=0):
    """k one-byte word chars, no two neighbours equal (no elongation run)."""
    return "".join(FILL1[(i + shift) % 7] for i in range(k))


def fillx(k):
    """k chars of 1, 2 and 3 bytes, so odd and even byte positions both hold leads."""
    out, i = [], 0
    while sum(len(x) for x in out) < k:
        out.append(FILLX[i % len(FILLX)])
        i += 1
    return "".join(out)[:k]


def count_rows():
    """Rows whose P (marks + leads), V and W entry counts are each of EDGES (a row of c chars lists
    c + 1 entries of P with its mark and c + 2 of V and W with its sentinels; c runs over a window
    below every edge), of one-byte chars and of mixed widths."""
    rows = []
    for n in EDGES:
        for c in range(n - 3, n + 1):
            rows.append(fill(c, shift=n))
            rows.append(fillx(c))
    return rows


def mark_rows():
    """Row marks at odd and even P indices: rows of 1 .. 4 bytes back to back, an empty row between
    two rows and at both ends of a tile, 64 one-byte rows in one unit, one row of exactly the tile
    buffer (768 bytes) and one of 769 (over it: the fallback kernels)."""
    rows = ["a", "bc", "d", "कख", "e", "fgh", "क", "ij", "", "kl", "", "", "ém", ""]
    rows += [FILL1[i % 7] for i in range(64)]
    rows += [("ab " * 256)[:768], ("cd " * 257)[:769], "xy"]
    rows += ["क" * 2 + fill(61), "z", fill(126), "खq", fill(127), "r"]  # marks right at a step's end
    return rows


def elongation_rows():
    """Runs of 3, 4, 5 and 6 equal chars and a run across newlines starting at V indices around the
    lane-pair, 64- and 128-element edges: inside one lane's pair, split over two lanes, split over
    two steps, and long enough that the previous kept element lies beyond dropped ones on both
    sides of a lane or step boundary."""
    rows = []
    for k in (0, 1, 2, 61, 62, 63, 64, 124, 125, 126, 127, 128, 129):
        for run in ("zzz", "zzzz", "zzzzz", "zzzzzz", "z\n\n\nz", "zz zz", "zzककककz"):
            rows.append(fill(k) + run + "q" + fill(3))
    return rows


NFC_CASES = ("क़",               # a precomposed nukta letter: two V entries
             "ऩ",         # a composing pair (-> U+0929)
             "क़́",   # two marks out of canonical order: swapped in the tile
             "क़़", "क़क़")


def nfc_rows():
    """The in-tile NFC cases and an invalid byte as the last elements of a step, the first of the
    next and mid-step (their successors one step on): the hand-over of the step carries."""
    rows = []
    for k in (30, 31, 60, 61, 62, 63, 64, 123, 124, 125, 126, 127, 128, 129):
        for case in NFC_CASES:
            rows.append((fill(k) + case + "ab " + case).encode())
        rows.append(fill(k).encode() + b"\x80" + b"ok")
        rows.append(fill(k).encode() + b"\xe0\xa4" + b" ok")
    return rows


def pretoken_rows():
    """Pre-tokens that start on the last element of a step and on the first of the next: one-symbol
    pre-tokens, two-symbol ones, and a tile's very last pre-token in each shape."""
    rows = []
    for j in (29, 30, 31, 60, 61, 62, 63, 64, 124, 125, 126, 127, 128):
        rows.append("a " * j + "xy")
        rows.append("a " * j + "z")
        rows.append(("ab " * j)[:2 * j + 1] + " namaste")
        rows.append(fill(j) + " k")
        rows.append(fill(j) + " क्ष")
    return rows


RARE = (" ",    # a compat space: HF NFKC maps it to ' '
        "　",    # ... a 3-byte one
        "中",    # outside the vocabulary
        "ਕ",    # outside the LDS hot tables (Gurmukhi)
        "’",    # punctuation outside the hot tables
        "\U0001F600")  # a 4-byte char


def rare_rows():
    """A compat space, a char outside the vocabulary and chars outside the LDS hot tables as the first
    and the second element of a lane's pair, mid-step and at the step edges."""
    rows = []
    for k in (10, 11, 62, 63, 64, 126, 127, 128):
        for ch in RARE:
            rows.append(fill(k) + ch + "ab" + ch + ch + "c")
    return rows


def all_rows():
    """Every row above as UTF-8 bytes, the groups interleaved with each other's rows (so tiles of
    several rows mix short and long rows and marks fall everywhere)."""
    groups = [count_rows(), mark_rows(), elongation_rows(), nfc_rows(), pretoken_rows(), rare_rows()]
    rows = [r if isinstance(r, bytes) else r.encode("utf-8") for g in groups for r in g]
    return rows
