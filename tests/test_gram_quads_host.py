"""Host check of the wave-tile plan of csrc/gram_plan.h (no GPU): gram_quads_pack and gram_quads_table.

A block of the panel Gram stages the panels of tile pair (I, J) and each of its four waves computes one 64 x 64
wave tile of those 256 columns.  Given a keep mask over the wave tiles of the upper triangle, the packed plan
must compute every kept wave tile exactly once per row split, no dropped one, name operand groups that ARE
the rows and columns of the wave tile it writes, and deal the blocks to the XCDs padded at the tails as
build_task_order does.  tests/gram_quads_check.cpp is compiled with g++ under the address and
undefined-behaviour sanitizers and run as a program of its own.

tests/golden/gram_quads_headline_mask.txt is the mask of the headline term set (d = 20, p = 4096, 40 knots:
selectterms(4096)), one character per wave tile in row-major order of the upper triangle of 64 column groups,
'1' = dropped: 217 of 2080, counted in NumPy with the rule of the device analysis (the canonical occurrence of
an entry is the one in the wave tile with the smallest b - a, then the smallest a; a wave tile that holds no
canonical occurrence and lies in no diagonal tile is dropped)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TASK = 2**64 - 1
XCD = 8
IDLE = 3


def slot(n, i, j):
    return i * n - i * (i - 1) // 2 + (j - i)


def wave_tiles(nb):
    return [(a, b) for a in range(2 * nb) for b in range(a, 2 * nb)]


def mask_of(nb, dropped):
    m = ["0"] * len(wave_tiles(nb))
    for a, b in dropped:
        m[slot(2 * nb, a, b)] = "1"
    return "".join(m)


def random_mask(nb, seed):
    """about a third of the wave tiles outside the diagonal tiles dropped"""
    state, out = (seed * 2654435761 + nb) % 2**32, []
    for a, b in wave_tiles(nb):
        state = (state * 1664525 + 1013904223) % 2**32
        out.append("1" if a // 2 != b // 2 and (state >> 16) % 3 == 0 else "0")
    return "".join(out)


def headline_mask():
    with open(os.path.join(ROOT, "tests", "golden", "gram_quads_headline_mask.txt")) as f:
        return f.read().strip()


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("gram_quads") / "gram_quads_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gram_quads_check.cpp"), "-o", exe],
                   check=True)

    def run(queries):
        queries = list(queries)
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        rows = [np.array(line.split(), dtype=np.uint64) for line in r.stdout.splitlines()]
        assert len(rows) == len(queries)
        return rows

    return run


def written(I, J, byte):
    """the wave tile (a, b) a wave with this byte writes in a block that stages (I, J), None when it idles;
    its operand groups must be inside the two panels and be that wave tile's rows and columns"""
    A, B, wm, wn, sel = byte & 3, byte >> 2 & 3, byte >> 4 & 1, byte >> 5 & 1, byte >> 6
    assert 0 <= byte < 256
    if sel == IDLE:
        return None
    oi, oj = (J if sel == 1 else I), (I if sel == 0 else J)
    group = lambda g: 2 * I + g if g < 2 else 2 * J + g - 2   # the staged row is [panel I | panel J]
    a, b = 2 * oi + wm, 2 * oj + wn
    assert (group(A), group(B)) == (a, b), "the operands are not the wave tile's rows and columns"
    assert a <= b
    return a, b


def check_blocks(nb, mask, blocks):
    """blocks: (I, J, four bytes) of one split -> every kept wave tile once, no dropped one; returns their number"""
    kept = {t for t, m in zip(wave_tiles(nb), mask) if m == "0"}
    seen = []
    for I, J, *w in blocks:
        assert 0 <= I <= J < nb
        tiles = [written(I, J, b) for b in w]
        assert any(t is not None for t in tiles), "a block without work"
        tiles = [t for t in tiles if t is not None]
        seen += tiles
        for t in tiles:
            # off-diagonal wave tiles stay in the block of their own tile pair
            assert t[0] // 2 == t[1] // 2 or (t[0] // 2, t[1] // 2) == (I, J)
    assert len(seen) == len(set(seen)), "a wave tile is computed twice"
    assert set(seen) == kept
    return len(blocks)


MASKS = {
    "none dropped": lambda nb: mask_of(nb, []),
    "one wave tile": lambda nb: mask_of(nb, [(0, 2 * nb - 1)]),
    "a whole tile pair": lambda nb: mask_of(nb, [(r, 2 * (nb - 1) + c) for r in (0, 1) for c in (0, 1)]),
    "one tile's off-diagonal": lambda nb: mask_of(nb, [(a, b) for a, b in wave_tiles(nb)
                                                       if a // 2 != b // 2 and 1 in (a // 2, b // 2)]),
    "random": lambda nb: random_mask(nb, 3),
}


@pytest.mark.parametrize("which", sorted(MASKS))
def test_every_kept_wave_tile_once(ask, which):
    sizes = [nb for nb in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33) if nb >= 2 or which == "none dropped"]
    masks = [MASKS[which](nb) for nb in sizes]
    packs = ask("K %d %s" % (nb, m) for nb, m in zip(sizes, masks))
    cases = [(nb, m, ns, ct) for nb, m in zip(sizes, masks) for ns in (1, 3, 32) for ct in (0, 1)]
    tables = ask("Q %d %d %d %s" % (nb, ns, ct, m) for nb, m, ns, ct in cases)
    count = {}
    for nb, m, pk in zip(sizes, masks, packs):
        count[nb] = check_blocks(nb, m, pk.reshape(-1, 6).astype(np.int64).tolist())
        kept = m.count("0")
        assert count[nb] >= -(-kept // 4)
        if which == "none dropped":   # what four diagonal tiles as three blocks reach, or better
            assert count[nb] <= nb * (nb - 1) // 2 + -(-3 * nb // 4) + (1 if nb > 1 else 0)
    for (nb, m, ns, ct), row in zip(cases, tables):
        tab, wb = row[:len(row) // 2], row[len(row) // 2:].astype(np.int64)
        assert len(tab) % XCD == 0 and len(tab) == len(wb)
        pad = tab.reshape(-1, XCD) == np.uint64(NO_TASK)
        assert not np.any(pad[:-1] & ~pad[1:]), "a task follows a padding entry in its XCD's sequence"
        live = tab != np.uint64(NO_TASK)
        t = tab[live].astype(np.int64)
        I, J, y, kind = t & 0xffffff, t >> 24 & 0xffffff, t >> 48 & 0x3fff, t >> 62
        assert np.all(kind == 0)
        for s in range(ns):
            sel = y == s
            blocks = [(int(i), int(j)) + tuple(int(w >> 8 * k & 255) for k in range(4))
                      for i, j, w in zip(I[sel], J[sel], wb[live][sel])]
            assert check_blocks(nb, m, blocks) == count[nb], (nb, ns, ct, s)
        assert set(y.tolist()) == set(range(ns))


def test_headline_mask(ask):
    """d = 20, p = 4096: 217 of 2080 wave tiles dropped -> at most 469 blocks per split (484 with whole tile pairs
    skipped, 520 without; the bound is ceil(1863 / 4) = 466), and the plan is priced below the whole-pair one at
    the benchmark's shape (15625 row tiles, 512 slots, 32 splits: 15006 for the whole-pair table)"""
    m = headline_mask()
    assert len(m) == 2080 and m.count("1") == 217
    pk, = ask(["K 32 " + m])
    n = check_blocks(32, m, pk.reshape(-1, 6).astype(np.int64).tolist())
    idle = sum(1 for row in pk.reshape(-1, 6) for b in row[2:] if int(b) >> 6 == IDLE)
    print("headline: %d blocks per split, %d idle waves" % (n, idle))
    assert n <= 469
    (cont, cost), = ask(["D 32 15625 512 32 " + m])
    print("dealing %d, gram_cost %.1f" % (cont, int(cost) / 1000.0))
    assert int(cost) / 1000.0 < 15006 - 200
