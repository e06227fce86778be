"""Host check of csrc/gram_plan.h (no GPU): what a launch of the panel Gram runs.  The task tables of both
dealings hold every wanted task exactly once, with and without a mask of skipped tile pairs; the split and
dealing the cost model picks are those the code picked before it moved into the header (recorded from it);
the rectangular table of launch_atb and the row-chunk size likewise.  tests/gram_plan_check.cpp is compiled
with g++ under the address and undefined-behaviour sanitizers and run as a program of its own."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TASK = 2**64 - 1
XCD = 8


def mask_for(nb, seed):
    """about a quarter of the off-diagonal tile pairs skipped, never the diagonal: one character per slot"""
    state, out = (seed * 2654435761 + nb) % 2**32, []
    for i in range(nb):
        for j in range(i, nb):
            state = (state * 1664525 + 1013904223) % 2**32
            out.append("1" if i != j and (state >> 16) % 4 == 0 else "0")
    return "".join(out)


def slot(nb, i, j):
    return i * nb - i * (i - 1) // 2 + (j - i)


def task(i, j, y, kind=0):
    return i | j << 24 | y << 48 | kind << 62


def wanted_tasks(nb, nsplit, diag4, mask):
    """every (split, i <= j) pair that is not skipped; under diag4 the three tasks of every complete group of
    four diagonal tiles in place of its four diagonal pairs"""
    one = []
    for i in range(nb):
        for j in range(i, nb):
            g = i // 4 * 4
            if i == j and diag4 and g + 3 < nb:
                if i - g < 3:
                    one.append((i, i + 1, 1 + i - g))
            elif mask is None or mask[slot(nb, i, j)] == "0":
                one.append((i, j, 0))
    return sorted(task(i, j, y, k) for y in range(nsplit) for i, j, k in one)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("gram_plan") / "gram_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gram_plan_check.cpp"), "-o", exe],
                   check=True)

    def run(queries):
        queries = list(queries)
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        rows = [np.array(line.split(), dtype=np.uint64) for line in r.stdout.splitlines()]
        assert len(rows) == len(queries)
        return rows

    return run


def check_padding_at_the_tails(tab):
    """a multiple of 8 long, and within each XCD's sequence (tab[m * 8 + k], m ascending) no task after a
    padding entry; returns the tasks"""
    assert len(tab) % XCD == 0
    seqs = tab.reshape(-1, XCD)
    pad = seqs == np.uint64(NO_TASK)
    assert not np.any(pad[:-1] & ~pad[1:]), "a task follows a padding entry in its XCD's sequence"
    return tab[tab != np.uint64(NO_TASK)]


def test_task_tables_hold_every_wanted_task_once(ask):
    """nb = 1..40, five splits, diag4 on and off, both dealings, without and with a mask: 1600 tables"""
    cases = [(nb, ns, d4, ct, m) for nb in range(1, 41) for ns in (1, 2, 3, 7, 32) for d4 in (0, 1) for ct in (0, 1)
             for m in (None, mask_for(nb, 1))]
    tabs = ask("T %d %d %d %d %s" % (nb, ns, d4, ct, m or "-") for nb, ns, d4, ct, m in cases)
    plain = [c for c in cases if c[4] is None]
    blocks = ask("X %d %d %d %d" % c[:4] for c in plain)
    want_blocks = {c[:4]: int(b[0]) for c, b in zip(plain, blocks)}
    for (nb, ns, d4, ct, m), tab in zip(cases, tabs):
        tasks = check_padding_at_the_tails(tab)
        want = np.array(wanted_tasks(nb, ns, d4, m), dtype=np.uint64)
        assert np.array_equal(np.sort(tasks), want), (nb, ns, d4, ct, m)
        if m is None:  # the quantity the split pricing trusts
            assert len(tab) // XCD == want_blocks[(nb, ns, d4, ct)], (nb, ns, d4, ct)
    assert len(cases) == 1600
    print("%d tables, %d tasks" % (len(cases), sum(len(t) for t in tabs)))


def test_pair_slot(ask):
    cases = [(nb, i, j) for nb in (1, 2, 5, 40) for i in range(nb) for j in range(i, nb)]
    got = ask("S %d %d %d" % c for c in cases)
    assert [int(g[0]) for g in got] == [slot(*c) for c in cases]
    assert [slot(5, i, j) for i in range(5) for j in range(i, 5)] == list(range(15))  # row-major, no gaps


def test_rect_table_of_launch_atb(ask):
    """every (i, j) once with split 0, padding at the tails only; and the table as launch_atb built it before:
    8 x 8 squares, column squares outermost, each square whole to the XCD with the fewest blocks so far"""
    sizes = (1, 2, 7, 8, 9, 17)
    cases = list(itertools.product(sizes, sizes))
    for (mt, nt), tab in zip(cases, ask("R %d %d" % c for c in cases)):
        tasks = check_padding_at_the_tails(tab)
        assert sorted(tasks.tolist()) == sorted(task(i, j, 0) for i in range(mt) for j in range(nt)), (mt, nt)
        seq = [[] for _ in range(XCD)]
        for bj in range(0, nt, 8):
            for bi in range(0, mt, 8):
                k = min(range(XCD), key=lambda q: (len(seq[q]), q))
                seq[k] += [task(i, j, 0) for i in range(bi, min(mt, bi + 8)) for j in range(bj, min(nt, bj + 8))]
        want = np.full((max(len(s) for s in seq), XCD), NO_TASK, dtype=np.uint64)
        for k, s in enumerate(seq):
            want[:len(s), k] = s
        assert np.array_equal(tab, want.ravel()), (mt, nt)


# (nsplit, dealing: w = whole units, c = continuous) as the planning code of gram_of_staged chose them before it
# became gram_choose_split; per (slots, diag4) one row per nb, one entry per ntiles
NB = (1, 2, 4, 5, 8, 9, 16, 32, 33, 128)
NTILES = (1, 8, 24, 26, 64, 489, 1954, 15625)
PLANS = {
    (208, 0): (
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 20c 40w 62c",
        " 1c  1c  3c  3c  6c 13c 40w 40w",
        " 1c  1c  2c  2c  5c 17c 40w 40w",
        " 1c  1c  2c  2c  4c  9c 32w 60w",
        " 1c  1c  3c  3c  3c 12w 16w 32w",
        " 1w  1w  2w  2w  3w  7w 11w 24w",
        " 1w  1w  1w  1w  4w  4w 17w 20w",
        " 1w  1w  1w  1w  1w  2w  2w  2w",
    ),
    (208, 1): (
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 23c 23c 23c",
        " 1c  1c  3c  3c  7c 14c 44c 59c",
        " 1c  1c  3c  3c  6c  6c 24w 64w",
        " 1c  1c  2c  2c  7c 19w 24w 58w",
        " 1c  1c  3c  3c  3c 14w 14w 44w",
        " 1c  1c  1c  1c  2c  4w  4w  4w",
        " 1w  1w  2w  2w  2w  6w  6w  6w",
        " 1w  1w  1w  1w  1w  3w  3w  3w",
    ),
    (512, 0): (
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 51c 51c 51c",
        " 1w  1w  3w  3w  8w 34c 34c 34c",
        " 1c  1c  3c  3c  7c 14c 14c 56w",
        " 1c  1c  3c  3c  5c 11c 34w 34w",
        " 1c  1c  3c  3c  7c 15c 26w 64w",
        " 1w  1w  3w  3w  4w 12w 16w 32w",
        " 1w  1w  3w  3w  4w  5w 10w 31w",
        " 1w  1w  1w  1w  1w  3w  3w  3w",
    ),
    (512, 1): (
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 56w 56w 56w",
        " 1w  1w  3w  3w  8w 36c 36c 36c",
        " 1c  1c  3c  3c  7c 15c 15c 15c",
        " 1c  1c  3c  3c  5c 23w 35w 59w",
        " 1c  1c  3c  3c  7c 15c 42w 58w",
        " 1w  1w  3w  3w  4w 12w 23w 32w",
        " 1w  1w  3w  3w  4w  6w 12w 12w",
        " 1w  1w  1w  1w  1w  3w  3w  3w",
    ),
    (608, 0): (
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 60c 60c 60c",
        " 1w  1w  3w  3w  8w 40w 40w 40w",
        " 1w  1w  3w  3w  8w 16w 16w 50c",
        " 1w  1w  3w  3w  6w 13w 27w 27w",
        " 1c  1c  2c  2c  4w 22w 22w 58w",
        " 1w  1w  1w  1w  4w  8w  8w 23w",
        " 1w  1w  1w  1w  1w 13w 13w 13w",
        " 1w  1w  1w  1w  1w  3w  3w  3w",
    ),
    (608, 1): (
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 61w 64w 64w",
        " 1w  1w  3w  3w  8w 43c 43c 43c",
        " 1w  1w  3w  3w  8w 17c 35c 53c",
        " 1w  1w  3w  3w  7c 14w 14w 14w",
        " 1c  1c  2c  2c  4w  9c 18w 32w",
        " 1w  1w  1w  1w  4w  7w  7w  7w",
        " 1w  1w  1w  1w  1w  6w 12w 23w",
        " 1w  1w  1w  1w  1w  3w  3w  3w",
    ),
}
# the dealing for mask_for(nb, 1) at the split of PLANS, slots = 512: (nb, ntiles, diag4) -> continuous
DEALINGS = {
    (4, 64, 0): 0, (4, 64, 1): 0, (4, 1954, 0): 0, (4, 1954, 1): 0,
    (8, 64, 0): 0, (8, 64, 1): 0, (8, 1954, 0): 0, (8, 1954, 1): 0,
    (9, 64, 0): 1, (9, 64, 1): 1, (9, 1954, 0): 1, (9, 1954, 1): 1,
    (16, 64, 0): 1, (16, 64, 1): 1, (16, 1954, 0): 0, (16, 1954, 1): 0,
    (32, 64, 0): 0, (32, 64, 1): 0, (32, 1954, 0): 0, (32, 1954, 1): 0,
    (33, 64, 0): 0, (33, 64, 1): 0, (33, 1954, 0): 0, (33, 1954, 1): 0,
}


def recorded_plan(slots, diag4, nb, ntiles):
    e = PLANS[(slots, diag4)][NB.index(nb)].split()[NTILES.index(ntiles)]
    return int(e[:-1]), {"w": 0, "c": 1}[e[-1]]


def test_plans_as_before(ask):
    cases = [(nb, nt, sl, d4) for (sl, d4) in PLANS for nb in NB for nt in NTILES]
    got = ask("P %d %d %d %d" % c for c in cases)
    bad = []
    for (nb, nt, sl, d4), g in zip(cases, got):
        nsplit, cont, max_split = (int(v) for v in g)
        assert max_split == max(1, min(64, nt // 8, (4 << 30) // (nb * (nb + 1) // 2 * 128 * 128 * 8)))
        assert 1 <= nsplit <= max_split
        if (nsplit, cont) != recorded_plan(sl, d4, nb, nt):
            bad.append(((nb, nt, sl, d4), (nsplit, cont)))
    print("%d plans compared" % len(cases))
    assert not bad, bad[:5]
    # p, rows -> plan at slots = 512, as the issue that asked for the header lists them
    for (p, rows, d4), plan in {(4096, 125000, 1): (23, 0), (4096, 125000, 0): (16, 0), (1024, 125000, 1): (15, 1),
                                (1024, 125000, 0): (14, 1), (1024, 4096, 1): (7, 1), (640, 1601, 0): (3, 0),
                                (1100, 1601, 1): (3, 1), (16384, 125000, 0): (3, 0), (2048, 31250, 1): (15, 1),
                                (256, 512, 0): (1, 0)}.items():
        assert recorded_plan(512, d4, (p + 127) // 128, (rows + 63) // 64) == plan


def test_masked_dealings_as_before(ask):
    cases = sorted(DEALINGS)
    got = ask("D %d %d 512 %d %d %s" % (nb, nt, d4, recorded_plan(512, d4, nb, nt)[0], mask_for(nb, 1))
              for nb, nt, d4 in cases)
    assert {c: int(g[0]) for c, g in zip(cases, got)} == DEALINGS


def chunk_tiles_before(free_b, tile_bytes, ntiles, forced_rows):
    """launch_gram_panel's and grad_batch_normal_eq's arithmetic as both wrote it out; None: the refusal"""
    ctiles = min(free_b // 4, 16 << 30) // tile_bytes
    if forced_rows:
        ctiles = forced_rows // 64
    ctiles = min(max(ctiles, 1), ntiles)
    return None if ctiles * tile_bytes > free_b else ctiles


def test_chunk_tiles_as_before(ask):
    gib = 1 << 30
    free = (0, 1 << 20, 3 * gib, 40 * gib, 64 * gib, 64 * gib + 4096, 256 * gib)   # (64 GiB / 4: the 16 GiB cap)
    tile = (256 * 64 * 8, 4096 * 64 * 8, 4096 * 64 * 8 * 20, 3 * gib, 5 * gib)     # (p_pad x 64 rows x L doubles)
    ntiles = (1, 2, 63, 1954, 15625)
    forced = (0, 1, 63, 64, 512, 1024, 10**7)
    cases = list(itertools.product(free, tile, ntiles, forced))
    got = ask("C %d %d %d %d" % c for c in cases)
    want = [chunk_tiles_before(*c) for c in cases]
    assert [int(g[0]) for g in got] == [w or 0 for w in want]
    hit = {"cap": any(f // 4 > 16 * gib and not r and w == (16 * gib) // t < n for (f, t, n, r), w in zip(cases, want)),
           "floor": any(min(f // 4, 16 * gib) < t <= f and not r and w == 1 for (f, t, n, r), w in zip(cases, want)),
           "refusal": any(w is None for w in want),
           "forced": any(r and w == r // 64 > 1 for (f, t, n, r), w in zip(cases, want))}
    print("%d chunk sizes compared" % len(cases), hit)
    assert all(hit.values()), hit
