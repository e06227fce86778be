"""Host check of the Gram's own column order (csrc/gram_order.h; no GPU): the permutation, the sequential
farthest-first pass at wave-tile granularity, its sources, the packing of its mask and the engagement rule.

The headline term set (d = 20, p = 4096, 40 knots: the oracle's selectterms(4096)) is written as a level table for
tests/gram_order_check.cpp, which is compiled with g++ under the address and undefined-behaviour sanitizers and
run as a program of its own.  The checker asserts what it can see alone (stable factor-count sort and inverse, at
least 304 wave tiles dropped, every dropped entry's source in a kept wave tile with the same level pairs, at most
451 blocks per split, the rule says yes at 15 625 row tiles and no at 64).

This file restates the count in NumPy independently -- classes from the unordered level pairs (a random 64-bit
number per (dimension, lower level, higher level), summed over the dimensions), then the pass: the wave tiles
outside the diagonal tile pairs from the largest b - a down, the smallest a first, a tile dropped when every
entry still has another occurrence in a tile not yet dropped -- and must agree with the checker's mask tile for
tile.  The parallel rule on the terms' own order must be the committed mask of the wave-tile plan
(tests/golden/gram_quads_headline_mask.txt, 217 dropped)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def slot(n, i, j):
    return i * n - i * (i - 1) // 2 + (j - i)


def stable_factor_sort(terms):
    return np.argsort(np.count_nonzero(terms, axis=1), kind="stable")


def entry_classes(terms, seed=20):
    """upper-triangle entries (s, t) of G and the class of each: equal unordered level pairs in every dimension"""
    p, d = terms.shape
    s, t = np.triu_indices(p)
    L = int(terms.max()) + 1
    R = np.random.default_rng(seed).integers(0, 2**63, size=(d, L, L), dtype=np.int64).astype(np.uint64)
    key = np.zeros(len(s), dtype=np.uint64)
    for k in range(d):
        a, b = terms[s, k], terms[t, k]
        key += R[k, np.minimum(a, b), np.maximum(a, b)]
    _, cls = np.unique(key, return_inverse=True)
    return s, t, cls.ravel()


def sequential_pass(terms):
    """{(a, b)}: the wave tiles the sequential farthest-first pass drops for the columns in the order of `terms`;
    also (upper entries, distinct entries).  sequential_pass.put_back: the tiles of the latest call that were taken
    off the counts and put back although every class they hold occurs at least twice in G -- those the device's walk
    visits and rejects (a tile with a once-only class it never visits)"""
    p = len(terms)
    s, t, cls = entry_classes(terms)
    ncls = int(cls.max()) + 1
    a, b = s // 64, t // 64
    ng = 2 * ((p + 127) // 128)
    # a class with an entry on the diagonal of G (a duplicate term) is left alone: not counted, its tiles stay
    diag_cls = np.zeros(ncls, dtype=bool)
    diag_cls[cls[s == t]] = True
    counted = ~diag_cls[cls]
    cnt = np.bincount(cls[counted], minlength=ncls)
    total = cnt.copy()
    sequential_pass.put_back = []
    rank = slot(ng, a, b)           # any numbering of the tiles will do here
    order = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[order], np.arange(ng * (ng + 1) // 2 + 1))
    dropped = set()
    for dist in range(ng - 1, 0, -1):
        for i in range(ng - dist):
            j = i + dist
            if i // 2 == j // 2 or (j + 1) * 64 > p:
                continue
            r = slot(ng, i, j)
            e = order[bounds[r]:bounds[r + 1]]
            if not np.all(counted[e]):
                continue
            c = cls[e]
            np.subtract.at(cnt, c, 1)
            if np.all(cnt[c] >= 1):
                dropped.add((i, j))
            else:
                np.add.at(cnt, c, 1)
                if np.all(total[c] >= 2):
                    sequential_pass.put_back.append((i, j))
    return dropped, len(s), ncls


def parallel_rule(terms):
    """the rule of the device analysis in the terms' own order (tests/test_gpu_gram_quads.py: wave_tile_drops)"""
    p = len(terms)
    s, t, cls = entry_classes(terms)
    a, b = s // 64, t // 64
    ng = 2 * ((p + 127) // 128)
    prio = (b - a) * ng + a
    best = np.full(cls.max() + 1, prio.max() + 1)
    np.minimum.at(best, cls, prio)
    canonical = prio == best[cls]
    kept = set(zip(a[canonical].tolist(), b[canonical].tolist()))
    return {(i, j) for i in range(ng) for j in range(i, ng)
            if i // 2 != j // 2 and (j + 1) * 64 <= p and (i, j) not in kept}


def mask_tiles(mask, ng):
    tiles = [(i, j) for i in range(ng) for j in range(i, ng)]
    assert len(mask) == len(tiles)
    return {tl for tl, m in zip(tiles, mask) if m == "1"}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("gram_order")
    exe = str(tmp / "gram_order_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gram_order_check.cpp"), "-o", exe],
                   check=True)

    def run(terms, *bounds):
        path = str(tmp / ("levels_%d_%d.txt" % terms.shape))
        with open(path, "w") as f:
            f.write("%d %d\n" % terms.shape)
            np.savetxt(f, terms, fmt="%d")
        r = subprocess.run([exe, path] + [str(v) for v in bounds], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        return dict(line.split(None, 1) for line in r.stdout.splitlines())

    return run


@pytest.fixture(scope="module")
def headline_terms():
    import ob_oracle as O
    om = O.OuterMod()
    om.setcovfs(["mat25"] * 20)
    om.setknot(O.bench_knots(["mat25"] * 20, 40))
    terms = np.asarray(om.selectterms(4096), dtype=np.int64)
    terms.setflags(write=False)
    return terms


def test_headline_term_set(checker, headline_terms):
    terms = headline_terms
    assert np.bincount(np.count_nonzero(terms, axis=1)).tolist() == [1, 100, 1003, 1897, 1095]
    out = checker(terms, 304, 451)
    print({k: v for k, v in out.items() if "mask" not in k})
    assert out["identity"] == "0"
    assert int(out["dropped"]) >= 304 and int(out["blocks"]) <= 451
    assert (out["engage_headline"], out["engage_64"]) == ("1", "0")
    ng = 64
    # the NumPy restatement, tile for tile
    perm = stable_factor_sort(terms)
    drops, upper, distinct = sequential_pass(terms[perm])
    assert (upper, distinct) == (8390656, 2719650)
    assert mask_tiles(out["mask"], ng) == drops and len(drops) == int(out["dropped"])
    # the competing plan is the committed one
    with open(os.path.join(ROOT, "tests", "golden", "gram_quads_headline_mask.txt")) as f:
        golden = f.read().strip()
    assert out["as_given_mask"] == golden and int(out["as_given_parallel"]) == 217
    assert mask_tiles(golden, ng) == parallel_rule(terms)


def small_sets():
    """The two constructed d = 6 sets of tests/test_gpu_gram_quads.py shuffled by a fixed seed (0 - 5 factors
    interleaved), and p300: 64 base terms of exactly three factors on dimensions 0 - 3, once per (v, w) in (0,0),
    (1,0), (0,1), (1,1) on dimensions 4 and 5, and 44 terms of six factors, shuffled likewise.  Sorted by factor
    count p300 is [the (0,0) group | the (1,0) and (0,1) groups interleaved | the (1,1) group | 44 terms and 84
    padding columns]: wave tile (0, 3), (0,0) x (1,1), repeats (1,0) x (0,1) entries and is the one that drops;
    the parallel rule on the shuffled order drops none.  p256: the same 64 base terms once per (v, w) in the
    caller's order (1,1), (1,0), (0,0), (0,1), shuffled inside each group only; the stable sort makes it
    [(0,0) | (1,0) | (0,1) | (1,1)], one column group each.  Wave tiles (0, 3) and (1, 2) hold the same classes --
    the level pairs {0,1}, {0,1} on dimensions 4 and 5 -- four times where the base terms differ and twice where
    they are equal: the walk drops (0, 3), then takes (1, 2) off the counts, finds the equal-base classes at zero
    and puts it back (the path a tile with a once-only class never reaches)."""
    import itertools
    base = list(itertools.product(range(4), range(4), range(4)))
    groups = {
        "p384": ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 0, 2)),
        "p512": tuple((u, v, w) for w in (0, 1) for v in (0, 1) for u in (0, 1)),
    }
    out = {}
    for name, g in groups.items():
        terms = np.array([list(s) + list(q) for q in g for s in base], dtype=np.int64)
        out[name] = terms[np.random.default_rng(5).permutation(len(terms))]
    base3 = [b for b in itertools.product(range(4), repeat=4) if np.count_nonzero(b) == 3][:64]
    base4 = list(itertools.product(range(1, 4), repeat=4))[:44]
    p300 = np.array([list(b) + list(g) for g in ((0, 0), (1, 0), (0, 1), (1, 1)) for b in base3]
                    + [list(b) + [1, 1] for b in base4], dtype=np.int64)
    out["p300"] = p300[np.random.default_rng(5).permutation(len(p300))]
    rng = np.random.default_rng(6)
    out["p256"] = np.array([list(base3[k]) + list(g) for g in ((1, 1), (1, 0), (0, 0), (0, 1))
                            for k in rng.permutation(64)], dtype=np.int64)
    return out


@pytest.mark.parametrize("which", ["p384", "p512", "p300", "p256"])
def test_small_sets_agree_tile_for_tile(checker, which):
    terms = small_sets()[which]
    out = checker(terms)
    perm = stable_factor_sort(terms)
    assert not np.array_equal(perm, np.arange(len(terms)))
    drops, _, _ = sequential_pass(terms[perm])
    ng = 2 * ((len(terms) + 127) // 128)
    print(which, sorted(drops), out["blocks"])
    assert mask_tiles(out["mask"], ng) == drops
    assert mask_tiles(out["as_given_mask"], ng) == parallel_rule(terms)
    assert len(drops) >= 1
    if which == "p300":
        assert drops == {(0, 3)} and not parallel_rule(terms)
    if which == "p256":
        assert drops == {(0, 3)} and sequential_pass.put_back == [(1, 2)]
