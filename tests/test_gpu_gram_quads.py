"""The panel Gram's plan at wave-tile granularity (gram_dedup.hip, gram_plan.h: gram_quads_pack), forced with
OBHIP_GRAM_DEDUP_QUADS=1: 64 x 64 wave tiles all of whose entries repeat in wave tiles nearer the diagonal are
dropped, the kept ones packed into blocks anew, the dropped ones filled from their sources.

Two constructed d = 6 term sets, terms (l0, l1, l2, u, v, w) with the 64 base terms (l0, l1, l2) in {0..3}^3
repeated once per (u, v, w), one 64-column group each:

  p384  (u, v, w) = (0,0,0), (1,0,0), (0,1,0), (1,1,0), (0,0,1), (0,0,2): three tiles, six groups.  73 920
        upper-triangle entries, 20 000 distinct.  No tile pair can be skipped; at 64 x 64 exactly wave tile
        (0, 3) -- rows 0-63, columns 192-255, groups (0,0,0) x (1,1,0) -- goes, a repeat of wave tile (1, 2),
        (1,0,0) x (0,1,0): the same unordered pairs {0,1}, {0,1}, {0,0}.  The free wave of tile pair (0, 1) takes one of
        the nine diagonal wave tiles and the other eight make two blocks: 5 blocks per split against the 6 of one
        block per tile pair.
  p512  (u, v, w) in {0,1}^3, u fastest: four tiles, eight groups.  131 328 entries, 27 000 distinct.  Nine wave tiles
        go: (0,3), (0,5), (0,6), (0,7), (1,6), (1,7), (2,5), (2,7), (4,7) -- all four of tile pair (0, 3), which
        the whole-pair analysis skips too, and one each of the other five off-diagonal pairs, whose free waves
        take five of the twelve diagonal wave tiles; the other seven take three neighbour blocks as the matching
        leaves them (1, 1, 3, 2 per tile): 8 blocks per split, as many as the whole-pair plan's 5 + 3.

Both counts are restated in NumPy below (wave_tile_drops, the rule of the device analysis) and asserted.

Checked: G finite and exactly symmetric; every entry within tests/extended_ref.py's ref_gram tolerance (none of
this file's own); every entry of a kept wave tile outside the diagonal tile pairs equal to the
OBHIP_GRAM_DEDUP=0 run bit for bit (those stay in their block; a diagonal wave tile may move to a block with
another chunk rotation); the table's sources hold the entry's own level pairs and lie in kept wave tiles; the
run is poisoned (no value may come from what an earlier launch left in the workspace)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import extended_ref as E
from conftest import knots_for, make_pair, sample_x
from test_gpu_gram_dedup import KINDS6, fill_table, gram, info

pytestmark = pytest.mark.gpu

GROUPS = {
    "p384": ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 0, 2)),
    "p512": tuple((u, v, w) for w in (0, 1) for v in (0, 1) for u in (0, 1)),
}
# (upper entries, distinct, dropped wave tiles, blocks per split packed, tile pairs the whole-pair plan skips)
EXPECT = {
    "p384": (73920, 20000, {(0, 3)}, 5, 0),
    "p512": (131328, 27000, {(0, 3), (0, 5), (0, 6), (0, 7), (1, 6), (1, 7), (2, 5), (2, 7), (4, 7)}, 8, 1),
}


def constructed_terms(which):
    base = list(itertools.product(range(4), range(4), range(4)))
    return np.array([list(s) + list(g) for g in GROUPS[which] for s in base], dtype=np.int64)


def wave_tile_drops(terms):
    """(upper entries, distinct entries, dropped wave tiles): an entry's canonical occurrence is the one in the
    wave tile with the smallest b - a, then the smallest a; a wave tile outside the diagonal tile pairs that
    holds no canonical occurrence is dropped"""
    p = len(terms)
    s, t = np.triu_indices(p)
    lo, hi = np.minimum(terms[s], terms[t]), np.maximum(terms[s], terms[t])
    _, cls = np.unique(np.concatenate([lo, hi], axis=1), axis=0, return_inverse=True)
    cls = cls.ravel()
    a, b = s // 64, t // 64
    ng = (p + 63) // 64
    prio = (b - a) * ng + a
    best = np.full(cls.max() + 1, prio.max() + 1)
    np.minimum.at(best, cls, prio)
    canonical = prio == best[cls]
    kept = set(zip(a[canonical].tolist(), b[canonical].tolist()))
    drops = {(i, j) for i in range(ng) for j in range(i, ng) if i // 2 != j // 2 and (i, j) not in kept}
    return len(s), int(cls.max()) + 1, drops


@functools.lru_cache(maxsize=None)
def model(which):
    import outerbase_amd as ob
    om_o, om_d = make_pair(KINDS6, knots_for(KINDS6, 20))
    rot, _, _ = om_d.rotation()
    knots = [np.asarray(k, dtype=np.float64) for k in knots_for(KINDS6, 20)]
    return dict(om_o=om_o, om_d=om_d, hyp=ob.gethyp(om_d), rot=rot, knots=knots, terms=constructed_terms(which))


@functools.lru_cache(maxsize=None)
def rows(which, n):
    """x and the long double reference of G on all columns, computed once and shared"""
    import ob_oracle as O
    m = model(which)
    x = sample_x(np.random.default_rng(177 + n), n, KINDS6)
    ref = E.ExtendedRef(KINDS6, m["knots"], m["hyp"], m["rot"], x)
    B, bB = ref.getmat(m["terms"])
    Bo = O.ob_getmat(O.OuterBase(m["om_o"], x), m["terms"])
    Cc = E.constant_from_oracle_ratio(E.worst_ratio(Bo, B, bB))
    want, tol = E.ref_gram(B, bB, np.arange(B.shape[1]), Cc)
    for arr in (want, tol):
        arr.setflags(write=False)
    return dict(x=x, want=want, tol=tol)


def quads_info(t):
    from outerbase_amd._lib import call
    tiles, dropped, blocks, engaged = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    call("obhip_gram_dedup_quads_info", t._h, C.byref(tiles), C.byref(dropped), C.byref(blocks), C.byref(engaged))
    return tiles.value, dropped.value, blocks.value, engaged.value


def check_table(terms, src):
    """every entry of a dropped wave tile against its source: the same unordered level pairs, a source that is
    computed; whole wave tiles, none in a diagonal tile pair; returns the dropped wave tiles"""
    p = len(terms)
    s, t = np.nonzero(src >= 0)
    assert np.all(s < t)
    q = src[s, t]
    ss, st = q // p, q % p
    assert np.all(ss <= st) and np.all(src[ss, st] < 0), "a source lies in a dropped wave tile"
    assert np.array_equal(np.minimum(terms[s], terms[t]), np.minimum(terms[ss], terms[st]))
    assert np.array_equal(np.maximum(terms[s], terms[t]), np.maximum(terms[ss], terms[st]))
    tiles = set(zip((s // 64).tolist(), (t // 64).tolist()))
    assert all(a // 2 != b // 2 for a, b in tiles) and len(s) == 64 * 64 * len(tiles)
    return tiles


@pytest.mark.parametrize("which,n,chunk_rows", [("p384", 200, None), ("p384", 1500, None), ("p384", 1500, 512),
                                                ("p384", 200, 512), ("p512", 200, None), ("p512", 1500, None),
                                                ("p512", 1500, 512)])
def test_constructed_sets(which, n, chunk_rows, monkeypatch):
    from outerbase_amd import obmod
    m, c = model(which), rows(which, n)
    terms, p = m["terms"], len(m["terms"])
    upper, distinct, drops, blocks, pairs_skipped = EXPECT[which]
    assert wave_tile_drops(terms) == (upper, distinct, drops)
    if chunk_rows:
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(chunk_rows))
    monkeypatch.setenv("OBHIP_GRAM_DEDUP_QUADS", "1")
    t = obmod._Terms(m["om_d"], terms)
    monkeypatch.setenv("OBHIP_GRAM_DEDUP", "0")
    assert quads_info(t)[1:] == (0, 0, 0)
    G0 = gram(m["om_d"], t, c["x"])
    monkeypatch.delenv("OBHIP_GRAM_DEDUP")
    ng = p // 64
    assert quads_info(t) == (ng * (ng + 1) // 2, len(drops), blocks, 1)
    assert info(t)[1] == pairs_skipped      # the whole-pair analysis is what it was
    src = fill_table(t)
    assert check_table(terms, src) == drops
    G1 = gram(m["om_d"], t, c["x"], poison=True)
    assert quads_info(t)[3] == 1
    dropped = (src >= 0) | (src >= 0).T
    tile = np.arange(p) // 128
    home = (tile[:, None] != tile[None, :]) & ~dropped    # kept wave tiles outside the diagonal tile pairs, and mirrors
    r0, r1 = E.worst_ratio(G0, c["want"], c["tol"]), E.worst_ratio(G1, c["want"], c["tol"])
    on_copied = E.worst_ratio(G1[dropped], c["want"][dropped], c["tol"][dropped])
    moved = int(np.count_nonzero(G1[~home & ~dropped] != G0[~home & ~dropped]))
    print("%s n = %d chunk %s: %d wave tiles dropped, %d blocks per split; err/tol switched off %.3g, on %.3g (copied "
          "entries %.3g); %d entries of the diagonal tile pairs differ in their last bits"
          % (which, n, chunk_rows, len(drops), blocks, r0, r1, on_copied, moved))
    assert np.all(np.isfinite(G1)) and np.array_equal(G1, G1.T)
    assert np.array_equal(G1[home], G0[home]), "an entry of a kept off-diagonal wave tile differs from the switched-off run"
    assert r1 <= 1.0


@pytest.mark.parametrize("which", ["p384", "p512"])
def test_unset_at_these_sizes_is_the_whole_pair_plan(which, monkeypatch):
    """a launch of 24 row tiles is modelled at far less than the analysis costs: not engaged, not even analysed,
    and info, table and G are those of OBHIP_GRAM_DEDUP_QUADS=0"""
    from outerbase_amd import obmod
    m, c = model(which), rows(which, 1500)
    got = {}
    for sw in ("0", None):
        if sw is None:
            monkeypatch.delenv("OBHIP_GRAM_DEDUP_QUADS")
        else:
            monkeypatch.setenv("OBHIP_GRAM_DEDUP_QUADS", sw)
        t = obmod._Terms(m["om_d"], m["terms"])
        G = gram(m["om_d"], t, c["x"], poison=True)
        assert quads_info(t)[1:] == (0, 0, 0)
        got[sw] = (info(t)[:2], fill_table(t), G)
    assert got[None][0] == got["0"][0] and got[None][0][1] == EXPECT[which][4]
    assert np.array_equal(got[None][1], got["0"][1]) and np.array_equal(got[None][2], got["0"][2])
    skipped = got[None][1] >= 0
    assert np.count_nonzero(skipped) == 128 * 128 * EXPECT[which][4]


def test_sharded_fit_fills_the_packed_triangle_before_the_exchange(monkeypatch):
    """Two simulated ranks on p384: the exchanged buffer is twice the packed upper triangle of the one-rank G (the
    dropped wave tile filled BEFORE the sum over the ranks); theta is finite and solves the normal equations to
    the 1e-10 of the whole-pair test of the same name, within the decade of the switched-off run's residual."""
    import torch
    from outerbase_amd._lib import call
    from outerbase_amd.driver import HotPath
    terms, n, p = constructed_terms("p384"), 1500, 384
    monkeypatch.setenv("OBHIP_GRAM_DEDUP_QUADS", "1")
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("OBHIP_GRAM_DEDUP", sw)
        hp = HotPath(KINDS6, 20, p, n, rank=0, world=2, transport="sim", row0=0, n_total=2 * n, terms=terms)
        hp.setup()
        hp.step()
        torch.cuda.synchronize()
        assert quads_info(hp.t)[1:] == ((1, 5, 1) if sw == "1" else (0, 0, 0))
        G = torch.empty((p, p), dtype=torch.float64, device="cuda")
        call("obhip_gram_dev", hp.basis, hp.t._h, None, G.data_ptr(), None)
        torch.cuda.synchronize()
        tri = p * (p + 1) // 2
        ex, G = hp.exbuf.cpu().numpy(), G.cpu().numpy()
        theta = hp.theta.cpu().numpy()
        res[sw] = (hp.newton_residual_rel(), theta)
        hp.close()
        assert np.array_equal(G, G.T) and np.array_equal(ex[:tri], 2.0 * G[np.triu_indices(p)])
        assert np.all(np.isfinite(theta))
    print("newton_residual_rel: switched off %.3g, on %.3g" % (res["0"][0], res["1"][0]))
    assert res["1"][0] < 1e-10 and res["1"][0] <= 10.0 * res["0"][0]
