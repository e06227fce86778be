"""Tile pairs of the panel Gram whose entries all repeat elsewhere in G get no task (gram_dedup.hip).

G[s][t] depends on the per-dimension unordered level pairs {s_k, t_k} only, so the entries of such a
tile pair are copied from tile pairs nearer the diagonal.  Checked here: the kept entries are the
bits of the switched-off run (OBHIP_GRAM_DEDUP=0), G is exactly symmetric, every entry -- copied ones
included -- is within the tolerance tests/extended_ref.py's ref_gram gives for a computed entry (no
tolerance of this file's own), and the fill table names sources whose level pairs ARE the entry's.

The constructed term set: d = 6, terms (l0, l1, l2, l3, u, v) with l0, l1, l2 in 0..3 and l3 in
0..1 (128 base terms) repeated for (u, v) = (0,0), (1,0), (0,1), (1,1).  Tile pair (0, 3) pairs
(.,0,0) with (.,1,1), tile pair (1, 2) pairs (.,1,0) with (.,0,1): the same unordered pairs {0,1},
{0,1} in the last two dimensions, and (1, 2) is nearer the diagonal, so (0, 3) is redundant.

With OBHIP_GRAM_DEDUP_HASHBITS=8 distinct entries share their hash by the thousand; the exact
comparison with the segment head then fails and, by the rule of the analysis, such an entry counts
as unique and its tile pair is computed.  So under collisions the skipped count can only fall (it
is printed, and asserted not to rise); what must hold is everything else.  With 26 bits collisions
and the skip meet: a NumPy restatement of the device's hash over the constructed set's 131 328
upper-triangle entries (27 000 distinct) counts 130 453 entries whose segment head is another entry
at 8 bits, 187 at 24 bits (tile pair (0, 3) kept in both), 41 at 26 bits, none of them in tile pair
(0, 3), which is then skipped and filled -- the fill path under collisions -- and none from 28 bits."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import extended_ref as E
from conftest import knots_for, make_pair, sample_x

pytestmark = pytest.mark.gpu

KINDS6 = ["mat25", "mat25pow", "mat25ang", "mat25", "mat25", "mat25pow"]


def constructed_terms():
    base = list(itertools.product(range(4), range(4), range(4), range(2)))
    return np.array([list(s) + [u, v] for (u, v) in ((0, 0), (1, 0), (0, 1), (1, 1)) for s in base], dtype=np.int64)


def single_factor_terms(d, levels):
    """one factor per term, every (dimension, level) once: no two entries of the upper triangle of
    G share their level pairs"""
    t = np.zeros((d * levels, d), dtype=np.int64)
    for k in range(d):
        for l in range(levels):
            t[k * levels + l, k] = l + 1
    return t


@functools.lru_cache(maxsize=None)
def small_model(which):
    import outerbase_amd as ob
    if which == "constructed":
        kinds, terms = KINDS6, constructed_terms()
    elif which == "single":
        kinds, terms = ["mat25"] * 20, single_factor_terms(20, 19)      # p = 380: three tiles, the last padded
    else:
        kinds, terms = ["mat25", "mat25pow", "mat25ang", "mat25"], None  # p = 127 / 129: test_gpu_extended's "mixed d4"
    om_o, om_d = make_pair(kinds, knots_for(kinds, 20))
    if terms is None:
        terms = om_d.selectterms(int(which))
    rot, _, _ = om_d.rotation()
    knots = [np.asarray(k, dtype=np.float64) for k in knots_for(kinds, 20)]
    return dict(kinds=kinds, knots=knots, om_o=om_o, om_d=om_d, hyp=ob.gethyp(om_d), rot=rot, terms=np.asarray(terms))


@functools.lru_cache(maxsize=4)
def small_rows(which, n):
    """x and the long double reference of G on ALL columns, computed once and shared"""
    import ob_oracle as O
    m = small_model(which)
    x = sample_x(np.random.default_rng(77 + n), n, m["kinds"])
    ref = E.ExtendedRef(m["kinds"], m["knots"], m["hyp"], m["rot"], x)
    B, bB = ref.getmat(m["terms"])
    Bo = O.ob_getmat(O.OuterBase(m["om_o"], x), m["terms"])
    Cc = E.constant_from_oracle_ratio(E.worst_ratio(Bo, B, bB))
    cols = np.arange(B.shape[1])
    want, tol = E.ref_gram(B, bB, cols, Cc)
    for a in (want, tol):
        a.setflags(write=False)
    return dict(x=x, cols=cols, want=want, tol=tol)


def info(t):
    from outerbase_amd._lib import call
    pairs, skipped, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    call("obhip_gram_dedup_info", t._h, C.byref(pairs), C.byref(skipped), C.byref(ms))
    return pairs.value, skipped.value, ms.value


def fill_table(t):
    import torch
    from outerbase_amd._lib import call
    src = torch.empty((t.p, t.p), dtype=torch.int64, device="cuda")
    call("obhip_gram_dedup_table_dev", t._h, src.data_ptr())
    torch.cuda.synchronize()
    return src.cpu().numpy()


def gram(om, t, x, poison=False):
    """obhip_gram_dev on a basis of its own (so that OBHIP_GRAM_CHUNK_ROWS decides the path).
    poison: first a Gram of OTHER rows of the same shape with every tile pair computed, so that the
    partial-tile workspace a reused allocation hands this run holds sums of other data in every slot:
    a kept tile pair without a task could not pass by what an earlier run left there"""
    if poison:
        os.environ["OBHIP_GRAM_DEDUP"] = "0"
        try:
            u = (x - 0.02)[::-1]
            gram(om, t, 0.02 + 0.98 * u * u / u.max(axis=0))   # other rows, inside the same domain
        finally:
            del os.environ["OBHIP_GRAM_DEDUP"]
    import torch
    from outerbase_amd._lib import call, lib
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    h = C.c_void_p()
    call("obhip_basis_create_dev", C.byref(h), om._h, dx.data_ptr(), x.shape[0], t.maxlevels().ctypes.data)
    try:
        G = torch.full((t.p, t.p), float("nan"), dtype=torch.float64, device="cuda")
        call("obhip_gram_dev", h, t._h, None, G.data_ptr(), None)
        torch.cuda.synchronize()
    finally:
        lib.obhip_basis_destroy(h)
    return G.cpu().numpy()


def skipped_mask(src):
    """p x p: True on the entries of skipped tile pairs and on their mirrors"""
    m = src >= 0
    return m | m.T


def check_table_sound(terms, src):
    """every entry of a skipped tile pair against its source: the per-dimension unordered level
    pairs, recomputed here, must be the same, and the source must be an entry that is computed"""
    p = len(terms)
    s, t = np.nonzero(src >= 0)
    assert np.all(s < t)
    q = src[s, t]
    ss, st = q // p, q % p
    assert np.all(ss <= st) and np.all(src[ss, st] < 0), "a source lies in a skipped tile pair"
    lo, hi = np.minimum(terms[s], terms[t]), np.maximum(terms[s], terms[t])
    lo2, hi2 = np.minimum(terms[ss], terms[st]), np.maximum(terms[ss], terms[st])
    assert np.array_equal(lo, lo2) and np.array_equal(hi, hi2)
    # whole tile pairs, none on the diagonal
    tiles = set(zip((s // 128).tolist(), (t // 128).tolist()))
    assert all(i < j for i, j in tiles) and len(s) == 128 * 128 * len(tiles)
    return tiles


def compare_runs(label, om, t, terms, x, cols, want, tol, monkeypatch, min_skipped):
    """dedup on against the switched-off run and against the extended reference on rows `cols` of G"""
    monkeypatch.setenv("OBHIP_GRAM_DEDUP", "0")
    assert info(t)[1] == 0
    G0 = gram(om, t, x)
    monkeypatch.delenv("OBHIP_GRAM_DEDUP")
    pairs, skipped, ms = info(t)
    src = fill_table(t)
    tiles = check_table_sound(terms, src)
    G1 = gram(om, t, x, poison=True)
    sk = skipped_mask(src)
    r0, r1 = E.worst_ratio(G0[cols, :], want, tol), E.worst_ratio(G1[cols, :], want, tol)
    on_copied = E.worst_ratio(G1[cols, :][sk[cols, :]], want[sk[cols, :]], tol[sk[cols, :]]) if sk[cols, :].any() else 0.0
    print("%s: %d of %d tile pairs skipped %s, analysis %.2f ms; err/tol switched off %.3g, on %.3g (copied entries %.3g)"
          % (label, skipped, pairs, sorted(tiles), ms, r0, r1, on_copied))
    assert len(tiles) == skipped and skipped >= min_skipped
    assert np.all(np.isfinite(G1)) and np.array_equal(G1, G1.T)
    assert np.array_equal(G1[~sk], G0[~sk]), "a kept entry differs from the switched-off run"
    assert r1 <= 1.0
    return skipped, tiles


@pytest.mark.parametrize("n,chunk_rows,hashbits", [(200, None, None), (1500, None, None), (1500, 512, None),
                                                   (200, 64, None), (1500, None, 8), (1500, 512, 8),
                                                   (1500, None, 24), (1500, None, 26), (1500, 512, 26)])
def test_constructed_set(n, chunk_rows, hashbits, monkeypatch):
    """d = 6, p = 512 (module docstring): tile pair (0, 3) is copied from (1, 2) -- whole design
    matrix and row chunks (accumulating reductions, the fill after each), full and truncated hash."""
    from outerbase_amd import obmod
    m = small_model("constructed")
    c = small_rows("constructed", n)
    if chunk_rows:
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(chunk_rows))
    if hashbits:
        monkeypatch.setenv("OBHIP_GRAM_DEDUP_HASHBITS", str(hashbits))
    t = obmod._Terms(m["om_d"], m["terms"])
    skipped, tiles = compare_runs("constructed n = %d chunk %s hashbits %s" % (n, chunk_rows, hashbits), m["om_d"], t,
                                  m["terms"], c["x"], c["cols"], c["want"], c["tol"], monkeypatch,
                                  0 if hashbits in (8, 24) else 1)
    if hashbits in (8, 24):
        assert skipped <= 1      # collisions only ever keep a tile pair
    else:
        assert tiles == {(0, 3)}  # (checked on the CPU when the set was constructed; module docstring for 26 bits)


def test_mat25x8_p4096(monkeypatch):
    """test_gpu_extended's packed-diagonal set at n = 1500, on gram_column_sample's columns"""
    from outerbase_amd import obmod
    from test_gpu_extended import SEED, model, rows
    name, n = "mat25x8 p4096", 1500
    m, c = model(name), rows(name, n)
    cols = E.gram_column_sample(c["bB"], SEED[name])
    want, tol = E.ref_gram(c["B"], c["bB"], cols, c["C"])
    t = obmod._Terms(m["om_d"], m["terms"])
    compare_runs(name, m["om_d"], t, np.asarray(m["terms"], dtype=np.int64), c["x"], cols, want, tol, monkeypatch, 1)


@pytest.mark.parametrize("which,n", [("single", 300), ("127", 200), ("129", 200)])
def test_term_sets_without_repeats_change_nothing(which, n, monkeypatch):
    """nothing to skip (one factor per term; one and two tiles with padding): skipped == 0 and G is
    the switched-off run's bit for bit"""
    from outerbase_amd import obmod
    m = small_model(which)
    x = sample_x(np.random.default_rng(5), n, m["kinds"])
    t = obmod._Terms(m["om_d"], m["terms"])
    monkeypatch.setenv("OBHIP_GRAM_DEDUP", "0")
    G0 = gram(m["om_d"], t, x)
    monkeypatch.delenv("OBHIP_GRAM_DEDUP")
    pairs, skipped, ms = info(t)
    G1 = gram(m["om_d"], t, x)
    print("%s: p = %d, %d tile pairs, %d skipped, analysis %.2f ms" % (which, t.p, pairs, skipped, ms))
    assert skipped == 0 and not (fill_table(t) >= 0).any()
    assert np.array_equal(G0, G1) and np.array_equal(G1, G1.T)


def test_sharded_fit_fills_the_packed_triangle_before_the_exchange(monkeypatch):
    """Two simulated ranks on the constructed set: the exchanged buffer is twice the packed upper
    triangle of the one-rank G (the skipped tile pair filled BEFORE the sum over the ranks), theta
    is finite and solves the normal equations to the 1e-10 of
    test_sim_ranks_multi_fit_is_the_fit_of_the_shard_repeated and within the decade of the
    switched-off run's residual (both are rounding residue of the same solve)."""
    import torch
    from outerbase_amd._lib import call
    from outerbase_amd.driver import HotPath
    terms, n, p = constructed_terms(), 1500, 512
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("OBHIP_GRAM_DEDUP", sw)
        hp = HotPath(KINDS6, 20, p, n, rank=0, world=2, transport="sim", row0=0, n_total=2 * n, terms=terms)
        hp.setup()
        hp.step()
        torch.cuda.synchronize()
        assert info(hp.t)[1] == (1 if sw == "1" else 0)
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
    print("newton_residual_rel: switched off %.3g, on %.3g; max |theta on - off| / max |theta| %.3g"
          % (res["0"][0], res["1"][0], np.max(np.abs(res["1"][1] - res["0"][1])) / np.max(np.abs(res["0"][1]))))
    assert res["1"][0] < 1e-10 and res["1"][0] <= 10.0 * res["0"][0]
