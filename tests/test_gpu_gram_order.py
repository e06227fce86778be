"""The panel Gram in its own column order (csrc/gram_order.h, gram_dedup.hip), forced with OBHIP_GRAM_ORDER=1: the
columns staged in a stable sort by factor count, the wave tiles dropped by the sequential pass, every result back
in the caller's term coordinates.

Term sets (tests/test_gram_order_host.py: small_sets): the two constructed d = 6 sets of test_gpu_gram_quads.py
shuffled by a fixed seed -- terms of 0 - 5 factors interleaved, so the permutation moves terms across tile
boundaries -- and p300, whose padding columns must stay last and whose wave tile (0, 3) of Gram order drops while
the parallel rule on the shuffled order drops nothing; and p256, where the device's walk must take a wave tile off
the counts and put it back.  n = 1000 and 4097; whole, in three row chunks, and through two simulated ranks (the
packed sink).

Checked: the device's mask is the NumPy restatement's, tile for tile; G finite (the sink starts as NaN and the
workspace is poisoned: no entry left unwritten) and exactly symmetric; every entry within tests/extended_ref.py's
ref_gram tolerance (no number of this file's own), the worst err/tol printed for kept and copied entries apart;
the table's sources, mapped back to term coordinates, hold the entry's own level pairs and are computed entries;
with the switch at 0 and unset G, info and table are equal bit for bit (nothing engages at these sizes: the code
that runs is the parent's); B^T Y of the fused staging and of the multi-response pass on an ordered staged matrix
equal the switched-off run's bit for bit (the same sums in the same order, written to their terms); diagH and
the coefficients of a multi-response fit agree with the switched-off run at the multi-response test's 1e-10
and 1e-6."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_ref as E
from conftest import knots_for, make_pair, sample_x
from test_gpu_gram_dedup import KINDS6, fill_table, gram, info
from test_gpu_gram_quads import quads_info
from test_gram_order_host import sequential_pass, small_sets, stable_factor_sort

pytestmark = pytest.mark.gpu

CHUNK_ROWS = {1000: 384, 4097: 1408}     # three chunks of the 16 and the 65 row tiles


@functools.lru_cache(maxsize=None)
def model(which):
    import outerbase_amd as ob
    om_o, om_d = make_pair(KINDS6, knots_for(KINDS6, 20))
    rot, _, _ = om_d.rotation()
    knots = [np.asarray(k, dtype=np.float64) for k in knots_for(KINDS6, 20)]
    terms = small_sets()[which]
    perm = stable_factor_sort(terms)
    drops, _, _ = sequential_pass(terms[perm])
    return dict(om_o=om_o, om_d=om_d, hyp=ob.gethyp(om_d), rot=rot, knots=knots, terms=terms, perm=perm, drops=drops)


@functools.lru_cache(maxsize=None)
def rows(which, n):
    """x and the long double reference of G on all columns, computed once and shared"""
    import ob_oracle as O
    m = model(which)
    x = sample_x(np.random.default_rng(277 + n), n, KINDS6)
    ref = E.ExtendedRef(KINDS6, m["knots"], m["hyp"], m["rot"], x)
    B, bB = ref.getmat(m["terms"])
    Bo = O.ob_getmat(O.OuterBase(m["om_o"], x), m["terms"])
    Cc = E.constant_from_oracle_ratio(E.worst_ratio(Bo, B, bB))
    want, tol = E.ref_gram(B, bB, np.arange(B.shape[1]), Cc)
    for arr in (want, tol):
        arr.setflags(write=False)
    return dict(x=x, want=want, tol=tol)


def check_table(m, src):
    """the table in term coordinates: every dropped entry's source holds its level pairs and is computed; mapped to
    Gram order the dropped entries are whole wave tiles -- returned"""
    terms, p = m["terms"], len(m["terms"])
    s, t = np.nonzero(src >= 0)
    assert np.all(s < t)
    q = src[s, t]
    ss, st = q // p, q % p
    assert np.all(ss < st) and np.all(src[ss, st] < 0), "a source is a dropped entry"
    assert np.array_equal(np.minimum(terms[s], terms[t]), np.minimum(terms[ss], terms[st]))
    assert np.array_equal(np.maximum(terms[s], terms[t]), np.maximum(terms[ss], terms[st]))
    inv = np.argsort(m["perm"])
    gs, gt = np.minimum(inv[s], inv[t]), np.maximum(inv[s], inv[t])
    tiles = set(zip((gs // 64).tolist(), (gt // 64).tolist()))
    assert len(s) == 64 * 64 * len(tiles)
    return tiles


@pytest.mark.parametrize("n", [1000, 4097])
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("which", ["p384", "p512", "p300", "p256"])
def test_ordered_gram(which, chunked, n, monkeypatch):
    from outerbase_amd import obmod
    m, c = model(which), rows(which, n)
    terms, p = m["terms"], len(m["terms"])
    assert len(m["drops"]) >= 1 and not np.array_equal(m["perm"], np.arange(p))
    if chunked:
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(CHUNK_ROWS[n]))
    # switched off and unset: the same bits, the same reports, nothing of the order
    got = {}
    for sw in ("0", None):
        if sw is None:
            monkeypatch.delenv("OBHIP_GRAM_ORDER", raising=False)
        else:
            monkeypatch.setenv("OBHIP_GRAM_ORDER", sw)
        t = obmod._Terms(m["om_d"], terms)
        G = gram(m["om_d"], t, c["x"], poison=True)
        oi = t.gram_order_info()
        assert (oi["engaged"], oi["dropped"], oi["blocks_per_split"], oi["setup_ms"]) == (False, 0, 0, 0.0)
        got[sw] = (info(t)[:2], quads_info(t), fill_table(t), G)
    assert got[None][:2] == got["0"][:2]
    assert np.array_equal(got[None][2], got["0"][2]) and np.array_equal(got[None][3], got["0"][3])
    G0 = got["0"][3]
    # forced
    monkeypatch.setenv("OBHIP_GRAM_ORDER", "1")
    t = obmod._Terms(m["om_d"], terms)
    oi = t.gram_order_info()
    ng = 2 * ((p + 127) // 128)
    assert oi["engaged"] and oi["dropped"] == len(m["drops"]) and oi["setup_ms"] > 0.0
    assert quads_info(t) == (ng * (ng + 1) // 2, len(m["drops"]), oi["blocks_per_split"], 1)
    src = fill_table(t)
    assert check_table(m, src) == m["drops"], "the device's mask is not the serial definition's"
    G1 = gram(m["om_d"], t, c["x"], poison=True)
    assert t.gram_order_info()["engaged"]
    copied = (src >= 0) | (src >= 0).T
    r0 = E.worst_ratio(G0, c["want"], c["tol"])
    kept = E.worst_ratio(G1[~copied], c["want"][~copied], c["tol"][~copied])
    cop = E.worst_ratio(G1[copied], c["want"][copied], c["tol"][copied])
    print("%s n = %d chunked %s: %d wave tiles dropped, %d blocks per split, set-up %.2f ms; err/tol switched off %.3g, "
          "ordered: kept entries %.3g, copied entries %.3g" % (which, n, chunked, oi["dropped"], oi["blocks_per_split"],
                                                              oi["setup_ms"], r0, kept, cop))
    assert np.all(np.isfinite(G1)) and np.array_equal(G1, G1.T)
    assert kept <= 1.0 and cop <= 1.0


@pytest.mark.parametrize("n", [1000, 4097])
@pytest.mark.parametrize("which", ["p384", "p512", "p300"])
def test_two_ranks_fill_the_packed_triangle(which, n, monkeypatch):
    """two simulated ranks: the exchanged buffer is twice the packed upper triangle of the one-rank G of the same
    switch -- the packed sink takes every entry, kept and copied, at (min, max) of its terms -- and theta solves the
    normal equations as well as the switched-off run's"""
    import torch
    from outerbase_amd._lib import call
    from outerbase_amd.driver import HotPath
    m = model(which)
    terms, p = m["terms"], len(m["terms"])
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("OBHIP_GRAM_ORDER", sw)
        hp = HotPath(KINDS6, 20, p, n, rank=0, world=2, transport="sim", row0=0, n_total=2 * n, terms=terms)
        hp.setup()
        hp.step()
        torch.cuda.synchronize()
        assert hp.t.gram_order_info()["engaged"] == (sw == "1")
        G = torch.empty((p, p), dtype=torch.float64, device="cuda")
        call("obhip_gram_dev", hp.basis, hp.t._h, None, G.data_ptr(), None)
        torch.cuda.synchronize()
        tri = p * (p + 1) // 2
        ex, G, theta = hp.exbuf.cpu().numpy(), G.cpu().numpy(), hp.theta.cpu().numpy()
        res[sw] = (hp.newton_residual_rel(), ex[tri:tri + p].copy())
        hp.close()
        assert np.array_equal(G, G.T) and np.array_equal(ex[:tri], 2.0 * G[np.triu_indices(p)])
        assert np.all(np.isfinite(theta))
    print("%s n = %d newton_residual_rel: switched off %.3g, ordered %.3g" % (which, n, res["0"][0], res["1"][0]))
    assert np.array_equal(res["1"][1], res["0"][1]), "B^T y of the fused staging is not in term coordinates"
    assert res["1"][0] < 1e-10 and res["1"][0] <= 10.0 * res["0"][0]


def test_a_launch_that_cannot_take_the_order_reports_so(monkeypatch):
    """forced, but staged by the generic kernel, which takes no column order: the launch runs in the terms' own
    order, G is the switched-off run's bit for bit, and the info entries and the table describe that launch"""
    from outerbase_amd import obmod
    m, c = model("p384"), rows("p384", 1000)
    monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    got = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("OBHIP_GRAM_ORDER", sw)
        t = obmod._Terms(m["om_d"], m["terms"])
        G = gram(m["om_d"], t, c["x"], poison=True)
        assert not t.gram_order_info()["engaged"]
        got[sw] = (quads_info(t), fill_table(t), G)
    assert got["1"][0] == got["0"][0]
    assert np.array_equal(got["1"][1], got["0"][1]) and np.array_equal(got["1"][2], got["0"][2])


@pytest.mark.parametrize("which,n", [("p384", 1000), ("p300", 4097)])
def test_multi_response_fit_after_an_ordered_gram(which, n, monkeypatch):
    """q = 10 responses (the nine beyond the first go through the multi-response pass over the staged matrix,
    which is in Gram order): B^T Y bit for bit the switched-off run's, diagH (e2 G + the prior precision on the
    diagonal, by term) at 1e-10 and the coefficients at 1e-6 relative, the multi-response test's own"""
    import torch
    from outerbase_amd import obmod
    from outerbase_amd._lib import call, lib
    from test_gpu_multi_response import RHO, SIGMA, _dev, _responses, _standardised
    m, c = model(which), rows(which, n)
    terms, p, q = m["terms"], len(m["terms"]), 10
    x = c["x"]
    Y = _standardised(_responses(x, np.sin(3.0 * x[:, 0]) + x[:, 1] * x[:, 3], q))
    out = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("OBHIP_GRAM_ORDER", sw)
        t = obmod._Terms(m["om_d"], terms)
        dx, dY = _dev(x), _dev(Y)
        h = C.c_void_p()
        call("obhip_basis_create_dev", C.byref(h), m["om_d"]._h, dx.data_ptr(), n, t.maxlevels().ctypes.data)
        try:
            wsb = C.c_uint64(0)
            call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
            ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
            H = torch.full((p, p), float("nan"), dtype=torch.float64, device="cuda")
            g = torch.full((q, p), float("nan"), dtype=torch.float64, device="cuda")
            th = torch.full((q, p), float("nan"), dtype=torch.float64, device="cuda")
            dh = torch.full((p,), float("nan"), dtype=torch.float64, device="cuda")
            call("obhip_fit_newton_multi_dev", None, h, t._h, m["om_d"]._h, dY.data_ptr(), q, dY.shape[1], SIGMA, RHO,
                 H.data_ptr(), g.data_ptr(), th.data_ptr(), dh.data_ptr(), None, 0, ws.data_ptr(), wsb.value)
            torch.cuda.synchronize()
            assert t.gram_order_info()["engaged"] == (sw == "1")
        finally:
            lib.obhip_basis_destroy(h)
        out[sw] = (g.cpu().numpy(), th.cpu().numpy(), dh.cpu().numpy())
    (g0, th0, dh0), (g1, th1, dh1) = out["0"], out["1"]
    assert np.all(np.isfinite(th1)) and np.all(np.isfinite(dh1))
    assert np.array_equal(g1, g0), "B^T Y of the ordered staged matrix is not in term coordinates"
    assert np.allclose(dh1, dh0, rtol=1e-10, atol=0.0)
    worst = max(np.max(np.abs(th1[j] - th0[j])) / np.max(np.abs(th0[j])) for j in range(q))
    print("%s n = %d: theta against the switched-off run %.3g (relative, worst response)" % (which, n, worst))
    assert worst < 1e-6
