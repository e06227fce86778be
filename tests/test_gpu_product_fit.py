"""The Newton fit on gridded data on the GPU (obhip_normal_acc_add_product_dev, obhip_product_side_dev;
NewtonAccumulator.add_product / remove_product, fit_newton_product, product_side) against the long-double
reference of tests/product_fit_ref.py on the expanded rows, per entry, with the staging kernel's tile in LDS and
-- OBHIP_FORCE_GENERIC -- in HBM.  product_fit_ref.py's docstring says where every tolerance comes from; the fits
are held to test_gpu_stream._against_one_shot's backward-error rule, restated here:
eta <= max(4 eta of the one-shot fit on the expanded rows, p 2^-53).  Every check prints its figures
(test_gpu_extended.Report) before the case asserts."""
import functools
import math

import numpy as np
import pytest

import extended_ref as E
import product_fit_ref as F
import product_ref as P
from conftest import sample_x
from multi_schedule_worker import backward_errors
from test_gpu_extended import SEED, Report, model
from test_gpu_product import big_model, blocks

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIGMA, RHO = math.log(0.01), 6.0
D4 = "mixed d4 p700"
ROUTES = ("fused", "hbm")


def route(monkeypatch, which):
    if which == "hbm":
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


@functools.lru_cache(maxsize=None)
def sub_model(p, keep=None, dims_b=()):
    """the first p of mixed d4's 700 selected terms -- of those with no factor on the dimensions dims_b
    (keep = "none") or with at least one (keep = "all")"""
    m = model(D4)
    terms = np.asarray(m["terms"])
    if keep is not None:
        has = (terms[:, list(dims_b)] > 0).any(1)
        terms = terms[has if keep == "all" else ~has]
    assert len(terms) >= p
    out = {k: v for k, v in m.items() if not k.startswith("_")}
    out["terms"] = np.ascontiguousarray(terms[:p])
    return out


def responses(xa, xb, q, seed):
    """(na, nb, q) raw responses: smooth in both blocks, a little noise, another scale and offset per column"""
    rng = np.random.default_rng(seed)
    a, b = xa.sum(1)[:, None], xb.sum(1)[None, :]
    cols = [(1.0 + r) * (np.cos(2.0 * a + 0.3 * r) * (1.0 + b) + np.sin(3.0 * b) + 0.05 * rng.standard_normal((len(xa), len(xb))))
            - 3.0 * r + 2.0 for r in range(q)]
    return np.stack(cols, axis=2)


def full(tri, p):
    G = np.zeros((p, p))
    G[np.triu_indices(p)] = tri
    return G + np.triu(G, 1).T


def same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def add_dev(acc, xa, xb, Y, dims_b, pad=0, sign=+1):
    """the device entry with lda = na + pad, the padding filled with NaN: read once, it would show everywhere"""
    import torch
    from outerbase_amd.product import check_dims_b
    na, nb, q = Y.shape
    Yp = np.full((q, nb, na + pad), np.nan)
    Yp[:, :, :na] = Y.transpose(2, 1, 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    acc._product_batch_dev(t(xa.T), t(xb.T), t(Yp), na, nb, check_dims_b(acc.om.d, dims_b), na + pad, sign)


def check_state(rep, label, st, ref, Y, cols, extra=0):
    """triangle on the sampled columns, B^T (Y - shift) and B^T 1 of an exported state against the reference"""
    q = Y.shape[2]
    rep.check(label + " triangle", full(st["tri"], ref.p)[cols, :], *ref.gram(cols, extra))
    V = Y - st["shift"][None, None, :]         # as the device forms it: one IEEE subtraction per entry
    for r in range(q):
        rep.check(label + " B^T (y_%d - c)" % r, st["rhs"][:, r], *ref.tmatmul(ref.flat(V[:, :, r]), extra))
    rep.check(label + " B^T 1", st["b1"], *ref.tmatmul(np.ones(ref.na * ref.nb), extra))


def check_moments(label, st, Yrows):
    """test_gpu_stream's figures: 1e-13 for the mean relative to max(|mean|, sd), 1e-12 for the sd"""
    n = len(Yrows)
    assert np.all(st["n"] == n)
    if n < 2:
        return
    cent, sd = st["shift"] + st["mu"], np.sqrt(st["M2"] / (n - 1))
    wc, ws = Yrows.mean(0), Yrows.std(0, ddof=1)
    ec = float(np.max(np.abs(cent - wc) / np.maximum(np.abs(wc), ws)))
    es = float(np.max(np.abs(sd - ws) / ws))
    print("%s: mean err / max(|mean|, sd) %.3g (1e-13), sd rel err %.3g (1e-12)" % (label, ec, es))
    assert ec <= 1e-13 and es <= 1e-12


# ---- 1. the staged side matrices -----------------------------------------------------------------
@pytest.mark.parametrize("which", ROUTES)
@pytest.mark.parametrize("p", [1, 63, 129, 300])
def test_side_matrices_per_entry(p, which, monkeypatch):
    import outerbase_amd as ob
    route(monkeypatch, which)
    m, dims_b = sub_model(p), (1, 3)
    Cc = E.constant_from_oracle_ratio(P.probe_ratio(m, SEED[D4]))
    assert ob.product_fit_layout(m["om_d"], m["terms"], dims_b)[2:] == (True, True)
    rep = Report("sides p=%d %s" % (p, which))
    for n in (1, 63, 64, 65, 129):
        x = sample_x(np.random.default_rng(SEED[D4] + n), n, m["kinds"])
        for side, dims in ((0, P.dims_a_of(4, dims_b)), (1, list(dims_b))):
            got = ob.product_side(m["om_d"], m["terms"], x[:, dims], dims_b, side, padded=True)
            assert got.shape == ((n + 63) // 64 * 64, (p + 255) // 256 * 256)
            assert np.all(got[n:] == 0.0) and np.all(got[:, p:] == 0.0), "pad rows and columns are exact zeros"
            rep.check("n=%d side %d" % (n, side), got[:n, :p], *F.side_ref(m, x[:, dims], dims, Cc))
    rep.done()


@functools.lru_cache(maxsize=None)
def many_factor_model():
    """d = 12: terms with 9, 10 and 11 factors among the first eleven dimensions (levels 1 and 2), some short
    ones and the constant: side A of dims_b = (11,) needs a column list of width 12, beyond the fused form's 8"""
    m = big_model()
    rng = np.random.default_rng(5)
    terms = [np.zeros(12, dtype=np.int64)]
    for nnz in (9, 10, 11, 11, 10, 9, 3, 1, 2):
        t = np.zeros(12, dtype=np.int64)
        t[rng.choice(11, size=nnz, replace=False)] = rng.integers(1, 3, size=nnz)
        t[11] = rng.integers(0, 3)
        terms.append(t)
    out = {k: v for k, v in m.items() if not k.startswith("_")}
    out["terms"] = np.unique(np.stack(terms), axis=0)
    return out


def test_side_matrix_of_terms_with_nine_to_eleven_factors():
    import outerbase_amd as ob
    m, dims_b = many_factor_model(), (11,)
    nnz_a = (m["terms"][:, :11] > 0).sum(1)
    assert nnz_a.max() == 11 and {9, 10, 11} <= set(nnz_a.tolist())
    mu_a, mu_b, fa, fb = ob.product_fit_layout(m["om_d"], m["terms"], dims_b)
    assert not fa and fb, "side A is meant for the HBM form by its factor count"
    Cc = E.constant_from_oracle_ratio(P.probe_ratio(m, 4242))
    rep = Report("sides, 9-11 factors")
    for n in (1, 65, 129):
        x = sample_x(np.random.default_rng(900 + n), n, m["kinds"])
        for side, dims in ((0, list(range(11))), (1, [11])):
            got = ob.product_side(m["om_d"], m["terms"], x[:, dims], dims_b, side, padded=True)
            assert np.all(got[n:] == 0.0) and np.all(got[:, len(m["terms"]):] == 0.0)
            rep.check("n=%d side %d" % (n, side), got[:n, :len(m["terms"])], *F.side_ref(m, x[:, dims], dims, Cc))
    rep.done()


# ---- 2. the state --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def reference(p, keep, dims_b, na, nb):
    m = sub_model(p, keep, dims_b if keep else ())
    xa, xb = blocks(m, SEED[D4], na, nb, dims_b)
    ref = F.ProductFitRef(m, xa, xb, dims_b, SEED[D4])
    print("p=%d %s | %d x %d, dims_b = %s: oracle err/bound %.3g, C = %.3g" % (p, keep, na, nb, list(dims_b), ref.ratio, ref.C))
    return m, xa, xb, ref


# p, terms kept, dims_b (first / last / interleaved dimensions), (na, nb), q, lda - na, rows per chunk (0: by memory)
STATE_CASES = [
    (129, None, (0,), (1, 65), 1, 0, 0),
    (129, None, (3,), (64, 64), 3, 7, 0),
    (300, None, (1, 3), (65, 129), 17, 0, 64),
    (63, None, (0, 1), (129, 3), 1, 7, 64),
    (129, None, (0, 2), (129, 130), 3, 7, 64),
    (100, "none", (1, 3), (65, 129), 1, 0, 0),
    (100, "all", (2, 3), (64, 64), 3, 0, 64),
]


@pytest.mark.parametrize("p,keep,dims_b,shape,q,pad,chunk", STATE_CASES)
def test_state_per_entry(p, keep, dims_b, shape, q, pad, chunk, monkeypatch):
    import outerbase_amd as ob
    m, xa, xb, ref = reference(p, keep, dims_b, *shape)
    if keep:
        on_b = (np.asarray(m["terms"])[:, list(dims_b)] > 0).any(1)
        assert on_b.all() if keep == "all" else not on_b.any()
    Y = responses(xa, xb, q, 11 + p)
    cols = E.gram_column_sample(ref.bB, 4242 + p)
    if chunk:
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(chunk))
    rep = Report("state p=%d %s %s %dx%d q=%d lda+%d chunk %d" % (p, keep, list(dims_b), shape[0], shape[1], q, pad, chunk))
    for which in ROUTES:
        route(monkeypatch, which)
        with ob.NewtonAccumulator(m["om_d"], m["terms"], q) as acc:
            add_dev(acc, xa, xb, Y, dims_b, pad)
            assert acc.rows == shape[0] * shape[1] and acc.batches == 1 and acc.grad_rows == 0
            st = acc.state()
        assert np.array_equal(st["shift"], Y[0, 0])
        check_state(rep, which, st, ref, Y, cols)
        check_moments(which, st, Y.reshape(-1, q))
    rep.done()


def test_add_and_remove():
    """add(G1); add(G2); remove(G2) against G1's reference under the rule over everything that ever went in; a
    state emptied by removal is reset"""
    import outerbase_amd as ob
    p, dims_b, q = 129, (1, 3), 3
    m, xa, xb, ref = reference(p, None, dims_b, 65, 64)
    xa2, xb2 = blocks(m, SEED[D4] + 1, 64, 66, dims_b)
    ref2 = F.ProductFitRef(m, xa2, xb2, dims_b, SEED[D4])
    Y, Y2 = responses(xa, xb, q, 1), responses(xa2, xb2, q, 2)
    cols = E.gram_column_sample(ref.bB, 77)
    rep = Report("add, add, remove")
    with ob.NewtonAccumulator(m["om_d"], m["terms"], q) as acc:
        acc.add_product(xa, xb, Y, dims_b).add_product(xa2, xb2, Y2, dims_b)
        assert acc.rows == 65 * 64 + 64 * 66 and acc.batches == 2
        acc.remove_product(xa2, xb2, Y2, dims_b)
        assert acc.rows == 65 * 64 and acc.batches == 1
        st = acc.state()
        # what went in: G1's summands and G2's, each sum a product of two side sums; three folds
        k1, k2 = ref.k, ref2.k
        w, b1_, a1 = ref.gram_parts(cols)
        _, b2_, a2 = ref2.gram_parts(cols)
        kg = max(k1, k2) + F.extra_gram(4) + 3
        rep.check("triangle", full(st["tri"], p)[cols, :], w, E._sum_tol(max(ref.C, ref2.C), b1_ + b2_, kg, a1 + a2))
        kv = max(k1, k2) + F.extra_vec(4) + 3
        for r in range(q):
            w, bo, ab = ref.tm_parts(ref.flat(Y[:, :, r] - st["shift"][r]))
            _, bo2, ab2 = ref2.tm_parts(ref2.flat(Y2[:, :, r] - st["shift"][r]))
            rep.check("B^T (y_%d - c)" % r, st["rhs"][:, r], w, E._sum_tol(max(ref.C, ref2.C), bo + bo2, kv, ab + ab2))
        w, bo, ab = ref.tm_parts(np.ones(65 * 64))
        _, bo2, ab2 = ref2.tm_parts(np.ones(64 * 66))
        rep.check("B^T 1", st["b1"], w, E._sum_tol(max(ref.C, ref2.C), bo + bo2, kv, ab + ab2))
        check_moments("after the removal", st, Y.reshape(-1, q))
        acc.remove_product(xa, xb, Y, dims_b)
        assert acc.rows == 0 and acc.batches == 0
        assert all(np.all(v == 0.0) for v in acc.state().values()), "a state emptied by removal is reset"
    rep.done()


def test_grid_batch_mixed_with_rows_and_merged():
    """a grid batch plus an ordinary add of other rows, then merged with an accumulator of another shift (rows
    again): against the long-double sums over all rows, the rule applied to the summands that were added, as
    test_gpu_stream's merged_tol argues"""
    import outerbase_amd as ob
    p, dims_b, q = 129, (0, 2), 1
    m, xa, xb, ref = reference(p, None, dims_b, 65, 64)
    Y = responses(xa, xb, q, 3)
    rng = np.random.default_rng(8)
    xr, xs = sample_x(rng, 200, m["kinds"]), sample_x(rng, 150, m["kinds"])
    yr, ys = rng.standard_normal((200, 1)) + 1.0, rng.standard_normal((150, 1)) - 4.0
    ext = lambda x: E.ExtendedRef(m["kinds"], m["knots"], m["hyp"], m["rot"], x).getmat(m["terms"])
    (Br, bBr), (Bs, bBs) = ext(xr), ext(xs)
    cols = E.gram_column_sample(ref.bB, 78)
    rep = Report("grid + rows, merged")
    with ob.NewtonAccumulator(m["om_d"], m["terms"], q) as acc, ob.NewtonAccumulator(m["om_d"], m["terms"], q) as src:
        acc.add_product(xa, xb, Y, dims_b).add(xr, yr)
        src.add(xs, ys)
        acc.merge(src)
        n = 65 * 64 + 350
        assert acc.rows == n and acc.batches == 3
        st = acc.state()
        cA, cS = st["shift"][0], ys[0, 0]
        assert cA == Y[0, 0, 0] and cS != cA
        Cc = ref.C
        f, af = E._f64, lambda a: np.abs(E._f64(a))
        wg, bg, ag = ref.gram_parts(cols)
        for Bx, bx in ((Br, bBr), (Bs, bBs)):
            wg = wg + Bx[:, cols].T @ Bx
            bg = bg + E.gram_bound(Bx, bx, cols)
            ag = ag + af(Bx)[:, cols].T @ af(Bx)
        rep.check("triangle", full(st["tri"], p)[cols, :], wg, E._sum_tol(Cc, bg, 200 + F.extra_gram(4) + 3, ag))
        # R: the grid's and the rows' summands with y - c_A, the source's with y - c_S, then (c_S - c_A) B_s^T 1
        vg, vr, vs = ref.flat(Y[:, :, 0] - cA), yr[:, 0] - cA, ys[:, 0] - cS
        w, bo, ab = ref.tm_parts(vg)
        want = w + Br.T @ np.asarray(vr, dtype=E.ld) + Bs.T @ np.asarray(ys[:, 0] - cA, dtype=E.ld)
        bound = bo + f(bBr).T @ np.abs(vr) + f(bBs).T @ np.abs(vs) + abs(cS - cA) * f(bBs).sum(0)
        absum = ab + af(Br).T @ np.abs(vr) + af(Bs).T @ np.abs(vs) + abs(cS - cA) * af(Bs).sum(0)
        rep.check("B^T (y - c)", st["rhs"][:, 0], want, E._sum_tol(Cc, bound, 200 + F.extra_vec(4) + 3, absum) + 2 * U * absum)
        w, bo, ab = ref.tm_parts(np.ones(65 * 64))
        want = w + Br.sum(0) + Bs.sum(0)
        rep.check("B^T 1", st["b1"], want, E._sum_tol(Cc, bo + f(bBr).sum(0) + f(bBs).sum(0), 200 + F.extra_vec(4) + 3,
                                                      ab + af(Br).sum(0) + af(Bs).sum(0)))
        check_moments("merged", st, np.concatenate([Y.reshape(-1, 1), yr, ys]))
    rep.done()


def test_two_equal_calls_give_the_same_bits(monkeypatch):
    import outerbase_amd as ob
    m, xa, xb, _ = reference(300, None, (1, 3), 65, 129)
    Y = responses(xa, xb, 3, 4)
    monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", "64")
    states = []
    for _ in range(2):
        with ob.NewtonAccumulator(m["om_d"], m["terms"], 3) as acc:
            states.append(acc.add_product(xa, xb, Y, (1, 3)).state())
    assert same_state(*states)


# ---- 3. fits -------------------------------------------------------------------------------------
def against_one_shot(m, fit, x, Yrows, label, H=None, R=None):
    """test_gpu_stream._against_one_shot, restated: fit against fit_newton_multi on the rows x at once, and both
    against H and the right-hand side by the backward error.  H, R None: the oracle's, on the rows."""
    import ob_oracle as O
    import outerbase_amd as ob
    q, p = Yrows.shape[1], len(m["terms"])
    one = ob.fit_newton_multi(m["om_d"], m["terms"], x, Yrows)
    wt = max(np.max(np.abs(fit.coeff[:, j] - one.coeff[:, j])) / np.max(np.abs(one.coeff[:, j])) for j in range(q))
    # (a figure, not a criterion: the distance of two solutions is the backward error times the condition of H, and
    # a grid with three rows on one side determines few coefficients beyond the prior -- 2.3e-6 at 129 x 3, p = 63,
    # with both backward errors at 1.2e-15; 3.4e-7 at 64 x 64, 3e-9 at 65 x 129, measured on an MI355X)
    print("%s: Theta %.3g relative to the one-shot fit (worst column); diagH %.3g" % (label, wt, np.max(np.abs(fit.diagH / one.diagH - 1))))
    assert np.allclose(fit.diagH, one.diagH, rtol=1e-10, atol=0)
    ec = float(np.max(np.abs(fit.y_cent - one.y_cent) / np.maximum(np.abs(one.y_cent), one.y_sca)))
    es = float(np.max(np.abs(fit.y_sca - one.y_sca) / one.y_sca))
    print("%s: against the one-shot fit: mean err / max(|mean|, sd) %.3g (1e-13), sd rel err %.3g (1e-12)" % (label, ec, es))
    assert ec <= 1e-13 and es <= 1e-12
    if H is None:
        obo = O.OuterBase(m["om_o"], x)
        H = O.total_hess(obo, m["terms"], SIGMA, RHO)
        Ys = (Yrows - Yrows.mean(axis=0)) / Yrows.std(axis=0, ddof=1)
        R = math.exp(-2 * SIGMA) * (O.ob_getmat(obo, m["terms"]).T @ Ys)
    eta, eta1 = backward_errors(H, fit.coeff, R), backward_errors(H, one.coeff, R)
    lim = np.maximum(4 * eta1, p * U)
    print("%s: backward error grid %.3g, one-shot %.3g, worst eta / allowed %.3g" % (label, eta.max(), eta1.max(), np.max(eta / lim)))
    assert np.all(np.isfinite(eta)) and np.all(eta <= lim)
    return one


@pytest.mark.parametrize("p,keep,dims_b,shape,q,pad,chunk", STATE_CASES[1:5])
def test_fit_equals_the_fit_of_the_expanded_rows(p, keep, dims_b, shape, q, pad, chunk):
    import outerbase_amd as ob
    m = sub_model(p)
    xa, xb = blocks(m, SEED[D4], shape[0], shape[1], dims_b)
    Y = responses(xa, xb, q, 11 + p)
    fit = ob.fit_newton_product(m["om_d"], m["terms"], xa, xb, Y, dims_b)
    assert fit.coeff.shape == (p, q) and fit.sigma == SIGMA and fit.rho == RHO
    against_one_shot(m, fit, P.expand(xa, xb, dims_b), Y.reshape(-1, q), "%dx%d p=%d q=%d" % (shape[0], shape[1], p, q))


def test_fit_of_six_million_pairs():
    """na = 2000, nb = 3000, p = 300: no long-double reference; H and the right-hand side of the backward error
    come from an accumulator filled with the expanded rows (its state in float64) and the oracle's prior"""
    import ob_oracle as O
    import outerbase_amd as ob
    p, dims_b, q, na, nb = 300, (1, 3), 1, 2000, 3000
    m = sub_model(p)
    xa, xb = blocks(m, SEED[D4], na, nb, dims_b)
    Y = responses(xa, xb, q, 6)
    fit = ob.fit_newton_product(m["om_d"], m["terms"], xa, xb, Y, dims_b)
    x, Yr = P.expand(xa, xb, dims_b), Y.reshape(-1, q)
    with ob.NewtonAccumulator(m["om_d"], m["terms"], q) as acc:
        st = acc.add(x, Yr).state()
    n = na * nb
    e2 = math.exp(-2 * SIGMA)
    H = e2 * full(st["tri"], p) + np.diag(O.prior_prec(m["om_o"], m["terms"], RHO))
    sd = np.sqrt(st["M2"] / (n - 1))
    R = e2 * (st["rhs"] - st["b1"][:, None] * st["mu"][None, :]) / sd[None, :]
    against_one_shot(m, fit, x, Yr, "2000x3000 p=300", H, R)


# ---- 4. composition ------------------------------------------------------------------------------
def test_minus_of_a_block_of_xa_rows():
    """fit(minus=acc_block), the block of xa rows added as its own grid batch, against the fit of the remaining
    expanded rows; neither accumulator is written"""
    import outerbase_amd as ob
    p, dims_b, q = 129, (1, 3), 3
    m = sub_model(p)
    xa, xb = blocks(m, SEED[D4], 129, 64, dims_b)
    Y = responses(xa, xb, q, 7)
    hold = np.arange(40, 75)
    rest = np.setdiff1d(np.arange(129), hold)
    with ob.NewtonAccumulator(m["om_d"], m["terms"], q) as total, ob.NewtonAccumulator(m["om_d"], m["terms"], q) as block:
        total.add_product(xa, xb, Y, dims_b)
        block.add_product(xa[hold], xb, Y[hold], dims_b)
        before = total.state(), block.state()
        fit = total.fit(minus=block)
        assert same_state(before[0], total.state()) and same_state(before[1], block.state())
    against_one_shot(m, fit, P.expand(xa[rest], xb, dims_b), Y[rest].reshape(-1, q), "minus a block of xa")


def test_posterior_equals_the_posterior_of_the_rows():
    """acc.posterior() after add_product against the one of an accumulator filled by rows: logdet and var to the
    tolerances test_gpu_design.test_accumulator_route_forms_the_hessian_of_the_solve holds its two routes to --
    |va - vb| <= 2 C bound_d of design_ref, |logdet difference| <= 64 u p max(|logdet|, p)"""
    import design_ref as D
    import ob_oracle as O
    import outerbase_amd as ob
    from test_gpu_design import model as design_model
    om_o, om_d, terms = design_model("d8", 67)
    p, dims_b = len(terms), (5, 6, 7)
    rng = np.random.default_rng(43)
    x = sample_x(rng, 40 + 30, om_o.kinds)
    xa, xb = P.split_x(x[:40], dims_b)[0], P.split_x(x[40:], dims_b)[1]
    Y = responses(xa, xb, 2, 9)
    xnew = sample_x(rng, 65, om_o.kinds)
    sigma, rho = math.log(0.1), 1.0
    with ob.NewtonAccumulator(om_d, terms, 2) as grid, ob.NewtonAccumulator(om_d, terms, 2) as rows:
        grid.add_product(xa, xb, Y, dims_b)
        rows.add(P.expand(xa, xb, dims_b), Y.reshape(-1, 2))
        H = math.exp(-2 * sigma) * full(rows.state()["tri"], p) + np.diag(O.prior_prec(om_o, terms, rho))
        c = D.make_case(om_o, terms, H, sigma, xnew, D.MAXVAR)
        _, st = D.states(c, [], 0)
        Cc, _ = D.constant_of(c, st, [])
        tol = Cc * st[0]["bound_d"]
        with grid.posterior(sigma, rho) as pg, rows.posterior(sigma, rho) as pr:
            vg, vr = pg.var(xnew), pr.var(xnew)
            rg, rr = E.worst_ratio(vg, st[0]["d"], tol), E.worst_ratio(vr, st[0]["d"], tol)
            r12 = float(np.max(np.abs(vg - vr) / (2 * tol)))
            print("posterior: var err/tolerance grid %.3g, rows %.3g, one against the other %.3g; logdet %.17g vs %.17g"
                  % (rg, rr, r12, pg.logdet, pr.logdet))
            assert rg < 1 and rr < 1 and r12 < 1
            assert abs(pg.logdet - pr.logdet) <= 64 * U * p * max(abs(pr.logdet), p)


def test_predict_product_closes_the_loop():
    """fit.predict_product(xa, xb, dims_b) - Y has the RMSE of the row fit's residual, to 1e-10 relative"""
    import outerbase_amd as ob
    p, dims_b, q = 129, (0, 2), 3
    m = sub_model(p)
    xa, xb = blocks(m, SEED[D4], 65, 129, dims_b)
    Y = responses(xa, xb, q, 10)
    fit = ob.fit_newton_product(m["om_d"], m["terms"], xa, xb, Y, dims_b)
    x, Yr = P.expand(xa, xb, dims_b), Y.reshape(-1, q)
    one = ob.fit_newton_multi(m["om_d"], m["terms"], x, Yr)
    rg = np.sqrt(np.mean((fit.predict_product(xa, xb, dims_b) - Y).reshape(-1, q) ** 2, axis=0))
    r1 = np.sqrt(np.mean((one.predict(x) - Yr) ** 2, axis=0))
    print("rmse grid fit %s, row fit %s, relative difference %s" % (rg, r1, np.abs(rg / r1 - 1)))
    assert np.all(np.abs(rg - r1) <= 1e-10 * r1)


# ---- 5. errors -----------------------------------------------------------------------------------
def test_refused_calls_leave_the_state_as_it_was():
    """every refusal of obhip_normal_acc_add_product_dev, argument errors first (OBHIP_ERR_INVALID = 1), then the
    state's (OBHIP_ERR_STATE = 4): the exported state keeps its bits.  (A dims_b that differs between add and
    remove cannot be refused: the accumulator does not remember the split -- include/obhip.h says so.)"""
    import torch
    import outerbase_amd as ob
    from outerbase_amd import _lib
    from conftest import knots_for, make_pair
    p, dims_b, q = 63, (1, 3), 1
    kinds = ["mat25", "mat25pow", "mat25ang", "mat25"]
    om_o, om = make_pair(kinds, knots_for(kinds, 40))      # its own model: the hyper-parameters move below
    terms = om_o.selectterms(p)
    x = sample_x(np.random.default_rng(12), 12, kinds)
    xa, xb = P.split_x(x[:5], dims_b)[0], P.split_x(x[5:], dims_b)[1]
    Y = responses(xa, xb, q, 12)
    add = _lib.lib.obhip_normal_acc_add_product_dev
    u32 = lambda v: np.asarray(v, dtype=np.uint32)
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros(4096, dtype=torch.float64, device=dev)
    a, ok = buf.data_ptr(), u32(dims_b)
    with ob.NewtonAccumulator(om, terms, q) as acc:
        acc.add_product(xa, xb, Y, dims_b)
        before = acc.state()
        h = acc._h
        for db in ([4], [1, 1], [3, 1], [], [0, 1, 2, 3]):
            d = u32(db)
            assert add(h, a, 5, a, 7, d.ctypes.data, d.size, a, 5, 1) == 1
        assert add(h, a, 5, a, 7, None, 2, a, 5, 1) == 1
        assert add(h, None, 5, a, 7, ok.ctypes.data, 2, a, 5, 1) == 1
        assert add(h, a, 5, None, 7, ok.ctypes.data, 2, a, 5, 1) == 1
        assert add(h, a, 5, a, 7, ok.ctypes.data, 2, None, 5, 1) == 1
        assert add(h, a, 5, a, 7, ok.ctypes.data, 2, a, 4, 1) == 1             # lda < na
        assert add(h, a, 0, a, 7, ok.ctypes.data, 2, a, 5, 1) == 1             # no rows
        assert add(h, a, 5, a, 0, ok.ctypes.data, 2, a, 5, 1) == 1
        for sign in (0, 2, -2):
            assert add(h, a, 5, a, 7, ok.ctypes.data, 2, a, 5, sign) == 1
        assert add(h, a, 5, a, 8, ok.ctypes.data, 2, a, 5, -1) == 4            # more rows than the state holds
        assert same_state(before, acc.state())
        # the model's state changed since the first batch: the tie holds for grid batches too
        om.updatehyp(ob.gethyp(om) + 0.1)
        for f in (lambda: acc.add_product(xa, xb, Y, dims_b), lambda: acc.remove_product(xa, xb, Y, dims_b)):
            with pytest.raises(ob.ObhipError, match="changed since") as ei:
                f()
            assert ei.value.code == 4
        assert acc.rows == 35 and same_state(before, acc.state())
