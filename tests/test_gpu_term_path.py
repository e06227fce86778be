"""The term-count path per entry against the long-double instrument of tests/term_path_ref.py, which factors every
prefix of a real Hessian on its own -- that one factor nests them all is the claim under test.  Through the thin
forms on a Posterior handle (obhip_posterior_path_coef_dev, _theta_dev, _evidence, _scores_dev) on Hessians the test
designs, and once end to end through NewtonAccumulator.term_path.

Every sum is held to  C x (bound propagated from the design matrix's) + rest  (term_path_ref's docstring), C eight
times the float64 LAPACK route's own err / bound on the same case; test_term_path_host.py holds that route to the
same tolerance at every shape used here and stages the failures these shapes must be able to see.  Each check prints
one line: C and err / tolerance of the device and of the float64 route.

The shapes: p at one column tile of 32 and around it (1, 15, 16, 17), around the 128 of the stored product's tiles
(127, 128, 129) and four of them (385); n at one row tile, its edges and three tiles (1, 127, 128, 129, 300); step
1, 7 (checkpoints inside and across column tiles), 129 and 1000 (the one checkpoint k = p); q within one register
block of 4 and beyond it (3, 6).  These calls are the first to run the stored fixed-order product with the
triangular cut (launch_atb, kAtbStoreFixed, tri)."""
import functools
import math

import numpy as np
import pytest

import extended_ref as E
import posterior_ref as P
import term_path_ref as T
from conftest import knots_for, make_pair
from extended_ref import gamma

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_model(short):
    """the device model on the oracle's rotation: short length scales for the dyadic cases, the defaults for the
    real Hessians -- the same model term_path_ref's cases were made on"""
    om_o, om_d = make_pair(P.KINDS, knots_for(P.KINDS, P.NKNOTS), hyp=P.HYP_SHORT if short else None)
    want = T.short_model() if short else P.oracle_model()
    assert np.array_equal(om_o.rotmat, want.rotmat) and np.array_equal(om_d.rotation()[0], want.rotmat)
    return om_d


def posterior_of(c, short):
    import outerbase_amd as ob
    return ob.Posterior.from_hessian(device_model(short), c["terms"], c["H"], c["sigma"])


def run_case(c, short, chunk_rows=0, Y=None, meansd=None):
    with posterior_of(c, short) as post:
        U = post.term_path_coef(c["G"])
        return post.term_path_scores(U, c["x"], c["Y"] if Y is None else Y, step=c["step"], loo=c["loo"],
                                     chunk_rows=chunk_rows, meansd=meansd)


def check_scores(label, got, c):
    scores, sumv = got
    K = len(c["ref"]["ks"])
    assert scores.shape == (K, c["q"], 3) and sumv.shape == (K,)
    assert np.all(np.isfinite(scores)) and np.all(np.isfinite(sumv)), label
    dev = T.score_ratios(scores, sumv, c)
    host = T.score_ratios(c["h64"]["scores"], c["h64"]["sumv"], c)
    fmt = lambda r: " ".join("%s %.3g" % kv for kv in r.items())
    print("term path | %s: K %d, C %.3g; device err/tol %s; float64 route err/tol %s" % (label, K, c["C"], fmt(dev), fmt(host)))
    assert max(dev.values()) <= 1.0, (label, dev)
    if not c["loo"]:
        assert np.array_equal(scores[:, :, 0], scores[:, :, 1])         # hold-out: e = r


# ---- hold-out mode on the dyadic Hessian, sigma = 0 --------------------------------------------------------------
@pytest.mark.parametrize("p,n,step", T.HOLD_CASES)
def test_hold_out_scores_on_the_dyadic_hessian(p, n, step):
    c = T.hold_case(p, n, step)
    check_scores("hold-out p=%d n=%d step=%d" % (p, n, step), run_case(c, True), c)


@pytest.mark.parametrize("q", T.HOLD_Q)
def test_hold_out_scores_of_several_responses(q):
    """q = 3: one pass with an unfilled register block; q = 6: two passes over the same stored Z, the second
    unfilled, sumv written by the first alone"""
    c = T.hold_case(129, 130, 16, q)
    check_scores("hold-out p=129 n=130 step=16 q=%d" % q, run_case(c, True), c)


# ---- leave-one-out mode on a Hessian formed from 1500 data rows ----------------------------------------------------
@pytest.mark.parametrize("p,step", T.LOO_CASES)
@pytest.mark.parametrize("q", T.LOO_Q)
def test_leave_one_out_scores_on_the_data_hessian(p, step, q):
    c = T.loo_case(p, step, q)
    assert c["ref"]["hmax"] <= 0.9
    check_scores("loo p=%d step=%d q=%d n=300" % (p, step, q), run_case(c, False), c)


def test_chunked_repeated_and_standardised_on_the_device():
    """n = 300, p = 385, leave-one-out, q = 3: chunk_rows = 128 (three chunks, one tile each, the group sums carried
    from chunk to chunk) against 0 (one chunk) bit for bit; the same call twice bit for bit; and raw responses with
    d_meansd against the same responses standardised on the host by the same two operations, bit for bit."""
    c = T.loo_case(385, 64, 3)
    whole = run_case(c, False)
    check_scores("loo p=385 n=300, one chunk", whole, c)
    for label, other in (("chunk_rows=128", run_case(c, False, chunk_rows=128)), ("again", run_case(c, False)),
                         ("chunk_rows=256", run_case(c, False, chunk_rows=256))):
        assert np.array_equal(whole[0], other[0]) and np.array_equal(whole[1], other[1]), label
    meansd = np.array([[10.0, 3.0, 1500.0], [-2.5, 0.7, 1500.0], [0.0, 4.0, 1500.0]])
    raw = c["Y"] * meansd[None, :, 1] + meansd[None, :, 0]
    std = (raw - meansd[None, :, 0]) / meansd[None, :, 1]
    a, b = run_case(c, False, Y=raw, meansd=meansd), run_case(c, False, Y=std)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[1], whole[1])                               # sumv does not see the responses


def test_no_rows_give_zeros():
    c = T.hold_case(17, 130, 16)
    with posterior_of(c, True) as post:
        U = post.term_path_coef(c["G"])
        scores, sumv = post.term_path_scores(U, np.zeros((0, 4)), np.zeros((0, 1)), step=16)
    assert scores.shape == (2, 1, 3) and not np.any(scores) and not np.any(sumv)


# ---- the coefficients ---------------------------------------------------------------------------------------------
def test_path_coefficients_against_the_reference():
    """U = L^-1 G and Theta_k at k in (1, 64, 65, p), p = 385, q = 3 on the data Hessian: the reference factors
    H[:k,:k] on its own for every k; zeros behind row k"""
    c = T.real(385)
    ks = (1, 64, 65, 385)
    u, ru, thetas = T.ref_coef(c["H"], None, False, c["G"], 64, ks_theta=ks, backward=True)
    with posterior_of(c, False) as post:
        U = post.term_path_coef(c["G"])
        r = E.worst_ratio(U, u, ru)
        print("term path | U p=385 q=3: err/rest %.3g, max-norm %.3g" % (r, E.maxnorm_relerr(U, u)))
        assert np.all(np.isfinite(U)) and r <= 1.0
        for k in ks:
            th = post.term_path_theta(U, k)
            r = E.worst_ratio(th, thetas[k][0], thetas[k][1])
            print("term path | Theta_k k=%d: err/rest %.3g, max-norm %.3g" % (k, r, E.maxnorm_relerr(th, thetas[k][0])))
            assert np.all(np.isfinite(th)) and r <= 1.0 and not np.any(th[k:])
        one = post.term_path_coef(c["G"][:, 0])                         # a response alone: its column's bits
        assert np.array_equal(one[:, 0], U[:, 0])


def _theta_route_tolerance(Bo, Ystd, k, sigma, rho, om, terms):
    """what one float64 route may miss theta_k = inv(H_k) g_k by, per entry, to first order: the backward error of its
    Cholesky factorisation and substitutions, |dH| <= gamma(3 k + 1) |L| |L|^T, and the rounding of the entries of
    H_k and g_k themselves, sums over the n rows in any order: gamma(n + 4) e^{-2 sigma} (|B|^T |B| |theta| + |B|^T |y|)
    (the prior precisions to 8 u); all through |inv(H_k)|"""
    import ob_oracle as O
    n = Bo.shape[0]
    e2 = math.exp(-2 * sigma)
    Bk = Bo[:, :k]
    prec = O.prior_prec(om, terms[:k], rho)
    H = e2 * (Bk.T @ Bk) + np.diag(prec)
    g = e2 * (Bk.T @ Ystd)
    L = np.linalg.cholesky(H)
    theta = np.linalg.solve(H, g)
    aHi, aL, aB = np.abs(np.linalg.inv(H)), np.abs(L), np.abs(Bk)
    moved = gamma(3 * k + 1) * ((aL @ aL.T) @ np.abs(theta)) \
        + gamma(n + 4) * e2 * (aB.T @ (aB @ np.abs(theta)) + aB.T @ np.abs(Ystd)) + 8 * E.U * prec[:, None] * np.abs(theta)
    return theta, aHi @ moved


def _check_path_evidence(got, om, terms, Bo, Ystd, sigma, rho, step):
    """NewtonAccumulator.term_path's log_evidence -- the glue: prec from getvar and rho, yty = rows - 1, n_rows -- against
    the long-double reference on the float64 host Hessian H = e^{-2 sigma} B^T B + diag(prec) and G = e^{-2 sigma} B^T
    y_std, every prefix factored on its own.  The device forms its own H and G from the same rows, sums over n rows in
    another order: |dH| <= gamma(n + 4) e^{-2 sigma} |B|^T |B| + 8 u diag(prec), |dG| <= gamma(n + 4) e^{-2 sigma} |B|^T
    |y| (which also covers the few u of its own centre and scale), and to first order the evidence moves by
    1/2 tr(inv(H_k) dH) + 1/2 theta^T dH theta + theta^T dG; that is added to the reference's rest."""
    import ob_oracle as O
    n, q = Ystd.shape
    e2 = math.exp(-2 * sigma)
    prec = O.prior_prec(om, terms, rho)
    H = e2 * (Bo.T @ Bo) + np.diag(prec)
    H = 0.5 * (H + H.T)
    G = e2 * (Bo.T @ Ystd)
    yty = np.full(q, n - 1.0)
    want, rest = T.ref_evidence(H, None, False, G, prec, yty, n, sigma, step, backward=True)
    aB = np.abs(Bo)
    for c, k in enumerate(T.checkpoints(len(prec), step)):
        Hinv = np.linalg.inv(H[:k, :k])
        ath = np.abs(Hinv @ G[:k])
        dH = gamma(n + 4) * e2 * (aB[:, :k].T @ aB[:, :k]) + 8 * E.U * np.diag(prec[:k])
        dG = gamma(n + 4) * e2 * (aB[:, :k].T @ np.abs(Ystd))
        rest[c] += 0.5 * np.sum(np.abs(Hinv) * dH) + 0.5 * np.einsum("iq,ij,jq->q", ath, dH, ath) + (ath * dG).sum(axis=0)
    r = E.worst_ratio(got, want, rest)
    r64 = E.worst_ratio(T.host_evidence64(H, G, prec, yty, n, sigma, step), want, rest)
    print("term path | log_evidence through NewtonAccumulator.term_path, p=%d n=%d step=%d: err/rest %.3g (float64 route "
          "%.3g), max-norm %.3g" % (len(prec), n, step, r, r64, E.maxnorm_relerr(got, want)))
    assert got.shape == want.shape and np.all(np.isfinite(got)) and r <= 1.0


def test_refusals_on_a_live_handle_change_nothing():
    """what the entries refuse on a handle that lives, each OBHIP_ERR_INVALID before any launch: the outputs keep their
    sentinel, and the same valid call gives the same bits before and after"""
    import torch
    from outerbase_amd._lib import lib
    c = T.hold_case(17, 130, 16)
    p, n = 17, 130
    with posterior_of(c, True) as post:
        U = post.term_path_coef(c["G"])
        before = post.term_path_scores(U, c["x"], c["Y"], step=16)
        dev = torch.device("cuda", torch.cuda.current_device())
        f64 = torch.float64
        dU = torch.from_numpy(np.ascontiguousarray(U.T)).to(dev)
        dx = torch.from_numpy(np.ascontiguousarray(c["x"].T)).to(dev)
        dY = torch.from_numpy(np.ascontiguousarray(c["Y"].T)).to(dev)
        sc = torch.full((2, 1, 3), -7.0, dtype=f64, device=dev)
        sv = torch.full((2,), -7.0, dtype=f64, device=dev)
        th = torch.full((1, p), -7.0, dtype=f64, device=dev)
        ev = np.full((2, 1), -7.0)
        prec, yty = np.ones(p), np.ones(1)
        h, u, x, y = post._h, dU.data_ptr(), dx.data_ptr(), dY.data_ptr()
        S = lambda **kw: [kw.get(a, b) for a, b in (("h", h), ("u", u), ("q", 1), ("x", x), ("n", n), ("y", y), ("ldy", n),
                                                   ("ms", None), ("step", 16), ("loo", 0), ("chunk", 0),
                                                   ("sc", sc.data_ptr()), ("sv", sv.data_ptr()))]
        refused = [
            ("scores step=0", "obhip_posterior_path_scores_dev", S(step=0)),
            ("scores q=0", "obhip_posterior_path_scores_dev", S(q=0)),
            ("scores q=65535", "obhip_posterior_path_scores_dev", S(q=65535)),
            ("scores chunk_rows=100", "obhip_posterior_path_scores_dev", S(chunk=100)),
            ("scores chunk_rows=129", "obhip_posterior_path_scores_dev", S(chunk=129)),
            ("scores ldy<n", "obhip_posterior_path_scores_dev", S(ldy=n - 1)),
            ("scores loo=2", "obhip_posterior_path_scores_dev", S(loo=2)),
            ("scores x=NULL", "obhip_posterior_path_scores_dev", S(x=None)),
            ("scores Y=NULL", "obhip_posterior_path_scores_dev", S(y=None)),
            ("scores U=NULL", "obhip_posterior_path_scores_dev", S(u=None)),
            ("scores sumv=NULL", "obhip_posterior_path_scores_dev", S(sv=None)),
            ("theta k=0", "obhip_posterior_path_theta_dev", [h, u, 1, 0, th.data_ptr()]),
            ("theta k=p+1", "obhip_posterior_path_theta_dev", [h, u, 1, p + 1, th.data_ptr()]),
            ("theta q=0", "obhip_posterior_path_theta_dev", [h, u, 0, 1, th.data_ptr()]),
            ("theta U=NULL", "obhip_posterior_path_theta_dev", [h, None, 1, 1, th.data_ptr()]),
            ("coef q=0", "obhip_posterior_path_coef_dev", [h, u, 0, th.data_ptr()]),
            ("coef G=NULL", "obhip_posterior_path_coef_dev", [h, None, 1, th.data_ptr()]),
            ("evidence step=0", "obhip_posterior_path_evidence", [h, u, 1, prec.ctypes.data, yty.ctypes.data, n, 0, ev.ctypes.data]),
            ("evidence q=0", "obhip_posterior_path_evidence", [h, u, 0, prec.ctypes.data, yty.ctypes.data, n, 16, ev.ctypes.data]),
            ("evidence prec=NULL", "obhip_posterior_path_evidence", [h, u, 1, None, yty.ctypes.data, n, 16, ev.ctypes.data]),
            ("diag out=NULL", "obhip_posterior_hessian_diag_dev", [h, None]),
        ]
        for label, name, args in refused:
            assert getattr(lib, name)(*args) == 1, label                  # OBHIP_ERR_INVALID
            assert lib.obhip_last_error(), label
        torch.cuda.synchronize()
        for out in (sc, sv, th):
            assert bool(torch.all(out == -7.0))
        assert np.all(ev == -7.0)
        after = post.term_path_scores(U, c["x"], c["Y"], step=16)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert np.array_equal(post.term_path_coef(c["G"]), U)
        diag = torch.empty(p, dtype=f64, device=dev)
        assert lib.obhip_posterior_hessian_diag_dev(h, diag.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(diag.cpu().numpy(), np.diagonal(c["H"]))


def test_path_theta_against_the_streaming_fit_of_the_prefix():
    """p = 129, n = 300 rows, q = 2, sigma = log 0.1: TermPathResult.fit(k) (obhip_posterior_path_theta_dev on the
    factor of all 129 terms) against NewtonAccumulator(terms[:k]).fit on the same rows (obhip_normal_acc_solve_dev:
    its own Gram, its own factor) at k in (1, 64, 65, 129), each route allowed its own first-order error"""
    import ob_oracle as O
    import outerbase_amd as ob
    om_o, om_d = P.oracle_model(), device_model(False)
    p, n, q, sigma, rho = 129, 300, 2, math.log(0.1), 6.0
    terms = np.asarray(om_o.selectterms(p), dtype=np.int64)
    x = P.inside_rows(n, 31)
    rng = np.random.default_rng(8)
    Y = 10.0 + 3.0 * np.stack([np.sin(x.sum(axis=1)), np.cos(2 * x[:, 0]) + 0.1 * rng.standard_normal(n)], axis=1)
    Bo = O.ob_getmat(O.OuterBase(om_o, x), terms)
    Ystd = (Y - Y.mean(axis=0)) / Y.std(axis=0, ddof=1)
    with ob.NewtonAccumulator(om_d, terms, q) as acc:
        acc.add(x, Y)
        with acc.term_path(sigma=sigma, rho=rho, step=16) as path:
            assert list(path.sizes) == T.checkpoints(p, 16) and path.log_evidence.shape == (9, q)
            assert path.sse is None and path.dof is None
            _check_path_evidence(path.log_evidence, om_o, terms, Bo, Ystd, sigma, rho, 16)
            for k in (1, 64, 65, p):
                got = path.fit(k)
                with ob.NewtonAccumulator(om_d, terms[:k], q) as acck:
                    want = acck.add(x, Y).fit(sigma=sigma, rho=rho)
                theta64, tol = _theta_route_tolerance(Bo, Ystd, k, sigma, rho, om_o, terms)
                assert got.coeff.shape == want.coeff.shape == (k, q)
                r = float(np.max(np.abs(got.coeff - want.coeff) / (2 * tol)))
                r64 = float(np.max(np.abs(got.coeff - theta64) / (2 * tol)))
                print("term path | fit(%d) against the streaming fit of terms[:%d]: |difference| / (both tolerances) %.3g "
                      "(against the float64 host solve %.3g), max-norm %.3g"
                      % (k, k, r, r64, E.maxnorm_relerr(got.coeff, want.coeff)))
                assert r <= 1.0 and r64 <= 1.0
                assert np.array_equal(got.diagH, want.diagH) and np.array_equal(got.y_cent, want.y_cent)
                assert np.array_equal(got.y_sca, want.y_sca)


# ---- the evidence -------------------------------------------------------------------------------------------------
def test_evidence_at_every_checkpoint():
    """obhip_posterior_path_evidence on the data Hessian, p = 385, step 64, q = 3, 1500 rows (every prefix factored
    on its own by the reference), and on the dyadic one, p = 129, step 7, where checkpoints fall inside tiles"""
    c = T.real(385)
    prec = np.exp(-np.linspace(0.0, 9.0, 385))
    yty = np.array([1499.0, 1499.0, 1499.0])
    want, rest = T.ref_evidence(c["H"], None, False, c["G"], prec, yty, 1500, c["sigma"], 64, backward=True)
    with posterior_of(c, False) as post:
        got = post.term_path_evidence(post.term_path_coef(c["G"]), prec, yty, 1500, step=64)
    r = E.worst_ratio(got, want, rest)
    r64 = E.worst_ratio(T.host_evidence64(c["H"], c["G"], prec, yty, 1500, c["sigma"], 64), want, rest)
    print("term path | evidence data H p=385 step=64: device err/rest %.3g, float64 route %.3g, max-norm %.3g"
          % (r, r64, E.maxnorm_relerr(got, want)))
    assert got.shape == (7, 3) and np.all(np.isfinite(got)) and r <= 1.0
    d = T.hold_case(129, 130, 7)
    prec = np.exp(-np.linspace(0.0, 5.0, 129))
    yty = np.array([129.0])
    want, rest = T.ref_evidence(d["H"], T.dyadic(129)["L"], True, d["G"], prec, yty, 130, 0.0, 7)
    with posterior_of(d, True) as post:
        got = post.term_path_evidence(post.term_path_coef(d["G"]), prec, yty, 130, step=7)
    r = E.worst_ratio(got, want, rest)
    print("term path | evidence dyadic H p=129 step=7: device err/rest %.3g, max-norm %.3g" % (r, E.maxnorm_relerr(got, want)))
    assert got.shape == (19, 1) and r <= 1.0


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_term_path_end_to_end():
    """NewtonAccumulator.term_path on 300 rows, scored on 200 others: .best("lpd") is a checkpoint, .fit(best)
    predicts what fit_newton_multi on terms[:best] predicts within the two routes' tolerances, and the path's sse at
    that size is the sum of squares of that fit's residuals on the hold-out rows, to what those tolerances move it"""
    import ob_oracle as O
    import outerbase_amd as ob
    om_o, om_d = P.oracle_model(), device_model(False)
    p, n, nh, q, sigma, rho = 129, 300, 200, 2, math.log(0.1), 6.0
    terms = np.asarray(om_o.selectterms(p), dtype=np.int64)
    xall = P.inside_rows(n + nh, 41)
    rng = np.random.default_rng(9)
    Yall = 10.0 + 3.0 * np.stack([np.sin(xall.sum(axis=1)), np.cos(2 * xall[:, 0])], axis=1) \
        + 0.3 * rng.standard_normal((n + nh, q))
    x, Y, xh, Yh = xall[:n], Yall[:n], xall[n:], Yall[n:]
    with ob.NewtonAccumulator(om_d, terms, q) as acc:
        acc.add(x, Y)
        with acc.term_path(sigma=sigma, rho=rho, step=16, x=xh, Y=Yh) as path, \
                acc.term_path(sigma=sigma, rho=rho, step=16, x=x, Y=Y, loo=True) as loo:
            assert path.sse.shape == path.lpd.shape == path.rmse.shape == path.log_evidence.shape == (9, q)
            assert np.array_equal(path.sse, path.spe) and path.dof is None
            assert np.array_equal(path.log_evidence, loo.log_evidence)
            assert np.all(loo.spe >= loo.sse) and np.all(np.diff(loo.dof) > 0) and 0 < loo.dof[0] < loo.dof[-1] < p
            best = path.best("lpd")
            assert best in list(path.sizes) and path.best("spe", response=0) in list(path.sizes)
            fit = path.fit(best)
        direct = ob.fit_newton_multi(om_d, terms[:best], x, Y, sigma=sigma, rho=rho)
    Ystd = (Y - Y.mean(axis=0)) / Y.std(axis=0, ddof=1)
    _, tol = _theta_route_tolerance(O.ob_getmat(O.OuterBase(om_o, x), terms), Ystd, best, sigma, rho, om_o, terms)
    Bh = O.ob_getmat(O.OuterBase(om_o, xh), terms[:best])
    sd = Y.std(axis=0, ddof=1)
    # a prediction moves by |b|^T (what theta may move by) sd, and by the predictor's own gamma(k + d + 8) |b|^T |theta| sd
    tolpred = (np.abs(Bh) @ (tol + gamma(best + 12) * np.abs(direct.coeff))) * sd[None, :] \
        + 8 * E.U * np.abs(Yh)
    got, want = fit.predict(xh), direct.predict(xh)
    r = float(np.max(np.abs(got - want) / (2 * tolpred)))
    c = list(path.sizes).index(best)
    res = Yh - want
    sse_tol = (2 * np.abs(res) * 2 * tolpred).sum(axis=0) + gamma(nh + 8) * (res * res).sum(axis=0)
    rs = float(np.max(np.abs(path.sse[c] - (res * res).sum(axis=0)) / sse_tol))
    print("term path | end to end: best by lpd %d of %s; fit(best).predict against fit_newton_multi(terms[:best]) "
          "|difference| / (both tolerances) %.3g; path sse against that fit's residuals %.3g"
          % (best, [int(k) for k in path.sizes], r, rs))
    assert r <= 1.0 and rs <= 1.0
