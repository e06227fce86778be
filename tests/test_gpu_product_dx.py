"""The gradient by xb on the product of two input blocks on the GPU (obhip_predict_product_grad_dev,
obhip_product_loglik_grad_dev, MultiFit.calibration_loglik(grad=True), TorchCalibration) against the
extended-precision instrument of tests/product_dx_ref.py, on the fused kernel and -- OBHIP_FORCE_GENERIC -- on the
row route.  Every check prints its figures (test_gpu_extended.Report) before the case asserts."""
import functools

import numpy as np
import pytest

import extended_ref as E
import product_dx_ref as D
from test_gpu_extended import SEED, Report, model
from test_gpu_parity import random_terms
from test_gpu_product import MIXED, ROUTES, SIGMA, big_model, blocks, field_data, fitted, raw_call, route
from test_product_host import coefficients

pytestmark = pytest.mark.gpu

NUMERIC = 5


@functools.lru_cache(maxsize=2)
def reference(name, na, nb, dims_b):
    m = big_model() if name == "big" else model(name)
    seed = 4242 if name == "big" else SEED[name]
    xa, xb = blocks(m, seed, na, nb, dims_b)
    ref = D.ProductDxRef(m, xa, xb, dims_b, seed)
    print("%s | %d x %d, dims_b = %s: oracle err/bound %.3g, C = %.3g" % (name, na, nb, list(dims_b), ref.ratio, ref.C))
    return m, seed, xa, xb, ref


def check_pairs(rep, label, m, ref, theta, cv, xa, xb, dims_b, bits=True):
    import outerbase_amd as ob
    (dm, tdm), (dv, tdv) = ref.pair_grads(theta, cv)
    gm, gv = ob.predict_product_grad(m["om_d"], m["terms"], theta, xa, xb, dims_b, coeffvar=cv, sigma=SIGMA)
    assert gm.shape == gv.shape == (len(xa), len(xb), len(dims_b))
    rep.check(label + " m'", gm, dm, tdm)
    rep.check(label + " v'", gv, dv, tdv)
    only = ob.predict_product_grad(m["om_d"], m["terms"], theta, xa, xb, dims_b, sigma=SIGMA)
    if bits:
        assert np.array_equal(only, gm), label + ": m' without the variance has other bits"
    return gm, gv


@pytest.mark.parametrize("p,dims_b,shape", [(p, db, s) for p, db, s, _ in MIXED[:5]])
def test_pair_gradients_against_extended_reference(p, dims_b, shape, monkeypatch):
    from outerbase_amd import product_grad_layout
    name = "mixed d4 p%d" % p
    m, seed, xa, xb, ref = reference(name, shape[0], shape[1], dims_b)
    assert product_grad_layout(m["om_d"], m["terms"], dims_b)[3], "the case is meant for the fused kernel"
    Theta, cv = coefficients(m, 1, seed)
    rep = Report("%s %s %dx%d" % (name, list(dims_b), shape[0], shape[1]))
    for which in ROUTES:
        route(monkeypatch, which)
        check_pairs(rep, which, m, ref, Theta[:, 0], cv, xa, xb, dims_b)
    rep.done()


def check_sums(rep, label, m, ref, theta, y, ov, cv, xa, xb, dims_b, conditioned=True):
    import outerbase_amd as ob
    chi2, logdet, dchi2, dlogdet = ob.product_loglik_grad(m["om_d"], m["terms"], theta, xa, y, xb, dims_b, obsvar=ov,
                                                          coeffvar=cv, sigma=SIGMA)
    (c2, t2), (lg, tl) = ref.sums(theta, y, ov, cv, SIGMA)
    (dc, tdc), (dl, tdl) = ref.sums_grad(theta, y, ov, cv, SIGMA)
    f = lambda a: np.asarray(a, dtype=np.float64)
    rel2, rell = float(np.max(t2 / np.abs(f(c2)))), float(np.max(tl / np.abs(f(lg))))
    print("%s | %s: tol / |chi2| %.3g, tol / |logdet| %.3g, tol / max|d chi2| %.3g, tol / max|d logdet| %.3g" % (
        rep.case, label, rel2, rell, float(np.max(tdc) / np.max(np.abs(f(dc)))),
        float(np.max(tdl) / max(np.max(np.abs(f(dl))), 1e-300))))
    # the condition on the inputs, as test_gpu_product.check_sums asks it of the two sums
    assert not conditioned or (rel2 <= 1e-6 and rell <= 1e-9)
    rep.check(label + " chi2", chi2, c2, t2)
    rep.check(label + " logdet", logdet, lg, tl)
    rep.check(label + " d chi2", dchi2, dc, tdc)
    rep.check(label + " d logdet", dlogdet, dl, tdl)
    if cv is None:
        assert not np.any(dlogdet), label + ": the noise term alone has no gradient"


def sums_case(name, shape, dims_b, monkeypatch, combos, conditioned=True, routes=ROUTES):
    m, seed, xa, xb, ref = reference(name, shape[0], shape[1], dims_b)
    Theta, cv = coefficients(m, 1, seed)
    theta = Theta[:, 0]
    y, ov = field_data(ref, theta, seed, shape[0])
    rep = Report("sums %s %s %dx%d" % (name, list(dims_b), shape[0], shape[1]))
    for which in routes:
        route(monkeypatch, which)
        for use_cv, use_ov in combos:
            check_sums(rep, "%s coeffvar %d obsvar %d" % (which, use_cv, use_ov), m, ref, theta, y,
                       ov if use_ov else None, cv if use_cv else None, xa, xb, dims_b, conditioned)
    rep.done()


ALL = ((True, True), (True, False), (False, True), (False, False))


@pytest.mark.parametrize("p,shape,dims_b", [(129, (17, 23), (0,)), (129, (65, 64), (1, 3)), (129, (130, 9), (0, 1, 2)),
                                            (700, (17, 23), (1, 3)), (700, (65, 64), (0, 1, 2)), (700, (130, 9), (0,))])
def test_likelihood_gradients_against_extended_reference(p, shape, dims_b, monkeypatch):
    """the shapes of test_gpu_product's likelihood sums, with and without obsvar and coeffvar, conditioned"""
    sums_case("mixed d4 p%d" % p, shape, dims_b, monkeypatch, ALL)


@pytest.mark.parametrize("name,dims_b,shape", [("star mat25x20 p4096", tuple(range(12, 20)), (20, 33)),
                                               ("random d10 W6", (0, 2, 4, 6, 8), (33, 20))])
def test_likelihood_gradients_of_the_wide_splits(name, dims_b, shape, monkeypatch):
    """L = 8 with a view per dimension and three-factor terms; several B factors per term"""
    from outerbase_amd import product_grad_layout
    m = model(name)
    mu_a, mu_b, view_terms, fused = product_grad_layout(m["om_d"], m["terms"], dims_b)
    print("%s: mu_a = %d, mu_b = %d, view_terms / p = %.3f, fused = %d" % (name, mu_a, mu_b, view_terms / len(m["terms"]),
                                                                           fused))
    assert fused
    sums_case(name, shape, dims_b, monkeypatch, ((True, True),), conditioned=False)


def test_term_set_outside_the_fused_domain():
    """test_gpu_product's big split: the entries take the row route by themselves and meet the tolerances"""
    from outerbase_amd import product_grad_layout
    dims_b, na, nb = (10, 11), 65, 9
    m, seed, xa, xb, ref = reference("big", na, nb, dims_b)
    mu_a, mu_b, view_terms, fused = product_grad_layout(m["om_d"], m["terms"], dims_b)
    print("big: mu_a = %d, mu_b = %d, view_terms = %d, fused = %d" % (mu_a, mu_b, view_terms, fused))
    assert not fused
    Theta, cv = coefficients(m, 1, seed)
    rep = Report("outside the fused domain")
    check_pairs(rep, "rows", m, ref, Theta[:, 0], cv, xa, xb, dims_b)
    y, ov = field_data(ref, Theta[:, 0], seed, na)
    check_sums(rep, "rows", m, ref, Theta[:, 0], y, ov, cv, xa, xb, dims_b, conditioned=False)
    rep.done()


def edge_model(which):
    """mixed d4 with term sets of random_terms: "empty view" -- dimension 1 of B = (1, 3) occurs in no term, its
    gradient is rho times the dense part alone; "only B" -- every term has factors on B = (1, 3) only"""
    m = model("mixed d4 p129")
    terms = random_terms(np.random.default_rng(31), 150, 4, 6, 3)
    terms[:, [1] if which == "empty view" else [0, 2]] = 0
    terms = np.unique(terms, axis=0)
    assert len(terms) > 30 and not np.any(terms[0])
    return {k: v for k, v in dict(m, terms=terms, name=which).items() if k != "_product_probe"}


@functools.lru_cache(maxsize=None)
def edge_reference(which):
    m = edge_model(which)
    xa, xb = blocks(m, 77, 65, 33, (1, 3))
    return m, xa, xb, D.ProductDxRef(m, xa, xb, (1, 3), 77)


@pytest.mark.parametrize("which", ["empty view", "only B"])
def test_edge_term_sets(which, monkeypatch):
    from outerbase_amd import product_grad_layout
    m, xa, xb, ref = edge_reference(which)
    terms, dims_b = m["terms"], (1, 3)
    mu_a, mu_b, view_terms, fused = product_grad_layout(m["om_d"], terms, dims_b)
    assert fused and view_terms == int((terms[:, list(dims_b)] > 0).sum())
    assert (which == "empty view" and not np.any(terms[:, 1])) or (which == "only B" and mu_a == 1)
    Theta, cv = coefficients(m, 1, 77)
    theta = Theta[:, 0]
    y, ov = field_data(ref, theta, 77, len(xa))
    rep = Report(which)
    for r in ROUTES:
        route(monkeypatch, r)
        check_pairs(rep, r, m, ref, theta, cv, xa, xb, dims_b)
        check_sums(rep, r, m, ref, theta, y, ov, cv, xa, xb, dims_b, conditioned=False)
    rep.done()


def raw_grad_call(m, theta, xa, xb, dims_b, cv, lda, y=None, ov=None, pad=64, want_rc=0):
    """the C entries on NaN-filled torch buffers with `pad` doubles behind them: (dmean, dvar, out) as the flat
    buffers came back (cv None: no dvar, no variance in the sums)"""
    import torch
    from outerbase_amd import obmod
    from outerbase_amd._lib import ObhipError, call
    dev = torch.device("cuda")
    t = obmod._terms_of(m["om_d"], m["terms"])
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    db = np.asarray(dims_b, dtype=np.uint32)
    na, nb, L = len(xa), len(xb), len(dims_b)
    dxa, dxb, dth, dcv = up(xa.T), up(xb.T), up(theta), up(cv)
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    dmean, dvar, out = nan(L * nb * lda + pad), nan(L * nb * lda + pad), nan((2 + 2 * L) * nb + pad)
    ptr = lambda a: None if a is None else a.data_ptr()
    call("obhip_predict_product_grad_dev", m["om_d"]._h, t._h, dth.data_ptr(), db.ctypes.data, db.size, dxa.data_ptr(), na,
         dxb.data_ptr(), nb, dmean.data_ptr(), lda, ptr(dcv), SIGMA, None if cv is None else dvar.data_ptr())
    if y is not None:
        dy, dov = up(y), up(ov)
        args = ("obhip_product_loglik_grad_dev", m["om_d"]._h, t._h, dth.data_ptr(), db.ctypes.data, db.size,
                dxa.data_ptr(), na, dy.data_ptr(), ptr(dov), dxb.data_ptr(), nb, ptr(dcv), SIGMA, out.data_ptr())
        if want_rc:
            with pytest.raises(ObhipError) as err:
                call(*args)
            assert err.value.code == want_rc
        else:
            call(*args)
    return dmean.cpu().numpy(), dvar.cpu().numpy(), out.cpu().numpy()


def test_bits(monkeypatch):
    """a second call returns the same bits on both routes; columns 0-1 of the likelihood entry are the bits of
    obhip_product_loglik_dev; the mean-only call gives the bits of the m' of the call with the variance"""
    dims_b, na, nb = (0, 1, 2), 130, 17
    m, seed, xa, xb, ref = reference("mixed d4 p700", na, nb, dims_b)
    Theta, cv = coefficients(m, 1, seed)
    theta = Theta[:, 0]
    y, ov = field_data(ref, theta, seed, na)
    for which in ROUTES:
        route(monkeypatch, which)
        first = raw_grad_call(m, theta, xa, xb, dims_b, cv, na, y, ov)
        again = raw_grad_call(m, theta, xa, xb, dims_b, cv, na, y, ov)
        for a, b in zip(first, again):
            assert np.array_equal(a, b, equal_nan=True), which
        assert np.all(np.isfinite(first[2][:8 * nb]))
        values = raw_call(m, Theta, xa, xb, dims_b, cv, na, y, ov)[2]
        assert np.array_equal(first[2][:2 * nb], values[:2 * nb]), which + ": chi2 and logdet have other bits"
        only = raw_grad_call(m, theta, xa, xb, dims_b, None, na)
        assert np.array_equal(only[0], first[0], equal_nan=True), which + ": m' without the variance has other bits"
        assert np.all(np.isnan(only[1]))


def test_masking_and_untouched_memory(monkeypatch):
    """na = 65: the 63 padding rows of the second A tile stay out of every sum -- each equals that of rows 0..63
    plus the one-row call's -- and nothing is written past nb (2 + 2 L), past L nb lda or into the rows na..lda of
    a column; a bad obsvar is refused with OBHIP_ERR_NUMERIC and leaves d_out untouched"""
    na, nb, dims_b, lda, L = 65, 64, (1, 3), 70, 2
    m, seed, xa, xb, ref = reference("mixed d4 p129", na, nb, dims_b)
    Theta, cv = coefficients(m, 1, seed)
    theta = Theta[:, 0]
    y, ov = field_data(ref, theta, seed, na)
    (dm, tdm), (dv, tdv) = ref.pair_grads(theta, cv)
    (c2, t2), (lg, tl) = ref.sums(theta, y, ov, cv, SIGMA)
    (dc, tdc), (dl, tdl) = ref.sums_grad(theta, y, ov, cv, SIGMA)
    want = np.concatenate([np.asarray(c2)[None], np.asarray(lg)[None], np.asarray(dc).T, np.asarray(dl).T]).ravel()
    tol = np.concatenate([t2[None], tl[None], tdc.T, tdl.T]).ravel()
    ncols = 2 + 2 * L
    rep = Report("masking")
    for which in ROUTES:
        route(monkeypatch, which)
        dmean, dvar, out = raw_grad_call(m, theta, xa, xb, dims_b, cv, lda, y, ov)
        assert np.all(np.isnan(dmean[L * nb * lda:])) and np.all(np.isnan(dvar[L * nb * lda:]))
        assert np.all(np.isnan(out[ncols * nb:])) and np.all(np.isfinite(out[:ncols * nb]))
        dmean, dvar = dmean[:L * nb * lda].reshape(L, nb, lda), dvar[:L * nb * lda].reshape(L, nb, lda)
        assert np.all(np.isnan(dmean[:, :, na:])) and np.all(np.isnan(dvar[:, :, na:]))
        rep.check("%s m', lda = %d" % (which, lda), dmean[:, :, :na].transpose(2, 1, 0), dm, tdm)
        rep.check("%s v', lda = %d" % (which, lda), dvar[:, :, :na].transpose(2, 1, 0), dv, tdv)
        head = raw_grad_call(m, theta, xa[:64], xb, dims_b, cv, 64, y[:64], ov[:64])[2][:ncols * nb]
        last = raw_grad_call(m, theta, xa[64:], xb, dims_b, cv, 1, y[64:], ov[64:])[2][:ncols * nb]
        got, parts = out[:ncols * nb], head + last
        rep.check(which + " sums and gradients", got, want, tol)
        rep.check(which + " rows 0..63 + row 64", parts, want, tol + E.U * (np.abs(head) + np.abs(last)))
        # a padding row in a sum would add a term of the size of a real one: far above this
        assert np.max(np.abs(got - parts) - 2 * (tol + E.U * (np.abs(head) + np.abs(last)))) <= 0, which
        bad = ov.copy()
        bad[3] = -1e-300
        assert np.all(np.isnan(raw_grad_call(m, theta, xa, xb, dims_b, cv, lda, y, bad, want_rc=NUMERIC)[2])), which
    rep.done()


def calibration_case():
    """the fit of test_gpu_product.fitted, response 2, calibrated over the two mat25 dimensions (0, 3)"""
    m, fit = fitted()
    dims_t, na, nb, response = (0, 3), 40, 33, 2
    xa, xb = blocks(m, 7, na, nb, dims_t)
    rng = np.random.default_rng(8)
    sca = fit.y_sca[response]
    truth = fit.predict_product(xa, xb[:1], dims_t)[:, 0, response]
    y = truth + 0.05 * sca * rng.standard_normal(na)
    ov = (0.01 * (1.0 + rng.random(na))) * sca * sca
    return m, fit, dims_t, xa, xb, y, ov, response


def test_calibration_loglik_gradient(monkeypatch):
    """.loglik of grad=True equals the grad=False call bit for bit; .grad agrees with the instrument after
    de-standardisation: -(d chi2 + d logdet) / 2 of the standardised data, which the scale leaves unchanged"""
    m, fit, dims_t, xa, xb, y, ov, response = calibration_case()
    ref = D.ProductDxRef(m, xa, xb, dims_t, 7)
    theta, cv = fit.coeff[:, response], 1.0 / fit.diagH
    ys, ovs = (y - fit.y_cent[response]) / fit.y_sca[response], ov / fit.y_sca[response] ** 2
    rep = Report("calibration_loglik(grad=True)")
    for which in ROUTES:
        route(monkeypatch, which)
        for emulator_var in (True, False):
            kw = dict(obs_var=ov, response=response, emulator_var=emulator_var)
            plain = fit.calibration_loglik(xa, y, xb, dims_t, **kw)
            got = fit.calibration_loglik(xa, y, xb, dims_t, grad=True, **kw)
            assert not hasattr(plain, "grad") and got.grad.shape == (len(xb), 2)
            for what in ("loglik", "chi2", "logdet"):
                assert np.array_equal(getattr(got, what), getattr(plain, what)), (which, emulator_var, what)
            (dc, tdc), (dl, tdl) = ref.sums_grad(theta, ys, ovs, cv if emulator_var else None, fit.sigma)
            rep.check("%s emulator_var %d grad" % (which, emulator_var), got.grad, -0.5 * (dc + dl), 0.5 * (tdc + tdl))
    rep.done()


def test_torch_calibration():
    """backward reproduces calibration_loglik's grad exactly for a random cotangent; five LBFGS steps from 33
    starting points: no point's loglik decreases"""
    import torch
    import outerbase_amd as ob
    m, fit, dims_t, xa, xb, y, ov, response = calibration_case()
    want = fit.calibration_loglik(xa, y, xb, dims_t, obs_var=ov, response=response, grad=True)
    cal = ob.TorchCalibration(fit, xa, y, dims_t, obs_var=ov, response=response, emulator_var=True)
    dev = torch.device("cuda")
    t = torch.from_numpy(np.ascontiguousarray(xb)).to(dev).requires_grad_(True)
    ll = cal(t)
    assert ll.shape == (len(xb),)
    err = float(np.max(np.abs(ll.detach().cpu().numpy() - want.loglik) / np.abs(want.loglik)))
    print("TorchCalibration loglik against calibration_loglik: %.3g" % err)
    assert err <= 1e-13      # the same sums; the constant shift is added in another order
    cot = torch.from_numpy(np.random.default_rng(9).standard_normal(len(xb))).to(dev)
    ll.backward(cot)
    assert np.array_equal(t.grad.cpu().numpy(), cot.cpu().numpy()[:, None] * want.grad)
    with pytest.raises(TypeError):
        cal(torch.from_numpy(xb))
    with pytest.raises(ValueError, match="nb x len"):
        cal(t[:, :1])
    # 33 starting points in one loop
    t = torch.from_numpy(np.ascontiguousarray(xb)).to(dev).requires_grad_(True)
    opt = torch.optim.LBFGS([t], lr=0.05, max_iter=4, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = -cal(t).sum()
        loss.backward()
        return loss
    before = cal(t).detach().cpu().numpy()
    for _ in range(5):
        opt.step(closure)
    after = cal(t).detach().cpu().numpy()
    print("LBFGS: sum loglik %.6g -> %.6g, smallest change of a point %.3g" % (before.sum(), after.sum(),
                                                                             float(np.min(after - before))))
    assert np.all(np.isfinite(after)) and np.all(after >= before)
