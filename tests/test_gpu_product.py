"""The predictor on the product of two input blocks on the GPU (obhip_predict_product_dev,
obhip_product_loglik_dev, MultiFit.predict_product / calibration_loglik) against the extended-precision
reference of tests/product_ref.py, per entry, on the fused kernel and -- OBHIP_FORCE_GENERIC -- on the row
route.  Every check prints its figures (test_gpu_extended.Report) before the case asserts."""
import functools
import math

import numpy as np
import pytest

import extended_ref as E
import product_ref as P
from conftest import knots_for, make_pair, sample_x
from test_gpu_extended import SEED, Report, model
from test_gpu_parity import random_terms
from test_product_host import coefficients

pytestmark = pytest.mark.gpu

SIGMA = math.log(0.01)
ROUTES = ("fused", "rows")


def route(monkeypatch, which):
    if which == "rows":
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


def blocks(m, seed, na, nb, dims_b):
    rng = np.random.default_rng(seed + 31 * na + nb)
    xa = P.split_x(sample_x(rng, na, m["kinds"]), dims_b)[0]
    xb = P.split_x(sample_x(rng, nb, m["kinds"]), dims_b)[1]
    return xa, xb


@functools.lru_cache(maxsize=2)
def reference(name, na, nb, dims_b):
    m = big_model() if name == "big" else model(name)
    seed = 4242 if name == "big" else SEED[name]
    xa, xb = blocks(m, seed, na, nb, dims_b)
    ref = P.ProductRef(m, xa, xb, dims_b, seed)
    print("%s | %d x %d, dims_b = %s: oracle err/bound %.3g, C = %.3g" % (name, na, nb, list(dims_b), ref.ratio, ref.C))
    return m, seed, xa, xb, ref


@functools.lru_cache(maxsize=None)
def big_model():
    """d = 12, levels up to 39 on 40 knots: ten dimensions on side A use more basis columns than the fused
    kernel's LDS holds (320 x 64 doubles are the whole budget)"""
    import outerbase_amd as ob
    kinds = ["mat25", "mat25pow", "mat25", "mat25"] * 3
    knots = knots_for(kinds, 40)
    om_o, om_d = make_pair(kinds, knots, share_rotation=True)
    rot, bv, ml = om_d.rotation()
    terms = np.unique(random_terms(np.random.default_rng(77), 900, 12, 39, 3), axis=0)
    return dict(name="big", kinds=kinds, knots=[np.asarray(k, dtype=np.float64) for k in knots], om_o=om_o, om_d=om_d,
                hyp=ob.gethyp(om_d), rot=rot, terms=terms)


def check_mean_var(rep, label, m, ref, Theta, cv, xa, xb, dims_b):
    import outerbase_amd as ob
    mean, var = ob.predict_product(m["om_d"], m["terms"], Theta, xa, xb, dims_b, coeffvar=cv, sigma=SIGMA)
    assert mean.shape == (len(xa), len(xb), Theta.shape[1]) and var.shape == (len(xa), len(xb))
    for r in range(Theta.shape[1]):
        want, tol = ref.mean(Theta[:, r])
        rep.check("%s mean, response %d" % (label, r), mean[:, :, r], want, tol)
    want, tol = ref.var(cv, SIGMA)
    rep.check(label + " variance", var, want, tol)
    only = ob.predict_product(m["om_d"], m["terms"], Theta, xa, xb, dims_b, sigma=SIGMA)
    assert np.array_equal(only, mean), label + ": the mean without the variance has other bits"


MIXED = [  # p, dims_b, (na, nb), q: every value of every column of the issue's table occurs
    (1, (0,), (1, 1), 1),
    (127, (3,), (63, 65), 3),
    (129, (1, 3), (64, 64), 17),
    (700, (0, 1, 2), (130, 17), 1),
    (700, (1, 3), (17, 130), 3),
    (129, (0,), (130, 17), 17),
]
OTHERS = [
    ("star mat25x20 p4096", tuple(range(12, 20)), (20, 33), 1),
    ("star mat25x20 p4096", (0, 5, 10, 15), (20, 33), 1),
    ("random d10 W6", (0, 2, 4, 6, 8), (33, 20), 1),
]


@pytest.mark.parametrize("name,dims_b,shape,q", [("mixed d4 p%d" % p, db, s, q) for p, db, s, q in MIXED] + OTHERS)
def test_mean_and_variance_against_extended_reference(name, dims_b, shape, q, monkeypatch):
    from outerbase_amd import product_layout
    m, seed, xa, xb, ref = reference(name, shape[0], shape[1], dims_b)
    assert product_layout(m["om_d"], m["terms"], dims_b)[2], "the case is meant for the fused kernel"
    Theta, cv = coefficients(m, q, seed)
    rep = Report("%s %s %dx%d q=%d" % (name, list(dims_b), shape[0], shape[1], q))
    for which in ROUTES:
        route(monkeypatch, which)
        check_mean_var(rep, which, m, ref, Theta, cv, xa, xb, dims_b)
    rep.done()


def field_data(ref, theta, seed, na):
    """y = the reference mean of candidate 0 + 0.05 N(0, 1), obsvar = 0.01 (1 + U(0, 1))"""
    rng = np.random.default_rng(seed + 5)
    y = np.asarray(ref.mean(theta)[0][:, 0], dtype=np.float64) + 0.05 * rng.standard_normal(na)
    return y, 0.01 * (1.0 + rng.random(na))


def check_sums(rep, label, m, ref, theta, y, ov, cv, xa, xb, dims_b, conditioned=True):
    import outerbase_amd as ob
    chi2, logdet = ob.product_loglik(m["om_d"], m["terms"], theta, xa, y, xb, dims_b, obsvar=ov, coeffvar=cv, sigma=SIGMA)
    (c2, t2), (lg, tl) = ref.sums(theta, y, ov, cv, SIGMA)
    # the condition on the inputs: a tolerance that is a visible fraction of the sums would hide errors
    rel2 = float(np.max(t2 / np.abs(np.asarray(c2, dtype=np.float64))))
    rell = float(np.max(tl / np.abs(np.asarray(lg, dtype=np.float64))))
    print("%s | %s: tol / |chi2| %.3g, tol / |logdet| %.3g" % (rep.case, label, rel2, rell))
    assert not conditioned or (rel2 <= 1e-6 and rell <= 1e-9)
    rep.check(label + " chi2", chi2, c2, t2)
    rep.check(label + " logdet", logdet, lg, tl)
    return chi2, logdet


@pytest.mark.parametrize("p,shape,dims_b", [(129, (17, 23), (0,)), (129, (65, 64), (1, 3)), (129, (130, 9), (0, 1, 2)),
                                            (700, (17, 23), (1, 3)), (700, (65, 64), (0, 1, 2)), (700, (130, 9), (0,))])
def test_likelihood_sums_against_extended_reference(p, shape, dims_b, monkeypatch):
    m, seed, xa, xb, ref = reference("mixed d4 p%d" % p, shape[0], shape[1], dims_b)
    Theta, cv = coefficients(m, 1, seed)
    theta = Theta[:, 0]
    y, ov = field_data(ref, theta, seed, shape[0])
    rep = Report("sums p=%d %s %dx%d" % (p, list(dims_b), shape[0], shape[1]))
    for which in ROUTES:
        route(monkeypatch, which)
        for use_cv in (True, False):
            for use_ov in (True, False):
                check_sums(rep, "%s coeffvar %d obsvar %d" % (which, use_cv, use_ov), m, ref, theta, y,
                           ov if use_ov else None, cv if use_cv else None, xa, xb, dims_b)
    rep.done()


def test_term_set_outside_the_fused_domain():
    """side A alone needs more LDS than the kernel has: the entry takes the row route by itself.  The term set
    reaches level 39 of 40 knots, whose propagated bounds are larger than those of the conditioned cases above:
    the tolerance of chi2 comes to 2.2e-6 of it here (printed, not asserted; the device uses 0.3 % of it)."""
    from outerbase_amd import product_layout
    dims_b, na, nb = (10, 11), 65, 9
    m, seed, xa, xb, ref = reference("big", na, nb, dims_b)
    mu_a, mu_b, fused = product_layout(m["om_d"], m["terms"], dims_b)
    print("big: mu_a = %d, mu_b = %d, fused = %d" % (mu_a, mu_b, fused))
    assert mu_a * 64 * 8 > 160 * 1024 and not fused
    Theta, cv = coefficients(m, 2, seed)
    rep = Report("outside the fused domain")
    check_mean_var(rep, "rows", m, ref, Theta, cv, xa, xb, dims_b)
    y, ov = field_data(ref, Theta[:, 0], seed, na)
    check_sums(rep, "rows", m, ref, Theta[:, 0], y, ov, cv, xa, xb, dims_b, conditioned=False)
    rep.done()


@functools.lru_cache(maxsize=None)
def fitted():
    import outerbase_amd as ob
    m = model("mixed d4 p700")
    rng = np.random.default_rng(99)
    x = sample_x(rng, 1500, m["kinds"])
    f = np.sin(3 * x[:, 0]) * x[:, 1] + np.cos(x[:, 2]) + x[:, 3] ** 2
    Y = np.stack([f, 2.0 + 10.0 * f * x[:, 3], -5.0 + 0.1 * np.exp(x[:, 0])], axis=1) + 0.01 * rng.standard_normal((1500, 3))
    return m, ob.fit_newton_multi(m["om_d"], m["terms"], x, Y)


def test_device_against_device():
    """MultiFit.predict_product against MultiFit.predict on the expanded rows (1e-11 max-norm relative, the
    project's device-against-device figure) and calibration_loglik against the same sums formed in NumPy from
    MultiFit.predict(..., var=True) (1e-9 relative)"""
    m, fit = fitted()
    dims_b, na, nb = (1, 3), 200, 300
    xa, xb = blocks(m, 7, na, nb, dims_b)
    mean, var = fit.predict_product(xa, xb, dims_b, var=True)
    wm, wv = fit.predict(P.expand(xa, xb, dims_b), var=True)
    wm, wv = wm.reshape(na, nb, 3), wv.reshape(na, nb, 3)
    em = float(np.max(np.abs(mean - wm)) / np.max(np.abs(wm)))
    ev = float(np.max(np.abs(var - wv)) / np.max(np.abs(wv)))
    print("predict_product against predict: mean %.3g, variance %.3g" % (em, ev))
    assert np.array_equal(fit.predict_product(xa, xb, dims_b), mean)
    rng = np.random.default_rng(8)
    worst = 0.0
    for response in (0, 2):
        sca = fit.y_sca[response]
        y = wm[:, 0, response] + 0.05 * sca * rng.standard_normal(na)
        ov = (0.01 * (1.0 + rng.random(na))) * sca * sca
        for emulator_var in (True, False):
            got = fit.calibration_loglik(xa, y, xb, dims_b, obs_var=ov, response=response, emulator_var=emulator_var)
            v = (wv[:, :, response] if emulator_var else math.exp(2 * fit.sigma) * sca * sca) + ov[:, None]
            r = y[:, None] - wm[:, :, response]
            chi2, logdet = (r * r / v).sum(0), (np.log(v) * np.ones((na, nb))).sum(0)
            lik = -0.5 * (chi2 + logdet) - 0.5 * na * math.log(2 * math.pi)
            for what, g, w in (("chi2", got.chi2, chi2), ("logdet", got.logdet, logdet), ("loglik", got.loglik, lik)):
                e = float(np.max(np.abs(g - w) / np.abs(w)))
                print("calibration_loglik response %d emulator_var %d: %s %.3g" % (response, emulator_var, what, e))
                worst = max(worst, e)
    assert em <= 1e-11 and ev <= 1e-11
    assert worst <= 1e-9


def raw_call(m, Theta, xa, xb, dims_b, cv, lda, y=None, ov=None, pad=64):
    """the C entries on NaN-filled torch buffers with `pad` doubles behind them: (mean, var, sums) as the
    flat buffers came back"""
    import torch
    from outerbase_amd import obmod
    from outerbase_amd._lib import call
    dev = torch.device("cuda")
    t = obmod._terms_of(m["om_d"], m["terms"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    db = np.asarray(dims_b, dtype=np.uint32)
    na, nb, q = len(xa), len(xb), Theta.shape[1]
    dxa, dxb, dth, dcv = up(xa.T), up(xb.T), up(Theta.T), up(cv)
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    mean, var, out = nan(q * nb * lda + pad), nan(nb * lda + pad), nan(2 * nb + pad)
    call("obhip_predict_product_dev", m["om_d"]._h, t._h, dth.data_ptr(), q, db.ctypes.data, db.size, dxa.data_ptr(), na,
         dxb.data_ptr(), nb, mean.data_ptr(), lda, dcv.data_ptr(), SIGMA, var.data_ptr())
    if y is not None:
        dy, dov = up(y), up(ov)
        call("obhip_product_loglik_dev", m["om_d"]._h, t._h, dth.data_ptr(), db.ctypes.data, db.size, dxa.data_ptr(), na,
             dy.data_ptr(), dov.data_ptr(), dxb.data_ptr(), nb, dcv.data_ptr(), SIGMA, out.data_ptr())
    return mean.cpu().numpy(), var.cpu().numpy(), out.cpu().numpy()


def test_same_bits_on_a_second_call(monkeypatch):
    m, seed, xa, xb, ref = reference("mixed d4 p700", 130, 17, (0, 1, 2))
    Theta, cv = coefficients(m, 3, seed)
    y, ov = field_data(ref, Theta[:, 0], seed, 130)
    for which in ROUTES:
        route(monkeypatch, which)
        first = raw_call(m, Theta, xa, xb, (0, 1, 2), cv, 130, y, ov)
        again = raw_call(m, Theta, xa, xb, (0, 1, 2), cv, 130, y, ov)
        for a, b in zip(first, again):
            assert np.array_equal(a, b, equal_nan=True), which


def test_masking_and_untouched_memory(monkeypatch):
    """na = 65: the 63 padding rows of the second A tile stay out of the sums -- chi2 and logdet equal those
    of rows 0..63 plus the one-row call's -- and nothing is written past nb x 2, past q nb lda or into the
    rows na..lda of a column"""
    na, nb, dims_b, lda, q = 65, 64, (1, 3), 70, 2
    m, seed, xa, xb, ref = reference("mixed d4 p129", na, nb, dims_b)
    Theta, cv = coefficients(m, q, seed)
    y, ov = field_data(ref, Theta[:, 0], seed, na)
    (c2, t2), (lg, tl) = ref.sums(Theta[:, 0], y, ov, cv, SIGMA)
    rep = Report("masking")
    for which in ROUTES:
        route(monkeypatch, which)
        mean, var, out = raw_call(m, Theta, xa, xb, dims_b, cv, lda, y, ov)
        assert np.all(np.isnan(mean[q * nb * lda:])) and np.all(np.isnan(var[nb * lda:])) and np.all(np.isnan(out[2 * nb:]))
        mean, var = mean[:q * nb * lda].reshape(q, nb, lda), var[:nb * lda].reshape(nb, lda)
        assert np.all(np.isnan(mean[:, :, na:])) and np.all(np.isnan(var[:, na:]))
        assert np.all(np.isfinite(mean[:, :, :na])) and np.all(np.isfinite(var[:, :na])) and np.all(np.isfinite(out[:2 * nb]))
        for r in range(q):
            want, tol = ref.mean(Theta[:, r])
            rep.check("%s mean, lda = %d, response %d" % (which, lda, r), mean[r, :, :na].T, want, tol)
        head = raw_call(m, Theta, xa[:64], xb, dims_b, cv, 64, y[:64], ov[:64])[2][:2 * nb]
        last = raw_call(m, Theta, xa[64:], xb, dims_b, cv, 1, y[64:], ov[64:])[2][:2 * nb]
        for w, (what, want, tol) in enumerate((("chi2", c2, t2), ("logdet", lg, tl))):
            got, parts = out[w * nb:(w + 1) * nb], head[w * nb:(w + 1) * nb] + last[w * nb:(w + 1) * nb]
            rep.check("%s %s" % (which, what), got, want, tol)
            rep.check("%s %s of rows 0..63 + row 64" % (which, what), parts, want, tol + E.U * np.abs(parts))
            # a padding row in the sums would add a term of the size of a real one: far above this
            assert np.max(np.abs(got - parts)) <= 2 * np.max(tol + E.U * np.abs(parts)), (which, what)
    rep.done()
