"""The GLM fit on the device (obhip_glm_rows_dev, obhip_fit_glm_dev, obhip_predict_glm_dev, outerbase_amd.glm)
against the long-double reference of tests/glm_ref.py.  No tolerance below is a fixed figure: each is the
rounding bound of what is compared, or eight times the distance the float64 restatement of the same
computation keeps from the long-double one on the same inputs (extended_ref.constant_from_oracle_ratio's
rule); every test prints its figures before it asserts."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import extended_ref as E
import glm_ref as R
from conftest import knots_for, make_pair

pytestmark = pytest.mark.gpu

ld = np.longdouble
U = 2.0 ** -53
TINY = float(np.finfo(np.float64).tiny)
FAMILIES = [R.GAUSSIAN, R.BINOMIAL, R.POISSON]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Case:
    """model pair, terms, prior precisions; bases and fits on it"""

    def __init__(self, p, rho, kinds=R.KINDS, knots=20, drop_constant=False):
        import ob_oracle as O
        from outerbase_amd import obmod
        self.kinds, self.rho, self.d = kinds, rho, len(kinds)
        self.knots = knots_for(kinds, knots)
        self.om_o, self.om = make_pair(kinds, self.knots)
        terms = self.om_o.selectterms(p + 1 if drop_constant else p)
        if drop_constant:
            assert not terms[0].any() and terms[1:].any(axis=1).all()
            terms = np.ascontiguousarray(terms[1:])
        self.terms, self.p = terms, len(terms)
        self.t = obmod._Terms(self.om, terms)
        self.prec = O.prior_prec(self.om_o, terms, rho)

    def basis(self, x):
        from outerbase_amd._lib import call
        self.dx = _t(x.T)
        h = C.c_void_p()
        call("obhip_basis_create_dev", C.byref(h), self.om._h, self.dx.data_ptr(), x.shape[0],
             self.t.maxlevels().ctypes.data)
        return h

    def getmat(self, basis, n):
        from outerbase_amd._lib import call
        B = np.empty((n, self.p), order="F")
        call("obhip_basis_getmat", basis, self.t._h, B.ctypes.data)
        return B

    def fit(self, basis, n, family, y, a=None, o=None, tol=R.TOL, maxit=25, rho=None, theta0=None):
        """-> dict(rc, theta, eta, H, diagH, info)"""
        import torch
        from outerbase_amd._lib import call, lib
        from outerbase_amd.glm import GlmInfo
        p = self.p
        wsb = C.c_uint64(0)
        call("obhip_glm_workspace_bytes", p, n, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
        nan = float("nan")
        H = torch.full((p, p), nan, dtype=torch.float64, device="cuda")
        th = torch.full((p,), nan, dtype=torch.float64, device="cuda") if theta0 is None else _t(theta0)
        dh = torch.full((p,), nan, dtype=torch.float64, device="cuda")
        eta = torch.full((n,), nan, dtype=torch.float64, device="cuda")
        dy, da, do = _t(y), None if a is None else _t(a), None if o is None else _t(o)
        info = GlmInfo()
        info.warm_start = 0 if theta0 is None else 1
        rc = lib.obhip_fit_glm_dev(basis, self.t._h, self.om._h, family, dy.data_ptr(), _ptr(da), _ptr(do), R.SIGMA,
                                   self.rho if rho is None else rho, tol, maxit, H.data_ptr(), th.data_ptr(),
                                   dh.data_ptr(), eta.data_ptr(), C.byref(info), ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
        return dict(rc=rc, theta=th.cpu().numpy(), eta=eta.cpu().numpy(), H=H, diagH=dh.cpu().numpy(), info=info,
                    iterations=int(info.iterations), halvings=int(info.halvings), converged=bool(info.converged))


@functools.lru_cache(maxsize=None)
def case(p, rho):
    return _Case(p, rho)


def _counts(r):
    return (r["iterations"], r["halvings"], r["converged"])


# ---- 1. the row pass --------------------------------------------------------------------------------
def _row_inputs(family, n, seed):
    rng = np.random.default_rng(seed)
    eta = 3.0 * rng.standard_normal(n)
    special = [40.0, -40.0, 745.0, -745.0, 709.0, -800.0, 800.0]
    eta[:len(special)] = special
    a = rng.uniform(0.5, 3.0, n)
    a[:len(special)] = 1.0                  # (a e^709 stays finite)
    if family == R.BINOMIAL:
        m = rng.integers(1, 6, n)
        y = rng.integers(0, 6, n) % (m + 1) / m
        y[:8] = [1.0, 0.0, 1.0, 0.0, 0.5, 0.0, 1.0, 0.25]
    elif family == R.POISSON:
        y = rng.poisson(3.0, n).astype(np.float64)
        y[:8] = [0.0, 2.0, 1.0, 0.0, 3.0, 0.0, 1.0, 0.0]
    else:
        y = eta + rng.standard_normal(n)
    scale = rng.uniform(0.2, 2.0, n)
    return eta, y, a, scale


def _padded(v, n_pad):
    out = np.full(n_pad, np.nan)
    out[:len(v)] = v
    return out


def _entry_ratio(got, want, den):
    """max |got - want| / den over the entries (0 for an empty selection)"""
    if len(want) == 0:
        return 0.0
    err = np.abs(np.asarray(got, dtype=ld) - want)
    return float(np.max(err / np.maximum(den, TINY)))


@pytest.mark.parametrize("n", [37, 64, 1000, 200003])
@pytest.mark.parametrize("family", FAMILIES)
def test_row_pass_against_the_long_double_formulas(family, n):
    """mu, scale sqrt(w), u per entry and the three sums of obhip_glm_rows_dev.  Sizes: a partial row tile,
    exactly one, several, and more rows than the first stage of the sum has threads (several strides).  eta
    carries +-40, +-745, 709, -800 and 800 (Poisson: e^745 and e^800 overflow, two rows are counted and left
    out), y carries 0, 1 and proportions (Poisson: 0); every input buffer holds NaN from row n to the end of
    its row tile.  Per entry the error is taken relative to the entry (u: to a (|y| + mu) / sqrt(w), the terms
    it is the difference of), separately on the rows with |eta| <= 700 and beyond (where e^{-|eta|} is
    subnormal and w keeps a digit or none in any float64 evaluation), and held to eight times the NumPy
    float64 evaluation's own worst on the same rows.  The sums: gamma(n) sum |summand| for the order plus
    that constant times the magnitudes for the summands."""
    import torch
    from outerbase_amd._lib import call
    eta, y, a, scale = _row_inputs(family, n, 100 * family + n)
    n_pad = (n + 63) // 64 * 64
    d = {k: _t(_padded(v, n_pad)) for k, v in dict(eta=eta, y=y, a=a, scale=scale).items()}

    def run(trial=False):
        out = {k: torch.full((n_pad,), 7.0, dtype=torch.float64, device="cuda") for k in ("eta", "mu", "sw", "u")}
        sums = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
        o = {k: None for k in out} if trial else {k: v.data_ptr() for k, v in out.items()}
        call("obhip_glm_rows_dev", family, n, d["eta"].data_ptr(), None, 0.0, d["y"].data_ptr(), d["a"].data_ptr(), None,
             R.SIGMA, d["scale"].data_ptr(), o["eta"], o["mu"], o["sw"], o["u"], sums.data_ptr())
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}, sums.cpu().numpy()
    got, sums = run()
    got2, sums2 = run()
    _, sums_trial = run(trial=True)
    r64 = R.rows(family, eta, y, a, scale=scale)
    rl = R.rows(family, eta, y, a, scale=scale, dtype=ld)
    # the padding, and the rows without weight
    assert np.all(got["sw"][n:] == 0.0) and np.all(got["u"][n:] == 0.0)
    assert np.all(got["eta"][n:] == 7.0) and np.all(got["mu"][n:] == 7.0)
    dead = ~((r64["w"] > 0) & np.isfinite(r64["w"]))
    assert dead.sum() >= (0 if family == R.GAUSSIAN else 2)
    assert np.all(got["sw"][:n][dead] == 0.0) and np.all(got["u"][:n][dead] == 0.0)
    assert np.array_equal(got["eta"][:n], eta)
    for k in got:
        assert np.array_equal(got[k], got2[k], equal_nan=True)
    assert np.array_equal(sums, sums2) and np.array_equal(sums, sums_trial)
    assert np.all(np.isfinite(got["sw"])) and np.all(np.isfinite(got["u"]))
    # per entry
    live = ~dead
    uden = np.asarray(a * (np.abs(y) + np.abs(rl["mu"])), dtype=ld)
    if family == R.GAUSSIAN:
        uden = uden * math.exp(-2 * R.SIGMA)
    uden = uden / np.where(live, rl["sw"], 1)
    for name, sel in (("|eta| <= 700", live & (np.abs(eta) <= 700)), ("beyond", live & (np.abs(eta) > 700))):
        for key, gk, den in (("mu", "mu", np.abs(rl["mu"])), ("scale_w", "sw", np.abs(rl["scale_w"])), ("u", "u", uden)):
            ref64 = r64[key]
            e_np = _entry_ratio(ref64[sel], rl[key][sel], den[sel])
            e_dev = _entry_ratio(got[gk][:n][sel], rl[key][sel], den[sel])
            print("%s n=%d rows %s (%d): %s error / entry device %.3g, NumPy float64 %.3g"
                  % (R.FAMILY_NAMES[family], n, name, int(sel.sum()), key, e_dev, e_np))
            assert e_dev <= 8.0 * e_np
    # the sums: the rows left out are counted and the sum stays finite; the bound is checked on a second (trial)
    # pass with the rows beyond |eta| = 700 moved to eta = 1 (a Poisson mean of e^709 would drown every other
    # summand, and its bound with them)
    want_count = 2 if family == R.POISSON else 0
    # (an overflow is a fact of float64: the long-double e^745 is finite)
    assert sums[2] == want_count and r64["sums"][2] == want_count
    assert np.isfinite(sums[0]) and np.isfinite(sums[1])
    eta = np.where(np.abs(eta) > 700, 1.0, eta)
    d["eta"] = _t(_padded(eta, n_pad))
    _, sums = run(trial=True)
    r64, rl = R.rows(family, eta, y, a), R.rows(family, eta, y, a, dtype=ld)
    fin = rl["fin"]
    assert fin.all() and sums[2] == 0
    absl = float(np.sum(np.abs(rl["al"][fin])))
    summag = float(rl["sums"][1])
    magf = np.where(fin, rl["mag"], 1)
    c_l = E.constant_from_oracle_ratio(np.max(np.abs(np.where(fin, (r64["al"] - rl["al"]) / magf, 0))))
    c_m = E.constant_from_oracle_ratio(np.max(np.abs(np.where(fin, (r64["mag"] - rl["mag"]) / magf, 0))))
    tol_l = E.gamma(n) * absl + c_l * summag
    tol_m = (E.gamma(n) + c_m) * summag
    e_l, e_m = abs(float(sums[0] - rl["sums"][0])), abs(float(sums[1] - rl["sums"][1]))
    print("%s n=%d: sum a l error %.3g (allowed %.3g; NumPy %.3g), sum of magnitudes error %.3g (allowed %.3g), rows "
          "left out %d" % (R.FAMILY_NAMES[family], n, e_l, tol_l, abs(float(r64["sums"][0] - rl["sums"][0])), e_m, tol_m,
                           int(sums[2])))
    assert np.isfinite(sums[0]) and e_l <= tol_l and e_m <= tol_m


def test_row_pass_start_and_trial_step():
    """eta = o + alpha deta where a pass starts from the offset (d_eta NULL): one fused multiply-add per row,
    so within 2^-53 |eta| of the exact value; weights NULL are ones; a trial pass gives the bits of the pass
    that writes."""
    import torch
    from outerbase_amd._lib import call
    n, n_pad, fam = 1000, 1024, R.POISSON
    rng = np.random.default_rng(5)
    o, deta, y = rng.standard_normal(n), rng.standard_normal(n), rng.poisson(2.0, n).astype(np.float64)
    do, dd, dy, dsc = _t(o), _t(deta), _t(y), _t(np.ones(n_pad))
    out = [torch.full((n_pad,), 7.0, dtype=torch.float64, device="cuda") for _ in range(4)]
    s1 = torch.zeros(3, dtype=torch.float64, device="cuda")
    s2 = torch.zeros(3, dtype=torch.float64, device="cuda")
    call("obhip_glm_rows_dev", fam, n, None, dd.data_ptr(), 0.25, dy.data_ptr(), None, do.data_ptr(), 0.0, dsc.data_ptr(),
         out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), s1.data_ptr())
    call("obhip_glm_rows_dev", fam, n, None, dd.data_ptr(), 0.25, dy.data_ptr(), None, do.data_ptr(), 0.0, None,
         None, None, None, None, s2.data_ptr())
    torch.cuda.synchronize()
    exact = np.asarray(o, dtype=ld) + ld(0.25) * np.asarray(deta, dtype=ld)
    err = np.abs(np.asarray(out[0].cpu().numpy()[:n], dtype=ld) - exact)
    print("start pass: eta error / (2^-53 |eta|) %.3g" % float(np.max(err / (U * np.abs(exact)))))
    assert np.all(err <= U * np.abs(exact))
    assert torch.equal(s1, s2)
    eta = out[0].cpu().numpy()[:n]
    rl = R.rows(fam, eta, y, np.ones(n), dtype=ld)
    assert abs(float(s1[0].item() - rl["sums"][0])) <= (E.gamma(n) + 8 * U) * float(rl["sums"][1])


# ---- 2. one iteration: the weighted Gram through every Gram path ------------------------------------------
@pytest.mark.parametrize("mode", ["whole", "chunk", "backend3"])
@pytest.mark.parametrize("n,p,rho", R.SIZES)
def test_one_iteration_forms_the_weighted_hessian(n, p, rho, mode, monkeypatch):
    """maxit = 1 from theta = 0 (binomial with trials as weights: w = a / 4 at eta = 0): the Hessian against
    extended_ref.ref_gram of the long-double B scaled by sqrt(w), plus P, under its bound rule on
    gram_column_sample's columns, and d_diagH likewise.  The factorisation leaves L in the lower triangle of d_H
    and uses the strict upper triangle as scratch (kernels_chol.hip), so the Hessian is taken back from its
    factor, L L^T in long double, and the bound grows by the backward error of a Cholesky factorisation in any
    order of summation, gamma(p + 1) |L| |L|^T (Higham, Accuracy and Stability, theorem 10.3).  The exchanged row factors must reach the staged matrix
    (whole), its row chunks (OBHIP_GRAM_CHUNK_ROWS=1024; GramFuse declined) and the fused kernel (backend 3)."""
    import ob_oracle as O
    from outerbase_amd._lib import call, lib
    c = case(p, rho)
    x, y, a, o = R.data(R.BINOMIAL, n)
    ref = E.ExtendedRef(c.kinds, [np.asarray(k, dtype=np.float64) for k in c.knots], c.om_o.hyp, c.om_o.rotmat, x)
    B, bB = ref.getmat(c.terms)
    Bo = O.ob_getmat(O.OuterBase(c.om_o, x), c.terms)
    Cc = E.constant_from_oracle_ratio(E.worst_ratio(Bo, B, bB))
    sw = R.rows(R.BINOMIAL, np.zeros(n), y, a, dtype=ld)["sw"]
    # (the float64 square root and its product with the row factor, two roundings more per entry: the 4 u |B_w|^T
    # |B_w| added to the bound below)
    Bw, bBw = B * sw[:, None], bB * sw[:, None]
    cols = E.gram_column_sample(bBw, 11)
    want, tol = E.ref_gram(Bw, bBw, cols, Cc, extra=1)
    want[np.arange(len(cols)), cols] += np.asarray(c.prec, dtype=ld)[cols]
    tol = tol + 4 * U * np.abs(E._f64(Bw)[:, cols].T @ E._f64(Bw))
    if mode == "chunk":
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", "1024")
    if mode == "backend3":
        call("obhip_set_gram_backend", 3)
    basis = c.basis(x)
    try:
        r = c.fit(basis, n, R.BINOMIAL, y, a, o, maxit=1)
    finally:
        lib.obhip_basis_destroy(basis)
        call("obhip_set_gram_backend", 0)
    assert r["rc"] == 0 and r["iterations"] == 1 and not r["converged"]
    L = np.tril(r["H"].cpu().numpy())
    Ll = np.asarray(L, dtype=ld)
    tol = tol + E.gamma(p + 1) * (np.abs(L)[cols, :] @ np.abs(L).T)
    upper = np.arange(p)[None, :] > cols[:, None]
    ratio = E.ratio_map(E._f64(Ll[cols, :] @ Ll.T), want, tol)
    r_up = float(np.max(ratio[upper]))
    r_diag = float(np.max(E.ratio_map(r["diagH"][cols], want[np.arange(len(cols)), cols], tol[np.arange(len(cols)), cols])))
    print("one iteration %s n=%d p=%d: C %.3g, L L^T off the diagonal error / bound %.3g, diagH %.3g"
          % (mode, n, p, Cc, r_up, r_diag))
    assert np.all(np.isfinite(L)) and np.all(np.isfinite(r["diagH"]))
    assert r_up <= 1.0 and r_diag <= 1.0


# ---- 3. converged fits ----------------------------------------------------------------------------------
def _fit_against_reference(c, n, family, x, y, a, o, label, hessian64=False, only_eta=False):
    from outerbase_amd._lib import lib
    basis = c.basis(x)
    try:
        B = c.getmat(basis, n)
        r = c.fit(basis, n, family, y, a, o)
    finally:
        lib.obhip_basis_destroy(basis)
    assert r["rc"] == 0
    r64 = R.fit(B, c.prec, family, y, a, o, dtype=np.float64)
    rl = R.fit(B, c.prec, family, y, a, o, dtype=ld, hessian64=hessian64)
    dist = min(R.threshold_distance(r64), R.threshold_distance(rl))
    print("%s: iterations / halvings / converged device %s, float64 %s, long double %s; dec of the last step device "
          "%.3g; decs float64 %s, long double %s; nearest dec / threshold factor %.3g"
          % (label, _counts(r), _counts(r64), _counts(rl), r["info"].dec, ["%.3g" % v for v in r64["decs"]],
             ["%.3g" % v for v in rl["decs"]], dist))
    assert dist >= 100.0, "a decrement this close to its threshold makes the case invalid: choose another seed"
    assert _counts(r) == _counts(rl) == _counts(r64) and r["converged"]
    mu_dev = R.link(family, np.asarray(r["eta"], dtype=ld))[0]
    worst = 0.0
    for key, got in (("eta", r["eta"]), ("mu", mu_dev), ("theta", r["theta"])):
        e_dev, e_64 = R.relerr(got, rl[key]), R.relerr(r64[key], rl[key])
        print("%s: %s device %.3g, float64 restatement %.3g of the largest entry" % (label, key, e_dev, e_64))
        if not (only_eta and key != "eta"):
            worst = max(worst, e_dev / (8.0 * e_64))
    f_rel = abs(r["info"].F - rl["F"]) / abs(rl["F"])
    d_rel = abs(r["info"].deviance - rl["deviance"]) / abs(rl["deviance"])
    print("%s: F %.17g (reference %.17g, relative %.3g), deviance %.17g (relative %.3g)"
          % (label, r["info"].F, rl["F"], f_rel, r["info"].deviance, d_rel))
    # F and the deviance are sums of n + p terms of either sign: the order's bound relative to sum |summand|,
    # which is below 1e3 |F| on these cases (printed above), so 1e3 (n + p) 2^-53
    assert f_rel <= 1e3 * (n + c.p) * U and d_rel <= 1e3 * (n + c.p) * U
    assert worst <= 1.0
    return r, rl


@pytest.mark.parametrize("n,p,rho", R.SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_converged_fit_against_the_long_double_reference(family, n, p, rho):
    """eta, mu and theta of obhip_fit_glm_dev (tol = 1e-13) against the long-double reference run on
    obhip_basis_getmat's B: the same iterations and halvings as the reference (Poisson: 6 and 2, its first step
    overshoots) and within eight times the float64 restatement's own distance."""
    x, y, a, o = R.data(family, n)
    _fit_against_reference(case(p, rho), n, family, x, y, a, o, "%s n=%d p=%d rho=%g" % (R.FAMILY_NAMES[family], n, p, rho))


def test_converged_fit_with_the_star_kernels():
    """p = 2400 on twenty dimensions: nine star-waves and more, so B delta and B_w^T u go through the star
    kernels.  eta only, against the reference whose Hessian alone is formed in float64."""
    from test_gpu_star import share_info
    kinds = ["mat25"] * 20
    c = _Case(2400, 3.0, kinds=kinds, knots=40)
    info = share_info(c.om, c.terms)
    print("star case: %s" % {k: info[k] for k in ("nswf", "nleft")})
    assert info["nswf"] >= 9
    x, y, a, o = R.data(R.BINOMIAL, 2000, kinds=kinds)
    _fit_against_reference(c, 2000, R.BINOMIAL, x, y, a, o, "star binomial n=2000 p=2400", hessian64=True, only_eta=True)


# ---- 4. identities ----------------------------------------------------------------------------------------
def test_gaussian_family_without_weights_is_the_one_step_fit():
    """a = 1, o = 0: theta against obhip_fit_newton_multi_dev (q = 1) on the same basis, by the normwise backward
    error of test_multi_solve_backward_error in the system (e2 B^T B + P) theta = e2 B^T y formed in long double
    from getmat's B: within max(4 eta_single, (n + p) 2^-53), n for the rounding of the Gram's sums."""
    import torch
    from outerbase_amd._lib import call, lib
    n, p, rho = 1000, 129, 6.0
    c = case(p, rho)
    x, y, _, _ = R.data(R.GAUSSIAN, n)
    basis = c.basis(x)
    try:
        B = c.getmat(basis, n)
        r = c.fit(basis, n, R.GAUSSIAN, y)
        wsb = C.c_uint64(0)
        call("obhip_newton_multi_workspace_bytes", p, 1, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
        H = torch.empty((p, p), dtype=torch.float64, device="cuda")
        g, th, dh = (torch.empty(p, dtype=torch.float64, device="cuda") for _ in range(3))
        dy = _t(y)
        call("obhip_fit_newton_multi_dev", None, basis, c.t._h, c.om._h, dy.data_ptr(), 1, n, R.SIGMA, rho, H.data_ptr(),
             g.data_ptr(), th.data_ptr(), dh.data_ptr(), None, 0, ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
    finally:
        lib.obhip_basis_destroy(basis)
    assert r["rc"] == 0 and _counts(r) == (2, 0, True)
    Bl, e2 = np.asarray(B, dtype=ld), np.exp(-2 * ld(R.SIGMA))
    Hl = e2 * (Bl.T @ Bl) + np.diag(np.asarray(c.prec, dtype=ld))
    rhs = e2 * (Bl.T @ np.asarray(y, dtype=ld))

    def backward(theta):
        t = np.asarray(theta, dtype=ld)
        return float(np.max(np.abs(Hl @ t - rhs)) / (np.max(np.sum(np.abs(Hl), axis=1)) * np.max(np.abs(t)) + np.max(np.abs(rhs))))
    e_glm, e_one = backward(r["theta"]), backward(th.cpu().numpy())
    print("gaussian family against the one-step fit: backward error %.3g, one-step fit %.3g, theta apart %.3g"
          % (e_glm, e_one, R.relerr(r["theta"], th.cpu().numpy())))
    assert e_glm <= max(4 * e_one, (n + p) * U)
    assert np.allclose(r["diagH"], dh.cpu().numpy(), rtol=1e-12)


@functools.lru_cache(maxsize=None)
def _weights_case(family):
    """integer weights against the same rows repeated: device and float64 reference, each both ways"""
    from outerbase_amd._lib import lib
    n, p, rho = 1000, 129, 0.0
    c = case(p, rho)
    x, y, a, o = R.data(family, n)
    k = np.random.default_rng(17).integers(1, 4, n)
    rep = np.repeat(np.arange(n), k)
    aw = k.astype(np.float64) * (1.0 if a is None else a)
    out = {}
    for name, (xx, yy, aa, oo) in dict(weighted=(x, y, aw, o), repeated=(x[rep], y[rep], None if a is None else a[rep],
                                                                         None if o is None else o[rep])).items():
        basis = c.basis(xx)
        try:
            B = c.getmat(basis, len(yy))
            out[name] = c.fit(basis, len(yy), family, yy, aa, oo)
        finally:
            lib.obhip_basis_destroy(basis)
        out[name + "64"] = R.fit(B, c.prec, family, yy, aa, oo, dtype=np.float64)
        assert out[name]["rc"] == 0
    out["dev"] = R.relerr(out["weighted"]["theta"], out["repeated"]["theta"])
    out["ref"] = R.relerr(out["weighted64"]["theta"], out["repeated64"]["theta"])
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_integer_weights_are_repeated_rows(family):
    """a_i in {1, 2, 3} (times the case's own weights) against the same rows repeated a_i times: the two device
    fits agree as the float64 reference's own two runs agree (eight times that), with equal counts."""
    w = _weights_case(family)
    print("%s weights against repeated rows: theta device %.3g, float64 reference %.3g; counts %s %s"
          % (R.FAMILY_NAMES[family], w["dev"], w["ref"], _counts(w["weighted"]), _counts(w["repeated"])))
    assert _counts(w["weighted"]) == _counts(w["repeated"]) == _counts(w["weighted64"]) == _counts(w["repeated64"])
    assert w["dev"] <= 8.0 * w["ref"]


def test_binomial_complement_negates_the_coefficients():
    """y -> 1 - y gives theta -> -theta, held to the figure measured for the binomial family above"""
    from outerbase_amd._lib import lib
    n, p, rho = 1000, 129, 0.0
    c = case(p, rho)
    x, y, a, o = R.data(R.BINOMIAL, n)
    basis = c.basis(x)
    try:
        r1 = c.fit(basis, n, R.BINOMIAL, y, a)
        r2 = c.fit(basis, n, R.BINOMIAL, 1.0 - y, a)
    finally:
        lib.obhip_basis_destroy(basis)
    lim = 8.0 * _weights_case(R.BINOMIAL)["ref"]
    e = R.relerr(-r2["theta"], r1["theta"])
    print("binomial complement: theta + theta' %.3g of the largest entry (allowed %.3g), counts %s %s"
          % (e, lim, _counts(r1), _counts(r2)))
    assert r1["rc"] == 0 and r2["rc"] == 0 and _counts(r1) == _counts(r2)
    assert e <= lim


def test_poisson_offset_without_a_constant_term():
    """with no constant term in the term set a shift of the offset cannot be absorbed by a coefficient: the fit
    with o - 0.5 against the long-double reference, as the converged fits above"""
    n = 1000
    c = _Case(128, 0.0, drop_constant=True)
    x, y, a, o = R.data(R.POISSON, n)
    _fit_against_reference(c, n, R.POISSON, x, y, a, o - 0.5, "poisson offset - 0.5, no constant term, n=1000 p=128")


# ---- 5. the basis comes back intact ----------------------------------------------------------------------
def test_the_basis_is_handed_back_intact():
    """obhip_basis_getmat and a Gaussian obhip_fit_newton_multi_dev before and after obhip_fit_glm_dev on the same
    handle give equal bits -- after a fit that converges, after one that ends with OBHIP_ERR_NUMERIC (Poisson,
    rho = -40, y scaled by 1e300: the step overflows every trial) and after OBHIP_ERR_INVALID; the host-buffer
    entry refuses data outside the family's domain."""
    import torch
    from outerbase_amd._lib import call, lib
    n, p, rho = 1000, 129, 0.0
    c = case(p, rho)
    x, y, a, o = R.data(R.POISSON, n)
    yg = R.data(R.GAUSSIAN, n)[1]
    basis = c.basis(x)

    def snapshot():
        B = c.getmat(basis, n)
        wsb = C.c_uint64(0)
        call("obhip_newton_multi_workspace_bytes", p, 1, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
        H = torch.empty((p, p), dtype=torch.float64, device="cuda")
        g, th, dh = (torch.empty(p, dtype=torch.float64, device="cuda") for _ in range(3))
        dy = _t(yg)
        call("obhip_fit_newton_multi_dev", None, basis, c.t._h, c.om._h, dy.data_ptr(), 1, n, R.SIGMA, 6.0, H.data_ptr(),
             g.data_ptr(), th.data_ptr(), dh.data_ptr(), None, 0, ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
        return B, g.cpu().numpy(), th.cpu().numpy(), dh.cpu().numpy(), torch.tril(H).cpu().numpy()
    try:
        s0 = snapshot()
        s1 = snapshot()                      # (the second fit finds the staged matrix: response 0 by its own pass)
        ok = c.fit(basis, n, R.POISSON, y, a, o)
        s2 = snapshot()
        s3 = snapshot()
        bad = c.fit(basis, n, R.POISSON, y * 1e300, a, o, rho=-40.0, maxit=100)
        msg = lib.obhip_last_error().decode()
        s4 = snapshot()
        inv = c.fit(basis, n, 9, y, a, o)
        s5 = snapshot()
        yb = np.ascontiguousarray(R.data(R.BINOMIAL, n)[1])
        th = np.zeros(p)
        from outerbase_amd.glm import GlmInfo
        info = GlmInfo()

        def host(yy, aa):
            return lib.obhip_fit_glm(basis, c.t._h, c.om._h, R.BINOMIAL, yy.ctypes.data, None if aa is None else aa.ctypes.data,
                                     None, 0.0, 0.0, 1e-8, 25, th.ctypes.data, None, None, C.byref(info))
        ybad, abad = yb.copy(), np.ones(n)
        ybad[7], abad[9] = 1.5, 0.0
        rc_y, rc_a, rc_ok = host(ybad, None), host(yb, abad), host(yb, None)
        s6 = snapshot()
    finally:
        lib.obhip_basis_destroy(basis)
    print("intact: converged fit rc %d, overflowing fit rc %d (%s), unknown family rc %d, host entry rc %d %d %d"
          % (ok["rc"], bad["rc"], msg, inv["rc"], rc_y, rc_a, rc_ok))
    assert ok["rc"] == 0 and ok["converged"] and bad["rc"] == 5 and inv["rc"] == 1
    assert rc_y == 1 and rc_a == 1 and rc_ok == 0 and info.converged == 1
    # (s0, s2, s4, s6 stage the design matrix anew, s1, s3, s5 find it staged: B^T y rides along or not)
    for first, later in ((s0, s2), (s0, s4), (s1, s3), (s1, s5), (s0, s6)):
        for u, v in zip(first, later):
            assert np.array_equal(u, v)


# ---- 6. the predictor -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["binomial", "poisson"])
def test_predict_on_link_and_response_scale(family):
    """GlmFit.predict against B(xnew) theta from getmat pushed through the long-double inverse link, with and
    without an offset.  Link scale: the dot product's bound (p + 2 d) 2^-53 |B| |theta| (test_gpu_multi_response's),
    one rounding more for the offset; response scale: that bound times d mu / d eta plus four roundings of mu.
    Variances: B^2 (1 / diagH) under the same dot-product bound, the response's (d mu / d eta)^2 times it, where
    |d log (d mu / d eta) / d eta| <= 1 carries the error of eta over.  n = 0 gives empty arrays."""
    import ob_oracle as O
    import outerbase_amd as ob
    fam = ob.glm.FAMILIES[family]
    n, p = 1000, 129
    c = case(p, 0.0)
    x, y, a, o = R.data(fam, n)
    fit = ob.fit_glm(c.om, c.terms, x, y, family=family, weights=a, offset=o, rho=0.0, tol=R.TOL)
    want_counts = (5, 0) if fam == R.BINOMIAL else (6, 2)
    print("%s fit_glm: iterations %d halvings %d converged %s deviance %.6g logpost %.6g"
          % (family, fit.iterations, fit.halvings, fit.converged, fit.deviance, fit.logpost))
    assert (fit.iterations, fit.halvings) == want_counts and fit.converged
    assert fit.coeff.shape == (p,) and fit.diagH.shape == (p,) and fit.eta.shape == (n,)
    xn, _ = O.synth_xy(9, 0, 333, c.kinds)
    on = np.log(np.random.default_rng(2).uniform(0.5, 4.0, 333))
    B = ob.outerbase(c.om, xn, levelcap=c.t.maxlevels()).getmat(c.terms)
    Bl, th, cv = np.asarray(B, dtype=ld), np.asarray(fit.coeff, dtype=ld), np.asarray(1.0 / fit.diagH, dtype=ld)
    k = (p + 2 * c.d) * U
    for off in (None, on):
        eta = Bl @ th + (0 if off is None else np.asarray(off, dtype=ld))
        tol_eta = k * (np.abs(B) @ np.abs(fit.coeff)) + U * np.abs(E._f64(eta))
        var = (Bl * Bl) @ cv
        tol_var = k * E._f64(var) + TINY
        mu, dmu, _ = R.link(fam, eta)
        got_l, got_lv = fit.predict(xn, offset=off, kind="link", var=True)
        got_r, got_rv = fit.predict(xn, offset=off, var=True)
        assert np.array_equal(got_l, fit.predict(xn, offset=off, kind="link")) and np.array_equal(got_r, fit.predict(xn, offset=off))
        tol_mu = E._f64(dmu) * tol_eta + 4 * U * E._f64(mu)
        tol_rv = E._f64(dmu * dmu * var) * (2 * tol_eta + 8 * U) + E._f64(dmu * dmu) * tol_var
        rs = [E.worst_ratio(g, w, t) for g, w, t in ((got_l, eta, tol_eta), (got_lv, var, tol_var), (got_r, mu, tol_mu),
                                                     (got_rv, dmu * dmu * var, tol_rv))]
        print("%s predict offset=%s: error / bound link %.3g, its variance %.3g, response %.3g, its variance %.3g"
              % (family, off is not None, rs[0], rs[1], rs[2], rs[3]))
        assert max(rs) <= 1.0
    assert fit.predict(np.zeros((0, c.d))).shape == (0,)
    m0, v0 = fit.predict(np.zeros((0, c.d)), var=True)
    assert m0.shape == v0.shape == (0,)
