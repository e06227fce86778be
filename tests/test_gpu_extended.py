"""Every kernel family against the extended-precision instrument of tests/extended_ref.py, per entry.

The older parity tests compare with the float64 oracle by max |a - b| / max |b| and widen that flat
tolerance to 1e-5 .. 1e-7 where term sets reach high levels.  Here every entry of every result is
held to  C x (its own propagated conditioning bound) + gamma_k x (sum of |summands|)  against long
double sums (see extended_ref's docstring); C is eight times what the float64 oracle itself measures
on the same case (its rows, and a 300-row sample where they are few), at most 2e-13.  All models share the oracle's rotation (make_pair), so only
kernels are compared.  Each check prints one line: max-norm error and max(err / tolerance) of the
device and of the oracle -- the log shows whose the old 1e-6 was."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import extended_ref as E
from conftest import knots_for, make_pair, sample_x
from extended_products_worker import device_products
from test_gpu_parity import random_terms
from test_gpu_star import share_info

pytestmark = pytest.mark.gpu


class Report:
    """one printed line per check; the case fails at its end with every line above tolerance"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def check(self, what, got, want, tol, oracle=None, floor=0.0):
        assert np.all(np.isfinite(got)), (self.case, what)
        rmap = E.ratio_map(got, want, tol, floor)
        worst = float(rmap.max())
        line = "%s | %s: device max-norm %.3g err/tol %.3g" % (self.case, what, E.maxnorm_relerr(got, want), worst)
        if oracle is not None:
            line += "; oracle max-norm %.3g err/tol %.3g" % (E.maxnorm_relerr(oracle, want),
                                                              E.worst_ratio(oracle, want, tol, floor))
        if not worst <= 1.0:
            line += "  <-- worst entry %s, %d of %d above tolerance" % (
                np.unravel_index(int(np.argmax(rmap)), rmap.shape), int((rmap > 1).sum()), rmap.size)
            self.bad.append(line)
        print(line)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


# ---- the cases -------------------------------------------------------------------------------------
def _select(p, cap=None):
    def f(om_o, om_d, rng):
        if cap is None:
            return om_d.selectterms(p)
        t = om_d.selectterms(3 * p)
        t = t[t.max(1) <= cap][:p]
        assert len(t) == p
        return t
    return f


def _random(p, maxlev, max_nnz):
    return lambda om_o, om_d, rng: np.unique(random_terms(rng, p, om_o.d, maxlev, max_nnz), axis=0)


def _extreme_hyp(scale):
    import ob_oracle as O
    kinds = ["mat25", "mat25pow", "mat25"]
    hyp = np.concatenate([np.asarray(O.COV_INFO[k]["hyp0"], dtype=float) for k in kinds])
    hyp[0] = hyp[1] = O.COV_INFO["mat25"]["hyplb"][0] if scale is None else scale
    return hyp


MANY = ["mat25", "mat25pow", "mat25"]
# name: kinds, knots (count for knots_for, or the list), terms, level cap, hyp, domain ("star": k_star's)
CASES = {
    "star mat25x20 p4096": (["mat25"] * 20, 40, _select(4096, 12), None, None, "star"),
    "star mat25x20 p2500": (["mat25"] * 20, 40, _select(2500, 12), None, None, "star"),
    "star mat25powx8 p3000": (["mat25pow"] * 8, 40, _select(3000, 12), None, None, "star"),
    "star mixedx4 p3300": (["mat25", "mat25pow", "mat25ang"] * 4, 40, _select(3300, 12), None, None, "star"),
    "mat25x20 p9000": (["mat25"] * 20, 40, _select(9000), None, None, "star3"),
    "mat25x8 p520": (["mat25"] * 8, 30, _select(520), None, None, None),
    "mat25x8 p1100": (["mat25"] * 8, 30, _select(1100), None, None, None),
    "mat25x8 p2048": (["mat25"] * 8, 30, _select(2048), None, None, None),
    "mat25x8 p4096": (["mat25"] * 8, 30, _select(4096), None, None, None),
    "mixed d4 p700": (["mat25", "mat25pow", "mat25ang", "mat25"], 40, _select(700), None, None, None),
    "120 knots, knot loop": (MANY, [np.linspace(0.001, 0.976, 120)] * 3, _random(60, 119, 3), None, None, None),
    "120 knots, 3 levels, tables": (MANY, [np.linspace(0.001, 0.976, 120)] * 3, _random(60, 3, 3), 3, None, None),
    "40 knots, knot loop": (MANY, [np.linspace(0.001, 0.976, 40)] * 3, _random(60, 39, 3), None, None, None),
    "scale at lower bound": (MANY, 20, _select(40), None, "lb", None),
    "scale -3.3": (MANY, 20, _select(40), None, -3.3, None),
    "random d10 W6": (["mat25", "mat25pow", "mat25ang", "mat25", "mat25"] * 2, 16, _random(2500, 5, 6), None, None,
                      "foreign"),
}
PRODUCT_CASES = list(CASES)
for _p in (1, 127, 128, 129):       # test_gram_backends' smaller term sets of the same model
    CASES["mixed d4 p%d" % _p] = (["mat25", "mat25pow", "mat25ang", "mat25"], 40, _select(_p), None, None, None)

GRAD_CASES = {
    # test_gradhyp_with_more_hyperparameters_than_one_pass_holds: 16 knots, n = 300, p = 260
    "grad 18 mat25 + pow, ang, pow, ang": (["mat25"] * 18 + ["mat25pow", "mat25ang", "mat25pow", "mat25ang"], 16, 300, 260),
    "grad mat25x20": (["mat25"] * 20, 16, 300, 260),
    "grad mat25x16 + powx3": (["mat25"] * 16 + ["mat25pow"] * 3, 16, 300, 260),
    "grad powx3": (["mat25pow"] * 3, 16, 300, 260),
    "grad mat25x3": (["mat25"] * 3, 16, 300, 260),
    # test_gradhyp_products_match_oracle: 24 knots (the last two reach level 8 and beyond)
    "grad pow + mat25x7": (["mat25pow"] + ["mat25"] * 7, 24, 200, 100),
    "grad mat25, pow, ang": (["mat25", "mat25pow", "mat25ang"], 24, 333, 150),
    "grad mat25x5 p700": (["mat25"] * 5, 24, 1000, 700),
}
for _name, (_kinds, _m, _n, _p) in GRAD_CASES.items():
    CASES[_name] = (_kinds, _m, _select(_p), None, None, None)
SEED = {name: 1000 + i for i, name in enumerate(CASES)}


@functools.lru_cache(maxsize=None)
def model(name):
    import outerbase_amd as ob
    kinds, knots, terms_of, cap, hyp, domain = CASES[name]
    knots = knots_for(kinds, knots) if isinstance(knots, int) else knots
    if hyp is not None:
        hyp = _extreme_hyp(None if hyp == "lb" else hyp)
    om_o, om_d = make_pair(kinds, knots, hyp=hyp, share_rotation=True)
    # the float64 data both sides hold, taken as exact by the instrument
    rot, bv, ml = om_d.rotation()
    rotg, _ = om_d.rotation_grad()
    assert np.array_equal(rot, om_o.rotmat) and np.array_equal(rotg, om_o.rotmat_gradhyp)
    hyp_d = ob.gethyp(om_d)
    assert np.array_equal(hyp_d, om_o.hyp)
    terms = terms_of(om_o, om_d, np.random.default_rng(SEED[name]))
    if domain in ("star", "star3"):
        info = share_info(om_d, terms)
        assert info["nleft"] <= 192 and (9 <= info["nswf"] <= 16 if domain == "star" else info["nswf"] > 32)
    elif domain == "foreign":
        assert share_info(om_d, terms)["nleft"] > 192           # the star kernels step aside: k_*_tl
    levelcap = None if cap is None else np.full(len(kinds), cap, dtype=np.int64)
    return dict(name=name, kinds=kinds, knots=[np.asarray(k, dtype=np.float64) for k in knots], om_o=om_o, om_d=om_d,
                hyp=hyp_d, rot=rot, rotg=rotg, bv=bv, ml=ml, terms=terms, levelcap=levelcap, cap=cap)


PROBE_ROWS = 300


@functools.lru_cache(maxsize=3)
def rows(name, n, grad=False):
    """x, the long double B (and dB) with bounds, the oracle's float64 B (and dB) and the case's C"""
    import ob_oracle as O
    m = model(name)
    x = sample_x(np.random.default_rng(SEED[name] + 7 * n), n, m["kinds"])
    ref = E.ExtendedRef(m["kinds"], m["knots"], m["hyp"], m["rot"], x, m["rotg"] if grad else None)
    c = dict(x=x, ref=ref)
    c["B"], c["bB"] = ref.getmat(m["terms"])
    c["bo"] = O.OuterBase(m["om_o"], x, dograd=grad)
    c["Bo"] = O.ob_getmat(c["bo"], m["terms"])
    ratio = E.worst_ratio(c["Bo"], c["B"], c["bB"])
    if grad:
        c["dB"], c["bdB"] = ref.getmat_gradhyp(m["terms"])
        c["dBo"] = O.ob_getmat_gradhyp(c["bo"], m["terms"])
        ratio = max(ratio, E.worst_ratio(c["dBo"], c["dB"], c["bdB"]))
    c["ratio"] = ratio
    # C belongs to the case (model and term set), not to a handful of rows: the maximum over one
    # row or two is noise (down to 7e-17 on two entries), so few rows also take the case's 300-row sample
    probe = rows(name, PROBE_ROWS)["ratio"] if n < PROBE_ROWS // 2 else ratio
    c["C"] = E.constant_from_oracle_ratio(max(ratio, probe))
    print("%s | n = %d: oracle err/bound %.3g (on %d rows %.3g), C = %.3g" % (name, n, ratio, PROBE_ROWS, probe, c["C"]))
    return c


def vectors(name, n, p):
    rng = np.random.default_rng(SEED[name] + 13 * n + 1)
    a, v = rng.standard_normal(p), rng.standard_normal(n)
    return a, v, np.abs(a) + 0.1, -0.3


def compare_products(rep, m, c, got, a, v, cv, sig, label, floor=0.0):
    """the device results `got` (device_products) against the instrument; the oracle's figures beside
    them come from the oracle's float64 design matrix through the same float64 NumPy sums.  `floor`: an
    absolute term for the extreme length scales, where entries (and sooner their squares) underflow and
    a float64 result is no longer good to a relative error"""
    B, bB, Bo, C, ref = c["B"], c["bB"], c["Bo"], c["C"], c["ref"]
    ncol = None if m["cap"] is None else m["cap"] + 1
    bo = c["bo"]
    for k in range(len(m["kinds"])):
        R, bR = ref.getbase(k)
        rep.check("%s getbase(%d)" % (label, k + 1), got["getbase%d" % k][:, :ncol], R[:, :ncol], C * np.asarray(
            bR[:, :ncol], dtype=np.float64), bo.getbase(k + 1)[:, :ncol], floor)
    rep.check(label + " getmat", got["getmat"], B, C * np.asarray(bB, dtype=np.float64), Bo, floor)
    sq, aa = Bo * Bo, np.abs(a)
    want, tol = E.ref_matmul(B, bB, a, C)
    rep.check(label + " matmul", got["matmul"], want, tol, Bo @ a, floor)
    rep.check(label + " predict mean", got["predict_mean"], want, tol, Bo @ a, floor)
    rep.check(label + " predict mean (no variance)", got["predict_mean_only"], want, tol, Bo @ a, floor)
    want, tol = E.ref_tmatmul(B, bB, v, C)
    rep.check(label + " tmatmul", got["tmatmul"], want, tol, Bo.T @ v, floor)
    want, tol = E.ref_matmul(B, bB, aa, C, squared=True)
    rep.check(label + " sqmm", got["sqmm"], want, tol, sq @ aa, floor)
    want, tol = E.ref_tmatmul(B, bB, v, C, squared=True)
    rep.check(label + " sqtmm", got["sqtmm"], want, tol, sq.T @ v, floor)
    want, tol = E.ref_sqcolsums(B, bB, C)
    rep.check(label + " sqcolsums", got["sqcolsums"], want, tol, sq.sum(0), floor)
    want, tol = E.ref_predict_var(B, bB, cv, sig, C)
    rep.check(label + " predict var", got["predict_var"], want, tol, sq @ cv + math.exp(2 * sig), floor)


# the cases that also meet the generic (no LDS tile) kernels, through OBHIP_FORCE_GENERIC (read per call)
GENERIC_TOO = {"star mat25powx8 p3000", "mixed d4 p700", "random d10 W6", "120 knots, 3 levels, tables"}


@pytest.mark.parametrize("name", PRODUCT_CASES)
def test_products_against_extended_reference(name, monkeypatch):
    """getbase, getmat, B a, B^T v, (B o B) a, (B o B)^T v, sqcolsums and the fused predictor at n = 1
    and n = 300.  The term sets choose the kernel generation as in test_gpu_star.py: k_star on the
    downward-closed sets of nine star-waves and more, k_*_tl on the smaller and the random ones."""
    m = model(name)
    rep = Report(name)
    extreme = name.startswith("scale")
    for n in (1, 300):
        c = rows(name, n)
        a, v, cv, sig = vectors(name, n, len(m["terms"]))
        got = device_products(m["om_d"], m["terms"], c["x"], a, v, cv, sig, m["levelcap"])
        # (the absolute floor of test_extreme_length_scales_and_inputs_outside_the_domain)
        compare_products(rep, m, c, got, a, v, cv, sig, "n = %d" % n, floor=1e-290 if extreme else 0.0)
        if n == 300 and name in GENERIC_TOO:
            monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
            got = device_products(m["om_d"], m["terms"], c["x"], a, v, cv, sig, m["levelcap"])
            monkeypatch.delenv("OBHIP_FORCE_GENERIC")
            compare_products(rep, m, c, got, a, v, cv, sig, "n = %d generic" % n, floor=1e-290 if extreme else 0.0)
    rep.done()


@pytest.mark.parametrize("name", ["star mat25x20 p4096", "random d10 W6"])
def test_lane_row_kernels_against_extended_reference(name, tmp_path):
    """The first-generation lane = row kernels (k_mm, k_tmm, the lane = row predictor).  Their
    switches are read once per process, so a child process runs them."""
    m = model(name)
    n = 300
    c = rows(name, n)
    a, v, cv, sig = vectors(name, n, len(m["terms"]))
    st = np.concatenate([[0], np.cumsum([len(k) for k in m["knots"]])])
    np.savez(tmp_path / "in.npz", kinds=",".join(m["kinds"]), knotptst=st, knotpt=np.concatenate(m["knots"]),
             hyp=m["hyp"], rotmat=m["rot"], basisvar=m["bv"], maxlevel=m["ml"], terms=m["terms"], x=c["x"], a=a, v=v,
             cv=cv, sig=sig)
    env = dict(os.environ, OBHIP_MM_LANE_ROW="1", OBHIP_TMM_LANE_ROW="1", OBHIP_PREDICT_LANE_ROW="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "extended_products_worker.py")
    r = subprocess.run([sys.executable, worker, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(np.load(tmp_path / "out.npz"))
    rep = Report(name)
    compare_products(rep, m, c, got, a, v, cv, sig, "n = %d lane = row" % n)
    rep.done()


# ---- the Gram ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [
    ("mat25x8 p1100", 3000), ("mat25x8 p520", 700), ("mat25x8 p2048", 2500), ("mat25x8 p4096", 1500),   # packed diagonals
    ("mixed d4 p1", 2), ("mixed d4 p127", 65), ("mixed d4 p128", 200), ("mixed d4 p129", 1000), ("mixed d4 p700", 5000),
])
def test_gram_against_extended_reference(name, n, monkeypatch):
    """G = B^T B (loglik_std's hess() x e^{2 sigma}) of both Gram back ends and of both schedules of
    the diagonal tiles at the shapes of test_gram_diagonal_tiles_packed_four_into_three_blocks and
    test_gram_backends, on a column sample against ALL p columns: two seeded-random columns of every
    64-column block plus the 64 columns of largest mean bound, so every 64 x 64 quadrant of every
    128 x 128 tile has at least two sampled rows; the exact symmetry asserted here carries that to
    the transposed blocks.  The design matrix and its products at these rows ride along."""
    import outerbase_amd as ob
    from outerbase_amd import _lib
    m = model(name)
    terms, p = m["terms"], len(m["terms"])
    c = rows(name, n)
    rep = Report(name)
    a, v, cv, sig = vectors(name, n, p)
    compare_products(rep, m, c, device_products(m["om_d"], terms, c["x"], a, v, cv, sig), a, v, cv, sig, "n = %d" % n)
    cols = E.gram_column_sample(c["bB"], SEED[name])
    assert all(np.sum((cols >= c0) & (cols < c0 + 64)) >= min(2, p - c0) for c0 in range(0, p, 64))
    # n summands; the scale e^{-2 sigma} goes on on the device and comes off here: two exponentials
    # and two multiplications more
    want, tol = E.ref_gram(c["B"], c["bB"], cols, c["C"], extra=4)
    Go = c["Bo"][:, cols].T @ c["Bo"]
    # back end 3 generates its operand panels in the kernel: terms of at most 8 factors on at most 128
    # used basis columns (p = 2048 and 4096 of the packed-diagonal sets use 136 and 199: it refuses them)
    used = len({(l, t) for l in range(terms.shape[1]) for t in set(terms[:, l]) if t > 0})
    fused_takes = used <= 128 and int((terms > 0).sum(1).max()) <= 8
    assert fused_takes == (name not in ("mat25x8 p2048", "mat25x8 p4096"))
    try:
        for backend, diag4 in ((3, "1"), (4, "1"), (4, "0")):
            _lib.call("obhip_set_gram_backend", backend)
            monkeypatch.setenv("OBHIP_GRAM_DIAG4", diag4)
            lik = ob.loglik_std(m["om_d"], terms, v, c["x"])
            if backend == 3 and not fused_takes:
                with pytest.raises(ob.ObhipError, match="fused Gram kernel"):
                    lik.hess()
                continue
            G = lik.hess() * math.exp(2 * lik.para[0])
            assert np.array_equal(G, G.T)
            rep.check("n = %d Gram back end %d, DIAG4 = %s" % (n, backend, diag4), G[cols, :], want, tol, Go)
    finally:
        _lib.call("obhip_set_gram_backend", 0)
    rep.done()


# ---- hyper-parameter gradients -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_gradhyp_against_extended_reference(name, monkeypatch):
    """getmat_gradhyp, matmul_gradhyp, tmatmul_gradhyp and sqcolsums_gradhyp with the gradient basis
    from the interval tables and from the knot loop (OBHIP_GRAD_KNOTLOOP=1), every entry against its
    own bound: 26, 20, 22, 6 and 3 hyper-parameters (two 16-blocks; groups of four on the 4 x 4 x 4
    matrix instruction), and the shapes whose term sets reach level 8 and beyond."""
    import ob_oracle as O
    import outerbase_amd as ob
    m = model(name)
    n, p = GRAD_CASES[name][2:]
    terms = m["terms"]
    if name in ("grad mat25, pow, ang", "grad mat25x5 p700"):
        assert terms.max() >= 8
    c = rows(name, n, True)
    a, v, _, _ = vectors(name, n, p)
    C, bo = c["C"], c["bo"]
    rep = Report(name)
    for path in ("tables", "knot loop"):
        if path == "knot loop":
            monkeypatch.setenv("OBHIP_GRAD_KNOTLOOP", "1")
        bd = ob.outerbase(m["om_d"], c["x"])
        rep.check(path + " getmat_gradhyp", bd.getmat_gradhyp(terms), c["dB"], C * np.asarray(c["bdB"], dtype=np.float64),
                  c["dBo"])
        want, tol = E.ref_matmul_gradhyp(c["dB"], c["bdB"], a, C)
        rep.check(path + " matmul_gradhyp", bd.matmul_gradhyp(terms, a), want, tol, O.ob_mm_gradhyp(bo, terms, a)[1])
        want, tol = E.ref_tmatmul_gradhyp(c["dB"], c["bdB"], v, C)
        rep.check(path + " tmatmul_gradhyp", bd.tmatmul_gradhyp(terms, v), want, tol, O.ob_tmm_gradhyp(bo, terms, v)[1])
        want, tol = E.ref_sqcolsums_gradhyp(c["B"], c["bB"], c["dB"], c["bdB"], C)
        rep.check(path + " sqcolsums_gradhyp", bd.sqcolsums_gradhyp(terms), want, tol, O.ob_sqcolsums_gradhyp(bo, terms))
    rep.done()
