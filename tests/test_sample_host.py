"""Host-side checks of the posterior draws (no GPU): the long-double reference of tests/sample_ref.py against
50-digit arithmetic, the law of the draws without statistics (Z = I), the float64 restatement inside its
allowance on every case test_gpu_sample.py uses, six mistakes the instrument must see, the gap between the
best and the second-best candidate of every draw of every GPU case (on the reference alone), and the
library's host side -- symbols, Python names, the Makefile, no new switch, argument errors that return
before any device call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import extended_ref as E
import posterior_ref as P
import sample_ref as R
from test_sobol_host import d5_model, golden_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ld = np.longdouble
NAN = float("nan")
NEW = {"obhip_posterior_draw_dev": 6, "obhip_posterior_sample_dev": 8, "obhip_posterior_extremum_dev": 11}
CASES = R.SHAPES + [R.WIDE]
VARIANTS = ["twin", "skip winners", "nan", "all skipped"]


@functools.lru_cache(maxsize=None)
def model(name, p):
    if name == "wide":
        from test_gpu_predict_grad import wide
        kinds, om_o, om_d, terms, used, _ = wide()
        assert used == 198
        return om_o, om_d, np.ascontiguousarray(terms)
    mdl = {"d3": lambda: golden_model("mixed_d3"), "d8": lambda: golden_model("ref_basic_d8"), "d5": d5_model}[name]()
    terms = np.ascontiguousarray(mdl["om_o"].selectterms(p))
    assert len(terms) == p
    return mdl["om_o"], mdl["om_d"], terms


def twin_of(j):
    """where the copy of row j goes: the other workgroup of the fused kernel (rows 0-63 | 64-127)"""
    return 1 if j >= 64 else 100


@functools.lru_cache(maxsize=None)
def built(name, p, m, S, seed, variant=None):
    """case, C of the case and the reference's picks (minimum and maximum) -- computed once, shared by every
    test that needs it, the GPU file's included, and left unchanged"""
    om_o, om_d, terms = model(name, p)
    kw, drop, base = {}, (), None
    if variant is not None:
        base = built(name, p, m, S, seed)
        x = base["c"].x.copy()
        if variant == "twin":                       # the best row of draw 0 twice, bit for bit
            j = int(base["index"][0])
            x[twin_of(j)] = x[j]
            drop = (max(j, twin_of(j)),)
        elif variant == "skip winners":             # every draw's winner is skipped
            kw["skip"] = np.zeros(m, dtype=np.uint8)
            kw["skip"][np.unique(base["index"])] = 1
        elif variant == "nan":                      # the winner of draw 0 loses a coordinate
            x[int(base["index"][0]), 1] = NAN
        elif variant == "all skipped":
            kw["skip"] = np.ones(m, dtype=np.uint8)
        kw.update(x=x, theta=base["c"].theta, Z=base["c"].Z)
    c = R.seeded_case(om_o, terms, m, S, seed, **kw)
    Cc, r = R.constant_of(c)
    index, value = R.extremum(c.path, c.elig)
    imax, vmax = R.extremum(c.path, c.elig, maximize=True)
    return dict(c=c, C=Cc, r=r, om_d=om_d, terms=terms, index=index, value=value, index_max=imax, value_max=vmax,
                drop=drop, base=base)


def _mp(v):
    """a long double as an mpmath number, exactly"""
    import mpmath
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - ld(hi)))


def test_reference_against_fifty_digits():
    """Cholesky, back substitution and paths of the long-double reference against mpmath at 50 digits:
    p = 12, m = 7, S = 3, to 64 long-double roundoffs per summand and magnitude"""
    import mpmath
    mpmath.mp.dps = 50
    om_o, _, terms = model("d3", 12)
    c = R.seeded_case(om_o, terms, 7, 3, seed=5)
    p, S, m = c.p, c.S, c.m
    A = mpmath.matrix(p, p)
    for a in range(p):
        for b in range(p):
            A[a, b] = mpmath.mpf(float(c.H[a, b]))
    L = mpmath.cholesky(A)
    worst = 0.0
    for a in range(p):
        for b in range(a + 1):
            mag = sum(abs(L[a, k] * L[b, k]) for k in range(b + 1)) / abs(L[b, b])
            worst = max(worst, float(abs(_mp(c.L[a, b]) - L[a, b]) / (64 * E.EPS * (p + 1) * mag)))
    # Theta = theta + L^-T z by back substitution
    Th = mpmath.matrix(p, S)
    for s in range(S):
        for k in range(p - 1, -1, -1):
            acc = mpmath.mpf(float(c.Z[k, s]))
            for j in range(k + 1, p):
                acc -= L[j, k] * Th[j, s]
            Th[k, s] = acc / L[k, k]
    wt = 0.0
    for s in range(S):
        for k in range(p):
            want = mpmath.mpf(float(c.theta[k])) + Th[k, s]
            wt = max(wt, float(abs(_mp(c.Theta[k, s]) - want)) / (64 * E.EPS * c.bTheta[k, s]))
    wp = 0.0
    for i in range(m):
        for s in range(S):
            want = sum(_mp(c.B[i, k]) * (mpmath.mpf(float(c.theta[k])) + Th[k, s]) for k in range(p))
            wp = max(wp, float(abs(_mp(c.path[i, s]) - want)) / (64 * E.EPS * c.bpath[i, s]))
    print("sample | p=12 m=7 S=3 against 50 digits: err / (64 eps x bound) factor %.3g, draws %.3g, paths %.3g" % (worst, wt, wp))
    assert worst < 1 and wt < 1 and wp < 1


def test_identity_normals_give_the_posterior_covariance():
    """Z = I_p: (Theta - theta 1^T)(Theta - theta 1^T)^T = inv(H), against the long-double inverse: the law of the
    draws without statistics"""
    om_o, _, terms = model("d8", 67)
    p = len(terms)
    c = R.seeded_case(om_o, terms, 3, p, seed=7, Z=np.eye(p))
    Dm = c.Theta - np.asarray(c.theta, dtype=ld)[:, None]
    W = P.inverse_ld(c.L)
    want = W.T @ W
    assert np.all(np.tril(Dm, -1) == 0)                              # L^-T is upper triangular
    aX = np.abs(E._f64(Dm))
    tD = 2 * E.EPS * (np.abs(c.theta)[:, None] + aX)                 # theta added and taken off again
    r = E.worst_ratio(Dm @ Dm.T, want, 64 * E.EPS * p * (aX @ aX.T) + tD @ aX.T + aX @ tD.T)
    Hinv = np.linalg.inv(c.H)
    rel = float(np.max(np.abs(E._f64(want) - Hinv)) / np.max(np.abs(Hinv)))
    print("sample | Z = I at p=%d: D D^T against W^T W err / allowance %.3g; against LAPACK's inverse %.3g relative" % (p, r, rel))
    assert r < 1 and rel < 1e-10


@pytest.mark.parametrize("name,p,m,S,seed", CASES)
def test_float64_restatement_stays_inside_its_allowance(name, p, m, S, seed):
    b = built(name, p, m, S, seed)
    c = b["c"]
    Theta, path = R.host64(c)
    w = R.ratios(c, Theta, path, b["C"])
    print("sample | %s p=%d m=%d S=%d: float64 restatement err / bound %.3g (C = %.3g, cap %.3g), err / tolerance %s; "
          "%d distinct picks" % (name, c.p, m, S, b["r"], b["C"], E.C_CAP, ", ".join("%s %.3g" % kv for kv in w.items()),
                                 len(np.unique(b["index"]))))
    assert 8 * b["r"] < E.C_CAP, "the constant is capped: the bound does not describe this case"
    assert max(w.values()) < 1
    i64, v64 = R.extremum(path, c.elig)
    assert np.array_equal(i64, b["index"]) and R.value_ratio(c, i64, v64, b["C"]) < 1


def test_the_instrument_sees_six_mistakes():
    b = built(*R.SEMANTICS)
    c, Cc = b["c"], b["C"]
    good = R.ratios(c, *R.host64(c), C=Cc)
    assert max(good.values()) < 1
    # L^-1 for L^-T: draws of the right marginal size with the wrong covariance
    lin = R.ratios(c, *R.host64(c, "inverse not transposed"), C=Cc)
    nth = R.ratios(c, *R.host64(c, "theta dropped"), C=Cc)
    print("sample | L^-1 for L^-T: %s; theta dropped: %s" % (lin, nth))
    assert lin["theta"] > 1000 and lin["path"] > 1000
    assert nth["theta"] > 1000 and nth["path"] > 1000
    # maximize ignored: other picks
    imx, _ = R.extremum(c.path, c.elig, maximize=True, mutate="maximize ignored")
    assert np.array_equal(imx, b["index"]) and not np.any(imx == b["index_max"])
    # the highest index on a tie
    t = built(*R.SEMANTICS, "twin")
    lo, hi = sorted([int(b["index"][0]), twin_of(int(b["index"][0]))])
    assert t["index"][0] == lo
    ihi, _ = R.extremum(t["c"].path, t["c"].elig, mutate="highest index on a tie")
    assert ihi[0] == hi and ihi[0] != t["index"][0]
    # skip ignored: the skipped winners come back
    s = built(*R.SEMANTICS, "skip winners")
    assert not set(s["index"]) & set(b["index"])
    ign, _ = R.extremum(s["c"].path, s["c"].finite, mutate="skip ignored")
    assert np.array_equal(ign, b["index"]) and not np.array_equal(ign, s["index"])
    # a NaN row winning
    n = built(*R.SEMANTICS, "nan")
    j = int(b["index"][0])
    assert n["index"][0] != j and j not in n["index"]
    keep = b["index"] != j
    assert np.array_equal(n["index"][keep], b["index"][keep])           # the others unchanged
    path = E._f64(n["c"].path).copy()
    path[j] = NAN                                                        # what the device has in that row
    won, _ = R.extremum(path, np.ones(c.m, dtype=bool), mutate="nan wins")
    assert np.all(won == j)
    ok, _ = R.extremum(path, np.ones(c.m, dtype=bool))
    assert np.array_equal(ok, n["index"])
    # nothing eligible
    a = built(*R.SEMANTICS, "all skipped")
    assert np.all(a["index"] == -1) and np.all(np.isnan(E._f64(a["value"])))


def _gaps(b, label):
    for mx in (False, True):
        gap = R.gap_ratio(b["c"], b["C"], maximize=mx, drop=b["drop"])
        print("sample | %s %s: smallest gap / allowance %.3g" % (label, "max" if mx else "min", gap))
        assert gap > 1000, "the seeded case does not separate the best two candidates: choose another seed"


@pytest.mark.parametrize("name,p,m,S,seed", CASES + [R.SEMANTICS])
def test_best_and_second_best_are_a_thousand_allowances_apart(name, p, m, S, seed):
    """a condition of the case, on the reference alone: only then are the picks determined"""
    b = built(name, p, m, S, seed)
    _gaps(b, "%s p=%d m=%d S=%d" % (name, b["c"].p, m, S))


@pytest.mark.parametrize("variant", VARIANTS[:3])
def test_the_semantics_cases_are_separated_too(variant):
    """the deliberate twins are exempt: the copy is left out of the comparison"""
    _gaps(built(*R.SEMANTICS, variant), variant)


# ---- the library's host side ---------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name, nargs in NEW.items():
        assert name in protos, name
        assert len(protos[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names_makefile_and_no_new_switch():
    import outerbase_amd as ob
    assert "ThompsonResult" in ob.__all__ and hasattr(ob, "ThompsonResult")
    for meth in ("draw", "sample", "thompson"):
        assert callable(getattr(ob.Posterior, meth))
        doc = " ".join(getattr(ob.Posterior, meth).__doc__.split())
        assert "same torch build" in doc and "portable" in doc
    csrc = os.path.join(ROOT, "outerbase_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kernels_sample.hip" in mk and "sample.cpp" in mk
    read = set()
    for f in ("kernels_sample.hip", "sample.cpp", "posterior.cpp"):
        read |= set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', open(os.path.join(csrc, f)).read()))
    assert read <= {"OBHIP_FORCE_GENERIC"}
    # kernel boundaries only: nothing cooperative, no atomics, no random number generator
    for f in ("kernels_sample.hip", "sample.cpp"):
        src = open(os.path.join(csrc, f)).read()
        code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
        assert "atomic" not in code and "Cooperative" not in code and "grid_group" not in code
        assert "rand" not in code.lower().replace("operand", "")


def test_argument_errors_return_before_any_device_call():
    """with no handle at all: what does not need the handle is refused first, each with its own message.
    (ldz < p needs a handle's p: test_gpu_sample.py refuses it there.)"""
    from outerbase_amd._lib import lib
    buf = (C.c_double * 64)()
    a = C.cast(buf, C.c_void_p)
    err = lib.obhip_last_error
    draw, sample, ext = lib.obhip_posterior_draw_dev, lib.obhip_posterior_sample_dev, lib.obhip_posterior_extremum_dev
    assert draw(None, a, a, 8, 0, a) == 1 and b"S = 0" in err()
    assert draw(None, a, None, 8, 2, a) == 1 and b"d_z" in err()
    assert draw(None, None, a, 8, 2, a) == 1 and b"d_theta" in err()
    assert draw(None, a, a, 8, 2, None) == 1 and b"d_Theta" in err()
    assert draw(None, a, a, 8, 2, a) == 1 and b"null posterior" in err()
    assert sample(None, a, a, 8, 0, a, 4, a) == 1 and b"S = 0" in err()
    assert sample(None, a, None, 8, 2, a, 4, a) == 1 and b"d_z" in err()
    assert sample(None, a, a, 8, 2, a, 4, None) == 1 and b"d_path" in err()
    assert sample(None, a, a, 8, 2, None, 4, a) == 1 and b"d_x" in err()
    assert sample(None, a, a, 8, 2, None, 0, None) == 1 and b"null posterior" in err()      # n = 0 needs neither
    assert ext(None, a, a, 8, 0, a, 4, None, 0, a, a) == 1 and b"S = 0" in err()
    assert ext(None, a, a, 8, 2, a, 0, None, 0, a, a) == 1 and b"m = 0" in err()
    assert ext(None, a, None, 8, 2, a, 4, None, 0, a, a) == 1 and b"d_z" in err()
    assert ext(None, a, a, 8, 2, None, 4, None, 0, a, a) == 1 and b"d_xcand" in err()
    assert ext(None, a, a, 8, 2, a, 4, None, 0, None, a) == 1 and b"outputs" in err()
    assert ext(None, a, a, 8, 2, a, 4, None, 1, a, None) == 1 and b"outputs" in err()
    assert ext(None, a, a, 8, 2, a, 4, None, 0, a, a) == 1 and b"null posterior" in err()
    assert all(v == 0.0 for v in buf)                                                        # nothing was written


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    p = len(terms)
    post = ob.Posterior(om, ob.obmod._terms_of(om, terms), C.c_void_p(1))               # never reaches the library
    try:
        x, th = np.full((5, 3), 0.5), np.zeros(p)
        for bad in (dict(), dict(n_draws=3, z=np.zeros((p, 3))), dict(z=np.zeros((p + 1, 3))), dict(z=np.zeros(p)),
                    dict(n_draws=0, seed=1), dict(n_draws=3)):
            with pytest.raises(ValueError):
                post.draw(th, **bad)
        with pytest.raises(ValueError):
            post.draw(np.zeros(p + 1), n_draws=2, seed=1)
        with pytest.raises(ValueError):
            post.sample(x[:, :2], th, n_draws=2, seed=1)
        with pytest.raises(ValueError):
            post.thompson(x[:0], th, n_draws=2, seed=1)
        with pytest.raises(ValueError):
            post.thompson(x, th, n_draws=2, seed=1, skip=np.zeros(4))
        post.meansd = np.array([[0.0, 0.0, 9.0]])
        with pytest.raises(ValueError):
            post.thompson(x, th, n_draws=2, seed=1, response=0)                         # a scale <= 0
        with pytest.raises(ValueError):
            post.sample(x, th, n_draws=2, seed=1, response=0)
    finally:
        post._h = None
