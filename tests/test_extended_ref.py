"""The extended-precision instrument of tests/extended_ref.py itself (no GPU): right against 50-digit
arithmetic, the float64 oracle sits at a few eps64 of its per-entry bound at every case (the
evidence that the oracle's 1e-6 .. 1e-8 max-norm errors at high levels are conditioning, lost on
any float64 side), and it catches perturbations of 1e-9 and 1e-11 that the flat max-norm
tolerances of the older parity tests let through."""
import functools

import numpy as np
import pytest

import extended_ref as E
from conftest import knots_for, sample_x

ld = np.longdouble


def oracle_model(kinds, knots):
    import ob_oracle as O
    om = O.OuterMod()
    om.setcovfs(kinds)
    om.setknot(knots)
    return om


def reference_of(om, x, grad=False):
    knots = [om.knots_of(k) for k in range(om.d)]
    return E.ExtendedRef(om.kinds, knots, om.hyp, om.rotmat, x, om.rotmat_gradhyp if grad else None)


CASES = {
    # name: (kinds, knots per dimension, terms, level cap, rows, gradient cube too)
    "mat25x8 p4096": (["mat25"] * 8, 30, 4096, None, 300, False),
    "mat25powx8 p3000": (["mat25pow"] * 8, 40, 3000, 12, 300, False),
    "mat25x20 p4096": (["mat25"] * 20, 40, 4096, None, 300, False),
    "mat25x16+powx3 p260": (["mat25"] * 16 + ["mat25pow"] * 3, 16, 260, None, 200, True),
    "mat25x18+pow,ang,pow,ang p260": (["mat25"] * 18 + ["mat25pow", "mat25ang", "mat25pow", "mat25ang"],
                                      16, 260, None, 200, True),
    "mixed d4 p700": (["mat25", "mat25pow", "mat25ang", "mat25"], 40, 700, None, 200, True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """oracle and extended-precision B (and dB) of one case, built once per session"""
    import ob_oracle as O
    kinds, m, p, cap, n, grad = CASES[name]
    om = oracle_model(kinds, knots_for(kinds, m))
    if cap is None:
        terms = om.selectterms(p)
    else:
        terms = om.selectterms(3 * p)
        terms = terms[terms.max(1) <= cap][:p]
    assert len(terms) == p
    x = sample_x(np.random.default_rng(p + n), n, kinds)
    ref = reference_of(om, x, grad)
    c = dict(om=om, terms=terms, x=x, ref=ref)
    c["B"], c["bB"] = ref.getmat(terms)
    bo = O.OuterBase(om, x, dograd=grad)
    c["Bo"] = O.ob_getmat(bo, terms)
    c["ratio"] = E.worst_ratio(c["Bo"], c["B"], c["bB"])
    if grad:
        c["dB"], c["bdB"] = ref.getmat_gradhyp(terms)
        c["dBo"] = O.ob_getmat_gradhyp(bo, terms)
        c["ratio_grad"] = E.worst_ratio(c["dBo"], c["dB"], c["bdB"])
    return c


def test_long_double_is_an_extended_format():
    assert E.EPS < 2e-19, E.PRECISION_MESSAGE
    E.require_extended()


# ---- against 50-digit arithmetic --------------------------------------------------------------
def _mp_of(v):
    """exact mpmath value of a long double (its float64 head and tail)"""
    import mpmath
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - ld(hi)))


def _mp_cov(kind, xv, kn, hyp):
    """(K_j, [dK_j / d hyp_h]) over the knots, mpmath, the same formulas written out again"""
    import mpmath as mp
    xv, hyp = mp.mpf(float(xv)), [mp.mpf(float(h)) for h in hyp]
    K, dK = [], [[] for _ in hyp]
    for kj in kn:
        kj = mp.mpf(float(kj))
        if kind == "mat25ang":
            hs = (mp.sin(xv) - mp.sin(kj)) / mp.exp(2 * hyp[0])
            hc = (mp.cos(xv) - mp.cos(kj)) / mp.exp(2 * hyp[1])
            h = mp.sqrt(hs * hs + hc * hc)
            K.append((1 + h + h * h / 3) * mp.exp(-h))
            w = mp.exp(-h) * (h + 1)
            dK[0].append(mp.mpf(2) / 3 * hs * hs * w)
            dK[1].append(mp.mpf(2) / 3 * hc * hc * w)
            continue
        if kind == "mat25":
            els = mp.exp(2 * hyp[0])
            t1, t2 = xv / els, kj / els
        else:
            powv = mp.exp(hyp[1] / 4)
            els = mp.exp(2 * hyp[0] + hyp[1] / 4)
            t1, t2 = mp.power(xv, powv) / els, mp.power(kj, powv) / els
        h = t1 - t2
        ah = abs(h)
        K.append((1 + ah + ah * ah / 3) * mp.exp(-ah))
        h2 = h * (1 + ah) * mp.exp(-ah)
        dK[0].append(mp.mpf(2) / 3 * h * h2)
        if kind == "mat25pow":
            g1 = mp.log(xv) * t1 - mp.log(kj) * t2
            dK[1].append(-g1 * powv / 12 * h2 + h * h2 / 12)
    return K, dK


def _mp_entry(om, x, term, i, h=None):
    """B[i, term] (h None) or dB[i, term, h] in mpmath"""
    import mpmath as mp
    out = mp.mpf(1)
    for k in range(om.d):
        kn = om.knots_of(k)
        m, o = len(kn), int(om.knotptst[k])
        rot = om.rotmat[:m, o:o + m]
        K, dK = _mp_cov(om.kinds[k], x[i, k], kn, om.hyp_of(k))

        def col(vals, mat, c):
            return mp.fsum(vals[j] * mp.mpf(float(mat[j, c])) for j in range(m))
        R0 = col(K, rot, 0)
        c = int(term[k])
        if h is not None and om.hypmatch[h] == k:
            rotg = om.rotmat_gradhyp[:m, om.gest[h]:om.gest[h + 1]]
            out *= col(dK[h - int(om.hypst[k])], rot, c) + col(K, rotg, c)      # R0 . (T / R0)
        else:
            out *= R0 * (col(K, rot, c) / R0 if c > 0 else 1)
    return out


def test_instrument_against_50_digit_arithmetic():
    mpmath = pytest.importorskip("mpmath")
    c = case("mixed d4 p700")
    om, x, terms = c["om"], c["x"], c["terms"]
    rng = np.random.default_rng(50)
    n, p = c["B"].shape
    picks = [(int(i), int(t), None) for i, t in zip(rng.integers(0, n, 14), rng.integers(0, p, 14))]
    flat = np.argsort(-np.asarray(c["bB"], dtype=np.float64), axis=None)[:6]          # the largest bounds
    picks += [(int(f // p), int(f % p), None) for f in flat]
    nh = c["dB"].shape[2]
    picks += [(int(i), int(t), int(h)) for i, t, h in
              zip(rng.integers(0, n, 14), rng.integers(0, p, 14), rng.integers(0, nh, 14))]
    flat = np.argsort(-np.asarray(c["bdB"], dtype=np.float64), axis=None)[:6]
    picks += [(int(f // (p * nh)), int(f // nh % p), int(f % nh)) for f in flat]
    assert len(picks) == 40
    worst = 0.0
    with mpmath.workdps(50):
        for i, t, h in picks:
            want = _mp_entry(om, x, terms[t], i, h)
            got, bound = (c["B"][i, t], c["bB"][i, t]) if h is None else (c["dB"][i, t, h], c["bdB"][i, t, h])
            err = float(abs(_mp_of(got) - want))
            worst = max(worst, err / (E.EPS * float(bound)))
            assert err <= 64 * E.EPS * float(bound), (i, t, h, err, float(bound))
    print("long double against 50 digits: worst error %.3g eps_longdouble x bound" % worst)


@pytest.mark.parametrize("kind", ["mat25", "mat25pow", "mat25ang"])
def test_gradient_product_references_against_50_digit_arithmetic(kind):
    """ref_sqtmm_gradhyp (signed v), ref_sqmm_gradhyp, ref_matmul_gradhyp_dot and ref_residvar_gradhyp on a
    case small enough to sum every entry in 50 digits: the long double value, the sum of |summands| under
    gamma_k and the propagated bound under C are each what their docstrings say."""
    mp = pytest.importorskip("mpmath")
    kinds = [kind, "mat25", kind]
    om = oracle_model(kinds, knots_for(kinds, 8))
    n, terms = 3, np.array([[0, 0, 0], [1, 0, 0], [2, 1, 0], [0, 3, 2], [1, 2, 3]])
    p, nh = len(terms), len(om.hypmatch)
    rng = np.random.default_rng(len(kind))
    x = sample_x(rng, n, kinds)
    a, v = rng.standard_normal(p), rng.standard_normal(n)
    assert (a < 0).any() and (a > 0).any() and (v < 0).any() and (v > 0).any()
    ref = reference_of(om, x, grad=True)
    B, bB = ref.getmat(terms)
    dB, bdB = ref.getmat_gradhyp(terms)
    varc, bvarc = E.term_var(om.basisvar, om.knotptst, terms)
    lv = om.getlvar_gradhyp(terms)
    f = lambda q: mp.mpf(float(q))
    with mp.workdps(50):
        Bm = [[_mp_entry(om, x, terms[t], i) for t in range(p)] for i in range(n)]
        dBm = [[[_mp_entry(om, x, terms[t], i, h) for h in range(nh)] for t in range(p)] for i in range(n)]
        vm = [mp.exp(mp.fsum(f(om.basisvar[om.knotptst[l] + terms[t, l]]) for l in range(om.d))) for t in range(p)]
        R, T = range(n), range(p)
        # per product: entries -> (summands, their propagated bounds, k)
        sq = lambda i, t, h: (2 * Bm[i][t] * dBm[i][t][h],
                              2 * (f(bB[i, t]) * abs(dBm[i][t][h]) + abs(Bm[i][t]) * f(bdB[i, t, h])))
        res = lambda i, t, h: [(-vm[t] * sq(i, t, h)[0], vm[t] * sq(i, t, h)[1]),         # two summands per term
                               (-vm[t] * Bm[i][t] ** 2 * f(lv[t, h]), vm[t] * 2 * abs(Bm[i][t]) * f(bB[i, t]) * abs(f(lv[t, h])))]
        products = {
            "sqtmm": (E.ref_sqtmm_gradhyp, (B, bB, dB, bdB, v), (p, nh), n,
                      lambda t, h: [(f(v[i]) * sq(i, t, h)[0], abs(f(v[i])) * sq(i, t, h)[1]) for i in R]),
            "sqmm": (E.ref_sqmm_gradhyp, (B, bB, dB, bdB, a), (n, nh), p,
                     lambda i, h: [(f(a[t]) * sq(i, t, h)[0], abs(f(a[t])) * sq(i, t, h)[1]) for t in T]),
            "dot": (E.ref_matmul_gradhyp_dot, (dB, bdB, a, v), (nh,), n * p,
                    lambda h: [(f(v[i]) * f(a[t]) * dBm[i][t][h], abs(f(v[i]) * f(a[t])) * f(bdB[i, t, h]))
                               for i in R for t in T]),
            "residvar": (E.ref_residvar_gradhyp, (B, bB, dB, bdB, varc, bvarc, lv), (n, nh), 2 * p + 4,
                         lambda i, h: [q for t in T for q in res(i, t, h)]),
        }
        for name, (fn, args, shape, k, summands) in products.items():
            want, tol0 = fn(*args, 0.0)
            tol1 = fn(*args, 1.0)[1]
            assert want.shape == tol0.shape == shape, name
            worst = 0.0
            for idx in np.ndindex(*shape):
                s = summands(*idx)
                exact, absum, bound = mp.fsum(q[0] for q in s), mp.fsum(abs(q[0]) for q in s), mp.fsum(q[1] for q in s)
                scale = float(absum + bound)
                err = float(abs(_mp_of(want[idx]) - exact))
                worst = max(worst, err / (E.EPS * scale))
                assert err <= 64 * E.EPS * scale, (name, idx, err, scale)
                # C x (propagated bound) and gamma_k x (sum of |summands|), each to float64 rounding; residvar's
                # term for the float64 exponential of varc (not under C) comes on top of the latter
                # (to 1e-6: |summands| are taken of the long double entries, right to eps_longdouble x their bounds)
                assert abs(float(tol1[idx] - tol0[idx]) - float(bound)) <= 1e-6 * float(bound), (name, idx)
                g = E.gamma(k) * float(absum)
                top = float(np.max(bvarc / np.asarray(varc, dtype=np.float64))) * float(absum) if name == "residvar" else 0.0
                assert g * (1 - 1e-6) <= tol0[idx] <= (g + top) * (1 + 1e-6), (name, idx)
            print("%s %s: long double against 50 digits, worst %.3g eps_longdouble x (sum |summands| + bound)"
                  % (kind, name, worst))
        for t in range(p):       # term_var: the value, and its bound covers a float64 evaluation
            assert abs(_mp_of(varc[t]) - vm[t]) <= 8 * E.EPS * float(vm[t])
            v64 = np.exp(np.sum(om.basisvar[om.knotptst[:-1] + terms[t]]))
            assert abs(mp.mpf(float(v64)) - vm[t]) <= float(bvarc[t]) and bvarc[t] <= 1e-13 * float(vm[t])


# ---- the float64 oracle against the instrument ------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_sits_at_a_few_eps_of_the_per_entry_bound(name):
    c = case(name)
    line = "%s: oracle B max-norm %.3g, err/bound %.3g" % (name, E.maxnorm_relerr(c["Bo"], c["B"]), c["ratio"])
    assert c["ratio"] < 2e-15, line
    if "dB" in c:
        line += "; dB max-norm %.3g, err/bound %.3g" % (E.maxnorm_relerr(c["dBo"], c["dB"]), c["ratio_grad"])
        assert c["ratio_grad"] < 2e-15, line
    print(line)


def test_oracle_gram_sits_at_a_few_eps_of_its_bound():
    """the seventh row of the table: B^T B of the oracle's float64 B on the sampled columns"""
    c = case("mat25x8 p4096")
    cols = E.gram_column_sample(c["bB"], 4096)
    assert len(cols) >= 2 * 64 and all(np.sum((cols >= c0) & (cols < c0 + 64)) >= 2 for c0 in range(0, 4096, 64))
    want, _ = E.ref_gram(c["B"], c["bB"], cols, 0.0)
    G = c["Bo"][:, cols].T @ c["Bo"]
    ratio = E.worst_ratio(G, want, E.gram_bound(c["B"], c["bB"], cols))     # the bound alone, no summation term
    print("oracle Gram: max-norm %.3g, err/bound %.3g" % (E.maxnorm_relerr(G, want), ratio))
    assert ratio < 2e-15


# ---- it catches what the flat tolerance lets through -----------------------------------------
def test_mutated_column_passes_the_flat_tolerance_and_fails_the_per_entry_one():
    c = case("mat25x8 p4096")
    C = E.constant_from_oracle_ratio(c["ratio"])
    assert C < 1e-14
    tol = C * np.asarray(c["bB"], dtype=np.float64)
    assert E.worst_ratio(c["Bo"], c["B"], tol) <= 0.125 + 1e-12      # (C is eight times its ratio)
    col = int(np.nonzero((c["terms"].sum(1) == 1) & (c["terms"].max(1) == 1))[0][0])   # a level-1 column
    for eps, all_rows in ((1e-9, True), (1e-11, False)):
        Bm = c["Bo"].copy()
        Bm[:, col] *= 1 + eps
        assert E.maxnorm_relerr(Bm, c["B"]) < 1e-6                   # the old criterion: passes
        r = E.ratio_map(Bm, c["B"], tol)[:, col]
        print("column %d x (1 + %g): %.3g x tolerance, %d of %d rows fail" % (col, eps, r.max(), (r > 1).sum(), len(r)))
        assert r.max() > 1                                           # the new one: fails
        if all_rows:
            assert np.all(r > 1)


def test_mutated_gram_block_passes_the_flat_tolerance_and_fails_the_per_entry_one():
    c = case("mat25x8 p4096")
    C = E.constant_from_oracle_ratio(c["ratio"])
    cols = E.gram_column_sample(c["bB"], 4096)
    want, tol = E.ref_gram(c["B"], c["bB"], cols, C)
    G = c["Bo"][:, cols].T @ c["Bo"]
    clean = E.worst_ratio(G, want, tol)
    assert clean < 1
    rows = np.nonzero(cols < 64)[0]
    assert len(rows) >= 2
    Gm = G.copy()
    Gm[np.ix_(rows, np.arange(64, 128))] *= 1 + 1e-9                 # block (0-63) x (64-127) of G
    assert E.maxnorm_relerr(Gm, want) < 1e-6
    r = E.ratio_map(Gm, want, tol)[np.ix_(rows, np.arange(64, 128))]
    print("unmutated Gram %.3g x tolerance; block x (1 + 1e-9): %.3g x tolerance, %d of %d sampled entries fail"
          % (clean, r.max(), (r > 1).sum(), r.size))
    assert r.max() > 1 and (r > 1).sum() > r.size // 2


def test_mutated_gradient_slice_passes_the_flat_tolerance_and_fails_the_per_entry_one():
    c = case("mixed d4 p700")
    C = E.constant_from_oracle_ratio(max(c["ratio"], c["ratio_grad"]))
    tol = C * np.asarray(c["bdB"], dtype=np.float64)
    assert E.worst_ratio(c["dBo"], c["dB"], tol) < 1
    dm = c["dBo"].copy()
    dm[:, :, 1] *= 1 + 1e-9
    assert E.maxnorm_relerr(dm, c["dB"]) < 2e-7
    r = E.ratio_map(dm, c["dB"], tol)[:, :, 1]
    print("gradient slice x (1 + 1e-9): %.3g x tolerance, %d of %d entries fail" % (r.max(), (r > 1).sum(), r.size))
    assert r.max() > 1


# ---- shape edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7])
def test_shape_edges_of_the_helper(n):
    import ob_oracle as O
    kinds = ["mat25", "mat25pow", "mat25ang", "mat25", "mat25pow", "mat25ang", "mat25"]
    om = oracle_model(kinds, knots_for(kinds, 16))
    x = sample_x(np.random.default_rng(n), n, kinds)
    assert np.all((x[:, [2, 5]] >= 0) & (x[:, [2, 5]] < 2 * np.pi))   # mat25ang: [0, 2 pi)
    ref = reference_of(om, x, grad=True)
    bo = O.OuterBase(om, x, dograd=True)
    constant = np.zeros((1, 7), dtype=np.int64)
    one = np.array([[0, 0, 3, 0, 0, 0, 0]])
    six = np.array([[1, 2, 3, 0, 2, 1, 4]])
    for terms in (constant, one, six, np.vstack([constant, one, six])):
        B, bB = ref.getmat(terms)
        dB, bdB = ref.getmat_gradhyp(terms)
        assert B.shape == bB.shape == (n, len(terms)) and dB.shape == bdB.shape == (n, len(terms), 11)
        assert np.all(bB > 0) and np.all(bdB > 0)
        assert E.worst_ratio(O.ob_getmat(bo, terms), B, bB) < 2e-15
        assert E.worst_ratio(O.ob_getmat_gradhyp(bo, terms), dB, bdB) < 2e-15
        a, v = np.arange(1.0, len(terms) + 1), np.arange(1.0, n + 1)
        for want, tol in (E.ref_matmul(B, bB, a, 1e-15), E.ref_predict_var(B, bB, a, -0.3, 1e-15)):
            assert want.shape == tol.shape == (n,)
        for want, tol in (E.ref_tmatmul(B, bB, v, 1e-15), E.ref_sqcolsums(B, bB, 1e-15)):
            assert want.shape == tol.shape == (len(terms),)
        assert E.ref_matmul_gradhyp(dB, bdB, a, 1e-15)[0].shape == (n, 11)
        assert E.ref_tmatmul_gradhyp(dB, bdB, v, 1e-15)[0].shape == (len(terms), 11)
        assert E.ref_sqcolsums_gradhyp(B, bB, dB, bdB, 1e-15)[1].shape == (len(terms), 11)
    # the constant term is the product of the scale factors alone
    assert np.array_equal(ref.getmat(constant)[0][:, 0], functools.reduce(lambda u, w: u * w, ref.s))
