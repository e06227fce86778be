"""Observed input gradients as rows of the Newton fit on the GPU (obhip_design_dx_dev,
obhip_normal_acc_add_grad_dev, NewtonAccumulator.add_grad, fit_newton_grad) against the extended-precision
references of tests/extended_dx_ref.py and tests/grad_obs_ref.py.

Where the bounds come from (none is this file's own):
  staged entries  C . bound per entry, C eight times the float64 restatement's own err / bound on the same case (at
                  most 2e-13): test_gpu_predict_grad.py's rule; the bound of sqrt(w) D is sqrt(w) times D's.
  state           test_gpu_stream.py's statistics rule on the rows that were staged: C x (propagated bound) +
                  gamma_k x sum |summands|, the additions of batch and chunk sums through `extra`; the right-hand
                  sides by the plain rule of ref_tmatmul.
  fits            1e-6 relative for coefficients and predictions, 1e-10 for diagH: what test_gpu_stream.py and
                  test_gpu_multi_response.py grant the one-shot fit; backward error against the reference's H and
                  right-hand side within max(4 eta of the reference's own float64 solve, p 2^-53),
                  test_multi_solve_backward_error's rule with the float64 LAPACK solve as the yardstick.
Every test prints its figures before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_dx_ref as X
import extended_ref as E
import grad_obs_ref as R
from conftest import sample_x
from multi_schedule_worker import backward_errors
from test_gpu_predict_grad import NS, case, model
from test_predict_grad_host import special_rows

pytestmark = pytest.mark.gpu

ld = np.longdouble
U = 2.0 ** -53
NAN = float("nan")


# ---- 1. the staged entries ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dref(name, p, kind):
    """(dB / dx_l, bound) for every l on the model's 129 rows, once per case"""
    m, c = model(name), case(name, p, kind)
    out = [m["ref"].getmat_dx(c["terms"], l) for l in range(len(m["kinds"]))]
    for D, b in out:
        D.setflags(write=False), b.setflags(write=False)
    return out


def design_dev(om, terms, x, dims, weights, ldo):
    """obhip_design_dx_dev into a NaN-filled (L, n, ldo) buffer"""
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call
    t = ob.obmod._terms_of(om, terms)
    n, L = x.shape[0], len(dims)
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    out = torch.full((L, n, ldo), NAN, dtype=torch.float64, device="cuda")
    dims = np.ascontiguousarray(dims, dtype=np.uint32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    call("obhip_design_dx_dev", om._h, t._h, dx.data_ptr(), n, dims.ctypes.data, L, None if w is None else w.ctypes.data,
         out.data_ptr(), ldo)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_design(name, p, kind, label):
    import outerbase_amd as ob
    m, c = model(name), case(name, p, kind)
    terms, d = c["terms"], len(m["kinds"])
    pp = len(terms)
    refs = dref(name, p, kind)
    rng = np.random.default_rng(pp + d)
    lines, worst = [], 0.0

    def compare(got, n, dims, weights, what):
        nonlocal worst
        sq = np.ones(len(dims)) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64))
        w = 0.0
        for j, l in enumerate(dims):
            D, b = refs[l]
            assert np.all(np.isfinite(got[j]))
            w = max(w, E.worst_ratio(got[j], ld(sq[j]) * D[:n], c["C"] * sq[j] * E._f64(b[:n])))
        lines.append("%s %s p=%d n=%d %s: err/tolerance %.3g" % (label, name, pp, n, what, w))
        worst = max(worst, w)

    for n in NS:
        x = m["x"][:n]
        # every dimension, non-unit weights, a pitch above p: nothing but [0, n) x [0, p) of each block is written
        weights = rng.uniform(0.2, 3.0, d)
        got = design_dev(m["om_d"], terms, x, np.arange(d), weights, pp + 3)
        assert np.all(np.isnan(got[:, :, pp:])), "written beyond column p"
        compare(got[:, :, :pp], n, list(range(d)), weights, "all dimensions, ldo = p + 3")
    n = NS[-1]
    x = m["x"][:n]
    single = [d - 1]
    compare(ob.design_dx(m["om_d"], terms, x, dims=single), n, single, None, "dims %s" % single)
    if d >= 4:
        sub = [d - 1, 0, 2]                               # not contiguous, not ascending
        weights = [0.25, 2.0, 1.0]
        got = ob.design_dx(m["om_d"], terms, x, dims=sub, weights=weights)
        assert got.shape == (3, n, pp)
        compare(got, n, sub, weights, "dims %s weights %s" % (sub, weights))
    print("\n".join(lines))
    assert worst < 1, "\n".join(lines)


DESIGN_CASES = [("d1", 1), ("d1", 2), ("d1", 20), ("d4", 1), ("d4", 2), ("d4", 127), ("d4", 128), ("d4", 129), ("d4", 300),
                ("d11", 1), ("d11", 129), ("d11", 300), ("d4 knots130", 129)]


@pytest.mark.parametrize("name,p", DESIGN_CASES)
def test_staged_entries_fused(name, p, monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_design(name, p, "select", "fused")


@pytest.mark.parametrize("name,p", DESIGN_CASES)
def test_staged_entries_fallback(name, p, monkeypatch):
    monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    check_design(name, p, "select", "fallback")


@pytest.mark.parametrize("generic", [False, True])
def test_staged_entries_of_terms_of_nine_to_eleven_factors(generic, monkeypatch):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_design("d11", 40, "long", "9-11 factors" + (" forced" if generic else ""))


def test_unused_dimension_rows_are_rho_times_the_basis():
    """no term of d11's set uses dimension 7: D_7 = rho_7 B, every entry non-zero"""
    import outerbase_amd as ob
    m, c = model("d11"), case("d11", 129)
    assert not c["terms"][:, 7].any()
    got = ob.design_dx(m["om_d"], c["terms"], m["x"], dims=[7])[0]
    assert np.all(np.isfinite(got)) and np.all(got != 0)
    D, b = dref("d11", 129, "select")[7]
    w = E.worst_ratio(got, D, c["C"] * E._f64(b))
    print("dimension 7 of d11 (no term uses it): err/tolerance %.3g" % w)
    assert w < 1


# ---- 2. the state -----------------------------------------------------------------------------------
def _full(tri, p):
    G = np.zeros((p, p))
    G[np.triu_indices(p)] = tri
    return G + np.triu(G, 1).T


def _check(label, got, want, tol):
    assert np.all(np.isfinite(got)), label
    r = E.worst_ratio(got, want, tol)
    print("%s: max-norm %.3g, worst err/tol %.3g" % (label, E.maxnorm_relerr(got, want), r))
    return r <= 1.0


@functools.lru_cache(maxsize=None)
def state_case(which):
    """model, terms, 129 rows, the long-double derivative reference and C of the case"""
    if which == "d4":
        m, c = model("d4"), case("d4", 128)
        return dict(om_o=m["om_o"], om=m["om_d"], kinds=m["kinds"], terms=c["terms"], x=m["x"], ref=m["ref"], C=c["C"])
    from test_gpu_gram_dedup import small_model          # the smallest set with a redundant tile pair: d = 6, p = 512
    m = small_model("constructed")
    x = special_rows(np.random.default_rng(6), 129, m["kinds"], m["knots"])
    ref = X.reference_dx_of(m["om_o"], x)
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, m["om_o"], x, m["terms"]))
    return dict(om_o=m["om_o"], om=m["om_d"], kinds=m["kinds"], terms=m["terms"], x=x, ref=ref, C=Cc)


def grad_parts(s, rows, dims, weights, dY):
    """the stacked long-double rows of a batch, their bounds and the stacked observations"""
    S, bS = [], []
    sq = np.ones(len(dims)) if weights is None else np.sqrt(np.asarray(weights, dtype=np.float64))
    for j, l in enumerate(dims):
        D, b = s["ref"].getmat_dx(s["terms"], int(l))
        S.append(ld(sq[j]) * D[rows])
        bS.append(ld(sq[j]) * b[rows])
    return np.concatenate(S), np.concatenate(bS), R.stacked_g(dY[rows], sq)


def check_grad_state(label, st, S, bS, Gs, Cc, extra, gram=None):
    """tri and rhs against sum w D^T D and sum w D^T g over the stacked rows; b1 and the moments exactly 0"""
    p = S.shape[1]
    want, tol = gram if gram is not None else E.ref_gram(S, bS, np.arange(p), Cc, extra=extra)
    ok = _check(label + " triangle", _full(st["tri"], p), want, tol)
    for j in range(Gs.shape[1]):
        w, t = E.ref_tmatmul(S, bS, Gs[:, j], Cc)
        ok &= _check(label + " sum w D^T g_%d" % j, st["rhs"][:, j], w, t)
    for k in ("b1", "shift", "mu", "M2", "n"):
        assert not st[k].any(), k
    return ok


@pytest.mark.parametrize("q,chunk", [(1, None), (3, None), (1, 64), (3, 64)])
def test_state_after_gradient_batches(q, chunk, monkeypatch):
    import outerbase_amd as ob
    if chunk:
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(chunk))
    s = state_case("d4")
    dims, weights = [3, 0, 1], [0.5, 2.0, 1.5]
    _, dY = R.response(s["x"], q)
    dY = dY[:, dims, :]
    sizes = [63, 1, 65]
    S, bS, Gs = [], [], []
    with ob.NewtonAccumulator(s["om"], s["terms"], q) as acc:
        a = 0
        for nb in sizes:
            rows = np.arange(a, a + nb)
            acc.add_grad(s["x"][rows], dY[rows], dims=dims, weights=weights)
            parts = grad_parts(s, rows, dims, weights, dY)
            S.append(parts[0]), bS.append(parts[1]), Gs.append(parts[2])
            a += nb
        assert acc.rows == 0 and acc.grad_rows == 129 * 3 and acc.batches == 0
        st = acc.state()
    nchunks = sum(-(-nb // chunk) for nb in sizes) if chunk else len(sizes)
    assert check_grad_state("q=%d chunk %s batches %s" % (q, chunk, sizes), st, np.concatenate(S), np.concatenate(bS),
                            np.concatenate(Gs), s["C"], extra=nchunks + len(sizes))


@pytest.mark.parametrize("chunk", [None, 64])
def test_state_with_and_without_the_gram_deduplication(chunk, monkeypatch):
    """D_l^T D_l depends on the per-dimension unordered level pairs only, like B^T B: the skipped tile pair's entries,
    copied from their sources, are within the rule of computed ones, and the kept entries are the bits of the
    switched-off run"""
    import outerbase_amd as ob
    from test_gpu_gram_dedup import info
    if chunk:
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(chunk))
    s = state_case("constructed")
    _, dY = R.response(s["x"], 1)
    S, bS, Gs = grad_parts(s, np.arange(129), list(range(6)), None, dY)
    states = {}
    nchunks = -(-129 // chunk) if chunk else 1
    gram = E.ref_gram(S, bS, np.arange(S.shape[1]), s["C"], extra=nchunks + 1)      # (the slow part: once)
    for off in (True, False):
        if off:
            monkeypatch.setenv("OBHIP_GRAM_DEDUP", "0")
        else:
            monkeypatch.delenv("OBHIP_GRAM_DEDUP")
        with ob.NewtonAccumulator(s["om"], s["terms"], 1) as acc:
            acc.add_grad(s["x"], dY)
            skipped = info(acc._t)[1]
            print("dedup %s: %d tile pairs skipped" % ("off" if off else "on", skipped))
            assert skipped == 0 if off else skipped >= 1
            states[off] = acc.state()
        assert check_grad_state("constructed set, dedup %s, chunk %s" % ("off" if off else "on", chunk), states[off], S, bS,
                                Gs, s["C"], extra=nchunks + 1, gram=gram)
    same = states[True]["tri"] == states[False]["tri"]
    print("entries of the triangle that differ from the switched-off run: %d of %d" % ((~same).sum(), same.size))
    assert (~same).sum() <= 128 * 128                     # the one copied tile pair at most
    assert np.array_equal(states[True]["rhs"], states[False]["rhs"])


# ---- 3. order and removal -----------------------------------------------------------------------------
def _same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """value rows and gradient rows on the d4 model, q = 2, with the long-double sums of both kinds"""
    s = state_case("d4")
    Y, dY = R.response(s["x"], 2)
    dims, weights = [0, 1, 2, 3], list(R.WEIGHTS)
    B, bB = s["ref"].getmat(s["terms"])
    S, bS, Gs = grad_parts(s, np.arange(129), dims, weights, dY)
    return dict(s=s, Y=Y, dY=dY, dims=dims, weights=weights, B=B, bB=bB, S=S, bS=bS, Gs=Gs)


def check_mixed_state(label, st, c, vrows, with_grad, extra):
    """state against the sums over the value rows `vrows` (and all gradient rows), under the rule over ALL rows of
    both kinds that ever went in"""
    s = c["s"]
    p = len(s["terms"])
    cols = np.arange(p)
    T, bT = np.concatenate([c["B"], c["S"]]), np.concatenate([c["bB"], c["bS"]])
    _, tol = E.ref_gram(T, bT, cols, s["C"], extra=extra)
    want = c["B"][vrows].T @ c["B"][vrows] + (c["S"].T @ c["S"] if with_grad else 0)
    ok = _check(label + " triangle", _full(st["tri"], p), want, tol)
    V = c["Y"] - st["shift"][None, :]
    for j in range(2):
        _, tol = E.ref_tmatmul(T, bT, np.concatenate([V[:, j], c["Gs"][:, j]]), s["C"])
        want = c["B"][vrows].T @ np.asarray(V[vrows, j], dtype=ld) + (c["S"].T @ np.asarray(c["Gs"][:, j], dtype=ld) if with_grad else 0)
        ok &= _check(label + " rhs %d" % j, st["rhs"][:, j], want, tol)
    return ok


def test_order_of_value_and_gradient_batches():
    import outerbase_amd as ob
    c = mixed_case()
    s, x, Y, dY = c["s"], c["s"]["x"], c["Y"], c["dY"]
    kw = dict(dims=c["dims"], weights=c["weights"])
    lo, hi = slice(0, 64), slice(64, 129)
    orders = {"gradients first": [("g", lo), ("g", hi), ("v", lo), ("v", hi)],
              "values first": [("v", lo), ("v", hi), ("g", lo), ("g", hi)],
              "interleaved": [("g", hi), ("v", lo), ("g", lo), ("v", hi)]}
    ok, fits = True, {}
    for name, seq in orders.items():
        with ob.NewtonAccumulator(s["om"], s["terms"], 2) as acc:
            for kind, sl in seq:
                if kind == "g":
                    acc.add_grad(x[sl], dY[sl], **kw)
                else:
                    acc.add(x[sl], Y[sl])
            assert acc.rows == 129 and acc.grad_rows == 129 * 4 and acc.batches == 2
            st = acc.state()
            assert np.array_equal(st["shift"], Y[0]) and np.all(st["n"] == 129)
            ok &= check_mixed_state(name, st, c, np.arange(129), True, extra=4)
            fits[name] = acc.fit(sigma=R.SIGMA, rho=R.RHO)
    for name in orders:
        rel = R.relerr(fits[name].coeff, fits["values first"].coeff)
        print("%s: coefficients against `values first` %.3g" % (name, rel))
        assert rel < 1e-6
        assert np.array_equal(fits[name].y_cent, fits["values first"].y_cent)
    assert ok


def test_removal_of_gradient_rows_and_of_everything():
    import outerbase_amd as ob
    c = mixed_case()
    s, x, Y, dY = c["s"], c["s"]["x"], c["Y"], c["dY"]
    kw = dict(dims=c["dims"], weights=c["weights"])
    with ob.NewtonAccumulator(s["om"], s["terms"], 2) as acc, ob.NewtonAccumulator(s["om"], s["terms"], 2) as vals:
        vals.add(x, Y)
        acc.add(x, Y)
        acc.add_grad(x, dY, **kw)
        acc.remove_grad(x, dY, **kw)
        assert acc.rows == 129 and acc.grad_rows == 0
        assert check_mixed_state("add_grad; remove_grad on value rows", acc.state(), c, np.arange(129), False, extra=3)
        f, fv = acc.fit(sigma=R.SIGMA, rho=R.RHO), vals.fit(sigma=R.SIGMA, rho=R.RHO)
        rel = R.relerr(f.coeff, fv.coeff)
        print("fit after add_grad; remove_grad against the value-only fit: %.3g" % rel)
        assert rel < 1e-6
        # values out first (B^T 1 and the moments go with them), then the gradients: exactly nothing left
        acc.add_grad(x[:70], dY[:70], **kw)
        acc.remove(x, Y)
        st = acc.state()
        assert acc.rows == 0 and acc.grad_rows == 70 * 4
        assert not st["b1"].any() and not st["n"].any() and not st["M2"].any() and st["tri"].any()
        acc.remove_grad(x[:70], dY[:70], **kw)
        assert acc.rows == 0 and acc.grad_rows == 0
        assert not any(v.any() for v in acc.state().values())
        # and the other way round
        acc.add_grad(x[:70], dY[:70], **kw).add(x, Y)
        acc.remove_grad(x[:70], dY[:70], **kw)
        assert acc.state()["tri"].any()
        acc.remove(x, Y)
        assert not any(v.any() for v in acc.state().values())


def test_merge_and_minus_with_gradient_rows_on_either_side():
    import outerbase_amd as ob
    c = mixed_case()
    s, x, Y, dY = c["s"], c["s"]["x"], c["Y"], c["dY"]
    kw = dict(dims=c["dims"], weights=c["weights"])
    lo, hi = slice(0, 64), slice(64, 129)
    mk = lambda: ob.NewtonAccumulator(s["om"], s["terms"], 2)
    with mk() as a, mk() as b, mk() as g, mk() as total:
        a.add(x[lo], Y[lo]).add_grad(x[lo], dY[lo], **kw)
        b.add_grad(x[hi], dY[hi], **kw).add(x[hi], Y[hi])
        g.add_grad(x[hi], dY[hi], **kw)                                  # gradient rows only
        total.merge(a).merge(b)
        assert total.rows == 129 and total.grad_rows == 129 * 4 and b.grad_rows == 65 * 4
        assert check_mixed_state("a merged with b", total.state(), c, np.arange(129), True, extra=6)
        before = total.state(), b.state()
        f_minus = total.fit(sigma=R.SIGMA, rho=R.RHO, minus=b)
        assert _same_state(before[0], total.state()) and _same_state(before[1], b.state())
        rel = R.relerr(f_minus.coeff, a.fit(sigma=R.SIGMA, rho=R.RHO).coeff)
        print("fit(minus=b) against the fit of a alone: %.3g" % rel)
        assert rel < 1e-6
        # a gradient-only accumulator on either side
        with mk() as want:
            want.add(x, Y).add_grad(x[lo], dY[lo], **kw)
            fw = want.fit(sigma=R.SIGMA, rho=R.RHO)
        rel = R.relerr(total.fit(sigma=R.SIGMA, rho=R.RHO, minus=g).coeff, fw.coeff)
        print("fit(minus=gradient rows only): %.3g" % rel)
        assert rel < 1e-6
        total.merge(g, sign=-1)
        assert total.rows == 129 and total.grad_rows == 64 * 4
        rel = R.relerr(total.fit(sigma=R.SIGMA, rho=R.RHO).coeff, fw.coeff)
        print("merge(gradient rows only, sign=-1): %.3g" % rel)
        assert rel < 1e-6
        g.merge(a)                                                        # values into a gradient-only state
        assert g.rows == 64 and g.grad_rows == 129 * 4 and np.array_equal(g.state()["shift"], Y[0])
        with pytest.raises(ob.ObhipError) as ei:
            a.merge(g, sign=-1)                                           # more gradient equations than a holds
        assert ei.value.code == 4


# ---- 4. the fit ---------------------------------------------------------------------------------------
def check_fit(label, fit, Hl, Rl, theta, theta64, cent, sd, Bnew, xnew, p):
    rel = R.relerr(fit.coeff, theta)
    dh = float(np.max(np.abs(fit.diagH / E._f64(np.diag(Hl)) - 1)))
    want = E._f64((Bnew @ theta) * sd[None, :] + cent[None, :])
    pred = fit.predict(xnew)
    relp = R.relerr(pred, want)
    eta, eta1 = backward_errors(Hl, fit.coeff, Rl), backward_errors(Hl, theta64, Rl)
    lim = np.maximum(4 * eta1, p * U)
    print("%s: coefficients %.3g, predictions %.3g (1e-6), diagH %.3g (1e-10); backward error %.3g, float64 reference "
          "solve %.3g, worst eta / allowed %.3g" % (label, rel, relp, dh, eta.max(), eta1.max(), np.max(eta / lim)))
    assert np.allclose(fit.y_cent, E._f64(cent), rtol=1e-13, atol=0) and np.allclose(fit.y_sca, E._f64(sd), rtol=1e-12, atol=0)
    assert rel < 1e-6 and relp < 1e-6 and dh < 1e-10
    assert np.all(np.isfinite(eta)) and np.all(eta <= lim)


@pytest.mark.parametrize("n,p", R.CPU_CASES)
def test_fit_against_the_refined_long_double_solution(n, p):
    import outerbase_amd as ob
    c = R.cpu_case(n, p)
    _, om = R.pair()
    fit = ob.fit_newton_grad(om, c["terms"], c["x"], c["Y"], c["dY"], weights=R.WEIGHTS, sigma=R.SIGMA, rho=R.RHO)
    knots = [c["om_o"].knots_of(k) for k in range(4)]
    xnew = sample_x(np.random.default_rng(9), 50, c["om_o"].kinds)
    Bnew, _ = E.ExtendedRef(c["om_o"].kinds, knots, c["om_o"].hyp, c["om_o"].rotmat, xnew).getmat(c["terms"])
    check_fit("n=%d p=%d" % (n, p), fit, c["Hl"], c["Rl"], c["theta"], c["theta64"], c["cent"], c["sd"], Bnew, xnew, p)


def test_fit_p384_with_gradients_at_other_inputs():
    """the eight-dimensional model of test_gpu_stream.py: 150 value rows, gradients by dimensions (5, 0, 2) at 70
    other inputs, two responses"""
    import ob_oracle as O
    import outerbase_amd as ob
    from test_gpu_stream import _model
    kinds, knots, om_o, om = _model(384)
    p, dims, weights = 384, [5, 0, 2], [0.5, 1.0, 2.0]
    terms = om_o.selectterms(p)
    rng = np.random.default_rng(384)
    x, xg = sample_x(rng, 150, kinds), sample_x(rng, 70, kinds)
    Y, _ = R.response(x, 2)
    _, dYg = R.response(xg, 2)
    dYg = dYg[:, dims, :]
    fit = ob.fit_newton_grad(om, terms, x, Y, dYg, xg=xg, dims=dims, weights=weights, sigma=R.SIGMA, rho=R.RHO)
    kn = [np.asarray(k, dtype=np.float64) for k in knots]
    Bl, _ = E.ExtendedRef(kinds, kn, om_o.hyp, om_o.rotmat, x).getmat(terms)
    Sl, _, sq = R.stacked(X.reference_dx_of(om_o, xg), terms, dims, weights)
    prec = O.prior_prec(om_o, terms, R.RHO)
    Hl, Rl, cent, sd = R.normal_equations(Bl, Y, prec, R.SIGMA, Sl, R.stacked_g(dYg, sq), dtype=ld)
    theta64, theta = R.solve_refined(Hl, Rl)
    print("p=384: cond(H) %.3g" % np.linalg.cond(E._f64(Hl)))
    xnew = sample_x(rng, 50, kinds)
    Bnew, _ = E.ExtendedRef(kinds, kn, om_o.hyp, om_o.rotmat, xnew).getmat(terms)
    check_fit("p=384 d=8", fit, Hl, Rl, theta, theta64, cent, sd, Bnew, xnew, p)


# ---- 5. bits and errors -------------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bits(monkeypatch):
    import outerbase_amd as ob
    c = mixed_case()
    s, x, Y, dY = c["s"], c["s"]["x"], c["Y"], c["dY"]
    res = []
    for chunk in (None, None, 64, 64):
        if chunk:
            monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", str(chunk))
        with ob.NewtonAccumulator(s["om"], s["terms"], 2) as acc:
            acc.add_grad(x[:63], dY[:63][:, [2, 0]], dims=[2, 0], weights=[0.3, 1.7])
            acc.add(x[:100], Y[:100])
            acc.add_grad(x[63:], dY[63:])
            acc.remove_grad(x[:63], dY[:63][:, [2, 0]], dims=[2, 0], weights=[0.3, 1.7])
            f = acc.fit(sigma=R.SIGMA, rho=R.RHO)
            res.append((acc.state(), f.coeff, f.diagH))
        d = ob.design_dx(s["om"], s["terms"], x, dims=[1, 3], weights=[2.0, 0.5])
        res[-1] = res[-1] + (d,)
    for a, b in ((res[0], res[1]), (res[2], res[3])):
        assert _same_state(a[0], b[0])
        assert all(np.array_equal(u, v) for u, v in zip(a[1:], b[1:]))


def test_refusals_leave_the_state_unchanged_and_the_accumulator_usable():
    """Every refusal below is a host-side check that returns before a launch, in the documented order."""
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    from conftest import knots_for, make_pair
    kinds = ["mat25", "mat25pow", "mat25"]
    knots = knots_for(kinds, 20)
    _, om = make_pair(kinds, knots)
    terms = om.selectterms(60)
    x = sample_x(np.random.default_rng(3), 120, kinds)
    Y, dY = R.response(x, 2)
    with ob.NewtonAccumulator(om, terms, 2) as acc:
        acc.add_grad(x[:50], dY[:50])
        acc.add(x[:100], Y[:100])
        good, st0 = acc.fit(), acc.state()

        def unchanged():
            assert acc.rows == 100 and acc.grad_rows == 150 and _same_state(acc.state(), st0)
            assert np.array_equal(acc.fit().coeff, good.coeff)

        dx = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
        dg = torch.from_numpy(np.ascontiguousarray(dY.transpose(2, 1, 0))).cuda()
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        f64 = lambda *v: (C.c_double * len(v))(*v)
        add = lib.obhip_normal_acc_add_grad_dev
        h, X_, G_ = acc._h, dx.data_ptr(), dg.data_ptr()
        all3 = u32(0, 1, 2)
        assert add(h, None, 120, all3, 3, None, G_, 120, 1) == 1 and b"null" in lib.obhip_last_error()
        assert add(h, X_, 120, None, 3, None, G_, 120, 1) == 1
        assert add(h, X_, 120, all3, 3, None, None, 120, 1) == 1
        assert add(h, X_, 120, all3, 3, None, G_, 120, 2) == 1
        # ndims = 0, a repeated dimension, a dimension >= d, a bad weight, lddy < n: each before the next
        assert add(h, X_, 120, u32(1, 1), 0, f64(-1.0), G_, 1, 1) == 1 and b"ndims" in lib.obhip_last_error()
        assert add(h, X_, 120, u32(5, 5), 2, f64(-1.0, 1.0), G_, 1, 1) == 1 and b"twice" in lib.obhip_last_error()
        assert add(h, X_, 120, u32(1, 3), 2, f64(-1.0, 1.0), G_, 1, 1) == 1 and b"dimension 3" in lib.obhip_last_error()
        for bad in (0.0, -2.0, NAN, float("inf")):
            assert add(h, X_, 120, u32(1, 2), 2, f64(1.0, bad), G_, 1, 1) == 1 and b"weights" in lib.obhip_last_error()
        assert add(h, X_, 120, u32(1, 2), 2, f64(1.0, 2.0), G_, 119, 1) == 1 and b"lddy" in lib.obhip_last_error()
        unchanged()
        # more equations out than are in: 120 x 3 > 150, and through a merge
        assert add(h, X_, 120, all3, 3, None, G_, 120, -1) == 4 and b"removing 360 gradient equations" in lib.obhip_last_error()
        with pytest.raises(ob.ObhipError) as ei:
            acc.remove_grad(x[:51], dY[:51])
        assert ei.value.code == 4
        unchanged()
        assert add(h, X_, 0, all3, 3, None, None, 0, 1) == 0          # no rows: a no-op
        unchanged()
        eq, nb = C.c_uint64(0), C.c_uint64(0)
        assert lib.obhip_normal_acc_grad_info(h, C.byref(eq), C.byref(nb)) == 0 and (eq.value, nb.value) == (150, 1)
        # the model changes after the first GRADIENT batch of an accumulator without value rows
        with ob.NewtonAccumulator(om, terms, 2) as gonly:
            gonly.add_grad(x[:10], dY[:10])
            sg = gonly.state()
            hyp = ob.gethyp(om)
            om.updatehyp(hyp + 0.1)
            for f in (lambda: gonly.add_grad(x[10:20], dY[10:20]), lambda: gonly.add(x[:20], Y[:20]),
                      lambda: acc.add_grad(x[50:60], dY[50:60]), acc.fit):
                with pytest.raises(ob.ObhipError, match="changed since") as ei:
                    f()
                assert ei.value.code == 4
            assert _same_state(gonly.state(), sg) and gonly.grad_rows == 30
            assert _same_state(acc.state(), st0)
            om.updatehyp(hyp)
        # usable again after a reset
        acc.reset()
        assert acc.rows == 0 and acc.grad_rows == 0
        acc.add(x[:100], Y[:100]).add_grad(x[:50], dY[:50])
        rel = R.relerr(acc.fit().coeff, good.coeff)
        print("after reset, the same rows again: %.3g" % rel)
        assert rel < 1e-6
    torch.cuda.synchronize()
