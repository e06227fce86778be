"""The streaming Newton fit (obhip_normal_acc_*, obhip_cv_score_dev, outerbase_amd/stream.py): rows
added and removed in ragged batches, fits that leave another accumulator's rows out, K-fold CV.

Where the bounds come from:
  statistics   tests/extended_ref.py's own rule, per entry: C x (propagated conditioning bound) +
               gamma_k x (sum of |summands|), C = eight times what the float64 oracle measures on the
               same rows, at most 2e-13.  A batched sum is one more summation order of the same
               summands; the additions of the batch sums go into the Gram's gamma_k through `extra`
               (ref_tmatmul takes no `extra`: B^T (Y - c) and B^T 1 are held to the plain rule, which
               is the stricter).  After add(A); add(B); remove(B) the tolerance is the rule over the
               rows of A and B, nothing added for B's summands having gone in twice.  A merge of two
               accumulators with different shifts forms B^T (y - c_src) + (c_src - c_dst) B^T 1 for
               the source's rows: those entries are held to the rule on the summands that were
               actually added (see test_statistics_after_a_merge_that_moves_the_shift).
  moments      1e-13 for the mean, 1e-12 for the sd, test_fit_and_predict_against_the_oracle's figures
               for y_cent / y_sca, with no absolute term: the sd relative to itself, the mean
               relative to max(|mean|, sd) -- the size of the numbers a mean is a sum of; relative to
               |mean| alone the float64 mean of a centred response has no correct digit to offer.
               The large-offset case is measured against np.longdouble with the float64 two-pass
               value as the yardstick (see that test).
  fits         1e-6 relative for Theta and predictions, 1e-10 for diagH: what
               tests/test_gpu_multi_response.py grants the one-shot fit against the oracle; the
               backward error against the oracle's H and right-hand side is held to
               max(4 eta of the one-shot fit, p 2^-53), test_multi_solve_backward_error's rule.
Every test prints its figures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

import extended_ref as E
from conftest import knots_for, make_pair
from multi_schedule_worker import backward_errors

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MIXED = ["mat25", "mat25pow", "mat25ang", "mat25"]
SIGMA, RHO = math.log(0.01), 6.0
_MODELS = {}


def _model(p):
    """mixed d = 4 on 40 knots up to p = 300; eight mat25 dimensions on 30 knots above (the term
    sets of test_gpu_extended's packed-diagonal Gram cases)"""
    key = "small" if p <= 300 else "large"
    if key not in _MODELS:
        kinds = MIXED if key == "small" else ["mat25"] * 8
        knots = knots_for(kinds, 40 if key == "small" else 30)
        om_o, om = make_pair(kinds, knots)
        _MODELS[key] = (kinds, knots, om_o, om)
    return _MODELS[key]


def _responses(x, y, q, seed=5):
    """q raw columns: y, then smooth column-dependent transforms of it plus a little noise, on
    different scales and offsets"""
    rng = np.random.default_rng(seed)
    cols = [y]
    for j in range(1, q):
        cols.append((1.0 + j) * (math.cos(0.37 * j) * y + math.sin(0.37 * j) * y * x[:, j % x.shape[1]]
                                 + 0.05 * np.std(y) * rng.standard_normal(len(y))) - 3.0 * j)
    return np.stack(cols, axis=1)


class _Case:
    def __init__(self, n, p, q, seed=7):
        import ob_oracle as O
        self.kinds, self.knots, self.om_o, self.om = _model(p)
        self.n, self.p, self.q, self.d = n, p, q, len(self.kinds)
        self.terms = self.om_o.selectterms(p)
        self.x, y = O.synth_xy(seed, 0, n, self.kinds)
        self.Y = _responses(self.x, y, q)
        self.xnew, _ = O.synth_xy(seed + 1, 0, 500, self.kinds)

    def extended(self):
        """long double B with its bounds on all rows, and the case's C from the oracle's B"""
        import ob_oracle as O
        import outerbase_amd as ob
        rot, _, _ = self.om.rotation()
        assert np.array_equal(rot, self.om_o.rotmat)
        ref = E.ExtendedRef(self.kinds, [np.asarray(k, dtype=np.float64) for k in self.knots], ob.gethyp(self.om), rot,
                            self.x)
        B, bB = ref.getmat(self.terms)
        Bo = O.ob_getmat(O.OuterBase(self.om_o, self.x), self.terms)
        ratio = E.worst_ratio(Bo, B, bB)
        Cc = E.constant_from_oracle_ratio(ratio)
        print("n=%d p=%d: oracle err/bound %.3g, C = %.3g" % (self.n, self.p, ratio, Cc))
        return B, bB, Cc


def _slices(sizes):
    out, a = [], 0
    for s in sizes:
        out.append(slice(a, a + s))
        a += s
    return out


def _full(tri, p):
    G = np.zeros((p, p))
    G[np.triu_indices(p)] = tri
    return G + np.triu(G, 1).T


def _check(label, got, want, tol):
    assert np.all(np.isfinite(got)), label
    r = E.worst_ratio(got, want, tol)
    print("%s: max-norm %.3g, worst err/tol %.3g" % (label, E.maxnorm_relerr(got, want), r))
    return r <= 1.0


def _moment_errors(cent, sd, want_cent, want_sd):
    """worst error of the means relative to max(|mean|, sd), of the sds relative to themselves"""
    return (float(np.max(np.abs(cent - want_cent) / np.maximum(np.abs(want_cent), want_sd))),
            float(np.max(np.abs(sd - want_sd) / want_sd)))


def _same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


CASES = [(5000, 63, 1, [1, 0, 1200, 799, 3000]),
         (8000, 300, 3, [2500, 1, 0, 3499, 2000]),
         (20000, 300, 17, [7000, 1, 6000, 0, 6999]),
         (6000, 1024, 17, [3000, 1, 2999]),
         (1500, 4096, 3, [700, 1, 799])]


# ---- 1. + 2. the statistics and the moments ---------------------------------------------------
@pytest.mark.parametrize("n,p,q,sizes", CASES)
def test_statistics_against_the_extended_reference(n, p, q, sizes):
    """Triangle (on gram_column_sample's columns against all p), B^T (Y - shift) and B^T 1 after
    ragged adds, after add(A); add(B); remove(B), and after merging (and un-merging) two accumulators
    whose shifts differ; mean and sd of the rows in the state each time."""
    import outerbase_amd as ob
    c = _Case(n, p, q)
    assert sum(sizes) == n
    B, bB, Cc = c.extended()
    cols = E.gram_column_sample(bB, 4242 + p)
    ok = True

    def gram_parts(rows):
        """ref_gram's pieces on a row set: the long double sums (the slow part, formed once per row
        set), the propagated bound and the sum of |summands|"""
        Bf = np.abs(np.asarray(B[rows], dtype=np.float64))
        return B[rows][:, cols].T @ B[rows], E.gram_bound(B[rows], bB[rows], cols), Bf[:, cols].T @ Bf, len(rows)

    nA = n - sizes[-1]
    A, Bset, everything = np.arange(nA), np.arange(nA, n), np.arange(n)
    gA, gB = gram_parts(A), gram_parts(Bset)
    gram = {"A": gA, "B": gB, "all": tuple(a + b for a, b in zip(gA, gB))}    # sums over disjoint row sets add

    def gram_tol(which, extra):
        _, bound, absum, k = gram[which]
        return E._sum_tol(Cc, bound, k + extra, absum)                       # ref_gram's tolerance

    def tm_tol(rows, v):
        return E.ref_tmatmul(B[rows], bB[rows], v, Cc)[1]

    def compare(label, acc, want_rows, extra, rhs_tol=None):
        """state of acc against the sums over the rows of `want_rows`, which must be "all" unless
        rows were taken out again: the tolerance is always the rule over ALL rows that ever went in
        (A and B).  rhs_tol(j, shift): another tolerance for B^T (y_j - c), for a merged state."""
        nonlocal ok
        rows = {"A": A, "all": everything}[want_rows]
        st = acc.state()
        assert acc.rows == len(rows) and np.all(st["n"] == len(rows))
        G = _full(st["tri"], p)
        ok &= _check(label + " triangle", G[cols, :], gram[want_rows][0], gram_tol("all", extra))
        # the shifted responses as the device forms them: one IEEE subtraction per entry
        V = c.Y - st["shift"][None, :]
        for j in range(q):
            want = E.ref_tmatmul(B[rows], bB[rows], V[rows, j], Cc)[0]
            tol = tm_tol(everything, V[:, j]) if rhs_tol is None else rhs_tol(j, st["shift"])
            ok &= _check(label + " B^T (y_%d - c)" % j, st["rhs"][:, j], want, tol)
        want = E.ref_tmatmul(B[rows], bB[rows], np.ones(len(rows)), Cc)[0]
        ok &= _check(label + " B^T 1", st["b1"], want, tm_tol(everything, np.ones(n)))
        fit = acc.fit()
        ec, es = _moment_errors(fit.y_cent, fit.y_sca, c.Y[rows].mean(axis=0), c.Y[rows].std(axis=0, ddof=1))
        print("%s: mean err / max(|mean|, sd) %.3g (1e-13), sd rel err %.3g (1e-12)" % (label, ec, es))
        assert ec <= 1e-13 and es <= 1e-12
        return st

    with ob.NewtonAccumulator(c.om, c.terms, q) as acc:
        for s in _slices(sizes):
            acc.add(c.x[s], c.Y[s])
        assert acc.batches == sum(1 for s in sizes if s > 0)
        first = _slices(sizes)[[i for i, s in enumerate(sizes) if s > 0][0]].start
        st = compare("adds %s" % sizes, acc, "all", extra=len(sizes))
        assert np.array_equal(st["shift"], c.Y[first])
    with ob.NewtonAccumulator(c.om, c.terms, q) as acc:
        acc.add(c.x[A], c.Y[A]).add(c.x[Bset], c.Y[Bset])
        assert acc.rows == n and acc.batches == 2
        acc.remove(c.x[Bset], c.Y[Bset])
        assert acc.batches == 1
        compare("add A, add B, remove B", acc, "A", extra=3)
    # two accumulators with different shifts (the first row of A, the first row of B) merged: the
    # source's right-hand sides are moved, R_B + (c_B - c_A) b1_B.  What was added for a row of B is
    # B_ik (y_i - c_B) and (c_B - c_A) B_ik, so the rule applies to those summands: the rule over A
    # with y - c_A, over B with y - c_B, |c_B - c_A| times the rule over B with ones, and two more
    # roundings (the product-and-add, the fold) on numbers no larger than the sums of |summands|.
    if nA > 0 and nA < n:
        BfB = np.abs(np.asarray(B[Bset], dtype=np.float64))

        def merged_tol(j, shift):
            cA, cB = shift[j], c.Y[nA, j]
            vB = c.Y[Bset, j] - cB
            absum = BfB.T @ np.abs(vB) + abs(cB - cA) * BfB.sum(axis=0)
            return (tm_tol(A, c.Y[A, j] - cA) + tm_tol(Bset, vB) + abs(cB - cA) * tm_tol(Bset, np.ones(len(Bset)))
                    + 2 * U * absum)

        with ob.NewtonAccumulator(c.om, c.terms, q) as acc, ob.NewtonAccumulator(c.om, c.terms, q) as src:
            acc.add(c.x[A], c.Y[A])
            src.add(c.x[Bset], c.Y[Bset])
            assert np.array_equal(src.state()["shift"], c.Y[nA]) and not np.array_equal(c.Y[nA], c.Y[0])
            acc.merge(src)
            assert acc.rows == n and acc.batches == 2 and src.rows == len(Bset)
            st = compare("A merged with B (shift moved)", acc, "all", extra=2, rhs_tol=merged_tol)
            assert np.array_equal(st["shift"], c.Y[0])
            # and un-merged: back to A, under the same tolerances
            acc.merge(src, sign=-1)
            compare("A + B - B by merge", acc, "A", extra=3, rhs_tol=merged_tol)
    assert ok


def test_moments_of_a_response_far_from_zero():
    """A response whose mean is 1e6 standard deviations from zero, batches with different local
    means, one of them removed again.  Mean and sd from the accumulator against np.longdouble
    moments of the rows that remain; the yardstick is the float64 two-pass value (np.mean, np.std)
    on the same rows.  The accumulator merges five batch results and takes one out: it is allowed
    eight times the yardstick's own error -- the factor extended_ref grants another summation order
    -- with a floor of 1e-12 relative (below that the yardstick's error is a few ulps and says
    nothing).  Measured on an MI355X: the offset response's mean 8.8e-18 and sd 5.8e-17 relative, the
    same as the yardstick (ratio 1); the largest ratio of the case is 15, on the mean of response 0
    (1.3e-15 against 8.4e-17 relative).  The ratios are printed."""
    import outerbase_amd as ob
    c = _Case(9000, 63, 3)
    rng = np.random.default_rng(17)
    sizes = [1500, 1, 2500, 1999, 3000]
    drift = [0.0, 4.0, -3.0, 7.0, 1.5]
    Y = c.Y.copy()
    Y[:, 1] = rng.standard_normal(c.n) + 1e6
    for s, dr in zip(_slices(sizes), drift):
        Y[s, 1] += dr
    sl = _slices(sizes)
    with ob.NewtonAccumulator(c.om, c.terms, 3) as acc:
        for s in sl:
            acc.add(c.x[s], Y[s])
        acc.remove(c.x[sl[2]], Y[sl[2]])
        fit = acc.fit()
    keep = np.concatenate([np.arange(s.start, s.stop) for i, s in enumerate(sl) if i != 2])
    yl = np.asarray(Y[keep], dtype=np.longdouble)
    cent = yl.mean(axis=0)
    sd = np.sqrt(((yl - cent) ** 2).sum(axis=0) / (len(keep) - 1))
    for j in range(3):
        for what, got, yard, want in (("mean", fit.y_cent[j], Y[keep, j].mean(), cent[j]),
                                      ("sd", fit.y_sca[j], Y[keep, j].std(ddof=1), sd[j])):
            e_acc = float(abs(np.longdouble(got) - want) / abs(want))
            e_yard = float(abs(np.longdouble(yard) - want) / abs(want))
            print("response %d %s: accumulator %.3g, two-pass float64 %.3g relative, ratio %s"
                  % (j, what, e_acc, e_yard, "%.3g" % (e_acc / e_yard) if e_yard > 0 else "inf"))
            assert e_acc <= max(8.0 * e_yard, 1e-12)


# ---- 3. + 4. fits -----------------------------------------------------------------------------
def _against_one_shot(c, fit, rows, label):
    """fit (from an accumulator) against fit_newton_multi on the same rows at once, and both against
    the oracle's H and right-hand side by the backward error"""
    import ob_oracle as O
    import outerbase_amd as ob
    one = ob.fit_newton_multi(c.om, c.terms, c.x[rows], c.Y[rows])
    wt = max(np.max(np.abs(fit.coeff[:, j] - one.coeff[:, j])) / np.max(np.abs(one.coeff[:, j])) for j in range(c.q))
    ma, mo = fit.predict(c.xnew), one.predict(c.xnew)
    wm = max(np.max(np.abs(ma[:, j] - mo[:, j])) / np.max(np.abs(mo[:, j])) for j in range(c.q))
    print("%s: Theta %.3g, predictions %.3g relative to the one-shot fit (worst column); diagH %.3g"
          % (label, wt, wm, np.max(np.abs(fit.diagH / one.diagH - 1))))
    assert wt < 1e-6 and wm < 1e-6
    assert np.allclose(fit.diagH, one.diagH, rtol=1e-10, atol=0)
    ec, es = _moment_errors(fit.y_cent, fit.y_sca, one.y_cent, one.y_sca)
    print("%s: against the one-shot fit: mean err / max(|mean|, sd) %.3g (1e-13), sd rel err %.3g (1e-12)" % (label, ec, es))
    assert ec <= 1e-13 and es <= 1e-12
    obo = O.OuterBase(c.om_o, c.x[rows])
    H = O.total_hess(obo, c.terms, SIGMA, RHO)
    Ys = (c.Y[rows] - c.Y[rows].mean(axis=0)) / c.Y[rows].std(axis=0, ddof=1)
    R = math.exp(-2 * SIGMA) * (O.ob_getmat(obo, c.terms).T @ Ys)
    # (the oracle's diagonal is a figure here, not a criterion: on the eight-dimensional term sets
    # that reach high levels the one-shot fit itself is further than 1e-10 from the float64 oracle)
    print("%s: diagH against the oracle's float64 H: accumulator %.3g, one-shot %.3g relative"
          % (label, np.max(np.abs(fit.diagH / np.diag(H) - 1)), np.max(np.abs(one.diagH / np.diag(H) - 1))))
    eta, eta1 = backward_errors(H, fit.coeff, R), backward_errors(H, one.coeff, R)
    lim = np.maximum(4 * eta1, c.p * U)
    print("%s: backward error accumulator %.3g, one-shot %.3g, worst eta / allowed %.3g"
          % (label, eta.max(), eta1.max(), np.max(eta / lim)))
    assert np.all(np.isfinite(eta)) and np.all(eta <= lim)


@pytest.mark.parametrize("n,p,q,sizes", CASES[1:])
def test_fit_equals_the_one_shot_fit(n, p, q, sizes):
    import outerbase_amd as ob
    c = _Case(n, p, q)
    with ob.NewtonAccumulator(c.om, c.terms, q) as acc:
        for s in _slices(sizes):
            acc.add(c.x[s], c.Y[s])
        fit = acc.fit()
    assert fit.coeff.shape == (p, q) and fit.sigma == SIGMA and fit.rho == RHO
    _against_one_shot(c, fit, np.arange(n), "n=%d p=%d q=%d" % (n, p, q))


@pytest.mark.parametrize("n,p,q", [(8000, 300, 3), (5000, 63, 1), (6000, 1024, 17)])
def test_minus_is_a_refit_and_writes_neither_accumulator(n, p, q):
    import outerbase_amd as ob
    c = _Case(n, p, q)
    rng = np.random.default_rng(3)
    hold = np.sort(rng.choice(n, size=n // 3 + 1, replace=False))
    rest = np.setdiff1d(np.arange(n), hold)
    with ob.NewtonAccumulator(c.om, c.terms, q) as total, ob.NewtonAccumulator(c.om, c.terms, q) as fold:
        for s in _slices([n // 2, 1, n - n // 2 - 1]):
            total.add(c.x[s], c.Y[s])
        fold.add(c.x[hold[:7]], c.Y[hold[:7]]).add(c.x[hold[7:]], c.Y[hold[7:]])
        before = total.state(), fold.state()
        fit = total.fit(minus=fold)
        after = total.state(), fold.state()
        assert _same_state(before[0], after[0]) and _same_state(before[1], after[1])
        assert total.rows == n and fold.rows == len(hold)
        _against_one_shot(c, fit, rest, "minus n=%d p=%d q=%d" % (n, p, q))
        # and the destructive way round gives the same fit to the same tolerance
        total.merge(fold, sign=-1)
        assert total.rows == len(rest)
        fit2 = total.fit()
        assert np.max(np.abs(fit2.coeff - fit.coeff)) <= 1e-6 * np.max(np.abs(fit.coeff))


# ---- 5. cross-validation ----------------------------------------------------------------------
def test_cv_matches_direct_refits_for_every_fold_and_candidate():
    """K = 4, a 2 x 2 grid: the held-out predictions of every fold at every candidate (one
    single-candidate run per candidate gives them) and the RMSE table of the grid run against
    K x C fit_newton_multi + predict refits on the complement rows.  Predictions to the fits' 1e-6
    relative; an RMSE is a root mean square of prediction errors, so it moves by at most the largest
    prediction difference: 1e-6 max |prediction|."""
    import outerbase_amd as ob
    n, p, q, K = 4000, 300, 3, 4
    c = _Case(n, p, q)
    sigmas, rhos = (math.log(0.01), math.log(0.3)), (6.0, 1.0)
    res = ob.cv_newton_multi(c.om, c.terms, c.x, c.Y, folds=K, sigmas=sigmas, rhos=rhos, seed=11)
    again = ob.cv_newton_multi(c.om, c.terms, c.x, c.Y, folds=K, sigmas=sigmas, rhos=rhos, seed=11)
    fold_of = ob.cv_folds(n, K, seed=11)
    assert np.array_equal(res.fold_of, fold_of) and np.array_equal(again.fold_of, fold_of)
    assert np.array_equal(res.rmse, again.rmse) and np.array_equal(res.heldout, again.heldout) and res.best == again.best
    assert res.candidates == [(s, r) for s in sigmas for r in rhos] and res.rmse.shape == (4, q)
    direct = np.empty((4, n, q))
    for ci, (s, r) in enumerate(res.candidates):
        for k in range(K):
            out, inn = fold_of == k, fold_of != k
            f = ob.fit_newton_multi(c.om, c.terms, c.x[inn], c.Y[inn], sigma=s, rho=r)
            direct[ci, out] = f.predict(c.x[out])
    rmse = np.sqrt(np.mean((direct - c.Y[None]) ** 2, axis=1))
    score = np.mean(rmse / c.Y.std(axis=0, ddof=1)[None, :], axis=1)
    scale = np.max(np.abs(direct), axis=1)                     # C x q
    for ci, (s, r) in enumerate(res.candidates):
        one = ob.cv_newton_multi(c.om, c.terms, c.x, c.Y, folds=K, sigmas=(s,), rhos=(r,), seed=11)
        assert one.best == 0 and np.array_equal(one.rmse[0], res.rmse[ci])
        for k in range(K):
            out = fold_of == k
            w = np.max(np.abs(one.heldout[out] - direct[ci, out]) / scale[ci][None, :])
            print("candidate %d (sigma %.3g, rho %.3g) fold %d: held-out predictions %.3g relative" % (ci, s, r, k, w))
            assert w < 1e-6
        print("candidate %d: rmse %s direct %s score %.6g direct %.6g" % (ci, res.rmse[ci], rmse[ci], res.score[ci], score[ci]))
        assert np.all(np.abs(res.rmse[ci] - rmse[ci]) <= 1e-6 * scale[ci])
    assert res.best == int(np.argmin(score)) and (res.sigma, res.rho) == res.candidates[res.best]
    assert np.max(np.abs(res.heldout - direct[res.best]) / scale[res.best][None, :]) < 1e-6
    full = ob.fit_newton_multi(c.om, c.terms, c.x, c.Y, sigma=res.sigma, rho=res.rho)
    assert res.fit.sigma == res.sigma and res.fit.rho == res.rho
    assert np.max(np.abs(res.fit.coeff - full.coeff)) < 1e-6 * np.max(np.abs(full.coeff))


def test_cv_score_is_the_sum_of_squared_errors_and_repeats_its_bits():
    """obhip_cv_score_dev against the sum formed in np.longdouble: n summands r^2 >= 0 in any order,
    and every r = fma(sd, m, cent) - y carries two roundings of numbers of size |cent| + |sd m| + |y|:
    |got - S| <= gamma_n S + 2 sum |r| 3 u (|cent| + |sd m| + |y|) (first order).  With meansd = NULL
    the predictions are raw.  Two calls give the same bits."""
    import torch
    from outerbase_amd._lib import call
    rng = np.random.default_rng(2)
    n, q, ld = 70001, 5, 70001 + 9
    M, Y = rng.standard_normal((q, ld)), rng.standard_normal((q, ld)) * 3 + 10
    ms = np.stack([rng.standard_normal(q) + 10, rng.random(q) + 2.5, np.full(q, 123.0)], axis=1)
    dM, dY, dms = torch.from_numpy(M).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(ms).cuda()
    outs = [torch.full((q, 2), float("nan"), dtype=torch.float64, device="cuda") for _ in range(3)]
    call("obhip_cv_score_dev", dM.data_ptr(), dY.data_ptr(), n, q, ld, dms.data_ptr(), outs[0].data_ptr())
    call("obhip_cv_score_dev", dM.data_ptr(), dY.data_ptr(), n, q, ld, dms.data_ptr(), outs[1].data_ptr())
    call("obhip_cv_score_dev", dM.data_ptr(), dY.data_ptr(), n, q, ld, None, outs[2].data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    got, raw = outs[0].cpu().numpy(), outs[2].cpu().numpy()
    assert np.all(got[:, 1] == n) and np.all(raw[:, 1] == n)
    L = np.longdouble
    for j in range(q):
        pm = ms[j, 1] * M[j, :n].astype(L)
        r = ms[j, 0] + pm - Y[j, :n]
        S = (r * r).sum()
        tol = E.gamma(n) * float(S) + float((2 * np.abs(r) * 3 * U * (abs(ms[j, 0]) + np.abs(pm) + np.abs(Y[j, :n]))).sum())
        r0 = M[j, :n].astype(L) - Y[j, :n]
        S0 = (r0 * r0).sum()
        tol0 = E.gamma(n) * float(S0) + float((2 * np.abs(r0) * U * np.abs(r0)).sum())
        print("cv score column %d: err/tol %.3g, raw %.3g" % (j, float(abs(got[j, 0] - S)) / tol, float(abs(raw[j, 0] - S0)) / tol0))
        assert float(abs(got[j, 0] - S)) <= tol and float(abs(raw[j, 0] - S0)) <= tol0


# ---- 6. determinism ---------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bits():
    import outerbase_amd as ob
    c = _Case(6000, 300, 17)
    sl = _slices([2500, 1, 1499, 2000])
    res = []
    for _ in range(2):
        with ob.NewtonAccumulator(c.om, c.terms, 17) as acc, ob.NewtonAccumulator(c.om, c.terms, 17) as part:
            for s in sl:
                acc.add(c.x[s], c.Y[s])
            acc.remove(c.x[sl[2]], c.Y[sl[2]])
            part.add(c.x[sl[0]], c.Y[sl[0]])
            f1, f2 = acc.fit(), acc.fit(minus=part)
            res.append((acc.state(), f1.coeff, f1.diagH, f1._meansd, f2.coeff, f2._meansd))
    assert _same_state(res[0][0], res[1][0])
    for a, b in zip(res[0][1:], res[1][1:]):
        assert np.array_equal(a, b)


# ---- 7. errors ----------------------------------------------------------------------------------
def test_errors_leave_the_accumulator_unchanged_and_usable():
    """Every refusal below is a host-side check that returns before a launch."""
    import torch
    import ob_oracle as O
    import outerbase_amd as ob
    from outerbase_amd._lib import call, lib
    kinds = ["mat25", "mat25pow", "mat25"]
    knots = knots_for(kinds, 20)
    _, om = make_pair(kinds, knots)
    _, other = make_pair(kinds, knots)
    terms = om.selectterms(60)
    t = ob.obmod._Terms(om, terms)
    x, y = O.synth_xy(3, 0, 300, kinds)
    Y = _responses(x, y, 2)

    def basis(model, rows):
        dx = torch.from_numpy(np.ascontiguousarray(x[rows].T)).cuda()
        h = C.c_void_p()
        call("obhip_basis_create_dev", C.byref(h), model._h, dx.data_ptr(), len(rows), t.maxlevels().ctypes.data)
        return h, dx

    with ob.NewtonAccumulator(om, t, 2) as acc, ob.NewtonAccumulator(om, t, 2) as tiny:
        acc.add(x[:100], Y[:100])
        good, st0 = acc.fit(), acc.state()
        dY = torch.from_numpy(np.ascontiguousarray(Y.T)).cuda()

        def unchanged():
            assert acc.rows == 100 and acc.batches == 1 and _same_state(acc.state(), st0)
            assert np.array_equal(acc.fit().coeff, good.coeff)

        # removing more rows than are present
        b200, _k1 = basis(om, np.arange(200))
        assert lib.obhip_normal_acc_add_dev(acc._h, b200, dY.data_ptr(), 300, -1) == 4
        assert b"removing 200 rows" in lib.obhip_last_error()
        unchanged()
        # bad arguments
        assert lib.obhip_normal_acc_add_dev(acc._h, b200, dY.data_ptr(), 300, 0) == 1
        assert lib.obhip_normal_acc_add_dev(acc._h, b200, None, 300, 1) == 1
        assert lib.obhip_normal_acc_add_dev(acc._h, b200, dY.data_ptr(), 199, 1) == 1
        lib.obhip_basis_destroy(b200)
        unchanged()
        # a basis on a foreign model
        bf, _k2 = basis(other, np.arange(50))
        assert lib.obhip_normal_acc_add_dev(acc._h, bf, dY.data_ptr(), 300, 1) == 1
        assert b"another model" in lib.obhip_last_error()
        lib.obhip_basis_destroy(bf)
        unchanged()
        # fewer than two rows to solve on: one row in the state, and all but one taken out
        tiny.add(x[:1], Y[:1])
        with pytest.raises(ob.ObhipError, match="rows left") as ei:
            tiny.fit()
        assert ei.value.code == 4 and tiny.rows == 1
        tiny.add(x[1:99], Y[1:99])
        with pytest.raises(ob.ObhipError, match="rows left") as ei:
            acc.fit(minus=tiny)
        assert ei.value.code == 4
        tiny.add(x[100:110], Y[100:110])                     # 109 rows: more than acc holds
        with pytest.raises(ob.ObhipError) as ei:
            acc.fit(minus=tiny)
        assert ei.value.code == 4
        with pytest.raises(ob.ObhipError) as ei:
            acc.merge(tiny, sign=-1)
        assert ei.value.code == 4
        unchanged()
        # accumulators of different shapes do not combine; a workspace too small
        with ob.NewtonAccumulator(om, t, 3) as q3:
            q3.add(x[:10], _responses(x, y, 3)[:10])
            with pytest.raises(ob.ObhipError) as ei:
                acc.merge(q3)
            assert ei.value.code == 1
        b = acc._bufs
        assert lib.obhip_normal_acc_solve_dev(acc._h, None, SIGMA, RHO, b["H"].data_ptr(), b["theta"].data_ptr(), None,
                                              b["meansd"].data_ptr(), b["ws"].data_ptr(), b["ws"].numel() - 8) == 1
        assert lib.obhip_normal_acc_solve_dev(acc._h, None, SIGMA, RHO, None, b["theta"].data_ptr(), None,
                                              b["meansd"].data_ptr(), b["ws"].data_ptr(), b["ws"].numel()) == 1
        unchanged()
        # the model's hyper-parameters change between adds: G of the state belongs to the old ones
        hyp = ob.gethyp(om)
        om.updatehyp(hyp + 0.1)
        for f in (lambda: acc.add(x[100:200], Y[100:200]), acc.fit, lambda: tiny.merge(acc)):
            with pytest.raises(ob.ObhipError, match="changed since") as ei:
                f()
            assert ei.value.code == 4
        assert acc.rows == 100 and _same_state(acc.state(), st0)
        # usable again after a reset, under the new hyper-parameters
        acc.reset()
        assert acc.rows == 0 and acc.batches == 0
        acc.add(x[:100], Y[:100]).add(x[100:200], Y[100:200])
        one = ob.fit_newton_multi(om, terms, x[:200], Y[:200])
        assert np.max(np.abs(acc.fit().coeff - one.coeff)) < 1e-6 * np.max(np.abs(one.coeff))
    torch.cuda.synchronize()
