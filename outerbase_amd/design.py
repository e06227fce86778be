"""Sequential design: which inputs should the simulator be run at next?

A Posterior keeps the total Hessian H of one model and term set, its Cholesky factor and sigma on the
device (include/obhip.h, "posterior handle").  It answers with the full posterior covariance of the
coefficients where MultiFit.predict(var=True) uses the diagonal form: var gives b^T inv(H) b at any rows,
condition the posterior after runs at given rows (the model is linear in its coefficients, so that does
not depend on what the runs return), and select picks k of m candidate rows greedily by one of two
criteria, every step one pass of a fused kernel over the candidates (csrc/kernels_design.hip):

  maxvar   the largest posterior variance: greedy D-optimality, log det H grows by log(1 + d_j / nu);
  imse     the largest drop of the variance integrated over a reference measure: I-optimality.

Variances are in standardised units (response / its standard deviation).  A posterior made from an
accumulator carries meansd (q x 3: centre, scale, rows), so var * meansd[j, 1] ** 2 is response j's
variance in raw units; the selection does not depend on that scale, which multiplies every candidate's
score alike.

Draws.  The posterior of one response's coefficients is N(theta, inv(H)): draw gives coefficient samples
theta + L^-T z, sample their joint sample paths over rows x, thompson the optimum of every draw over a
candidate set in one fused pass per block of draws (csrc/kernels_sample.hip; the m x S paths are never
stored) -- Thompson sampling, the simplest batch acquisition that uses the response.  torch supplies the
normals (or the caller does, z=), the library the arithmetic.

Acquisition.  acquire picks k candidates one after the other by expected improvement, probability of
improvement, a confidence bound or the straddle contour criterion of the latent mean and variance; after
every pick the run there is given a value without being made (the kriging believer or a constant liar) and
every candidate's mean and variance are downdated on the device (csrc/kernels_acquire.hip).  var_grad and
acquire_grad give the latent variance, the same four criteria and their gradients by the inputs at any rows
(csrc/kernels_acquire_dx.hip): what a gradient ascent from the best candidates needs.  acquire_multi picks over the
q responses of one fit, which share the latent variance: an objective among the inputs that keep the other responses
within their limits (constrained expected improvement, probability of improvement, probability of feasibility), or the
trade-off curve of two responses (expected hypervolume improvement); csrc/kernels_acquire_multi.hip.

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C

import numpy as np

from . import obmod
from ._lib import call, lib

CRITERIA = {"maxvar": 0, "imse": 1}
ACQUISITIONS = {"ei": 0, "pi": 1, "lcb": 2, "straddle": 3}
LIES = {"believer": 0, "constant": 1}
MULTI_ACQUISITIONS = {"cei": 0, "cpi": 1, "pof": 2, "ehvi": 3}


def _stream():
    import torch
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch.device("cuda", torch.cuda.current_device())


def _rows(om, x, what):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != om.d:
        raise ValueError("%s must be n x d" % what)
    return x


def _dev_cols(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)      # column-major n x d


class DesignResult:
    """index (n_picked): the picked candidates in order; score (n_picked): the criterion at pick time
    (maxvar: w_j d_j; imse: the weighted drop of the integrated variance); var (m): b_i^T inv(H_k) b_i of
    every candidate after all picks; trace (n_picked + 1): maxvar: the cumulative gain of log det H,
    imse: the integrated variance tr(M S_t), either from t = 0.  Fewer than k picks: no eligible
    candidate was left."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class ThompsonResult:
    """index (S): per draw the candidate row at which its sample path is smallest (maximize: largest), -1
    when no candidate was eligible; value (S): the path there (NaN); picks: the distinct indices in order of
    first appearance, -1 left out; counts: per pick the number of draws that chose it -- counts / S is the
    empirical probability that the candidate is the optimum."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class AcquireResult:
    """index (n_picked): the picked candidates in order; score (n_picked): each one's criterion when it was
    picked; score0 (m): every candidate's criterion at the first step, eligible or not; mean, var (m): the latent
    mean and variance (without the noise) of every candidate after all fantasies; criterion.  Fewer than k
    picks: no eligible candidate was left."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class AcquireMultiResult:
    """index (n_picked): the picked candidates in order; score (n_picked): each one's criterion when it was picked;
    score0, pof0 (m): every candidate's criterion and feasibility factor at the first step, eligible or not; mean
    (m x q): the latent means of every candidate after all fantasies; var (m): their shared latent variance in
    standardised units (without the noise) and scale (q): response j's raw variance is scale[j]**2 * var; front
    (F x 2, ehvi): the front after all fantasies, ascending in the signed first objective; best (cei, cpi): the final
    incumbent, infinite while no pick was believed feasible; criterion.  Fewer than k picks: no eligible candidate
    was left."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class AcquireGradResult:
    """score (n): the criterion at every row; grad (n x d): its gradient by the inputs; mean, var (n): the latent
    mean and variance (without the noise); grad_mean, grad_var (n x d): their gradients; criterion.  A row with a
    coordinate that is not finite has NaN everywhere."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Posterior:
    """The posterior covariance inv(H) of the coefficients of (om, terms), resident on the device."""

    def __init__(self, om, t, handle, meansd=None):
        self.om, self._t, self._h, self.meansd = om, t, handle, meansd
        self.p = t.p

    @classmethod
    def from_hessian(cls, om, terms, H, sigma):
        """H: the total Hessian (p x p, symmetric positive definite, e.g. e^{-2 sigma} B^T B + diag(prec))"""
        import torch
        t = obmod._terms_of(om, terms)
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.shape != (t.p, t.p):
            raise ValueError("H must be p x p")
        dev = _stream()
        dH = torch.from_numpy(H).to(dev)
        h = C.c_void_p()
        call("obhip_posterior_create_dev", C.byref(h), om._h, t._h, dH.data_ptr(), float(sigma))
        return cls(om, t, h)

    # -- life time ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.obhip_posterior_destroy(self._h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _need(self):
        if not self._h:
            raise RuntimeError("the posterior is closed")

    # -- what it knows -----------------------------------------------------------------------
    def _info(self):
        self._need()
        p, s, ld = C.c_uint64(0), C.c_double(0), C.c_double(0)
        call("obhip_posterior_info", self._h, C.byref(p), C.byref(s), C.byref(ld))
        return p.value, s.value, ld.value

    @property
    def sigma(self):
        return self._info()[1]

    @property
    def logdet(self):
        """log det H, from the factor"""
        return self._info()[2]

    def var(self, x, noise=False):
        """b_i^T inv(H) b_i at the rows x (n x d), with noise=True plus e^{2 sigma}: standardised units"""
        import torch
        self._need()
        x = _rows(self.om, x, "x")
        n = x.shape[0]
        if n == 0:
            return np.zeros(0)
        dev = _stream()
        dx = _dev_cols(x, dev)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        call("obhip_posterior_var_dev", self._h, dx.data_ptr(), n, out.data_ptr(), int(bool(noise)))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def condition(self, x):
        """-> a new Posterior for H + e^{-2 sigma} B(x)^T B(x): after runs at the rows x, done or pending"""
        self._need()
        x = _rows(self.om, x, "x")
        if x.shape[0] == 0:
            raise ValueError("no rows to condition on")
        dev = _stream()
        dx = _dev_cols(x, dev)
        h = C.c_void_p()
        call("obhip_posterior_condition_dev", self._h, dx.data_ptr(), x.shape[0], C.byref(h))
        return Posterior(self.om, self._t, h, self.meansd)

    def select(self, xcand, k, criterion="maxvar", reference=None, ref_weights=None, weights=None, replace=False):
        """Pick k of the candidate rows xcand (m x d) greedily; after every pick the posterior is conditioned
        on a run there.  criterion "imse" needs reference (r x d rows, with ref_weights >= 0 or all 1), the
        measure the variance is integrated over.  weights (m, >= 0): a candidate's score is multiplied by
        its weight, weight 0 excludes it.  replace=True lets a row be picked again (a replicate).  A
        candidate with a coordinate that is not finite is never picked.  The picks do not depend on the
        scale of the response.  -> DesignResult"""
        import torch
        self._need()
        if criterion not in CRITERIA:
            raise ValueError("criterion must be one of %s" % sorted(CRITERIA))
        xcand = _rows(self.om, xcand, "xcand")
        m, k = xcand.shape[0], int(k)
        if m == 0 or k < 1:
            raise ValueError("select needs candidates and k >= 1")
        imse = criterion == "imse"
        r = 0
        if imse:
            if reference is None:
                raise ValueError("criterion 'imse' needs reference rows")
            reference = _rows(self.om, reference, "reference")
            r = reference.shape[0]
            if r == 0:
                raise ValueError("criterion 'imse' needs reference rows")
            if ref_weights is not None:
                ref_weights = np.ascontiguousarray(ref_weights, dtype=np.float64)
                if ref_weights.shape != (r,):
                    raise ValueError("ref_weights must have one entry per reference row")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            if weights.shape != (m,):
                raise ValueError("weights must have one entry per candidate")
        dev = _stream()
        f64, nan = torch.float64, float("nan")
        dx = _dev_cols(xcand, dev)
        dr = _dev_cols(reference, dev) if imse else None
        du = torch.from_numpy(ref_weights).to(dev) if imse and ref_weights is not None else None
        dw = torch.from_numpy(weights).to(dev) if weights is not None else None
        index = torch.full((k,), -1, dtype=torch.int64, device=dev)
        score = torch.full((k,), nan, dtype=f64, device=dev)
        var = torch.full((m,), nan, dtype=f64, device=dev)
        trace = torch.full((k + 1,), nan, dtype=f64, device=dev)
        npk = C.c_uint64(0)
        call("obhip_design_select_dev", self._h, dx.data_ptr(), m, CRITERIA[criterion],
             None if dr is None else dr.data_ptr(), r, None if du is None else du.data_ptr(),
             None if dw is None else dw.data_ptr(), k, int(bool(replace)), index.data_ptr(), score.data_ptr(),
             var.data_ptr(), trace.data_ptr(), C.byref(npk))
        torch.cuda.synchronize()
        n = npk.value
        return DesignResult(index=index.cpu().numpy()[:n].copy(), score=score.cpu().numpy()[:n].copy(),
                            var=var.cpu().numpy(), trace=trace.cpu().numpy()[:n + 1].copy(), criterion=criterion,
                            n_picked=n, k=k)

    # -- acquisition -------------------------------------------------------------------------
    def acquire(self, xcand, theta, k=1, criterion="ei", best=None, level=None, kappa=1.96, xi=0.0, maximize=False,
                lie="believer", lie_value=None, skip=None, response=None):
        """Pick k of the candidate rows xcand (m x d) one after the other by a criterion of the latent mean mu and
        standard deviation sd (without the noise) of the response with the standardised coefficients theta (p).
        Written for minimisation (maximize=True: the same on -mu, -best, -level, -lie_value), t = best - xi - mu,
        u = t / sd:
          "ei"        t Phi(u) + sd phi(u), expected improvement on the incumbent best (required);
          "pi"        Phi(u), probability of improvement on best (required);
          "lcb"       kappa sd - mu, the confidence bound;
          "straddle"  kappa sd - |mu - level|, the contour f = level (required).
        After a pick the run there is given a value without being made -- lie="believer": its mean, the means do
        not move; lie="constant": lie_value (None: best for ei / pi) -- every candidate's mean and variance are
        conditioned on it, and for ei / pi the incumbent becomes the smaller of best and that value.  skip (m,
        nonzero = leave out): rows that are never picked, like rows with a coordinate that is not finite, rows
        picked before and rows whose score is not finite.  The lowest index wins among equal scores: ei and pi
        underflow to exact zeros far from the incumbent.  response=j on a posterior that carries meansd: best,
        level, lie_value and xi are given in raw units of response j and standardised on the way in; mean, var and
        the ei / lcb / straddle scores are de-standardised on the way out (pi has no unit).  The scale is positive,
        so the picks do not move.  -> AcquireResult"""
        import torch
        self._need()
        if lie not in LIES:
            raise ValueError("lie must be one of %s" % sorted(LIES))
        xcand = _rows(self.om, xcand, "xcand")
        m, k = xcand.shape[0], int(k)
        if m == 0 or k < 1:
            raise ValueError("acquire needs candidates and k >= 1")
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (self.p,):
            raise ValueError("theta must be the p standardised coefficients of one response")
        if lie == "constant" and lie_value is None:
            if criterion in ACQUISITIONS and criterion not in ("ei", "pi"):
                raise ValueError("lie='constant' needs lie_value")
            lie_value = best                                     # (None: refused below, ei and pi need best)
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8)
            if skip.shape != (m,):
                raise ValueError("skip must have one entry per candidate")
        pars, lie_value, sc = self._acquire_args(criterion, best, level, kappa, xi, response,
                                                 0.0 if lie_value is None else lie_value)
        dev = _stream()
        f64, nan = torch.float64, float("nan")
        dx = _dev_cols(xcand, dev)
        dth = torch.from_numpy(theta).to(dev)
        dk = torch.from_numpy(skip).to(dev) if skip is not None else None
        index = torch.full((k,), -1, dtype=torch.int64, device=dev)
        score = torch.full((k,), nan, dtype=f64, device=dev)
        score0, mean, var = (torch.full((m,), nan, dtype=f64, device=dev) for _ in range(3))
        params = (C.c_double * 4)(*pars)
        npk = C.c_uint64(0)
        call("obhip_acquire_dev", self._h, dth.data_ptr(), dx.data_ptr(), m, ACQUISITIONS[criterion], params,
             int(bool(maximize)), LIES[lie], lie_value, None if dk is None else dk.data_ptr(), k, index.data_ptr(),
             score.data_ptr(), score0.data_ptr(), mean.data_ptr(), var.data_ptr(), C.byref(npk))
        torch.cuda.synchronize()
        n = npk.value
        score, score0, mean, var = (a.cpu().numpy() for a in (score, score0, mean, var))
        mean, var, (score, score0) = self._acquire_raw(sc, criterion, maximize, mean, var, score[:n].copy(), score0)
        return AcquireResult(index=index.cpu().numpy()[:n].copy(), score=score, score0=score0, mean=mean, var=var,
                             criterion=criterion, n_picked=n, k=k)

    # -- acquisition over several responses --------------------------------------------------
    def _acquire_multi_args(self, q, objective, maximize, constraints, criterion, best, ref, front, xi, lie, lie_value):
        """acquire_multi's arguments, checked and standardised: (criterion, objs, roles, signs, limits, xi, front
        (F0 x 2), lie_value (q), scales (q x 2: centre, scale))"""
        if lie not in LIES:
            raise ValueError("lie must be one of %s" % sorted(LIES))
        if not 1 <= q <= 16:
            raise ValueError("acquire_multi takes 1 to 16 responses")
        if objective is None:
            objs = []
        elif np.ndim(objective) == 0:
            objs = [int(objective)]
        else:
            objs = [int(j) for j in objective]
        if criterion is None:
            criterion = {0: "pof", 1: "cei", 2: "ehvi"}.get(len(objs))
        if criterion not in MULTI_ACQUISITIONS:
            raise ValueError("criterion must be one of %s" % sorted(MULTI_ACQUISITIONS))
        need = {"cei": 1, "cpi": 1, "pof": 0, "ehvi": 2}[criterion]
        if len(objs) != need:
            raise ValueError("criterion %r takes %d objectives, %d given" % (criterion, need, len(objs)))
        if len(objs) == 2 and not objs[0] < objs[1]:
            raise ValueError("the two objectives are given in ascending response order")
        mx = [bool(v) for v in (maximize if np.ndim(maximize) else [maximize] * len(objs))]
        if len(mx) != len(objs):
            raise ValueError("maximize: one flag, or one per objective")
        if self.meansd is None:
            scales = np.tile([0.0, 1.0], (q, 1))
        else:
            if np.shape(self.meansd)[0] != q:
                raise ValueError("the posterior carries meansd of %d responses, Theta has %d" % (np.shape(self.meansd)[0], q))
            scales = np.array([self._scale(j) for j in range(q)])
        roles, signs, limits = np.full(q, 2, dtype=np.int32), np.ones(q), np.zeros(q)
        std = lambda j, v: (float(v) - scales[j, 0]) / scales[j, 1]
        for j, g in zip(objs, mx):
            if not 0 <= j < q:
                raise ValueError("objective %d is not one of the %d responses" % (j, q))
            roles[j], signs[j] = 0, -1.0 if g else 1.0
        for con in constraints:
            j, op, lim = con
            j = int(j)
            if not 0 <= j < q or roles[j] != 2:
                raise ValueError("constraint on response %r: not a response, or named twice" % (j,))
            if op not in ("<=", ">="):
                raise ValueError("a constraint is (j, '<=' | '>=', limit)")
            if not np.isfinite(lim):
                raise ValueError("a constraint's limit must be finite")
            roles[j], signs[j], limits[j] = 1, 1.0 if op == "<=" else -1.0, std(j, lim)
        if criterion == "pof" and not np.any(roles == 1):
            raise ValueError("criterion 'pof' needs at least one constraint")
        xi = float(xi)
        if not np.isfinite(xi):
            raise ValueError("xi must be finite")
        fr = np.zeros((0, 2))
        if criterion in ("cei", "cpi"):
            j = objs[0]
            if best is None:                                     # no feasible run yet: +inf in the signed sense
                limits[j] = signs[j] * np.inf
            else:
                if not np.isfinite(best):
                    raise ValueError("best must be finite, or None: no feasible run yet")
                limits[j] = std(j, best)
            xi = xi / scales[j, 1]
        elif best is not None:
            raise ValueError("best belongs to criteria 'cei' and 'cpi'")
        if criterion == "ehvi":
            if ref is None or np.shape(ref) != (2,) or not np.all(np.isfinite(ref)):
                raise ValueError("criterion 'ehvi' needs ref, the finite reference point of the two objectives")
            for a, j in enumerate(objs):
                limits[j] = std(j, ref[a])
            if front is not None:
                fr = np.array(front, dtype=np.float64).reshape(-1, 2) if np.size(front) else fr
                if not np.all(np.isfinite(fr)):
                    raise ValueError("the front's points must be finite")
                fr = np.column_stack([(fr[:, a] - scales[j, 0]) / scales[j, 1] for a, j in enumerate(objs)])
        elif ref is not None or front is not None:
            raise ValueError("ref and front belong to criterion 'ehvi'")
        lv = np.zeros(q)
        if lie == "constant":
            if lie_value is None or np.shape(lie_value) != (q,) or not np.all(np.isfinite(lie_value)):
                raise ValueError("lie='constant' needs lie_value, one finite value per response")
            lv = np.array([std(j, lie_value[j]) for j in range(q)])
        return criterion, objs, roles, signs, limits, xi, np.ascontiguousarray(fr), lv, scales

    def acquire_multi(self, xcand, Theta, k=1, objective=None, maximize=False, constraints=(), criterion=None, best=None,
                      ref=None, front=None, xi=0.0, lie="believer", lie_value=None, skip=None):
        """Pick k of the candidate rows xcand (m x d) one after the other by a criterion over the q responses with
        the standardised coefficients Theta (p x q, MultiFit.coeff) of one fit: they share the latent variance and,
        given the data, are independent, so feasibility probabilities multiply.  objective: a response index, a pair
        of indices (ascending) or None; maximize: one flag, or one per objective; constraints: triples
        (j, "<=" | ">=", limit).  criterion (None: inferred from objective):
          "cei"   one objective: expected improvement on best times the probability that every constraint holds;
                  best=None: no feasible run yet, the score is that probability alone until a pick is believed feasible;
          "cpi"   the same with the probability of improvement;
          "pof"   no objective: the probability that every constraint holds;
          "ehvi"  two objectives: the expected improvement of the hypervolume dominated by front (F0 x 2 points of the
                  two objectives, any order, dominated points allowed) inside the box of the reference point ref,
                  times that probability.
        After a pick every response gets a value without the run being made -- lie="believer": its mean;
        lie="constant": lie_value (q) -- and all means and the variance are conditioned on it; only a pick whose values
        meet every constraint moves the incumbent or enters the front.  skip, ties and eligibility as acquire.  On a
        posterior that carries meansd limits, best, ref, front, xi and lie_value are given in raw units of their
        response and standardised on the way in; mean, front and best come back raw (var is shared by the responses
        and stays standardised: response j's raw variance is scale[j]**2 * var), cei scores are multiplied by the objective's scale and ehvi scores by the product of the
        two (cpi and pof have no unit).  All scales are positive, so the picks do not move.  -> AcquireMultiResult"""
        import torch
        self._need()
        xcand = _rows(self.om, xcand, "xcand")
        m, k = xcand.shape[0], int(k)
        if m == 0 or k < 1:
            raise ValueError("acquire_multi needs candidates and k >= 1")
        Theta = np.asarray(Theta, dtype=np.float64)
        if Theta.ndim == 1:
            Theta = Theta[:, None]
        if Theta.ndim != 2 or Theta.shape[0] != self.p:
            raise ValueError("Theta must be p x q: the standardised coefficients of q responses")
        q = Theta.shape[1]
        criterion, objs, roles, signs, limits, xi, fr, lv, scales = self._acquire_multi_args(
            q, objective, maximize, constraints, criterion, best, ref, front, xi, lie, lie_value)
        F0 = len(fr)
        if criterion == "ehvi" and F0 + k > 2048:
            raise ValueError("front and k together must not exceed 2048 points")
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8)
            if skip.shape != (m,):
                raise ValueError("skip must have one entry per candidate")
        dev = _stream()
        f64, nan = torch.float64, float("nan")
        dx = _dev_cols(xcand, dev)
        dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)           # column-major p x q
        dk = torch.from_numpy(skip).to(dev) if skip is not None else None
        index = torch.full((k,), -1, dtype=torch.int64, device=dev)
        score = torch.full((k,), nan, dtype=f64, device=dev)
        score0, pof0, var = (torch.full((m,), nan, dtype=f64, device=dev) for _ in range(3))
        mean = torch.full((q, m), nan, dtype=f64, device=dev)
        fout = np.full((F0 + k, 2), np.nan)
        nf, npk, bout = C.c_uint64(0), C.c_uint64(0), C.c_double(nan)
        call("obhip_acquire_multi_dev", self._h, dth.data_ptr(), q, dx.data_ptr(), m, MULTI_ACQUISITIONS[criterion],
             roles.ctypes.data, signs.ctypes.data, limits.ctypes.data, xi, fr.ctypes.data if F0 else None, F0, LIES[lie],
             lv.ctypes.data, None if dk is None else dk.data_ptr(), k, index.data_ptr(), score.data_ptr(),
             score0.data_ptr(), pof0.data_ptr(), mean.data_ptr(), var.data_ptr(), fout.ctypes.data, C.byref(nf),
             C.byref(bout), C.byref(npk))
        torch.cuda.synchronize()
        n = npk.value
        score, score0, pof0, var = (a.cpu().numpy() for a in (score, score0, pof0, var))
        mean = mean.cpu().numpy().T * scales[:, 1] + scales[:, 0]                  # m x q, raw
        unit = {"cei": scales[objs[0], 1] if objs else 1.0, "ehvi": np.prod(scales[objs, 1]) if objs else 1.0}.get(criterion, 1.0)
        fo, bo = None, None
        if criterion == "ehvi":
            fo = fout[:nf.value] * scales[objs, 1] + scales[objs, 0]
        if criterion in ("cei", "cpi"):
            bo = bout.value * scales[objs[0], 1] + scales[objs[0], 0]
        return AcquireMultiResult(index=index.cpu().numpy()[:n].copy(), score=unit * score[:n], score0=unit * score0,
                                  pof0=pof0, mean=mean, var=var, scale=scales[:, 1].copy(), front=fo, best=bo,
                                  criterion=criterion, n_picked=n, k=k)

    # -- acquisition gradients ---------------------------------------------------------------
    @staticmethod
    def _chunk_rows(chunk_rows):
        chunk_rows = int(chunk_rows)
        if chunk_rows < 0 or chunk_rows % 128:
            raise ValueError("chunk_rows must be 0 (the library's choice) or a positive multiple of 128")
        return chunk_rows

    def var_grad(self, x, noise=False, chunk_rows=0):
        """The latent variance d_i = b_i^T inv(H) b_i at the rows x (n x d) -- the full posterior covariance, what
        select and acquire score with; noise=True adds e^{2 sigma} -- and its gradient by the inputs,
        dd_i/dx = 2 (db_i/dx)^T inv(H) b_i -> (var (n), grad (n x d)), standardised units.  A row with a coordinate
        that is not finite gets NaN.  inv(H) is formed by the first call on this posterior and kept with it.
        chunk_rows bounds the workspace (two blocks of pad128(p) x chunk_rows doubles): 0 = the library's choice,
        otherwise a positive multiple of 128; the result does not depend on it, bit for bit."""
        import torch
        self._need()
        x = _rows(self.om, x, "x")
        chunk_rows = self._chunk_rows(chunk_rows)
        n, d = x.shape
        if n == 0:
            return np.zeros(0), np.zeros((0, d))
        dev = _stream()
        dx = _dev_cols(x, dev)
        var = torch.empty(n, dtype=torch.float64, device=dev)
        grad = torch.empty((d, n), dtype=torch.float64, device=dev)
        call("obhip_posterior_var_grad_dev", self._h, dx.data_ptr(), n, chunk_rows, int(bool(noise)), var.data_ptr(),
             grad.data_ptr())
        torch.cuda.synchronize()
        return var.cpu().numpy(), grad.cpu().numpy().T.copy()

    # -- the term-count path (include/obhip.h, "term-count path") ------------------------------
    def _path_dev(self, A, what):
        """A (p x q, or p) -> device tensor (q, p): column-major p x q"""
        import torch
        A = np.asarray(A, dtype=np.float64)
        A = A[:, None] if A.ndim == 1 else A
        if A.ndim != 2 or A.shape[0] != self.p or A.shape[1] == 0:
            raise ValueError("%s must be p x q" % what)
        return torch.from_numpy(np.ascontiguousarray(A.T)).to(_stream())

    def term_path_coef(self, G):
        """U = L^-1 G (p x q) for the right-hand sides G = e^{-2 sigma} B^T y (p x q, y standardised): the
        coefficients of the path, U[:k] those of the model of the first k terms."""
        import torch
        self._need()
        dG = self._path_dev(G, "G")
        dU = torch.empty_like(dG)
        call("obhip_posterior_path_coef_dev", self._h, dG.data_ptr(), dG.shape[0], dU.data_ptr())
        torch.cuda.synchronize()
        return dU.cpu().numpy().T.copy()

    def term_path_theta(self, U, k):
        """The coefficients theta_k = inv(H[:k,:k]) G[:k] of the model of the first k terms (p x q, zeros behind
        row k) from U = term_path_coef(G)."""
        import torch
        self._need()
        dU = self._path_dev(U, "U")
        dT = torch.empty_like(dU)
        call("obhip_posterior_path_theta_dev", self._h, dU.data_ptr(), dU.shape[0], int(k), dT.data_ptr())
        torch.cuda.synchronize()
        return dT.cpu().numpy().T.copy()

    def term_path_evidence(self, U, prec, yty, n_rows, step=16):
        """log p(y | first k terms) at every checkpoint k = step, 2 step, ..., p (K x q) for the STANDARDISED
        response: prec (p) the prior precisions of the terms, yty (q) = y^T y of the standardised response over
        the n_rows rows of the fit."""
        self._need()
        dU = self._path_dev(U, "U")
        q = dU.shape[0]
        prec = np.ascontiguousarray(prec, dtype=np.float64)
        yty = np.ascontiguousarray(np.atleast_1d(yty), dtype=np.float64)
        if prec.shape != (self.p,) or yty.shape != (q,):
            raise ValueError("prec must have p entries and yty q")
        K = C.c_uint64(0)
        call("obhip_term_path_layout", self.p, q, int(step), 0, 0, C.byref(K), None, None)
        out = np.empty((K.value, q))
        call("obhip_posterior_path_evidence", self._h, dU.data_ptr(), q, prec.ctypes.data, yty.ctypes.data, int(n_rows),
             int(step), out.ctypes.data)
        return out

    def _term_path_scores_dev(self, dU, dx, n, dY, dmeansd, step, loo, chunk_rows):
        """device tensors in (dU (q, p), dx (d, n), dY (q, n), dmeansd (q, 3) or None) -> scores (K, q, 3), sumv (K)"""
        import torch
        q = dU.shape[0]
        K = C.c_uint64(0)
        call("obhip_term_path_layout", self.p, q, int(step), n, chunk_rows, C.byref(K), None, None)
        scores = torch.empty((K.value, q, 3), dtype=torch.float64, device=dU.device)
        sumv = torch.empty(K.value, dtype=torch.float64, device=dU.device)
        call("obhip_posterior_path_scores_dev", self._h, dU.data_ptr(), q, None if n == 0 else dx.data_ptr(), n,
             None if n == 0 else dY.data_ptr(), n, None if dmeansd is None else dmeansd.data_ptr(), int(step),
             int(bool(loo)), chunk_rows, scores.data_ptr(), sumv.data_ptr())
        torch.cuda.synchronize()
        return scores.cpu().numpy(), sumv.cpu().numpy()

    def term_path_scores(self, U, x, Y, step=16, loo=False, chunk_rows=0, meansd=None):
        """The scores of the model of the first k terms at every checkpoint k = step, 2 step, ..., p, summed over
        the rows x (n x d) with responses Y (n x q) -> (scores (K x q x 3): sse, spe, lpd; sumv (K)), standardised
        units.  loo=False: rows that are not in the fit, e = r = y - mean_k, s^2 = e^{2 sigma} + v_k.  loo=True: rows
        of the fit, each once: the leave-one-out residual e = r / (1 - h) and variance e^{2 sigma} / (1 - h),
        h = v_k e^{-2 sigma}, the standardisation of the response held fixed.  Y is standardised already unless
        meansd (q x 3: centre, scale, rows) is given.  One factor and one pass over the rows serve every k;
        chunk_rows as in var_grad: the result does not depend on it, bit for bit."""
        import torch
        self._need()
        x = _rows(self.om, x, "x")
        chunk_rows = self._chunk_rows(chunk_rows)
        dU = self._path_dev(U, "U")
        q, n = dU.shape[0], x.shape[0]
        Y = np.asarray(Y, dtype=np.float64)
        Y = Y[:, None] if Y.ndim == 1 else Y
        if Y.shape != (n, q):
            raise ValueError("Y must be n x q")
        dev = dU.device
        dm = None
        if meansd is not None:
            meansd = np.ascontiguousarray(meansd, dtype=np.float64)
            if meansd.shape != (q, 3):
                raise ValueError("meansd must be q x 3")
            dm = torch.from_numpy(meansd).to(dev)
        dx = _dev_cols(x, dev) if n else None
        dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev) if n else None
        return self._term_path_scores_dev(dU, dx, n, dY, dm, step, loo, chunk_rows)

    def _acquire_args(self, criterion, best, level, kappa, xi, response, lie_value=None):
        """the criterion's parameters (and acquire's lie_value), checked and standardised:
        (best, xi, kappa, level), lie_value, (centre, scale) or None"""
        if criterion not in ACQUISITIONS:
            raise ValueError("criterion must be one of %s" % sorted(ACQUISITIONS))
        if criterion in ("ei", "pi") and best is None:
            raise ValueError("criterion %r needs best, the incumbent" % criterion)
        if criterion == "straddle" and level is None:
            raise ValueError("criterion 'straddle' needs level")
        best, level = 0.0 if best is None else float(best), 0.0 if level is None else float(level)
        kappa, xi, lie = float(kappa), float(xi), 0.0 if lie_value is None else float(lie_value)
        if not all(np.isfinite(v) for v in (best, level, lie, xi)):
            raise ValueError("best, level%s and xi must be finite" % ("" if lie_value is None else ", lie_value"))
        if not (np.isfinite(kappa) and kappa >= 0):
            raise ValueError("kappa must be finite and >= 0")
        sc = self._scale(response)
        if sc is not None:                                       # raw units -> standardised
            best, level, lie, xi = (best - sc[0]) / sc[1], (level - sc[0]) / sc[1], (lie - sc[0]) / sc[1], xi / sc[1]
        return (best, xi, kappa, level), lie, sc

    @staticmethod
    def _acquire_raw(sc, criterion, maximize, mean, var, *scores):
        """standardised -> raw units of the response with (centre, scale) sc: -> (mean, var, scores); pi has no unit"""
        if sc is None:
            return mean, var, scores
        if criterion in ("ei", "straddle"):
            scores = [sc[1] * s for s in scores]
        elif criterion == "lcb":                                 # kappa sd - mu: the centre comes back with the sign of -mu
            off = sc[0] if maximize else -sc[0]
            scores = [sc[1] * s + off for s in scores]
        return sc[0] + sc[1] * mean, sc[1] ** 2 * var, scores

    def acquire_grad(self, x, theta, criterion="ei", best=None, level=None, kappa=1.96, xi=0.0, maximize=False,
                     response=None, chunk_rows=0):
        """An acquisition criterion and its gradient by the inputs at the rows x (n x d): what moves a point
        continuously to where the criterion is best (screen a candidate cloud with acquire, then refine the best
        starts by gradient ascent on score).  theta (p): the standardised coefficients of one response.  With the
        latent mean mu = b^T theta, the latent variance d = b^T inv(H) b (without the noise), sd = sqrt(max(d, 0)),
        dsd = dd / (2 sd), written for minimisation (maximize=True: the same on -mu, -best, -level), t = best - xi
        - mu, u = t / sd:
          "ei"        score t Phi(u) + sd phi(u)     gradient -Phi(u) dmu + phi(u) dsd        (best required)
          "pi"        score Phi(u)                   gradient phi(u) (-dmu - u dsd) / sd      (best required)
          "lcb"       score kappa sd - mu            gradient kappa dsd - dmu
          "straddle"  score kappa sd - |mu - level|  gradient kappa dsd - sign(mu - level) dmu  (level required)
        sign(0) = 0.  Where d <= 0, dsd is taken as 0 and the scores are acquire's sd = 0 branches: the ei gradient
        is -dmu where t > 0 and 0 elsewhere, the pi gradient 0.  A row with a coordinate that is not finite gets NaN
        in every output.  The scores are those of acquire(k=1).score0 up to rounding (acquire sums d in another
        order).
        response=j on a posterior that carries meansd: best, level and xi are given in raw units of response j and
        standardised on the way in; with sca the response's scale, mean, score (ei, lcb, straddle) and their
        gradients come back times sca, var and its gradient times sca^2, pi is left alone; the centre is added to
        mean and to the lcb score and has no gradient.
        inv(H) is formed by the first call on this posterior and kept with it.  chunk_rows bounds the workspace
        (two blocks of pad128(p) x chunk_rows doubles): 0 = the library's choice, otherwise a positive multiple of
        128; the result does not depend on it, bit for bit.  Two calls give the same bits.
        -> AcquireGradResult(score (n), grad (n x d), mean (n), grad_mean (n x d), var (n), grad_var (n x d),
        criterion)"""
        import torch
        self._need()
        x = _rows(self.om, x, "x")
        chunk_rows = self._chunk_rows(chunk_rows)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (self.p,):
            raise ValueError("theta must be the p standardised coefficients of one response")
        pars, _, sc = self._acquire_args(criterion, best, level, kappa, xi, response)
        n, d = x.shape
        if n == 0:
            z1, z2 = np.zeros(0), np.zeros((0, d))
            return AcquireGradResult(score=z1, grad=z2, mean=z1.copy(), grad_mean=z2.copy(), var=z1.copy(),
                                     grad_var=z2.copy(), criterion=criterion)
        dev = _stream()
        dx = _dev_cols(x, dev)
        dth = torch.from_numpy(theta).to(dev)
        score, mean, var = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        grad, gmean, gvar = (torch.empty((d, n), dtype=torch.float64, device=dev) for _ in range(3))
        call("obhip_acquire_grad_dev", self._h, dth.data_ptr(), dx.data_ptr(), n, ACQUISITIONS[criterion],
             (C.c_double * 4)(*pars), int(bool(maximize)), chunk_rows, score.data_ptr(), grad.data_ptr(),
             mean.data_ptr(), gmean.data_ptr(), var.data_ptr(), gvar.data_ptr())
        torch.cuda.synchronize()
        score, mean, var = (a.cpu().numpy() for a in (score, mean, var))
        grad, gmean, gvar = (a.cpu().numpy().T.copy() for a in (grad, gmean, gvar))
        mean, var, (score,) = self._acquire_raw(sc, criterion, maximize, mean, var, score)
        if sc is not None:                                       # the gradients take the scales, not the centre
            gmean, gvar = sc[1] * gmean, sc[1] ** 2 * gvar
            if criterion != "pi":
                grad = sc[1] * grad
        return AcquireGradResult(score=score, grad=grad, mean=mean, grad_mean=gmean, var=var, grad_var=gvar,
                                 criterion=criterion)

    def acquire_grad_layout(self):
        """-> (fused, lds_bytes, default_chunk_rows): whether var_grad / acquire_grad keep their tile in LDS on this
        posterior's terms, the LDS of a workgroup, and the rows chunk_rows=0 stands for"""
        self._need()
        _stream()
        fused, lds, rows = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        call("obhip_acquire_grad_layout", self._h, C.byref(fused), C.byref(lds), C.byref(rows))
        return bool(fused.value), lds.value, rows.value

    # -- draws -------------------------------------------------------------------------------
    def _draw_args(self, theta, n_draws, seed, z):
        """the host side of the draws' arguments, checked: (theta, z^T or None, S, seed)"""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.shape != (self.p,):
            raise ValueError("theta must be the p standardised coefficients of one response")
        if (z is None) == (n_draws is None):
            raise ValueError("give exactly one of z (p x S) and n_draws")
        if z is not None:
            z = np.asarray(z, dtype=np.float64)
            if z.ndim != 2 or z.shape[0] != self.p or z.shape[1] < 1:
                raise ValueError("z must be p x S with S >= 1")
            return theta, np.ascontiguousarray(z.T), z.shape[1], None       # row s = column s of z
        if int(n_draws) < 1:
            raise ValueError("n_draws must be >= 1")
        if seed is None:
            raise ValueError("n_draws needs a seed")
        return theta, None, int(n_draws), int(seed)

    def _draw_dev(self, args, dev):
        """(d_theta, d_Z: column-major p x S with leading dimension p, S)"""
        import torch
        theta, zt, S, seed = args
        if zt is not None:
            dz = torch.from_numpy(zt).to(dev)
        else:
            gen = torch.Generator(dev).manual_seed(seed)
            dz = torch.randn(self.p, S, dtype=torch.float64, device=dev, generator=gen).t().contiguous()
        return torch.from_numpy(theta).to(dev), dz, S

    def _scale(self, response):
        """(centre, scale) the sample paths of `response` are de-standardised with, or None"""
        if response is None or self.meansd is None:
            return None
        cen, sca = float(self.meansd[int(response), 0]), float(self.meansd[int(response), 1])
        if not sca > 0:
            raise ValueError("response %d has scale %g: nothing to de-standardise with" % (int(response), sca))
        return cen, sca

    def draw(self, theta, n_draws=None, seed=None, z=None):
        """Coefficient draws theta + L^-T z_s from N(theta, inv(H)) -> p x S, standardised units.  theta: the p
        standardised coefficients of one response (MultiFit.coeff[:, j]).  Exactly one of z (p x S normals)
        and n_draws: with n_draws, Z = torch.randn(p, S, float64, on the device) from
        torch.Generator(device).manual_seed(seed).  A seed reproduces on the same torch build only; z= is the
        portable form."""
        import torch
        self._need()
        args = self._draw_args(theta, n_draws, seed, z)
        dev = _stream()
        dth, dz, S = self._draw_dev(args, dev)
        out = torch.empty((S, self.p), dtype=torch.float64, device=dev)
        call("obhip_posterior_draw_dev", self._h, dth.data_ptr(), dz.data_ptr(), self.p, S, out.data_ptr())
        torch.cuda.synchronize()
        return out.cpu().numpy().T.copy()

    def sample(self, x, theta, n_draws=None, seed=None, z=None, response=None):
        """Joint sample paths B(x) (theta + L^-T z_s) at the rows x (n x d) -> n x S.  Arguments as draw (a seed
        reproduces on the same torch build only; z= is the portable form).  response=j on a posterior that
        carries meansd: the paths are de-standardised with row j (centre + scale * path); otherwise they stay in
        standardised units."""
        import torch
        self._need()
        x = _rows(self.om, x, "x")
        sc = self._scale(response)
        args = self._draw_args(theta, n_draws, seed, z)
        n = x.shape[0]
        if n == 0:
            return np.zeros((0, args[2]))
        dev = _stream()
        dth, dz, S = self._draw_dev(args, dev)
        dx = _dev_cols(x, dev)
        out = torch.empty((S, n), dtype=torch.float64, device=dev)
        call("obhip_posterior_sample_dev", self._h, dth.data_ptr(), dz.data_ptr(), self.p, S, dx.data_ptr(), n,
             out.data_ptr())
        torch.cuda.synchronize()
        path = out.cpu().numpy().T.copy()
        return path if sc is None else sc[0] + sc[1] * path

    def thompson(self, xcand, theta, n_draws=None, seed=None, z=None, maximize=False, skip=None, response=None):
        """Per draw the candidate row of xcand (m x d) at which its sample path is smallest (maximize=True:
        largest) and the path there -> ThompsonResult.  Arguments as draw (a seed reproduces on the same torch
        build only; z= is the portable form).  skip (m, nonzero = leave out): rows that are never chosen, like
        rows with a coordinate that is not finite.  The lowest index wins among equal values.  response=j on a
        posterior that carries meansd de-standardises value with row j; its scale is positive, so the optimum
        does not move."""
        import torch
        self._need()
        xcand = _rows(self.om, xcand, "xcand")
        m = xcand.shape[0]
        if m == 0:
            raise ValueError("thompson needs candidates")
        if skip is not None:
            skip = np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8)
            if skip.shape != (m,):
                raise ValueError("skip must have one entry per candidate")
        sc = self._scale(response)
        args = self._draw_args(theta, n_draws, seed, z)
        dev = _stream()
        dth, dz, S = self._draw_dev(args, dev)
        dx = _dev_cols(xcand, dev)
        dk = torch.from_numpy(skip).to(dev) if skip is not None else None
        index = torch.full((S,), -1, dtype=torch.int64, device=dev)
        value = torch.full((S,), float("nan"), dtype=torch.float64, device=dev)
        call("obhip_posterior_extremum_dev", self._h, dth.data_ptr(), dz.data_ptr(), self.p, S, dx.data_ptr(), m,
             None if dk is None else dk.data_ptr(), int(bool(maximize)), index.data_ptr(), value.data_ptr())
        torch.cuda.synchronize()
        index, value = index.cpu().numpy(), value.cpu().numpy()
        if sc is not None:
            value = sc[0] + sc[1] * value
        picks, first, counts = np.unique(index[index >= 0], return_index=True, return_counts=True)
        order = np.argsort(first, kind="stable")
        return ThompsonResult(index=index, value=value, picks=picks[order], counts=counts[order],
                              maximize=bool(maximize), n_draws=S)
