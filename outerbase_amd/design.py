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

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C

import numpy as np

from . import obmod
from ._lib import call, lib

CRITERIA = {"maxvar": 0, "imse": 1}


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
