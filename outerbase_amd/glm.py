"""Newton fit of weighted Gaussian, binomial and Poisson responses (IRLS).

Rows with prior weights (replicates, known heteroscedastic noise), proportions out of m trials and
counts with an exposure offset are one computation: Newton's method on the penalised log-likelihood
sum_i a_i l(y_i, o_i + (B theta)_i) - theta^T P theta / 2, every step the library's Newton step with
B^T B replaced by B^T W B (include/obhip.h, "weighted, binomial and Poisson responses").  One
response, all rows on one device.

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C
import math

import numpy as np

from . import obmod
from ._lib import call
from .multi import DEFAULT_RHO

FAMILIES = {"gaussian": 0, "binomial": 1, "poisson": 2}  # OBHIP_GLM_*


class GlmInfo(C.Structure):
    """obhip_glm_info"""
    _fields_ = [("warm_start", C.c_int), ("converged", C.c_int), ("iterations", C.c_uint64),
                ("halvings", C.c_uint64), ("dec", C.c_double), ("F", C.c_double), ("deviance", C.c_double)]


def _family(family):
    if family not in FAMILIES:
        raise ValueError("family must be one of %s" % sorted(FAMILIES))
    return FAMILIES[family]


def _check_offset(offset, n):
    if offset is None:
        return None
    offset = np.ascontiguousarray(offset, dtype=np.float64)
    if offset.shape != (n,):
        raise ValueError("offset must have one entry per row")
    if not np.all(np.isfinite(offset)):
        raise ValueError("offset must be finite")
    return offset


def _check_glm(om, x, y, family, weights, offset):
    """arguments of fit_glm checked on the host, before any device call (as multi._check_xy does)"""
    fam = _family(family)
    x = np.asarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != om.d:
        raise ValueError("x must be n x d")
    n = x.shape[0]
    if n == 0:
        raise ValueError("x has no rows")
    if y.shape != (n,):
        raise ValueError("y must have one entry per row of x")
    if not np.all(np.isfinite(y)):
        raise ValueError("y must be finite")
    if family == "binomial" and not np.all((y >= 0.0) & (y <= 1.0)):
        raise ValueError("binomial y are proportions in [0, 1] (weights = trials)")
    if family == "poisson" and not np.all(y >= 0.0):
        raise ValueError("poisson y must be >= 0")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (n,):
            raise ValueError("weights must have one entry per row")
        if not np.all(np.isfinite(weights) & (weights > 0.0)):
            raise ValueError("weights must be finite and > 0")
    return fam, x, y, weights, _check_offset(offset, n)


class GlmFit:
    """Result of fit_glm: coeff (p), diagH (p: the diagonal of the last Hessian), iterations, halvings,
    converged, deviance, logpost (the penalised log-likelihood at coeff), eta (n: the fitted linear
    predictor, offset included)."""

    def __init__(self, om, t, family, coeff, diagH, eta, info, sigma, rho):
        self.om, self._t, self.family = om, t, family
        self.coeff, self.diagH, self.eta = coeff, diagH, eta
        self.iterations, self.halvings = int(info.iterations), int(info.halvings)
        self.converged = bool(info.converged)
        self.deviance, self.logpost, self.dec = float(info.deviance), float(info.F), float(info.dec)
        self.sigma, self.rho = sigma, rho

    def predict(self, xnew, offset=None, kind="response", var=False):
        """The mean at xnew on the response scale (kind="response": the inverse link of the linear
        predictor) or the linear predictor itself (kind="link"), offset added; with var=True also its
        variance: B^2 (1 / diagH) on the link scale, (d mu / d eta)^2 times that on the response scale
        (delta method)."""
        if kind not in ("response", "link"):
            raise ValueError('kind must be "response" or "link"')
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim != 2 or xnew.shape[1] != self.om.d:
            raise ValueError("xnew must be n x d")
        n = xnew.shape[0]
        offset = _check_offset(offset, n)
        if n == 0:
            z = np.zeros(0)
            return (z, z.copy()) if var else z
        import torch
        f64 = torch.float64
        dev = torch.device("cuda", torch.cuda.current_device())
        call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
        dx = torch.from_numpy(np.ascontiguousarray(xnew.T)).to(dev)
        dth = torch.from_numpy(np.ascontiguousarray(self.coeff)).to(dev)
        do = None if offset is None else torch.from_numpy(offset).to(dev)
        dcv = torch.from_numpy(1.0 / self.diagH).to(dev) if var else None
        link = kind == "link"
        out = torch.empty(n, dtype=f64, device=dev)
        vout = torch.empty(n, dtype=f64, device=dev) if var else None

        def p(tensor):
            return None if tensor is None else tensor.data_ptr()
        call("obhip_predict_glm_dev", self.om._h, self._t._h, FAMILIES[self.family], dth.data_ptr(), dx.data_ptr(), n,
             p(do), p(dcv), p(out) if link else None, p(vout) if link else None, None if link else p(out),
             None if link else p(vout))
        torch.cuda.synchronize()
        return (out.cpu().numpy(), vout.cpu().numpy()) if var else out.cpu().numpy()


def fit_glm(om, terms, x, y, family="binomial", weights=None, offset=None, sigma=None, rho=DEFAULT_RHO, tol=1e-8,
            maxit=25):
    """Maximise sum_i weights_i l(y_i, offset_i + (B theta)_i) - theta^T P theta / 2 over theta by Newton's
    method with a halving line search (obhip_fit_glm_dev).  family: "gaussian" (identity link; sigma, the log
    noise standard deviation, defaults to log(0.01) as in fit_newton_multi; y standardised by the caller),
    "binomial" (logit link; y proportions in [0, 1], weights = trials) or "poisson" (log link; y >= 0, offset =
    log exposure).  tol: the fit has converged when the Newton decrement g^T delta <= tol (1 + |F|)."""
    fam, x, y, weights, offset = _check_glm(om, x, y, family, weights, offset)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise ValueError("tol must be finite and >= 0")
    if int(maxit) < 1:
        raise ValueError("maxit must be >= 1")
    if sigma is None:
        sigma = math.log(0.01)
    import torch
    t = obmod._terms_of(om, terms)
    n, p, f64 = x.shape[0], t.p, torch.float64
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    dy = torch.from_numpy(y).to(dev)
    da = None if weights is None else torch.from_numpy(weights).to(dev)
    do = None if offset is None else torch.from_numpy(offset).to(dev)
    caps = t.maxlevels()
    basis = C.c_void_p()
    call("obhip_basis_create_dev", C.byref(basis), om._h, dx.data_ptr(), n, caps.ctypes.data)
    info = GlmInfo()
    try:
        wsb = C.c_uint64(0)
        call("obhip_glm_workspace_bytes", p, n, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        H = torch.empty((p, p), dtype=f64, device=dev)
        theta = torch.empty(p, dtype=f64, device=dev)
        diagH = torch.empty(p, dtype=f64, device=dev)
        eta = torch.empty(n, dtype=f64, device=dev)
        call("obhip_fit_glm_dev", basis, t._h, om._h, fam, dy.data_ptr(), None if da is None else da.data_ptr(),
             None if do is None else do.data_ptr(), sigma, rho, tol, int(maxit), H.data_ptr(), theta.data_ptr(),
             diagH.data_ptr(), eta.data_ptr(), C.byref(info), ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
    finally:
        call("obhip_basis_destroy", basis)
    return GlmFit(om, t, family, theta.cpu().numpy(), diagH.cpu().numpy(), eta.cpu().numpy(), info, sigma, rho)
