"""Prediction on the product of two input blocks and the calibration likelihood built on it.

The emulator at every pair (row i of xa, row j of xb): the dimensions dims_b take their inputs from xb, all
others from xa.  Field settings x candidate parameters (calibration), control x environment (robust design),
grid x data rows (slices, ICE curves).  The na nb full-width rows are never written: a design-matrix entry is
a product over the dimensions, so the pair's mean is a matrix product of two on-the-fly operands
(include/obhip.h, "product of two input blocks").

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C
import math

import numpy as np

from . import obmod
from ._lib import call
from .multi import DEFAULT_RHO


def check_dims_b(d, dims_b):
    """dims_b as uint32: 0-based, strictly ascending, 1 to d - 1 entries below d"""
    db = np.asarray(dims_b)
    if db.ndim != 1 or db.size < 1 or db.size > d - 1 or not np.issubdtype(db.dtype, np.integer):
        raise ValueError("dims_b must name 1 to d - 1 dimensions (0-based integers)")
    if db.min() < 0 or db.max() >= d:
        raise ValueError("dims_b entry out of range")
    if np.any(np.diff(db) <= 0):
        raise ValueError("dims_b must be strictly ascending")
    return np.ascontiguousarray(db, dtype=np.uint32)


def check_blocks(d, xa, xb, dims_b):
    db = check_dims_b(d, dims_b)
    xa = np.asarray(xa, dtype=np.float64)
    xb = np.asarray(xb, dtype=np.float64)
    if xa.ndim != 2 or xa.shape[1] != d - db.size:
        raise ValueError("xa must be na x (d - len(dims_b))")
    if xb.ndim != 2 or xb.shape[1] != db.size:
        raise ValueError("xb must be nb x len(dims_b)")
    return xa, xb, db


def product_layout(om, terms, dims_b):
    """(mu_a, mu_b, fused): the used basis columns of the two sides and whether the fused kernel takes the
    split (obhip_product_layout; host only)"""
    t = obmod._terms_of(om, terms)
    db = check_dims_b(om.d, dims_b)
    ma, mb, fu = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    call("obhip_product_layout", t._h, db.ctypes.data, db.size, C.byref(ma), C.byref(mb), C.byref(fu))
    return ma.value, mb.value, bool(fu.value)


def product_fit_layout(om, terms, dims_b):
    """(mu_a, mu_b, fused_a, fused_b): the used basis columns of the two sides and whether the staging kernel of
    the gridded fit keeps that side's tile in LDS (obhip_product_fit_layout; host only)"""
    t = obmod._terms_of(om, terms)
    db = check_dims_b(om.d, dims_b)
    ma, mb, fa, fb = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_int(0)
    call("obhip_product_fit_layout", t._h, db.ctypes.data, db.size, C.byref(ma), C.byref(mb), C.byref(fa), C.byref(fb))
    return ma.value, mb.value, bool(fa.value), bool(fb.value)


def product_side(om, terms, x, dims_b, side, padded=False):
    """One side matrix of the gridded fit at the rows x: out[i, k] = s_i times the factors of term k on that
    side (side 0: x is xa, n x (d - len(dims_b)); side 1: x is xb, n x len(dims_b)), an (n, p) array -- the
    design-matrix entry of a pair is product_side(.., xa, .., 0)[i, k] * product_side(.., xb, .., 1)[j, k].
    padded=True: the staged layout itself, rows up to a multiple of 64 and columns up to one of 256, all zeros
    beyond (n, p) (obhip_product_side_dev)."""
    import torch
    t = obmod._terms_of(om, terms)
    db = check_dims_b(om.d, dims_b)
    if side not in (0, 1):
        raise ValueError("side must be 0 (A) or 1 (B)")
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != (db.size if side else om.d - db.size):
        raise ValueError("x must be n x (the dimensions of the side)")
    if not np.all(np.isfinite(x)):
        raise ValueError("x must be finite")
    n, p = x.shape[0], t.p
    rows, pitch = ((n + 63) // 64 * 64, (p + 255) // 256 * 256)
    if n == 0:
        return np.zeros((0, pitch if padded else p))
    dev = _device()
    # filled with NaN: what the kernel does not write shows
    out = torch.full((rows, pitch), float("nan"), dtype=torch.float64, device=dev)
    call("obhip_product_side_dev", om._h, t._h, db.ctypes.data, db.size, int(side), _cols(x, dev).data_ptr(), n,
         out.data_ptr(), pitch)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return out if padded else out[:n, :p].copy()


def fit_newton_product(om, terms, xa, xb, Y, dims_b, sigma=None, rho=DEFAULT_RHO):
    """The Newton fit of fit_newton_multi on the full grid xa x xb: Y[i, j] (na x nb, or na x nb x q) is the
    response at the pair (xa[i], xb[j]) -- an accumulator filled once by NewtonAccumulator.add_product, so the
    na nb full-width rows are never written.  -> MultiFit; fit.predict_product(xa, xb, dims_b) closes the loop."""
    from .stream import NewtonAccumulator
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim not in (2, 3):
        raise ValueError("Y must be na x nb (x q)")
    if Y.shape[0] * Y.shape[1] < 2:
        raise ValueError("a fit needs two observations")
    with NewtonAccumulator(om, terms, 1 if Y.ndim == 2 else Y.shape[2]) as acc:
        acc.add_product(xa, xb, Y, dims_b)
        return acc.fit(sigma=sigma, rho=rho)


def _device():
    import torch
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch.device("cuda", torch.cuda.current_device())


def _cols(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a.T)).to(dev)  # column-major


def predict_product_dev(om, t, Theta, xa, xb, db, coeffvar, sigma):
    """device tensors (mean q x nb x na, var nb x na or None) in standardised units"""
    import torch
    dev = _device()
    p, q = Theta.shape
    na, nb = xa.shape[0], xb.shape[0]
    mean = torch.empty((q, nb, na), dtype=torch.float64, device=dev)
    var = dcv = None
    if coeffvar is not None:
        dcv = torch.from_numpy(np.ascontiguousarray(coeffvar, dtype=np.float64)).to(dev)
        var = torch.empty((nb, na), dtype=torch.float64, device=dev)
    dxa, dxb, dth = _cols(xa, dev), _cols(xb, dev), _cols(Theta, dev)
    call("obhip_predict_product_dev", om._h, t._h, dth.data_ptr(), q, db.ctypes.data, db.size, dxa.data_ptr(), na,
         dxb.data_ptr(), nb, mean.data_ptr(), na, None if dcv is None else dcv.data_ptr(), sigma,
         None if var is None else var.data_ptr())
    return mean, var


def predict_product(om, terms, Theta, xa, xb, dims_b, coeffvar=None, sigma=None):
    """mean (na, nb, q) of the q coefficient vectors Theta (p x q, or p) at every pair (xa[i], xb[j]); with
    coeffvar (p) also the variance (na, nb) of the diagonal form B^2 coeffvar + e^{2 sigma}, returned as
    (mean, var).  Standardised units.  sigma=None: log(0.01)."""
    t = obmod._terms_of(om, terms)
    xa, xb, db = check_blocks(om.d, xa, xb, dims_b)
    Theta = np.asarray(Theta, dtype=np.float64)
    if Theta.ndim == 1:
        Theta = Theta[:, None]
    if Theta.ndim != 2 or Theta.shape[0] != t.p or Theta.shape[1] == 0:
        raise ValueError("Theta must be p x q")
    if coeffvar is not None:
        coeffvar = np.asarray(coeffvar, dtype=np.float64)
        if coeffvar.shape != (t.p,):
            raise ValueError("coeffvar must have p entries")
    if sigma is None:
        sigma = math.log(0.01)
    na, nb, q = xa.shape[0], xb.shape[0], Theta.shape[1]
    if na == 0 or nb == 0:
        z = np.zeros((na, nb, q))
        return z if coeffvar is None else (z, np.zeros((na, nb)))
    mean, var = predict_product_dev(om, t, Theta, xa, xb, db, coeffvar, float(sigma))
    mean = mean.permute(2, 1, 0).cpu().numpy()
    return mean if var is None else (mean, var.cpu().numpy().T)


class CalibrationLoglik:
    """loglik, chi2 = sum_i r_ij^2 / v_ij and logdet = sum_i log v_ij per candidate j, in raw units; from
    calibration_loglik(..., grad=True) also grad (nb x L) = d loglik_j / d t_j"""

    def __init__(self, loglik, chi2, logdet, grad=None):
        self.loglik, self.chi2, self.logdet = loglik, chi2, logdet
        if grad is not None:
            self.grad = grad


def product_grad_layout(om, terms, dims_b):
    """(mu_a, mu_b, view_terms, fused): product_layout's used columns, the (term, dimension of dims_b) pairs
    with a factor -- the inner dimensions of the gradient's view products, summed -- and whether the fused
    gradient kernel takes the split (obhip_product_grad_layout; host only)"""
    t = obmod._terms_of(om, terms)
    db = check_dims_b(om.d, dims_b)
    ma, mb, vt, fu = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    call("obhip_product_grad_layout", t._h, db.ctypes.data, db.size, C.byref(ma), C.byref(mb), C.byref(vt), C.byref(fu))
    return ma.value, mb.value, vt.value, bool(fu.value)


def predict_product_grad(om, terms, theta, xa, xb, dims_b, coeffvar=None, sigma=None):
    """dmean (na, nb, L): the derivative of the mean of the coefficient vector theta (p) at every pair
    (xa[i], xb[j]) by xb[j, l]; with coeffvar (p) also the derivative of predict_product's variance, returned as
    (dmean, dvar).  Standardised units -- obhip_predict_product_grad_dev."""
    import torch
    t = obmod._terms_of(om, terms)
    xa, xb, db = check_blocks(om.d, xa, xb, dims_b)
    theta = np.asarray(theta, dtype=np.float64)
    if theta.shape != (t.p,):
        raise ValueError("theta must have p entries")
    if coeffvar is not None:
        coeffvar = np.asarray(coeffvar, dtype=np.float64)
        if coeffvar.shape != (t.p,):
            raise ValueError("coeffvar must have p entries")
    if sigma is None:
        sigma = math.log(0.01)
    na, nb, L = xa.shape[0], xb.shape[0], db.size
    if na == 0 or nb == 0:
        z = np.zeros((na, nb, L))
        return z if coeffvar is None else (z, z.copy())
    dev = _device()
    vec = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dth, dcv = vec(theta), vec(coeffvar)
    dxa, dxb = _cols(xa, dev), _cols(xb, dev)
    dmean = torch.empty((L, nb, na), dtype=torch.float64, device=dev)
    dvar = None if dcv is None else torch.empty((L, nb, na), dtype=torch.float64, device=dev)
    call("obhip_predict_product_grad_dev", om._h, t._h, dth.data_ptr(), db.ctypes.data, db.size, dxa.data_ptr(), na,
         dxb.data_ptr(), nb, dmean.data_ptr(), na, None if dcv is None else dcv.data_ptr(), float(sigma),
         None if dvar is None else dvar.data_ptr())
    dmean = dmean.permute(2, 1, 0).cpu().numpy()
    return dmean if dvar is None else (dmean, dvar.permute(2, 1, 0).cpu().numpy())


def product_loglik_grad(om, terms, theta, xa, y, xb, dims_b, obsvar=None, coeffvar=None, sigma=None):
    """(chi2, logdet, dchi2, dlogdet): product_loglik's sums (nb each; on the fused kernel the same bits) and
    their derivatives by xb[j, l] (nb x L each) -- obhip_product_loglik_grad_dev"""
    import torch
    t = obmod._terms_of(om, terms)
    xa, xb, db = check_blocks(om.d, xa, xb, dims_b)
    theta, y, obsvar, coeffvar, sigma = _loglik_args(t, theta, xa, y, obsvar, coeffvar, sigma)
    na, nb, L = xa.shape[0], xb.shape[0], db.size
    if na == 0 or nb == 0:
        return np.zeros(nb), np.zeros(nb), np.zeros((nb, L)), np.zeros((nb, L))
    dev = _device()
    vec = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = product_loglik_grad_dev(om, t, vec(theta), _cols(xa, dev), vec(y), vec(obsvar), _cols(xb, dev), db,
                                  vec(coeffvar), sigma).cpu().numpy()
    return out[0].copy(), out[1].copy(), out[2:2 + L].T.copy(), out[2 + L:].T.copy()


def product_loglik_grad_dev(om, t, dth, dxa, dy, dov, dxb, db, dcv, sigma):
    """the (2 + 2 L) x nb device tensor of obhip_product_loglik_grad_dev from device tensors (dxa, dxb
    column-major: |A| x na, L x nb); nothing passes through the host"""
    import torch
    na, nb = dxa.shape[1], dxb.shape[1]
    out = torch.empty((2 + 2 * db.size, nb), dtype=torch.float64, device=dxb.device)
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    call("obhip_product_loglik_grad_dev", om._h, t._h, dth.data_ptr(), db.ctypes.data, db.size, dxa.data_ptr(), na,
         dy.data_ptr(), None if dov is None else dov.data_ptr(), dxb.data_ptr(), nb,
         None if dcv is None else dcv.data_ptr(), float(sigma), out.data_ptr())
    return out


def _loglik_args(t, theta, xa, y, obsvar, coeffvar, sigma):
    """the checks of product_loglik on everything but the blocks"""
    theta = np.asarray(theta, dtype=np.float64)
    if theta.shape != (t.p,):
        raise ValueError("theta must have p entries")
    y = np.asarray(y, dtype=np.float64)
    na = xa.shape[0]
    if y.shape != (na,):
        raise ValueError("y must have one entry per row of xa")
    if not np.all(np.isfinite(y)):
        raise ValueError("y must be finite")
    if obsvar is not None:
        obsvar = np.asarray(obsvar, dtype=np.float64)
        if obsvar.shape != (na,):
            raise ValueError("obsvar must have one entry per row of xa")
        if not np.all(np.isfinite(obsvar)) or np.any(obsvar < 0):
            raise ValueError("obsvar must be finite and not negative")
    if coeffvar is not None:
        coeffvar = np.asarray(coeffvar, dtype=np.float64)
        if coeffvar.shape != (t.p,):
            raise ValueError("coeffvar must have p entries")
    return theta, y, obsvar, coeffvar, math.log(0.01) if sigma is None else float(sigma)


def product_loglik(om, terms, theta, xa, y, xb, dims_b, obsvar=None, coeffvar=None, sigma=None):
    """(chi2, logdet), nb each, of the standardised field data y (na) at the settings xa for every candidate
    row of xb: r = y - mean, v = var + obsvar (var = e^{2 sigma} without coeffvar) -- obhip_product_loglik_dev"""
    import torch
    t = obmod._terms_of(om, terms)
    xa, xb, db = check_blocks(om.d, xa, xb, dims_b)
    theta, y, obsvar, coeffvar, sigma = _loglik_args(t, theta, xa, y, obsvar, coeffvar, sigma)
    na, nb = xa.shape[0], xb.shape[0]
    if na == 0 or nb == 0:
        return np.zeros(nb), np.zeros(nb)
    dev = _device()
    vec = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dth, dy, dov, dcv = vec(theta), vec(y), vec(obsvar), vec(coeffvar)
    dxa, dxb = _cols(xa, dev), _cols(xb, dev)
    out = torch.empty((2, nb), dtype=torch.float64, device=dev)
    call("obhip_product_loglik_dev", om._h, t._h, dth.data_ptr(), db.ctypes.data, db.size, dxa.data_ptr(), na,
         dy.data_ptr(), None if dov is None else dov.data_ptr(), dxb.data_ptr(), nb,
         None if dcv is None else dcv.data_ptr(), float(sigma), out.data_ptr())
    out = out.cpu().numpy()
    return out[0].copy(), out[1].copy()
