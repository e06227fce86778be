"""Newton fit and prediction of several responses over one design.

Computer codes rarely return one number: q outputs (time steps, sensors, grid cells) over the
same inputs x share the model, the term set, sigma and rho, hence the Gram B^T B, the Hessian
and its Cholesky factor.  fit_newton_multi forms those once and batches what depends on Y over
the responses (include/obhip.h, "several responses over one design"); every response is
standardised on its own as obfit standardises its y (R/fitting.R:55-57).

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C
import math

import numpy as np

from . import obmod
from ._lib import call

DEFAULT_RHO = 6.0  # logpr_gauss.cpp:48


def _check_xy(om, x, Y, min_rows=2):
    x = np.asarray(x, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    if x.ndim != 2 or x.shape[1] != om.d:
        raise ValueError("x must be n x d")
    if Y.ndim != 2:
        raise ValueError("Y must be n x q")
    if Y.shape[0] != x.shape[0]:
        raise ValueError("Y has %d rows, x has %d" % (Y.shape[0], x.shape[0]))
    if Y.shape[1] == 0:
        raise ValueError("Y has no columns")
    if x.shape[0] < min_rows:
        raise ValueError("the standard deviation of a response needs two rows")
    if not np.all(np.isfinite(Y)):
        raise ValueError("Y must be finite")
    return x, Y


class MultiFit:
    """Result of fit_newton_multi: coeff (p x q), y_cent / y_sca (q each), diagH (p)."""

    def __init__(self, om, t, coeff, meansd, diagH, sigma, rho):
        self.om, self._t = om, t
        self.coeff = coeff
        self.y_cent = meansd[:, 0].copy()
        self.y_sca = meansd[:, 1].copy()
        self._meansd = meansd
        self.diagH = diagH
        self.sigma, self.rho = sigma, rho
        self.q = coeff.shape[1]

    def predict(self, xnew, var=False):
        """De-standardised mean (n x q) at xnew; with var=True also the predictive variance
        (n x q) of the diagonal form B^2 coeffvar + e^{2 sigma} (obhip_predict_dev) with
        coeffvar = 1 / diagH, scaled by the square of every response's standard deviation."""
        import torch
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim != 2 or xnew.shape[1] != self.om.d:
            raise ValueError("xnew must be n x d")
        n, q, f64 = xnew.shape[0], self.q, torch.float64
        if n == 0:
            z = np.zeros((0, q))
            return (z, z.copy()) if var else z
        dev = torch.device("cuda", torch.cuda.current_device())
        call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
        dx = torch.from_numpy(np.ascontiguousarray(xnew.T)).to(dev)          # column-major n x d
        dth = torch.from_numpy(np.ascontiguousarray(self.coeff.T)).to(dev)   # column-major p x q
        dms = torch.from_numpy(np.ascontiguousarray(self._meansd)).to(dev)
        mean = torch.empty((q, n), dtype=f64, device=dev)
        dcv = dvar = None
        if var:
            dcv = torch.from_numpy(1.0 / self.diagH).to(dev)
            dvar = torch.empty(n, dtype=f64, device=dev)
        call("obhip_predict_multi_dev", self.om._h, self._t._h, dth.data_ptr(), q, dx.data_ptr(), n,
             mean.data_ptr(), None if dcv is None else dcv.data_ptr(), self.sigma,
             None if dvar is None else dvar.data_ptr())
        call("obhip_destandardise_multi_dev", mean.data_ptr(), n, q, n, dms.data_ptr(), 0)
        if not var:
            return mean.cpu().numpy().T
        vq = dvar.repeat(q, 1).contiguous()
        call("obhip_destandardise_multi_dev", vq.data_ptr(), n, q, n, dms.data_ptr(), 1)
        return mean.cpu().numpy().T, vq.cpu().numpy().T

    def _dev_inputs(self, xnew):
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
        dx = torch.from_numpy(np.ascontiguousarray(xnew.T)).to(dev)          # column-major n x d
        dth = torch.from_numpy(np.ascontiguousarray(self.coeff.T)).to(dev)   # column-major p x q
        return dev, dx, dth

    def predict_grad(self, xnew, var=False):
        """De-standardised (mean n x q, grad n x d x q) at xnew, grad[i, l, j] = d mean_ij / d x_il;
        with var=True also (var n x q, gradvar n x d x q).  The means and gradients of all q responses
        come from one obhip_predict_jac_multi_dev call, which evaluates the basis and forms every term
        product once; the variance and its gradient, the same for every response in standardised
        units, come from one obhip_predict_grad_dev call with response 0 (its mean and gradient are
        discarded, so var=True and var=False return the same mean and grad bits) and are scaled by
        y_sca^2 as predict does with the variance."""
        import torch
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim != 2 or xnew.shape[1] != self.om.d:
            raise ValueError("xnew must be n x d")
        n, q, d, f64 = xnew.shape[0], self.q, self.om.d, torch.float64
        if n == 0:
            z, g = np.zeros((0, q)), np.zeros((0, d, q))
            return (z, g, z.copy(), g.copy()) if var else (z, g)
        dev, dx, dth = self._dev_inputs(xnew)
        mean = torch.empty((q, n), dtype=f64, device=dev)
        grad = torch.empty((q, d, n), dtype=f64, device=dev)
        call("obhip_predict_jac_multi_dev", self.om._h, self._t._h, dth.data_ptr(), q, dx.data_ptr(), n,
             mean.data_ptr(), grad.data_ptr())
        if var:
            dcv = torch.from_numpy(1.0 / self.diagH).to(dev)
            dvar = torch.empty(n, dtype=f64, device=dev)
            dgv = torch.empty((d, n), dtype=f64, device=dev)
            g0 = torch.empty((d, n), dtype=f64, device=dev)
            call("obhip_predict_grad_dev", self.om._h, self._t._h, dth[0].data_ptr(), dx.data_ptr(), n,
                 None, g0.data_ptr(), dcv.data_ptr(), self.sigma, dvar.data_ptr(), dgv.data_ptr())
        sca = torch.from_numpy(self.y_sca).to(dev)
        cent = torch.from_numpy(self.y_cent).to(dev)
        mean = mean * sca[:, None] + cent[:, None]
        grad = grad * sca[:, None, None]
        out = (mean.cpu().numpy().T, grad.permute(2, 1, 0).cpu().numpy())
        if not var:
            return out
        s2 = sca * sca
        return out + ((dvar[None, :] * s2[:, None]).cpu().numpy().T,
                      (dgv[None, :, :] * s2[:, None, None]).permute(2, 1, 0).cpu().numpy())

    def vjp(self, xnew, cot):
        """sum_j cot[i, j] d mean_ij / d x_il (n x d) of the de-standardised means: the backward pass of
        predict for the cotangent cot (n x q, raw units), scaled by y_sca per response and sent through
        obhip_predict_vjp_multi_dev; the n x d x q Jacobian is never formed."""
        import torch
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim != 2 or xnew.shape[1] != self.om.d:
            raise ValueError("xnew must be n x d")
        cot = np.asarray(cot, dtype=np.float64)
        n, q, d = xnew.shape[0], self.q, self.om.d
        if cot.shape != (n, q):
            raise ValueError("cot must be n x q")
        if n == 0:
            return np.zeros((0, d))
        dev, dx, dth = self._dev_inputs(xnew)
        dw = torch.from_numpy(np.ascontiguousarray(cot.T)).to(dev) * torch.from_numpy(self.y_sca).to(dev)[:, None]
        out = torch.empty((d, n), dtype=torch.float64, device=dev)
        call("obhip_predict_vjp_multi_dev", self.om._h, self._t._h, dth.data_ptr(), q, dx.data_ptr(), n,
             dw.data_ptr(), n, None, out.data_ptr())
        return out.cpu().numpy().T

    def hvp(self, xnew, cot, V):
        """(hvp n x d, jvp n x q) of the de-standardised means for one direction per row (the rows of V):
        hvp[i, l] = sum_j cot[i, j] sum_m V[i, m] d2 mean_ij / d x_il d x_im and jvp[i, j] =
        sum_l V[i, l] d mean_ij / d x_il, raw units.  cot (n x q) is scaled by y_sca per response as in
        vjp and sent through obhip_predict_hvp_multi_dev; no Jacobian and no Hessian is formed."""
        import torch
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim != 2 or xnew.shape[1] != self.om.d:
            raise ValueError("xnew must be n x d")
        cot, V = np.asarray(cot, dtype=np.float64), np.asarray(V, dtype=np.float64)
        n, q, d = xnew.shape[0], self.q, self.om.d
        if cot.shape != (n, q):
            raise ValueError("cot must be n x q")
        if V.shape != (n, d):
            raise ValueError("V must be n x d")
        if n == 0:
            return np.zeros((0, d)), np.zeros((0, q))
        dev, dx, dth = self._dev_inputs(xnew)
        sca = torch.from_numpy(self.y_sca).to(dev)
        dw = torch.from_numpy(np.ascontiguousarray(cot.T)).to(dev) * sca[:, None]
        dv = torch.from_numpy(np.ascontiguousarray(V.T)).to(dev)
        hv = torch.empty((d, n), dtype=torch.float64, device=dev)
        jv = torch.empty((q, n), dtype=torch.float64, device=dev)
        call("obhip_predict_hvp_multi_dev", self.om._h, self._t._h, dth.data_ptr(), q, dx.data_ptr(), n,
             dw.data_ptr(), n, dv.data_ptr(), None, None, jv.data_ptr(), hv.data_ptr())
        return hv.cpu().numpy().T, (jv * sca[:, None]).cpu().numpy().T

    def predict_hess(self, xnew, response=0):
        """The Hessian of one response's de-standardised mean, hess[i, l, m] = d2 mean_i / d x_il d x_im
        (n x d x d): d hvp calls with unit directions, each evaluating the basis again -- for the few
        rows of an optimiser or a Laplace approximation, not for 1e6 rows."""
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim != 2 or xnew.shape[1] != self.om.d:
            raise ValueError("xnew must be n x d")
        if not 0 <= int(response) < self.q:
            raise ValueError("response must be in 0 .. q - 1")
        n, d = xnew.shape[0], self.om.d
        cot = np.zeros((n, self.q))
        cot[:, int(response)] = 1.0
        hess = np.empty((n, d, d))
        for m in range(d):
            V = np.zeros((n, d))
            V[:, m] = 1.0
            hess[:, :, m] = self.hvp(xnew, cot, V)[0]
        return hess

    def sobol(self, nodes, weights=None):
        """Sobol indices of every response under the product measure of nodes / weights
        (sensitivity.input_moments), in raw units: SobolResult with mean = y_cent + y_sca mu, the variances
        times y_sca^2 and the indices unchanged."""
        from . import sensitivity
        mom = sensitivity.input_moments(self.om, self._t, nodes, weights)
        res = sensitivity.sobol(self.om, self._t, self.coeff, mom)
        s2 = self.y_sca * self.y_sca
        res.mean = self.y_cent + self.y_sca * res.mean
        res.var = res.var * s2
        res.first_var = res.first_var * s2[None, :]
        res.total_var = res.total_var * s2[None, :]
        return res

    def main_effects(self, dim, grid, nodes, weights=None):
        """E[f | x_dim = z] - E[f] of every response at the points of grid (G x q), in raw units (times y_sca)"""
        from . import sensitivity
        mom = sensitivity.input_moments(self.om, self._t, nodes, weights)
        return sensitivity.main_effects(self.om, self._t, self.coeff, mom, dim, grid) * self.y_sca[None, :]

    def sobol2(self, nodes, weights=None):
        """Second-order and total-interaction indices of every response under the product measure of nodes /
        weights, in raw units: Sobol2Result with the variances times y_sca^2 and the shares unchanged."""
        from . import sensitivity
        mom = sensitivity.input_moments(self.om, self._t, nodes, weights)
        res = sensitivity.sobol2(self.om, self._t, self.coeff, mom)
        s2 = self.y_sca * self.y_sca
        res.var = res.var * s2
        res.first_var = res.first_var * s2[None, :]
        res.second_var = res.second_var * s2[None, :]
        res.total_interaction_var = res.total_interaction_var * s2[None, :]
        res.closed_var = res.closed_var * s2[None, :]
        res._mats(self.om.d)
        return res

    def shapley(self, nodes, weights=None, groups=None):
        """Shapley effects of every response under the product measure of nodes / weights, in raw units:
        ShapleyResult with the variances times y_sca^2 and the shares unchanged (sensitivity.shapley)."""
        from . import sensitivity
        sensitivity._check_groups(self.om.d, groups)
        mom = sensitivity.input_moments(self.om, self._t, nodes, weights)
        res = sensitivity.shapley(self.om, self._t, self.coeff, mom, groups)
        s2 = self.y_sca * self.y_sca
        res.effect_var = res.effect_var * s2[None, :]
        res.var = res.var * s2
        return res

    def active_subspace(self, nodes, weights=None, scale=None):
        """E[grad f grad f^T], the DGSM and the active subspace of every response under the product measure of
        nodes / weights, in raw units: ActiveSubspaceResult with C, dgsm and the eigenvalues times y_sca^2,
        mean_grad times y_sca and the eigenvectors unchanged (sensitivity.active_subspace)."""
        from . import sensitivity
        sensitivity._check_nodes(self.om, nodes, weights)
        sensitivity._check_scale(self.om.d, scale)
        gm = sensitivity.input_grad_moments(self.om, self._t, nodes, weights)
        res = sensitivity.active_subspace(self.om, self._t, self.coeff, gm, scale)
        s2 = self.y_sca * self.y_sca
        res.C = res.C * s2[None, None, :]
        res.dgsm = res.dgsm * s2[None, :]
        res.mean_grad = res.mean_grad * self.y_sca[None, :]
        res.eigenvalues = res.eigenvalues * s2[None, :]
        return res

    def conditional(self, x, noise_dims, nodes, weights=None, grad=False):
        """Mean and variance of every response over the noise inputs noise_dims (independent, the product measure of
        nodes / weights) at the control inputs of the rows x (n x d or n x |S|), in raw units: ConditionalResult
        with mean = y_cent + y_sca M, var times y_sca^2 and, with grad=True, grad_mean times y_sca and grad_var
        times y_sca^2 (sensitivity.conditional_moments)."""
        from . import sensitivity
        mom = sensitivity.input_moments(self.om, self._t, nodes, weights)
        res = sensitivity.conditional_moments(self.om, self._t, self.coeff, mom, noise_dims, x, grad=grad)
        s2 = self.y_sca * self.y_sca
        res.mean = self.y_cent[None, :] + self.y_sca[None, :] * res.mean
        res.var = res.var * s2[None, :]
        if grad:
            res.grad_mean = res.grad_mean * self.y_sca[None, None, :]
            res.grad_var = res.grad_var * s2[None, None, :]
        return res

    def interaction_effects(self, dim_i, dim_j, grid_i, grid_j, nodes, weights=None):
        """the interaction surface of every response on grid_i x grid_j (Gi x Gj x q), in raw units (times y_sca)"""
        from . import sensitivity
        mom = sensitivity.input_moments(self.om, self._t, nodes, weights)
        return (sensitivity.interaction_effects(self.om, self._t, self.coeff, mom, dim_i, dim_j, grid_i, grid_j)
                * self.y_sca[None, None, :])

    def predict_product(self, xa, xb, dims_b, var=False):
        """De-standardised mean (na x nb x q) at every pair (xa[i], xb[j]): the dimensions dims_b (0-based,
        ascending) take their inputs from xb, the others from xa (product.predict_product; the na nb
        full-width rows are never written).  With var=True also the variance (na x nb x q), scaled by
        y_sca^2 as predict scales it."""
        from . import product
        xa, xb, db = product.check_blocks(self.om.d, xa, xb, dims_b)
        na, nb, q = xa.shape[0], xb.shape[0], self.q
        if na == 0 or nb == 0:
            z = np.zeros((na, nb, q))
            return (z, z.copy()) if var else z
        mean, v = product.predict_product_dev(self.om, self._t, self.coeff, xa, xb, db,
                                              1.0 / self.diagH if var else None, self.sigma)
        mean = mean.permute(2, 1, 0).cpu().numpy() * self.y_sca[None, None, :] + self.y_cent[None, None, :]
        if not var:
            return mean
        return mean, v.cpu().numpy().T[:, :, None] * (self.y_sca * self.y_sca)[None, None, :]

    def calibration_loglik(self, x_field, y_field, t_cand, dims_t, obs_var=None, response=0, emulator_var=True,
                           grad=False):
        """Gaussian log-likelihood of the field data y_field (na, raw units) observed at the settings x_field
        (na x the dimensions not in dims_t) for every candidate t_cand[j] (nb x len(dims_t)) of the
        dimensions dims_t, under the emulator of one response:
            r_ij = y_i - mean_ij,  v_ij = emulator variance_ij (emulator_var; else its noise term) + obs_var_i
            loglik_j = -(chi2_j + logdet_j) / 2 - (na / 2) log 2 pi,  chi2 = sum_i r^2 / v,  logdet = sum_i log v.
        obs_var: na variances in raw units (or one for all rows; None: 0).  Returns a CalibrationLoglik with
        loglik, chi2, logdet (nb each).  The sums are formed on the device tile by tile
        (obhip_product_loglik_dev); the na x nb matrices are never written.
        grad=True: the result also has grad (nb x len(dims_t)), d loglik_j / d t_cand[j] = -(d chi2_j +
        d logdet_j) / 2 in raw units, from the same pass (obhip_product_loglik_grad_dev); the constant
        2 na log y_sca of logdet has no gradient."""
        from . import product
        x_field, t_cand, _ = product.check_blocks(self.om.d, x_field, t_cand, dims_t)
        y, ov = self._field_data(x_field, y_field, obs_var, response)
        na = x_field.shape[0]
        args = (self.om, self._t, self.coeff[:, response], x_field, y, t_cand, dims_t)
        kw = dict(obsvar=ov, coeffvar=1.0 / self.diagH if emulator_var else None, sigma=self.sigma)
        g = None
        if grad:
            chi2, logdet, dchi2, dlogdet = product.product_loglik_grad(*args, **kw)
            g = -0.5 * (dchi2 + dlogdet)
        else:
            chi2, logdet = product.product_loglik(*args, **kw)
        logdet = logdet + 2.0 * na * math.log(self.y_sca[response])
        return product.CalibrationLoglik(-0.5 * (chi2 + logdet) - 0.5 * na * math.log(2.0 * math.pi), chi2, logdet, g)

    def _field_data(self, x_field, y_field, obs_var, response):
        """calibration_loglik's checks: (standardised y, standardised obs_var or None) of one response"""
        if not (isinstance(response, (int, np.integer)) and 0 <= response < self.q):
            raise ValueError("response must be in 0 .. q - 1")
        y = np.asarray(y_field, dtype=np.float64)
        na = x_field.shape[0]
        if y.shape != (na,):
            raise ValueError("y_field must have one entry per row of x_field")
        cent, sca = self.y_cent[response], self.y_sca[response]
        ov = None
        if obs_var is not None:
            ov = np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (na,)) if np.ndim(obs_var) == 0 \
                else np.asarray(obs_var, dtype=np.float64)
            if ov.shape != (na,):
                raise ValueError("obs_var must be a number or have one entry per row of x_field")
            ov = ov / (sca * sca)
        return (y - cent) / sca, ov

    def torch(self):
        """a differentiable torch module of the de-standardised predictor (torch_emulator.TorchEmulator)"""
        from .torch_emulator import TorchEmulator
        return TorchEmulator(self)


def fit_newton_multi(om, terms, x, Y, sigma=None, rho=DEFAULT_RHO, comm=None):
    """One Newton step from coeff = 0 of lpdfvec(loglik_std, logpr_gauss) (lpdf::optnewton,
    fit.cpp:98-131) for every column of Y (n x q) over the rows x (n x d): one Gram, one
    Cholesky factorisation, batched passes for what depends on Y.  sigma=None: log(0.01), what
    loglik_std starts from for a standardised response (loglik_std.cpp:51).  comm: an obhip_comm
    handle of a row-sharded job (x, Y are then this rank's rows), None = one rank."""
    x, Y = _check_xy(om, x, Y)
    import torch
    if sigma is None:
        sigma = math.log(0.01)
    t = obmod._terms_of(om, terms)
    n, q, p, f64 = x.shape[0], Y.shape[1], t.p, torch.float64
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
    meansd = torch.empty((q, 3), dtype=f64, device=dev)
    call("obhip_standardise_multi_dev", comm, dY.data_ptr(), n, q, n, dY.data_ptr(), meansd.data_ptr())
    caps = t.maxlevels()
    basis = C.c_void_p()
    call("obhip_basis_create_dev", C.byref(basis), om._h, dx.data_ptr(), n, caps.ctypes.data)
    try:
        wsb, cnt, nr = C.c_uint64(0), C.c_uint64(0), C.c_int(1)
        call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
        exbuf = None
        if comm is not None:
            call("obhip_comm_info", comm, C.byref(nr), None, None, None, None)
            call("obhip_fit_newton_multi_count", p, q, nr.value, C.byref(cnt))
            exbuf = torch.zeros(cnt.value, dtype=f64, device=dev)
        ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
        H = torch.empty((p, p), dtype=f64, device=dev)
        rhs = torch.empty((q, p), dtype=f64, device=dev)
        theta = torch.empty((q, p), dtype=f64, device=dev)
        diagH = torch.empty(p, dtype=f64, device=dev)
        call("obhip_fit_newton_multi_dev", comm, basis, t._h, om._h, dY.data_ptr(), q, n, sigma, rho,
             H.data_ptr(), rhs.data_ptr(), theta.data_ptr(), diagH.data_ptr(),
             None if exbuf is None else exbuf.data_ptr(), cnt.value, ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
    finally:
        call("obhip_basis_destroy", basis)
    return MultiFit(om, t, theta.cpu().numpy().T.copy(), meansd.cpu().numpy(), diagH.cpu().numpy(),
                    sigma, rho)
