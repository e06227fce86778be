"""The multi-response predictor as a differentiable torch module.

A multi-output emulator is used for calibration and optimisation over its inputs: a scalar loss of
all q outputs is differentiated by x.  TorchEmulator wraps a MultiFit so that it can sit inside a
torch.optim loop: forward is obhip_predict_multi_dev, backward the vector-Jacobian product
obhip_predict_vjp_multi_dev, the backward of that the Hessian-vector and Jacobian-vector product
obhip_predict_hvp_multi_dev (include/obhip.h), all on the current stream; neither the n x d x q
Jacobian nor a Hessian is formed.  All arithmetic is in libobhip; torch holds the memory and the graph.

TorchCalibration does the same for the calibration log-likelihood by the candidate parameters and
TorchAcquisition for an acquisition criterion of a Posterior by the inputs (obhip_acquire_grad_dev), each
differentiable once.
"""
import ctypes as C

import numpy as np

from ._lib import call, torch

if torch is None:  # host-only use of the package: the name exists, building one needs torch
    class TorchEmulator:
        def __init__(self, *args, **kwargs):
            raise ImportError("TorchEmulator needs torch")

    class TorchCalibration:
        def __init__(self, *args, **kwargs):
            raise ImportError("TorchCalibration needs torch")

    class TorchAcquisition:
        def __init__(self, *args, **kwargs):
            raise ImportError("TorchAcquisition needs torch")
else:
    def _colmajor(a):
        """the (rows, cols) tensor a as a contiguous (cols, rows) tensor: column-major storage of a"""
        return a.detach().t().contiguous()

    class _Predict(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, emu):
            n, q = x.shape[0], emu.q
            xc = _colmajor(x)
            mean = torch.empty((q, n), dtype=torch.float64, device=x.device)
            if n > 0:
                call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
                call("obhip_predict_multi_dev", emu._om._h, emu._t._h, emu.theta.data_ptr(), q, xc.data_ptr(), n,
                     mean.data_ptr(), None, emu._sigma, None)
            ctx.emu, ctx.xc = emu, xc
            ctx.save_for_backward(x)
            return (mean * emu.y_sca[:, None] + emu.y_cent[:, None]).t()

        @staticmethod
        def backward(ctx, grad_output):
            x, = ctx.saved_tensors
            return _PredictVjp.apply(grad_output, x, ctx.xc, ctx.emu), None

    class _PredictVjp(torch.autograd.Function):
        """the backward of _Predict as a function of (grad_output, x): out = sum_j grad_output_ij y_sca_j
        d mean_ij / d x (obhip_predict_vjp_multi_dev; xc is x column-major, as the forward left it).
        Its own backward is _PredictHvp."""

        @staticmethod
        def forward(ctx, grad_output, x, xc, emu):
            d, n = xc.shape
            out = torch.zeros((d, n), dtype=torch.float64, device=xc.device)
            w = None
            if n > 0:
                w = (grad_output.detach().to(torch.float64) * emu.y_sca[None, :]).t().contiguous()   # n x q column-major
                call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
                call("obhip_predict_vjp_multi_dev", emu._om._h, emu._t._h, emu.theta.data_ptr(), emu.q, xc.data_ptr(),
                     n, w.data_ptr(), n, None, out.data_ptr())
            ctx.emu, ctx.xc, ctx.w = emu, xc, w
            ctx.save_for_backward(grad_output, x)
            return out.t()

        @staticmethod
        def backward(ctx, u):
            grad_output, x = ctx.saved_tensors
            gy, gx = _PredictHvp.apply(u, grad_output, x, ctx.xc, ctx.w, ctx.emu)
            return gy, gx, None, None

    class _PredictHvp(torch.autograd.Function):
        """the backward of _PredictVjp for the cotangent u (n x d) of its output: one
        obhip_predict_hvp_multi_dev call with the direction u gives the Hessian-vector product (for x)
        and jvp . y_sca (for grad_output).  The library has no third derivative: backward raises."""

        @staticmethod
        def forward(ctx, u, grad_output, x, xc, w, emu):
            d, n = xc.shape
            hv = torch.zeros((d, n), dtype=torch.float64, device=xc.device)
            jv = torch.zeros((emu.q, n), dtype=torch.float64, device=xc.device)
            if n > 0:
                v = _colmajor(u.to(torch.float64))
                call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
                call("obhip_predict_hvp_multi_dev", emu._om._h, emu._t._h, emu.theta.data_ptr(), emu.q, xc.data_ptr(),
                     n, w.data_ptr(), n, v.data_ptr(), None, None, jv.data_ptr(), hv.data_ptr())
            return (jv * emu.y_sca[:, None]).t(), hv.t()

        @staticmethod
        def backward(ctx, *grads):
            raise RuntimeError("TorchEmulator is twice differentiable by x: a third derivative was asked for "
                               "(the library has no third input derivatives of the predictor)")

    class TorchEmulator(torch.nn.Module):
        """forward(x): (n, d) float64 tensor on the current GPU -> (n, q) de-standardised means, differentiable
        by x twice (the second derivative through obhip_predict_hvp_multi_dev; a third raises).  Theta, y_cent
        and y_sca are device buffers uploaded once."""

        def __init__(self, fit):
            super().__init__()
            self._om, self._t, self._sigma = fit.om, fit._t, float(fit.sigma)
            self.q, self.d = int(fit.q), int(fit.om.d)
            dev = torch.device("cuda", torch.cuda.current_device())
            self.register_buffer("theta", torch.from_numpy(np.ascontiguousarray(fit.coeff.T)).to(dev))  # p x q column-major
            self.register_buffer("y_cent", torch.from_numpy(np.ascontiguousarray(fit.y_cent)).to(dev))
            self.register_buffer("y_sca", torch.from_numpy(np.ascontiguousarray(fit.y_sca)).to(dev))

        def forward(self, x):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64:
                raise TypeError("TorchEmulator takes a float64 tensor on the GPU")
            if x.dim() != 2 or x.shape[1] != self.d:
                raise ValueError("x must be n x d")
            if x.device != self.theta.device:
                raise ValueError("x is on another device than the emulator")
            return _Predict.apply(x, self)

    class _CalibrationLoglik(torch.autograd.Function):
        """loglik (nb) of the candidates t (nb x L) and, saved for backward, its gradient (nb x L): one
        obhip_product_loglik_grad_dev call.  backward is cot[:, None] * grad; the gradient itself is not
        differentiable (the library has no second derivatives on the product)."""

        @staticmethod
        def forward(ctx, t, cal):
            from . import product
            nb, L = t.shape
            if nb == 0:
                ctx.save_for_backward(torch.zeros_like(t))
                return torch.zeros((0,), dtype=torch.float64, device=t.device)
            out = product.product_loglik_grad_dev(cal._om, cal._t, cal.theta, cal.xa, cal.y, cal.obsvar, _colmajor(t),
                                                  cal._db, cal.coeffvar, cal._sigma)
            ctx.save_for_backward((-0.5 * (out[2:2 + L] + out[2 + L:])).t().contiguous())
            return -0.5 * (out[0] + out[1]) + cal._shift

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, cot):
            grad, = ctx.saved_tensors
            return cot[:, None] * grad, None

    class TorchCalibration(torch.nn.Module):
        """The calibration log-likelihood of MultiFit.calibration_loglik as a torch module: forward(t) takes
        the candidates t (nb x len(dims_t), float64 on the GPU) and returns loglik (nb), differentiable by t
        once (backward = cot[:, None] * d loglik / d t, from the same obhip_product_loglik_grad_dev call), so
        that nb chains or starting points move in one torch.optim loop.  The field data are uploaded once;
        nothing passes through the host in forward or backward."""

        def __init__(self, fit, x_field, y_field, dims_t, obs_var=None, response=0, emulator_var=True):
            super().__init__()
            from . import product
            # (a one-row stand-in for the candidates: the checks of the blocks need only their width)
            x_field, _, self._db = product.check_blocks(fit.om.d, x_field, np.zeros((1, np.size(dims_t))), dims_t)
            y, ov = fit._field_data(x_field, y_field, obs_var, response)
            y, ov = product._loglik_args(fit._t, fit.coeff[:, response], x_field, y, ov, None, fit.sigma)[1:3]
            self._om, self._t, self._sigma = fit.om, fit._t, float(fit.sigma)
            self.L, na = int(self._db.size), x_field.shape[0]
            self._shift = -0.5 * (2.0 * na * float(np.log(fit.y_sca[response])) + na * float(np.log(2.0 * np.pi)))
            dev = torch.device("cuda", torch.cuda.current_device())
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
            self.register_buffer("theta", up(fit.coeff[:, response]))
            self.register_buffer("xa", up(x_field.T).reshape(x_field.shape[1], na))   # column-major
            self.register_buffer("y", up(y))
            self.register_buffer("obsvar", up(ov))
            self.register_buffer("coeffvar", up(1.0 / fit.diagH) if emulator_var else None)

        def forward(self, t):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64:
                raise TypeError("TorchCalibration takes a float64 tensor on the GPU")
            if t.dim() != 2 or t.shape[1] != self.L:
                raise ValueError("t must be nb x len(dims_t)")
            if t.device != self.theta.device:
                raise ValueError("t is on another device than the calibration")
            return _CalibrationLoglik.apply(t, self)

    class _AcquireScore(torch.autograd.Function):
        """score (n) of the rows x (n x d) and, saved for backward, its gradient (n x d): one
        obhip_acquire_grad_dev call.  backward is cot[:, None] * grad; the gradient itself is not
        differentiable (the library has no second derivatives of the criteria)."""

        @staticmethod
        def forward(ctx, x, acq):
            n, d = x.shape
            score = torch.empty((n,), dtype=torch.float64, device=x.device)
            grad = torch.empty((d, n), dtype=torch.float64, device=x.device)
            if n > 0:
                xc = _colmajor(x)
                call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
                call("obhip_acquire_grad_dev", acq._post._h, acq.theta.data_ptr(), xc.data_ptr(), n, acq._crit,
                     (C.c_double * 4)(*acq._params), acq._maximize, acq._chunk_rows, score.data_ptr(), grad.data_ptr(),
                     None, None, None, None)
            ctx.save_for_backward(grad.t())
            return score

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, cot):
            grad, = ctx.saved_tensors
            return cot[:, None] * grad, None

    class TorchAcquisition(torch.nn.Module):
        """An acquisition criterion of a Posterior as a torch module: forward(x) takes the rows x (n x d, float64 on
        the GPU) and returns their n scores in standardised units, differentiable by x once (backward =
        grad_output[:, None] * d score / d x, from the same obhip_acquire_grad_dev call; a second derivative
        raises), so that n starting points climb in one torch.optim loop.  criterion, best, level, kappa, xi and
        maximize are Posterior.acquire_grad's; theta (p): the standardised coefficients of one response, uploaded
        once.  inv(H) is formed by the first forward on the posterior and kept with it; neither x nor the gradient
        passes through the host.  The posterior must stay open as long as the module is used."""

        def __init__(self, post, theta, criterion="ei", best=None, level=None, kappa=1.96, xi=0.0, maximize=False,
                     chunk_rows=0):
            super().__init__()
            from . import design
            post._need()
            theta = np.ascontiguousarray(theta, dtype=np.float64)
            if theta.shape != (post.p,):
                raise ValueError("theta must be the p standardised coefficients of one response")
            self._params, _, _ = post._acquire_args(criterion, best, level, kappa, xi, None)
            self._post, self._crit, self._maximize = post, design.ACQUISITIONS[criterion], int(bool(maximize))
            self._chunk_rows = post._chunk_rows(chunk_rows)
            self.criterion, self.d = criterion, int(post.om.d)
            dev = torch.device("cuda", torch.cuda.current_device())
            self.register_buffer("theta", torch.from_numpy(theta).to(dev))

        def forward(self, x):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64:
                raise TypeError("TorchAcquisition takes a float64 tensor on the GPU")
            if x.dim() != 2 or x.shape[1] != self.d:
                raise ValueError("x must be n x d")
            if x.device != self.theta.device:
                raise ValueError("x is on another device than the acquisition")
            self._post._need()
            return _AcquireScore.apply(x, self)
