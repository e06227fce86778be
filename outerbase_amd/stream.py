"""Streaming Newton fit: rows come and go, every row is passed over once.

fit_newton_multi takes all rows at once and pays the whole Gram per call.  A NewtonAccumulator
keeps the normal equations of the rows it has been given on the device (include/obhip.h,
"streaming Newton fit"): the packed upper triangle of G = B^T B, B^T (Y - c), B^T 1 and per
response the moments (n, mean, M2) in merge form.  Adding a batch costs the Gram of that batch,
a fit one Cholesky factorisation; batches can be taken out again, and a fit can leave the rows of
another accumulator out without touching either -- which makes K-fold cross-validation over a
grid of (sigma, rho) one pass over the rows plus K x C factorisations (cv_newton_multi).

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C
import math

import numpy as np

from . import obmod
from ._lib import call, lib
from .multi import DEFAULT_RHO, MultiFit, _check_xy


def _stream():
    import torch
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch.device("cuda", torch.cuda.current_device())


class NewtonAccumulator:
    """The normal equations of a growing / shrinking set of rows for q responses over one model and
    term set.  Device memory: 8 (p (p + 1) / 2 + p q + p + 4 q) bytes (obhip_normal_acc_bytes), and
    as much again as pooled scratch while a batch is added."""

    def __init__(self, om, terms, q=1):
        q = int(q)
        if q < 1:
            raise ValueError("q must be at least 1")
        self.om, self._t, self.q = om, obmod._terms_of(om, terms), q
        self.p = self._t.p
        self._h = None          # made on first use: nothing here touches the device
        self._closed = False
        self._bufs = None

    # -- life time ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.obhip_normal_acc_destroy(self._h)
        self._h = None
        self._closed = True
        self._bufs = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _need(self):
        if self._closed:
            raise RuntimeError("the accumulator is closed")
        if not self._h:
            h = C.c_void_p()
            call("obhip_normal_acc_create", C.byref(h), self.om._h, self._t._h, self.q)
            self._h = h

    # -- state -------------------------------------------------------------------------------
    def _info(self):
        self._need()
        v = [C.c_uint64(0) for _ in range(4)]
        call("obhip_normal_acc_info", self._h, *[C.byref(a) for a in v])
        return [a.value for a in v]

    @property
    def rows(self):
        return self._info()[2]

    @property
    def batches(self):
        return self._info()[3]

    def reset(self):
        self._need()
        call("obhip_normal_acc_reset", self._h)

    def state(self):
        """Host copy of the state: tri (packed upper triangle of G), rhs (p x q: B^T (Y - shift)),
        b1 (B^T 1), shift, mu (mean - shift), M2, n (q each)."""
        import torch
        self._need()
        dev = _stream()
        p, q = self.p, self.q
        nb = C.c_uint64(0)
        call("obhip_normal_acc_bytes", p, q, C.byref(nb))
        buf = torch.empty(nb.value // 8, dtype=torch.float64, device=dev)
        call("obhip_normal_acc_export_dev", self._h, buf.data_ptr(), buf.numel())
        s = buf.cpu().numpy()
        tri = p * (p + 1) // 2
        mom = s[tri + p * q + p:].reshape(q, 4)
        return dict(tri=s[:tri].copy(), rhs=s[tri:tri + p * q].reshape(q, p).T.copy(), b1=s[tri + p * q:tri + p * q + p].copy(),
                    shift=mom[:, 0].copy(), mu=mom[:, 1].copy(), M2=mom[:, 2].copy(), n=mom[:, 3].copy())

    # -- rows in and out ---------------------------------------------------------------------
    def _check(self, x, Y):
        x, Y = _check_xy(self.om, x, Y, min_rows=0)
        if Y.shape[1] != self.q:
            raise ValueError("Y has %d columns, the accumulator %d responses" % (Y.shape[1], self.q))
        if not np.all(np.isfinite(x)):
            raise ValueError("x must be finite")
        return x, Y

    def _batch_dev(self, dx, dY, n, sign):
        """dx (d, n), dY (q, n): device tensors, column-major n x d and n x q"""
        self._need()
        caps = self._t.maxlevels()
        basis = C.c_void_p()
        call("obhip_basis_create_dev", C.byref(basis), self.om._h, dx.data_ptr(), n, caps.ctypes.data)
        try:
            call("obhip_normal_acc_add_dev", self._h, basis, dY.data_ptr(), n, sign)
            import torch
            torch.cuda.synchronize()
        finally:
            call("obhip_basis_destroy", basis)

    def _batch(self, x, Y, sign):
        x, Y = self._check(x, Y)
        self._need()
        n = x.shape[0]
        if n == 0:
            return self
        import torch
        dev = _stream()
        dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
        dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev)
        self._batch_dev(dx, dY, n, sign)
        return self

    def add(self, x, Y):
        """Add the rows x (n x d) with their raw responses Y (n x q, or n for q = 1); n = 0 is a
        no-op.  The basis of the batch is built, used once and destroyed."""
        return self._batch(x, Y, +1)

    def remove(self, x, Y):
        """Take out rows that were added before (the same x and Y)."""
        return self._batch(x, Y, -1)

    # -- observed input gradients -------------------------------------------------------------
    @property
    def grad_rows(self):
        """Gradient equations in the state: rows times differentiated dimensions of every batch."""
        self._need()
        eq = C.c_uint64(0)
        call("obhip_normal_acc_grad_info", self._h, C.byref(eq), None)
        return eq.value

    def _grad_batch(self, x, dY, dims, weights, sign):
        x, dims, weights = _check_grad_x(self.om, x, dims, weights)
        n, L = x.shape[0], len(dims)
        dY = np.asarray(dY, dtype=np.float64)
        if dY.ndim == 2:
            dY = dY[:, :, None]
        if dY.ndim != 3 or dY.shape != (n, L, self.q):
            raise ValueError("dY must be n x %d (x %d): one column per differentiated dimension (and response)"
                             % (L, self.q))
        if not np.all(np.isfinite(dY)):
            raise ValueError("dY must be finite")
        self._need()
        if n == 0:
            return self
        import torch
        dev = _stream()
        dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
        dg = torch.from_numpy(np.ascontiguousarray(dY.transpose(2, 1, 0))).to(dev)     # [response][dimension][row]
        call("obhip_normal_acc_add_grad_dev", self._h, dx.data_ptr(), n, dims.ctypes.data, L,
             None if weights is None else weights.ctypes.data, dg.data_ptr(), n, sign)
        torch.cuda.synchronize()
        return self

    def add_grad(self, x, dY, dims=None, weights=None):
        """Add the observed gradients dY (n x L, or n x L x q: dY[i, j] = dy / dx_dims[j] at row i, raw
        units) at the rows x (n x d) as n L further equations of the fit, dimension dims[j] weighted by
        weights[j] > 0 (include/obhip.h, "observed input gradients").  dims=None: all d dimensions;
        weights=None: all 1.  The responses' mean and standard deviation stay those of the value rows."""
        return self._grad_batch(x, dY, dims, weights, +1)

    def remove_grad(self, x, dY, dims=None, weights=None):
        """Take out gradient rows that were added before (the same x, dY, dims and weights)."""
        return self._grad_batch(x, dY, dims, weights, -1)

    # -- gridded data: the product of two input blocks ------------------------------------------
    def _product_batch(self, xa, xb, Y, dims_b, sign):
        from .product import check_blocks
        xa, xb, db = check_blocks(self.om.d, xa, xb, dims_b)
        na, nb = xa.shape[0], xb.shape[0]
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 2:
            Y = Y[:, :, None]
        if Y.ndim != 3 or Y.shape != (na, nb, self.q):
            raise ValueError("Y must be na x nb (x %d): one value per pair (and response)" % self.q)
        if na == 0 or nb == 0:
            raise ValueError("a grid batch needs rows on both sides")
        if not (np.all(np.isfinite(xa)) and np.all(np.isfinite(xb))):
            raise ValueError("xa and xb must be finite")
        if not np.all(np.isfinite(Y)):
            raise ValueError("Y must be finite")
        self._need()
        import torch
        dev = _stream()
        dxa = torch.from_numpy(np.ascontiguousarray(xa.T)).to(dev)
        dxb = torch.from_numpy(np.ascontiguousarray(xb.T)).to(dev)
        dY = torch.from_numpy(np.ascontiguousarray(Y.transpose(2, 1, 0))).to(dev)       # [response][j][i]
        self._product_batch_dev(dxa, dxb, dY, na, nb, db, na, sign)
        return self

    def _product_batch_dev(self, dxa, dxb, dY, na, nb, db, lda, sign):
        """dxa (|A|, na), dxb (|B|, nb), dY (q, nb, lda): device tensors; db: check_dims_b's uint32 array"""
        import torch
        self._need()
        call("obhip_normal_acc_add_product_dev", self._h, dxa.data_ptr(), na, dxb.data_ptr(), nb, db.ctypes.data, db.size,
             dY.data_ptr(), lda, sign)
        torch.cuda.synchronize()

    def add_product(self, xa, xb, Y, dims_b):
        """Add the na nb observations of a full grid: Y[i, j] (na x nb, or na x nb x q: the shape of
        predict_product's mean) is the response at the pair (xa[i], xb[j]), xb holding the dimensions dims_b and
        xa all others (include/obhip.h, "Newton fit on the product of two input blocks").  The pairs are never
        written out: the cost is the Gram of na + nb rows and one matrix product."""
        return self._product_batch(xa, xb, Y, dims_b, +1)

    def remove_product(self, xa, xb, Y, dims_b):
        """Take out a grid batch that was added before (the same xa, xb, Y and dims_b: the accumulator does not
        remember the split)."""
        return self._product_batch(xa, xb, Y, dims_b, -1)

    def merge(self, other, sign=+1):
        """self += sign * other (another accumulator of the same model, terms and q)"""
        if not isinstance(other, NewtonAccumulator):
            raise TypeError("merge takes a NewtonAccumulator")
        if sign not in (1, -1):
            raise ValueError("sign must be +1 or -1")
        self._need()
        other._need()
        _stream()
        call("obhip_normal_acc_combine_dev", self._h, other._h, int(sign))
        return self

    # -- the fit -----------------------------------------------------------------------------
    def _solve_dev(self, sigma, rho, minus=None):
        """-> Theta (q, p), diagH (p), meansd (q, 3): device tensors, reused by the next call"""
        import torch
        self._need()
        if minus is not None:
            if not isinstance(minus, NewtonAccumulator):
                raise TypeError("minus must be a NewtonAccumulator")
            minus._need()
        dev = _stream()
        p, q, f64 = self.p, self.q, torch.float64
        if self._bufs is None or self._bufs["H"].device != dev:
            wsb = C.c_uint64(0)
            call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
            self._bufs = dict(ws=torch.empty(wsb.value, dtype=torch.uint8, device=dev),
                              H=torch.empty((p, p), dtype=f64, device=dev),
                              theta=torch.empty((q, p), dtype=f64, device=dev),
                              diagH=torch.empty(p, dtype=f64, device=dev),
                              meansd=torch.empty((q, 3), dtype=f64, device=dev))
        b = self._bufs
        call("obhip_normal_acc_solve_dev", self._h, None if minus is None else minus._h, sigma, rho,
             b["H"].data_ptr(), b["theta"].data_ptr(), b["diagH"].data_ptr(), b["meansd"].data_ptr(),
             b["ws"].data_ptr(), b["ws"].numel())
        return b["theta"], b["diagH"], b["meansd"]

    def fit(self, sigma=None, rho=DEFAULT_RHO, minus=None):
        """One Newton step from coeff = 0 (lpdf::optnewton, fit.cpp:98-131) on the rows in the
        accumulator -- with minus, on those rows without the rows of that accumulator, neither being
        changed -- every response standardised over exactly those rows.  -> MultiFit, as
        fit_newton_multi returns it.  sigma=None: log(0.01)."""
        import torch
        if sigma is None:
            sigma = math.log(0.01)
        theta, diagH, meansd = self._solve_dev(float(sigma), float(rho), minus)
        torch.cuda.synchronize()
        return MultiFit(self.om, self._t, theta.cpu().numpy().T.copy(), meansd.cpu().numpy(), diagH.cpu().numpy(),
                        float(sigma), float(rho))

    def posterior(self, sigma=None, rho=DEFAULT_RHO, minus=None):
        """The posterior covariance of the coefficients given the rows in the accumulator (without those of
        minus): a design.Posterior on the Hessian that fit(sigma, rho, minus) factors, formed on the device
        (obhip_normal_acc_posterior_dev).  It carries the responses' meansd (q x 3) of the same rows.
        sigma=None: log(0.01)."""
        import torch
        from .design import Posterior
        if sigma is None:
            sigma = math.log(0.01)
        _, _, meansd = self._solve_dev(float(sigma), float(rho), minus)     # checks minus, sets the stream
        h = C.c_void_p()
        call("obhip_normal_acc_posterior_dev", self._h, None if minus is None else minus._h, float(sigma), float(rho),
             C.byref(h))
        torch.cuda.synchronize()
        return Posterior(self.om, self._t, h, meansd.cpu().numpy().copy())

    def term_path(self, sigma=None, rho=DEFAULT_RHO, minus=None, step=16, x=None, Y=None, loo=False, chunk_rows=0):
        """How many terms?  The terms of the accumulator stand in list order (selectterms sorts by prior
        variance), so every prefix of the list is a model of its own; this scores the model of the first k terms
        for every checkpoint k = step, 2 step, ..., p from ONE factorisation and ONE pass over the rows
        (include/obhip.h, "term-count path"): the factor of the whole list nests the factor of every prefix.

        Always: the log evidence log p(y | k) of the rows in the accumulator (without those of minus).  With rows
        x (n x d) and their raw responses Y (n x q) also the row scores per checkpoint: loo=False for rows that
        are NOT in the fit (hold-out error and log score), loo=True for the rows of the fit themselves, each
        once (PRESS, the leave-one-out log score and the hat trace), the standardisation of the responses held
        fixed.  sigma=None: log(0.01).  chunk_rows bounds the workspace of the row pass: 0 = the library's choice,
        otherwise a positive multiple of 128; the result does not depend on it, bit for bit.  -> TermPathResult
        (close it, or use it as a context manager: it keeps the factor on the device for fit(k))."""
        import torch
        from .design import Posterior
        if sigma is None:
            sigma = math.log(0.01)
        sigma, rho, step = float(sigma), float(rho), int(step)
        if step < 1:
            raise ValueError("step must be at least 1")
        chunk_rows = Posterior._chunk_rows(chunk_rows)
        if (x is None) != (Y is None):
            raise ValueError("x and Y come together")
        if x is not None:
            x, Y = self._check(x, Y)
        if self.grad_rows or (minus is not None and minus.grad_rows):
            raise ValueError("the evidence of the term-count path is that of value rows: the accumulator holds gradient rows")
        self._need()
        if minus is not None:
            if not isinstance(minus, NewtonAccumulator):
                raise TypeError("minus must be a NewtonAccumulator")
            minus._need()
        dev = _stream()
        p, q, f64 = self.p, self.q, torch.float64
        mh = None if minus is None else minus._h
        # the right-hand sides and the moments first: what refuses a fit (too few rows, a changed model) refuses here
        dG = torch.empty((q, p), dtype=f64, device=dev)
        dmeansd = torch.empty((q, 3), dtype=f64, device=dev)
        call("obhip_normal_acc_rhs_dev", self._h, mh, sigma, dG.data_ptr(), dmeansd.data_ptr())
        h = C.c_void_p()
        call("obhip_normal_acc_posterior_dev", self._h, mh, sigma, rho, C.byref(h))     # the one factorisation
        post = Posterior(self.om, self._t, h, dmeansd.cpu().numpy().copy())
        try:
            ddiag = torch.empty(p, dtype=f64, device=dev)
            call("obhip_posterior_hessian_diag_dev", post._h, ddiag.data_ptr())
            diagH = ddiag.cpu().numpy()
            dU = torch.empty_like(dG)
            call("obhip_posterior_path_coef_dev", post._h, dG.data_ptr(), q, dU.data_ptr())
            K = C.c_uint64(0)
            call("obhip_term_path_layout", p, q, step, 0, 0, C.byref(K), None, None)
            K = K.value
            sizes = np.minimum((np.arange(K, dtype=np.int64) + 1) * step, p)
            ms = post.meansd
            rows = ms[:, 2]
            prec = np.ascontiguousarray(1.0 / (self.om.getvar(self._t.array) * math.exp(2 * rho)))
            yty = np.ascontiguousarray(rows - 1.0)      # of the standardised response: sd has the n - 1 denominator
            ev = np.empty((K, q))
            call("obhip_posterior_path_evidence", post._h, dU.data_ptr(), q, prec.ctypes.data, yty.ctypes.data,
                 int(rows[0]), step, ev.ctypes.data)
            res = TermPathResult(self.om, self._t, post, dU, sizes, ev, diagH, sigma, rho, bool(loo))
            if x is not None:
                n = x.shape[0]
                dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev) if n else None
                dY = torch.from_numpy(np.ascontiguousarray(Y.T)).to(dev) if n else None
                sc, sumv = post._term_path_scores_dev(dU, dx, n, dY, dmeansd, step, loo, chunk_rows)
                sd = ms[:, 1]
                res.n = n
                res.sse = sc[:, :, 0] * sd[None, :] ** 2
                res.spe = sc[:, :, 1] * sd[None, :] ** 2
                res.lpd = sc[:, :, 2] - n * np.log(sd)[None, :]
                res.rmse = np.sqrt(res.spe / n) if n else np.full((K, q), np.nan)
                res.dof = sumv / math.exp(2 * sigma) if loo else None
            return res
        except BaseException:
            post.close()
            raise


class TermPathResult:
    """The path over the number of terms (NewtonAccumulator.term_path).

    sizes (K): the checkpoints k = step, 2 step, ..., p.  log_evidence (K x q): log p(y | first k terms) of the
    rows of the fit -- for the STANDARDISED response (y - centre) / scale, as the fit sees it: add -n log(scale)
    for the raw response; the difference between two sizes does not depend on that.  With rows given: sse (K x q)
    = sum (y - mean_k)^2; spe = the sum of squared prediction errors (loo: PRESS, else sse); lpd = the sum of the
    log predictive densities (loo: each row's by the fit without it); rmse = sqrt(spe / n) -- all in RAW units --
    and dof (K) = the hat trace sum_i h_i under loo, else None.  Without rows they are None.  The leave-one-out
    scores hold the centre and scale of the responses fixed."""

    def __init__(self, om, t, post, dU, sizes, log_evidence, diagH, sigma, rho, loo):
        self.om, self._t, self._post, self._dU = om, t, post, dU
        self.sizes, self.log_evidence = sizes, log_evidence
        self._diagH, self.sigma, self.rho, self.loo = diagH, sigma, rho, loo
        self.n = 0
        self.sse = self.spe = self.lpd = self.rmse = self.dof = None

    def close(self):
        if getattr(self, "_post", None) is not None:
            self._post.close()
        self._post = self._dU = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def best(self, by="evidence", response=None):
        """The size that is best by "evidence" (largest), "lpd" (largest) or "spe" (smallest) for one response,
        or for the mean over the responses (response=None).  The lowest size wins a tie."""
        table = {"evidence": (self.log_evidence, 1.0), "lpd": (self.lpd, 1.0), "spe": (self.spe, -1.0)}
        if by not in table:
            raise ValueError("by must be one of %s" % sorted(table))
        a, sign = table[by]
        if a is None:
            raise ValueError("no rows were given: only the evidence is there")
        s = sign * (a.mean(axis=1) if response is None else a[:, int(response)])
        return int(self.sizes[int(np.argmax(s))])       # (argmax: the first among equals)

    def fit(self, k):
        """The MultiFit of the first k terms (1 <= k <= p, a checkpoint or not), as fit_newton_multi on terms[:k]
        and the same rows gives it: the coefficients come from the factor the path has."""
        import torch
        if self._post is None:
            raise RuntimeError("the path is closed")
        k = int(k)
        if not 1 <= k <= self._t.p:
            raise ValueError("k must be between 1 and p")
        _stream()
        dT = torch.empty_like(self._dU)
        call("obhip_posterior_path_theta_dev", self._post._h, self._dU.data_ptr(), self._dU.shape[0], k, dT.data_ptr())
        torch.cuda.synchronize()
        theta = dT.cpu().numpy().T[:k].copy()
        return MultiFit(self.om, obmod._Terms(self.om, self._t.array[:k]), theta, self._post.meansd.copy(),
                        self._diagH[:k].copy(), self.sigma, self.rho)


def _check_grad_x(om, x, dims, weights):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != om.d:
        raise ValueError("x must be n x d")
    if not np.all(np.isfinite(x)):
        raise ValueError("x must be finite")
    dims = np.arange(om.d, dtype=np.uint32) if dims is None else np.atleast_1d(np.asarray(dims))
    if dims.ndim != 1 or len(dims) == 0 or not np.issubdtype(dims.dtype, np.integer):
        raise ValueError("dims must be a non-empty list of dimensions")
    if np.any(dims < 0) or np.any(dims >= om.d) or len(set(dims.tolist())) != len(dims):
        raise ValueError("dims must be distinct dimensions below d = %d" % om.d)
    dims = np.ascontiguousarray(dims, dtype=np.uint32)
    if weights is not None:
        weights = np.ascontiguousarray(np.atleast_1d(weights), dtype=np.float64)
        if weights.shape != dims.shape or not np.all(np.isfinite(weights)) or np.any(weights <= 0):
            raise ValueError("weights must be one finite positive number per differentiated dimension")
    return x, dims, weights


def design_dx(om, terms, x, dims=None, weights=None):
    """The derivative design matrix at the rows x (n x d): out[j, i, k] = sqrt(weights[j]) dB[i, k] / dx_dims[j],
    an (L, n, p) array (obhip_design_dx_dev).  dims=None: all d dimensions; weights=None: all 1."""
    import torch
    x, dims, weights = _check_grad_x(om, x, dims, weights)
    t = obmod._terms_of(om, terms)
    n, L = x.shape[0], len(dims)
    if n == 0:
        return np.zeros((L, 0, t.p))
    dev = _stream()
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    out = torch.empty((L, n, t.p), dtype=torch.float64, device=dev)
    call("obhip_design_dx_dev", om._h, t._h, dx.data_ptr(), n, dims.ctypes.data, L,
         None if weights is None else weights.ctypes.data, out.data_ptr(), t.p)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def fit_newton_grad(om, terms, x, Y, dY, xg=None, dims=None, weights=None, sigma=None, rho=DEFAULT_RHO):
    """The Newton fit of fit_newton_multi on the rows x (n x d) with responses Y (n x q) AND their observed
    input gradients dY (ng x L, or ng x L x q) at the rows xg (None: at x itself): an accumulator filled
    once.  dims, weights: as NewtonAccumulator.add_grad.  dY=None: the value rows alone.  -> MultiFit"""
    x, Y = _check_xy(om, x, Y)
    with NewtonAccumulator(om, terms, Y.shape[1]) as acc:
        acc.add(x, Y)
        if dY is not None:
            acc.add_grad(x if xg is None else xg, dY, dims=dims, weights=weights)
        return acc.fit(sigma=sigma, rho=rho)


def cv_folds(n, folds, seed=0):
    """Fold of every row: a seeded permutation dealt round-robin, so the fold sizes differ by at
    most one and the same (n, folds, seed) always gives the same assignment."""
    n, folds = int(n), int(folds)
    if folds < 2 or folds > n:
        raise ValueError("folds must be between 2 and the number of rows")
    perm = np.random.default_rng(seed).permutation(n)
    fold_of = np.empty(n, dtype=np.int64)
    fold_of[perm] = np.arange(n) % folds
    return fold_of


class CVResult:
    """candidates: the C pairs (sigma, rho), sigma-major; rmse (C x q): held-out root mean squared
    error per response in raw units; score (C): mean over the responses of rmse / sd(y);
    best: its argmin (the first among equals); sigma, rho: that candidate; heldout (n x q): every
    row's prediction by the fit that did not see it, at the best candidate; fit: the MultiFit of all
    rows at the best candidate; fold_of (n)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def cv_newton_multi(om, terms, x, Y, folds=5, sigmas=(math.log(0.01),), rhos=(DEFAULT_RHO,), seed=0):
    """K-fold cross-validation of the Newton fit over the grid sigmas x rhos.

    Rows are dealt to K folds by cv_folds(n, folds, seed).  Every fold's rows go through the Gram
    kernels ONCE into an accumulator of their own, and the K accumulators are summed into one more:
    the Gram work is one pass over the n rows whatever K and the grid are.  For every candidate and
    fold the fit of `all rows minus the fold` is one unpack of two triangles and one Cholesky
    factorisation (NewtonAccumulator.fit(minus=...)); the fold's rows are predicted with
    obhip_predict_multi_dev and scored on the device (obhip_cv_score_dev).

    Device memory: K + 1 accumulators -- (K + 1) x 8 (p (p + 1) / 2 + p q + p + 4 q) bytes, 67 MB
    each at p = 4096 -- plus one more as scratch while the folds are added, the p x p Hessian, and
    x, Y and two n x q prediction buffers.

    -> CVResult"""
    x, Y = _check_xy(om, x, Y)
    if not np.all(np.isfinite(x)):
        raise ValueError("x must be finite")
    sigmas = [float(s) for s in np.atleast_1d(sigmas)]
    rhos = [float(r) for r in np.atleast_1d(rhos)]
    if not sigmas or not rhos or not np.all(np.isfinite(sigmas + rhos)):
        raise ValueError("sigmas and rhos must be non-empty and finite")
    n, q = Y.shape
    fold_of = cv_folds(n, folds, seed)
    K = int(folds)
    if n - int(np.bincount(fold_of, minlength=K).max()) < 2:
        raise ValueError("a fit needs two rows outside every fold")
    import torch
    dev = _stream()
    t = obmod._terms_of(om, terms)
    f64 = torch.float64
    idx = [np.nonzero(fold_of == k)[0] for k in range(K)]
    accs, total = [], None
    try:
        dxs, dYs = [], []
        for k in range(K):
            a = NewtonAccumulator(om, t, q)
            accs.append(a)
            dxs.append(torch.from_numpy(np.ascontiguousarray(x[idx[k]].T)).to(dev))
            dYs.append(torch.from_numpy(np.ascontiguousarray(Y[idx[k]].T)).to(dev))
            a._batch_dev(dxs[k], dYs[k], len(idx[k]), +1)
        total = NewtonAccumulator(om, t, q)
        for a in accs:
            total.merge(a)
        cands = [(s, r) for s in sigmas for r in rhos]
        sd = Y.std(axis=0, ddof=1)
        rmse = np.empty((len(cands), q))
        score = np.empty(len(cands))
        held = [[torch.empty((q, len(i)), dtype=f64, device=dev) for i in idx] for _ in range(2)]
        out = torch.empty((K, q, 2), dtype=f64, device=dev)
        best, cur = -1, 0
        for c, (s, r) in enumerate(cands):
            for k in range(K):
                theta, _, meansd = total._solve_dev(s, r, minus=accs[k])
                m, nk = held[cur][k], len(idx[k])
                call("obhip_predict_multi_dev", om._h, t._h, theta.data_ptr(), q, dxs[k].data_ptr(), nk, m.data_ptr(),
                     None, s, None)
                call("obhip_cv_score_dev", m.data_ptr(), dYs[k].data_ptr(), nk, q, nk, meansd.data_ptr(),
                     out[k].data_ptr())
                call("obhip_destandardise_multi_dev", m.data_ptr(), nk, q, nk, meansd.data_ptr(), 0)
            torch.cuda.synchronize()
            o = out.cpu().numpy()
            sse = np.zeros(q)
            for k in range(K):          # fold after fold: a fixed order
                sse += o[k, :, 0]
            assert int(o[:, 0, 1].sum()) == n
            rmse[c] = np.sqrt(sse / n)
            score[c] = float(np.mean(rmse[c] / sd))
            if best < 0 or score[c] < score[best]:
                best, cur = c, 1 - cur
        heldout = np.empty((n, q))
        for k in range(K):
            heldout[idx[k]] = held[1 - cur][k].cpu().numpy().T
        fit = total.fit(cands[best][0], cands[best][1])
    finally:
        for a in accs:
            a.close()
        if total is not None:
            total.close()
    return CVResult(candidates=cands, rmse=rmse, score=score, best=best, sigma=cands[best][0], rho=cands[best][1],
                    heldout=heldout, fit=fit, fold_of=fold_of)
