"""Sobol indices, Shapley effects, main effects and active subspaces of the fitted mean, in closed form.

The fitted mean is a sum of products of one-dimensional functions, f(x) = sum_k theta_k prod_l
psi_{l, t_kl}(x_l) with psi_l = getbase(l).  Under independent inputs with a discrete measure per
dimension (nodes and weights), its variance decomposition is a sum over per-dimension moment tables
of the psi (include/obhip.h, "variance-based sensitivity"): no pick-freeze sampling, no sampling
error.  The measure is what the caller passes as nodes: the training rows themselves (empirical
marginals) or a quadrature rule of a density (uniform_nodes).

torch holds the device memory; all arithmetic is in libobhip.
"""
import ctypes as C

import numpy as np

from . import obmod
from ._lib import call


def _device():
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch, dev


def _levels(t):
    return (t.maxlevels() + 1).astype(np.int64)


class InputMoments:
    """Result of input_moments: mean[l] (L_l) and cov[l] (L_l x L_l) per dimension, L_l = 1 + the highest
    level the terms use in dimension l, and the packed device copies mean_dev / cov_dev that sobol and
    main_effects read."""

    def __init__(self, terms, levels, mean_dev, cov_dev):
        self.terms, self.levels = terms, levels
        self.mean_dev, self.cov_dev = mean_dev, cov_dev
        pm, pc = mean_dev.cpu().numpy(), cov_dev.cpu().numpy()
        om_ = np.concatenate([[0], np.cumsum(levels)])
        oc_ = np.concatenate([[0], np.cumsum(levels * levels)])
        self.mean = [pm[om_[l]:om_[l + 1]].copy() for l in range(len(levels))]
        self.cov = [pc[oc_[l]:oc_[l + 1]].reshape(levels[l], levels[l]).copy() for l in range(len(levels))]


class SobolResult:
    """mean (q), var (q); first_var, total_var, first, total (d x q each): Var E[f | x_l], V - Var E[f | x_~l]
    and their shares S_l, T_l of var (NaN where var == 0); g: the packed g_l on the device (main effects)."""

    def __init__(self, out, d, g_dev):
        self.mean, self.var = out[:, 0].copy(), out[:, 1].copy()
        self.first_var = np.ascontiguousarray(out[:, 2:2 + d].T)
        self.total_var = np.ascontiguousarray(out[:, 2 + d:2 + 2 * d].T)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(self.var == 0.0, np.nan, self.var)
            self.first, self.total = self.first_var / v, self.total_var / v
        self.g = g_dev


def _pair_matrix(v, pairs, d):
    """n_pairs x q -> symmetric d x d x q with a NaN diagonal"""
    m = np.full((d, d, v.shape[1]), np.nan)
    m[pairs[:, 0], pairs[:, 1]] = v
    m[pairs[:, 1], pairs[:, 0]] = v
    return m


class Sobol2Result:
    """pairs (n_pairs x 2): the pairs i < j of dimensions in the order (0,1), (0,2), .. (0,d-1), (1,2), ..
    Per pair and response (n_pairs x q), and as symmetric d x d x q matrices with a NaN diagonal (*_mat):
    second_var = Var E[f | x_i, x_j] - V1_i - V1_j, the pure second-order variance; total_interaction_var, the
    variances of all subsets that hold both i and j (superset importance); second, total_interaction: their
    shares of var (NaN where var == 0).  closed_var (n_pairs x q) = V1_i + V1_j + second_var = Var E[f | x_i, x_j].
    var (q) and first_var (d x q) are those of sobol; G: the packed G_ij on the device (interaction surfaces)."""

    def __init__(self, out, d, G_dev, first):
        q = out.shape[0]
        self.pairs = np.array([(i, j) for i in range(d) for j in range(i + 1, d)], dtype=np.int64).reshape(-1, 2)
        n_pairs = len(self.pairs)
        self.var, self.first_var = first.var, first.first_var
        self.second_var = np.ascontiguousarray(out[:, :n_pairs].T).reshape(n_pairs, q)
        self.total_interaction_var = np.ascontiguousarray(out[:, n_pairs:].T).reshape(n_pairs, q)
        i, j = self.pairs[:, 0], self.pairs[:, 1]
        self.closed_var = self.first_var[i] + self.first_var[j] + self.second_var
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(self.var == 0.0, np.nan, self.var)
            self.second, self.total_interaction = self.second_var / v, self.total_interaction_var / v
        self.G = G_dev
        self._mats(d)

    def _mats(self, d):
        for name in ("second_var", "total_interaction_var", "second", "total_interaction"):
            setattr(self, name + "_mat", _pair_matrix(getattr(self, name), self.pairs, d))


class ShapleyResult:
    """players: the list of dimension lists; effect_var (P x q): the Shapley effect of every player in variance
    units; var (q): their column sums, the variance of the fitted mean; effect = effect_var / var (NaN where
    var == 0), shares that sum to 1."""

    def __init__(self, out, players):
        self.players = players
        self.effect_var = np.ascontiguousarray(out.T)
        self.var = self.effect_var.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.effect = self.effect_var / np.where(self.var == 0.0, np.nan, self.var)


def _check_groups(d, groups):
    """-> (players: list of dimension lists, ids: d int32 player ids or None for the default)"""
    if groups is None:
        return [[l] for l in range(d)], None
    players = [[int(l) for l in g] for g in groups]
    flat = [l for g in players for l in g]
    if any(len(g) == 0 for g in players) or sorted(flat) != list(range(d)):
        raise ValueError("groups must be non-empty lists of dimension indices that partition range(d)")
    ids = np.empty(d, dtype=np.int32)
    for g, dims in enumerate(players):
        ids[dims] = g
    return players, ids


def _check_nodes(om, nodes, weights):
    nodes = np.asarray(nodes, dtype=np.float64)
    if nodes.ndim != 2 or nodes.shape[1] != om.d:
        raise ValueError("nodes must be n x d")
    if nodes.shape[0] == 0:
        raise ValueError("nodes has no rows: there is no measure")
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float64)
        if weights.shape != nodes.shape:
            raise ValueError("weights must be n x d like nodes")
    return nodes, weights


def _check_theta(t, Theta):
    Theta = np.asarray(Theta, dtype=np.float64)
    if Theta.ndim == 1:
        Theta = Theta[:, None]
    if Theta.ndim != 2 or Theta.shape[0] != t.p:
        raise ValueError("Theta must have one row per term")
    if Theta.shape[1] == 0:
        raise ValueError("Theta has no columns")
    return Theta


def uniform_nodes(lo, hi, order=64):
    """(nodes, weights), order x d each: the Gauss-Legendre rule of `order` points on [lo_l, hi_l] per dimension
    (numpy.polynomial.legendre.leggauss), for inputs uniform on a box; the weights of a dimension sum to
    hi_l - lo_l and are normalised by the library.  The indices are exact for this discrete measure; how well it
    stands for the continuous uniform density is the quadrature order, the caller's accuracy knob."""
    lo, hi = np.atleast_1d(np.asarray(lo, dtype=np.float64)), np.atleast_1d(np.asarray(hi, dtype=np.float64))
    if lo.shape != hi.shape or lo.ndim != 1 or not np.all(hi > lo):
        raise ValueError("lo and hi must be vectors of one length with hi > lo")
    if int(order) < 1:
        raise ValueError("order must be >= 1")
    z, w = np.polynomial.legendre.leggauss(int(order))
    half, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    return mid[None, :] + half[None, :] * z[:, None], half[None, :] * w[:, None]


def input_moments(om, terms, nodes, weights=None):
    """The moment tables of the 1-D bases over the product measure of nodes (n x d) and weights (n x d, >= 0,
    normalised per dimension; None: all equal) -- obhip_dim_moments_dev."""
    nodes, weights = _check_nodes(om, nodes, weights)
    t = obmod._terms_of(om, terms)
    torch, dev = _device()
    n = nodes.shape[0]
    nm, nc = C.c_uint64(0), C.c_uint64(0)
    call("obhip_sobol_layout", t._h, C.byref(nm), C.byref(nc))
    dx = torch.from_numpy(np.ascontiguousarray(nodes.T)).to(dev)
    dw = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights.T)).to(dev)
    mean = torch.empty(nm.value, dtype=torch.float64, device=dev)
    cov = torch.empty(nc.value, dtype=torch.float64, device=dev)
    call("obhip_dim_moments_dev", om._h, t._h, dx.data_ptr(), n, n, None if dw is None else dw.data_ptr(), n,
         mean.data_ptr(), cov.data_ptr())
    return InputMoments(t, _levels(t), mean, cov)


def sobol(om, terms, Theta, moments):
    """SobolResult of the responses Theta (p x q, or p) under the measure of `moments` -- obhip_sobol_dev."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    torch, dev = _device()
    q, d = Theta.shape[1], t.d
    wsb = C.c_uint64(0)
    call("obhip_sobol_workspace_bytes", t.p, d, q, C.byref(wsb))
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((q, 2 + 2 * d), dtype=torch.float64, device=dev)
    g = torch.empty((q, int(moments.levels.sum())), dtype=torch.float64, device=dev)
    call("obhip_sobol_dev", t._h, dth.data_ptr(), q, moments.mean_dev.data_ptr(), moments.cov_dev.data_ptr(),
         out.data_ptr(), g.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    return SobolResult(out.cpu().numpy(), d, g)


def main_effects(om, terms, Theta, moments, dim, grid):
    """E[f | x_dim = z] - E[f] at the points z of grid (G), G x q: the main-effect curve of every response."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    if grid.ndim != 1:
        raise ValueError("grid must be a vector")
    if not 0 <= int(dim) < t.d:
        raise ValueError("dim out of range (0-based)")
    res = sobol(om, t, Theta, moments)
    q, G = Theta.shape[1], grid.shape[0]
    if G == 0:
        return np.zeros((0, q))
    torch, dev = _device()
    dz = torch.from_numpy(grid).to(dev)
    out = torch.empty((q, G), dtype=torch.float64, device=dev)
    call("obhip_main_effect_dev", om._h, t._h, int(dim), res.g.data_ptr(), q, dz.data_ptr(), G, out.data_ptr())
    out -= torch.from_numpy(res.mean).to(dev)[:, None]
    return out.cpu().numpy().T


def sobol2(om, terms, Theta, moments):
    """Sobol2Result of the responses Theta (p x q, or p) under the measure of `moments`: which inputs matter
    together -- obhip_sobol2_dev, and sobol for var and the first-order variances."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    first = sobol(om, t, Theta, moments)
    torch, dev = _device()
    q, d = Theta.shape[1], t.d
    npairs, nG, wsb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    call("obhip_sobol2_layout", t._h, C.byref(npairs), C.byref(nG))
    call("obhip_sobol2_workspace_bytes", t.p, d, q, C.byref(wsb))
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((q, 2 * npairs.value), dtype=torch.float64, device=dev)
    G = torch.empty((q, nG.value), dtype=torch.float64, device=dev)
    call("obhip_sobol2_dev", t._h, dth.data_ptr(), q, moments.mean_dev.data_ptr(), moments.cov_dev.data_ptr(),
         out.data_ptr() if npairs.value else None, G.data_ptr() if nG.value else None, ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    return Sobol2Result(out.cpu().numpy(), d, G, first)


def interaction_effects(om, terms, Theta, moments, dim_i, dim_j, grid_i, grid_j):
    """E[f | x_i = z, x_j = z'] - E[f | x_i = z] - E[f | x_j = z'] + E[f] on grid_i (Gi) x grid_j (Gj), Gi x Gj x q:
    the two-input interaction surface of every response, both main effects and the mean taken off."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    grid_i = np.ascontiguousarray(grid_i, dtype=np.float64)
    grid_j = np.ascontiguousarray(grid_j, dtype=np.float64)
    if grid_i.ndim != 1 or grid_j.ndim != 1:
        raise ValueError("grid_i and grid_j must be vectors")
    dim_i, dim_j = int(dim_i), int(dim_j)
    if not (0 <= dim_i < t.d and 0 <= dim_j < t.d):
        raise ValueError("dim_i or dim_j out of range (0-based)")
    if dim_i == dim_j:
        raise ValueError("dim_i and dim_j must differ")
    q, Gi, Gj = Theta.shape[1], grid_i.shape[0], grid_j.shape[0]
    if Gi * Gj == 0:
        return np.zeros((Gi, Gj, q))
    res = sobol2(om, t, Theta, moments)
    mi = main_effects(om, t, Theta, moments, dim_i, grid_i)                     # Gi x q, mu taken off
    mj = main_effects(om, t, Theta, moments, dim_j, grid_j)
    mu = sobol(om, t, Theta, moments).mean
    torch, dev = _device()
    dzi, dzj = torch.from_numpy(grid_i).to(dev), torch.from_numpy(grid_j).to(dev)
    out = torch.empty((q, Gi, Gj), dtype=torch.float64, device=dev)
    call("obhip_interaction_effect_dev", om._h, t._h, dim_i, dim_j, res.G.data_ptr(), q, dzi.data_ptr(), Gi,
         dzj.data_ptr(), Gj, out.data_ptr())
    surf = out.cpu().numpy().transpose(1, 2, 0)
    return surf - mi[:, None, :] - mj[None, :, :] - mu[None, None, :]


def shapley(om, terms, Theta, moments, groups=None):
    """ShapleyResult of the responses Theta (p x q, or p) under the measure of `moments`: one effect per player,
    summing to the variance.  groups: lists of dimension indices that partition range(d), each list one player;
    None: every dimension its own player -- obhip_shapley_dev."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    players, ids = _check_groups(t.d, groups)
    q, d = Theta.shape[1], t.d
    gp = None if ids is None else ids.ctypes.data
    P, wsb = C.c_uint64(0), C.c_uint64(0)
    call("obhip_shapley_layout", t._h, gp, C.byref(P), None)
    call("obhip_shapley_workspace_bytes", t.p, d, q, C.byref(wsb))
    torch, dev = _device()
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((q, P.value), dtype=torch.float64, device=dev)
    call("obhip_shapley_dev", t._h, gp, dth.data_ptr(), q, moments.mean_dev.data_ptr(), moments.cov_dev.data_ptr(),
         out.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    return ShapleyResult(out.cpu().numpy(), players)


class GradMoments:
    """Result of input_grad_moments: `moments`, the InputMoments of the same measure (mean, cov), and per dimension
    dmean[l] (L_l) = E[psi'], cross[l] (L_l x L_l, not symmetric) = E[psi'_a psi_b], dd[l] (L_l x L_l, symmetric) =
    E[psi'_a psi'_b], psi' = d psi / d x_l in raw input units; the packed device copies dmean_dev, cross_dev,
    dd_dev are what active_subspace reads.  One object serves sobol / sobol2 / shapley (through .moments) and
    active_subspace."""

    def __init__(self, moments, dmean_dev, cross_dev, dd_dev):
        self.moments, self.terms, self.levels = moments, moments.terms, moments.levels
        self.mean_dev, self.cov_dev, self.mean, self.cov = moments.mean_dev, moments.cov_dev, moments.mean, moments.cov
        self.dmean_dev, self.cross_dev, self.dd_dev = dmean_dev, cross_dev, dd_dev
        levels = self.levels
        pm, px, pd = dmean_dev.cpu().numpy(), cross_dev.cpu().numpy(), dd_dev.cpu().numpy()
        om_ = np.concatenate([[0], np.cumsum(levels)])
        oc_ = np.concatenate([[0], np.cumsum(levels * levels)])
        self.dmean = [pm[om_[l]:om_[l + 1]].copy() for l in range(len(levels))]
        self.cross = [px[oc_[l]:oc_[l + 1]].reshape(levels[l], levels[l]).copy() for l in range(len(levels))]
        self.dd = [pd[oc_[l]:oc_[l + 1]].reshape(levels[l], levels[l]).copy() for l in range(len(levels))]


def sym_eigh(A):
    """(w, V) of the symmetric matrix A by the library's Jacobi solver (obhip_sym_eigh, host only): w descending,
    V[:, j] the unit eigenvector of w[j], its component of largest magnitude positive."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] == 0:
        raise ValueError("A must be a square matrix with at least one row")
    n = A.shape[0]
    a = np.asfortranarray(A)
    w, V = np.empty(n), np.empty((n, n), order="F")
    call("obhip_sym_eigh", n, a.ctypes.data, w.ctypes.data, V.ctypes.data)
    return w, np.ascontiguousarray(V)


class ActiveSubspaceResult:
    """C (d x d x q) = E[grad f grad f^T] per response, symmetric by construction (the device returns one triangle);
    dgsm (d x q) = its diagonal, the derivative-based global sensitivity measures nu_l; mean_grad (d x q) = E[grad f];
    scale (d, or None); eigenvalues (d x q, descending) and eigenvectors (d x d x q, [:, j, r] the j-th of response
    r) of diag(scale) C diag(scale) -- of C itself without scale."""

    def __init__(self, out, d, scale):
        q = out.shape[0]
        self.mean_grad = np.ascontiguousarray(out[:, :d].T)
        iu = np.triu_indices(d)
        self.C = np.empty((d, d, q))
        self.C[iu[0], iu[1]] = out[:, d:].T
        self.C[iu[1], iu[0]] = out[:, d:].T
        self.dgsm = np.ascontiguousarray(self.C[np.arange(d), np.arange(d)])
        self.scale = scale
        self.eigenvalues, self.eigenvectors = np.empty((d, q)), np.empty((d, d, q))
        self._eig()

    def _eig(self):
        s = np.ones(self.C.shape[0]) if self.scale is None else self.scale
        for r in range(self.C.shape[2]):
            self.eigenvalues[:, r], self.eigenvectors[:, :, r] = sym_eigh(self.C[:, :, r] * s[:, None] * s[None, :])

    def activity_scores(self, k):
        """alpha_l = sum_{j < k} lambda_j W[l, j]^2 (Constantine and Diaz 2017), d x q: what dimension l
        contributes to the first k eigen-directions"""
        k = int(k)
        if not 1 <= k <= self.C.shape[0]:
            raise ValueError("k must be 1 .. d")
        return np.einsum("jr,ljr->lr", self.eigenvalues[:k], self.eigenvectors[:, :k] ** 2)

    def project(self, x, k, response=0):
        """the active variables y = W_k^T (x / scale) of the rows x (n x d) for one response, n x k: the coordinates
        along the first k eigenvectors, in the scaled inputs the eigenvectors belong to"""
        x = np.asarray(x, dtype=np.float64)
        d = self.C.shape[0]
        if x.ndim != 2 or x.shape[1] != d:
            raise ValueError("x must be n x d")
        k, response = int(k), int(response)
        if not 1 <= k <= d:
            raise ValueError("k must be 1 .. d")
        if not 0 <= response < self.C.shape[2]:
            raise ValueError("response out of range")
        if self.scale is not None:
            x = x / self.scale[None, :]
        return x @ self.eigenvectors[:, :k, response]


def _check_scale(d, scale):
    if scale is None:
        return None
    scale = np.asarray(scale, dtype=np.float64)
    if scale.shape != (d,) or not np.all(np.isfinite(scale)) or not np.all(scale > 0):
        raise ValueError("scale must be d positive numbers")
    return scale


def input_grad_moments(om, terms, nodes, weights=None):
    """GradMoments of the product measure of nodes / weights (as input_moments takes them): the moment tables and
    the three gradient tables -- obhip_dim_moments_dev and obhip_dim_grad_moments_dev."""
    nodes, weights = _check_nodes(om, nodes, weights)
    t = obmod._terms_of(om, terms)
    mom = input_moments(om, t, nodes, weights)
    torch, dev = _device()
    n = nodes.shape[0]
    nm, nc = C.c_uint64(0), C.c_uint64(0)
    call("obhip_active_layout", t._h, C.byref(nm), C.byref(nc), None)
    dx = torch.from_numpy(np.ascontiguousarray(nodes.T)).to(dev)
    dw = None if weights is None else torch.from_numpy(np.ascontiguousarray(weights.T)).to(dev)
    dmean = torch.empty(nm.value, dtype=torch.float64, device=dev)
    cross = torch.empty(nc.value, dtype=torch.float64, device=dev)
    dd = torch.empty(nc.value, dtype=torch.float64, device=dev)
    call("obhip_dim_grad_moments_dev", om._h, t._h, dx.data_ptr(), n, n, None if dw is None else dw.data_ptr(), n,
         dmean.data_ptr(), cross.data_ptr(), dd.data_ptr())
    return GradMoments(mom, dmean, cross, dd)


def active_subspace(om, terms, Theta, gmoments, scale=None):
    """ActiveSubspaceResult of the responses Theta (p x q, or p) under the measure of `gmoments`
    (input_grad_moments) -- obhip_active_dev, then obhip_sym_eigh per response.  scale: d positive numbers (the box
    widths, say): the eigen step takes diag(scale) C diag(scale), the matrix of the inputs x / scale."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    scale = _check_scale(t.d, scale)
    torch, dev = _device()
    q, d = Theta.shape[1], t.d
    wsb, nout = C.c_uint64(0), C.c_uint64(0)
    call("obhip_active_layout", t._h, None, None, C.byref(nout))
    call("obhip_active_workspace_bytes", t.p, d, q, C.byref(wsb))
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((q, nout.value), dtype=torch.float64, device=dev)
    g = gmoments
    call("obhip_active_dev", t._h, dth.data_ptr(), q, g.mean_dev.data_ptr(), g.cov_dev.data_ptr(),
         g.dmean_dev.data_ptr(), g.cross_dev.data_ptr(), g.dd_dev.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb.value)
    torch.cuda.synchronize()
    return ActiveSubspaceResult(out.cpu().numpy(), d, scale)


class ConditionalResult:
    """mean, var (n x q): E[f | x_S] and Var[f | x_S] over the noise inputs at the control inputs of every row;
    grad_mean, grad_var (n x |S| x q, or None): their derivatives by the control inputs, [i, a, j] by the a-th of
    control_dims; control_dims: the dimensions that are not noise, ascending."""

    def __init__(self, mean, var, grad_mean, grad_var, control_dims):
        self.mean, self.var, self.grad_mean, self.grad_var = mean, var, grad_mean, grad_var
        self.control_dims = control_dims


def _check_noise_dims(d, noise_dims):
    """-> (dims_e uint32, control_dims int64)"""
    de = np.atleast_1d(np.asarray(noise_dims)).astype(np.int64)
    if de.ndim != 1 or de.size < 1 or de.size > d - 1:
        raise ValueError("noise_dims must name 1 to d - 1 dimensions")
    if np.any(de < 0) or np.any(de >= d) or np.any(np.diff(de) <= 0):
        raise ValueError("noise_dims must be strictly ascending dimension indices (0-based)")
    return np.ascontiguousarray(de, dtype=np.uint32), np.setdiff1d(np.arange(d), de)


def conditional_layout(om, terms, noise_dims):
    """{"n_groups", "group_of" (p), "mu_s", "fused", "control_dims"} of the split into noise and control dimensions:
    the groups of terms by their levels on the noise dimensions, numbered in the order of their first term, the used
    basis columns of the control side and whether the row kernels keep its tile in LDS -- obhip_conditional_layout
    (host only)."""
    t = obmod._terms_of(om, terms)
    de, ctrl = _check_noise_dims(t.d, noise_dims)
    G, mu, fused = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
    gof = np.empty(t.p, dtype=np.uint32)
    call("obhip_conditional_layout", t._h, de.ctypes.data, de.size, C.byref(G), gof.ctypes.data, C.byref(mu),
         C.byref(fused))
    return {"n_groups": int(G.value), "group_of": gof.astype(np.int64), "mu_s": int(mu.value),
            "fused": bool(fused.value), "control_dims": ctrl}


def conditional_tables(om, terms, moments, noise_dims):
    """(mE (G), K (G x G)) of the groups under the measure of `moments`: the product of the means and the telescoped
    covariance bracket on the groups' level tuples -- obhip_conditional_tables_dev."""
    t = obmod._terms_of(om, terms)
    de, _ = _check_noise_dims(t.d, noise_dims)
    G = conditional_layout(om, t, noise_dims)["n_groups"]
    torch, dev = _device()
    mE = torch.empty(G, dtype=torch.float64, device=dev)
    K = torch.empty((G, G), dtype=torch.float64, device=dev)
    call("obhip_conditional_tables_dev", t._h, de.ctypes.data, de.size, moments.mean_dev.data_ptr(),
         moments.cov_dev.data_ptr(), mE.data_ptr(), K.data_ptr())
    torch.cuda.synchronize()
    return mE.cpu().numpy(), K.cpu().numpy()


def conditional_moments(om, terms, Theta, moments, noise_dims, x, grad=False, chunk_rows=0):
    """ConditionalResult of the responses Theta (p x q, or p) at the rows x: the mean and the variance of the fitted
    mean over the noise inputs, which are independent and follow the measure of `moments`, with the other inputs
    held at the row's values; grad=True: also their gradients by the control inputs.  x: n x d (the noise columns
    are ignored) or n x |S| (the control dimensions ascending).  chunk_rows: 0 or a positive multiple of 128, the
    rows worked on at a time; it changes no bit of the result -- obhip_conditional_moments_dev."""
    t = obmod._terms_of(om, terms)
    Theta = _check_theta(t, Theta)
    de, ctrl = _check_noise_dims(t.d, noise_dims)
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] not in (t.d, ctrl.size):
        raise ValueError("x must be n x d or n x |S|")
    if x.shape[1] == t.d:
        x = x[:, ctrl]
    chunk_rows = int(chunk_rows)
    if chunk_rows < 0 or chunk_rows % 128:
        raise ValueError("chunk_rows must be 0 or a positive multiple of 128")
    n, q, ns = x.shape[0], Theta.shape[1], ctrl.size
    if n == 0:
        z, g = np.zeros((0, q)), np.zeros((0, ns, q))
        return ConditionalResult(z, z.copy(), g if grad else None, g.copy() if grad else None, ctrl)
    torch, dev = _device()
    f64 = torch.float64
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    mean = torch.empty((q, n), dtype=f64, device=dev)
    var = torch.empty((q, n), dtype=f64, device=dev)
    gm = torch.empty((q, ns, n), dtype=f64, device=dev) if grad else None
    gv = torch.empty((q, ns, n), dtype=f64, device=dev) if grad else None
    call("obhip_conditional_moments_dev", om._h, t._h, dth.data_ptr(), q, de.ctypes.data, de.size,
         moments.mean_dev.data_ptr(), moments.cov_dev.data_ptr(), dx.data_ptr(), n, chunk_rows, mean.data_ptr(),
         var.data_ptr(), gm.data_ptr() if grad else None, gv.data_ptr() if grad else None)
    torch.cuda.synchronize()
    return ConditionalResult(mean.cpu().numpy().T, var.cpu().numpy().T,
                             gm.permute(2, 1, 0).cpu().numpy() if grad else None,
                             gv.permute(2, 1, 0).cpu().numpy() if grad else None, ctrl)
