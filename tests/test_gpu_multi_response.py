"""q responses over one design: one Gram, one Cholesky factor, batched B^T Y, triangular solves
and predictor (obhip_*_multi*, outerbase_amd/multi.py, driver.MultiHotPath).  Every bound below is
derived from what is compared -- rounding bounds of dot products, backward errors relative to the
single-response solve -- or is a figure the project's own tests already use; each test prints its
figures before it asserts."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import knots_for, make_pair

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KINDS = ["mat25", "mat25pow", "mat25ang", "mat25"]
SIGMA, RHO = math.log(0.01), 6.0


def _dev(a):
    """column-major device copy of a host matrix (rows x cols) -> tensor (cols, rows)"""
    import torch
    a = np.asarray(a, dtype=np.float64)
    return torch.from_numpy(np.ascontiguousarray(a.T if a.ndim == 2 else a)).cuda()


def _responses(x, y, q, seed=5):
    """q columns over the rows (x, y): y itself, then smooth column-dependent transforms of it
    plus a little noise; raw (not standardised)"""
    rng = np.random.default_rng(seed)
    cols = [y]
    for j in range(1, q):
        cols.append(math.cos(0.37 * j) * y + math.sin(0.37 * j) * y * x[:, j % x.shape[1]]
                    + 0.05 * np.std(y) * rng.standard_normal(len(y)))
    return np.stack(cols, axis=1)


def _standardised(Y):
    return (Y - Y.mean(axis=0)) / Y.std(axis=0, ddof=1)


class _Case:
    def __init__(self, n, p, q, seed=7, kinds=KINDS, knots=20):
        import ob_oracle as O
        from outerbase_amd import obmod
        self.kinds, self.n, self.p, self.q, self.d = kinds, n, p, q, len(kinds)
        self.om_o, self.om = make_pair(kinds, knots_for(kinds, knots))
        self.terms = self.om_o.selectterms(p)
        self.t = obmod._Terms(self.om, self.terms)
        self.x, y = O.synth_xy(seed, 0, n, kinds)
        self.Yraw = _responses(self.x, y, q)
        self.Y = _standardised(self.Yraw)
        self.xnew, _ = O.synth_xy(seed + 1, 0, max(n // 2, 1), kinds)

    def basis(self, x=None):
        from outerbase_amd._lib import call
        x = self.x if x is None else x
        self.dx = _dev(x)
        h = C.c_void_p()
        call("obhip_basis_create_dev", C.byref(h), self.om._h, self.dx.data_ptr(), x.shape[0],
             self.t.maxlevels().ctypes.data)
        return h

    def fit(self, basis, dY, comm=None, ex=None, q=None, sigma=SIGMA):
        """-> H (factor), B^T Y (q, p), Theta (q, p), diagH"""
        import torch
        from outerbase_amd._lib import call
        p, q = self.p, self.q if q is None else q
        wsb = C.c_uint64(0)
        call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
        H = torch.full((p, p), float("nan"), dtype=torch.float64, device="cuda")
        g = torch.full((q, p), float("nan"), dtype=torch.float64, device="cuda")
        th = torch.full((q, p), float("nan"), dtype=torch.float64, device="cuda")
        dh = torch.empty(p, dtype=torch.float64, device="cuda")
        call("obhip_fit_newton_multi_dev", comm, basis, self.t._h, self.om._h, dY.data_ptr(), q,
             dY.shape[1], sigma, RHO, H.data_ptr(), g.data_ptr(), th.data_ptr(), dh.data_ptr(),
             None if ex is None else ex.data_ptr(), 0 if ex is None else ex.numel(), ws.data_ptr(), wsb.value)
        torch.cuda.synchronize()
        return H, g, th, dh


# ---- 1. B^T Y ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,q,mode", [
    (5000, 300, 17, "whole"), (3001, 129, 40, "whole"), (2500, 260, 3, "whole"), (700, 1, 16, "whole"),
    (1500, 300, 1, "whole"), (2500, 260, 9, "whole"), (5000, 260, 17, "chunk"), (3001, 129, 16, "backend3")])
def test_bty_against_the_exact_product(n, p, q, mode, monkeypatch):
    """B^T Y of the fit entry against the product formed in np.longdouble from obhip_basis_getmat's
    B.  Every entry within the dot-product rounding bound (n + 2 d) 2^-53 (|B|^T |Y|)_kj, which
    holds for any summation order (2 d: the at most d + 1 factors of an entry of B multiplied in
    another order than getmat does).  The column loop over obhip_basis_tmm_dev is measured against
    the same bound; should IT break the bound somewhere, the batched kernel is held to the project's
    device-against-device figure instead, 1e-11 normwise (tests/test_gpu_star.py:85).
    whole: B staged whole (k_aty_multi once eight columns are left beside response 0, the column
    loop below that: q = 3); chunk / backend3: B not resident, the column loop."""
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call, lib
    c = _Case(n, p, q)
    if mode == "chunk":
        monkeypatch.setenv("OBHIP_GRAM_CHUNK_ROWS", "1024")
    if mode == "backend3":
        call("obhip_set_gram_backend", 3)
    basis = c.basis()
    try:
        dY = _dev(c.Y)
        _, g, _, _ = c.fit(basis, dY)
        got = g.cpu().numpy().T
        loop = torch.empty((q, p), dtype=torch.float64, device="cuda")
        for j in range(q):
            call("obhip_basis_tmm_dev", basis, c.t._h, dY[j].data_ptr(), loop[j].data_ptr(), 0)
        torch.cuda.synchronize()
        loop = loop.cpu().numpy().T
        # B of THIS basis (its level caps decide how the basis columns are evaluated)
        B = np.empty((n, p), order="F")
        call("obhip_basis_getmat", basis, c.t._h, B.ctypes.data)
    finally:
        lib.obhip_basis_destroy(basis)
        call("obhip_set_gram_backend", 0)
    exact = np.asarray(B.T, dtype=np.longdouble) @ np.asarray(c.Y, dtype=np.longdouble)
    bound = np.asarray((n + 2 * c.d) * U * (np.abs(B).T @ np.abs(c.Y)), dtype=np.float64)
    r_new = float(np.max(np.abs(np.asarray(got - exact, dtype=np.float64)) / bound))
    r_loop = float(np.max(np.abs(np.asarray(loop - exact, dtype=np.float64)) / bound))
    print("B^T Y %s n=%d p=%d q=%d: error / bound batched %.3g, column loop %.3g" % (mode, n, p, q, r_new, r_loop))
    assert np.all(np.isfinite(got))
    if r_loop <= 1.0:
        assert r_new <= 1.0
    else:  # the existing kernel is outside the theorem's bound: device against device
        assert np.linalg.norm(got - loop) <= 1e-11 * np.linalg.norm(loop)


# ---- 2. the solves --------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,ncheck", [(129, 17, None), (260, 40, None), (1, 3, None), (1500, 16, None),
                                        (4096, 17, 2)])
def test_multi_solve_backward_error(p, q, ncheck):
    """obhip_newton_multi_solve_dev on a G kept aside: per column the normwise backward error
    eta_j = ||H theta_j - r_j||_inf / (||H||_inf ||theta_j||_inf + ||r_j||_inf), in extended
    precision on the host -- independent of the (poor) conditioning of H -- must stay within
    max(4 eta_single_j, p 2^-53), eta_single_j the same for obhip_newton_solve_dev on that column:
    the other blocking of the substitution changes the constant of the rounding bound, not its
    order.  (p = 4096: eta_single of two columns; the others are held to the smaller of the two.)"""
    import outerbase_amd as ob
    from multi_schedule_worker import allowed, solve_case
    kinds = ["mat25"] * 6
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 40))
    em, es, cols = solve_case(om, p, q, ncheck)
    lim = allowed(em, es, cols, p)
    print("solve p=%d q=%d: eta batched max %.3g (columns %s: %s), single %s, largest eta / allowed %.3g"
          % (p, q, em.max(), cols[:4], em[cols[:4]], es[:4], np.max(em / lim)))
    assert np.all(np.isfinite(em)) and np.all(em <= lim)


@pytest.mark.parametrize("panels", [1, 2, 8])
def test_multi_solve_under_forced_cholesky_schedules(panels):
    """The batched substitution reads the factor and the 16 x 16 inverses the panel step leaves in
    the workspace; their place depends on the schedule (OBHIP_CHOL_PANELS, read once per process):
    the same backward-error criterion in a child process per schedule."""
    sizes = [1, 64, 129, 260, 1000]
    env = dict(os.environ, OBHIP_CHOL_PANELS=str(panels))
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_schedule_worker.py")
    r = subprocess.run([sys.executable, worker, "17"] + [str(v) for v in sizes], env=env, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("ok", "BAD"))]
    assert [int(ln[1]) for ln in lines] == sizes, r.stdout
    assert all(ln[0] == "ok" for ln in lines), r.stdout


# ---- 3. the predictor ---------------------------------------------------------------------------
@pytest.mark.parametrize("nnew,p,q,generic", [
    (1000, 300, 17, False), (192, 129, 3, False), (777, 260, 40, False), (1000, 300, 16, False),
    (333, 1, 17, False), (500, 300, 1, False), (192, 129, 9, False), (1000, 300, 17, True), (0, 129, 16, False)])
def test_predict_multi_against_the_single_predictor(nnew, p, q, generic, monkeypatch):
    """Column j of obhip_predict_multi_dev against obhip_predict_dev on theta_j: the two may differ
    by summation order only, |delta_i| <= (p + 2 d) 2^-53 (|B(xnew)| |theta_j|)_i with |B| from
    getmat on the new rows; the variance likewise against the single path's.  Both sides of the
    fused kernel's domain limit (OBHIP_FORCE_GENERIC takes the column loop, and so do fewer than
    eight columns beside response 0: q = 3), n not a multiple of the 64-row tile, n = 0."""
    import torch
    import ob_oracle as O
    import outerbase_amd as ob
    from outerbase_amd._lib import call
    c = _Case(1200, p, q)
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    rng = np.random.default_rng(11)
    sd = np.sqrt(c.om.getvar(c.terms))
    Theta = rng.standard_normal((p, q)) * sd[:, None]      # coefficients on the prior's scale
    cv = rng.random(p) * sd ** 2
    dT, dcv = _dev(Theta), _dev(cv)
    if nnew == 0:
        mean = torch.full((q, 4), 7.0, dtype=torch.float64, device="cuda")
        call("obhip_predict_multi_dev", c.om._h, c.t._h, dT.data_ptr(), q, None, 0, mean.data_ptr(), None, SIGMA, None)
        torch.cuda.synchronize()
        assert bool((mean == 7.0).all())
        return
    xn, _ = O.synth_xy(9, 0, nnew, c.kinds)
    dx = _dev(xn)
    mean = torch.full((q, nnew), float("nan"), dtype=torch.float64, device="cuda")
    var = torch.full((nnew,), float("nan"), dtype=torch.float64, device="cuda")
    call("obhip_predict_multi_dev", c.om._h, c.t._h, dT.data_ptr(), q, dx.data_ptr(), nnew, mean.data_ptr(),
         dcv.data_ptr(), SIGMA, var.data_ptr())
    one = torch.empty((q, nnew), dtype=torch.float64, device="cuda")
    var1 = torch.empty(nnew, dtype=torch.float64, device="cuda")
    for j in range(q):
        call("obhip_predict_dev", c.om._h, c.t._h, dT[j].data_ptr(), dx.data_ptr(), nnew, one[j].data_ptr(),
             dcv.data_ptr(), SIGMA, var1.data_ptr())
    torch.cuda.synchronize()
    B = np.abs(ob.outerbase(c.om, xn, levelcap=c.t.maxlevels()).getmat(c.terms))
    bound = (p + 2 * c.d) * U * (B @ np.abs(Theta))
    diff = np.abs(mean.cpu().numpy().T - one.cpu().numpy().T)
    ratio = float(np.max(diff / bound))
    vb = (p + 2 * c.d) * U * ((B * B) @ cv + math.exp(2 * SIGMA))
    vratio = float(np.max(np.abs(var.cpu().numpy() - var1.cpu().numpy()) / vb))
    print("predict n=%d p=%d q=%d generic=%s: |multi - single| / bound mean %.3g var %.3g, normwise %.3g"
          % (nnew, p, q, generic, ratio, vratio, diff.max() / np.abs(one.cpu().numpy()).max()))
    assert np.all(np.isfinite(mean.cpu().numpy()))
    assert ratio <= 1.0 and vratio <= 1.0


# ---- 4. end to end against the oracle -----------------------------------------------------------
@pytest.mark.parametrize("n,p,q", [(1500, 129, 3), (3000, 300, 17)])
def test_fit_and_predict_against_the_oracle(n, p, q):
    """outerbase_amd.fit_newton_multi (+ predict) column by column against O.fit_newton and
    O.predict_mean at the project's own 1e-6 relative (BASELINE north_star,
    test_fit_newton_sharded_entry_equals_the_composed_calls)."""
    import ob_oracle as O
    import outerbase_amd as ob
    c = _Case(n, p, q)
    fit = ob.fit_newton_multi(c.om, c.terms, c.x, c.Yraw)
    assert fit.coeff.shape == (p, q) and fit.y_cent.shape == (q,) and fit.diagH.shape == (p,)
    assert np.allclose(fit.y_cent, c.Yraw.mean(axis=0), rtol=1e-13)
    assert np.allclose(fit.y_sca, c.Yraw.std(axis=0, ddof=1), rtol=1e-12)
    mean, var = fit.predict(c.xnew, var=True)
    assert mean.shape == (c.xnew.shape[0], q) and var.shape == mean.shape
    obo = O.OuterBase(c.om_o, c.x)
    worst_t = worst_m = 0.0
    for j in range(q):
        theta_o, H = O.fit_newton(obo, c.terms, c.Y[:, j], sigma=SIGMA)
        worst_t = max(worst_t, np.max(np.abs(fit.coeff[:, j] - theta_o)) / np.max(np.abs(theta_o)))
        want = fit.y_cent[j] + fit.y_sca[j] * O.predict_mean(c.om_o, c.terms, theta_o, c.xnew)
        worst_m = max(worst_m, np.max(np.abs(mean[:, j] - want)) / np.max(np.abs(want)))
    print("oracle n=%d p=%d q=%d: theta %.3g mean %.3g (relative, worst column)" % (n, p, q, worst_t, worst_m))
    assert worst_t < 1e-6 and worst_m < 1e-6
    assert np.allclose(fit.diagH, np.diag(H), rtol=1e-10)
    # var: the single path's diagonal form, scaled per response
    B = ob.outerbase(c.om, c.xnew, levelcap=c.t.maxlevels()).getmat(c.terms)
    v0 = (B * B) @ (1.0 / fit.diagH) + math.exp(2 * SIGMA)
    assert np.allclose(var, v0[:, None] * fit.y_sca[None, :] ** 2, rtol=1e-10)
    assert fit.predict(np.zeros((0, c.d))).shape == (0, q)


# ---- 5. standardisation ---------------------------------------------------------------------------
def test_standardise_multi_equals_the_single_entry_per_column():
    """Per column what obhip_standardise_dev gives (to what test_standardise_dev_is_two_pass
    allows; the summation order is the same, so in fact the same bits), with ldy > n, a column
    1e7 standard deviations from zero, and a constant column that does not disturb its neighbours;
    de-standardisation of means and variances."""
    import torch
    from outerbase_amd._lib import call
    rng = np.random.default_rng(3)
    n, q, ld = 70001, 5, 70001 + 13
    Y = rng.standard_normal((n, q))
    Y[:, 1] += 1e7
    Y[:, 3] = 4.25
    buf = torch.full((q, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(Y.T)).cuda()
    out = torch.full((q, ld), -3.0, dtype=torch.float64, device="cuda")
    ms = torch.zeros((q, 3), dtype=torch.float64, device="cuda")
    call("obhip_standardise_multi_dev", None, buf.data_ptr(), n, q, ld, out.data_ptr(), ms.data_ptr())
    torch.cuda.synchronize()
    assert bool((out[:, n:] == -3.0).all())                 # the padding rows of ldy are not touched
    same_bits = True
    for j in range(q):
        yj = buf[j, :n].contiguous()
        o1 = torch.empty_like(yj)
        m1 = torch.zeros(3, dtype=torch.float64, device="cuda")
        call("obhip_standardise_dev", None, yj.data_ptr(), n, o1.data_ptr(), m1.data_ptr())
        torch.cuda.synchronize()
        a, b = ms[j].cpu().numpy(), m1.cpu().numpy()
        same_bits &= bool(torch.equal(ms[j], m1)) and np.array_equal(out[j, :n].cpu().numpy(), o1.cpu().numpy(), equal_nan=True)
        assert abs(a[0] - b[0]) <= 1e-15 * abs(b[0]) + 1e-16 and a[2] == n
        if j == 3:
            assert a[1] == 0.0 and b[1] == 0.0 and not np.isfinite(out[j, :n].cpu().numpy()).any()
            continue
        assert abs(a[1] - b[1]) < 1e-12 * b[1]
        assert np.max(np.abs(out[j, :n].cpu().numpy() - o1.cpu().numpy())) < (1e-8 if j == 1 else 1e-13)
        cent, sd = Y[:, j].mean(), Y[:, j].std(ddof=1)
        assert abs(a[0] - cent) <= 1e-15 * abs(cent) + 1e-16 and abs(a[1] - sd) < 1e-12 * sd
    print("standardise_multi: same bits as the single entry:", same_bits)
    back = out.clone()
    call("obhip_destandardise_multi_dev", back.data_ptr(), n, q, ld, ms.data_ptr(), 0)
    v = torch.full((q, ld), 2.0, dtype=torch.float64, device="cuda")
    call("obhip_destandardise_multi_dev", v.data_ptr(), n, q, ld, ms.data_ptr(), 1)
    torch.cuda.synchronize()
    for j in (0, 1, 2, 4):
        assert np.max(np.abs(back[j, :n].cpu().numpy() - Y[:, j])) < 1e-15 * (abs(Y[:, j]).max() + 10)
        sd = Y[:, j].std(ddof=1)
        assert np.allclose(v[j, :n].cpu().numpy(), 2.0 * sd * sd, rtol=1e-12) and bool((v[j, n:] == 2.0).all())


# ---- 6. sharding -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,q", [(3000, 300, 17), (1500, 129, 3)])
def test_one_rank_communicator_reproduces_the_fit_and_fills_the_exchange_buffer(n, p, q):
    """A one-rank host communicator: packed triangle and B^T Y into the exchange buffer ->
    exchange (identity) -> unpack forms H.  Same Theta, diagH, B^T Y and factor as comm = NULL; the
    buffer holds the raw packed G, then B^T Y (p x q, column-major), then zeros."""
    import torch
    from outerbase_amd._lib import call, lib
    c = _Case(n, p, q)
    basis = c.basis()
    try:
        dY = _dev(c.Y)
        c.fit(basis, dY)      # stages the design matrix: response 0 rides along that pass only
        H0, g0, th0, dh0 = c.fit(basis, dY)
        comm = C.c_void_p()
        call("obhip_comm_init_host", C.byref(comm), 1, 0, None, None)
        cnt = C.c_uint64(0)
        call("obhip_fit_newton_multi_count", p, q, 1, C.byref(cnt))
        ex = torch.zeros(cnt.value, dtype=torch.float64, device="cuda")
        H1, g1, th1, dh1 = c.fit(basis, dY, comm=comm, ex=ex)
        lib.obhip_comm_destroy(comm)
        G = torch.empty((p, p), dtype=torch.float64, device="cuda")
        call("obhip_gram_dev", basis, c.t._h, None, G.data_ptr(), None)
        torch.cuda.synchronize()
    finally:
        lib.obhip_basis_destroy(basis)
    tri = p * (p + 1) // 2
    hb = ex.cpu().numpy()
    assert np.array_equal(hb[:tri], G.cpu().numpy()[np.triu_indices(p)])
    assert np.array_equal(hb[tri:tri + p * q], g0.cpu().numpy().ravel()) and not hb[tri + p * q:].any()
    assert torch.equal(g0, g1) and torch.equal(th0, th1) and torch.equal(dh0, dh1)
    assert torch.equal(torch.tril(H0), torch.tril(H1))


def test_sim_ranks_multi_fit_is_the_fit_of_the_shard_repeated():
    """obhip_comm_init_sim(N) under MultiHotPath, following
    test_sim_ranks_fit_is_the_fit_of_the_shard_repeated: the fit of N virtual ranks holding this
    process's rows is the one-rank fit of those rows repeated N times, for every response."""
    import torch
    from outerbase_amd.driver import MultiHotPath
    kinds = ["mat25", "mat25pow", "mat25"]
    N, n, p, q = 4, 3000, 150, 17
    sim = MultiHotPath(kinds, 20, p, n, rank=0, world=N, transport="sim", row0=0, n_total=N * n, responses=q)
    sim.setup()
    assert sim.comm_info()["path"].startswith("sim")
    sim.step()
    torch.cuda.synchronize()
    one = MultiHotPath(kinds, 20, p, N * n, terms=sim.terms, responses=q)
    one.setup()
    one.x.copy_(sim.x.repeat(1, N))
    one.xnew.copy_(sim.xnew.repeat(1, N))
    one.Y_raw.copy_(sim.Y_raw.repeat(1, N))
    one.step()
    torch.cuda.synchronize()
    ms, mo = sim.Meansd.cpu().numpy(), one.Meansd.cpu().numpy()
    assert np.all(np.abs(ms[:, 0] - mo[:, 0]) < 1e-13 * np.abs(ms[:, 0])) and np.all(np.abs(ms[:, 1] - mo[:, 1]) < 1e-12)
    assert np.all(ms[:, 2] == N * n)
    ts, to = sim.Theta.cpu().numpy(), one.Theta.cpu().numpy()
    for j in range(q):
        assert np.max(np.abs(ts[j] - to[j])) < 1e-8 * np.max(np.abs(to[j]))
    a, b = sim.Mean.cpu().numpy(), one.Mean[:, :n].cpu().numpy()
    for j in range(q):
        assert np.max(np.abs(a[j] - b[j])) < 1e-9 * np.max(np.abs(b[j]))
    assert sim.newton_residual_rel() < 1e-10
    sim.close()
    one.close()


def test_multi_hot_path_with_one_response_is_the_hot_path():
    """q = 1 takes the single-response code path throughout: the same bits as HotPath."""
    import torch
    from outerbase_amd.driver import HotPath, MultiHotPath
    kinds = ["mat25", "mat25pow", "mat25"]
    a = HotPath(kinds, 20, 150, 3000)
    b = MultiHotPath(kinds, 20, 150, 3000, responses=1)
    for h in (a, b):
        h.setup()
        h.step()
    torch.cuda.synchronize()
    assert torch.equal(a.theta, b.Theta[0]) and torch.equal(a.mean, b.Mean[0]) and torch.equal(a.g, b.Grhs[0])
    assert torch.equal(a.meansd, b.Meansd[0]) and torch.equal(a.diagH, b.diagH)
    a.close()
    b.close()


# ---- 7. repeatability --------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    import torch
    from outerbase_amd._lib import call, lib
    c = _Case(5000, 300, 40)
    basis = c.basis()
    try:
        dY = _dev(c.Y)
        r1 = c.fit(basis, dY)
        call("obhip_basis_rebuild", basis)       # the staging pass runs again: response 0 rides along
        r2 = c.fit(basis, dY)
        r3 = c.fit(basis, dY)                     # the staged matrix is still valid: response 0 by its own pass
        r4 = c.fit(basis, dY)
    finally:
        lib.obhip_basis_destroy(basis)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    for a, b in zip(r3, r4):
        assert torch.equal(a, b)
    dx = _dev(c.xnew)
    n = c.xnew.shape[0]
    m = [torch.empty((c.q, n), dtype=torch.float64, device="cuda") for _ in range(2)]
    for mm in m:
        call("obhip_predict_multi_dev", c.om._h, c.t._h, r1[2].data_ptr(), c.q, dx.data_ptr(), n, mm.data_ptr(),
             None, SIGMA, None)
    torch.cuda.synchronize()
    assert torch.equal(m[0], m[1])


# ---- 8. errors -------------------------------------------------------------------------------------------
def test_multi_entries_report_errors():
    """A Hessian that is not positive definite (the recipe of
    test_newton_solve_reports_a_hessian_that_is_not_positive_definite: a handled numeric error) is
    OBHIP_ERR_NUMERIC; null and too-small buffers are OBHIP_ERR_INVALID."""
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call, lib
    kinds = ["mat25"] * 6
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 40))
    p, q, bad_at = 200, 5, 130
    terms = om.selectterms(p)
    t = ob.obmod._Terms(om, terms)
    torch.manual_seed(1)
    A = torch.randn((p, p + 3), dtype=torch.float64, device="cuda")
    G = A @ A.T + 0.5 * torch.eye(p, dtype=torch.float64, device="cuda")
    good = G.clone()
    G[bad_at, bad_at] = -1e15
    R = torch.randn((q, p), dtype=torch.float64, device="cuda")
    wsb = C.c_uint64(0)
    call("obhip_newton_multi_workspace_bytes", p, q, C.byref(wsb))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
    th = torch.empty((q, p), dtype=torch.float64, device="cuda")
    with pytest.raises(ob.ObhipError, match="not positive definite") as ei:
        call("obhip_newton_multi_solve_dev", om._h, t._h, G.data_ptr(), R.data_ptr(), q, 0.3, 2.0, th.data_ptr(),
             None, ws.data_ptr(), wsb.value)
    assert ei.value.code == 5 and "column %d" % (bad_at // 64 * 64) in str(ei.value)
    args = (om._h, t._h, good.data_ptr(), R.data_ptr(), q, 0.3, 2.0, th.data_ptr(), None, ws.data_ptr())
    assert lib.obhip_newton_multi_solve_dev(*args, wsb.value - 8) == 1
    assert lib.obhip_newton_multi_solve_dev(om._h, t._h, None, R.data_ptr(), q, 0.3, 2.0, th.data_ptr(), None,
                                            ws.data_ptr(), wsb.value) == 1
    assert lib.obhip_newton_multi_solve_dev(om._h, t._h, good.data_ptr(), R.data_ptr(), 0, 0.3, 2.0, th.data_ptr(),
                                            None, ws.data_ptr(), wsb.value) == 1
    # the fit entry: null Y, ldy below the rows, a workspace or an exchange buffer too small
    c = _Case(700, 60, 3)
    basis = c.basis()
    try:
        dY = _dev(c.Y)
        call("obhip_newton_multi_workspace_bytes", c.p, 3, C.byref(wsb))
        ws = torch.empty(wsb.value, dtype=torch.uint8, device="cuda")
        H = torch.empty((c.p, c.p), dtype=torch.float64, device="cuda")
        g = torch.empty((3, c.p), dtype=torch.float64, device="cuda")
        th = torch.empty((3, c.p), dtype=torch.float64, device="cuda")

        def fit(comm=None, y=dY.data_ptr(), ldy=700, ex=None, exn=0, w=wsb.value):
            return lib.obhip_fit_newton_multi_dev(comm, basis, c.t._h, c.om._h, y, 3, ldy, SIGMA, RHO, H.data_ptr(),
                                                  g.data_ptr(), th.data_ptr(), None, ex, exn, ws.data_ptr(), w)
        assert fit() == 0
        assert fit(y=None) == 1 and fit(ldy=699) == 1 and fit(w=wsb.value - 8) == 1
        comm = C.c_void_p()
        call("obhip_comm_init_host", C.byref(comm), 1, 0, None, None)
        cnt = C.c_uint64(0)
        call("obhip_fit_newton_multi_count", c.p, 3, 1, C.byref(cnt))
        ex = torch.zeros(cnt.value, dtype=torch.float64, device="cuda")
        assert fit(comm=comm, ex=ex.data_ptr(), exn=cnt.value - 1) == 1 and fit(comm=comm) == 1
        assert fit(comm=comm, ex=ex.data_ptr(), exn=cnt.value) == 0
        lib.obhip_comm_destroy(comm)
        assert lib.obhip_predict_multi_dev(c.om._h, c.t._h, None, 3, c.dx.data_ptr(), 700, g.data_ptr(), None, SIGMA,
                                           None) == 1
        assert lib.obhip_standardise_multi_dev(None, dY.data_ptr(), 700, 3, 699, dY.data_ptr(), g.data_ptr()) == 1
        assert lib.obhip_standardise_multi_dev(None, dY.data_ptr(), 700, 0, 700, dY.data_ptr(), g.data_ptr()) == 1
    finally:
        lib.obhip_basis_destroy(basis)
    torch.cuda.synchronize()
