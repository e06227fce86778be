"""The acquisition gradients on the device (csrc/acquire_dx.cpp, kernels_acquire_dx.hip) against the long-double
reference of tests/acquire_grad_ref.py, at the smallest shapes at which each part can go wrong:

    d3 p=5 at n = 1 / 63 / 64 / 65 / 129     the 64-row tile edge, two 128-row tiles of the stored product
    d3 p=1                                   the constant term alone: every view is empty, the gradient is the rho part
    d8 p=67, all three families mixed        two groups of 64 terms in the dense pass, eight dimensions = eight waves
    d5 p=130 n=300                           three term groups, five tiles, three chunks under chunk_rows = 128
    d4 p=65, 130 knots in one dimension      no interval tables there: the knot-loop derivative
    d11 p=40, 9 - 11 factors per term        beyond W2 = 4: the tile in pooled scratch whatever the switch says
    d=40 p=357, 198 used columns             the tile does not fit the LDS: outside the fused domain

Every case runs the four criteria in both directions and var_grad (no criterion), on its own route and again under
OBHIP_FORCE_GENERIC (read at every call, set per test as the neighbouring files do; each setting once more in a fresh
process that was started with it).  The conditions of the cases are
asserted on the reference alone by test_acquire_grad_host.py and again here before the device is looked at.  Every entry
of all six outputs is held to the allowances of acquire_grad_ref.py, C eight times the float64 restatement's own
err / bound on the same case; every check prints err / tolerance.  Output buffers are padded with NaN and the padding
must stay as it was."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import acquire_grad_ref as R
import acquire_ref as A
import extended_ref as E
import posterior_ref as P

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3
FUSED = {"d3 p=5": True, "d3 p=1": True, "d8 p=67": True, "d5 p=130": True, "d4 knots130 p=65": True,
         "d11 9-11 factors": False, "wide d=40 p=357": False}
TILE_EDGES = (1, 63, 64, 65, 129)


def posterior_of(c):
    import outerbase_amd as ob
    return ob.Posterior.from_hessian(c.om_d, c.terms, c.H, c.sigma)


def set_route(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


def dev_grad(post, x, theta=None, cfg=None, chunk=0, want=R.QUANTITIES, noise=False):
    """obhip_acquire_grad_dev (cfg None: obhip_posterior_var_grad_dev) into NaN-padded buffers; what `want` leaves out
    is passed as NULL; the padding must come back untouched"""
    import torch
    from outerbase_amd._lib import call
    from outerbase_amd.design import ACQUISITIONS, _dev_cols, _stream
    dev = _stream()
    n, d = x.shape
    dx = _dev_cols(x, dev)
    buf = {q: torch.full(((n if q in ("score", "mean", "var") else n * d) + PAD,), NAN, dtype=torch.float64, device=dev)
           for q in want}
    ptr = lambda q: buf[q].data_ptr() if q in buf else None
    if cfg is None:
        call("obhip_posterior_var_grad_dev", post._h, dx.data_ptr(), n, chunk, int(noise), ptr("var"), ptr("grad_var"))
    else:
        dth = torch.from_numpy(np.ascontiguousarray(theta)).to(dev)
        params = (C.c_double * 4)(cfg.best, cfg.xi, cfg.kappa, cfg.level)
        call("obhip_acquire_grad_dev", post._h, dth.data_ptr(), dx.data_ptr(), n, ACQUISITIONS[cfg.criterion], params,
             int(cfg.maximize), chunk, ptr("score"), ptr("grad"), ptr("mean"), ptr("grad_mean"), ptr("var"),
             ptr("grad_var"))
    torch.cuda.synchronize()
    out = {}
    for q, b in buf.items():
        a = b.cpu().numpy()
        assert np.all(np.isnan(a[len(a) - PAD:])), "%s written beyond its end" % q
        out[q] = a[:n] if q in ("score", "mean", "var") else a[:n * d].reshape(d, n).T.copy()
    return out


def check(label, b, got, rows=None):
    """the conditions on the reference, then every entry of what the device returned"""
    c, cfg = b["c"], b["cfg"]
    assert 8 * b["r"] < E.C_CAP, label
    dmin, lmin = R.conditions(c, cfg, b["C"])
    assert dmin > 1000 and lmin > 1000, label
    w = R.ratios(got, b["ref"], b["C"], rows=rows)
    line = "acquire_grad | %s: C %.3g (float64 restatement err/bound %.3g); device err/tolerance %s" % (
        label, b["C"], b["r"], ", ".join("%s %.3g" % kv for kv in w.items()))
    print(line)
    assert max(w.values()) < 1, line
    return w


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("ci", range(8))
@pytest.mark.parametrize("name", list(R.CASES))
def test_every_entry_of_all_six_outputs_against_the_extended_reference(name, ci, generic, monkeypatch):
    set_route(monkeypatch, generic)
    b = R.built(name, ci)
    c, cfg = b["c"], b["cfg"]
    route = "generic" if generic else "own route"
    with posterior_of(c) as post:
        fused, lds, rows = post.acquire_grad_layout()
        assert fused == (FUSED[name] and not generic) and rows >= 128 and rows % 128 == 0
        assert lds <= 160 * 1024 and (lds > 16384) == fused
        for n in (TILE_EDGES if name == "d3 p=5" else (c.n,)):
            got = dev_grad(post, c.x[:n], c.theta, cfg)
            assert set(got) == set(R.QUANTITIES)
            check("%s n=%d %r %s" % (name, n, cfg, route), b, got, rows=n)


def fresh_process_check():
    """what the child of test_each_route_from_the_start_of_a_fresh_process runs: d5 p=130 n=300, the eight calls and
    var_grad against the reference, on whatever route the process was started with"""
    name = "d5 p=130"
    c = R.case(name)[0]
    with posterior_of(c) as post:
        print("fused %d" % post.acquire_grad_layout()[0])
        for ci in range(8):
            b = R.built(name, ci)
            check("%s %r fresh process" % (name, b["cfg"]), b, dev_grad(post, c.x, c.theta, b["cfg"]))
        check("%s var_grad fresh process" % name, R.built(name, 0), dev_grad(post, c.x, want=("var", "grad_var")))
    print("fresh process ok")


@pytest.mark.parametrize("generic", [False, True])
def test_each_route_from_the_start_of_a_fresh_process(generic):
    """the switch is read at every call, so the tests above set it in process; here each setting once more in a
    process that was started with it"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, PYTHONNOUSERSITE="1")
    env.pop("OBHIP_FORCE_GENERIC", None)
    if generic:
        env["OBHIP_FORCE_GENERIC"] = "1"
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_acquire_grad as T; T.fresh_process_check()"
            % (here, os.path.join(root, "oracle"), root))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fresh process ok" in out.stdout and ("fused 0" if generic else "fused 1") in out.stdout


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_variance_and_its_gradient_without_a_criterion(name, generic, monkeypatch):
    """obhip_posterior_var_grad_dev: within the allowance, the bits of the criterion call's var and grad_var, and the
    noise added to var alone"""
    set_route(monkeypatch, generic)
    b = R.built(name, 0)
    c = b["c"]
    with posterior_of(c) as post:
        got = dev_grad(post, c.x, want=("var", "grad_var"))
        full = dev_grad(post, c.x, c.theta, b["cfg"])
        noisy = dev_grad(post, c.x, want=("var", "grad_var"), noise=True)
    assert set(check("%s var_grad %s" % (name, "generic" if generic else "own route"), b, got)) == {"var", "grad_var"}
    for q in ("var", "grad_var"):
        assert np.array_equal(got[q], full[q]), q
    assert np.array_equal(noisy["grad_var"], got["grad_var"])
    nu = math.exp(2.0 * c.sigma)
    assert np.all(np.abs(noisy["var"] - (got["var"] + nu)) <= 4 * E.U * (got["var"] + nu))


@functools.lru_cache(maxsize=None)
def acquire_allowances(name, ci):
    """the allowances of acquire(k=1)'s score0, mean and var (acquire_ref.py, its own C) and of Posterior.var
    (posterior_ref.py, its own C) on the case's rows"""
    b = R.built(name, ci)
    c, cfg = b["c"], b["cfg"]
    picks, _, st = A.states(c.a, cfg, None, 1)
    Ca, ra = A.constant_of(c.a, cfg, st, picks)
    assert 8 * ra < E.C_CAP
    s0 = st[0]
    want, bound, rest, _ = P.ref_var(c.L, c.B, c.bB, c.sigma)
    Cv, rv = P.constant_of(P.host_var64(c.H, c.a.Bo, c.sigma), want, bound)
    assert 8 * rv < E.C_CAP
    # acquire returns mean and var AFTER its pick: under the believer the means stay, the variances drop by a_i^2 / gamma,
    # which the reference knows in long double (its state before the pick minus its state after it)
    assert len(picks) == 1 and len(st) == 2
    return dict(score=Ca * s0["bound_score"] + s0["rest_score"], mean=Ca * st[1]["bound_mu"], var=Ca * st[1]["bound_d"],
                drop=E._f64(s0["d"] - st[1]["d"]), post_var=P.tolerance(Cv, bound, rest))


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_values_against_acquire_and_posterior_var_on_the_same_rows(name, generic, monkeypatch):
    """score, mean and var against acquire(k=1)'s score0, mean and var, and var against Posterior.var: within the sum
    of the two allowances (acquire and Posterior.var form d as || L^-1 b ||^2, this entry as b^T (S b)).  acquire's
    var is the one after its pick: the reference's own long-double drop a_i^2 / gamma is taken off this entry's first"""
    set_route(monkeypatch, generic)
    c = R.case(name)[0]
    worst = {}
    with posterior_of(c) as post:
        pv = post.var(c.x)
        for ci in range(8):
            b = R.built(name, ci)
            cfg, al = b["cfg"], acquire_allowances(name, ci)
            par = dict(criterion=cfg.criterion, best=cfg.best, level=cfg.level, kappa=cfg.kappa, xi=cfg.xi,
                       maximize=cfg.maximize)
            res = post.acquire_grad(c.x, c.theta, **par)
            acq = post.acquire(c.x, c.theta, k=1, **par)
            mine = {q: R.allowance(b["ref"], q, b["C"]) for q in ("score", "mean", "var")}
            w = dict(score=np.max(np.abs(res.score - acq.score0) / (mine["score"] + al["score"])),
                     mean=np.max(np.abs(res.mean - acq.mean) / (mine["mean"] + al["mean"])),
                     var=np.max(np.abs(res.var - al["drop"] - acq.var) / (mine["var"] + al["var"])),
                     post_var=np.max(np.abs(res.var - pv) / (mine["var"] + al["post_var"])))
            assert res.criterion == cfg.criterion and res.grad.shape == (c.n, c.d)
            for q, v in w.items():
                worst[q] = max(worst.get(q, 0.0), float(v))
    print("acquire_grad | %s %s against acquire(k=1) and Posterior.var: difference / (sum of the two allowances) %s"
          % (name, "generic" if generic else "own route", ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1


@pytest.mark.parametrize("generic", [False, True])
def test_chunks_twins_and_repeats_give_the_same_bits(generic, monkeypatch):
    """d5 p=130 n=300: chunk_rows = 128 (three chunks, the last of 44 rows) against the unchunked call; a row copied
    to another tile, another lane and another chunk; the same call twice -- array_equal in every output"""
    set_route(monkeypatch, generic)
    name = "d5 p=130"
    c = R.case(name)[0]
    x = c.x.copy()
    x[261] = x[3]                                                   # tile 0 lane 3 | tile 4 lane 5, chunk 2 of 3
    x[130] = x[3]                                                   # tile 2 lane 2, chunk 1
    with posterior_of(c) as post:
        for ci in (R.cfg_index(A.EI, False), R.cfg_index(A.PI, True), R.cfg_index(A.STRADDLE, True)):
            cfg = R.built(name, ci)["cfg"]
            one = dev_grad(post, x, c.theta, cfg)
            two = dev_grad(post, x, c.theta, cfg)
            cut = dev_grad(post, x, c.theta, cfg, chunk=128)
            for q in R.QUANTITIES:
                assert np.all(np.isfinite(one[q])), q
                assert np.array_equal(one[q], two[q]), "two calls differ in %s" % q
                assert np.array_equal(one[q], cut[q]), "chunk_rows = 128 differs from the unchunked call in %s" % q
                assert np.array_equal(one[q][3], one[q][261]) and np.array_equal(one[q][3], one[q][130]), "twin rows differ in %s" % q
                assert not np.array_equal(one[q][3], one[q][4])
        v1 = dev_grad(post, x, want=("var", "grad_var"))
        v2 = dev_grad(post, x, want=("var", "grad_var"), chunk=256)
        for q in v1:
            assert np.array_equal(v1[q], v2[q]), q


@pytest.mark.parametrize("generic", [False, True])
def test_rows_that_are_not_finite_get_nan_and_disturb_nothing(generic, monkeypatch):
    set_route(monkeypatch, generic)
    name = "d5 p=130"
    c = R.case(name)[0]
    x = c.x.copy()
    bad = [5, 64, 299]
    x[5, 1], x[64, 0], x[299, 4] = NAN, float("inf"), -float("inf")
    keep = np.ones(c.n, dtype=bool)
    keep[bad] = False
    with posterior_of(c) as post:
        for ci in range(8):
            cfg = R.built(name, ci)["cfg"]
            clean, got = dev_grad(post, c.x, c.theta, cfg), dev_grad(post, x, c.theta, cfg)
            for q in R.QUANTITIES:
                assert np.all(np.isnan(got[q][bad])), q
                assert np.array_equal(got[q][keep], clean[q][keep]), q
        clean, got = dev_grad(post, c.x, want=("var", "grad_var")), dev_grad(post, x, want=("var", "grad_var"))
        for q in clean:
            assert np.all(np.isnan(got[q][bad])) and np.array_equal(got[q][keep], clean[q][keep]), q


def test_outputs_not_asked_for_are_not_needed_and_the_python_method_returns_the_entrys_bits():
    name = "d8 p=67"
    c = R.case(name)[0]
    with posterior_of(c) as post:
        for ci in range(8):
            cfg = R.built(name, ci)["cfg"]
            full = dev_grad(post, c.x, c.theta, cfg)
            for want in (("score", "grad"), ("score", "grad", "grad_var"), ("score", "grad", "mean", "var")):
                part = dev_grad(post, c.x, c.theta, cfg, want=want)
                assert set(part) == set(want)
                for q in want:
                    assert np.array_equal(part[q], full[q]), q
            res = post.acquire_grad(c.x, c.theta, criterion=cfg.criterion, best=cfg.best, level=cfg.level,
                                    kappa=cfg.kappa, xi=cfg.xi, maximize=cfg.maximize)
            for q in R.QUANTITIES:
                assert np.array_equal(getattr(res, q), full[q]), q
        v, g = post.var_grad(c.x)
        assert np.array_equal(v, full["var"]) and np.array_equal(g, full["grad_var"])


def test_response_scaling():
    """centre 8 and scale 4 -- powers of two, so that standardising best, level and xi on the way in and the scaling
    on the way out are exact: every output is the standardised call's, times sca (mean, ei, lcb, straddle and their
    gradients), times sca^2 (var and its gradient) or unchanged (pi); the centre is added to mean and to the lcb score
    and has no gradient"""
    name = "d8 p=67"
    c = R.case(name)[0]
    cen, sca = 8.0, 4.0
    with posterior_of(c) as post:
        post.meansd = np.array([[cen, sca, 40.0]])
        for ci in range(8):
            cfg = R.built(name, ci)["cfg"]
            std = post.acquire_grad(c.x, c.theta, criterion=cfg.criterion, best=cfg.best, level=cfg.level, kappa=cfg.kappa,
                                    xi=cfg.xi, maximize=cfg.maximize)
            raw = post.acquire_grad(c.x, c.theta, criterion=cfg.criterion, best=cen + sca * cfg.best,
                                    level=cen + sca * cfg.level, kappa=cfg.kappa, xi=sca * cfg.xi, maximize=cfg.maximize,
                                    response=0)
            assert np.array_equal(raw.mean, cen + sca * std.mean) and np.array_equal(raw.grad_mean, sca * std.grad_mean)
            assert np.array_equal(raw.var, sca ** 2 * std.var) and np.array_equal(raw.grad_var, sca ** 2 * std.grad_var)
            if cfg.criterion == A.PI:
                assert np.array_equal(raw.score, std.score) and np.array_equal(raw.grad, std.grad)
            else:
                off = 0.0 if cfg.criterion != A.LCB else (cen if cfg.maximize else -cen)
                assert np.array_equal(raw.score, sca * std.score + off) and np.array_equal(raw.grad, sca * std.grad)


@pytest.mark.parametrize("generic", [False, True])
def test_torch_module_forward_and_backward_are_the_entrys_bits(generic, monkeypatch):
    import torch
    import outerbase_amd as ob
    set_route(monkeypatch, generic)
    name = "d5 p=130"
    c = R.case(name)[0]
    rng = np.random.default_rng(9)
    with posterior_of(c) as post:
        for ci in range(8):
            cfg = R.built(name, ci)["cfg"]
            full = dev_grad(post, c.x, c.theta, cfg, want=("score", "grad"))
            acq = ob.TorchAcquisition(post, c.theta, criterion=cfg.criterion, best=cfg.best, level=cfg.level,
                                      kappa=cfg.kappa, xi=cfg.xi, maximize=cfg.maximize)
            x = torch.from_numpy(c.x).cuda().requires_grad_(True)
            score = acq(x)
            assert score.shape == (c.n,) and score.is_cuda and np.array_equal(score.detach().cpu().numpy(), full["score"])
            score.sum().backward()
            assert np.array_equal(x.grad.cpu().numpy(), full["grad"])
            cot = rng.standard_normal(c.n)
            x.grad = None
            (acq(x) * torch.from_numpy(cot).cuda()).sum().backward()
            assert np.array_equal(x.grad.cpu().numpy(), cot[:, None] * full["grad"])
        # once differentiable: a second derivative raises instead of returning zeros
        x = torch.from_numpy(c.x[:7]).cuda().requires_grad_(True)
        g, = torch.autograd.grad(acq(x).sum(), x, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
        # n = 0 and the argument checks
        assert acq(torch.zeros((0, c.d), dtype=torch.float64, device="cuda")).shape == (0,)
        with pytest.raises(TypeError):
            acq(torch.zeros((3, c.d), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            acq(torch.zeros((3, c.d + 1), dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            ob.TorchAcquisition(post, c.theta, criterion="ei")


def test_a_conditioned_handle_does_not_reuse_the_first_handles_inverse():
    """condition() on a handle that has formed its inv(H) returns a handle that forms its own: the bits of
    conditioning a handle that never formed one, and the values of a fresh Posterior.from_hessian of the conditioned H
    formed on the host, H2 = H + e^{-2 sigma} B^T B.  The device's H2 is the Gram kernels' float64 sum over 40 + 7 rows;
    a relative perturbation e of H moves b^T inv(H) b by at most cond(H) e relatively, so the two agree to
    64 (40 + 7) U cond(H2) d -- and the stale inverse would be off by orders of magnitude more."""
    import ob_oracle as O
    import outerbase_amd as ob
    name = "d8 p=67"
    c = R.case(name)[0]
    xnew = c.x[:7]
    Bn = O.ob_getmat(O.OuterBase(c.om_o, xnew), c.terms)
    H2 = c.H + math.exp(-2.0 * c.sigma) * (Bn.T @ Bn)
    H2 = (H2 + H2.T) / 2
    tol_rel = 64 * 47 * E.U * float(np.linalg.cond(H2))
    with posterior_of(c) as post, posterior_of(c) as plain:
        v0, g0 = post.var_grad(c.x)                                  # post has its inverse now
        with post.condition(xnew) as cond, plain.condition(xnew) as cond2, \
                ob.Posterior.from_hessian(c.om_d, c.terms, H2, c.sigma) as fresh:
            v1, g1 = cond.var_grad(c.x)
            v2, g2 = cond2.var_grad(c.x)
            v3, g3 = fresh.var_grad(c.x)
            pv = cond.var(c.x)
        v0b, g0b = post.var_grad(c.x)                                # and post still has its own
    assert np.array_equal(v1, v2) and np.array_equal(g1, g2)
    assert np.array_equal(v0, v0b) and np.array_equal(g0, g0b)
    rel = float(np.max(np.abs(v1 - v3) / v3))
    gscale = np.max(np.abs(g3), axis=0)
    relg = float(np.max(np.abs(g1 - g3) / gscale))
    stale = float(np.max(np.abs(v0 - v3) / v3))
    print("acquire_grad | conditioned handle against from_hessian(H2): var %.3g, gradient %.3g of its scale (allowed %.3g); "
          "the first handle's values are off by %.3g" % (rel, relg, tol_rel, stale))
    assert rel < tol_rel and relg < tol_rel and stale > 1000 * tol_rel
    assert np.all(np.abs(v1 - pv) <= 1e3 * tol_rel * pv)


def test_refused_calls_change_nothing_and_select_is_what_it_was():
    import torch
    from outerbase_amd._lib import lib
    c = R.case("d3 p=5")[0]
    with posterior_of(c) as post:
        with pytest.raises(ValueError):
            post.select(c.x, 2, criterion="ei")
        a = torch.full((1024,), NAN, dtype=torch.float64, device="cuda")
        x = torch.from_numpy(np.ascontiguousarray(c.x.T)).cuda()
        good = (C.c_double * 4)(0.0, 0.0, 1.96, 0.0)
        bad = (C.c_double * 4)(NAN, 0.0, 1.96, 0.0)
        f = lib.obhip_acquire_grad_dev
        p = a.data_ptr()
        assert f(post._h, p, x.data_ptr(), c.n, 0, bad, 0, 0, p, p, p, p, p, p) == 1       # best is NaN
        assert f(post._h, p, x.data_ptr(), c.n, 0, good, 0, 64, p, p, p, p, p, p) == 1     # chunk_rows
        assert f(post._h, p, x.data_ptr(), c.n, 0, good, 0, 0, p, None, p, p, p, p) == 1   # gradscore is required
        assert lib.obhip_posterior_var_grad_dev(post._h, x.data_ptr(), c.n, 100, 0, p, p) == 1
        assert lib.obhip_posterior_var_grad_dev(post._h, x.data_ptr(), c.n, 0, 0, p, None) == 1
        assert f(post._h, None, None, 0, 0, good, 0, 0, None, None, None, None, None, None) == 1   # theta even for n = 0
        assert f(post._h, p, None, 0, 0, good, 0, 0, None, None, None, None, None, None) == 0      # n = 0: a no-op
        assert lib.obhip_posterior_var_grad_dev(post._h, None, 0, 0, 0, None, None) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(a).all())


def test_the_cached_inverse_is_never_downdated_and_the_copy_is_the_fresh_product():
    """d5 p=130 n = m = 300: pp = 256, so the padding of S is live, and 300 rows are three 128-row tiles, the last
    ragged.  Handle A forms the inverse with its first acquire_grad (chunk_rows = 128), then selects (maxvar), acquires
    (ei, constant liar), selects (imse, 64 reference rows) -- three picks each, every pick a downdate of the entry's
    own copy of S -- and calls var_grad and acquire_grad again.  Handle B, fresh from the same Hessian, runs the
    selections and the acquisition first: it is their first call that forms the inverse, and the gradients come last.
    Every output of every call is the same on both, bit for bit, and so are A's first and last acquire_grad."""
    name = "d5 p=130"
    c = R.case(name)[0]
    cfg = next(b["cfg"] for b in (R.built(name, ci) for ci in range(8))
               if b["cfg"].criterion == A.EI and not b["cfg"].maximize)
    assert c.x.shape == (300, 5) and len(c.terms) == 130
    ei = dict(criterion="ei", best=cfg.best, xi=cfg.xi)
    picks = lambda post: (post.select(c.x, 3, criterion="maxvar"),
                          post.acquire(c.x, c.theta, k=3, lie="constant", **ei),
                          post.select(c.x, 3, criterion="imse", reference=c.x[:64]))
    with posterior_of(c) as pa, posterior_of(c) as pb:
        first = pa.acquire_grad(c.x, c.theta, chunk_rows=128, **ei)
        got_a = picks(pa) + (pa.var_grad(c.x), pa.acquire_grad(c.x, c.theta, **ei))
        got_b = picks(pb) + (pb.var_grad(c.x), pb.acquire_grad(c.x, c.theta, **ei))
    fields = lambda r: r if isinstance(r, tuple) else tuple(v for _, v in sorted(vars(r).items()))
    count = 0
    for ra, rb in zip(got_a + (first,), got_b + (got_a[-1],)):
        for va, vb in zip(fields(ra), fields(rb)):
            assert np.array_equal(va, vb, equal_nan=True) if isinstance(va, np.ndarray) else va == vb
            count += isinstance(va, np.ndarray)
    assert count == 4 + 5 + 4 + 2 + 6 + 6
    assert all(len(r.index) == 3 for r in got_a[:3])
