"""The Jacobian and vector-Jacobian product of the multi-response predictor on the GPU
(obhip_predict_jac_multi_dev, obhip_predict_vjp_multi_dev and what is built on them) against the
extended-precision reference of tests/extended_jac_ref.py: every entry of mean, jac and vjp within
its own tolerance (C . bound + gamma . sum |summands|, C as in test_gpu_predict_grad.py).  The
coefficient columns are scaled 1e-3 .. 1e3, so that cross-talk between responses or response blocks
cannot hide under a flat norm.  Fused kernel and the per-response fallback, the edges of the 64-row
tile, of the 16-response block and of the 64-response chunk, q = 1, determinism, optional outputs,
MultiFit and the torch module."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_dx_ref as X
import extended_jac_ref as J
import extended_ref as E
from conftest import sample_x
from test_gpu_predict_grad import NS, _destandardised, case, model, run_dev, wide

pytestmark = pytest.mark.gpu

QS = (2, 3, 16, 17, 33, 65)       # both sides of the 16-response block and of the 64-response chunk
QMAX = 65
NAN = float("nan")


def _theta(p, seed):
    return np.random.default_rng(seed).standard_normal((p, QMAX)) * J.response_scales(QMAX)[None, :]


@functools.lru_cache(maxsize=None)
def jcase(name, p, kind="select"):
    """the case of test_gpu_predict_grad with QMAX coefficient columns, random weights and the
    reference values with their tolerances on all rows, computed once; a call with q responses on
    the first n rows is compared with that corner of these"""
    m, c = model(name), case(name, p, kind)
    pp = len(c["terms"])
    Theta = _theta(pp, 100 + pp)
    W = np.random.default_rng(200 + pp).standard_normal((len(m["x"]), QMAX))
    jac, tol = J.ref_jac(m["ref"], c["terms"], Theta, c["C"])
    return dict(terms=c["terms"], Theta=Theta, W=W, mean=J.ref_mean(m["ref"], c["terms"], Theta, c["C"]),
                jac=(jac, tol), om_d=m["om_d"], x=m["x"])


@functools.lru_cache(maxsize=None)
def wide_case():
    kinds, om_o, om_d, terms, used, x = wide()
    ref = X.reference_dx_of(om_o, x)
    Cc = E.constant_from_oracle_ratio(X.f64_ratio(ref, om_o, x, terms))
    Theta = _theta(len(terms), 7)
    W = np.random.default_rng(8).standard_normal((len(x), QMAX))
    return dict(terms=terms, Theta=Theta, W=W, mean=J.ref_mean(ref, terms, Theta, Cc),
                jac=J.ref_jac(ref, terms, Theta, Cc), om_d=om_d, x=x)


def _setup(om_d, terms, Theta, x):
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call
    t = ob.obmod._terms_of(om_d, terms)
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    return torch, call, t, dev, dx, dth


def run_jac(om_d, terms, Theta, x, want_mean=True):
    """obhip_predict_jac_multi_dev on torch buffers pre-filled with NaN -> (mean n x q, jac n x d x q)"""
    torch, call, t, dev, dx, dth = _setup(om_d, terms, Theta, x)
    (n, d), q = x.shape, Theta.shape[1]
    mean = torch.full((q, n), NAN, dtype=torch.float64, device=dev)
    jac = torch.full((q, d, n), NAN, dtype=torch.float64, device=dev)
    call("obhip_predict_jac_multi_dev", om_d._h, t._h, dth.data_ptr(), q, dx.data_ptr(), n,
         mean.data_ptr() if want_mean else None, jac.data_ptr())
    torch.cuda.synchronize()
    return mean.cpu().numpy().T, jac.permute(2, 1, 0).cpu().numpy()


def run_vjp(om_d, terms, Theta, x, W, want_mean=True, pad=0):
    """obhip_predict_vjp_multi_dev -> (mean n x q, out n x d); W with ldw = n + pad, the padding NaN"""
    torch, call, t, dev, dx, dth = _setup(om_d, terms, Theta, x)
    (n, d), q = x.shape, Theta.shape[1]
    wp = np.full((q, n + pad), NAN)
    wp[:, :n] = W.T
    dw = torch.from_numpy(wp).to(dev)
    mean = torch.full((q, n), NAN, dtype=torch.float64, device=dev)
    out = torch.full((d, n), NAN, dtype=torch.float64, device=dev)
    call("obhip_predict_vjp_multi_dev", om_d._h, t._h, dth.data_ptr(), q, dx.data_ptr(), n, dw.data_ptr(), n + pad,
         mean.data_ptr() if want_mean else None, out.data_ptr())
    torch.cuda.synchronize()
    return mean.cpu().numpy().T, out.cpu().numpy().T


def check_jcase(c, label, ns=NS):
    lines, worst = [], {"mean": 0.0, "jac": 0.0, "vjp": 0.0}
    for n in ns:
        for q in QS:
            Theta, x, W = c["Theta"][:, :q], c["x"][:n], c["W"][:n, :q]
            mean, jac = run_jac(c["om_d"], c["terms"], Theta, x)
            mean2, out = run_vjp(c["om_d"], c["terms"], Theta, x, W)
            jw, jt = c["jac"][0][:n, :, :q], c["jac"][1][:n, :, :q]
            w = {"mean": max(E.worst_ratio(mean, c["mean"][0][:n, :q], c["mean"][1][:n, :q]),
                             E.worst_ratio(mean2, c["mean"][0][:n, :q], c["mean"][1][:n, :q])),
                 "jac": E.worst_ratio(jac, jw, jt),
                 "vjp": E.worst_ratio(out, *J.ref_vjp(jw, jt, W))}
            if max(w.values()) >= 1 or not np.array_equal(mean, mean2):
                lines.append("%s p=%d n=%d q=%d: err/tolerance %s%s" % (
                    label, len(c["terms"]), n, q, ", ".join("%s %.3g" % kv for kv in w.items()),
                    "" if np.array_equal(mean, mean2) else "; the two entries' means differ"))
            worst = {k: max(worst[k], w[k]) for k in w}
    print("%s p=%d: worst err/tolerance %s" % (label, len(c["terms"]), ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert not lines, "\n".join(lines)


CASES = [("d1", 2), ("d4", 1), ("d4", 65), ("d4", 300), ("d11", 300)]


@pytest.mark.parametrize("name,p", CASES)
def test_fused_kernel_against_extended_reference(name, p, monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_jcase(jcase(name, p), "fused " + name)


@pytest.mark.parametrize("name,p", CASES)
def test_fallback_against_extended_reference(name, p, monkeypatch):
    monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    check_jcase(jcase(name, p), "fallback " + name)


@pytest.mark.parametrize("generic", [False, True])
def test_terms_of_nine_to_eleven_factors(generic, monkeypatch):
    """any number of factors per term: the fused kernel reads the column lists from memory"""
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_jcase(jcase("d11", 40, "long"), "9-11 factors generic=%s" % generic)


def test_term_set_beyond_the_fused_domain(monkeypatch):
    """more used columns than the tile holds: the per-response route, with and without the switch"""
    c = wide_case()
    monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    check_jcase(c, "wide generic", ns=(65,))
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_jcase(c, "wide", ns=(65,))


@pytest.mark.parametrize("generic", [False, True])
def test_knot_loop(generic, monkeypatch):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_jcase(jcase("d4 knots130", 65), "knot loop generic=%s" % generic, ns=(65, 129))


def test_one_response_carries_the_bits_of_predict_grad_dev(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = jcase("d11", 300)
    for n in (63, 129):
        x, Theta = c["x"][:n], c["Theta"][:, 1:2]
        mean1, grad1, _, _ = run_dev(c["om_d"], c["terms"], Theta[:, 0].copy(), x)
        mean, jac = run_jac(c["om_d"], c["terms"], Theta, x)
        assert np.array_equal(mean[:, 0], mean1) and np.array_equal(jac[:, :, 0], grad1)
        mean, out = run_vjp(c["om_d"], c["terms"], Theta, x, np.ones((n, 1)))
        assert np.array_equal(mean[:, 0], mean1) and np.array_equal(out, grad1)


@pytest.mark.parametrize("generic", [False, True])
def test_two_calls_give_identical_bits(generic, monkeypatch):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = jcase("d11", 300)
    Theta, x, W = c["Theta"], c["x"], c["W"]
    a = run_jac(c["om_d"], c["terms"], Theta, x) + run_vjp(c["om_d"], c["terms"], Theta, x, W)
    b = run_jac(c["om_d"], c["terms"], Theta, x) + run_vjp(c["om_d"], c["terms"], Theta, x, W)
    assert all(np.all(np.isfinite(u)) for u in a)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("generic", [False, True])
def test_optional_outputs_do_not_change_the_bits(generic, monkeypatch):
    """d_mean = NULL leaves the Jacobian's and the VJP's bits unchanged, and the two entries give the
    same means; with ldw = n + 3 the padding of d_W, filled with NaN, is never read"""
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = jcase("d4", 300)
    n, q = 65, 33
    Theta, x, W = c["Theta"][:, :q], c["x"][:n], c["W"][:n, :q]
    mean, jac = run_jac(c["om_d"], c["terms"], Theta, x)
    nomean, jac2 = run_jac(c["om_d"], c["terms"], Theta, x, want_mean=False)
    assert np.all(np.isnan(nomean)) and np.array_equal(jac, jac2)
    mean3, out = run_vjp(c["om_d"], c["terms"], Theta, x, W)
    nomean, out2 = run_vjp(c["om_d"], c["terms"], Theta, x, W, want_mean=False)
    assert np.all(np.isnan(nomean)) and np.array_equal(out, out2) and np.array_equal(mean, mean3)
    mean4, out3 = run_vjp(c["om_d"], c["terms"], Theta, x, W, pad=3)
    assert np.all(np.isfinite(out3)) and np.array_equal(out, out3) and np.array_equal(mean, mean4)


@pytest.mark.parametrize("generic", [False, True])
def test_vjp_against_the_devices_own_jacobian(generic, monkeypatch):
    """a consistency check beside the reference check: both are within their tolerances of the same
    values, the einsum of the device's Jacobian is summed in long double"""
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    c = jcase("d11", 300)
    n = 129
    worst = 0.0
    for q in (17, 65):
        Theta, x, W = c["Theta"][:, :q], c["x"][:n], c["W"][:n, :q]
        _, jac = run_jac(c["om_d"], c["terms"], Theta, x)
        _, out = run_vjp(c["om_d"], c["terms"], Theta, x, W)
        _, tol = J.ref_vjp(c["jac"][0][:n, :, :q], c["jac"][1][:n, :, :q], W)
        own = np.einsum("ij,ilj->il", np.asarray(W, dtype=np.longdouble), np.asarray(jac, dtype=np.longdouble))
        worst = max(worst, E.worst_ratio(out, own, tol))
    print("vjp against einsum(W, device jac): %.3g of the reference tolerance" % worst)
    assert worst < 1


def test_python_entries(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    import outerbase_amd as ob
    c = jcase("d4", 65)
    n, q = 65, 17
    Theta, x, W = c["Theta"][:, :q], c["x"][:n], c["W"][:n, :q]
    mean, jac = ob.predict_jac(c["om_d"], c["terms"], Theta, x)
    mean_d, jac_d = run_jac(c["om_d"], c["terms"], Theta, x)
    assert mean.shape == (n, q) and jac.shape == (n, 4, q)
    assert np.array_equal(mean, mean_d) and np.array_equal(jac, jac_d)
    mean2, out = ob.predict_vjp(c["om_d"], c["terms"], Theta, x, W)
    mean_v, out_v = run_vjp(c["om_d"], c["terms"], Theta, x, W)
    assert out.shape == (n, 4) and np.array_equal(mean2, mean_v) and np.array_equal(out, out_v)
    m0, j0 = ob.predict_jac(c["om_d"], c["terms"], Theta, x[:0])
    assert m0.shape == (0, q) and j0.shape == (0, 4, q)


# ---- what is built on the entries ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(q):
    import outerbase_amd as ob
    m, c = model("d4"), case("d4", 65)
    rng = np.random.default_rng(9 + q)
    xtr = sample_x(rng, 400, m["kinds"])
    base = [np.sin(3 * xtr[:, 0]) + xtr[:, 1], 5.0 + 2.0 * xtr[:, 3] * xtr[:, 1], np.cos(xtr[:, 2]) * 0.1]
    Y = np.stack([base[j % 3] * (1.0 + 0.5 * j) + 0.3 * j * xtr[:, j % 4] for j in range(q)], axis=1)
    Y += 0.01 * rng.standard_normal(Y.shape)
    return ob.fit_newton_multi(m["om_d"], c["terms"], xtr, Y)


@pytest.mark.parametrize("q", [3, 17])
def test_multifit_predict_grad_and_vjp(q, monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    m, c = model("d4"), case("d4", 65)
    mf = fitted(q)
    n = 65
    x, ref = m["x"][:n], m["ref"]
    mean, grad = mf.predict_grad(x)
    assert mean.shape == (n, q) and grad.shape == (n, 4, q)
    mw, mt = J.ref_mean(ref, c["terms"], mf.coeff, c["C"])
    jw, jt = J.ref_jac(ref, c["terms"], mf.coeff, c["C"])
    mw, mt, jw, jt = mw[:n], mt[:n], jw[:n], jt[:n]
    worst = {"mean": 0.0, "grad": 0.0}
    for j in range(q):
        sca, cent = float(mf.y_sca[j]), float(mf.y_cent[j])
        worst["mean"] = max(worst["mean"], E.worst_ratio(mean[:, j], *_destandardised(mw[:, j], mt[:, j], sca, cent)))
        worst["grad"] = max(worst["grad"], E.worst_ratio(grad[:, :, j], *_destandardised(jw[:, :, j], jt[:, :, j], sca)))
    # the VJP: the device is handed W = fl(cot . y_sca), which is formed here in the same arithmetic
    cot = np.random.default_rng(q).standard_normal((n, q))
    W = cot * mf.y_sca[None, :]
    out = mf.vjp(x, cot)
    assert out.shape == (n, 4)
    vw, vt = J.ref_vjp(jw, jt, W)
    worst["vjp"] = E.worst_ratio(out, vw, vt)
    # against sum_j cot . grad of predict_grad, summed in long double: grad_j = fl(sca_j jac_j) is within
    # |sca_j| tol_j + gamma_1 |sca_j jac_j| of the truth and W_ij within gamma_1 of cot_ij sca_j, so the
    # two differ by at most the VJP's tolerance plus sum_j |cot_ij| (|sca_j| tol_ilj + 2 gamma_1 |sca_j jac_ilj|)
    own = np.einsum("ij,ilj->il", np.asarray(cot, dtype=np.longdouble), np.asarray(grad, dtype=np.longdouble))
    asca = np.abs(mf.y_sca)[None, None, :]
    extra = (np.abs(cot)[:, None, :] * (asca * jt + 2 * E.gamma(1) * asca * np.abs(E._f64(jw)))).sum(axis=2)
    worst["vjp vs grad"] = E.worst_ratio(out, own, vt + extra)
    print("MultiFit q=%d: err/tolerance %s" % (q, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1


def _interior_x(rng, n, knots):
    """rows from the middle half of every dimension's knot range"""
    return np.stack([np.min(k) + (np.max(k) - np.min(k)) * rng.uniform(0.25, 0.75, n) for k in knots], axis=1)


def test_torch_emulator(monkeypatch):
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    import torch
    import outerbase_amd as ob
    m = model("d4")
    mf = fitted(3)
    emu = mf.torch()
    assert isinstance(emu, ob.TorchEmulator) and isinstance(emu, torch.nn.Module)
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(31)
    # forward
    xn = m["x"][:65]
    y = emu(torch.from_numpy(xn).to(dev))
    want = mf.predict(xn)
    assert y.shape == (65, 3) and not y.requires_grad
    assert np.max(np.abs(y.cpu().numpy() - want)) <= 1e-12 * np.max(np.abs(want))
    # any layout: a transposed view gives the same bits
    xt = torch.from_numpy(np.ascontiguousarray(xn.T)).to(dev).t()
    assert not xt.is_contiguous() and torch.equal(emu(xt), y)
    # gradcheck with torch's float64 defaults
    xg = torch.from_numpy(_interior_x(rng, 5, m["knots"])).to(dev).requires_grad_(True)
    assert torch.autograd.gradcheck(emu, (xg,))
    # backward = MultiFit.vjp, bit for bit
    xs = _interior_x(rng, 70, m["knots"])
    cot = rng.standard_normal((70, 3))
    xv = torch.from_numpy(xs).to(dev).requires_grad_(True)
    (emu(xv) * torch.from_numpy(cot).to(dev)).sum().backward()
    assert np.array_equal(xv.grad.cpu().numpy(), mf.vjp(xs, cot))
    # what it refuses
    with pytest.raises(TypeError):
        emu(torch.from_numpy(xn.astype(np.float32)).to(dev))
    with pytest.raises(TypeError):
        emu(torch.from_numpy(xn))
    # one Adam step on || emu(x) - target ||^2
    target = torch.from_numpy(mf.predict(_interior_x(rng, 70, m["knots"]))).to(dev)
    xo = torch.from_numpy(xs).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([xo], lr=1e-4)
    loss0 = ((emu(xo) - target) ** 2).sum()
    opt.zero_grad()
    loss0.backward()
    opt.step()
    loss1 = ((emu(xo) - target) ** 2).sum()
    print("Adam step: loss %.6g -> %.6g" % (loss0.item(), loss1.item()))
    assert loss1.item() < loss0.item()
