"""The Hessian-vector and Jacobian-vector product of the multi-response predictor on the GPU
(obhip_predict_hvp_multi_dev and what is built on it) against the extended-precision reference of
tests/extended_d2_ref.py: every entry of mean, vjp, jvp and hvp within its own tolerance
(C . bound + gamma . sum |summands|; C eight times the float64 normalised restatement's own
err / bound on the same case, which test_predict_hvp_host.py holds strictly below the cap).  The
coefficient columns and the rows of V are scaled 1e-3 .. 1e3, a few rows of V are zero.  Fused kernel
and the HBM-tile fallback, the edges of a 32- and a 64-row tile, of the 16-response block and of the
chunk, the constant term alone, 9-11 factors, an unused dimension, the d = 40 set outside the fused
domain, determinism, optional outputs, NaN rows, MultiFit and the torch module's double backward."""
import ctypes as C
import functools

import numpy as np
import pytest

import extended_d2_ref as D2
import extended_jac_ref as J
import extended_ref as E
from test_gpu_predict_grad import _destandardised, case, model, wide

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 63, 64, 65, 129)     # the edges of a 32- and of a 64-row tile
QS = (1, 2, 16, 17, 33)                   # both sides of the 16-response block and of the 32-response chunk
QMAX = 65
NAN = float("nan")
ld = np.longdouble

# (model, p, kind of term set): the cases of this file; test_predict_hvp_host.py asserts C < C_CAP on each
HCASES = [("d1", 2, "select"), ("d4", 1, "select"), ("d4", 2, "select"), ("d4", 65, "select"),
          ("d4", 300, "select"), ("d11", 300, "select"), ("d11", 40, "long"), ("d4 knots130", 65, "select")]


def _theta(p, seed):
    return np.random.default_rng(seed).standard_normal((p, QMAX)) * J.response_scales(QMAX)[None, :]


@functools.lru_cache(maxsize=None)
def d2_ref(name):
    m = model(name)
    return D2.reference_d2_of(m["om_o"], m["x"])


@functools.lru_cache(maxsize=None)
def hparts(name, p, kind="select"):
    """terms, V, the reference's per-term sums and the float64 restatement's err / bound of a case"""
    if name == "wide":
        kinds, om_o, om_d, terms, used, x = wide()
        ref = D2.reference_d2_of(om_o, x)
    else:
        m = model(name)
        om_o, om_d, x, terms, ref = m["om_o"], m["om_d"], m["x"], case(name, p, kind)["terms"], d2_ref(name)
    V = D2.direction_rows(len(x), x.shape[1], 300 + len(terms))
    hvt, jvt = ref.hv_terms(terms, V), ref.jv_terms(terms, V)
    ratio = D2.f64_ratio(ref, om_o, x, terms, V, (hvt, jvt))
    return dict(om_o=om_o, om_d=om_d, x=x, terms=terms, ref=ref, V=V, hvt=hvt, jvt=jvt, ratio=ratio)


@functools.lru_cache(maxsize=None)
def hcase(name, p, kind="select"):
    """hparts with QMAX coefficient columns, random weights and the reference values with their
    tolerances on all rows, computed once; a call with q responses on the first n rows is compared
    with that corner of these"""
    c = dict(hparts(name, p, kind))
    ref, terms, d = c["ref"], c["terms"], c["x"].shape[1]
    Cc = E.constant_from_oracle_ratio(c["ratio"])
    pp = len(terms)
    Theta = _theta(pp, 100 + pp)
    W = np.random.default_rng(200 + pp).standard_normal((len(c["x"]), QMAX))
    c.update(C=Cc, Theta=Theta, W=W, mean=J.ref_mean(ref, terms, Theta, Cc), jac=J.ref_jac(ref, terms, Theta, Cc),
             hv=D2.ref_hv(c["hvt"], Theta, Cc), jv=D2.ref_jvp(c["jvt"], Theta, Cc, d))
    return c


def run_hvp(om_d, terms, Theta, x, V, W, want=("mean", "vjp", "jvp", "hvp"), pad=0):
    """obhip_predict_hvp_multi_dev on torch buffers pre-filled with NaN -> dict of mean n x q, vjp n x d,
    jvp n x q, hvp n x d; W with ldw = n + pad, the padding NaN; outputs not in `want` are passed as NULL"""
    import torch
    import outerbase_amd as ob
    from outerbase_amd._lib import call
    t = ob.obmod._terms_of(om_d, terms)
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    (n, d), q = x.shape, Theta.shape[1]
    dx = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    dv = torch.from_numpy(np.ascontiguousarray(V.T)).to(dev)
    dw = None
    if W is not None:
        wp = np.full((q, n + pad), NAN)
        wp[:, :n] = W.T
        dw = torch.from_numpy(wp).to(dev)
    out = {"mean": torch.full((q, n), NAN, dtype=torch.float64, device=dev),
           "vjp": torch.full((d, n), NAN, dtype=torch.float64, device=dev),
           "jvp": torch.full((q, n), NAN, dtype=torch.float64, device=dev),
           "hvp": torch.full((d, n), NAN, dtype=torch.float64, device=dev)}
    a = {k: (v.data_ptr() if k in want else None) for k, v in out.items()}
    call("obhip_predict_hvp_multi_dev", om_d._h, t._h, dth.data_ptr(), q, dx.data_ptr(), n,
         None if dw is None else dw.data_ptr(), n + pad, dv.data_ptr(), a["mean"], a["vjp"], a["jvp"], a["hvp"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().T for k, v in out.items()}


def corner(c, n, q, W=None, V_sign=1.0):
    """reference values and tolerances of a call on the first n rows and q responses"""
    W = c["W"][:n, :q] if W is None else W
    jw, jt = c["jac"][0][:n, :, :q], c["jac"][1][:n, :, :q]
    hw, ht = c["hv"][0][:n, :, :q], c["hv"][1][:n, :, :q]
    hv = J.ref_vjp(hw, ht, W)
    return {"mean": (c["mean"][0][:n, :q], c["mean"][1][:n, :q]), "vjp": J.ref_vjp(jw, jt, W),
            "jvp": (V_sign * c["jv"][0][:n, :q], c["jv"][1][:n, :q]), "hvp": (V_sign * hv[0], hv[1])}


def worst_of(got, want):
    return {k: E.worst_ratio(got[k], *want[k]) for k in ("mean", "vjp", "jvp", "hvp")}


def check_hcase(c, label, ns=NS, qs=QS):
    lines, worst = [], {"mean": 0.0, "vjp": 0.0, "jvp": 0.0, "hvp": 0.0}
    for n in ns:
        for q in qs:
            got = run_hvp(c["om_d"], c["terms"], c["Theta"][:, :q], c["x"][:n], c["V"][:n], c["W"][:n, :q])
            w = worst_of(got, corner(c, n, q))
            if not max(w.values()) < 1:
                lines.append("%s p=%d n=%d q=%d: err/tolerance %s" % (label, len(c["terms"]), n, q,
                             ", ".join("%s %.3g" % kv for kv in w.items())))
            worst = {k: max(worst[k], w[k]) for k in w}
    print("%s p=%d: worst err/tolerance %s" % (label, len(c["terms"]), ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert not lines, "\n".join(lines)


def _route(generic, monkeypatch):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name,p,kind", HCASES)
def test_against_extended_reference(name, p, kind, generic, monkeypatch):
    """d1, d4 of mixed kinds (p = 1: the constant term alone), d11 with a dimension no term uses and
    with terms of 9-11 factors, the knot loop of 130 knots; rows on knots and at x = 0.02"""
    _route(generic, monkeypatch)
    ns = NS if kind == "select" and name != "d4 knots130" else (33, 129)
    check_hcase(hcase(name, p, kind), "%s %s" % ("fallback" if generic else "fused", name), ns=ns)


@pytest.mark.parametrize("generic", [False, True])
def test_sixty_five_responses(generic, monkeypatch):
    """two full chunks and one response: the sums over the responses continue across the launches"""
    _route(generic, monkeypatch)
    check_hcase(hcase("d4", 65), "q=65 generic=%s" % generic, ns=(65,), qs=(65,))


def test_term_set_beyond_the_fused_domain(monkeypatch):
    """d = 40 with 198 used columns: the tile does not fit the LDS, the pooled HBM tile takes the call
    with and without the switch"""
    from outerbase_amd._lib import call
    import outerbase_amd as ob
    c = hcase("wide", 0)
    fused = C.c_int(-1)
    t = ob.obmod._terms_of(c["om_d"], c["terms"])         # (held: the handle lives as long as the object)
    call("obhip_predict_hvp_layout", t._h, 1, None, None, None, C.byref(fused))
    assert fused.value == 0
    monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    check_hcase(c, "wide generic", ns=(65,), qs=(1, 17))
    monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)
    check_hcase(c, "wide", ns=(65,), qs=(1, 17))


@pytest.mark.parametrize("generic", [False, True])
def test_two_calls_give_identical_bits_and_optional_outputs_do_not_change_them(generic, monkeypatch):
    """each output's bits with and without the other optional outputs; the padding of W (NaN) is not
    read; outputs that are not asked for keep their sentinels"""
    _route(generic, monkeypatch)
    c = hcase("d11", 300)
    n, q = 65, 33
    a = (c["om_d"], c["terms"], c["Theta"][:, :q], c["x"][:n], c["V"][:n], c["W"][:n, :q])
    full, again = run_hvp(*a), run_hvp(*a)
    assert all(np.all(np.isfinite(v)) for v in full.values())
    assert all(np.array_equal(full[k], again[k]) for k in full)
    for want in (("hvp",), ("jvp",), ("hvp", "jvp"), ("vjp", "jvp"), ("mean", "hvp")):
        part = run_hvp(*a, want=want)
        for k in full:
            if k in want:
                assert np.array_equal(part[k], full[k]), (want, k)
            else:
                assert np.all(np.isnan(part[k])), (want, k)
    nojw = run_hvp(*a[:5], None, want=("mean", "jvp"))                       # no W: the JVP alone
    assert np.array_equal(nojw["jvp"], full["jvp"]) and np.array_equal(nojw["mean"], full["mean"])
    padded = run_hvp(*a, pad=3)
    assert all(np.array_equal(full[k], padded[k]) for k in full)


@pytest.mark.parametrize("generic", [False, True])
def test_a_nan_coordinate_gives_nan_in_that_row_only(generic, monkeypatch):
    _route(generic, monkeypatch)
    c = hcase("d4", 65)
    n, q = 65, 17
    x = c["x"][:n].copy()
    x[40, 2] = NAN
    got = run_hvp(c["om_d"], c["terms"], c["Theta"][:, :q], x, c["V"][:n], c["W"][:n, :q])
    clean = run_hvp(c["om_d"], c["terms"], c["Theta"][:, :q], c["x"][:n], c["V"][:n], c["W"][:n, :q])
    keep = np.arange(n) != 40
    for k in got:
        assert np.all(np.isnan(got[k][40])), k
        assert np.array_equal(got[k][keep], clean[k][keep]), k


def test_sign_of_the_direction(monkeypatch):
    """hvp(W, -V) and jvp(-V) are the negatives of hvp(W, V) and jvp(V) within tolerance; zero rows of V
    give exact zeros"""
    _route(False, monkeypatch)
    c = hcase("d11", 300)
    n, q = 129, 17
    a = (c["om_d"], c["terms"], c["Theta"][:, :q], c["x"][:n])
    pos = run_hvp(*a, c["V"][:n], c["W"][:n, :q])
    neg = run_hvp(*a, -c["V"][:n], c["W"][:n, :q])
    w = worst_of(neg, corner(c, n, q, V_sign=-1.0))
    print("direction -V: err/tolerance %s" % ", ".join("%s %.3g" % kv for kv in w.items()))
    assert max(w.values()) < 1
    want = corner(c, n, q)
    for k in ("jvp", "hvp"):
        assert E.worst_ratio(-neg[k], pos[k], 2 * want[k][1]) < 1
    zero = ~np.any(c["V"][:n], axis=1)
    assert zero.sum() >= 3 and not np.any(pos["hvp"][zero]) and not np.any(pos["jvp"][zero])


@pytest.mark.parametrize("generic", [False, True])
def test_hessian_from_unit_directions_is_symmetric(generic, monkeypatch):
    _route(generic, monkeypatch)
    m, cs = model("d4"), hcase("d4", 65)
    n, q, d = 33, 3, 4
    x, terms, Theta, W, ref = m["x"][:n], cs["terms"], cs["Theta"][:, :q], cs["W"][:n, :q], D2.reference_d2_of(m["om_o"], m["x"][:n])
    H, T = np.empty((n, d, d)), np.empty((n, d, d))
    worst = 0.0
    for k in range(d):
        V = np.zeros((n, d))
        V[:, k] = 1.0
        want, tol = D2.ref_hvp(ref.hv_terms(terms, V), Theta, W, cs["C"])
        H[:, :, k] = run_hvp(m["om_d"], terms, Theta, x, V, W, want=("hvp",))["hvp"]
        T[:, :, k] = tol
        worst = max(worst, E.worst_ratio(H[:, :, k], want, tol))
    sym = E.worst_ratio(H, H.transpose(0, 2, 1), T + T.transpose(0, 2, 1))
    print("Hessian from unit directions: err/tolerance %.3g, asymmetry / (sum of the two tolerances) %.3g" % (worst, sym))
    assert worst < 1 and sym < 1


@pytest.mark.parametrize("generic", [False, True])
def test_mean_and_vjp_agree_with_the_vjp_entry(generic, monkeypatch):
    _route(generic, monkeypatch)
    from test_gpu_predict_jac import run_vjp
    c = hcase("d11", 300)
    n, q = 129, 33
    a = (c["om_d"], c["terms"], c["Theta"][:, :q], c["x"][:n])
    got = run_hvp(*a, c["V"][:n], c["W"][:n, :q])
    mean, out = run_vjp(*a, c["W"][:n, :q])
    want = corner(c, n, q)
    assert E.worst_ratio(got["mean"], mean, 2 * want["mean"][1]) < 1
    assert E.worst_ratio(got["vjp"], out, 2 * want["vjp"][1]) < 1


def test_python_entries(monkeypatch):
    _route(False, monkeypatch)
    import outerbase_amd as ob
    c = hcase("d4", 65)
    n, q = 33, 17
    Theta, x, V, W = c["Theta"][:, :q], c["x"][:n], c["V"][:n], c["W"][:n, :q]
    dev = run_hvp(c["om_d"], c["terms"], Theta, x, V, W)
    hvp, jvp = ob.predict_hvp(c["om_d"], c["terms"], Theta, x, V, W)
    assert hvp.shape == (n, 4) and jvp.shape == (n, q)
    assert np.array_equal(hvp, dev["hvp"]) and np.array_equal(jvp, dev["jvp"])
    none, jvp2 = ob.predict_hvp(c["om_d"], c["terms"], Theta, x, V)
    assert none is None and np.array_equal(jvp2, jvp)
    h0, j0 = ob.predict_hvp(c["om_d"], c["terms"], Theta, x[:0], V[:0], W[:0])
    assert h0.shape == (0, 4) and j0.shape == (0, q)
    hess = ob.predict_hess(c["om_d"], c["terms"], Theta[:, 1], x[:5])
    assert hess.shape == (5, 4, 4)
    for k in range(4):
        Vk = np.zeros((5, 4))
        Vk[:, k] = 1.0
        assert np.array_equal(hess[:, :, k], run_hvp(c["om_d"], c["terms"], Theta[:, 1:2], x[:5], Vk, np.ones((5, 1)),
                                                     want=("hvp",))["hvp"])
    with pytest.raises(ValueError):
        ob.predict_hvp(c["om_d"], c["terms"], Theta, x, V[:, :3], W)
    with pytest.raises(ValueError):
        ob.predict_hvp(c["om_d"], c["terms"], Theta, x, V, W[:, :3])


# ---- what is built on the entry --------------------------------------------------------------------
def test_multifit_hvp_and_predict_hess(monkeypatch):
    _route(False, monkeypatch)
    from test_gpu_predict_jac import fitted
    m, c = model("d4"), hcase("d4", 65)
    q, n, d = 3, 33, 4
    mf = fitted(q)
    x, V, ref, Cc = m["x"][:n], c["V"][:n], D2.reference_d2_of(m["om_o"], m["x"][:n]), c["C"]
    cot = np.random.default_rng(12).standard_normal((n, q))
    W = cot * mf.y_sca[None, :]                    # what the device is handed, formed in the same arithmetic
    hv, jv = mf.hvp(x, cot, V)
    assert hv.shape == (n, d) and jv.shape == (n, q)
    worst = {"hvp": E.worst_ratio(hv, *D2.ref_hvp(ref.hv_terms(c["terms"], V), mf.coeff, W, Cc))}
    jw, jt = D2.ref_jvp(ref.jv_terms(c["terms"], V), mf.coeff, Cc, d)
    worst["jvp"] = max(E.worst_ratio(jv[:, j], *_destandardised(jw[:, j], jt[:, j], float(mf.y_sca[j]))) for j in range(q))
    hess = mf.predict_hess(x[:5], response=1)
    assert hess.shape == (5, d, d)
    ref5 = D2.reference_d2_of(m["om_o"], m["x"][:5])
    e1 = np.zeros((5, q))
    e1[:, 1] = mf.y_sca[1]
    worst["hess"] = 0.0
    for k in range(d):
        Vk = np.zeros((5, d))
        Vk[:, k] = 1.0
        worst["hess"] = max(worst["hess"], E.worst_ratio(hess[:, :, k], *D2.ref_hvp(ref5.hv_terms(c["terms"], Vk), mf.coeff, e1, Cc)))
    print("MultiFit q=3: err/tolerance %s" % ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) < 1


@pytest.mark.parametrize("q", [1, 3])
def test_torch_double_backward(q, monkeypatch):
    _route(False, monkeypatch)
    import torch
    from test_gpu_predict_jac import _interior_x, fitted
    m, c = model("d4"), hcase("d4", 65)
    mf = fitted(q)
    emu = mf.torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(50 + q)
    n, d = 5, 4
    xs, cs, U = _interior_x(rng, n, m["knots"]), rng.standard_normal((n, q)), rng.standard_normal((n, d))
    x = torch.from_numpy(xs).to(dev).requires_grad_(True)
    cw = torch.from_numpy(cs).to(dev).requires_grad_(True)
    y = emu(x)
    g, = torch.autograd.grad((y * cw).sum(), x, create_graph=True)
    gx, gc = torch.autograd.grad((g * torch.from_numpy(U).to(dev)).sum(), (x, cw), create_graph=True)
    # forward and first backward carry the bits of a run without create_graph
    x2 = torch.from_numpy(xs).to(dev).requires_grad_(True)
    y2 = emu(x2)
    (y2 * cw.detach()).sum().backward()
    assert torch.equal(y, y2) and torch.equal(g, x2.grad)
    assert np.array_equal(x2.grad.cpu().numpy(), mf.vjp(xs, cs))
    # the second derivatives against the reference
    ref, Cc = D2.reference_d2_of(m["om_o"], xs), c["C"]
    W = cs * mf.y_sca[None, :]
    worst = {"d/dx": E.worst_ratio(gx.detach().cpu().numpy(), *D2.ref_hvp(ref.hv_terms(c["terms"], U), mf.coeff, W, Cc))}
    jw, jt = D2.ref_jvp(ref.jv_terms(c["terms"], U), mf.coeff, Cc, d)
    gcn = gc.detach().cpu().numpy()
    worst["d/dc"] = max(E.worst_ratio(gcn[:, j], *_destandardised(jw[:, j], jt[:, j], float(mf.y_sca[j]))) for j in range(q))
    print("torch double backward q=%d: err/tolerance %s" % (q, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) < 1
    # a third derivative is refused in words
    with pytest.raises(RuntimeError, match="third derivative"):
        torch.autograd.grad(gx.sum(), x)
