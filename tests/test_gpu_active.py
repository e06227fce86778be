"""E[grad f grad f^T], E[grad f] and the active subspace on the GPU (obhip_dim_grad_moments_dev, obhip_active_dev
and what is built on them) against the long-double reference of tests/active_ref.py.

Stage 1 (tables): every entry of dm, X and D within Cc . bound + gamma . sum |summands|.  Stage 2 (sums on random
CONSISTENT float64 tables): every gbar and entry of C within its own gamma . sum |summands|.  End to end: device
tables, then device sums, against long-double sums of long-double tables; allowance eight times the float64
restatement's own error on the same case.  Every test prints err / tolerance.

TW = 128 is the pair kernel's term-tile width, RC = 2 its response chunk, T = 5 the dimensions per block of its
output triangle (d = 5 | 6 and 10 | 11 add a block), 8 and 24 the dimensions whose row offsets it keeps in registers
(d = 8 | 9, 24 | 25; d = 40 takes the others from memory).  The table kernel takes 256 threads up to 16 levels and 64
beyond, level tiles of 8 (9 and 17 levels: one more tile)."""
import ctypes as C
import functools

import numpy as np
import pytest

import active_ref as A
import extended_dx_ref as X
import extended_jac_ref as J
import extended_ref as E
import sobol_ref as S
from conftest import knots_for, make_pair, sample_x
from test_active_host import ACTIVE_CASES, active_tables
from test_gpu_sobol import NS, moment_model
from test_sobol_host import golden_model, reference_of, some_zero_weights, theta_of

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 7
ld = np.longdouble


def _dev():
    import torch
    from outerbase_amd._lib import call
    dev = torch.device("cuda", torch.cuda.current_device())
    call("obhip_set_stream", C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return torch, call, dev


# ---- stage 1: the gradient tables ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_model(name):
    """moment_model's cases and `levels17`: two mat25 dimensions whose terms reach 9 and 17 levels (level tiles of 8:
    two and three tiles; 17 levels: the 64-thread blocks)"""
    if name != "levels17":
        return moment_model(name)
    kinds = ["mat25", "mat25"]
    om_o, om_d = make_pair(kinds, knots_for(kinds, 20))
    terms = np.array([[0, 0], [1, 0], [0, 1], [8, 1], [1, 16], [3, 5], [7, 15], [8, 16], [2, 9], [5, 0]], dtype=np.int64)
    rng = np.random.default_rng(17)
    x = sample_x(rng, max(NS), kinds)
    return dict(kinds=kinds, om_o=om_o, om_d=om_d, terms=terms, x=x, w=some_zero_weights(rng, max(NS), 2),
                levels=S.levels_of(terms))


def run_grad_moments(om_d, terms, x, w=None, pad=0, wpad=0):
    """obhip_dim_grad_moments_dev on NaN-padded torch buffers -> (packed dmean, cross, dd, padding untouched)"""
    import outerbase_amd as ob
    torch, call, dev = _dev()
    t = ob.obmod._terms_of(om_d, terms)
    n, d = x.shape
    xp = np.full((d, n + pad), NAN)
    xp[:, :n] = x.T
    dx = torch.from_numpy(xp).to(dev)
    dw = None
    if w is not None:
        wp = np.full((d, n + wpad), NAN)
        wp[:, :n] = w.T
        dw = torch.from_numpy(wp).to(dev)
    levels = S.levels_of(terms)
    nm, nc = int(levels.sum()), int((levels ** 2).sum())
    bufs = [torch.full((k + PAD,), NAN, dtype=torch.float64, device=dev) for k in (nm, nc, nc)]
    call("obhip_dim_grad_moments_dev", om_d._h, t._h, dx.data_ptr(), n, n + pad, None if dw is None else dw.data_ptr(),
         n + wpad, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr())
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    clean = all(bool(np.all(np.isnan(h[k:]))) for h, k in zip(host, (nm, nc, nc)))
    return host[0][:nm], host[1][:nc], host[2][:nc], clean


@pytest.mark.parametrize("name", ["mixed_d3", "mat25_d8", "knots130", "levels17"])
def test_gradient_tables_against_extended_reference(name):
    c = grad_model(name)
    levels, d = c["levels"], len(c["levels"])
    lines, worst = [], 0.0
    for n in NS:
        x = c["x"][:n]
        raw = A.raw_dx(c["om_o"], x)
        Cc = E.constant_from_oracle_ratio(A.f64_raw_ratio(c["om_o"], x, levels, raw))
        for mode in ("none", "weights", "padded weights"):
            w = None if mode == "none" else c["w"][:n]
            got = run_grad_moments(c["om_d"], c["terms"], x, w, pad=3, wpad=5 if mode == "padded weights" else 0)
            got2 = run_grad_moments(c["om_d"], c["terms"], x, w)
            same = all(np.array_equal(a, b) for a, b in zip(got[:3], got2[:3]))  # two calls, other padding
            gdm, gX, gD = A.unpack_grad_tables(*got[:3], levels)
            (dm, Xc, Dd), (tdm, tX, tD) = A.ref_grad_tables(raw, levels, w, Cc)
            r = max(max(E.worst_ratio(gdm[l], dm[l], tdm[l]), E.worst_ratio(gX[l], Xc[l], tX[l]),
                        E.worst_ratio(gD[l], Dd[l], tD[l])) for l in range(d))
            sym = all(np.array_equal(a, a.T) for a in gD)
            worst = max(worst, r)
            if not (r < 1 and same and sym and got[3] and got2[3]):
                lines.append("%s n=%d %s: err/tolerance %.3g, same bits %s, D symmetric %s, padding clean %s" % (
                    name, n, mode, r, same, sym, got[3] and got2[3]))
    print("%s: worst err/tolerance %.3g" % (name, worst))
    assert not lines, "\n".join(lines)


def test_bad_weights_are_a_numeric_error():
    from outerbase_amd import ObhipError
    c = grad_model("mixed_d3")
    n = 65
    for what in ("zero column", "negative", "nan", "inf"):
        w = c["w"][:n].copy()
        if what == "zero column":
            w[:, 1] = 0.0
        else:
            w[40, 2] = {"negative": -0.5, "nan": NAN, "inf": float("inf")}[what]
        with pytest.raises(ObhipError) as e:
            run_grad_moments(c["om_d"], c["terms"], c["x"][:n], w)
        assert e.value.code == 5, what                                           # OBHIP_ERR_NUMERIC
    assert run_grad_moments(c["om_d"], c["terms"], c["x"][:n], c["w"][:n])[3]    # and the library goes on


# ---- stage 2: the sums on random consistent tables -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def active_case(p, d, q):
    import outerbase_amd as ob
    c = active_tables(p, d, q)
    kinds = ["mat25"] * d
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    ob.setknot(om, knots_for(kinds, 20))
    return dict(c, om=om, t=ob.obmod._Terms(om, c["terms"]))


def run_active(t, Theta, m, Cv, dm, Xc, Dd):
    """obhip_active_dev on NaN-filled buffers with PAD doubles behind the output -> (out, padding untouched)"""
    torch, call, dev = _dev()
    q, d = Theta.shape[1], t.d
    nout, wsb = C.c_uint64(0), C.c_uint64(0)
    call("obhip_active_layout", t._h, None, None, C.byref(nout))
    call("obhip_active_workspace_bytes", t.p, d, q, C.byref(wsb))
    nout = nout.value
    assert nout == d + d * (d + 1) // 2
    ws = torch.full((wsb.value // 8,), NAN, dtype=torch.float64, device=dev)
    dth = torch.from_numpy(np.ascontiguousarray(Theta.T)).to(dev)
    tabs = [torch.from_numpy(a).to(dev) for a in S.pack_tables(m, Cv) + A.pack_grad_tables(dm, Xc, Dd)]
    out = torch.full((q * nout + PAD,), NAN, dtype=torch.float64, device=dev)
    call("obhip_active_dev", t._h, dth.data_ptr(), q, *[a.data_ptr() for a in tabs], out.data_ptr(), ws.data_ptr(),
         wsb.value)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return out[:q * nout].reshape(q, nout), bool(np.all(np.isnan(out[q * nout:])))


def _tabs(c):
    return c["m"], c["Cv"], c["dm"], c["Xc"], c["Dd"]


@pytest.mark.parametrize("p,d,q", ACTIVE_CASES)
def test_pair_sums_on_random_consistent_tables(p, d, q):
    c = active_case(p, d, q)
    want, tol = A.pack_out(c["fa"])
    out, clean = run_active(c["t"], c["Theta"], *_tabs(c))
    out2, clean2 = run_active(c["t"], c["Theta"], *_tabs(c))
    assert clean and clean2                                                      # the padding is untouched
    assert np.array_equal(out, out2)                                             # the same bits on every call
    assert out.shape == (q, d + d * (d + 1) // 2) and np.all(np.isfinite(out))
    rg = E.worst_ratio(out[:, :d], want[:, :d], tol[:, :d])
    rC = E.worst_ratio(out[:, d:], want[:, d:], tol[:, d:])
    print("p=%d d=%d q=%d: err/tolerance gbar %.3g, C %.3g" % (p, d, q, rg, rC))
    assert rg < 1 and rC < 1


def test_sobol_and_sobol2_return_the_same_bits_around_the_new_entries():
    from test_gpu_sobol import run_sobol
    from test_gpu_sobol2 import run_sobol2
    c = active_case(300, 20, 5)
    pm, pc = S.pack_tables(c["m"], c["Cv"])
    before, g_before = run_sobol(c["t"], c["Theta"], pm, pc)
    before2, G_before, _ = run_sobol2(c["t"], c["Theta"], pm, pc)
    run_active(c["t"], c["Theta"], *_tabs(c))
    g = grad_model("mixed_d3")
    run_grad_moments(g["om_d"], g["terms"], g["x"][:65], g["w"][:65])
    after, g_after = run_sobol(c["t"], c["Theta"], pm, pc)
    after2, G_after, _ = run_sobol2(c["t"], c["Theta"], pm, pc)
    assert np.array_equal(before, after) and np.array_equal(g_before, g_after)
    assert np.array_equal(before2, after2) and np.array_equal(G_before, G_after)


# ---- end to end ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2e_active(name):
    import ob_oracle as O
    mdl = golden_model(name)
    kinds, terms, om_o = mdl["kinds"], mdl["terms"], mdl["om_o"]
    d = len(kinds)
    rng = np.random.default_rng(7 + d)
    n = 200
    nodes, w = sample_x(rng, n, kinds), some_zero_weights(rng, n, d)
    Theta = theta_of(terms, 5, 11 + d)
    levels = S.levels_of(terms)
    raw = A.raw_dx(om_o, nodes)
    m, Cv = S.tables_from_bases([r[0] for r in raw], levels, w)
    g = A.grad_tables_from_bases([r[0] for r in raw], [r[2] for r in raw], levels, w)
    b = O.OuterBase(om_o, nodes)
    r64 = A.raw_dx(om_o, nodes, dtype=np.float64)
    m64, C64 = S.tables_from_bases([b.getbase(l + 1) for l in range(d)], levels, w, dtype=np.float64)
    g64 = A.grad_tables_from_bases([b.getbase(l + 1) for l in range(d)], [r[2] for r in r64], levels, w, dtype=np.float64)
    return dict(mdl=mdl, nodes=nodes, w=w, Theta=Theta, levels=levels, fa=A.formulas_active(terms, Theta, m, Cv, *g),
                fa64=A.formulas_active(terms, Theta, m64, C64, *g64, dtype=np.float64))


@pytest.mark.parametrize("name", ["mixed_d3", "mat25_d8"])
def test_active_subspace_end_to_end(name):
    """per entry the scale is the stage-2 tolerance (gamma . sum |summands|); the float64 restatement's worst
    err / scale is measured here, and the device is allowed eight times that"""
    import outerbase_amd as ob
    c = e2e_active(name)
    mdl, f, f64 = c["mdl"], c["fa"], c["fa64"]
    d, q = len(c["levels"]), c["Theta"].shape[1]
    gm = ob.input_grad_moments(mdl["om_d"], mdl["terms"], c["nodes"], c["w"])
    res = ob.active_subspace(mdl["om_d"], mdl["terms"], c["Theta"], gm)
    got = dict(gbar=res.mean_grad, C=res.C)
    r64 = max(E.worst_ratio(f64[k], f[k], f["tol_" + k]) for k in got)
    rdev = max(E.worst_ratio(got[k], f[k], f["tol_" + k]) for k in got)
    print("%s end to end: float64 restatement %.3g, device %.3g of the scale; device / restatement %.3g" % (
        name, r64, rdev, rdev / r64))
    assert rdev <= 8 * r64
    assert res.C.shape == (d, d, q) and np.array_equal(res.C, res.C.transpose(1, 0, 2))
    assert np.array_equal(res.dgsm, res.C[np.arange(d), np.arange(d)]) and np.all(res.dgsm > 0)
    for r in range(q):
        Cr, lam, W = res.C[:, :, r], res.eigenvalues[:, r], res.eigenvectors[:, :, r]
        nrm = np.linalg.norm(Cr)
        assert np.linalg.norm(Cr @ W - W * lam[None, :]) <= 10 * d * 2.0 ** -52 * nrm
        assert np.all(np.diff(lam) <= 0) and lam[-1] >= -10 * d * 2.0 ** -52 * nrm
    sc = res.activity_scores(2)
    assert sc.shape == (d, q) and np.all(sc >= 0)
    assert np.allclose(res.activity_scores(d), res.dgsm, rtol=1e-9)            # sum_j lambda_j W_lj^2 = C_ll
    y = res.project(c["nodes"][:9], 2, response=1)
    assert y.shape == (9, 2) and np.array_equal(y, c["nodes"][:9] @ res.eigenvectors[:, :2, 1])
    # the scale: diag(s) C diag(s) before the eigen step, C itself as it was; the mean tables serve sobol too
    s = np.linspace(0.5, 2.0, d)
    res_s = ob.active_subspace(mdl["om_d"], mdl["terms"], c["Theta"], gm, scale=s)
    assert np.array_equal(res_s.C, res.C)
    lam_s = np.linalg.eigvalsh(res.C[:, :, 0] * s[:, None] * s[None, :])[::-1]
    assert np.allclose(res_s.eigenvalues[:, 0], lam_s, rtol=1e-9, atol=1e-12 * lam_s[0])
    assert np.array_equal(ob.sobol(mdl["om_d"], mdl["terms"], c["Theta"], gm).var,
                          ob.sobol(mdl["om_d"], mdl["terms"], c["Theta"], gm.moments).var)


def test_against_the_jacobian_kernel_on_a_grid():
    """mixed_d3 with 6 x 5 x 4 nodes (the shorter columns by zero weights): C of the closed form and sum w J J^T of
    predict_jac on the 120 grid rows, each held to the long-double brute force with its own tolerance -- the closed
    form to eight times the float64 restatement's error in units of the stage-2 scale, the Jacobian route to the
    tolerance of J (extended_jac_ref) carried through the products, the sum taken in long double.  Their mutual
    distance is printed."""
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    kinds, terms, om_o, om_d = mdl["kinds"], mdl["terms"], mdl["om_o"], mdl["om_d"]
    rng = np.random.default_rng(654)
    nodes = sample_x(rng, 6, kinds)
    w = rng.uniform(0.5, 1.5, (6, 3))
    w[5:, 1] = 0.0
    w[4:, 2] = 0.0
    Theta = theta_of(terms, 3, 21)
    levels = S.levels_of(terms)
    rows, idx = S.grid_rows(nodes)
    wn = S.normalised_weights(w, 6, 3)
    Wrow = np.prod(wn[idx, np.arange(3)[None, :]], axis=1)
    keep = E._f64(Wrow) > 0
    assert keep.sum() == 120
    rows, idx_k, Wk = rows[keep], idx[keep], Wrow[keep]
    gref = X.reference_dx_of(om_o, rows)
    Cj = E.constant_from_oracle_ratio(X.f64_ratio(gref, om_o, rows, terms))
    Jl, tJ = J.ref_jac(gref, terms, Theta, Cj)                                  # 120 x d x q
    brute = np.einsum("i,ilj,imj->lmj", Wk, Jl, Jl)
    aJ = np.abs(E._f64(Jl))
    tol_jac = np.einsum("i,ilj,imj->lmj", E._f64(Wk), tJ, aJ) + np.einsum("i,ilj,imj->lmj", E._f64(Wk), aJ, tJ) \
        + np.einsum("i,ilj,imj->lmj", E._f64(Wk), tJ, tJ)
    _, jac = ob.predict_jac(om_d, terms, Theta, rows)
    Cjac = np.einsum("i,ilj,imj->lmj", Wk, np.asarray(jac, dtype=ld), np.asarray(jac, dtype=ld))
    r_jac = E.worst_ratio(E._f64(Cjac), brute, tol_jac)
    # the closed form: the scale is the stage-2 tolerance on the long-double tables of the same measure
    raw = A.raw_dx(om_o, nodes)
    m, Cv = S.tables_from_bases([r[0] for r in raw], levels, w)
    g = A.grad_tables_from_bases([r[0] for r in raw], [r[2] for r in raw], levels, w)
    f = A.formulas_active(terms, Theta, m, Cv, *g)
    import ob_oracle as O
    b = O.OuterBase(om_o, nodes)
    r64 = A.raw_dx(om_o, nodes, dtype=np.float64)
    m64, C64 = S.tables_from_bases([b.getbase(l + 1) for l in range(3)], levels, w, dtype=np.float64)
    g64 = A.grad_tables_from_bases([b.getbase(l + 1) for l in range(3)], [r[2] for r in r64], levels, w, dtype=np.float64)
    f64 = A.formulas_active(terms, Theta, m64, C64, *g64, dtype=np.float64)
    res = ob.active_subspace(om_d, terms, Theta, ob.input_grad_moments(om_d, terms, nodes, w))
    r_form = E.worst_ratio(E._f64(f["C"]), brute, f["tol_C"])                    # the two long-double routes
    r64c = E.worst_ratio(f64["C"], brute, f["tol_C"])
    r_dev = E.worst_ratio(res.C, brute, f["tol_C"])
    mutual = float(np.max(np.abs(res.C - E._f64(Cjac)) / np.abs(E._f64(brute))))
    print("closed form vs brute force: long double %.3g, float64 restatement %.3g, device %.3g of the stage-2 scale; "
          "Jacobian route err/tolerance %.3g; closed form vs Jacobian route, relative %.3g" % (
              r_form, r64c, r_dev, r_jac, mutual))
    assert r_form < 1e-2
    assert r_dev <= 8 * max(r64c, r_form)
    assert r_jac < 1


# ---- the Python layer ------------------------------------------------------------------------------------------
def test_multifit_active_subspace_is_the_module_function_in_raw_units():
    import outerbase_amd as ob
    c = e2e_active("mixed_d3")
    mdl, q = c["mdl"], c["Theta"].shape[1]
    rng = np.random.default_rng(5)
    meansd = np.stack([rng.standard_normal(q), rng.uniform(0.5, 3.0, q), np.ones(q)], axis=1)
    t = ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    mf = ob.MultiFit(mdl["om_d"], t, c["Theta"], meansd, np.ones(len(mdl["terms"])), 0.0, 6.0)
    s = np.array([0.5, 1.0, 2.0])
    res = mf.active_subspace(c["nodes"], c["w"], scale=s)
    gm = ob.input_grad_moments(mdl["om_d"], t, c["nodes"], c["w"])
    base = ob.active_subspace(mdl["om_d"], t, c["Theta"], gm, scale=s)
    s1, s2 = meansd[:, 1], meansd[:, 1] * meansd[:, 1]
    assert np.array_equal(res.C, base.C * s2[None, None, :]) and np.array_equal(res.dgsm, base.dgsm * s2[None, :])
    assert np.array_equal(res.mean_grad, base.mean_grad * s1[None, :])
    assert np.array_equal(res.eigenvalues, base.eigenvalues * s2[None, :])
    assert np.array_equal(res.eigenvectors, base.eigenvectors)


def test_zero_coefficients_give_a_zero_matrix_and_finite_eigenvectors():
    import outerbase_amd as ob
    c = e2e_active("mixed_d3")
    mdl = c["mdl"]
    gm = ob.input_grad_moments(mdl["om_d"], mdl["terms"], c["nodes"])
    res = ob.active_subspace(mdl["om_d"], mdl["terms"], np.zeros((len(mdl["terms"]), 3)), gm)
    assert res.C.shape == (3, 3, 3) and np.all(res.C == 0) and np.all(res.mean_grad == 0) and np.all(res.dgsm == 0)
    assert np.all(res.eigenvalues == 0) and np.all(np.isfinite(res.eigenvectors))
    for r in range(3):
        assert np.array_equal(res.eigenvectors[:, :, r].T @ res.eigenvectors[:, :, r], np.eye(3))


def test_one_dimension():
    """d = 1 is valid: one gbar and one C_00 = sum theta theta' D[t,t']"""
    import outerbase_amd as ob
    kinds = ["mat25"]
    om_o, om_d = make_pair(kinds, knots_for(kinds, 20))
    terms = np.arange(6, dtype=np.int64)[:, None]
    rng = np.random.default_rng(1)
    nodes, Theta = sample_x(rng, 50, kinds), rng.standard_normal((6, 2))
    raw = A.raw_dx(om_o, nodes)
    levels = S.levels_of(terms)
    m, Cv = S.tables_from_bases([raw[0][0]], levels, None)
    g = A.grad_tables_from_bases([raw[0][0]], [raw[0][2]], levels, None)
    f = A.formulas_active(terms, Theta, m, Cv, *g)
    res = ob.active_subspace(om_d, terms, Theta, ob.input_grad_moments(om_d, terms, nodes))
    assert res.C.shape == (1, 1, 2) and np.array_equal(res.eigenvalues[0], res.C[0, 0]) and np.all(res.eigenvectors == 1)
    rel = max(float(np.max(np.abs(res.C - E._f64(f["C"])) / np.abs(E._f64(f["C"])))),
              float(np.max(np.abs(res.mean_grad - E._f64(f["gbar"])) / f["abs_gbar"])))
    print("d = 1: relative error %.3g" % rel)
    assert rel < 1e-9


def test_ridge_function():
    """Theta fitted to g(a^T x) on mixed_d3: grad f is along a everywhere, C is nearly of rank one.  The angle of the
    leading eigenvector to a is printed; the assertion is that the first eigenvalue exceeds the second by the factor
    the long-double reference itself shows, less 1 %."""
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    kinds, terms, om_o, om_d = mdl["kinds"], mdl["terms"], mdl["om_o"], mdl["om_d"]
    rng = np.random.default_rng(99)
    a = np.array([0.75, -0.6, 0.08])
    a /= np.linalg.norm(a)
    xs = sample_x(rng, 400, kinds)
    B = E._f64(reference_of(om_o, xs).getmat(terms)[0])
    y = np.tanh(xs @ a - np.mean(xs @ a))
    p = len(terms)
    theta = np.linalg.lstsq(np.vstack([B, 1e-4 * np.eye(p)]), np.concatenate([y, np.zeros(p)]), rcond=None)[0]
    nodes = xs[:64]
    raw = A.raw_dx(om_o, nodes)
    levels = S.levels_of(terms)
    m, Cv = S.tables_from_bases([r[0] for r in raw], levels, None)
    g = A.grad_tables_from_bases([r[0] for r in raw], [r[2] for r in raw], levels, None)
    f = A.formulas_active(terms, theta, m, Cv, *g)
    lam_ref = np.linalg.eigvalsh(E._f64(f["C"][:, :, 0]))[::-1]
    res = ob.active_subspace(om_d, terms, theta, ob.input_grad_moments(om_d, terms, nodes))
    lam, w1 = res.eigenvalues[:, 0], res.eigenvectors[:, 0, 0]
    angle = float(np.degrees(np.arccos(min(1.0, abs(w1 @ a)))))
    print("ridge: eigenvalues %s (reference %s), gap %.3g (reference %.3g), angle of the leading eigenvector to a: "
          "%.3g degrees" % (lam, lam_ref, lam[0] / lam[1], lam_ref[0] / lam_ref[1], angle))
    assert lam_ref[0] / lam_ref[1] > 10                                         # a ridge, to begin with
    assert lam[0] / lam[1] >= 0.99 * lam_ref[0] / lam_ref[1]
