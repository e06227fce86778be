"""Host-side checks of the active-subspace quantities (no GPU): the closed form of tests/active_ref.py against a
brute-force sum of grad f grad f^T over the full tensor grid of nodes, the float64 restatement inside every tolerance,
C positive semi-definite, five mutations the instrument must fail, no tested value a pure cancellation, and the
library's host side -- symbols, the eigen-solver, Python names, argument errors before any device call."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import active_ref as A
import extended_dx_ref as X
import extended_ref as E
import sobol_ref as S
from conftest import knots_for
from test_sobol2_host import CANCEL_MAX, DIGITS, GRID_CASES, PAIR2_CASES, pair2_tables
from test_sobol_host import golden_model, grid_case

ld = np.longdouble
NEW = {"obhip_active_layout": 4, "obhip_dim_grad_moments_dev": 10, "obhip_active_workspace_bytes": 4,
       "obhip_active_dev": 11, "obhip_dim_grad_moments": 10, "obhip_active": 9, "obhip_sym_eigh": 4}
# stage 2 on the GPU (test_gpu_active.py) and its cancellation check here: the shapes of the pair kernel of the
# second-order indices, whose tiling the new one shares (TW = 128, RC = 2, T = 5, 8 | 24 offsets in registers)
ACTIVE_CASES = PAIR2_CASES + [(130, 4, 4)]             # (q = 4: two full response chunks)
EIGH_CONST = 10.0     # residual and orthogonality of obhip_sym_eigh: EIGH_CONST . n . 2^-52 . ||A||_F


@functools.lru_cache(maxsize=None)
def active_tables(p, d, q):
    """the terms, levels and coefficients of pair2_tables with the five CONSISTENT tables of a synthetic measure"""
    c = pair2_tables(p, d, q)
    rng = np.random.default_rng(3000 * p + 10 * d + q)
    m, Cv, dm, Xc, Dd = A.consistent_tables(rng, c["levels"])
    return dict(terms=c["terms"], levels=c["levels"], Theta=c["Theta"], m=m, Cv=Cv, dm=dm, Xc=Xc, Dd=Dd,
                fa=A.formulas_active(c["terms"], c["Theta"], m, Cv, dm, Xc, Dd))


@functools.lru_cache(maxsize=None)
def grid_case_active(name):
    c = grid_case(name)
    om_o, n = c["mdl"]["om_o"], len(c["nodes"])
    raw = A.raw_dx(om_o, c["nodes"])
    dm, Xc, Dd = A.grad_tables_from_bases([r[0] for r in raw], [r[2] for r in raw], c["levels"], c["weights"])
    rows, idx = S.grid_rows(c["nodes"])
    gref = X.reference_dx_of(om_o, rows)
    return dict(c, raw=raw, dm=dm, Xc=Xc, Dd=Dd, brute_a=A.brute_active(gref, idx, n, c["terms"], c["Theta"], c["weights"]),
                fa=A.formulas_active(c["terms"], c["Theta"], c["m"], c["Cv"], dm, Xc, Dd))


def tables64(c):
    """the five long-double tables of a grid case rounded to float64, as lists per dimension"""
    m64, C64 = S.unpack_tables(*S.pack_tables(c["m"], c["Cv"]), c["levels"])
    pdm, px, pd = A.pack_grad_tables(c["dm"], c["Xc"], c["Dd"])
    dm64, X64 = S.unpack_tables(pdm, px, c["levels"])
    _, D64 = S.unpack_tables(pdm, pd, c["levels"])
    return m64, C64, dm64, X64, D64


def _inside(got, f):
    return dict(gbar=E.worst_ratio(got["gbar"], f["gbar"], f["tol_gbar"]), C=E.worst_ratio(got["C"], f["C"], f["tol_C"]))


# ---- the instrument ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRID_CASES)
def test_closed_form_agrees_with_the_brute_force_sum(name):
    """two algebraically different routes in long double: they differ by rounding only.  K = grid rows + p^2 + 3 d +
    4 summands at most on either route; the scale is the sum of both routes' absolute sums."""
    c = grid_case_active(name)
    p, d = c["terms"].shape
    f, b = c["fa"], c["brute_a"]
    K = c["rows"] + p * p + 3 * d + 4
    rC = float(np.max(np.abs(E._f64(f["C"] - b["C"])) / (2 * K * E.EPS * (f["abs_C"] + b["abs_C"]))))
    rg = float(np.max(np.abs(E._f64(f["gbar"] - b["gbar"])) / (2 * K * E.EPS * (f["abs_gbar"] + b["abs_gbar"]))))
    rel = float(np.max(np.abs(E._f64(f["C"] - b["C"])) / np.abs(E._f64(b["C"]))))
    print("%s (%d grid rows, p=%d): err / (2 K EPS abs sums): C %.3g, gbar %.3g; C relative %.3g" % (
        name, c["rows"], p, rC, rg, rel))
    assert max(rC, rg) < 1e-2                             # a small fraction of the worst-case bound
    assert np.array_equal(f["C"].shape, (d, d, c["Theta"].shape[1]))
    sym = np.abs(E._f64(f["C"] - f["C"].transpose(1, 0, 2)))
    assert np.all(sym <= 2 * K * E.EPS * f["abs_C"])      # both triangles were evaluated: symmetric to rounding


@pytest.mark.parametrize("name", GRID_CASES)
def test_float64_restatement_stays_inside_every_tolerance(name):
    c = grid_case_active(name)
    t64 = tables64(c)
    f = A.formulas_active(c["terms"], c["Theta"], *t64)
    g64 = A.formulas_active(c["terms"], c["Theta"], *t64, dtype=np.float64)
    w64 = A.formulas_active(c["terms"], c["Theta"], *t64, dtype=np.float64,
                            pair_weights=A.ordered_weights(len(c["terms"]), 16)[1])
    r, rw = _inside(g64, f), _inside(w64, f)
    print("%s: float64 err / tolerance: formulas %s, weighted %s" % (name, r, rw))
    assert max(r.values()) < 1 and max(rw.values()) < 1


@pytest.mark.parametrize("name", GRID_CASES)
def test_C_is_positive_semi_definite(name):
    """smallest eigenvalue >= -tolerance: an eigenvalue moves by at most the Frobenius norm of the perturbation
    (Weyl), here tol_C, and numpy's own eigh is allowed d eps ||C||"""
    c = grid_case_active(name)
    f = c["fa"]
    d = f["C"].shape[0]
    for r in range(f["C"].shape[2]):
        Cr = E._f64(f["C"][:, :, r])
        lam = np.linalg.eigvalsh(0.5 * (Cr + Cr.T))
        slack = np.linalg.norm(f["tol_C"][:, :, r]) + d * 2.0 ** -52 * np.linalg.norm(Cr)
        print("%s response %d: eigenvalues %.3g .. %.3g, slack %.3g" % (name, r, lam[0], lam[-1], slack))
        assert lam[0] >= -slack and lam[-1] > 0


def test_the_instrument_fails_five_mutations():
    c = grid_case_active("mixed_d3")
    terms, Theta, p = c["terms"], c["Theta"], len(c["terms"])
    t64 = tables64(c)
    f = A.formulas_active(terms, Theta, *t64)
    tile = 16
    I = np.arange(p) // tile
    assert I.max() >= 2
    iu = np.triu_indices(3, 1)

    def run(W, Th=Theta, **kw):
        return A.formulas_active(terms, Th, *t64, dtype=np.float64, pair_weights=W, **kw)

    def parts(got):
        """err / tolerance of (gbar, diagonal of C, upper triangle of C off the diagonal)"""
        r = E.ratio_map(got["C"], f["C"], f["tol_C"])
        return (E.worst_ratio(got["gbar"], f["gbar"], f["tol_gbar"]), float(np.max(r[np.arange(3), np.arange(3)])),
                float(np.max(r[iu[0], iu[1]])))
    U, W1 = A.ordered_weights(p, tile)
    assert np.all(W1 == 1.0) and np.all(U[I[:, None] > I[None, :]] == 0.0)
    assert max(parts(run(W1))) < 1
    unt = parts(run(W1, untransposed=True))               # X_m read untransposed
    W = W1.copy()
    W[np.ix_(I == 2, I == 0)] = 0.0                      # the mirror orientation of tile pair (0, 2) left out
    once = parts(run(W))
    W = W1.copy()
    W[np.ix_(I == 1, I == 1)] = 2.0                      # a diagonal tile pair counted twice (its 1/2 forgotten)
    twice = parts(run(W))
    dx = parts(run(W1, d_is_x=True))                      # D replaced by X
    print("err / tolerance (gbar, diagonal, off-diagonal): untransposed %s; mirror left out %s; diagonal tile twice %s; "
          "D replaced by X %s" % (unt, once, twice, dx))
    assert unt[0] < 1 and unt[1] < 1 and unt[2] > 1
    assert once[1] > 1 and once[2] > 1
    assert twice[1] > 1 and twice[2] > 1
    assert dx[0] < 1 and dx[1] > 1 and dx[2] < 1
    for shift in (1, -1):                                # response j read from column j +- 1
        r = parts(run(W1, np.roll(Theta, shift, axis=1)))
        print("columns shifted by %+d: %s" % (shift, r))
        assert min(r) > 1


def _cancellation(f):
    v, g = np.abs(E._f64(f["C"])), np.abs(E._f64(f["gbar"]))
    return (max(float(np.max(f["abs_C"] / v)), float(np.max(f["abs_gbar"] / g))),
            max(float(np.max(f["tol_C"] / v)), float(np.max(f["tol_gbar"] / g))))


@pytest.mark.parametrize("name", GRID_CASES)
def test_no_grid_value_is_pure_cancellation(name):
    r, t = _cancellation(grid_case_active(name)["fa"])
    print("%s: largest sum |summands| / |value| %.3g, tolerance / |value| %.3g" % (name, r, t))
    assert r < CANCEL_MAX and t < DIGITS


@pytest.mark.parametrize("p,d,q", ACTIVE_CASES)
def test_no_stage2_value_is_pure_cancellation(p, d, q):
    r, t = _cancellation(active_tables(p, d, q)["fa"])
    print("p=%d d=%d q=%d: largest sum |summands| / |value| %.3g, tolerance / |value| %.3g" % (p, d, q, r, t))
    assert r < CANCEL_MAX and t < DIGITS


def test_consistent_tables_are_the_moments_of_one_measure():
    """A_l = C_l + m_l m_l^T is the raw second moment, so [[A, X^T], [X, D]] is a Gram matrix: positive semi-definite;
    D and C are symmetric bit for bit"""
    rng = np.random.default_rng(4)
    m, Cv, dm, Xc, Dd = A.consistent_tables(rng, [1, 3, 6, 9])
    for l in range(4):
        Am = Cv[l] + np.outer(m[l], m[l])
        G = np.block([[Am, Xc[l].T], [Xc[l], Dd[l]]])
        assert np.array_equal(Dd[l], Dd[l].T) and np.array_equal(Cv[l], Cv[l].T)
        assert np.linalg.eigvalsh(0.5 * (G + G.T))[0] > -1e-14 * np.linalg.norm(G)
        assert abs(m[l][0] - 1) < 0.5


# ---- the library's host side ---------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name, nargs in NEW.items():
        assert name in protos, name
        assert len(protos[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert hasattr(testing, name), name
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive


def test_python_names():
    import outerbase_amd as ob
    for name in ("input_grad_moments", "active_subspace", "GradMoments", "ActiveSubspaceResult", "sym_eigh"):
        assert name in ob.__all__ and hasattr(ob, name)
    assert callable(ob.MultiFit.active_subspace)


def _sym(rng, n, lam=None):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n) if lam is None else np.asarray(lam, dtype=np.float64)
    M = (Q * lam[None, :]) @ Q.T
    return 0.5 * (M + M.T)


@pytest.mark.parametrize("n,repeated", [(1, False), (2, False), (5, False), (40, False), (5, True), (40, True)])
def test_sym_eigh_against_numpy(n, repeated):
    import outerbase_amd as ob
    rng = np.random.default_rng(100 * n + repeated)
    lam = None
    if repeated:
        lam = rng.standard_normal(n)
        lam[1:4] = lam[0]                                # one eigenvalue four times
    M = _sym(rng, n, lam)
    w, V = ob.sym_eigh(M)
    wn = np.linalg.eigvalsh(M)[::-1]
    nrm = np.linalg.norm(M)
    bound = EIGH_CONST * n * 2.0 ** -52 * nrm
    res, orth = np.linalg.norm(M @ V - V * w[None, :]), np.linalg.norm(V.T @ V - np.eye(n))
    print("n=%d repeated=%s: residual / bound %.3g, orthogonality / (bound / ||A||) %.3g, eigenvalues vs numpy / bound %.3g"
          % (n, repeated, res / bound, orth * nrm / bound, np.max(np.abs(w - wn)) / bound))
    assert res <= bound and orth * nrm <= bound
    assert np.all(np.abs(w - wn) <= bound)
    assert np.all(np.diff(w) <= 0)                       # descending
    for j in range(n):                                   # the sign rule: the first entry of largest magnitude is positive
        assert V[np.argmax(np.abs(V[:, j])), j] > 0
    assert np.array_equal(ob.sym_eigh(M)[1], V)


def test_sym_eigh_edges():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    w, V = ob.sym_eigh(np.zeros((3, 3)))
    assert np.all(w == 0) and np.array_equal(V.T @ V, np.eye(3)) and np.all((V == 0) | (V == 1))   # finite, unit vectors
    w, V = ob.sym_eigh(np.array([[2.0, 0.0], [0.0, 2.0]]))                 # a repeated eigenvalue: any basis, signed +
    assert np.array_equal(w, [2.0, 2.0]) and np.all(V >= 0) and np.array_equal(V.T @ V, np.eye(2))
    w, V = ob.sym_eigh(np.array([[1.0, -1.0], [-1.0, 1.0]]))              # |v_0| = |v_1|: index 0 is the positive one
    assert abs(w[0] - 2) < 1e-15 and abs(w[1]) < 1e-15 and V[0, 0] > 0 and V[1, 0] < 0 and V[0, 1] > 0
    buf = (C.c_double * 16)()
    a = C.cast(buf, C.c_void_p)
    assert lib.obhip_sym_eigh(0, a, a, a) == 1 and lib.obhip_sym_eigh(4097, a, a, a) == 1
    assert b"4096" in lib.obhip_last_error()
    assert lib.obhip_sym_eigh(2, None, a, a) == 1 and lib.obhip_sym_eigh(2, a, None, a) == 1
    assert lib.obhip_sym_eigh(2, a, a, None) == 1
    with pytest.raises(ob.ObhipError):
        ob.sym_eigh(np.array([[1.0, np.nan], [np.nan, 1.0]]))
    with pytest.raises(ValueError):
        ob.sym_eigh(np.zeros((2, 3)))


def test_argument_errors_return_before_any_device_call():
    import outerbase_amd as ob
    from outerbase_amd._lib import lib
    mdl = golden_model("mixed_d3")
    om, t = mdl["om_d"], ob.obmod._Terms(mdl["om_d"], mdl["terms"])
    buf = (C.c_double * 4096)()
    a = C.cast(buf, C.c_void_p)
    nm, nc, no, wsb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert lib.obhip_active_layout(None, C.byref(nm), C.byref(nc), C.byref(no)) == 1
    assert lib.obhip_active_layout(t._h, C.byref(nm), C.byref(nc), C.byref(no)) == 0
    L = S.levels_of(mdl["terms"])
    assert nm.value == L.sum() and nc.value == (L * L).sum() and no.value == 3 + 6
    assert lib.obhip_active_layout(t._h, None, None, None) == 0
    wsf = lib.obhip_active_workspace_bytes
    assert wsf(40, 3, 2, None) == 1 and wsf(0, 3, 2, C.byref(wsb)) == 1 and wsf(40, 0, 2, C.byref(wsb)) == 1
    assert wsf(40, 256, 2, C.byref(wsb)) == 1 and wsf(40, 3, 0, C.byref(wsb)) == 1
    assert wsf(40, 3, 65536, C.byref(wsb)) == 1 and wsf((1 << 24) + 1, 3, 2, C.byref(wsb)) == 1
    assert wsf(len(mdl["terms"]), 3, 2, C.byref(wsb)) == 0 and wsb.value > 0
    act = lib.obhip_active_dev
    args = [t._h, a, 2, a, a, a, a, a, a, a, wsb.value]
    for i in (0, 1, 3, 4, 5, 6, 7, 8, 9):                                   # every pointer in turn
        bad = list(args)
        bad[i] = None
        assert act(*bad) == 1, i
    assert act(t._h, a, 0, a, a, a, a, a, a, a, wsb.value) == 1            # q = 0
    assert act(t._h, a, 65536, a, a, a, a, a, a, a, wsb.value) == 1
    assert act(t._h, a, 2, a, a, a, a, a, a, a, wsb.value - 1) == 1        # workspace too small
    assert b"workspace" in lib.obhip_last_error()
    host = lib.obhip_active
    assert host(None, a, 2, a, a, a, a, a, a) == 1 and host(t._h, a, 0, a, a, a, a, a, a) == 1
    assert host(t._h, a, 2, a, a, a, a, a, None) == 1 and host(t._h, None, 2, a, a, a, a, a, a) == 1
    gm = lib.obhip_dim_grad_moments_dev
    gargs = [om._h, t._h, a, 4, 4, a, 4, a, a, a]
    for i in (0, 1, 2, 7, 8, 9):
        bad = list(gargs)
        bad[i] = None
        assert gm(*bad) == 1, i
    assert gm(om._h, t._h, a, 0, 4, a, 4, a, a, a) == 1                    # no nodes
    assert b"measure" in lib.obhip_last_error()
    assert gm(om._h, t._h, a, 4, 3, a, 4, a, a, a) == 1                    # ldx < n
    assert gm(om._h, t._h, a, 4, 4, a, 3, a, a, a) == 1                    # ldw < n
    assert gm(om._h, t._h, a, (1 << 40) + 1, 1 << 41, None, 0, a, a, a) == 1
    hostm = lib.obhip_dim_grad_moments
    assert hostm(om._h, t._h, None, 4, 4, None, 0, a, a, a) == 1 and hostm(om._h, t._h, a, 0, 4, None, 0, a, a, a) == 1
    one = ob.outermod()
    ob.setcovfs(one, ["mat25"])
    ob.setknot(one, knots_for(["mat25"], 20))
    t1 = ob.obmod._Terms(one, np.arange(4, dtype=np.int64)[:, None])
    assert lib.obhip_active_layout(t1._h, C.byref(nm), C.byref(nc), C.byref(no)) == 0 and no.value == 2   # d = 1 is valid
    assert gm(one._h, t._h, a, 4, 4, a, 4, a, a, a) == 1                   # terms of another model's dimension count
    # the limits of obhip_sobol2_dev: a level beyond 255, tables beyond the LDS of a workgroup
    wide = ob.outermod()
    ob.setcovfs(wide, ["mat25"] * 2)
    ob.setknot(wide, [np.linspace(0.001, 0.999, 300)] * 2)
    tw = ob.obmod._Terms(wide, np.array([[0, 0], [256, 1]], dtype=np.int64))
    assert lib.obhip_active_layout(tw._h, C.byref(nm), C.byref(nc), C.byref(no)) == 1
    assert b"255" in lib.obhip_last_error()
    assert act(tw._h, a, 2, a, a, a, a, a, a, a, 1 << 30) == 1
    big = ob.outermod()
    ob.setcovfs(big, ["mat25"] * 2)
    ob.setknot(big, [np.linspace(0.001, 0.999, 64)] * 2)
    tb = ob.obmod._Terms(big, np.array([[0, 0], [59, 59]], dtype=np.int64))
    assert lib.obhip_active_layout(tb._h, C.byref(nm), C.byref(nc), C.byref(no)) == 1
    assert b"LDS" in lib.obhip_last_error()
    assert act(tb._h, a, 2, a, a, a, a, a, a, a, 1 << 30) == 1
    assert gm(big._h, tb._h, a, 4, 4, a, 4, a, a, a) == 1


def test_shape_errors_raise_before_any_device_call():
    import outerbase_amd as ob
    mdl = golden_model("mixed_d3")
    om, terms = mdl["om_d"], mdl["terms"]
    p = len(terms)
    with pytest.raises(ValueError):
        ob.input_grad_moments(om, terms, np.zeros((5, 2)))
    with pytest.raises(ValueError):
        ob.input_grad_moments(om, terms, np.zeros((0, 3)))
    with pytest.raises(ValueError):
        ob.input_grad_moments(om, terms, np.zeros((5, 3)), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        ob.active_subspace(om, terms, np.zeros((p + 1, 2)), None)
    with pytest.raises(ValueError):
        ob.active_subspace(om, terms, np.zeros((p, 0)), None)
    for bad in (np.ones(2), np.array([1.0, 0.0, 1.0]), np.array([1.0, -1.0, 1.0]), np.array([1.0, np.nan, 1.0]),
                np.ones((3, 1))):
        with pytest.raises(ValueError):
            ob.active_subspace(om, terms, np.zeros((p, 2)), None, scale=bad)
    mf = ob.MultiFit(om, ob.obmod._Terms(om, terms), np.zeros((p, 2)), np.array([[0.0, 1.0, 1.0]] * 2), np.ones(p), 0.0, 6.0)
    with pytest.raises(ValueError):
        mf.active_subspace(np.zeros((5, 2)))
    with pytest.raises(ValueError):
        mf.active_subspace(np.full((5, 3), 0.5), scale=np.zeros(3))
