"""Host-side checks of the Newton fit on gridded data (no GPU): the long-double reference of
tests/product_fit_ref.py against the float64 oracle, the separated algebra in float64 inside the reference's
per-entry rule, a mutated algebra that a flat 1e-6 lets through and the rule does not, and the plumbing -- symbols,
Python names, Makefile, environment switches, ABI version, refusals before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import extended_ref as E
import product_fit_ref as F
import product_ref as P
from conftest import sample_x
from test_product_host import model, side_factors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "outerbase_amd", "csrc")
INVALID = 1
NEW = {"obhip_normal_acc_add_product_dev": 10, "obhip_product_side_dev": 9, "obhip_product_fit_layout": 7}
NEW_SOURCES = ("product_fit.cpp", "kernels_product_fit.hip")
# mixed d4 = mat25, mat25pow, mat25ang, mat25: every kind stands on either side in one of these
SPLITS = ([0], [1, 3], [0, 1, 2], [2])


def case(p, dims_b, na, nb, seed_shift=0):
    m, seed = model("mixed d4 p%d" % p)
    rng = np.random.default_rng(seed + 17 + seed_shift)
    x = sample_x(rng, na + nb, m["kinds"])
    xa, xb = P.split_x(x[:na], dims_b)[0], P.split_x(x[na:], dims_b)[1]
    ref = F.ProductFitRef(m, xa, xb, dims_b, seed)
    U, sa = side_factors(m, xa, P.dims_a_of(4, dims_b), 0.5)
    V, sb = side_factors(m, xb, list(dims_b), 0.5)
    Y = np.cos(3.0 * xa.sum(1))[:, None] * (1.0 + xb.sum(1))[None, :] + 0.1 * rng.standard_normal((na, nb)) + 5.0
    return m, ref, U * sa[:, None], V * sb[:, None], sa, Y


@pytest.mark.parametrize("dims_b", SPLITS)
def test_reference_agrees_with_the_float64_oracle(dims_b):
    """The oracle's ob_getmat on the expanded rows, summed in float64 over all na nb rows, against the reference
    under the ROWS' rule (k = na nb: that many summands were added); and the separated algebra in float64 from
    the oracle's own side factors under the reference's rule, k = na + nb + extra."""
    import ob_oracle as O
    m, ref, At, Bt, _, Y = case(129, dims_b, 37, 41)
    Bo = O.ob_getmat(O.OuterBase(m["om_o"], ref.x), m["terms"])
    cols = E.gram_column_sample(ref.bB, 99)
    v = ref.flat(Y - Y[0, 0])
    want, bound, absum = ref.gram_parts(cols)
    r_rows = E.worst_ratio(Bo[:, cols].T @ Bo, want, E._sum_tol(ref.C, bound, ref.na * ref.nb, absum))
    wr, br, ar = ref.tm_parts(v)
    r_rows = max(r_rows, E.worst_ratio(Bo.T @ v, wr, E._sum_tol(ref.C, br, ref.na * ref.nb, ar)))
    G, R, b1 = F.device_algebra(At, Bt, Y - Y[0, 0])
    r_g = E.worst_ratio(G[cols, :], *ref.gram(cols))
    r_r = E.worst_ratio(R, *ref.tmatmul(v))
    r_1 = E.worst_ratio(b1, *ref.tmatmul(np.ones(ref.na * ref.nb)))
    print("dims_b = %s: oracle rows err/tol %.3g; separated float64 err/tol triangle %.3g, R %.3g, b1 %.3g"
          % (dims_b, r_rows, r_g, r_r, r_1))
    assert max(r_rows, r_g, r_r, r_1) <= 1.0


def test_a_mutated_algebra_passes_a_flat_bound_and_fails_the_rule():
    """One 64-row chunk of xb left out of one column of R.  The response is 1e-7 of its usual size on that
    chunk, so the column moves by about 1e-7 of itself: a flat 1e-6 of the max-norm lets it through, the
    per-entry rule (about 1e-13 of the sum of |summands|) does not.  The unmutated algebra passes both."""
    dims_b = [1, 3]
    m, ref, At, Bt, sa, Y = case(129, dims_b, 20, 130)
    Y = Y - Y[0, 0]
    Y[:, 64:128] *= 1e-7
    v = ref.flat(Y)
    want, tol = ref.tmatmul(v)
    k = int(np.argmax(np.abs(E._f64(want))))
    good = F.device_algebra(At, Bt, Y)[1]
    bad = F.device_algebra(At, Bt, Y, skip_chunk=(1, k))[1]
    flat = lambda got: E.maxnorm_relerr(got, want)
    print("column %d: flat error good %.3g, mutated %.3g; err/tol good %.3g, mutated %.3g"
          % (k, flat(good), flat(bad), E.worst_ratio(good, want, tol), E.worst_ratio(bad, want, tol)))
    assert flat(good) < 1e-6 and E.worst_ratio(good, want, tol) <= 1.0
    assert flat(bad) < 1e-6 and E.worst_ratio(bad, want, tol) > 1.0
    assert bad[k] != good[k]


def test_new_symbols_are_declared_and_exported_by_both_libraries():
    from outerbase_amd import _lib
    testing = C.CDLL(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"))
    for name, nargs in NEW.items():
        assert name in _lib.PROTOS and len(_lib.PROTOS[name][1]) == nargs, name
        assert hasattr(_lib.lib, name) and hasattr(testing, name), name
    assert _lib.lib.obhip_abi_version() == 5 and testing.obhip_abi_version() == 5    # purely additive
    header = open(_lib.HEADER).read()
    for name in NEW:
        i = header.index("int " + name + "(")
        assert "No reference counterpart" in header[header.rindex("/*", 0, i):i], name


def test_python_names_are_exported():
    import outerbase_amd as ob
    for name in ("fit_newton_product", "product_side", "product_fit_layout"):
        assert name in ob.__all__ and callable(getattr(ob, name)), name
    assert callable(ob.NewtonAccumulator.add_product) and callable(ob.NewtonAccumulator.remove_product)


def test_new_sources_are_built_and_read_no_new_switch():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    known = set()
    for f in os.listdir(CSRC):
        if f.endswith((".cpp", ".hip", ".h")) and f not in NEW_SOURCES:
            known |= set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', open(os.path.join(CSRC, f)).read()))
    for f in NEW_SOURCES:
        assert re.search(r"^SRC_(HIP|CPP) = .*\b%s\b" % re.escape(f), mk, flags=re.M), f
        read = set(re.findall(r'getenv\("([A-Z0-9_]+)"\)', open(os.path.join(CSRC, f)).read()))
        assert read <= known and read <= {"OBHIP_GRAM_CHUNK_ROWS", "OBHIP_FORCE_GENERIC"}, (f, read)


def test_layout_on_the_host():
    from outerbase_amd import product_fit_layout, product_layout
    m, _ = model("mixed d4 p129")
    for dims_b in SPLITS:
        mu_a, mu_b, fa, fb = product_fit_layout(m["om_d"], m["terms"], dims_b)
        assert (mu_a, mu_b) == product_layout(m["om_d"], m["terms"], dims_b)[:2] and fa and fb


def test_refusals_before_any_device_call():
    """every refusal that needs no device returns OBHIP_ERR_INVALID here, where a call that reached the device
    would return OBHIP_ERR_NO_DEVICE; what was refused wrote nothing.  (An accumulator needs a device to exist:
    the rest of obhip_normal_acc_add_product_dev's order is checked in test_gpu_product_fit.py.)"""
    from outerbase_amd import _lib, obmod
    lib = _lib.lib
    m, _ = model("mixed d4 p129")
    t = obmod._terms_of(m["om_d"], m["terms"])
    om, p = m["om_d"]._h, t.p
    buf = np.zeros(4096)
    sentinel = np.full(64 * 256, np.nan)
    a, out = buf.ctypes.data, sentinel.ctypes.data
    u32 = lambda v: np.asarray(v, dtype=np.uint32)
    ok = u32([1, 3])
    mu = C.c_uint64(7)
    fu = C.c_int(7)
    side = lib.obhip_product_side_dev
    for db in ([4], [1, 1], [3, 1], [], [0, 1, 2, 3]):
        d = u32(db)
        assert lib.obhip_product_fit_layout(t._h, d.ctypes.data, d.size, C.byref(mu), None, C.byref(fu), None) == INVALID
        assert side(om, t._h, d.ctypes.data, d.size, 0, a, 3, out, 256) == INVALID
    assert mu.value == 7 and fu.value == 7
    assert lib.obhip_product_fit_layout(None, ok.ctypes.data, 2, None, None, None, None) == INVALID
    assert lib.obhip_product_fit_layout(t._h, None, 2, None, None, None, None) == INVALID
    assert side(None, t._h, ok.ctypes.data, 2, 0, a, 3, out, 256) == INVALID
    assert side(om, None, ok.ctypes.data, 2, 0, a, 3, out, 256) == INVALID
    assert side(om, t._h, None, 2, 0, a, 3, out, 256) == INVALID
    for bad_side in (-1, 2):
        assert side(om, t._h, ok.ctypes.data, 2, bad_side, a, 3, out, 256) == INVALID
    assert side(om, t._h, ok.ctypes.data, 2, 1, a, 3, out, p - 1) == INVALID        # pitch < p
    assert side(om, t._h, ok.ctypes.data, 2, 0, None, 3, out, 256) == INVALID
    assert side(om, t._h, ok.ctypes.data, 2, 0, a, 3, None, 256) == INVALID
    assert side(om, t._h, ok.ctypes.data, 2, 0, None, 0, None, 256) == 0            # nothing to do
    assert np.all(np.isnan(sentinel))
    add = lib.obhip_normal_acc_add_product_dev
    assert add(None, a, 3, a, 2, ok.ctypes.data, 2, a, 3, 1) == INVALID


def test_python_argument_checks():
    import outerbase_amd as ob
    m, _ = model("mixed d4 p129")
    om, terms = m["om_d"], m["terms"]
    xa, xb = np.full((3, 2), 0.5), np.full((2, 2), 0.5)
    with pytest.raises(ValueError):
        ob.product_side(om, terms, xa, [1, 3], 2)
    with pytest.raises(ValueError):
        ob.product_side(om, terms, np.full((3, 3), 0.5), [1, 3], 0)
    with pytest.raises(ValueError):
        ob.product_fit_layout(om, terms, [3, 1])
    with pytest.raises(ValueError):
        ob.fit_newton_product(om, terms, xa, xb, np.zeros(6), [1, 3])
    acc = ob.NewtonAccumulator(om, terms, 2)
    for Y in (np.zeros((3, 2)), np.zeros((3, 2, 3)), np.zeros((2, 3, 2))):      # q = 2: the shape must say so
        with pytest.raises(ValueError):
            acc.add_product(xa, xb, Y, [1, 3])
    with pytest.raises(ValueError):
        acc.add_product(xa[:0], xb, np.zeros((0, 2, 2)), [1, 3])
    with pytest.raises(ValueError):
        acc.add_product(xa, xb, np.full((3, 2, 2), np.nan), [1, 3])
    with pytest.raises(ValueError):
        acc.remove_product(xa, xb, np.zeros((3, 2, 2)), [3, 1])
    acc.close()
