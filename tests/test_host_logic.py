"""CPU-side tests of libobhip: the ABI surface, the host logic behind it
(covariances on knots, eigen-model, term selection, variances, priors, error
behaviour) against the oracle, and the loud failure without a GPU.  No device
arithmetic is called here.
"""
import ctypes as C
import os
import subprocess

import math

import numpy as np
import pytest

import ob_oracle as O
from conftest import KNOTS_REF, ROOT, make_pair


def test_library_exports_every_declared_symbol():
    from outerbase_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 55
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = sorted(set(protos) - exported)
    assert not missing, "declared in include/obhip.h but not exported: %s" % missing
    extra = sorted(s for s in exported if s.startswith("obhip_") and s not in protos)
    assert not extra, "exported but not declared: %s" % extra
    assert _lib.lib.obhip_abi_version() == 5


def test_header_cites_reference_for_every_entry_point():
    from outerbase_amd import _lib
    src = open(_lib.HEADER).read()
    for token in ("interfaceR.cpp", "modandbase.cpp", "linalg.cpp", "covfuncs.cpp", "fit.cpp",
                  "loglik_std.cpp", "loglik_gauss.cpp", "logpr_gauss.cpp"):
        assert token in src


@pytest.mark.parametrize("kind", ["mat25", "mat25pow", "mat25ang"])
def test_cov_gradhyp_host_matches_oracle(kind):
    """covf::cov_gradhyp through the ABI (module row interfaceR.cpp:775) vs the oracle."""
    import outerbase_amd as ob
    c = getattr(ob, "covf_" + kind)()
    rng = np.random.default_rng(3)
    lo, up = (0.05, 0.95) if kind != "mat25ang" else (0.1, 6.1)
    x1, x2 = rng.uniform(lo, up, 11), rng.uniform(lo, up, 7)
    c.hyp = c.hyp0 + 0.2 * rng.standard_normal(len(c.hyp0))
    got = c.cov_gradhyp(x1, x2)
    want = O.cov_gradhyp(kind, x1, x2, c.hyp)
    assert got.shape == want.shape == (11, 7, len(c.hyp0))
    assert np.max(np.abs(got - want)) < 1e-13 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("kind", ["mat25", "mat25pow", "mat25ang"])
def test_cov_host_matches_oracle(kind):
    import outerbase_amd as ob
    cls = {"mat25": ob.covf_mat25, "mat25pow": ob.covf_mat25pow, "mat25ang": ob.covf_mat25ang}[kind]
    c = cls()
    info = O.COV_INFO[kind]
    assert np.allclose(c.hyp0, info["hyp0"]) and np.allclose(c.hyplb, info["hyplb"])
    assert np.allclose(c.hypub, info["hypub"]) and np.allclose(c.hypvar, info["hypvar"])
    assert c.lowbnd == info["lowbnd"] and c.uppbnd == info["uppbnd"]
    rng = np.random.default_rng(0)
    x1 = info["lowbnd"] + (info["uppbnd"] - info["lowbnd"]) * (0.01 + 0.98 * rng.random(17))
    x2 = info["lowbnd"] + (info["uppbnd"] - info["lowbnd"]) * (0.01 + 0.98 * rng.random(9))
    c.hyp = np.asarray(info["hyp0"]) + 0.3
    assert np.allclose(c.cov(x1, x2), O.cov(kind, x1, x2, c.hyp), rtol=1e-14, atol=1e-15)
    assert np.allclose(np.diag(c.cov(x1, x1)), c.covdiag(x1))
    assert abs(c.lpdf(c.hyp) - O.cov_hyp_lpdf(kind, c.hyp)) < 1e-12
    assert c.lpdf(np.asarray(info["hypub"]) + 1.0) == -np.inf


def test_eigenmodel_matches_lapack_on_leading_levels():
    """outermod::build (modandbase.cpp:210-255) with the library's Jacobi solver
    vs the oracle's LAPACK: eigenvalues to 1e-9 relative and rotation columns to
    1e-7 on the levels with lambda_j / lambda_0 > 1e-9; maxlevel identical."""
    kinds = ["mat25pow", "mat25", "mat25ang"]
    om_o, om_d = make_pair(kinds, O.bench_knots(kinds, 40), share_rotation=False)
    rot, bv, ml = om_d.rotation()
    assert rot.shape == om_o.rotmat.shape
    for l in range(3):
        o = om_o.knotptst[l]
        lam = np.exp(om_o.basisvar[o:o + 40])
        good = np.nonzero(lam / lam[0] > 1e-9)[0]
        assert len(good) >= 8
        assert np.allclose(bv[o + good], om_o.basisvar[o + good], atol=1e-7)
        if kinds[l] == "mat25ang":
            # the periodic kernel has (near-)degenerate sin/cos eigen-pairs: only the
            # eigenvalues are determined, the basis inside a pair is not
            continue
        num = np.abs(rot[:, o + good] - om_o.rotmat[:, o + good]).max(axis=0)
        den = np.abs(om_o.rotmat[:, o + good]).max(axis=0)
        assert np.all(num / den < 1e-5)
    assert np.all(np.abs(ml - om_o.maxlevel) <= 2)
    assert np.all(ml >= 8)


def test_eigenmodel_gradient_matches_oracle():
    """gradient part of outermod::build (modandbase.cpp:257-274) and getlvar_gradhyp
    (:364-379): library (Jacobi) vs oracle (LAPACK) on the leading levels; the layout
    (hypmatch, gest) exactly."""
    kinds = ["mat25pow", "mat25", "mat25ang", "mat25"]
    hyp = np.array([0.1, -0.05, 0.08, -0.1, 0.05, 0.02])
    om_o, om_d = make_pair(kinds, O.bench_knots(kinds, 24), hyp=hyp, share_rotation=False)
    hm, ge = om_d.grad_layout()
    assert np.array_equal(hm, om_o.hypmatch) and np.array_equal(ge, om_o.gest)
    rg, lv = om_d.rotation_grad()
    assert rg.shape == om_o.rotmat_gradhyp.shape
    lead = 6
    for h in range(len(hm)):
        sl = slice(ge[h], ge[h] + lead)
        assert np.allclose(lv[sl], om_o.logbasisvar_gradhyp[sl], atol=1e-7)
        if kinds[hm[h]] == "mat25ang":
            continue  # degenerate sin/cos eigen-pairs, see above
        ref = om_o.rotmat_gradhyp[:, sl]
        assert np.max(np.abs(rg[:, sl] - ref)) < 1e-6 * np.max(np.abs(ref))
    terms = om_o.selectterms(60)
    assert np.allclose(om_d.getlvar_gradhyp(terms), om_o.getlvar_gradhyp(terms), atol=1e-6)
    # injected gradient tables come back unchanged
    om_d.set_rotation_grad(om_o.rotmat_gradhyp, om_o.logbasisvar_gradhyp)
    rg2, lv2 = om_d.rotation_grad()
    assert np.array_equal(rg2, om_o.rotmat_gradhyp) and np.array_equal(lv2, om_o.logbasisvar_gradhyp)


@pytest.mark.parametrize("kinds,m,p", [
    (["mat25pow"] + ["mat25"] * 7, None, 20),          # test-obombasic.R
    (["mat25"] * 10, 40, 1024),                        # BASELINE config 2
    (["mat25", "mat25pow", "mat25ang"] * 2, 24, 500),
])
def test_selectterms_equals_oracle(kinds, m, p):
    knots = [KNOTS_REF] * len(kinds) if m is None else O.bench_knots(kinds, m)
    om_o, om_d = make_pair(kinds, knots)
    got = om_d.selectterms(p)
    assert np.array_equal(got, om_o.selectterms(p))
    assert np.allclose(om_d.getvar(got), om_o.getvar(got), rtol=1e-13)
    # the seeded variant (stand-in for the reference's R-RNG shuffle) keeps the invariants
    rnd = om_d.selectterms(p, seed=12345)
    assert np.array_equal(rnd, om_d.selectterms(p, seed=12345))
    seen = set()
    for t in rnd:
        tt = tuple(int(v) for v in t)
        for l in range(len(kinds)):
            if t[l] > 0:
                par = list(tt)
                par[l] -= 1
                assert tuple(par) in seen
        seen.add(tt)
    assert len(seen) == p


def test_headline_terms_statistics():
    """the deterministic selection used by bench.py for BASELINE config 3."""
    kinds = ["mat25"] * 20
    _, om_d = make_pair(kinds, O.bench_knots(kinds, 40), share_rotation=False)
    terms = om_d.selectterms(4096)
    assert terms.shape == (4096, 20)
    assert terms.max() == 5
    nnz = (terms > 0).sum(axis=1)
    assert nnz.max() == 4 and int(nnz.sum()) == 12177


def test_hyp_and_prior_plumbing():
    import outerbase_amd as ob
    kinds = ["mat25pow", "mat25", "mat25ang"]
    om_o, om_d = make_pair(kinds, O.bench_knots(kinds, 16), share_rotation=False)
    hyp = ob.gethyp(om_d)
    assert np.array_equal(hyp, om_o.hyp) and len(hyp) == 5
    assert ob.hypnames(om_d) == ["inpt1.scale", "inpt1.power", "inpt2.scale", "inpt3.sin.sc",
                                 "inpt3.cos.sc"]
    h2 = hyp + np.array([0.1, -0.05, 0.2, 0.0, -0.3])
    assert abs(om_d.hyplpdf(h2) - om_o.hyplpdf(h2)) < 1e-12
    assert om_d.hyplpdf(hyp[:3]) == -np.inf
    om_d.updatehyp(h2)
    om_o.hyp_set(h2)
    assert np.allclose(om_d.basisvar[:5], om_o.basisvar[:5], atol=1e-9)
    t = om_o.selectterms(40)
    pr = ob.logpr_gauss(om_d, t)
    pr.update(np.linspace(-1, 1, 40))
    coeffsd = np.sqrt(om_o.getvar(t))
    sca = np.exp(6.0)
    sr = np.linspace(-1, 1, 40) / (coeffsd * sca)
    assert abs(pr.val - (-0.5 * np.sum(sr ** 2) - np.sum(np.log(coeffsd * sca)))) < 1e-6 * abs(pr.val)
    assert np.allclose(pr.diaghess(), O.prior_prec(om_o, t, 6.0), rtol=1e-6)
    assert np.array_equal(ob.getpara(pr), [6.0])


def test_error_behaviour_matches_reference():
    import outerbase_amd as ob
    from outerbase_amd import _lib
    om = ob.outermod()
    with pytest.raises(RuntimeError):          # interfaceR.cpp:95-98
        ob.setknot(om, [KNOTS_REF])
    with pytest.raises(ValueError):
        ob.setcovfs(om, ["mat52"])
    ob.setcovfs(om, ["mat25", "mat25"])
    with pytest.raises(ValueError):            # interfaceR.cpp:99-106 dims
        ob.setknot(om, [KNOTS_REF])
    with pytest.raises(ob.ObhipError) as e:    # interfaceR.cpp:107-119 bounds
        ob.setknot(om, [KNOTS_REF, KNOTS_REF + 0.5])
    assert "knot point needs to be between" in str(e.value)
    with pytest.raises(ob.ObhipError):         # selectterms before knots
        om.selectterms(5)
    ob.setknot(om, [KNOTS_REF, KNOTS_REF])
    with pytest.raises(ob.ObhipError):         # modandbase.cpp:171-176 (check the reference commented out)
        om.updatehyp([0.0])
    with pytest.raises(ob.ObhipError):         # level beyond the knots
        om.getvar(np.array([[0, 99]]))
    assert _lib.lib.obhip_last_error() != b""


def test_no_gpu_fails_loudly():
    """Without a device every device-touching entry point returns
    OBHIP_ERR_NO_DEVICE; there is no CPU fallback to fall into."""
    import torch
    import outerbase_amd as ob
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    assert ob.device_count() == 0
    om = ob.outermod()
    ob.setcovfs(om, ["mat25"] * 3)
    ob.setknot(om, [KNOTS_REF] * 3)
    x = np.random.default_rng(0).random((10, 3))
    with pytest.raises(ob.ObhipError) as e:
        ob.outerbase(om, x)
    assert e.value.code == 2 and "no CPU fallback" in str(e.value)
    t = om.selectterms(8)
    with pytest.raises(ob.ObhipError):
        ob.loglik_gauss(om, t, x[:, 0], x)
    from outerbase_amd import _lib
    p = C.c_void_p()
    assert _lib.lib.obhip_malloc(C.byref(p), 64) == 2
    # the communicator entry points of ABI 4: virtual ranks need the device too; argument errors
    # come back as OBHIP_ERR_INVALID, never as a crash
    h = C.c_void_p()
    assert _lib.lib.obhip_comm_init_sim(C.byref(h), 8) == 2
    assert _lib.lib.obhip_comm_selftest_dev(None, 100, None) == 1
    assert _lib.lib.obhip_comm_exchange_path(None, 100, None, None) == 1
    # a host communicator needs no device to exist; its exchange path is reported, its self-test
    # (device buffers) is refused without a GPU
    assert _lib.lib.obhip_comm_init_host(C.byref(h), 1, 0, None, None) == 0
    path, st = C.c_int(-1), C.c_int(-1)
    assert _lib.lib.obhip_comm_exchange_path(h, 1 << 20, C.byref(path), C.byref(st)) == 0
    assert (path.value, st.value) == (3, 0)
    assert _lib.lib.obhip_comm_selftest_dev(h, 100, None) == 2
    _lib.lib.obhip_comm_destroy(h)


def test_product_path_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "outerbase_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "ob_oracle" not in txt and "oracle/" not in txt, f


# ---- the R-side harness restated (outerbase_amd/fitting.py) -----------------------------------
def test_bfgs_std_minimises_and_steps_away_from_infinite_values():
    """BFGS_std (R/outersupport.R:30-171): a smooth bowl with an infinite wall next to
    the start, as hyper-parameter priors produce (".lpdfwrapper" returns Inf, :224)."""
    from outerbase_amd.fitting import BFGS_std

    # the reference stops once the predicted decrease st.g is above -length(g)/4 twice
    # (:133-137), a rule made for log-likelihoods of many observations: scale accordingly
    sc = 1e6

    def funcw(pl, shift):
        u = np.concatenate([pl["hyp"], pl["para"]]) - shift
        if pl["hyp"][0] > 1.5:                       # outside the box
            return {"val": math.inf, "gval": None}
        val = sc * float(np.sum(u ** 2) + 0.1 * np.sum(u ** 4))
        g = sc * (2 * u + 0.4 * u ** 3)
        return {"val": val, "gval": {"hyp": g[:2], "para": g[2:]}}

    shift = np.array([1.0, -0.5, 0.3])
    start = {"hyp": np.array([1.4, 1.0]), "para": np.array([2.0])}
    out = BFGS_std(funcw, start, lr=0.5, shift=shift)
    got = np.concatenate([out["parlist"]["hyp"], out["parlist"]["para"]])
    assert np.max(np.abs(got - shift)) < 2e-3
    assert out["optid"]["val"] < 1e-6 * funcw(start, shift)["val"]
    assert out["B"].shape == (3, 3)


def test_fitting_helpers_and_argument_checks():
    """.genknotlist / .getsteps / .checkcov and obfit's stop() conditions
    (R/fitting.R:30-53, 158-195)."""
    from outerbase_amd import fitting as F
    rng = np.random.default_rng(0)
    x = rng.random((200, 4))
    # (.genknotlist evaluates its quantiles on the device: tests/test_gpu_parity.py)
    assert F._getsteps(4096, 1e6, 1e4) == O.getsteps(4096, 1e6, 1e4) == 35
    with pytest.raises(ValueError, match="do not align"):
        F.obfit(x, np.zeros(10))
    with pytest.raises(ValueError, match="dimension 2"):
        F.obfit(x[:, :2], np.zeros(200))
    with pytest.raises(ValueError, match="twice the dimension"):
        F.obfit(x, np.zeros(200), numb=7)
    with pytest.raises(ValueError, match="listcov"):
        F.obfit(x, rng.random(200), numb=20, covnames=["nope"] * 4)
    with pytest.raises(ValueError, match="exceed limits"):
        F.obfit(x * 3, rng.random(200), numb=20)
    with pytest.raises(ValueError, match="too small"):
        F.obfit(0.5 + 0.01 * x, rng.random(200), numb=20)


# ---- the reference-side binding (glue/obhip_glue.cpp) ----------------------------------------
def _module_surface(src):
    """names exposed by an RCPP_MODULE block: free functions, and per class its methods and
    fields / properties"""
    import re
    body = src[src.index("RCPP_MODULE(obmod)"):]
    funcs = set(re.findall(r'\bfunction\(\s*"(\w+)"', body))
    classes = {}
    for m in re.finditer(r'class_<\w+>\(\s*"(\w+)"\s*\)(.*?);', body, flags=re.S):
        names = set(re.findall(r'\.(?:method|field|field_readonly|property)\(\s*"(\w+)"', m.group(2)))
        classes[m.group(1)] = names
    return funcs, classes


def test_glue_declares_only_abi_symbols():
    import re
    from outerbase_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    glue = open(os.path.join(root, "glue", "obhip_glue.cpp")).read()
    used = set(re.findall(r"\b(obhip_\w+)\s*\(", glue))
    protos = _lib.parse_header()
    assert used and not sorted(used - set(protos)), sorted(used - set(protos))
    funcs, classes = _module_surface(glue)
    assert funcs == {"setcovfs", "setknot", "gethyp", "getpara"}
    assert set(classes) == {"outermod", "outerbase", "lpdf", "predictor", "loglik_std", "loglik_gauss",
                            "loglik_gda", "logpr_gauss", "lpdfvec", "covf", "covf_mat25",
                            "covf_mat25pow", "covf_mat25ang"}


def test_glue_keeps_its_module_surface():
    """Every function, class, method and field of the glue's RCPP_MODULE(obmod) -- the names of
    the reference's module (src/interfaceR.cpp:661-793) -- recorded in
    tests/golden/module_surface.json is still there under the same name."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = json.load(open(os.path.join(root, "tests", "golden", "module_surface.json")))
    rf = set(rec["functions"])
    rc = {cls: set(names) for cls, names in rec["classes"].items()}
    assert rf and len(rc) == 13
    gf, gc = _module_surface(open(os.path.join(root, "glue", "obhip_glue.cpp")).read())
    assert rf == gf
    assert set(rc) == set(gc)
    for cls, names in rc.items():
        assert names <= gc[cls], (cls, sorted(names - gc[cls]))


def test_glue_passes_the_compilers_front_end():
    """glue/obhip_glue.cpp through g++'s parser and type checker against include/obhip.h and a
    declaration-only stand-in for <Rcpp.h> (tests/rcpp_stub/Rcpp.h: test infrastructure -- R and
    Rcpp are not in this image).  Catches misspelt or mis-typed ABI calls and malformed module
    declarations; it says nothing about Rcpp's real semantics and nothing is linked."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [gxx, "-std=c++11", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "tests", "rcpp_stub"),
           "-I" + os.path.join(root, "include"), os.path.join(root, "glue", "obhip_glue.cpp")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    # the check is live: a call with a wrong argument list must be rejected
    src = open(os.path.join(root, "glue", "obhip_glue.cpp")).read()
    broken = src.replace("ck(obhip_basis_rebuild(h));", "ck(obhip_basis_rebuild(h, 1));", 1)
    assert broken != src
    r = subprocess.run(cmd[:-1] + ["-x", "c++", "-"], input=broken.encode(), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert r.returncode != 0 and b"obhip_basis_rebuild" in r.stdout


def test_every_environment_switch_is_documented():
    """Every OBHIP_* variable the library reads is a row of INTEGRATION.md's table, and the table
    lists nothing the library does not read (round-4 verdict: 30 switches, two documented
    nowhere)."""
    import glob
    import re
    csrc = os.path.join(ROOT, "outerbase_amd", "csrc")
    read = set()
    for f in glob.glob(os.path.join(csrc, "*")):
        if f.endswith((".cpp", ".hip", ".h")):
            read |= set(re.findall(r'getenv\("(OBHIP_[A-Z0-9_]+)"\)', open(f).read()))
    assert len(read) >= 25
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    i = doc.index("Environment variables the library reads")
    j = doc.index("## Behavioural differences")
    rows = [ln for ln in doc[i:j].splitlines() if ln.startswith("| `OBHIP_")]
    listed = set()
    for ln in rows:
        listed |= set(re.findall(r"`(OBHIP_[A-Z0-9_]+)", ln))
    assert read - listed == set(), "undocumented switches: %s" % sorted(read - listed)
    assert listed - read == set(), "documented but never read: %s" % sorted(listed - read)


def test_shipping_library_has_no_fault_injector():
    """The exchange's fault injector (tests of obhip_comm_selftest_dev's in-process switch) lives in
    the test build only: libobhip.so neither exports obhip_testing_* nor consults the environment
    for it; libobhip_testing.so exports the arming entry point."""
    from outerbase_amd import _lib
    assert not hasattr(_lib.lib, "obhip_testing_fault_inject_pair")
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"FAULT_INJECT" not in blob and b"obhip_testing" not in blob
    tst = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "libobhip_testing.so"), "rb").read()
    assert b"obhip_testing_fault_inject_pair" in tst
    src = open(os.path.join(ROOT, "outerbase_amd", "csrc", "comm.cpp")).read()
    assert src.count("#ifdef OBHIP_TESTING") == 3 and "FAULT_INJECT" not in src


def _check_star_tables(om_d, terms):
    """The star tables of a term set (obhip_terms_share_tables): every padded term is in exactly
    one family star or left over (and then in exactly one plain star), and every term's factors
    are exactly its star's shared part plus its own slots."""
    import outerbase_amd as ob
    from outerbase_amd._lib import call, ptr
    tt = ob.obmod._Terms(om_d, terms)
    info = np.zeros(11, dtype=np.uint64)
    call("obhip_terms_share_tables", tt._h, ptr(info), None, None, None, None)
    p_pad, nleft, reads, reads_plain, W, lds_cyc, lds_cyc0, nswf, nswp, reads_left, lds_cyc_re = (int(v) for v in info)
    p, d = terms.shape
    assert p_pad == (p + 255) // 256 * 256 and W == max(2, ((terms > 0).sum(1).max() + 1) // 2 * 2)
    nst = 64 * (nswf + nswp)
    assert nst <= p_pad // 4 + 128 and nswp == (nleft + 255) // 256
    term = np.zeros(4 * nst, dtype=np.uint32)
    shape = np.zeros(nswf + nswp, dtype=np.uint32)
    fac = np.zeros(nst * 4 * W, dtype=np.uint16)
    left = np.zeros(max(nleft, 1), dtype=np.uint32)
    call("obhip_terms_share_tables", tt._h, ptr(info), ptr(term), ptr(shape), ptr(fac), ptr(left))
    left = left[:nleft]
    term = term.reshape(nst, 4)
    none = 0xffffffff
    fam_terms = term[:64 * nswf][term[:64 * nswf] != none]
    plain_terms = term[64 * nswf:][term[64 * nswf:] != none]
    assert sorted(fam_terms.tolist() + left.tolist()) == list(range(p_pad))       # a partition
    assert sorted(plain_terms.tolist()) == sorted(left.tolist())
    maxlev = terms.max(0)
    off = 1 + np.concatenate([[0], np.cumsum(maxlev)])
    want = [sorted(int(off[l] + terms[k, l] - 1) for l in range(d) if terms[k, l] > 0) for k in range(p)]
    want += [[] for _ in range(p_pad - p)]
    fac = fac.reshape(nst, 4 * W)
    tot = tot_left = 0
    for s in range(nst):
        P, S = int(shape[s // 64]) & 0xff, int(shape[s // 64]) >> 8
        if s // 64 < nswf:
            assert S == 1 and 1 <= P < W
        else:
            assert P == 0 and S in (W, max(W - 2, 1) if W >= 4 else W)
        shared = [int(v) for v in fac[s, :P] if v]
        for j in range(4):
            own = [int(v) for v in fac[s, P + j * S:P + (j + 1) * S] if v]
            if term[s, j] == none:
                assert not own                                          # an empty slot
            else:
                assert sorted(shared + own) == want[int(term[s, j])]
        assert not fac[s, P + 4 * S:].any()
    for w in range(nswf + nswp):
        c = (int(shape[w]) & 0xff) + 4 * (int(shape[w]) >> 8)
        if w < nswf:
            tot += c
        else:
            tot_left += c
    assert tot == reads and tot_left == reads_left
    assert 2 * (reads + reads_left) <= lds_cyc <= lds_cyc0 and 2 * (reads + reads_left) <= lds_cyc_re <= lds_cyc0
    return nleft, reads, reads_plain


def test_star_tables_of_downward_closed_and_arbitrary_term_sets():
    """Shared sub-products (csrc/share.cpp): on selectterms' downward-closed sets
    (modandbase.cpp:419-436) nearly every term lands in a star of four that differ in one factor
    and the column reads per row fall by 40-50 %; a term set that is NOT downward-closed
    (caller-supplied terms) is accepted all the same -- what finds no family goes into plain
    stars."""
    import ob_oracle as O
    import outerbase_amd as ob
    kinds = ["mat25"] * 20
    om_o, om_d = make_pair(kinds, O.bench_knots(kinds))
    terms = om_d.selectterms(4096)                                      # the headline term set
    nleft, reads, reads_plain = _check_star_tables(om_d, terms)
    assert nleft <= 64 and reads <= 0.55 * reads_plain and reads_plain == 194
    kinds = ["mat25pow"] * 8
    om_o, om_d = make_pair(kinds, O.bench_knots(kinds))
    nleft, reads, reads_plain = _check_star_tables(om_d, om_d.selectterms(3000))    # six-factor terms
    assert nleft <= 192 and reads <= 0.65 * reads_plain
    # not downward-closed: random multi-indices, a few of them sharing factors by chance
    rng = np.random.default_rng(5)
    kinds = ["mat25"] * 12
    om_o, om_d = make_pair(kinds, O.bench_knots(kinds))
    for p, nnz in ((700, 4), (300, 2), (1500, 7)):
        t = np.zeros((p, 12), dtype=np.int64)
        for k in range(p):
            dims = rng.choice(12, size=int(rng.integers(0, nnz + 1)), replace=False)
            t[k, dims] = rng.integers(1, 6, len(dims))
        t = np.unique(t, axis=0)
        nleft, reads, reads_plain = _check_star_tables(om_d, t)
        assert nleft > 0
    # isolated terms only: everything plain, nothing shared
    t = np.zeros((40, 12), dtype=np.int64)
    for k in range(40):
        t[k, [(3 * k) % 12, (3 * k + 1) % 12]] = 1 + k % 5, 1 + (k // 5) % 5
    _check_star_tables(om_d, np.unique(t, axis=0))
