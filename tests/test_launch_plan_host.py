"""Host check of csrc/launch_plan.h (no GPU): the row split and the units per lane that every product
launch takes from it, against a restatement of the formulas each call site wrote out before they were
folded into split_rows / units_per_lane.  tests/launch_plan_check.cpp is compiled with g++ under the
address and undefined-behaviour sanitizers and run as a program of its own."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (1, 104, 256, 304)
PBLOCKS = (1, 2, 3, 9, 17)
NTILES = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 1000, 15625)
P_PAD = (256, 512, 768, 1024, 1280, 2048, 2304, 4096, 4352, 9216)


def _finish(ntiles, nsplit):
    tps = (ntiles + nsplit - 1) // nsplit
    return (ntiles + tps - 1) // tps, tps


def _cap4(ntiles, nsplit):  # "each block at least 4 tiles"
    return _finish(ntiles, min(nsplit, max(1, ntiles // 4)))


def _cap1(ntiles, nsplit):
    return _finish(ntiles, min(nsplit, ntiles))


# every call-site form: name -> (the formula as the site wrote it, the `want` it now passes, min_tiles)
SITES = {
    "star_grid": (lambda c, pb, nt: _cap4(nt, max(1, c // pb)), lambda c, pb: c // pb, 4),
    "mm_tl / materialize_tl": (lambda c, pb, nt: _cap1(nt, max(1, c * 4 // pb)), lambda c, pb: c * 4 // pb, 1),
    "tmm_tl / tmm_dual / tmm_d3": (lambda c, pb, nt: _cap4(nt, max(1, c * 2 // pb)), lambda c, pb: c * 2 // pb, 4),
    "hessmult_fused": (lambda c, pb, nt: _cap4(nt, max(1, c)), lambda c, pb: c, 4),
    "tmm rows": (lambda c, pb, nt: _cap4(nt, max(1, (256 * 6 + pb - 1) // pb)),
                 lambda c, pb: (256 * 6 + pb - 1) // pb, 4),
    "tmm_ge0, two blocks per CU": (lambda c, pb, nt: _cap1(nt, max(1, c * 2 // pb)), lambda c, pb: c * 2 // pb, 1),
    "tmm_ge0, one block per CU": (lambda c, pb, nt: _cap1(nt, max(1, c // pb)), lambda c, pb: c // pb, 1),
    "bt_times_ge0": (lambda c, pb, nt: _finish(nt, max(1, min(nt, 1024 // pb))), lambda c, pb: 1024 // pb, 1),
    "tmm_generic": (lambda c, pb, nt: _cap4(nt, max(1, 4096 // max(1, pb))), lambda c, pb: 4096 // max(1, pb), 4),
    "predict_tl": (lambda c, pb, nt: _finish(nt, min(nt, c * 4)), lambda c, pb: c * 4, 1),
    "star_predict": (lambda c, pb, nt: _finish(nt, min(nt, c)), lambda c, pb: c, 1),
}

# (terms per unit, ceiling) pairs of the code: 8 waves x 64 terms per group with 8 | 4 (k_mm_tl, k_hm_tl,
# k_predict_tl) and 4 | 2 (k_predict_tl with the variance); 8 waves x 128 per pair with 4 | 2 (k_tmm_tl,
# k_materialize_tl)
UNITS = ((512, 8), (512, 4), (512, 2), (1024, 4), (1024, 2))


def _units_before(p_pad, tpu, mx):
    u = 1
    while u < mx and tpu * u < p_pad:
        u *= 2
    return u


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "launch_plan_check.cpp"), "-o", exe],
                   check=True)

    def run(queries):
        queries = list(queries)
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == len(queries)
        return rows

    return run


def test_every_call_site_splits_the_rows_as_before(ask):
    cases = [(name, c, pb, nt) for name in SITES for c, pb, nt in itertools.product(CUS, PBLOCKS, NTILES)]
    got = ask("S %d %d %d" % (nt, SITES[name][1](c, pb), SITES[name][2]) for name, c, pb, nt in cases)
    bad = [(case, g) for case, g in zip(cases, got) if g != SITES[case[0]][0](*case[1:])]
    print("%d splits compared over %d call-site forms" % (len(cases), len(SITES)))
    assert not bad, bad[:5]


def test_split_invariants(ask):
    wants = sorted({SITES[name][1](c, pb) for name in SITES for c in CUS for pb in PBLOCKS} | {0})
    cases = list(itertools.product(NTILES, wants, (1, 4)))
    got = ask("S %d %d %d" % c for c in cases)
    for (nt, want, mt), (nsplit, tps) in zip(cases, got):
        assert nsplit * tps >= nt > (nsplit - 1) * tps, (nt, want, mt, nsplit, tps)
        assert 1 <= nsplit <= max(1, nt // mt), (nt, want, mt, nsplit)
        assert nsplit <= max(1, want)
    print("%d splits checked" % len(cases))


def test_units_per_lane_as_before(ask):
    cases = list(itertools.product(P_PAD, UNITS))
    got = ask("U %d %d %d" % (p, tpu, mx) for p, (tpu, mx) in cases)
    for (p, (tpu, mx)), (u,) in zip(cases, got):
        assert u == _units_before(p, tpu, mx), (p, tpu, mx, u)
        # launch_hessmult_fused wrote the loop without a ceiling, behind the guard p_pad <= 512 x ceiling
        if tpu == 512 and p <= tpu * mx:
            v = 1
            while tpu * v < p:
                v *= 2
            assert u == v


def test_ceilings_by_term_width(ask):
    got = ask("C %d" % w2 for w2 in (1, 2, 3, 4))
    for w2, g in zip((1, 2, 3, 4), got):
        units, pairs = (8, 4) if w2 <= 2 else (4, 2)
        assert g == (units, pairs, units, units // 2)
    # every ceiling the dispatch can meet is one of the pairs test_units_per_lane_as_before runs
    assert {(512, g[0]) for g in got} | {(1024, g[1]) for g in got} | {(512, g[3]) for g in got} == set(UNITS)
