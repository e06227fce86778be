"""The N > 1 DEVICE path on the one GPU of the test box: two rank
processes share the GPU, each runs the device HotPath on its own contiguous row block, and
the one exchange buffer (packed triangle of G, B^T y, B^T 1, 3 scalars) is summed through
libobhip's host transport over gloo.  Compared with (a) the single-process device run on
all the rows and (b) the CPU oracle, both to 1e-6 relative as north_star asks.

This file sorts first and starts its rank processes before the pytest process itself has
touched the GPU; every GPU-using process here is a child with a fresh HIP runtime.
"""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "rank_worker.py")
KINDS = ["mat25", "mat25pow", "mat25", "mat25ang", "mat25", "mat25pow"]
KNOTS = 24


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(out_dir, world, backend, n_total, p, extra=(), worker=None):
    os.makedirs(out_dir, exist_ok=True)
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        argv = [sys.executable, WORKER, str(out_dir), backend, str(n_total), str(p), str(KNOTS),
                ",".join(KINDS)] + [str(e) for e in extra]
        if worker is not None:
            argv = [sys.executable, worker, str(out_dir)] + [str(e) for e in extra]
        procs.append(subprocess.Popen(
            argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(o.decode(errors="replace"))
    for rank, pr in enumerate(procs):
        assert pr.returncode == 0, "rank %d failed:\n%s" % (rank, outs[rank][-3000:])
    return [np.load(os.path.join(out_dir, "rank%d.npz" % r)) for r in range(world)]


def _oracle(n_total, p, rows_pred):
    """CPU oracle on all rows in one piece.  It takes the eigen-rotation of the library's
    own host-side model (no GPU involved), as every parity test does: trailing eigenpairs
    are not determined by either eigensolver."""
    import ob_oracle as O
    import outerbase_amd as ob
    om = O.OuterMod()
    om.setcovfs(KINDS)
    om.setknot(O.bench_knots(KINDS, KNOTS))
    om_d = ob.outermod()
    ob.setcovfs(om_d, KINDS)
    ob.setknot(om_d, O.bench_knots(KINDS, KNOTS))
    om.rotmat, om.basisvar, om.maxlevel = om_d.rotation()
    terms = om.selectterms(p)
    assert np.array_equal(terms, om_d.selectterms(p))
    x, y = O.synth_xy(42, 0, n_total, KINDS)
    cent, sd = y.mean(), y.std(ddof=1)
    theta, _ = O.fit_newton(O.OuterBase(om, x), terms, (y - cent) / sd, sigma=math.log(0.01))
    xnew, _ = O.synth_xy(43, 0, rows_pred, KINDS)
    return cent, sd, theta, cent + sd * O.predict_mean(om, terms, theta, xnew)


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("backend", ["newton", "cg"])
def test_two_rank_device_path_equals_single_process_and_oracle(tmp_path, backend):
    n_total, p = 6001, 300       # ragged split: 3000 + 3001 rows
    # PCG: run to convergence (tol 1e-13) -- stopped at obfit's iteration cap this small,
    # badly conditioned problem is far from converged, and unconverged CG iterates are not
    # reproducible to rounding across summation orders
    extra = (1e-13, 5000) if backend == "cg" else ()
    two = _run_ranks(tmp_path / "w2", 2, backend, n_total, p, extra)
    one = _run_ranks(tmp_path / "w1", 1, backend, n_total, p, extra)[0]
    assert [int(r["n"]) for r in two] == [3000, 3001] and int(two[1]["row0"]) == 3000
    assert all(int(r["ranks"]) == 2 for r in two)
    # replicated solve: the same theta on both ranks, bit for bit (Newton: same summed
    # buffer, same arithmetic)
    if backend == "newton":
        assert np.array_equal(two[0]["theta"], two[1]["theta"])
        assert np.array_equal(two[0]["G00"], two[1]["G00"])
    scale = np.max(np.abs(one["theta"]))
    for r in two:
        assert abs(r["cent"] - one["cent"]) < 1e-12 * max(1.0, abs(one["cent"]))
        assert abs(r["sd"] - one["sd"]) < 1e-12 * one["sd"]
        if backend == "newton":
            assert np.max(np.abs(r["theta"] - one["theta"])) < 1e-6 * scale
    # predictions of the two shards side by side == the single-process predictions
    mean2 = np.concatenate([two[0]["mean"], two[1]["mean"]])
    assert mean2.shape == one["mean"].shape
    assert np.max(np.abs(mean2 - one["mean"])) < 1e-6 * np.max(np.abs(one["mean"]))
    # and the CPU oracle on all rows in one piece
    cent, sd, theta_o, want = _oracle(n_total, p, 500)
    assert abs(one["cent"] - cent) < 1e-10 * max(1.0, abs(cent)) and abs(one["sd"] - sd) < 1e-10 * sd
    assert np.max(np.abs(mean2[:500] - want)) < 1e-6 * np.max(np.abs(want))
    if backend == "newton":
        assert np.max(np.abs(two[0]["theta"] - theta_o)) < 1e-6 * np.max(np.abs(theta_o))
    else:
        # same iterates on both ranks (every reduction is a sum over ranks); theta itself is
        # not pinned in the flat directions of the posterior, the predictions are
        assert np.array_equal(two[0]["theta"], two[1]["theta"])
        assert 0 < int(two[0]["iters"]) == int(two[1]["iters"]) < 5000


@pytest.mark.timeout(1500)
def test_row_sharded_obfit_equals_single_process(tmp_path):
    """obfit with the rows of the 8-d Borehole example sharded over two rank processes
    (ragged: 1000 + 1001 rows): y standardised, knots placed at quantiles and the first
    stage's rows drawn over ALL rows, every row sum of the second stage summed over ranks.
    Both ranks end with the same model, and it is the single-process model up to what the
    BFGS loop makes of the different summation order."""
    wk = os.path.join(ROOT, "tests", "obfit_worker.py")
    two = _run_ranks(tmp_path / "o2", 2, None, None, None, extra=(2001, 60), worker=wk)
    one = _run_ranks(tmp_path / "o1", 1, None, None, None, extra=(2001, 60), worker=wk)[0]
    for r in two:
        assert abs(r["y_cent"] - one["y_cent"]) < 1e-12 * abs(one["y_cent"])
        assert abs(r["y_sca"] - one["y_sca"]) < 1e-12 * one["y_sca"]
        assert np.array_equal(r["knots0"], one["knots0"])          # exact order statistics
    # the ranks agree with each other to the last bit (same sums on both)
    for k in ("hyp", "para", "coeff", "mean", "var"):
        assert np.array_equal(two[0][k], two[1][k]), k
    # and with the single process to optimisation accuracy
    assert np.max(np.abs(two[0]["hyp"] - one["hyp"])) < 1e-3
    sd = np.std(one["truth"])
    assert np.max(np.abs(two[0]["mean"] - one["mean"])) < 1e-4 * sd
    assert np.sqrt(np.mean((two[0]["mean"] - one["truth"]) ** 2)) < 0.03 * sd      # 60 terms only
    assert np.all(two[0]["var"] > 0)


@pytest.mark.timeout(1500)
def test_bench_self_launch_two_ranks(tmp_path):
    """`python bench.py --gpus 2` from a process that has not touched the GPU: bench.py starts
    its own two rank processes (torch.distributed.run), which share the one GPU of the test box
    and sum the exchange buffer through libobhip's host transport over gloo
    (OBHIP_DIST_BACKEND=gloo).  The line must describe a 2-rank strong-scaling job, and the
    predictions must be those of the 1-rank run on the same 200 000 rows."""
    import json
    bench = os.path.join(ROOT, "bench.py")
    base = [sys.executable, bench, "--rows", "200000", "--steps", "2", "--warmup", "1", "--full",
            "--no-cpu-baseline", "--no-config3", "--no-configs", "--fit-parity-rows", "6000"]
    env = dict(os.environ, OBHIP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    d2, d1 = str(tmp_path / "two.npz"), str(tmp_path / "one.npz")
    r2 = subprocess.run(base + ["--gpus", "2", "--dump", d2], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=900)
    assert r2.returncode == 0, r2.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in r2.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r2.stdout.decode()[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong"
    assert line["exchange"]["ranks"] == 2 and line["exchange"]["transport"] == "host"
    # the first contact with the transport verified itself before the warm-up
    st = line["exchange"]["selftest_result"]
    assert line["exchange"]["selftest"] == "passed" and st["allreduce_mismatches"] == 0
    assert st["elements"] * 8 + 24 == line["exchange"]["bytes_per_fit"]
    # parity of the 2-rank run itself: rank 0's predictions against the oracle's basis, Newton
    # stationarity with the matrix-free products summed through the communicator, and the
    # oracle's own fit on the first rows (sharded over both ranks) with nothing shared
    pc = line["parity_check"]
    assert pc["predict_max_rel_err"] < 1e-6 and pc["newton_residual_rel"] < 1e-10
    assert pc["theta_vs_oracle_rows"] < 1e-6 and pc["fit_vs_oracle"]["shared_rotation"]["predict_max_rel_err"] < 1e-6
    assert pc["fit_vs_oracle"]["terms_equal_oracle_selection"]
    assert line["config"]["rows_total"] == 200000 and line["config"]["rows_per_gpu"] == 100000
    assert line["value"] > 0 and line["alt_backend"]["max_rel_diff_of_predictions_vs_newton"] < 1e-6
    r1 = subprocess.run(base + ["--gpus", "1", "--no-alt-backend", "--no-fit-parity", "--dump", d1], env=env,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r1.returncode == 0, r1.stderr.decode(errors="replace")[-3000:]
    # the one-rank line also times an obfit function evaluation (PCG fit + hyper-gradients)
    line1 = [json.loads(l) for l in r1.stdout.decode().splitlines() if l.startswith("{")][-1]
    oe = line1["obfit_eval"]
    assert oe["ms_per_evaluation"] > 0 and np.isfinite(oe["gradhyp_norm"]) and oe["gradhyp_norm"] > 0
    assert oe["phases"]["tmm_d3"]["launches_per_evaluation"] >= 1        # the fused gradient pass ran
    two, one = np.load(d2), np.load(d1)
    assert int(two["world"]) == 2 and int(one["world"]) == 1 and int(two["n_total"]) == 200000
    assert np.max(np.abs(two["meansd"] - one["meansd"])) < 1e-12 * np.max(np.abs(one["meansd"]))
    assert np.max(np.abs(two["mean"] - one["mean"])) < 1e-6 * np.max(np.abs(one["mean"]))
    assert np.max(np.abs(two["theta"] - one["theta"])) < 1e-6 * np.max(np.abs(one["theta"]))
