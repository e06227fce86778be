"""The posterior draws on the device (csrc/sample.cpp, kernels_sample.hip) against the long-double reference of
tests/sample_ref.py, at the smallest shapes at which the kernels can go wrong: p = 5 (one partial 4-term step
of the matrix instruction), 67 and 130; S = 1, 15, 16, 17 around a 16-column block, 65 (the second pass of
the 64-draw chunk) and 129 (the second pass of the fused kernel's 128 draws); m = 1, 63, 64, 65, 129 around the 64-row tile and 1000 (16 workgroups through the partial
reduction); a d = 40 term set with 198 used columns in the tile.  Every case runs on the fused kernel and again
under OBHIP_FORCE_GENERIC (paths to scratch, k_sample_colext).

test_sample_host.py has shown ON THE REFERENCE ALONE that the best two candidates of every draw of every case
are more than 1000 allowances apart: the picks are determined, and the device must return the reference's,
all of them.  Draws, paths and values are held to C x (summands) x (magnitudes) of sample_ref.py, C eight times
the float64 restatement's own err / bound on the same case; every check prints err / tolerance.  Besides the
reference the entries are held to each other bit for bit: sample is the multi-response predictor on draw's
output, and extremum is min / argmin of sample's own matrix.  Output buffers are padded and the padding must
stay as it was."""
import numpy as np
import pytest

import extended_ref as E
import sample_ref as R
from test_sample_host import built, twin_of

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3
MULTI_MIN_COLS = 8          # kMultiMinCols: from that many columns on obhip_predict_multi_dev batches columns 1 ..
CASES = R.SHAPES + [R.WIDE]


def set_route(monkeypatch, generic):
    if generic:
        monkeypatch.setenv("OBHIP_FORCE_GENERIC", "1")
    else:
        monkeypatch.delenv("OBHIP_FORCE_GENERIC", raising=False)


def posterior_of(b):
    import design_ref as D
    import outerbase_amd as ob
    return ob.Posterior.from_hessian(b["om_d"], b["terms"], b["c"].H, D.SIGMA)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Dev:
    """the three C entries into padded buffers; the padding must come back untouched"""

    def __init__(self, post, c, theta=None, Z=None, x=None, skip=None):
        import torch
        from outerbase_amd.design import _dev_cols, _stream
        self.post, self.c, self.dev = post, c, _stream()
        self.p, self.S, self.m = c.p, c.S, c.m
        self.ldz = c.p + 2                                          # a leading dimension that is not p
        Zp = np.full((self.ldz, c.S), NAN)
        Zp[:c.p] = c.Z if Z is None else Z
        self.dz = torch.from_numpy(np.ascontiguousarray(Zp.T)).to(self.dev)
        self.dth = torch.from_numpy(np.ascontiguousarray(c.theta if theta is None else theta)).to(self.dev)
        self.dx = _dev_cols(c.x if x is None else x, self.dev)
        sk = c.skip if skip is None else skip
        self.dskip = torch.from_numpy(np.ascontiguousarray(sk, dtype=np.uint8)).to(self.dev) if np.any(sk) else None

    def draw(self):
        import torch
        from outerbase_amd._lib import call
        out = torch.full((self.p * self.S + PAD,), NAN, dtype=torch.float64, device=self.dev)
        call("obhip_posterior_draw_dev", self.post._h, self.dth.data_ptr(), self.dz.data_ptr(), self.ldz, self.S,
             out.data_ptr())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.all(np.isnan(out[self.p * self.S:])), "draw wrote beyond its end"
        return out[:self.p * self.S].reshape(self.S, self.p).T.copy()

    def sample(self):
        import torch
        from outerbase_amd._lib import call
        out = torch.full((self.m * self.S + PAD,), NAN, dtype=torch.float64, device=self.dev)
        call("obhip_posterior_sample_dev", self.post._h, self.dth.data_ptr(), self.dz.data_ptr(), self.ldz, self.S,
             self.dx.data_ptr(), self.m, out.data_ptr())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.all(np.isnan(out[self.m * self.S:])), "sample wrote beyond its end"
        return out[:self.m * self.S].reshape(self.S, self.m).T.copy()

    def extremum(self, maximize=False):
        import torch
        from outerbase_amd._lib import lib
        index = torch.full((self.S + PAD,), -7, dtype=torch.int64, device=self.dev)
        value = torch.full((self.S + PAD,), 7.5, dtype=torch.float64, device=self.dev)
        rc = lib.obhip_posterior_extremum_dev(self.post._h, self.dth.data_ptr(), self.dz.data_ptr(), self.ldz, self.S,
                                              self.dx.data_ptr(), self.m,
                                              None if self.dskip is None else self.dskip.data_ptr(), int(maximize),
                                              index.data_ptr(), value.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, lib.obhip_last_error()
        index, value = index.cpu().numpy(), value.cpu().numpy()
        assert np.all(index[self.S:] == -7) and np.all(value[self.S:] == 7.5), "extremum wrote beyond its end"
        return index[:self.S].copy(), value[:self.S].copy()

    def predict_multi(self, Theta):
        """obhip_predict_multi_dev on [Theta[:, 0], Theta, zero columns]: that entry gives column 0 to the
        single-response predictor and batches the rest from MULTI_MIN_COLS columns on -> its columns 1 .. S"""
        import torch
        from outerbase_amd._lib import call
        S = Theta.shape[1]
        ext = np.concatenate([Theta[:, :1], Theta, np.zeros((self.p, max(0, MULTI_MIN_COLS - S)))], axis=1)
        q = ext.shape[1]
        dT = torch.from_numpy(np.ascontiguousarray(ext.T)).to(self.dev)
        mean = torch.full((q * self.m,), NAN, dtype=torch.float64, device=self.dev)
        call("obhip_predict_multi_dev", self.post.om._h, self.post._t._h, dT.data_ptr(), q, self.dx.data_ptr(), self.m,
             mean.data_ptr(), None, 0.0, None)
        torch.cuda.synchronize()
        return mean.cpu().numpy().reshape(q, self.m).T[:, 1:S + 1].copy()


def own_extremum(path, elig, maximize):
    """min / argmin (first occurrence) of the device's own sample matrix over the eligible rows"""
    key = np.where(elig[:, None] & np.isfinite(path), -path if maximize else path, np.inf)
    idx = np.argmin(key, axis=0)
    none = ~np.isfinite(key[idx, np.arange(path.shape[1])])
    val = path[idx, np.arange(path.shape[1])]
    return np.where(none, -1, idx), np.where(none, NAN, val)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (bits(a) == bits(b))))


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("name,p,m,S,seed", CASES)
def test_draws_paths_and_optima_against_the_reference(name, p, m, S, seed, generic, monkeypatch):
    set_route(monkeypatch, generic)
    b = built(name, p, m, S, seed)
    c, Cc = b["c"], b["C"]
    label = "%s p=%d m=%d S=%d %s" % (name, c.p, m, S, "unfused" if generic else "fused")
    with posterior_of(b) as post:
        dev = Dev(post, c)
        Theta, path = dev.draw(), dev.sample()
        via_predictor = dev.predict_multi(Theta)
        imin, vmin = dev.extremum()
        imax, vmax = dev.extremum(maximize=True)
        if generic:                                                      # the two routes return the same indices
            set_route(monkeypatch, False)
            fmin, _ = dev.extremum()
            fmax, _ = dev.extremum(maximize=True)
            assert np.array_equal(fmin, imin) and np.array_equal(fmax, imax), label
    w = R.ratios(c, Theta, path, Cc)
    w["min"], w["max"] = R.value_ratio(c, imin, vmin, Cc), R.value_ratio(c, imax, vmax, Cc)
    line = "sample | %s: C %.3g (float64 restatement err/bound %.3g); device err/tolerance %s" % (
        label, Cc, b["r"], ", ".join("%s %.3g" % kv for kv in w.items()))
    print(line)
    # the entries against each other, bit for bit
    assert np.array_equal(bits(path), bits(via_predictor)), label + ": sample is not the predictor on draw's output"
    for mx, (i, v) in ((False, (imin, vmin)), (True, (imax, vmax))):
        oi, ov = own_extremum(path, c.elig, mx)
        assert np.array_equal(i, oi), label
        assert same_bits(v, ov), label
    # against the reference
    assert np.array_equal(imin, b["index"]) and np.array_equal(imax, b["index_max"]), label
    assert max(w.values()) < 1, line


def test_identity_normals_give_the_posterior_covariance_on_the_device():
    """Z = I at p = 67: (Theta - theta 1^T)(Theta - theta 1^T)^T = inv(H); the product is formed in long double
    from the device's draws, so that what is measured is the draws"""
    from test_sample_host import model
    import posterior_ref as P
    om_o, om_d, terms = model("d8", 67)
    p = len(terms)
    c = R.seeded_case(om_o, terms, 3, p, seed=7, Z=np.eye(p))
    Cc, r = R.constant_of(c)
    with posterior_of(dict(om_d=om_d, terms=terms, c=c)) as post:
        Theta = Dev(post, c).draw()
    rt = R.ratios(c, Theta, None, Cc)["theta"]
    Dm = np.asarray(Theta, dtype=E.ld) - np.asarray(c.theta, dtype=E.ld)[:, None]
    assert np.all(np.tril(E._f64(Dm), -1) == 0)                      # exactly: theta + 0 - theta
    W = P.inverse_ld(c.L)
    aX = np.abs(E._f64(W)).T
    bD = Cc * c.bTheta                                               # of every entry of Theta, hence of Dm
    rr = E.worst_ratio(Dm @ Dm.T, W.T @ W, bD @ aX.T + aX @ bD.T)
    print("sample | Z = I p=%d: C %.3g (err/bound %.3g); draws err/tolerance %.3g, D D^T against inv(H) %.3g" % (
        p, Cc, r, rt, rr))
    assert rt < 1 and rr < 1


@pytest.mark.parametrize("generic", [False, True])
def test_semantics(generic, monkeypatch):
    set_route(monkeypatch, generic)
    route = "unfused" if generic else "fused"
    base = built(*R.SEMANTICS)

    def run(b, maximize=False, **kw):
        with posterior_of(b) as post:
            return Dev(post, b["c"], **kw).extremum(maximize)

    def check(label, b, got):
        index, value = got
        assert np.array_equal(index, b["index"]), label
        r = R.value_ratio(b["c"], index, value, b["C"])
        print("sample | %s %s: value err/tolerance %.3g" % (label, route, r))
        assert r < 1, label
    # the best row of draw 0 twice, bit for bit, its copy in the other workgroup: the lower index wins
    t = built(*R.SEMANTICS, "twin")
    j = int(base["index"][0])
    lo, hi = sorted([j, twin_of(j)])
    assert t["index"][0] == lo and hi not in t["index"]
    check("twin rows", t, run(t))
    with posterior_of(t) as post:
        path = Dev(post, t["c"]).sample()
    assert np.array_equal(bits(path[lo]), bits(path[hi]))               # the twins tie in every draw
    # skip on every draw's winner: the reference's runner-up
    s = built(*R.SEMANTICS, "skip winners")
    assert not set(s["index"]) & set(base["index"])
    check("winners skipped", s, run(s))
    # a NaN coordinate in a winner: never picked, the others unchanged
    n = built(*R.SEMANTICS, "nan")
    got = run(n)
    check("nan row", n, got)
    keep = base["index"] != j
    assert j not in got[0] and np.array_equal(got[0][keep], base["index"][keep])
    # all rows skipped: -1 and NaN for every draw, and that is no error
    a = built(*R.SEMANTICS, "all skipped")
    index, value = run(a)
    assert np.all(index == -1) and np.all(np.isnan(value))
    # maximize with (theta, Z) is minimise with (-theta, -Z): the same indices, the values negated bit for bit
    c = base["c"]
    imax, vmax = run(base, maximize=True)
    imin, vmin = run(base, theta=-c.theta, Z=-c.Z)
    assert np.array_equal(imax, base["index_max"]) and np.array_equal(imin, imax)
    assert np.array_equal(bits(vmax), bits(-vmin))


def test_two_calls_return_the_same_bits():
    b = built(*R.SHAPES[7])                                             # d5, p = 130, m = 1000, S = 65
    with posterior_of(b) as post:
        dev = Dev(post, b["c"])
        one = (dev.draw(), dev.sample()) + dev.extremum() + dev.extremum(True)
        two = (dev.draw(), dev.sample()) + dev.extremum() + dev.extremum(True)
    for x, y in zip(one, two):
        assert np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y)


def test_refused_calls_change_nothing():
    import torch
    from outerbase_amd._lib import lib
    b = built(*R.SHAPES[1])                                             # d3, p = 5, m = 63, S = 15
    c = b["c"]
    with posterior_of(b) as post:
        dev = Dev(post, c)
        a = torch.full((c.m * c.S + 8,), NAN, dtype=torch.float64, device="cuda")
        i = torch.full((c.S + 8,), -7, dtype=torch.int64, device="cuda")
        h, th, z, x, A, I = post._h, dev.dth.data_ptr(), dev.dz.data_ptr(), dev.dx.data_ptr(), a.data_ptr(), i.data_ptr()
        err = lib.obhip_last_error
        assert lib.obhip_posterior_draw_dev(h, th, z, c.p - 1, c.S, A) == 1 and b"ldz < p" in err()
        assert lib.obhip_posterior_draw_dev(h, th, z, dev.ldz, 0, A) == 1 and b"S = 0" in err()
        assert lib.obhip_posterior_draw_dev(h, th, None, dev.ldz, c.S, A) == 1 and b"d_z" in err()
        assert lib.obhip_posterior_sample_dev(h, th, z, c.p - 1, c.S, x, c.m, A) == 1 and b"ldz < p" in err()
        assert lib.obhip_posterior_sample_dev(h, th, z, dev.ldz, 0, x, c.m, A) == 1 and b"S = 0" in err()
        assert lib.obhip_posterior_sample_dev(h, th, z, dev.ldz, c.S, x, c.m, None) == 1 and b"d_path" in err()
        assert lib.obhip_posterior_sample_dev(h, th, z, dev.ldz, c.S, None, 0, None) == 0          # n = 0: a no-op
        ext = lib.obhip_posterior_extremum_dev
        assert ext(h, th, z, c.p - 1, c.S, x, c.m, None, 0, I, A) == 1 and b"ldz < p" in err()
        assert ext(h, th, z, dev.ldz, 0, x, c.m, None, 0, I, A) == 1 and b"S = 0" in err()
        assert ext(h, th, z, dev.ldz, c.S, x, 0, None, 0, I, A) == 1 and b"m = 0" in err()
        assert ext(h, th, z, dev.ldz, c.S, x, c.m, None, 0, None, A) == 1 and b"outputs" in err()
        assert ext(h, th, z, dev.ldz, c.S, x, c.m, None, 0, I, None) == 1 and b"outputs" in err()
        torch.cuda.synchronize()
        assert bool(torch.isnan(a).all()) and bool((i == -7).all())


def test_python_methods():
    """thompson(z=) is the C entry; picks / counts are consistent with index; a seed reproduces; response=j
    de-standardises with meansd[j] on a posterior from NewtonAccumulator.posterior"""
    import math
    import outerbase_amd as ob
    from conftest import sample_x
    from test_sample_host import model
    b = built(*R.SEMANTICS)
    c = b["c"]
    with posterior_of(b) as post:
        iC, vC = Dev(post, c).extremum()
        res = post.thompson(c.x, c.theta, z=c.Z)
        assert np.array_equal(res.index, iC) and same_bits(res.value, vC)
        assert np.array_equal(post.draw(c.theta, z=c.Z), Dev(post, c).draw())
        assert np.array_equal(post.sample(c.x, c.theta, z=c.Z), Dev(post, c).sample())
        assert len(set(res.picks)) == len(res.picks) and res.counts.sum() == c.S
        seen = []
        for j in res.index:
            if j not in seen:
                seen.append(int(j))
        assert list(res.picks) == seen
        assert all(int(np.sum(res.index == j)) == n for j, n in zip(res.picks, res.counts))
        skip = np.zeros(c.m, dtype=bool)
        skip[res.picks] = True
        assert not set(post.thompson(c.x, c.theta, z=c.Z, skip=skip).picks) & set(res.picks)
        one, two = post.thompson(c.x, c.theta, n_draws=33, seed=4), post.thompson(c.x, c.theta, n_draws=33, seed=4)
        assert np.array_equal(one.index, two.index) and same_bits(one.value, two.value) and len(one.index) == 33
        assert np.array_equal(post.draw(c.theta, n_draws=5, seed=9), post.draw(c.theta, n_draws=5, seed=9))
        assert post.sample(c.x, c.theta, n_draws=5, seed=9).shape == (c.m, 5)
        assert post.thompson(c.x, c.theta, z=c.Z, response=0).value.shape == (c.S,)     # no meansd: standardised
    om_o, om_d, terms = model("d8", 67)
    rng = np.random.default_rng(43)
    x = sample_x(rng, 90, om_o.kinds)
    Y = rng.standard_normal((90, 2)) * np.array([1.0, 50.0]) + np.array([0.0, 7.0])
    xnew = sample_x(rng, 65, om_o.kinds)
    Z = rng.standard_normal((len(terms), 17))
    sigma, rho = math.log(0.1), 1.0
    with ob.NewtonAccumulator(om_d, terms, 2) as acc:
        acc.add(x, Y)
        fit = acc.fit(sigma, rho)
        theta = np.ascontiguousarray(fit.coeff[:, 1])
        with acc.posterior(sigma, rho) as post:
            cen, sca = post.meansd[1, 0], post.meansd[1, 1]
            raw, std = post.sample(xnew, theta, z=Z, response=1), post.sample(xnew, theta, z=Z)
            assert np.array_equal(raw, cen + sca * std)
            tr, ts = post.thompson(xnew, theta, z=Z, response=1), post.thompson(xnew, theta, z=Z)
            assert np.array_equal(tr.index, ts.index) and np.array_equal(tr.value, cen + sca * ts.value)
            assert sca > 10 and not np.array_equal(tr.value, ts.value)
