"""Every product of one design matrix on the device: `device_products`, used in-process by
tests/test_gpu_extended.py, and as a child process where a kernel generation is chosen by an
environment switch that the library reads once per process (OBHIP_MM_LANE_ROW, OBHIP_TMM_LANE_ROW,
OBHIP_PREDICT_LANE_ROW: the first-generation lane = row kernels).
usage: extended_products_worker.py <inputs.npz> <outputs.npz>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_products(om_d, terms, x, a, v, cv, sig, levelcap=None):
    """getbase of every dimension, getmat, B a, B^T v, their squared forms, sqcolsums and the fused
    predictor's mean and variance (obhip_predict), as float64 arrays by name"""
    import outerbase_amd as ob
    from outerbase_amd._lib import call, ptr
    n = x.shape[0]
    bd = ob.outerbase(om_d, x, levelcap=levelcap)
    out = {"getbase%d" % k: bd.getbase(k + 1) for k in range(om_d.d)}
    tt = ob.obmod._Terms(om_d, terms)
    out["getmat"] = bd.getmat(tt)
    out["matmul"] = bd.matmul(tt, a)
    out["tmatmul"] = bd.tmatmul(tt, v)
    out["sqmm"] = bd.sqmm(tt, np.abs(a))
    out["sqtmm"] = bd.sqtmm(tt, v)
    out["sqcolsums"] = bd.sqcolsums(tt)
    mean, var, mean_only = np.empty(n), np.empty(n), np.empty(n)
    xf = np.asfortranarray(x)
    # (the predictor builds its own basis at the rows: every level the terms use)
    call("obhip_predict", om_d._h, tt._h, ptr(a), ptr(xf), n, n, ptr(mean), ptr(cv), sig, ptr(var))
    call("obhip_predict", om_d._h, tt._h, ptr(a), ptr(xf), n, n, ptr(mean_only), None, sig, None)
    out.update(predict_mean=mean, predict_var=var, predict_mean_only=mean_only)
    return out


def main():
    import outerbase_amd as ob
    f = np.load(sys.argv[1])
    kinds = str(f["kinds"]).split(",")
    st = f["knotptst"]
    om = ob.outermod()
    ob.setcovfs(om, kinds)
    om.updatehyp(f["hyp"])
    ob.setknot(om, [f["knotpt"][st[k]:st[k + 1]] for k in range(len(kinds))])
    om.set_rotation(f["rotmat"], f["basisvar"], f["maxlevel"])
    assert np.array_equal(om.rotation()[0], f["rotmat"]) and np.array_equal(ob.gethyp(om), f["hyp"])
    out = device_products(om, f["terms"], f["x"], f["a"], f["v"], f["cv"], float(f["sig"]))
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
