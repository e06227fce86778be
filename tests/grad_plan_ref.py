"""A float64 NumPy restatement of how the device forms the hyper-gradient products (csrc/kernels_grad.hip,
grad_views.cpp, kernels_grad_dense.hip, kernels_grad_d3.hip), the shapes that reach every plan and kernel
variant of that family, and the defects staged on the restatement (test_grad_plan_host.py proves that the
per-entry instrument of extended_ref.py sees each of them on those shapes; test_gpu_grad_plans.py runs the
shapes on the device).  Nothing of oracle/ob_oracle.py takes part here.

The decomposition, with l = the dimension of hyper-parameter h, o = the product of a term's OTHER level
factors, b = its level factor in l (1 at level 0) and ge_h = the gradient factor of h:

    dB[i, t, h] = s_i (ge_h[i, 0] o b  +  o delta_h),   delta_h = ge_h[i, t_l] - b ge_h[i, 0]   (t_l > 0)

a dense part every term has and a delta part of the terms that have the dimension.  The transposed
products sum the dense part per row tile of 64 and per row split (nsplit blocks of tps tiles, the partial
sums of the splits added at the end), the delta part per group of dimensions (build_d3_groups) with a
split of its own, and scatter the latter onto the former: squared, 2 u2 with u2 = sum_i w_i s_i^2 (o delta)(o b).

The factors are those of extended_ref.ExtendedRef rounded once to float64 -- what a float64 basis holds at
best -- so that every later operation is float64 and every difference from the long double products is
rounding of this scheme."""
import zlib

import numpy as np

import extended_ref as E

TILE = 64
MU_CAP = 152                   # columns of one k_tmm_d3 tile, the ones column included (build_d3_groups)
CUS = 256                      # compute units of an MI355X: the host tests' row splits (the device tests read theirs)


# ---- the shapes --------------------------------------------------------------------------------------
# name: kinds, knots per dimension, n, p (terms drawn: duplicates go), highest level, most factors per term, expectations:
#   plan; nu / pblocks / W / nh of the k_tmm_d3 groups (each a set over the groups); groups ">= k";
#   dense kernel, W2, passes as (h0, nh, NHB, N4); d3split / densesplit = (nsplit, tps); env
def _c(kinds, m, n, p, maxlev, max_nnz, **expect):
    return dict(kinds=kinds, m=m, n=n, p=p, maxlev=maxlev, max_nnz=max_nnz, expect=expect)


M25, POW, ANG = "mat25", "mat25pow", "mat25ang"
PLAN_KINDS = [M25, POW] * 5
CASES = {
    # NU = 2, one block along the terms: every W2 x NH of the fused pass
    "nu2 W4 nh1": _c([M25] * 6, 12, 130, 200, 4, 2, plan="Fused", nu={2}, W={4}, nh={1}, pblocks={1}, kernel="ge0_db", W2=1),
    "nu2 W6 nh1": _c([M25] * 6, 12, 130, 200, 4, 4, plan="Fused", nu={2}, W={6}, nh={1}, pblocks={1}, W2=2),
    "nu2 W8 nh1": _c([M25] * 6, 12, 130, 200, 4, 6, plan="Fused", nu={2}, W={8}, nh={1}, pblocks={1}, W2=3),
    "nu2 W4 nh2": _c([POW] * 6, 12, 130, 200, 4, 2, plan="Fused", nu={2}, W={4}, nh={2}, pblocks={1},
                     passes=[(0, 12, 1, 0)]),
    "nu2 W6 nh2": _c([POW] * 6, 12, 130, 200, 4, 4, plan="Fused", nu={2}, W={6}, nh={2}, pblocks={1}),
    "nu2 W8 nh2": _c([POW] * 6, 12, 130, 200, 4, 6, plan="Fused", nu={2}, W={8}, nh={2}, pblocks={1}),
    # NU = 4 (more than 1024 view-terms in a group), one block and two (more than 2048); n = 700: 11 row
    # tiles, the fused pass splits them 6 + 5 and the last tile has 60 rows
    "nu4 one block n700": _c([M25] * 6, 12, 700, 560, 4, 4, plan="Fused", nu={4}, pblocks={1}, nh={1},
                             d3split=(2, 6), densesplit=(11, 1), passes=[(0, 6, 0, 2)]),
    "nu4 two blocks n700": _c([M25] * 6, 12, 700, 860, 4, 5, plan="Fused", nu={4}, pblocks={2}, nh={1},
                              d3split=(2, 6), densesplit=(11, 1)),
    "nu4 two blocks nh2": _c([POW] * 6, 12, 300, 860, 4, 5, plan="Fused", nu={4}, pblocks={2}, nh={2},
                             d3split=(1, 5)),
    # ... and the narrowest and the widest column lists with NU = 4, one and two delta columns (more than
    # 1024 view-terms of two factors within 151 columns: nearly all 630 such terms of 12 dimensions at 3 levels)
    "nu4 W4 nh1": _c([M25] * 12, 12, 130, 6000, 3, 2, plan="Fused", nu={4}, W={4}, nh={1}),
    "nu4 W8 nh1": _c([M25] * 6, 12, 130, 400, 4, 6, plan="Fused", nu={4}, W={8}, nh={1}),
    "nu4 W6 nh2": _c([POW] * 6, 12, 130, 500, 4, 4, plan="Fused", nu={4}, W={6}, nh={2}),
    "nu4 W4 nh2": _c([POW] * 12, 12, 130, 6000, 3, 2, plan="Fused", nu={4}, W={4}, nh={2}),
    "nu4 W8 nh2": _c([POW] * 6, 12, 130, 400, 4, 6, plan="Fused", nu={4}, W={8}, nh={2}),
    # whole waves beyond p_pad under the 1024 view-terms of a block: p_pad = 256 and 512
    "dead waves p_pad 256": _c([M25] * 6, 12, 65, 40, 4, 4, plan="Fused", nu={2}, p_pad={256}, d3split=(1, 2)),
    "dead waves p_pad 512": _c([M25] * 6, 12, 65, 100, 4, 6, plan="Fused", nu={2}, p_pad={512}),
    # rows: one row, one full tile, a tile and one row
    "n1 nh1": _c([M25] * 6, 12, 1, 100, 4, 4, plan="Fused", d3split=(1, 1), densesplit=(1, 1)),
    "n64 nh1": _c([M25] * 6, 12, 64, 100, 4, 4, plan="Fused", d3split=(1, 1), densesplit=(1, 1)),
    "n65 nh2": _c([POW] * 6, 12, 65, 100, 4, 4, plan="Fused", d3split=(1, 2), densesplit=(2, 1)),
    "n1 nh2": _c([POW] * 6, 12, 1, 100, 4, 4, plan="Fused", d3split=(1, 1)),
    # groups: a change of nh closes one, and so does a union of more than 151 columns
    "group closes on nh": _c([M25, POW, M25, ANG], 12, 130, 200, 4, 3, plan="Fused", nhseq=[1, 2, 1, 2]),
    "group closes on columns": _c([M25] * 8, 12, 130, 300, 8, 3, plan="Fused", groups=2, nh={1}),
    # one view of more than 151 columns (every term has dimension 1, so its view meets all columns of the
    # others): the restricted views with no switch set; and with 161 used columns two tiles no longer fit
    # the LDS: the dense kernel with one tile and 16 waves (138 to 275 used columns)
    "ge0views d20": _c([M25] * 20, 12, 200, 400, 8, 3, plan="Ge0Views", ngroups=0, kernel="ge0_16", Mu_range=(138, 275),
                       passes=[(0, 16, 1, 0), (16, 4, 1, 0)], fallback=0, all_have_first=True),
    # the dense pass' blocks of hyper-parameters
    "dense nhyp3": _c([M25] * 3, 12, 200, 100, 4, 3, plan="Fused", kernel="ge0_db", passes=[(0, 3, 0, 1)]),
    "dense nhyp18 W2=3": _c([M25] * 18, 12, 200, 300, 3, 6, plan="Fused", kernel="ge0_db", W2=3, passes=[(0, 18, 1, 1)]),
    "dense nhyp22 W2=4": _c([M25] * 22, 12, 200, 300, 3, 7, plan="Fused", kernel="ge0_db", W2=4, passes=[(0, 22, 1, 2)]),
    "dense nhyp26": _c([M25] * 18 + [POW, ANG, POW, ANG], 12, 200, 260, 3, 3, plan="Fused", kernel="ge0_db",
                       passes=[(0, 16, 1, 0), (16, 10, 1, 0)]),
    "dense nhyp36": _c([POW] * 18, 12, 200, 300, 3, 3, plan="Fused", kernel="ge0_db",
                       passes=[(0, 16, 1, 0), (16, 20, 1, 1)]),
    # 130 to 137 used columns and 22 hyper-parameters: two tiles of 16 + 8 gradient columns no longer fit,
    # the groups of four fall back to a pass of their own
    "dense fall-back n4 -> 0": _c([M25] * 22, 12, 200, 300, 6, 3, kernel="ge0_db", Mu_range=(130, 137),
                                  passes=[(0, 16, 1, 0), (16, 6, 0, 2)]),
    # the four plans (PLANS of test_gpu_grad_fused.py): "wide" has a term of nine factors
    "plan fused": _c(PLAN_KINDS, 10, 333, 120, 4, 5, plan="Fused"),
    "plan ge0_views": _c(PLAN_KINDS, 10, 333, 120, 4, 5, plan="Ge0Views", env={"OBHIP_GRAD_D3": "0"}, ngroups=0),
    "plan bmat_views": _c(PLAN_KINDS, 10, 333, 120, 3, 9, plan="BmatViews", kernel="bt_times_u", wide=True),
    "plan full_views": _c(PLAN_KINDS, 10, 333, 120, 3, 9, plan="FullViews", env={"OBHIP_GRAM_CHUNK_ROWS": "128"},
                          wide=True),
}
SEED = {name: zlib.crc32(name.encode()) for name in CASES}      # (by name: a new case moves no other case's inputs)


def case_terms(name, random_terms):
    """the case's terms from the suite's random_terms, duplicates removed; "wide": one term of nine factors"""
    c = CASES[name]
    rng = np.random.default_rng(SEED[name])
    terms = random_terms(rng, c["p"], len(c["kinds"]), c["maxlev"], c["max_nnz"])
    if c["expect"].get("all_have_first"):
        terms[1:, 0] = rng.integers(1, c["maxlev"] + 1, size=c["p"] - 1)
    if c["expect"].get("wide"):
        terms[1, :] = 0
        terms[1, :9] = 1
    return np.unique(terms, axis=0)


# ---- the grouping of build_d3_groups, restated ---------------------------------------------------------
def d3_groups(terms, numhyp, mu_cap=MU_CAP):
    """[{nh, members: [(dimension, first hyper-parameter)], off, W, Mu, p}] or None where a view does not fit.
    numhyp: hyper-parameters per dimension.  A member is a dimension's (up to) two hyper-parameters and the
    terms that have the dimension; its columns are the level columns of the other factors, its own level
    columns (staged apart) and one delta column per hyper-parameter and level."""
    terms = np.asarray(terms, dtype=np.int64)
    d = terms.shape[1]
    hypst = np.concatenate([[0], np.cumsum(numhyp)])
    mem = []
    for l in range(d):
        for h0 in range(int(hypst[l]), int(hypst[l + 1]), 2):
            nh = min(2, int(hypst[l + 1]) - h0)
            ix = np.nonzero(terms[:, l] > 0)[0]
            if len(ix) == 0:
                continue
            cols, maxw = set(), 0
            for k in ix:
                w = 1 + nh
                for q in range(d):
                    lv = int(terms[k, q])
                    if lv == 0:
                        continue
                    if q == l:
                        cols.add(("own", q, lv))
                        cols.update(("delta", h0 + j, lv) for j in range(nh))
                    else:
                        cols.add(("value", q, lv))
                        w += 1
                maxw = max(maxw, w)
            if len(cols) + 1 > mu_cap or maxw > 8:
                return None
            mem.append(dict(l=l, h0=h0, nh=nh, cols=cols, maxw=maxw, ix=ix))
    groups, i = [], 0
    while i < len(mem):
        used, maxw, j = set(mem[i]["cols"]), mem[i]["maxw"], i + 1
        while j < len(mem) and mem[j]["nh"] == mem[i]["nh"]:
            both = used | mem[j]["cols"]
            if len(both) + 1 > mu_cap:
                break
            used, maxw, j = both, max(maxw, mem[j]["maxw"]), j + 1
        off = np.concatenate([[0], np.cumsum([len(q["ix"]) for q in mem[i:j]])])
        groups.append(dict(nh=mem[i]["nh"], members=[(q["l"], q["h0"]) for q in mem[i:j]], off=off,
                           W=max(4, (maxw + 1) // 2 * 2), Mu=len(used) + 1, p=int(off[-1])))
        i = j
    return groups


def split_rows(ntiles, want, min_tiles=1):
    """(nsplit, tps) of csrc/launch_plan.h"""
    cap = max(1, ntiles // min_tiles)
    nsplit = min(max(1, want), cap)
    tps = (ntiles + nsplit - 1) // nsplit
    return (ntiles + tps - 1) // tps, tps


def d3_geometry(group, n, cus=CUS):
    p_pad = (group["p"] + 255) // 256 * 256
    nu = 4 if p_pad > 1024 else 2
    tpb = 8 * nu * 64
    pblocks = (p_pad + tpb - 1) // tpb
    nsplit, tps = split_rows((n + TILE - 1) // TILE, cus * 2 // pblocks, 4)
    return dict(p_pad=p_pad, nu=nu, pblocks=pblocks, nsplit=nsplit, tps=tps)


def dense_geometry(p, n, cus=CUS):
    """of k_tmm_ge0_db: 1024 terms per block, one block per compute unit"""
    pblocks = ((p + 255) // 256 * 256 + 1023) // 1024
    return split_rows((n + TILE - 1) // TILE, cus // pblocks)


# ---- the factors in float64 ----------------------------------------------------------------------------
class Factors:
    """s (n), r[k] (n x m_k, column 0 = 1), g[h] (n x m_k) of an ExtendedRef, each rounded once to float64"""

    def __init__(self, ref):
        f = lambda a: np.asarray(a, dtype=np.float64)
        self.n, self.d, self.nhyp = ref.n, ref.d, ref.nhyp
        self.hypmatch = [int(l) for l in ref.hypmatch]
        self.r = [f(r) for r in ref.r]
        for r in self.r:
            r[:, 0] = 1.0
        self.g = [f(g) for g in ref.g]
        self.s = f(ref._scale()[0])

    def others(self, terms, skip=None, drop_last_of=None):
        """o: the product of the level factors of every term (n x p), dimension `skip` left out;
        drop_last_of: a term index whose last factor is left out too (a staged defect)"""
        P = np.ones((self.n, len(terms)))
        for k in range(self.d):
            if k == skip:
                continue
            lev = terms[:, k].copy()
            if drop_last_of is not None and k == max(q for q in range(self.d) if q != skip and terms[drop_last_of, q] > 0):
                lev[drop_last_of] = 0
            P *= self.r[k][:, lev]
        return P


def _split_sum(X, w, nsplit, tps, drop=None, ragged_weight=None):
    """sum_i w_i X[i, :] as the device adds it up: per row tile, the tiles of a split one after the other,
    the splits at the end.  drop: a split whose partial sum is left out; ragged_weight: the weights the
    rows of the last tile take where that tile is not full (both staged defects)"""
    n = X.shape[0]
    ntiles = (n + TILE - 1) // TILE
    out = np.zeros(X.shape[1:])
    for r in range(nsplit):
        part = np.zeros(X.shape[1:])
        for tile in range(r * tps, min(ntiles, (r + 1) * tps)):
            sl = slice(tile * TILE, min(n, (tile + 1) * TILE))
            ww = w[sl]
            if ragged_weight is not None and tile == ntiles - 1 and n % TILE:
                ww = ragged_weight[sl]
            part += np.tensordot(ww, X[sl], axes=(0, 0))
        if r != drop:
            out += part
    return out


def fused_tmm(F, terms, groups, w, squared, dense_split, d3_splits, defect=None):
    """sum_i w_i dB[i, t, h] (squared: of B^2), p x nhyp, by the fused plan: the dense part of every term
    and the groups' delta parts scattered onto it.  dense_split and d3_splits[g]: (nsplit, tps).
    defect: None or (kind, ...) -- see DEFECTS."""
    terms = np.asarray(terms, dtype=np.int64)
    kind = defect[0] if defect else None
    p, nh_all = len(terms), F.nhyp
    P = F.others(terms)
    s1 = F.s * F.s if squared else F.s
    X = P * P if squared else P
    out = np.empty((p, nh_all))
    for h in range(nh_all):                                   # the dense part: ge_h[0] B for every term
        ge0 = F.g[h][:, 0] * (2.0 if squared else 1.0)
        out[:, h] = _split_sum(X, w * s1 * ge0, *dense_split)
    prev = None
    for gi, (grp, split) in enumerate(zip(groups, d3_splits)):
        nh = grp["nh"]
        here = kind is not None and defect[1] == gi
        u = np.zeros((nh, grp["p"]))
        index = np.zeros(grp["p"], dtype=np.int64)
        nz = np.zeros(grp["p"], dtype=np.int64)
        for j, (l, h0) in enumerate(grp["members"]):
            ix = np.nonzero(terms[:, l] > 0)[0]
            sl = slice(int(grp["off"][j]), int(grp["off"][j + 1]))
            index[sl] = ix
            nz[sl] = (terms[ix] > 0).sum(1) + nh
        order = np.argsort(-nz, kind="stable")               # sperm: by falling number of column slots
        longest = None
        if here and kind == "half variant":                   # units 2 and 3 of the first wave of block 0
            run0 = 2 * 64
            longest = int(order[run0 + int(np.argmax(nz[order[run0:run0 + 128]]))])
        for j, (l, h0) in enumerate(grp["members"]):
            ix = np.nonzero(terms[:, l] > 0)[0]
            sl = slice(int(grp["off"][j]), int(grp["off"][j + 1]))
            drop_last = None
            if longest is not None and sl.start <= longest < sl.stop:
                drop_last = longest - sl.start
            o = F.others(terms[ix], skip=l, drop_last_of=drop_last)
            ll, hh0 = l, h0
            if here and kind == "previous table" and j == defect[2]:
                ll, hh0 = prev                                # the own and delta columns of another member
            lev = np.minimum(terms[ix, l], F.r[ll].shape[1] - 1)
            b = F.r[ll][:, lev]
            for q in range(nh):
                delta = F.g[hh0 + q][:, lev] - b * F.g[hh0 + q][:, 0:1]
                drop = defect[3] if here and kind == "drop split" and (j, q) == tuple(defect[2]) else None
                if squared:
                    ragged = np.ones(F.n) * s1 if here and kind == "ragged w2" else None
                    val = _split_sum((o * delta) * (o * b), w * s1, *split, drop=drop, ragged_weight=ragged)
                    if not (here and kind == "no factor 2" and j == defect[2]):
                        val = 2.0 * val
                else:
                    val = _split_sum(o * delta, w * F.s, *split, drop=drop)
                u[q, sl] = val
            if here and kind == "swap pair" and j == defect[2]:
                u[[0, 1], sl] = u[[1, 0], sl]
        if here and kind == "wrong block":                    # runs of 64 sorted view-terms: run a's sums land on run b's
            a, b2 = order[defect[2] * 64:defect[2] * 64 + 64], order[defect[3] * 64:defect[3] * 64 + 64]
            m = min(len(a), len(b2))
            u[:, a[:m]], u[:, b2[:m]] = u[:, b2[:m]].copy(), u[:, a[:m]].copy()
        for j, (l, h0) in enumerate(grp["members"]):
            sl = slice(int(grp["off"][j]), int(grp["off"][j + 1]))
            for q in range(nh):
                out[index[sl], h0 + q] += u[q, sl]
        prev = grp["members"][-1]
    if kind == "slice":
        _, t0, h = defect
        out[t0:t0 + 64, h] *= 1.0 + 1e-9
    return out


def fused_mm(F, terms, a, squared):
    """sum_t a_t dB[i, t, h] (squared: of B^2), n x nhyp: ge_h[0] (B a) and the delta part of the terms that have
    the dimension (mm_gradhyp_dev)"""
    terms = np.asarray(terms, dtype=np.int64)
    P = F.others(terms)
    s1 = F.s * F.s if squared else F.s
    M = ((P * P if squared else P) @ a) * s1
    out = np.empty((F.n, F.nhyp))
    for h in range(F.nhyp):
        l = F.hypmatch[h]
        ix = np.nonzero(terms[:, l] > 0)[0]
        o = F.others(terms[ix], skip=l)
        b = F.r[l][:, terms[ix, l]]
        delta = F.g[h][:, terms[ix, l]] - b * F.g[h][:, 0:1]
        if squared:
            out[:, h] = 2.0 * (F.g[h][:, 0] * M + s1 * (((o * delta) * (o * b)) @ a[ix]))
        else:
            out[:, h] = F.g[h][:, 0] * M + s1 * ((o * delta) @ a[ix])
    return out


# the defects staged on fused_tmm and the shape each is staged on; the arguments are filled in by
# test_grad_plan_host.py from the case's groups
DEFECTS = {
    "one row split's partial left out of the reduce": ("drop split", "nu4 one block n700"),
    "the last, ragged tile taken with w2 = 1": ("ragged w2", "nu4 one block n700"),
    "the two hyper-parameters of an NH = 2 member swapped": ("swap pair", "nu4 two blocks nh2"),
    "a run of 64 view-terms scattered to the other block's": ("wrong block", "nu4 two blocks n700"),
    "the factor 2 missing on u2 for one member": ("no factor 2", "nu4 two blocks nh2"),
    "the second half-run on the first half's variant": ("half variant", "nu4 one block n700"),
    "a member's columns from the previous group's table": ("previous table", "group closes on columns"),
    "a 64 x 1 slice scaled by 1 + 1e-9": ("slice", "nu4 two blocks n700"),
}
