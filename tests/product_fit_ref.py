"""Host reference of the Newton fit on gridded data (obhip_normal_acc_add_product_dev): a long-double statement of
the accumulator's state -- triangle, B^T (Y - c), B^T 1 -- on the EXPANDED rows (product_ref.expand: row
i nb + j is the pair (xa[i], xb[j])), NumPy only, through extended_ref.ExtendedRef.

Tolerances are extended_ref's own rule, _sum_tol(C, bound, k, absum) = C x (propagated bound) + gamma_k x (sum of
|summands|), with C from the float64 oracle's ratio on the case as product_ref derives it.  What differs from the
row route is k.  The device never adds na nb summands: with At = diag(sA) U, Bt = diag(sB) V it forms

    G_kl = (sum_i At_ik At_il) (sum_j Bt_jk Bt_jl),   b1_k = (sum_i At_ik) (sum_j Bt_jk),
    R_k  = sum_i At_ik (sum_j (Y - c)_ij Bt_jk).

The absolute sum of the expanded summands is the product of the two sides' absolute sums (every summand is a
product of an A part and a B part, |a b| = |a| |b|), so the relative errors of the two nested sums add:
gamma_na + gamma_nb <= gamma_{na + nb} to first order, whatever order, chunking or matrix-core accumulation each
sum is taken in.  On top come, per summand, the roundings that the reference's entry B_(ij)k does not have:

  * the device multiplies the factors of an entry in another order (each side's product first, its scale last):
    2 d + 2 per design-matrix entry, as product_ref.py counts them for the predictor;
  * a triangle entry multiplies TWO design-matrix entries: 2 (2 d + 2); then the product of the two Grams and the
    addition of the fold: + 2;
  * an entry of R or b1 holds one design-matrix entry: 2 d + 2; then the product of the two sums (b1) or the
    multiplication by At in the final dot (R), and the fold: + 2.

So k = na + nb + extra with extra = 4 d + 6 (triangle) and 2 d + 4 (R, b1): far below the rows' k = na nb.  Batches
that were added, removed or merged add one to `extra` each, as test_gpu_stream.py counts them.
"""
import numpy as np

import extended_ref as E
import product_ref as P

ld = np.longdouble
MAX_PAIRS = 20000        # the long-double Gram on the expanded rows takes seconds below this


def extra_gram(d):
    return 2 * (2 * d + 2) + 2


def extra_vec(d):
    return (2 * d + 2) + 2


class ProductFitRef:
    """m: a model dict as test_gpu_extended.model returns it.  B, bB: the expanded rows' long-double design
    matrix and its bound, C: the case's constant."""

    def __init__(self, m, xa, xb, dims_b, seed=0):
        assert len(xa) * len(xb) <= MAX_PAIRS
        ref = P.ProductRef(m, xa, xb, dims_b, seed)
        self.na, self.nb, self.d, self.p = ref.na, ref.nb, ref.d, ref.p
        self.x = ref.x       # the expanded rows
        self.B, self.bB, self.C, self.ratio = ref.B, ref.bB, ref.C, ref.ratio
        self.k = self.na + self.nb
        self._Bf = np.abs(E._f64(self.B))

    def flat(self, Y):
        """Y (na, nb) -> the expanded rows' order"""
        return np.asarray(Y).reshape(self.na * self.nb)

    def gram_parts(self, cols, rows=None):
        """(want, bound, absum) of G[cols, :] over the expanded rows `rows` (None: all)"""
        B, bB, Bf = (self.B, self.bB, self._Bf) if rows is None else (self.B[rows], self.bB[rows], self._Bf[rows])
        return B[:, cols].T @ B, E.gram_bound(B, bB, cols), Bf[:, cols].T @ Bf

    def gram(self, cols, extra=0):
        want, bound, absum = self.gram_parts(cols)
        return want, E._sum_tol(self.C, bound, self.k + extra_gram(self.d) + extra, absum)

    def tm_parts(self, v, rows=None):
        """(want, bound, absum) of B^T v over the expanded rows"""
        B, bB, Bf = (self.B, self.bB, self._Bf) if rows is None else (self.B[rows], self.bB[rows], self._Bf[rows])
        v = np.asarray(v, dtype=ld)
        av = np.abs(E._f64(v))
        return B.T @ v, E._f64(bB).T @ av, Bf.T @ av

    def tmatmul(self, v, extra=0):
        want, bound, absum = self.tm_parts(v)
        return want, E._sum_tol(self.C, bound, self.k + extra_vec(self.d) + extra, absum)


def side_ref(m, xs, side, C):
    """(want, tol), n x p: one side matrix, s_i prod of the term's factors over the dimensions `side` at the rows
    xs (n x |side|, the side's columns in the order of `side`), in long double.  One entry is one product of at
    most 2 |side| factors (a scale and a level factor per dimension): the rule with a single summand, k = the
    2 |side| roundings of the float64 product."""
    d, terms = len(m["kinds"]), np.asarray(m["terms"], dtype=np.int64)
    x = np.full((len(xs), d), 0.5)
    x[:, list(side)] = xs
    ref = E.ExtendedRef(m["kinds"], m["knots"], m["hyp"], m["rot"], x)
    n, p = len(xs), len(terms)
    P0, S0 = np.ones(n, dtype=ld), np.zeros(n, dtype=ld)
    for l in side:
        P0, S0 = ref._times(P0, S0, ref.s[l], ref.bs[l])
    Pm, Sm = np.repeat(P0[:, None], p, axis=1), np.repeat(S0[:, None], p, axis=1)
    for l in side:
        idx = np.nonzero(terms[:, l] > 0)[0]
        if len(idx):
            lev = terms[idx, l]
            Pm[:, idx], Sm[:, idx] = ref._times(Pm[:, idx], Sm[:, idx], ref.r[l][:, lev], ref.br[l][:, lev])
    return Pm, E._sum_tol(C, Sm, 2 * len(side), np.abs(E._f64(Pm)))


def device_algebra(At, Bt, V, drop_scale_tile=None, scale_a=None, skip_chunk=None, chunk=64):
    """The separated normal equations in float64 NumPy from the two side matrices (na x p, nb x p) and the
    shifted responses V (na x nb): (G, R, b1).  Mutations for the host test: drop_scale_tile = t forms the A
    side's Gram with the row scale scale_a missing in the 64-row tile t; skip_chunk = (c, k) leaves the chunk c
    of `chunk` rows of xb out of R[k]."""
    A_for_gram = At
    if drop_scale_tile is not None:
        A_for_gram = At.copy()
        r = slice(64 * drop_scale_tile, 64 * drop_scale_tile + 64)
        A_for_gram[r] = At[r] / scale_a[r, None]
    G = (A_for_gram.T @ A_for_gram) * (Bt.T @ Bt)
    b1 = At.sum(0) * Bt.sum(0)
    W2 = V @ Bt
    if skip_chunk is not None:
        c, k = skip_chunk
        rows = slice(chunk * c, chunk * c + chunk)
        W2 = W2.copy()
        W2[:, k] -= V[:, rows] @ Bt[rows, k]
    R = (At * W2).sum(0)
    return G, R, b1
