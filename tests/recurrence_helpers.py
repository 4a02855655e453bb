"""A numpy restatement of the Chebyshev recurrence (gspx_cheby_filter: analysis of a filter bank and synthesis by the
vector-coefficient Clenshaw recurrence of run_synthesis_batch), and the graphs, polynomials and synthesis inputs the
recurrence tests run.  scipy CSR and numpy only: nothing of the library takes part in run_recurrence() and
run_clenshaw().  Every operand is rounded to the compute dtype first and every step is computed in it."""
import numpy as np
from scipy import sparse

from oracle import cheby_oracle as orc


def scaled_operator(L, lmax, dtype):
    """F = (4 / lmax) L - 2 I, its spectrum in [-2, 2], rounded to `dtype`."""
    n = L.shape[0]
    F = (4.0 / float(lmax)) * sparse.csr_matrix(L, dtype=np.float64) - 2.0 * sparse.identity(n)
    return sparse.csr_matrix(F).astype(np.dtype(dtype))


def run_recurrence(L, lmax, coeffs, x, dtype=np.float64):
    """(a)  T_0 = x, T_1 = F/2 x, T_k = F T_{k-1} - T_{k-2};  y_f = c_f0 / 2 x + sum_k c_fk T_k x, one accumulator per
    filter.  coeffs (Nf, M), x (N, nsig): returns (Nf, N, nsig) in `dtype`."""
    dt = np.dtype(dtype)
    c = np.atleast_2d(np.asarray(coeffs, dtype=np.float64))
    c = np.concatenate([0.5 * c[:, :1], c[:, 1:]], axis=1).astype(dt)
    F = scaled_operator(L, lmax, dt)
    t_old = np.asarray(x).astype(dt)
    t_cur = (dt.type(0.5) * (F @ t_old)).astype(dt, copy=False)
    acc = [(cf[0] * t_old + cf[1] * t_cur).astype(dt, copy=False) for cf in c]
    for k in range(2, c.shape[1]):
        t_old, t_cur = t_cur, ((F @ t_cur) - t_old).astype(dt, copy=False)
        acc = [(a + cf[k] * t_cur).astype(dt, copy=False) for a, cf in zip(acc, c)]
    return np.stack(acc)


def run_clenshaw(L, lmax, coeffs, s, dtype=np.float64):
    """(b)  out = sum_f p_f(L) s_f with u_k = sum_f c'_fk s_f (c'_f0 halved):  b_K = u_K,  b_k = u_k + F b_{k+1} - b_{k+2},
    out = u_0 + F/2 b_1 - b_2.  coeffs (Nf, M), s (Nf, N, nsig): returns (N, nsig) in `dtype`."""
    dt = np.dtype(dtype)
    c = np.atleast_2d(np.asarray(coeffs, dtype=np.float64))
    c = np.concatenate([0.5 * c[:, :1], c[:, 1:]], axis=1).astype(dt)
    F = scaled_operator(L, lmax, dt)
    s = np.asarray(s).astype(dt)
    K = c.shape[1] - 1

    def u(k):
        out = c[0, k] * s[0]
        for f in range(1, c.shape[0]):
            out = out + c[f, k] * s[f]
        return out.astype(dt, copy=False)

    b1, b2 = u(K), None  # b_{k+1}, b_{k+2}
    for k in range(K - 1, 0, -1):
        new = u(k) + (F @ b1)
        if b2 is not None:
            new = new - b2
        b1, b2 = new.astype(dt, copy=False), b1
    out = u(0) + dt.type(0.5) * (F @ b1)
    if b2 is not None:
        out = out - b2
    return out.astype(dt, copy=False)


# ---- the polynomials ---------------------------------------------------------------------------------------------
HEAT_ORDERS = (1, 2, 3, 7, 30)
SINGLE = tuple("heat20/%d" % m for m in HEAT_ORDERS)


def POLYNOMIALS(lmax):
    """name -> (Nf, M) Chebyshev coefficients: Heat(20) at orders 1, 2, 3, 7 and 30 (an order-m filter has M = m + 1
    coefficients and runs K = m recurrence steps; order 2 is the call whose step 2 - the one that reads T_0 from the
    caller's panel when the input is fused - is also the last flush into y), the Mexican-hat bank of 3 filters at
    order 12 and the one of 2 filters at order 1."""
    polys = {"heat20/%d" % m: np.atleast_2d(orc.compute_cheby_coeff(orc.heat_kernel(20, lmax), lmax, m))
             for m in HEAT_ORDERS}
    polys["bank3"] = np.array([orc.compute_cheby_coeff(k, lmax, 12) for k in orc.mexican_hat_kernels(lmax, 3)])
    polys["bank2"] = np.array([orc.compute_cheby_coeff(k, lmax, 1) for k in orc.mexican_hat_kernels(lmax, 2)])
    return polys


def steps(coeffs):
    """K, the recurrence steps of a filter of M = K + 1 coefficients."""
    return np.atleast_2d(coeffs).shape[1] - 1


# ---- synthesis inputs --------------------------------------------------------------------------------------------
SHIFT = 7


def synthesis_inputs(x, nf):
    """(nf, N, W) input panels of a synthesis made from the W columns of x: panel f holds 2^-f times x's columns
    rotated by 7 f, so every panel differs, every value stays exact in float32, and the first w columns of the result
    depend on the first w columns of every panel only."""
    return np.stack([np.ldexp(np.roll(x, -SHIFT * f, axis=1), -f) for f in range(nf)])


def synthesis_reference(analysis):
    """The oracle's synthesis of synthesis_inputs(x, nf) from its analysis of x, (nf, N, W): the filters act on every
    column alone, so  sum_f p_f(L) s_f  is the same sum over the rotated, scaled columns of p_f(L) x."""
    return sum(np.ldexp(np.roll(a, -SHIFT * f, axis=1), -f) for f, a in enumerate(analysis))


# ---- the band graphs ---------------------------------------------------------------------------------------------
def band_weights(n=4097, reach=4, seed=41):
    """A ring of n vertices, each linked to its `reach` neighbours on either side, random symmetric weights in
    [0.1, 1]: a block of 64 rows gathers 64 + 2 reach distinct rows, so every block of its natural order is staged."""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), reach)
    j = (i + np.tile(np.arange(1, reach + 1), n)) % n
    A = sparse.coo_matrix((rng.uniform(0.1, 1.0, i.size), (i, j)), shape=(n, n)).tocsr()
    W = sparse.csr_matrix(A + A.T)
    W.sum_duplicates()
    W.sort_indices()
    return W


def shuffled(W, seed=42):
    """(W', perm): W with vertex i relabelled p[i] by a random permutation, and the internal order perm[new] = old
    that puts the band back (perm = p)."""
    n = W.shape[0]
    p = np.random.default_rng(seed).permutation(n).astype(np.int32)
    C = sparse.coo_matrix(W)
    Ws = sparse.csr_matrix((C.data, (p[C.row], p[C.col])), shape=(n, n))
    Ws.sum_duplicates()
    Ws.sort_indices()
    return Ws, p
