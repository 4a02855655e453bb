"""A numpy restatement of a polynomial program (gspx_poly_program: the product form's and the Newton form's steps) and
the polynomials the program tests run, chosen for the step shapes their product forms have.  scipy CSR and numpy only:
nothing of the library takes part in run_program()."""
import numpy as np
from numpy.polynomial import chebyshev as npcheb
from numpy.polynomial import polynomial as nppoly
from scipy import sparse

from oracle import cheby_oracle as orc


def run_program(L, lmax, prog, x, old_is_x=False, dtype=np.float64):
    """h_0 = x;  h_{s+1} = scale_s F h_s + beta_s h_s + gamma_s o_s,  F = (4 / lmax) L - 2 I;  returns h_S.
    o_s = x for every step (old_is_x: the Newton form), else o_s = h_{s-1} and gamma_0 is ignored (the product form).
    Every operand is rounded to `dtype` first and every step is computed in it."""
    dt = np.dtype(dtype)
    prog = np.asarray(prog, dtype=np.float64).reshape(-1, 3)
    n = L.shape[0]
    F = sparse.csr_matrix((4.0 / float(lmax)) * sparse.csr_matrix(L, dtype=np.float64) - 2.0 * sparse.identity(n)).astype(dt)
    x = np.asarray(x).astype(dt)
    h, prev = x, None
    for s, (scale, beta, gamma) in enumerate(prog.astype(dt)):
        old = x if old_is_x else prev
        new = scale * (F @ h) + beta * h
        if old is not None and (old_is_x or s > 0) and gamma != 0:
            new = new + gamma * old
        prev, h = h, new.astype(dt, copy=False)
    return h


PAIRS3 = ((0.3, 0.5), (-0.6, 0.2), (0.0, 1.1))
REAL7 = (-0.9, -0.3, 0.2, 0.7, 1.4, -1.7, 0.05)


def _cheb_of_power(p):
    """Chebyshev coefficients, in the convention p(t) = c_0 / 2 + sum_k c_k T_k(t), of a power-basis polynomial."""
    c = npcheb.poly2cheb(p)
    c[0] *= 2
    return np.ascontiguousarray(c, dtype=np.float64)


def POLYNOMIALS(lmax):
    """name -> Chebyshev coefficients.  The heat polynomials approximate exp(-scale l / lmax) on [0, lmax]; the others
    are built from their roots in t = (2 / lmax) l - 1 and do not depend on lmax.  Their product forms' step shapes
    (steps, two-pass, three-pass, whether the first factor is a pair, kind of the last step) are SHAPES below."""
    heat = lambda scale, order: orc.compute_cheby_coeff(orc.heat_kernel(scale, lmax), lmax, order)  # noqa: E731
    real7 = npcheb.chebfromroots(list(REAL7))
    real7[0] *= 2
    pairs = np.array([1.0])
    for a, b in PAIRS3:
        pairs = nppoly.polymul(pairs, [a * a + b * b, -2 * a, 1.0])
    return {
        "heat5/1": heat(5, 1),
        "heat5/2": heat(5, 2),
        "heat5/3": heat(5, 3),
        "heat7/25": heat(7, 25),
        "heat40/30": heat(40, 30),
        "real7": np.ascontiguousarray(real7, dtype=np.float64),
        "pairs3": _cheb_of_power(pairs),
        "pairs3+real": _cheb_of_power(nppoly.polymul(pairs, [-0.4, 1.0])),
    }


# name -> (S in float64, two-pass steps, three-pass steps, first factor a pair, the last step is three-pass)
SHAPES = {
    "heat5/1": (1, 1, 0, False, False),
    "heat5/2": (2, 2, 0, False, False),
    "heat5/3": (3, 2, 1, False, True),
    "heat7/25": (18, 9, 9, True, True),
    "heat40/30": (30, 22, 8, True, False),
    "real7": (7, 7, 0, False, False),
    "pairs3": (6, 3, 3, True, True),
    "pairs3+real": (7, 4, 3, True, True),
}


def program_shape(prog):
    """(S, two-pass steps, three-pass steps, first factor a pair, last step three-pass) of a product-form program."""
    prog = np.asarray(prog).reshape(-1, 3)
    three = prog[:, 2] != 0
    three[0] = False  # gamma_0 is ignored
    S = prog.shape[0]
    return (S, int(S - three.sum()), int(three.sum()), bool(S > 1 and three[1]), bool(three[-1]))

# float32 trims heat7/25's converged tail (filters.PRODUCT_TRIM): four steps fewer, the same kinds of steps
SHAPES_F32 = dict(SHAPES, **{"heat7/25": (14, 7, 7, True, True)})


def shapes_for(dtype):
    return SHAPES if np.dtype(dtype) == np.float64 else SHAPES_F32


# the three small random graphs of the program tests: name -> (vertices, arguments of gpu_helpers.random_graph)
RANDOM_GRAPHS = {
    "hub3001": (3001, dict(avg_deg=9, seed=611, hub=True, isolated=4)),
    "rand577": (577, dict(avg_deg=9, seed=612, isolated=4)),
    "rand65": (65, dict(avg_deg=9, seed=613)),
}


def random_case(name, lap_type):
    """(W, L, lmax) of one of RANDOM_GRAPHS: lmax an upper bound of the spectrum (twice the largest degree, or 2)."""
    from gpu_helpers import random_graph, upper_lmax
    n, kw = RANDOM_GRAPHS[name]
    W = random_graph(n, **kw)
    return W, orc.laplacian(W, lap_type), (upper_lmax(W) if lap_type == "combinatorial" else 2.0)
