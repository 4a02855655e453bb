"""pygsp.filters surface for the Chebyshev path, backed by libgspx.

Mirrors (names, argument meaning, shapes, exceptions):

* ``compute_cheby_coeff``   pygsp/filters/approximations.py:9-55   (host quadrature, K+1 points)
* ``cheby_op``              pygsp/filters/approximations.py:58-114 -> gspx_cheby_filter (device)
* ``lanczos_op``            pygsp/filters/approximations.py:228-341 -> gspx_lanczos_krylov_dev / _combine_dev
* ``Filter.filter`` & co    pygsp/filters/filter.py:146-391, 506-600
* ``Heat``                  pygsp/filters/heat.py:102-119
* ``MexicanHat``            pygsp/filters/mexicanhat.py:55-84 (+ utils.compute_log_scales)
* ``Modulation``            pygsp/filters/modulation.py:126-177
* ``Gabor``                 pygsp/filters/gabor.py:72-92

``method='chebyshev'`` is the accelerated path for large graphs.  ``method='exact'`` (filter.py:292-301) filters in the
Fourier domain against the full basis: the basis itself comes from the host's eigh, the transforms and the spectral
multiply run on the device (gspx_panel_gram_to_dev, gspx_spectral_apply_dev).
"""
import functools

import numpy as np

from . import _capi

# Interface notes.  Function / class names, argument lists and exception messages follow the reference
# (BSD-3-Clause, epfl-lts2/pygsp) because they are the contract a drop-in has to honour; the bodies are
# this package's own.


def filterbank_handler(func):
    """Decorator with the calling convention of pygsp.utils.filterbank_handler (utils.py:37-53): the
    wrapped function sees one kernel of the bank (keyword ``i``); called without ``i`` on a bank of
    several kernels it is mapped over all of them and the results come back as a list."""
    def per_kernel(bank, *args, **kwargs):
        if bank.Nf > 1 and "i" not in kwargs:
            return [func(bank, *args, i=index, **kwargs) for index in range(bank.Nf)]
        return func(bank, *args, **kwargs)
    per_kernel.__name__ = func.__name__
    per_kernel.__doc__ = func.__doc__
    per_kernel.__wrapped__ = func
    return per_kernel


@filterbank_handler
def compute_cheby_coeff(f, m=30, N=None, *args, **kwargs):
    """Chebyshev coefficients c_0..c_m of kernel ``i`` of filterbank ``f`` on [0, lmax], by Gauss-Chebyshev
    quadrature on N = m + 1 points (approximations.py:9-55; host, float64):

        c_o = 2/N * sum_j g(lmax/2 * (cos(theta_j) + 1)) * cos(o * theta_j),   theta_j = pi (j + 1/2) / N

    The products are formed in the reference's order (2/N * dot(samples, cos(pi * o * (j + 1/2) / N))), so
    the coefficients equal the reference's to the last bit and the parity tests compare like with like."""
    which = kwargs.pop("i", 0)
    points = int(N) if N else m + 1
    half = f.G.lmax / 2
    nodes, table = _quadrature_tables(int(m), points)
    samples = f._kernels[which](half * nodes + half)
    return np.array([2.0 / points * np.dot(samples, table[order]) for order in range(m + 1)])


@functools.lru_cache(maxsize=64)
def _quadrature_tables(m, points):
    """cos(theta_j) and the rows cos(o theta_j), o = 0..m, of the quadrature above: functions of (m, N) alone,
    so they are kept between calls (two thirds of a call's host time on small graphs went into recomputing
    them) - the same expressions as before, hence the same bits."""
    grid = np.arange(points)
    nodes = np.cos(np.pi * (grid + 0.5) / points)
    table = np.array([np.cos(np.pi * order * (grid + 0.5) / points) for order in range(m + 1)])
    nodes.setflags(write=False)
    table.setflags(write=False)
    return nodes, table


# How a SINGLE filter's polynomial is evaluated on the device (filterbanks and synthesis always
# use the three-term recurrence):
#   'recurrence' - the reference's three-term Chebyshev recurrence (approximations.py:99-112); the default;
#   'newton'     - the identical polynomial in Newton form on Leja-ordered Chebyshev nodes, by
#                  Horner: a two-term recurrence, 3 instead of 3 2/3 panel passes per order;
#   'product'    - the identical polynomial as the product of its factors (t - r) over its roots, real roots one
#                  step each (gather h, write h': 2 panel passes), conjugate pairs two steps (2 + 3 passes): 2.2 - 2.5
#                  panel passes per order;
#   'auto'       - 'product', else 'newton', for the calls where they are the faster evaluation AND product_guard() /
#                  newton_guard() clears the polynomial for the compute dtype (one filter, analysis, one device, a
#                  panel beyond the launch-bound sizes that replay as one hipGraph); the recurrence for everything else.
EVALUATIONS = ("recurrence", "newton", "product", "auto")
EVALUATION = "recurrence"
AUTO_MIN_PANEL_BYTES = 32 << 20  # below: the recurrence replays as one hipGraph (gspx option graph_launch = 2)


def set_evaluation(mode):
    global EVALUATION
    if mode not in EVALUATIONS:
        raise ValueError("evaluation must be 'recurrence', 'newton', 'product' or 'auto'")
    EVALUATION = mode


def _leja_order(points):
    """Greedy Leja ordering: each next point maximises the product of distances to the chosen ones
    (keeps the partial products of the Newton basis bounded: stable Horner evaluation)."""
    pts = np.asarray(points, dtype=np.float64)
    n = pts.size
    chosen = np.empty(n)
    left = np.ones(n, dtype=bool)
    first = int(np.argmax(np.abs(pts)))
    chosen[0] = pts[first]
    left[first] = False
    logp = np.full(n, -np.inf)
    with np.errstate(divide="ignore"):
        logp[left] = np.log(np.abs(pts[left] - chosen[0]))
    for k in range(1, n):
        cand = np.where(left, logp, -np.inf)
        i = int(np.argmax(cand))
        chosen[k] = pts[i]
        left[i] = False
        with np.errstate(divide="ignore"):
            logp[left] += np.log(np.abs(pts[left] - chosen[k]))
    return chosen


_newton_cache = {}


def cheb_to_newton(c, ordering="leja"):
    """Chebyshev coefficients c_0..c_K of p(t) = c_0/2 + sum_k c_k T_k(t) (as compute_cheby_coeff
    returns them) -> (nodes r_0..r_{K-1}, divided differences d_0..d_K) of the SAME polynomial,
    p(t) = sum_j d_j prod_{i<j} (t - r_i).  Computed in 80+4K-digit decimal arithmetic from the
    float64 inputs, so the only rounding is the final conversion of d_j to float64.
    `ordering`: 'leja' (what the engine uses: bounded partial products, a stable Horner evaluation) or 'sorted'
    (the nodes in decreasing order: the textbook ill-conditioned Newton form, for the guard's tests)."""
    import decimal
    c = np.asarray(c, dtype=np.float64).ravel()
    if not np.all(np.isfinite(c)):
        raise ValueError("the Chebyshev coefficients must be finite")
    if ordering not in ("leja", "sorted"):
        raise ValueError("ordering must be 'leja' or 'sorted'")
    key = c.tobytes() + ordering.encode()
    hit = _newton_cache.get(key)
    if hit is not None:
        return hit
    K = c.size - 1
    if K < 1:
        raise TypeError("The coefficients have an invalid shape")
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 80 + 4 * K
        nodes = np.cos(np.pi * (np.arange(K) + 0.5) / K)
        if ordering == "leja":
            nodes = _leja_order(nodes)
        extra = 0.0 if np.all(np.abs(nodes) > 1e-3) else 0.987654321
        r = [D(float(v)) for v in nodes] + [D(extra)]
        cd = [D(float(v)) for v in c]

        def p(t):
            t0, t1 = D(1), t
            acc = cd[0] / 2 + cd[1] * t1
            for k in range(2, K + 1):
                t0, t1 = t1, 2 * t * t1 - t0
                acc += cd[k] * t1
            return acc

        d = [p(t) for t in r]
        for j in range(1, K + 1):
            for i in range(K, j - 1, -1):
                d[i] = (d[i] - d[i - 1]) / (r[i] - r[i - j])
        out = (np.ascontiguousarray(nodes), np.array([float(v) for v in d]))
    if len(_newton_cache) > 64:
        _newton_cache.clear()
    _newton_cache[key] = out
    return out


# Host-side stability guard of the Newton evaluation (VERDICT r5 "Next 2c").  Every eigencomponent of a signal goes
# through the SCALAR Horner recurrence h_j = (t - r_j) h_{j+1} + d_j at its own t in [-1, 1], so the scalar
# polynomial tells what the device will do:
#   grid_err       both forms evaluated on a grid over [-1, 1] (the Chebyshev sum in extended precision, the Horner
#                  form in the COMPUTE dtype with the rounded r_j, d_j the kernels receive): max |difference| / max |p|;
#   amplification  the running error bound of the Horner form: a rounding error made at stage j is carried to the
#                  result through prod_{i<j} (t - r_i), so  A = sum_j max_t |prod_{i<j}(t - r_i)| max_t |h_j(t)| / max |p|
#                  and eps A (times a small factor for the row products) bounds the relative error of the result;
#   finite         every d_j, r_j and intermediate representable in the compute dtype (fp32: orders beyond ~120
#                  overflow d_j ~ 2^j).
# On Leja-ordered Chebyshev nodes A stays below ~150 for the Heat / Mexican-hat kernels at orders 30-200
# (profiles/r06_newton_guard.md); the guard is what notices anything else.
NEWTON_GUARD = {
    # compute dtype: (largest grid_err, largest eps * A * 8)
    np.dtype(np.float64): (1e-12, 1e-10),
    np.dtype(np.float32): (2e-5, 2.5e-4),
}
_guard_cache = {}


def newton_stability(c, dtype=np.float64, nodes=None, dcoef=None):
    """The guard's measurements for the polynomial with Chebyshev coefficients `c` evaluated in `dtype` through
    the Newton form (`nodes`, `dcoef`; default: cheb_to_newton(c)).  Returns a dict: K, grid_err, amplification,
    eps_amplification, finite, d_max, p_max."""
    c = np.asarray(c, dtype=np.float64).ravel()
    dt = np.dtype(dtype)
    if nodes is None or dcoef is None:
        nodes, dcoef = cheb_to_newton(c)
    nodes, dcoef = np.asarray(nodes, dtype=np.float64), np.asarray(dcoef, dtype=np.float64)
    K = nodes.size
    grid = np.unique(np.concatenate([np.cos(np.linspace(0.0, np.pi, 8 * K + 9)), nodes, [-1.0, 1.0]]))
    # the Chebyshev sum, extended precision (approximations.py:99-112 on a scalar)
    tl, cl = grid.astype(np.longdouble), c.astype(np.longdouble)
    t_old, t_cur = np.ones_like(tl), tl.copy()
    p = cl[0] / 2 + cl[1] * t_cur
    for k in range(2, K + 1):
        t_old, t_cur = t_cur, 2 * tl * t_cur - t_old
        p = p + cl[k] * t_cur
    p_max = float(np.max(np.abs(p)))
    with np.errstate(all="ignore"):
        g, dd, rr = grid.astype(dt), dcoef.astype(dt), nodes.astype(dt)
        h = np.full_like(g, dd[K])
        h_max = [float(np.max(np.abs(h)))]
        for j in range(K - 1, -1, -1):
            h = (g - rr[j]) * h + dd[j]
            h_max.append(float(np.max(np.abs(h))))
        h_max.reverse()  # h_max[j]: the Horner intermediate whose leading coefficient is d_j
        finite = bool(np.all(np.isfinite(dd)) and np.all(np.isfinite(h_max)))
        part, part_max = np.ones_like(grid), [1.0]
        for j in range(K):
            part = part * (grid - nodes[j])
            part_max.append(float(np.max(np.abs(part))))
        scale = p_max if p_max > 0 else 1.0
        grid_err = float(np.max(np.abs(h.astype(np.longdouble) - p))) / scale if finite else float("inf")
        amp = float(sum(a * b for a, b in zip(part_max, h_max))) / scale if finite else float("inf")
    return {"K": int(K), "dtype": dt.name, "grid_err": grid_err, "amplification": amp,
            "eps_amplification": float(np.finfo(dt).eps) * amp, "finite": finite,
            "d_max": float(np.max(np.abs(dcoef))), "p_max": p_max}


def newton_guard(c, dtype=np.float64):
    """(ok, measurements): may the polynomial with Chebyshev coefficients `c` be evaluated in Newton form in
    `dtype`?  ok is False when the two forms of the scalar polynomial disagree on the grid beyond the dtype's
    threshold, when the running error bound exceeds it, or when a coefficient or intermediate is not representable
    (NEWTON_GUARD); evaluation='auto' then keeps the three-term recurrence."""
    c = np.asarray(c, dtype=np.float64).ravel()
    dt = np.dtype(dtype)
    key = (c.tobytes(), dt.str)
    hit = _guard_cache.get(key)
    if hit is not None:
        return hit
    if dt not in NEWTON_GUARD or c.size < 2 or not np.all(np.isfinite(c)):
        out = (False, {"K": int(c.size - 1), "dtype": dt.name, "finite": False, "reason": "coefficients"})
    else:
        m = newton_stability(c, dt)
        lim_grid, lim_amp = NEWTON_GUARD[dt]
        why = ("overflow" if not m["finite"] else "grid" if not m["grid_err"] <= lim_grid
               else "amplification" if not 8 * m["eps_amplification"] <= lim_amp else None)
        m["reason"] = why
        out = (why is None, m)
    if len(_guard_cache) > 256:
        _guard_cache.clear()
    _guard_cache[key] = out
    return out


def newton_program(nodes, dcoef):
    """The Newton form's Horner recurrence h <- (t - r_j) h + d_j x, j = K-1 .. 0, as (scale, beta, gamma) rows of a
    polynomial program with o_s = x (gspx_poly_program(old_is_x = 1)); what gspx_newton_filter runs."""
    nodes, d = np.asarray(nodes, dtype=np.float64), np.asarray(dcoef, dtype=np.float64)
    K = nodes.size
    rows = [[0.5 * d[K], 0.0, d[K - 1] - d[K] * nodes[K - 1]]]
    rows += [[0.5, -nodes[K - 1 - s], d[K - 1 - s]] for s in range(1, K)]
    return np.ascontiguousarray(rows, dtype=np.float64)


_product_cache = {}


def _leja_order_roots(points):
    """Greedy Leja ordering of the factors' representatives (a real root, or the upper one of a conjugate pair - its
    mirror counted with it): each next one maximises the product of distances to those chosen before."""
    pts = np.asarray(points, dtype=np.complex128)
    n = pts.size
    order, left = [], list(range(n))
    first = max(left, key=lambda i: abs(pts[i]))
    order.append(first)
    left.remove(first)
    with np.errstate(divide="ignore"):
        logp = {i: np.log(abs(pts[i] - pts[first])) + np.log(abs(pts[i] - np.conj(pts[first]))) for i in left}
        while left:
            i = max(left, key=lambda k: logp[k])
            order.append(i)
            left.remove(i)
            for k in left:
                logp[k] += np.log(abs(pts[k] - pts[i])) + np.log(abs(pts[k] - np.conj(pts[i])))
    return order


PRODUCT_TRIM = {np.dtype(np.float64): 1e-13, np.dtype(np.float32): 1e-9}  # (the quadrature's noise floor is ~3e-14)


def effective_coefficients(c, dtype=np.float64):
    """`c` without its negligible tail: trailing coefficients below PRODUCT_TRIM[dtype] of the largest are dropped (at
    least c_0, c_1 stay).  A converged Chebyshev series ends in rounding noise of the quadrature; every |T_k| <= 1 on the
    spectrum, so the polynomial moves by at most the sum of what is dropped - 1e-13 of its maximum at order 200 in fp64.
    What evaluation='auto' evaluates, in whichever form: an order-200 Heat(50) is 41 terms."""
    c = np.asarray(c, dtype=np.float64).ravel()
    trim = PRODUCT_TRIM.get(np.dtype(dtype), 1e-14)
    top = max(abs(c[0]) / 2, np.max(np.abs(c[1:]))) if c.size > 1 else 0.0
    K = c.size - 1
    while K > 1 and abs(c[K]) <= trim * top:
        K -= 1
    return c[:K + 1]


def cheb_to_product(c, dtype=np.float64):
    """Chebyshev coefficients c_0..c_K of p(t) = c_0/2 + sum_k c_k T_k(t) -> the PRODUCT-form program of the same
    polynomial, an (S, 3) array of (scale, beta, gamma) rows for gspx_poly_program(old_is_x = 0):

        p(t) = C prod_j sigma_j (t - r_j),      h_0 = x,  h_{s+1} = scale_s (2 t) h_s + beta_s h_s + gamma_s h_{s-1}

    The roots are the eigenvalues of the colleague matrix (numpy.polynomial.chebyshev.chebroots, float64).  A real
    root r is one step (sigma / 2, -sigma r, 0); a conjugate pair a +- ib two steps, (sigma / 2, -sigma a, 0) and
    (sigma / 2, -sigma a, sigma^2 b^2): sigma^2 ((t - a)^2 + b^2).  sigma_j = 2 / |r_j + sqrt(r_j^2 - 1)| is the
    logarithmic-capacity normalisation of the factor on [-1, 1] (the mean of log |sigma_j (t - r_j)| over the
    Chebyshev measure is 0), so partial products neither grow nor vanish on average whatever the order; the constant
    C = lead / prod sigma_j (formed in logarithms) rides on the first factor.  Factors are Leja-ordered.  Trailing
    coefficients below PRODUCT_TRIM[dtype] of the largest are dropped first: a converged Chebyshev series ends in
    rounding noise whose roots only add steps and error amplification (an order-200 Heat(50) is 41 factors, an
    order-200 Heat(10) 21 - the polynomial moves by 1e-13 of its maximum, which product_guard() measures along with
    everything else: its reference is the FULL polynomial)."""
    from numpy.polynomial import chebyshev as npcheb
    c = np.asarray(c, dtype=np.float64).ravel()
    if c.size < 2:
        raise TypeError("The coefficients have an invalid shape")
    if not np.all(np.isfinite(c)):
        raise ValueError("the Chebyshev coefficients must be finite")
    trim = PRODUCT_TRIM.get(np.dtype(dtype), 1e-14)
    key = c.tobytes() + np.dtype(dtype).str.encode()
    hit = _product_cache.get(key)
    if hit is not None:
        return hit
    cc = c.copy()
    cc[0] /= 2
    top = np.max(np.abs(cc))
    K = cc.size - 1
    while K > 1 and abs(cc[K]) <= trim * top:
        K -= 1
    cc = cc[:K + 1]
    if cc[K] == 0.0:
        raise ValueError("the polynomial is constant: no product form")
    roots = npcheb.chebroots(cc)
    lead_sign, lead_log = np.sign(cc[K]), np.log(abs(cc[K])) + (K - 1) * np.log(2.0)
    reps, used = [], np.zeros(roots.size, dtype=bool)
    for i, r in enumerate(roots):  # real roots and the upper member of every conjugate pair
        if used[i]:
            continue
        used[i] = True
        if abs(r.imag) <= 1e-11 * max(1.0, abs(r)):
            reps.append(complex(r.real, 0.0))
            continue
        dist = np.where(used, np.inf, np.abs(roots - np.conj(r)))
        j = int(np.argmin(dist))
        if not np.isfinite(dist[j]) or dist[j] > 1e-6 * max(1.0, abs(r)):
            raise ValueError("the roots of the polynomial do not pair up: no product form")
        used[j] = True
        reps.append(complex(0.5 * (r.real + roots[j].real), 0.5 * (abs(r.imag) + abs(roots[j].imag))))
    reps = [reps[i] for i in _leja_order_roots(reps)]
    rows, log_c = [], lead_log
    for r in reps:
        w = r + np.sqrt(r * r - 1)
        if abs(w) < 1:
            w = r - np.sqrt(r * r - 1)
        sig = 2.0 / abs(w)
        if r.imag == 0.0:
            rows.append([0.5 * sig, -sig * r.real, 0.0])
            log_c -= np.log(sig)
        else:
            rows.append([0.5 * sig, -sig * r.real, 0.0])
            rows.append([0.5 * sig, -sig * r.real, sig * sig * r.imag * r.imag])
            log_c -= 2 * np.log(sig)
    const = lead_sign * np.exp(log_c)
    rows[0][0] *= const
    rows[0][1] *= const
    if reps[0].imag != 0.0:  # the first factor is a pair: its second step adds sigma^2 b^2 h_0, which needs the constant too
        rows[1][2] *= const
    out = np.ascontiguousarray(rows, dtype=np.float64)
    out.setflags(write=False)
    if len(_product_cache) > 64:
        _product_cache.clear()
    _product_cache[key] = out
    return out


PRODUCT_GUARD = {
    # compute dtype: (largest grid_err, largest eps * A * 8).  The second figure is a WORST-CASE bound of the result's
    # relative error and is allowed up to the path's bar (1e-5 / 1e-3, BASELINE.json): the device stays two orders of
    # magnitude below it wherever it was measured (profiles/r06_product_form.md: bound 4.5e-4 -> 6.8e-7, 1e-4 -> 5e-11),
    # and tests/test_gpu_7_newton.py holds every form 'auto' picks to a tenth of the bar at 1M x 64.
    np.dtype(np.float64): (1e-10, 1e-5),
    np.dtype(np.float32): (1e-4, 1e-3),
}


def product_stability(c, dtype=np.float64, program=None):
    """The guard's measurements for the product form of the polynomial with Chebyshev coefficients `c` in `dtype`
    (program: default cheb_to_product(c)): the scalar recurrence every eigencomponent goes through, run in the compute
    dtype on a grid over [-1, 1], against the Chebyshev sum in extended precision (grid_err); the running error bound
    A = sum_s max_t |h_s| max_t |R_s| / max |p|, R_s = what the remaining steps multiply an error made at step s by
    (computed by running the remaining program on a unit impulse); finiteness of every coefficient and intermediate."""
    c = np.asarray(c, dtype=np.float64).ravel()
    dt = np.dtype(dtype)
    prog = np.asarray(cheb_to_product(c, dt) if program is None else program, dtype=np.float64).reshape(-1, 3)
    S = prog.shape[0]
    K = c.size - 1
    grid = np.unique(np.concatenate([np.cos(np.linspace(0.0, np.pi, 8 * K + 9)), [-1.0, 1.0]]))
    tl, cl = grid.astype(np.longdouble), c.astype(np.longdouble)
    t_old, t_cur = np.ones_like(tl), tl.copy()
    p = cl[0] / 2 + cl[1] * t_cur
    for k in range(2, K + 1):
        t_old, t_cur = t_cur, 2 * tl * t_cur - t_old
        p = p + cl[k] * t_cur
    p_max = float(np.max(np.abs(p)))
    scale = p_max if p_max > 0 else 1.0
    with np.errstate(all="ignore"):
        g, pr = grid.astype(dt), prog.astype(dt)
        h_prev, h = np.zeros_like(g), np.ones_like(g)
        h_max = []
        for s in range(S):
            gam = pr[s, 2] if s else dt.type(0)
            h_prev, h = h, (pr[s, 0] * 2) * g * h + pr[s, 1] * h + gam * h_prev
            h_max.append(float(np.max(np.abs(h))))
        finite = bool(np.all(np.isfinite(pr)) and np.all(np.isfinite(h_max)))
        grid_err = float(np.max(np.abs(h.astype(np.longdouble) - p))) / scale if finite else float("inf")
        # what the rest of the program does to a unit error in h_{s+1} (h_s exact): run steps s+1 .. S-1 on (0, 1)
        amp = 0.0
        if finite:
            e_prev, e = np.zeros_like(grid), np.ones_like(grid)  # after the LAST step an error stays as it is
            rest = [1.0]
            # backwards: the linear map of steps s+1.. is the forward recurrence started from (h_s, h_{s+1}) = (0, 1)
            for s in range(S - 1, 0, -1):
                a_prev, a_cur = np.zeros_like(grid), np.ones_like(grid)
                for q in range(s, S):
                    a_prev, a_cur = a_cur, (prog[q, 0] * 2) * grid * a_cur + prog[q, 1] * a_cur + prog[q, 2] * a_prev
                rest.append(float(np.max(np.abs(a_cur))))
                if S > 64 and (S - s) % 4:  # (long programs: every fourth suffix is enough for a bound of this kind)
                    rest[-1] = max(rest[-1], rest[-2])
            rest.reverse()  # rest[s]: amplification of an error made in h_{s+1}
            amp = float(sum(a * b for a, b in zip(h_max, rest))) / scale
    return {"S": int(S), "K": int(K), "dtype": dt.name, "grid_err": grid_err, "amplification": amp if finite else float("inf"),
            "eps_amplification": float(np.finfo(dt).eps) * amp if finite else float("inf"), "finite": finite,
            "h_max": max(h_max) if h_max else 0.0, "p_max": p_max,
            "panel_passes_per_order": float(sum(2 if r[2] == 0 else 3 for r in prog)) / max(K, 1)}


def product_guard(c, dtype=np.float64):
    """(ok, measurements): may the polynomial with Chebyshev coefficients `c` be evaluated in product form in `dtype`?
    False when the roots do not form a real polynomial's pairs, when the scalar program disagrees with the Chebyshev
    sum on the grid beyond the dtype's threshold, when the running error bound exceeds it, or when an intermediate is
    not representable (PRODUCT_GUARD)."""
    c = np.asarray(c, dtype=np.float64).ravel()
    dt = np.dtype(dtype)
    key = ("product", c.tobytes(), dt.str)
    hit = _guard_cache.get(key)
    if hit is not None:
        return hit
    if dt not in PRODUCT_GUARD or c.size < 2 or not np.all(np.isfinite(c)):
        out = (False, {"K": int(c.size - 1), "dtype": dt.name, "finite": False, "reason": "coefficients"})
    else:
        try:
            m = product_stability(c, dt)
        except (ValueError, np.linalg.LinAlgError) as e:
            m = {"K": int(c.size - 1), "dtype": dt.name, "finite": False, "reason": "roots: " + str(e)}
            out = (False, m)
        else:
            lim_grid, lim_amp = PRODUCT_GUARD[dt]
            why = ("overflow" if not m["finite"] else "grid" if not m["grid_err"] <= lim_grid
                   else "amplification" if not 8 * m["eps_amplification"] <= lim_amp else None)
            m["reason"] = why
            out = (why is None, m)
    if len(_guard_cache) > 256:
        _guard_cache.clear()
    _guard_cache[key] = out
    return out


def choose_evaluation(evaluation, coeffs, dtype, n_vertices, n_signals, split=False):
    """'recurrence', 'newton' or 'product' for one analysis call.  'newton' / 'product' are the caller's explicit choice
    (a polynomial that does not fit the compute dtype is an error then, not a silent fallback); 'auto' takes the product
    form, else the Newton form, only where they are faster and cleared by product_guard() / newton_guard()."""
    if evaluation not in EVALUATIONS:
        raise ValueError("evaluation must be 'recurrence', 'newton', 'product' or 'auto'")
    if evaluation == "recurrence" or coeffs.shape[0] != 1:
        return "recurrence"
    if evaluation == "product":
        if split:
            raise ValueError("evaluation='product' is a single-device evaluation; it cannot be combined with a device "
                             "list (devices=[...] / plugin.install(devices=[...]))")
        ok, m = product_guard(coeffs[0], dtype)
        if not m.get("finite", False):
            raise ValueError("evaluation='product': the product form of this order-{} polynomial is not representable "
                             "in {} ({}) - use the recurrence (or evaluation='auto')".format(m["K"], m["dtype"],
                                                                                             m.get("reason")))
        return "product"
    if evaluation == "newton":
        if split:
            # (the column split runs the three-term recurrence on every GPU: the same call must not return
            # different bits with and without a device list)
            raise ValueError("evaluation='newton' is a single-device evaluation; it cannot be combined with a device "
                             "list (devices=[...] / plugin.install(devices=[...]))")
        ok, m = newton_guard(coeffs[0], dtype)
        if not m.get("finite", False):
            raise ValueError("evaluation='newton': the Newton coefficients of this order-{} polynomial are not "
                             "representable in {} - use the recurrence (or evaluation='auto')".format(m["K"], m["dtype"]))
        return "newton"
    if split or n_vertices * n_signals * np.dtype(dtype).itemsize < AUTO_MIN_PANEL_BYTES:
        return "recurrence"
    if coeffs.shape[1] > 2 and product_guard(coeffs[0], dtype)[0]:
        return "product"
    return "newton" if newton_guard(effective_coefficients(coeffs[0], dtype), dtype)[0] else "recurrence"


def _as_coeff_matrix(c):
    """(Nf, M) float64 from what the reference accepts as ``c``: one vector, a 2-D array or a list of
    vectors (approximations.py:77-84, where M < 2 is the TypeError below)."""
    mat = np.ascontiguousarray(np.atleast_2d(np.asarray(c)), dtype=np.float64)
    if mat.ndim != 2 or mat.shape[1] < 2:
        raise TypeError("The coefficients have an invalid shape")
    return mat


def cheby_op(G, c, signal, **kwargs):
    """Chebyshev polynomial of the graph Laplacian applied to `signal`, on the GPU.

    Same contract as approximations.py:58-114: `c` is one coefficient vector, a 2-D array or a
    list of vectors; `signal` is (N,) or (N, Nsig) of any real dtype / memory order; returns a
    float64 array of shape (Nf*N,) or (Nf*N, Nsig), block f = rows [f*N, (f+1)*N).
    """
    coeffs = _as_coeff_matrix(c)
    panel = np.asanyarray(signal)
    if np.iscomplexobj(panel):
        raise TypeError("complex signals are not supported by the Chebyshev path")
    if panel.ndim not in (1, 2) or panel.shape[0] != G.N:
        raise ValueError("First dimension must be the number of vertices "
                         "G.N = {}, got {}.".format(G.N, panel.shape))
    vector_in = panel.ndim == 1
    x = panel[:, np.newaxis] if vector_in else panel
    devices = _device_list(G, kwargs.get("devices"))
    evaluation = kwargs.get("evaluation") or _configured_evaluation(G)
    if evaluation not in EVALUATIONS:
        raise ValueError("evaluation must be 'recurrence', 'newton', 'product' or 'auto'")
    if devices is not None and x.shape[1] > 0:
        choose_evaluation(evaluation, coeffs, np.float64, G.N, x.shape[1], split=True)  # ('newton' + a split: an error)
        # signal-parallel: the graph replicated per GPU, the columns split, one RCCL gather
        from . import multi
        y, ms = multi.filter_columns(G, coeffs, x, devices, _capi.ANALYSIS)
        how = "recurrence"
    else:
        dev = _device_graph_of(G)
        how = "recurrence"
        if evaluation != "recurrence":  # (the default never looks at the device graph's dtype or the guard)
            how = choose_evaluation(evaluation, coeffs, dev.dtype, G.N, x.shape[1])
        c_used = coeffs
        if evaluation == "auto" and how != "product" and coeffs.shape[0] == 1:  # ('auto' evaluates the series without
            c_used = effective_coefficients(coeffs[0], dev.dtype)[np.newaxis, :]  # its negligible tail, in every form)
        if how == "newton":  # (as a program: host arrays of any size go through the same pipelined entry point)
            y, ms = dev.program_filter(newton_program(*cheb_to_newton(c_used[0])), x, G.lmax, old_is_x=True)
        elif how == "product":
            y, ms = dev.program_filter(cheb_to_product(coeffs[0], dev.dtype), x, G.lmax)
        else:
            y, ms = dev.cheby_filter(c_used, x, G.lmax, _capi.ANALYSIS)
    _record_timing(G, ms, how)
    stacked = np.asarray(y, dtype=np.float64).reshape(coeffs.shape[0] * G.N, x.shape[1])
    return stacked[:, 0] if vector_in else stacked


def _grad_coefficients(cross):
    """(Nf, M) gradient of the coefficients from the (Nf, M, Nsig) cross-moments: summed over the signal columns in
    fp64 on the host, column 0 halved (c_0 enters the polynomial as c_0 / 2, approximations.py:101)."""
    grad = np.asarray(cross, dtype=np.float64).sum(axis=2)
    grad[:, 0] *= 0.5
    return grad


def _vjp_host(dev, lmax, coeffs, x, cot, synthesis):
    """Both halves of a vector-Jacobian product on host arrays, through the host-array calls of `dev` (an
    engine.DeviceGraph, or a stand-in with its cheby_filter / cheby_cross_moments).  Analysis forward: x (N, Nsig),
    cot (Nf, N, Nsig); d/dx = sum_f p_f(L) cot_f is the synthesis call (L symmetric), d/dc_fk = w_k <cot_f, T_k x>.
    Synthesis forward: x (Nf, N, Nsig), cot (N, Nsig); d/dx_f = p_f(L) cot is the analysis call and
    d/dc_fk = w_k <x_f, T_k cot>.  Returns (grad_x, (Nf, M) grad_c, device ms)."""
    M = coeffs.shape[1]
    if synthesis:
        gx, ms1 = dev.cheby_filter(coeffs, cot, lmax, _capi.ANALYSIS)
        cross, ms2 = dev.cheby_cross_moments(cot, x, lmax, M)
    else:
        gx, ms1 = dev.cheby_filter(coeffs, cot, lmax, _capi.SYNTHESIS)
        cross, ms2 = dev.cheby_cross_moments(x, cot, lmax, M)
    return np.asarray(gx, dtype=np.float64), _grad_coefficients(cross), ms1 + ms2


def _vjp_device(dev, lmax, coeffs, x_ptr, cot_ptr, gx_ptr, nsig, synthesis, need_x=True, need_c=True):
    """_vjp_host on device pointers (plane layouts as there); grad_x is written to gx_ptr.  need_x / need_c: which of
    the two device calls run (a half that is not needed costs nothing).  Returns ((Nf, M) grad_c or None, device ms)."""
    Nf, M = coeffs.shape
    ms, grad_c = 0.0, None
    if need_x:
        ms += dev.cheby_filter_dev(coeffs, cot_ptr, gx_ptr, nsig, lmax, _capi.ANALYSIS if synthesis else _capi.SYNTHESIS)
    if need_c:
        a, b = (cot_ptr, x_ptr) if synthesis else (x_ptr, cot_ptr)
        cross, ms2 = dev.cheby_cross_moments_dev(a, b, nsig, Nf, lmax, M)
        grad_c, ms = _grad_coefficients(cross), ms + ms2
    return grad_c, ms


def cheby_op_vjp(G, c, signal, cotangent, **kwargs):
    """Vector-Jacobian product of ``cheby_op(G, c, signal)``: for a cotangent of the shape cheby_op returns -
    (Nf N,) or (Nf N, Nsig), block f = rows [f N, (f + 1) N) - the pair (grad_signal, grad_c) with

        grad_signal = sum_f p_f(L) cotangent_f                       one synthesis call with `c` (L is symmetric)
        grad_c[f, k] = w_k sum_{n, j} (T_k(Lt) signal)[n, j] cotangent_f[n, j],   w_0 = 1/2, w_k = 1 otherwise

    grad_signal is a float64 array of signal's shape; grad_c a float64 array of c's shape, the cross-moments of the
    recurrence (gspx_cheby_cross_moments_dev) summed over the signal columns in fp64 on the host.  Only the
    recurrence evaluates the polynomial here: `evaluation` other than None / 'recurrence', and a device list, raise
    ValueError."""
    coeffs, x, planes = _vjp_arguments("cheby_op_vjp", G, c, signal, cotangent, kwargs)
    gx, grad_c, ms = _vjp_host(_device_graph_of(G), G.lmax, coeffs, x, planes, False)
    _record_timing(G, ms)
    return gx.reshape(np.shape(signal)), grad_c.reshape(np.shape(c) if np.ndim(c) else coeffs.shape)


def _vjp_arguments(who, G, c, signal, cotangent, kwargs):
    """The argument checks cheby_op_vjp and the calls that differentiate with respect to the graph share (`who` names
    the caller in the messages): ((Nf, M) coefficients, the signal as (N, Nsig), the cotangent as (Nf, N, Nsig) planes)."""
    coeffs = _as_coeff_matrix(c)
    if kwargs.get("evaluation") not in (None, "recurrence"):
        raise ValueError("{} differentiates the recurrence: evaluation must be None or 'recurrence'".format(who))
    if kwargs.get("devices") is not None:
        raise ValueError("{} runs on one GPU: it takes no device list".format(who))
    panel, cot = np.asanyarray(signal), np.asanyarray(cotangent)
    if np.iscomplexobj(panel) or np.iscomplexobj(cot):
        raise TypeError("complex signals are not supported by the Chebyshev path")
    if panel.ndim not in (1, 2) or panel.shape[0] != G.N:
        raise ValueError("First dimension must be the number of vertices "
                         "G.N = {}, got {}.".format(G.N, panel.shape))
    Nf = coeffs.shape[0]
    if cot.shape != (Nf * G.N,) + panel.shape[1:]:
        raise ValueError("the cotangent must have the shape cheby_op returns, {}, got {}"
                         .format((Nf * G.N,) + panel.shape[1:], cot.shape))
    x = panel.reshape(G.N, -1)
    return coeffs, x, cot.reshape(Nf, G.N, x.shape[1])


def _pair_list(G, pairs):
    """`pairs` as a contiguous (2, P) int32 array, every pair inside the graph and s != t; None stays None (the graph's
    own edge list)."""
    if pairs is None:
        return None
    p = np.asarray(pairs)
    if p.dtype.kind not in "iu":
        raise TypeError("pairs must be an integer array, got {}".format(p.dtype))
    if p.ndim != 2 or p.shape[0] != 2:
        raise ValueError("pairs must be (2, P), got {}".format(p.shape))
    if p.size and (p.min() < 0 or p.max() >= G.N):
        raise ValueError("pairs name a vertex outside 0 .. N - 1 = {}".format(G.N - 1))
    if np.any(p[0] == p[1]):
        raise ValueError("pairs must join two different vertices (s != t)")
    return np.ascontiguousarray(p, dtype=np.int32)


def cheby_op_vjp_laplacian(G, c, signal, cotangent, pairs=None, **kwargs):
    """How a loss that reads ``cheby_op(G, c, signal)`` changes with the ENTRIES of the Laplacian, at fixed G.lmax and
    with the entries taken as independent: with Gbar = dl/dL for the cotangent dl/dy (shape as cheby_op returns),

        gdiag[i] = Gbar_ii   for every vertex,          goff[p] = Gbar_st + Gbar_ts   for every pair p = (s, t),

    both float64, (N,) and (P,), summed over the signal columns (gspx_cheby_laplacian_grad_dev).  `pairs`: a (2, P)
    integer array of any pairs s != t - edges or not, either orientation, repeats allowed - or None for
    ``G.get_edge_list()``.  Argument checks and shapes are cheby_op_vjp's.  cheby_op_vjp_weights turns the two into the
    gradient of the edge weights."""
    coeffs, x, cot = _vjp_arguments("cheby_op_vjp_laplacian", G, c, signal, cotangent, kwargs)
    gdiag, goff, ms = _device_graph_of(G).cheby_laplacian_grad(coeffs, x, cot, G.lmax, _pair_list(G, pairs), True)
    _record_timing(G, ms)
    return np.asarray(gdiag, dtype=np.float64), np.asarray(goff, dtype=np.float64)


def _laplacian_call(G, coeffs, x, cot):
    """The host-array device call of _weight_gradient on G's device graph (looked up when the call is made)."""
    return lambda pairs, need_diag: _device_graph_of(G).cheby_laplacian_grad(coeffs, x, cot, G.lmax, pairs, need_diag)


def _weight_gradient(G, pairs, call):
    """(dl/dw (P,), device ms): the chain rule from the entries of L to the weights of the pairs, for G.lap_type.
    pairs: a checked (2, P) int32 array or None; call(pairs or None, need_diag) -> (gdiag, goff, ms) is the ONE
    device call (engine.DeviceGraph.cheby_laplacian_grad with the signals bound).  Every refusal comes before it."""
    if G.is_directed():
        raise ValueError("the weight gradient is defined for undirected graphs (one weight per unordered pair)")
    if G.lap_type not in ("combinatorial", "normalized"):
        raise ValueError("unknown Laplacian type {}".format(G.lap_type))
    loops = bool(np.any(G.W.diagonal() != 0))
    if loops and (pairs is None or G.lap_type == "normalized"):
        raise ValueError("the graph has self-loops: its own edge list is not a list of pairs s != t")
    es, et, ew = G.get_edge_list()
    s, t = (es, et) if pairs is None else pairs
    if G.lap_type == "combinatorial":  # L = D - W: dL_ss = dL_tt = 1, dL_st = dL_ts = -1
        gdiag, goff, ms = call(pairs, True)
        return gdiag[s] + gdiag[t] - goff, ms
    # L = I - S W S, S = diag(d^-1/2): the entry itself, and the degrees of both endpoints through every own edge
    d = np.ravel(np.asarray(G.W.sum(axis=1), dtype=np.float64))
    if np.any(d[s] == 0) or np.any(d[t] == 0):
        raise ValueError("the normalized Laplacian's weight gradient needs endpoints of positive degree")
    E = es.size
    if pairs is None:
        _, ge, ms = call(None, False)
        gp = ge
    else:  # own edges and pairs in ONE device call
        both = np.ascontiguousarray(np.concatenate([np.stack([es, et]).astype(np.int32), pairs], axis=1))
        _, goff, ms = call(both, False)
        ge, gp = goff[:E], goff[E:]
    sigma, delta = np.zeros(G.N), np.zeros(G.N)
    sigma[d > 0] = d[d > 0] ** -0.5
    flow = ge * ew * sigma[es] * sigma[et]
    R = np.bincount(es, weights=flow, minlength=G.N) + np.bincount(et, weights=flow, minlength=G.N)
    delta[d > 0] = R[d > 0] / (2.0 * d[d > 0])
    return -gp * sigma[s] * sigma[t] + delta[s] + delta[t], ms


def cheby_op_vjp_weights(G, c, signal, cotangent, pairs=None, **kwargs):
    """The gradient of a loss that reads ``cheby_op(G, c, signal)`` with respect to the EDGE WEIGHTS of `G`, for the
    cotangent dl/dy of the shape cheby_op returns: float64 (P,), one entry per pair of `pairs` ((2, P) integers, any
    pairs s != t) or per edge of ``G.get_edge_list()`` when `pairs` is None.  For a pair that is no edge it is the
    derivative with respect to giving that pair weight.

    The gradient is taken AT FIXED ``G.lmax``: the scaling of the Laplacian into [-1, 1] is a constant of the call, the
    dependence of lmax on the weights is not followed.  G.lap_type decides the chain rule: combinatorial
    (dl/dw = gdiag[s] + gdiag[t] - goff) or normalized (the entry -w / sqrt(d_s d_t) and both degrees; with `pairs`
    given, the graph's own edges and the pairs are evaluated in one device call).  Raises ValueError for a directed
    graph, for a graph with self-loops when its own list is asked for (normalized: always), for a normalized Laplacian
    with an endpoint of degree 0, and for `evaluation` other than None / 'recurrence' or a device list."""
    coeffs, x, cot = _vjp_arguments("cheby_op_vjp_weights", G, c, signal, cotangent, kwargs)
    grad, ms = _weight_gradient(G, _pair_list(G, pairs), _laplacian_call(G, coeffs, x, cot))
    _record_timing(G, ms)
    return grad


def filter_signals_vjp_weights(bank, s, cotangent, order=30, pairs=None, coefficients=None):
    """cheby_op_vjp_weights for ``filter_signals(bank, s, 'chebyshev', order)``: `s` goes through the shape rules of
    filter_signals and the cotangent has the shape that call returns.  In synthesis (y = sum_f p_f(L) s_f) the roles
    swap: p_f(L) is symmetric, so the same function of L is the analysis call with signal `cotangent` and cotangent
    planes s_f.  Host arrays only."""
    from . import engine
    coefficients = coefficients or compute_cheby_coeff
    G, Nf = bank.G, bank.Nf
    if isinstance(s, engine.DeviceArray) or isinstance(cotangent, engine.DeviceArray):
        raise TypeError("filter_vjp_weights takes host arrays")
    s = G._check_signal(s)
    N, nsig, nfeat = _cube_shape(G, Nf, s.shape)
    synthesis = nfeat != 1
    nfout = 1 if synthesis else Nf
    coeffs = _as_coeff_matrix(coefficients(bank, m=order))
    cot = np.asanyarray(cotangent)
    if np.iscomplexobj(s) or np.iscomplexobj(cot):
        raise TypeError("complex signals are not supported by the Chebyshev path")
    if cot.size != N * nsig * nfout or (cot.ndim and cot.shape[0] != N):
        raise ValueError("the cotangent must have the shape the filter call returns, got {}".format(cot.shape))
    cube, cot = s.reshape(N, nsig, nfeat), cot.reshape(N, nsig, nfout)
    if synthesis:
        x, planes = cot[:, :, 0], np.ascontiguousarray(np.moveaxis(cube, 2, 0))
    else:
        x, planes = cube[:, :, 0], np.ascontiguousarray(np.moveaxis(cot, 2, 0))
    grad, ms = _weight_gradient(G, _pair_list(G, pairs), _laplacian_call(G, coeffs, x, planes))
    _record_timing(G, ms)
    return grad


def _conv_arguments(G, theta, signal):
    """(theta (M, Fin, Fout) float64, the signal as an (N, B, Fin) cube, the signal's shape) of a cheby_conv call."""
    from . import engine
    if isinstance(signal, engine.DeviceArray):
        raise TypeError("cheby_conv takes host arrays: a DeviceArray keeps its planes as [feature][vertex][signal], "
                        "the convolution reads (vertex, sample, feature) with the feature index fastest")
    th = np.asarray(theta, dtype=np.float64)
    if th.ndim != 3:
        raise ValueError("theta must be (M, Fin, Fout), got {}".format(th.shape))
    if th.shape[0] < 2:
        raise TypeError("The coefficients have an invalid shape")
    panel = G._check_signal(signal)
    if np.iscomplexobj(panel):
        raise TypeError("complex signals are not supported by the Chebyshev path")
    if panel.ndim not in (2, 3) or panel.shape[0] != G.N or panel.shape[-1] != th.shape[1]:
        raise ValueError("the signal must be (N, Fin) or (N, B, Fin) with N = {} and Fin = {}, got {}"
                         .format(G.N, th.shape[1], panel.shape))
    return np.ascontiguousarray(th), panel.reshape(G.N, -1, th.shape[1]), panel.shape


def cheby_conv(G, theta, signal):
    """The Chebyshev graph convolution (the ChebNet layer of Defferrard et al.) of `signal` on `G`:

        Y[n, b, :] = sum_{k < M} (T_k(Lt) X)[n, b, :] theta[k],      theta[k] a Fin x Fout matrix.

    The sum is PLAIN: theta[0] is not halved (theta[k] = c_k I for k >= 1 and theta[0] = (c_0 / 2) I is
    ``cheby_op(G, c, signal)``).  theta: (M, Fin, Fout), M >= 2, read as float64; signal: host array (N, Fin) or
    (N, B, Fin), vertex first.  Returns float64 (N, Fout) or (N, B, Fout).  One gspx_cheby_conv_dev call: M Clenshaw
    steps on B Fout columns, each fed by one dense product X theta[k] on the device.  An engine.DeviceArray is refused
    (TypeError): its planes are laid out [feature][vertex][signal]."""
    th, cube, shape = _conv_arguments(G, theta, signal)
    y, ms = _device_graph_of(G).cheby_conv(th, cube, G.lmax)
    _record_timing(G, ms)
    return np.asarray(y, dtype=np.float64).reshape(shape[:-1] + (th.shape[2],))


def cheby_conv_vjp(G, theta, signal, cotangent):
    """Vector-Jacobian product of ``cheby_conv(G, theta, signal)`` for a cotangent of the shape that call returns: the
    pair (grad_signal, grad_theta) with

        grad_signal = cheby_conv(G, theta transposed per order, cotangent)       (L is symmetric: the same operator)
        grad_theta[k, i, o] = sum_{n, b} (T_k(Lt) signal)[n, b, i] cotangent[n, b, o]     (gspx_cheby_cross_grams_dev)

    both float64, of the shapes of `signal` and `theta`."""
    th, cube, shape = _conv_arguments(G, theta, signal)
    cot = np.asanyarray(cotangent)
    if np.iscomplexobj(cot):
        raise TypeError("complex signals are not supported by the Chebyshev path")
    if cot.shape != shape[:-1] + (th.shape[2],):
        raise ValueError("the cotangent must have the shape cheby_conv returns, {}, got {}"
                         .format(shape[:-1] + (th.shape[2],), cot.shape))
    cot = cot.reshape(G.N, -1, th.shape[2])
    dev = _device_graph_of(G)
    gx, ms1 = dev.cheby_conv(np.ascontiguousarray(th.transpose(0, 2, 1)), cot, G.lmax)
    grams, ms2 = dev.cheby_cross_grams(cube, cot, G.lmax, th.shape[0])
    _record_timing(G, ms1 + ms2)
    return np.asarray(gx, dtype=np.float64).reshape(shape), np.asarray(grams, dtype=np.float64)


def filter_signals_vjp(bank, s, cotangent, order=30, coefficients=None):
    """Vector-Jacobian product of ``filter_signals(bank, s, 'chebyshev', order)``: (grad_s, grad_coefficients) for a
    cotangent of the shape that call returns.  `s` goes through the shape rules of filter_signals; in synthesis the
    roles swap (d/ds_f = p_f(L) cotangent is an analysis call, d/dc_fk = w_k <s_f, T_k cotangent>).  grad_s has the
    shape of `s`; grad_coefficients is (Nf, order + 1) float64 on the host.  DeviceArrays in (both) give a DeviceArray
    grad_s out: the panels never leave the device, only the cross-moments come back."""
    from . import engine
    coefficients = coefficients or compute_cheby_coeff
    G, Nf = bank.G, bank.Nf
    on_device = isinstance(s, engine.DeviceArray)
    if on_device != isinstance(cotangent, engine.DeviceArray):
        raise TypeError("the signal and the cotangent must both be host arrays or both be DeviceArrays")
    if not on_device:
        s = G._check_signal(s)
    N, nsig, nfeat = _cube_shape(G, Nf, s.shape)
    synthesis = nfeat != 1
    nfout = 1 if synthesis else Nf
    coeffs = _as_coeff_matrix(coefficients(bank, m=order))
    dev = _device_graph_of(G)
    if on_device:
        for a in (s, cotangent):
            if not hasattr(dev, "cheby_filter_dev") or a.ctx is not dev.ctx:
                raise ValueError("the DeviceArray does not live on the context of this graph's device Laplacian")
            if a.dtype != dev.dtype:
                raise ValueError("the DeviceArray holds {} but the graph computes in {}".format(a.dtype, dev.dtype))
        if cotangent.cube[0] != N or cotangent.size != N * nsig * nfout:
            raise ValueError("the cotangent must have the shape the filter call returns, got {}".format(cotangent.shape))
        x_ptr, keep_x = s.planes(nsig, nfeat)
        g_ptr, keep_g = cotangent.planes(nsig, nfout)
        out = engine.DeviceArray.empty(dev.ctx, (N, nsig, nfeat), dev.dtype)
        out.shape = tuple(s.shape)
        grad_c, ms = np.zeros(coeffs.shape), 0.0
        if N * nsig:
            grad_c, ms = _vjp_device(dev, G.lmax, coeffs, x_ptr, g_ptr, out.ptr, nsig, synthesis)
        del keep_x, keep_g
        _record_timing(G, ms)
        return out, grad_c
    cot = np.asanyarray(cotangent)
    if np.iscomplexobj(s) or np.iscomplexobj(cot):
        raise TypeError("complex signals are not supported by the Chebyshev path")
    if cot.size != N * nsig * nfout or (cot.ndim and cot.shape[0] != N):
        raise ValueError("the cotangent must have the shape the filter call returns, got {}".format(cot.shape))
    cube, cot = s.reshape(N, nsig, nfeat), cot.reshape(N, nsig, nfout)
    if synthesis:
        gx, grad_c, ms = _vjp_host(dev, G.lmax, coeffs, np.ascontiguousarray(np.moveaxis(cube, 2, 0)), cot[:, :, 0], True)
        gx = np.moveaxis(gx.reshape(Nf, N, nsig), 0, 2)
    else:
        gx, grad_c, ms = _vjp_host(dev, G.lmax, coeffs, cube[:, :, 0], np.ascontiguousarray(np.moveaxis(cot, 2, 0)), False)
    _record_timing(G, ms)
    return np.ascontiguousarray(gx).reshape(s.shape), grad_c


def lanczos_op(f, s, order=30):
    """Lanczos approximation of the filter bank `f` applied to `s` (approximations.py:228-277), on the GPU.

    `f`: anything with ``G``, ``Nf`` and ``evaluate`` (this package's Filter or the real pygsp one); `s`: (N,) or
    (N, Nv), a host array or a float64 engine.DeviceArray.  Returns (N Nf,) or (N Nf, Nv), row i N + n = filter i
    at vertex n; a DeviceArray in gives a DeviceArray out.  Per column x: the Krylov basis V of L from x with full
    reorthogonalisation, H = V^T L V = Uh Eh Uh^T (Eh clipped at 0), y_i = V Uh f_i(Eh) Uh^T (V^T x), all in float64
    (an fp32 graph is filtered by its float64 device graph).  Differences from the reference, on purpose:
    Nf is read from ``f.Nf`` (the reference reads ``f.g``, which Filter no longer has); a Krylov breakdown
    (beta_k <= 64 eps b, b the upper bound of lambda_max, where the reference tests an absolute np.spacing(1))
    keeps the m x m leading block of H, so the result is exact when s lies in an invariant subspace (the reference
    slices H to a non-square matrix and fails); a zero column gives zeros (the reference: NaN)."""
    from . import engine, lanczos
    G = f.G
    order = int(order)
    if order < 1:
        raise ValueError("order must be >= 1, got {}".format(order))
    on_device = isinstance(s, engine.DeviceArray)
    shape = tuple(s.shape) if on_device else np.shape(s)
    if not on_device:
        s = np.asanyarray(s)
        if np.iscomplexobj(s):
            raise TypeError("complex signals are not supported by the Lanczos path")
    if len(shape) not in (1, 2) or shape[0] != G.N:
        raise ValueError("First dimension must be the number of vertices "
                         "G.N = {}, got {}.".format(G.N, shape))
    Nf = int(f.Nf)
    N = G.N
    n = 1 if len(shape) == 1 else shape[1]
    dev = G.device_graph(np.float64) if hasattr(G, "device_graph") else _plugin_graph64(G)
    out_shape = (N * Nf,) if len(shape) == 1 else (N * Nf, n)
    be = lanczos.DeviceBackend(dev)
    bound = G._get_upper_bound()
    if on_device:
        if s.dtype != np.float64:
            raise ValueError("Lanczos filtering needs a float64 DeviceArray, got {}".format(s.dtype))
        if s.ctx is not dev.ctx:
            raise ValueError("the DeviceArray does not live on the context of this graph's device Laplacian")
        x_ptr, keep = s.planes(n, 1)
        out = engine.DeviceArray.empty(dev.ctx, (N * Nf, n, 1), np.float64)
        if N * n:
            lanczos.filter_columns(be, f, (x_ptr, n), n, order, bound, (out.ptr, n))
        del keep
        out.shape = out_shape
        _record_timing(G, be.ms["krylov"] + be.ms["combine"], "lanczos")
        return out
    x = np.ascontiguousarray(s.reshape(N, n), dtype=np.float64)
    if N * n == 0:
        return np.zeros(out_shape)
    bx = dev.ctx.upload(x)
    by = dev.ctx.alloc(N * Nf * n * 8)
    try:
        lanczos.filter_columns(be, f, (bx.ptr, n), n, order, bound, (by.ptr, n))
        y = by.download((N * Nf, n), np.float64)
    finally:
        bx.free()
        by.free()
    _record_timing(G, be.ms["krylov"] + be.ms["combine"], "lanczos")
    return y.reshape(out_shape)


def _plugin_graph64(G):
    from . import plugin
    return plugin.device_graph_for(G, dtype=np.float64)


def _rect_coefficients(lo, hi, order):
    """Chebyshev coefficients of the indicator of [cos(hi_angle), cos(lo_angle)] given the two angles
    (closed form of the integrals; the k = 0 term is doubled because the recurrence halves c_0)."""
    k = np.arange(1, order + 1)
    return np.concatenate([[2.0 * (lo - hi) / np.pi], 2.0 / (k * np.pi) * (np.sin(k * lo) - np.sin(k * hi))])


def cheby_rect(G, bounds, signal, **kwargs):
    """Ideal band-pass [bounds[0], bounds[1]] by its Chebyshev expansion (approximations.py:117-163):
    the same recurrence as cheby_op with closed-form coefficients
    c_0 = 2 (b1 - b2)/pi,  c_k = 2/(k pi) (sin k b1 - sin k b2),  b = arccos(2 bounds/lmax - 1)."""
    ok = isinstance(bounds, (list, np.ndarray)) and len(bounds) == 2
    if not ok:
        raise ValueError("Bounds of wrong shape.")
    order = int(kwargs.pop("order", 30))
    angles = np.arccos(2.0 * np.asarray(bounds, dtype=np.float64) / G.lmax - 1.0)
    return cheby_op(G, _rect_coefficients(angles[0], angles[1], order), signal, **kwargs)


def compute_jackson_cheby_coeff(filter_bounds, delta_lambda, m):
    """Chebyshev and Jackson-damped coefficients of the ideal band-pass [a, b] on
    [lambda_min, lambda_max] (approximations.py:166-225).  Unlike the reference this does not
    rescale the caller's `filter_bounds` list in place."""
    lam_lo, lam_hi = float(delta_lambda[0]), float(delta_lambda[1])
    band_lo, band_hi = float(filter_bounds[0]), float(filter_bounds[1])
    if band_lo < lam_lo or band_hi > lam_hi:
        raise ValueError("Bounds of the filter are out of the lambda values")
    if lam_lo > lam_hi:
        raise ValueError("lambda_min is greater than lambda_max")
    centre, radius = (lam_hi + lam_lo) / 2, (lam_hi - lam_lo) / 2
    angle_lo, angle_hi = np.arccos((band_lo - centre) / radius), np.arccos((band_hi - centre) / radius)
    idx = np.arange(m + 1)
    ch = np.empty(m + 1)
    ch[0] = (2 / np.pi) * (angle_lo - angle_hi)
    ch[1:] = (2 / (np.pi * idx[1:])) * (np.sin(idx[1:] * angle_lo) - np.sin(idx[1:] * angle_hi))
    # Jackson damping factors (Jackson kernel of order m, step pi / (m + 2))
    step = np.pi / (m + 2)
    damping = ((1 - idx / (m + 2)) * np.sin(step) * np.cos(idx * step)
               + np.cos(step) * np.sin(idx * step) / (m + 2)) / np.sin(step)
    return ch, ch * damping


def _device_graph_of(G):
    """The libgspx graph of `G`: our own Graph builds it on device from W; a reference
    pygsp.graphs.Graph (plugin mode) gets one attached lazily from its host-built G.L."""
    if hasattr(G, "device_graph"):
        return G.device_graph()
    from . import plugin
    return plugin.device_graph_for(G)


def _device_list(G, devices):
    """The GPUs a call is split over: the `devices` argument of the call, else the list given to
    plugin.install(devices=[...]) when `G` is a reference graph; None (one device) otherwise."""
    if devices is None and not hasattr(G, "device_graph"):
        from . import plugin
        devices = plugin._config.get("devices")
    if devices is None:
        return None
    devices = [int(d) for d in devices]
    if not devices:
        raise ValueError("devices must name at least one GPU")
    return devices if len(devices) > 1 else None


def _record_timing(G, ms, evaluation="recurrence"):
    try:
        G._gspx_last_kernel_ms = ms
        G._gspx_last_evaluation = evaluation
    except Exception:
        pass


def _configured_evaluation(G):
    """The evaluation of a call that names none: plugin.install(evaluation=...) for a reference graph, the module
    default (set_evaluation) for the mirror classes."""
    if not hasattr(G, "device_graph"):
        from . import plugin
        return plugin._config.get("evaluation") or EVALUATION
    return EVALUATION


def _shape_of(s):
    """Shape of a signal argument without touching its data (a DeviceArray would be downloaded by np.shape)."""
    shape = getattr(s, "shape", None)
    return tuple(shape) if isinstance(shape, tuple) else np.shape(s)


def _cube_shape(G, Nf, shape):
    """The shape rules of Filter.filter (filter.py:267-290) applied to a signal's SHAPE alone: returns
    (vertices, signals, input features).  A trailing axis of length 1 or Nf is the feature axis; Nf (> 1) input
    features mean synthesis.  Same checks, same messages, same order as the reference."""
    shape = tuple(shape)
    if len(shape) == 0 or shape[0] != G.N:  # graph.py:632-640
        raise ValueError("First dimension must be the number of vertices "
                         "G.N = {}, got {}.".format(G.N, shape))
    if len(shape) == 1 or shape[-1] not in (1, Nf):
        if len(shape) == 3:
            raise ValueError("Third dimension (#features) should be either 1 or the number "
                             "of filters Nf = {}, got {}.".format(Nf, shape))
        shape = shape + (1,)
    if len(shape) < 3:
        shape = (shape[0], 1, shape[-1])
    if len(shape) > 3:
        raise ValueError("At most 3 dimensions: #nodes x #signals x #features.")
    return shape


def filter_signals(bank, s, method="chebyshev", order=30, devices=None, coefficients=None, evaluation=None):
    """``Filter.filter`` (filter.py:146-328) for any object with the reference's Filter attributes (``G``, ``Nf``,
    what `coefficients` reads): the mirror class below and - through plugin.install(wrap_filter=True) - the real
    pygsp.filters.Filter.  `coefficients(bank, m=order)`: compute_cheby_coeff of whichever package `bank`
    comes from.

    analysis:  one device call, output planes [filter][vertex][signal] viewed as (vertex, signal, filter);
    synthesis: ONE device call (vector-coefficient Clenshaw: K products) where the reference loops over the
               filters (filter.py:318-321: Nf x cheby_op = K Nf products and Nf host round trips);
    a DeviceArray in gives a DeviceArray out (nothing crosses PCIe).
    `evaluation` (analysis with one filter only): 'recurrence' | 'newton' | 'auto', default the configured one."""
    from . import engine
    coefficients = coefficients or compute_cheby_coeff
    on_device = isinstance(s, engine.DeviceArray)
    if on_device:
        cube_shape = _cube_shape(bank.G, bank.Nf, s.shape)
    else:
        s = bank.G._check_signal(s)
        cube_shape = _cube_shape(bank.G, bank.Nf, s.shape)
    synthesis = cube_shape[2] != 1
    if method == "exact":
        return _filter_exact(bank, s, cube_shape)
    if method != "chebyshev":
        raise ValueError("Unknown method {}.".format(method))
    coeffs = coefficients(bank, m=order)
    if on_device:
        return _filter_device_array(bank, s, cube_shape, _as_coeff_matrix(coeffs), devices, evaluation)
    cube = s.reshape(cube_shape)
    if not synthesis:
        # device buffer [filter][vertex][signal] -> (vertex, signal, filter), as filter.py:310-311
        flat = cheby_op(bank.G, coeffs, cube[:, :, 0], devices=devices, evaluation=evaluation)
        out = np.moveaxis(flat.reshape(bank.Nf, bank.G.N, cube.shape[1]), 0, 2)
    else:
        # out = sum_f p_f(L) s[:, :, f]  (filter.py:313-322), one device call
        if np.iscomplexobj(cube):
            raise TypeError("complex signals are not supported by the Chebyshev path")
        planes = np.ascontiguousarray(np.moveaxis(cube, 2, 0))
        split = _device_list(bank.G, devices)
        if split is not None and planes.shape[2] > 0:
            from . import multi
            y, ms = multi.filter_columns(bank.G, _as_coeff_matrix(coeffs), planes, split, _capi.SYNTHESIS)
        else:
            y, ms = _device_graph_of(bank.G).cheby_filter(_as_coeff_matrix(coeffs), planes, bank.G.lmax,
                                                          _capi.SYNTHESIS)
        _record_timing(bank.G, ms)
        out = np.asarray(y, dtype=np.float64)
    return np.squeeze(out)


# ---- method='exact': dense Fourier filtering against the full basis (filter.py:292-301) -----------------------------
def _exact_basis(G):
    """(float64 DeviceGraph, DevicePanel of U) of `G`: the mirror Graph's own copy, or the one plugin mode keeps on a
    reference graph."""
    if hasattr(G, "_basis_on_device"):
        return G._basis_on_device()
    from . import plugin
    return plugin.basis_on_device_for(G)


def _exact_upload(G, cube):
    """A host cube (N, Nsig, Nfeat) as a float64 DeviceArray on the context of G's device basis."""
    from . import engine
    return engine.DeviceArray.from_host(_exact_basis(G)[0].ctx, cube, np.float64)


def _exact_gft(G, a, S, F):
    """Device call 1: the coefficients U^T s of the DeviceArray `a` read as F planes of (N, S), as a DeviceArray of
    cube (N, S, F) (the basis is full: N coefficients per signal).  One gspx_panel_gram_to_dev per plane, written
    where the result lives."""
    from . import engine, fourier
    dev, U = _exact_basis(G)
    if a.ctx is not dev.ctx:
        raise ValueError("the DeviceArray does not live on the context of this graph's Fourier basis")
    N = a.cube[0]
    x_ptr, keep = a.planes(S, F)
    hat = engine.DeviceArray.empty(dev.ctx, (N, S, F), np.float64)
    ms = 0.0
    for f in range(F):
        ms += fourier.panel_gram_to(dev.ctx, N, U.ptr, U.ld, U.width, x_ptr + 8 * f * N * S, S, S,
                                    hat.ptr + 8 * f * N * S, S)
    del keep
    return hat, ms


def _exact_apply(G, hat, H, synthesis):
    """Device call 2: U (H-weighted coefficients), the multiplier fused into the product (gspx_spectral_apply_dev).
    `hat`: DeviceArray of coefficients, cube (N, Nsig, 1) for analysis or (N, Nsig, Nf) for synthesis; `H`: host
    (Nf, N) multipliers, the only data that crosses PCIe.  Returns the DeviceArray (N, Nsig, Nf) or (N, Nsig, 1)."""
    from . import engine, fourier
    dev, U = _exact_basis(G)
    ctx = dev.ctx
    N, S, _ = hat.cube
    Nf = H.shape[0]
    out = engine.DeviceArray.empty(ctx, (N, S, 1 if synthesis else Nf), np.float64)
    ms = 0.0
    if N * S:
        with ctx._temporaries() as tmp:
            h = tmp.upload(np.ascontiguousarray(H, dtype=np.float64))
            ms = fourier.spectral_apply(ctx, N, U.ptr, U.ld, U.width, hat.ptr, S, S, out.ptr, S,
                                        fourier.SPECTRAL_SYNTHESIS if synthesis else fourier.SPECTRAL_ANALYSIS,
                                        Nf, h.ptr)
    return out, ms


def _filter_exact(bank, s, cube_shape):
    """filter_signals(method='exact'): s_out = U diag(h) U^T s per filter (filter.py:292-301), as one Gram (the
    transform of the signals) and one spectral apply (multiplier and inverse transform in one product) on the float64
    device graph's context, against the device copy of U.  numpy in gives numpy out; a float64 DeviceArray in gives a
    DeviceArray out, and then only the Nf x N multipliers ``bank.evaluate(G.e)`` cross PCIe.  The full basis is needed:
    it comes from the host's eigh (Graph.compute_fourier_basis), which bounds this path to graphs of a few ten
    thousand vertices."""
    from . import engine
    G = bank.G
    if not (hasattr(G, "gft") and hasattr(G, "igft")):
        raise NotImplementedError(
            "method='exact' (dense Fourier filtering, filter.py:292-301) is outside the "
            "accelerated path; use the reference implementation for it.")
    on_device = isinstance(s, engine.DeviceArray)
    dtype = s.dtype if on_device else np.asarray(s).dtype
    if np.issubdtype(dtype, np.complexfloating):
        raise TypeError("complex signals are not supported by the exact path")
    if (on_device or np.issubdtype(dtype, np.floating)) and dtype != np.float64:
        raise TypeError("gft / igft of a device array need float64 signals (got {}); fp32 is not "
                        "supported".format(dtype))
    e = G.e
    if len(e) < G.N:
        raise ValueError("method='exact' needs the full Fourier basis, but the cached basis has {} of {} vectors; "
                         "call compute_fourier_basis() for the full one".format(len(e), G.N))
    H = np.asarray(bank.evaluate(e), dtype=np.float64).reshape(bank.Nf, G.N)
    N, nsig, nfeat = cube_shape
    synthesis = nfeat != 1
    a = s if on_device else _exact_upload(G, np.asarray(s, dtype=np.float64).reshape(cube_shape))
    hat, ms_gram = _exact_gft(G, a, nsig, nfeat)
    out, ms_apply = _exact_apply(G, hat, H, synthesis)
    hat.free()
    if not on_device:
        a.free()
    _record_timing(G, ms_gram + ms_apply, "exact")
    return out if on_device else out.numpy()


def _filter_device_array(bank, s, cube_shape, coeffs, devices, evaluation=None):
    """The device-resident form of filter_signals: `s` (engine.DeviceArray) is read as `cube_shape`, filtered
    where it lies and returned as a new DeviceArray whose `shape` is what the reference would have returned."""
    from . import engine
    if _device_list(bank.G, devices) is not None:
        raise ValueError("a DeviceArray lives on one GPU: it cannot be combined with a device list")
    dev = _device_graph_of(bank.G)
    if not hasattr(dev, "cheby_filter_dev") or s.ctx is not dev.ctx:
        raise ValueError("the DeviceArray does not live on the context of this graph's device Laplacian")
    if s.dtype != dev.dtype:
        raise ValueError("the DeviceArray holds {} but the graph computes in {}".format(s.dtype, dev.dtype))
    N, nsig, nfeat = cube_shape
    synthesis = nfeat != 1
    x_ptr, keep = s.planes(nsig, nfeat)
    out = engine.DeviceArray.empty(dev.ctx, (N, nsig, 1 if synthesis else bank.Nf), dev.dtype)
    ms, how = 0.0, "recurrence"
    if not synthesis:
        asked = evaluation or _configured_evaluation(bank.G)
        how = choose_evaluation(asked, coeffs, dev.dtype, N, nsig)
        if asked == "auto" and how != "product" and coeffs.shape[0] == 1 and N * nsig * dev.dtype.itemsize >= AUTO_MIN_PANEL_BYTES:
            coeffs = effective_coefficients(coeffs[0], dev.dtype)[np.newaxis, :]  # (see cheby_op)
    if N * nsig and how == "newton":
        ms = dev.newton_filter_dev(*cheb_to_newton(coeffs[0]), x_ptr, out.ptr, nsig, bank.G.lmax)
    elif N * nsig and how == "product":
        ms = dev.program_filter_dev(cheb_to_product(coeffs[0], dev.dtype), x_ptr, out.ptr, nsig, bank.G.lmax)
    elif N * nsig:
        ms = dev.cheby_filter_dev(coeffs, x_ptr, out.ptr, nsig, bank.G.lmax,
                                  _capi.SYNTHESIS if synthesis else _capi.ANALYSIS)
    del keep
    _record_timing(bank.G, ms, how)
    return out


class Filter:
    """A bank of kernels g_i(lambda) on a graph, applied by Chebyshev filtering on the device.

    The public surface is that of pygsp.filters.Filter for this path (filter.py:16-600): ``G``, ``Nf`` /
    ``n_filters`` / ``n_features_in`` / ``n_features_out`` / ``shape``, ``len()``, indexing, ``+``, ``@``,
    ``evaluate``, ``filter`` / ``analyze`` / ``synthesize`` / ``localize`` / ``compute_frame``."""

    def __init__(self, G, kernels):
        self.G = G
        self._kernels = list(kernels) if hasattr(kernels, "__iter__") else [kernels]

    # the bank maps one input feature to len(kernels) output features (filter.py:65-68)
    n_features_in = 1

    @property
    def n_features_out(self):
        return len(self._kernels)

    @property
    def n_filters(self):
        return self.n_features_in * self.n_features_out

    Nf = n_filters

    @property
    def shape(self):
        return self.n_features_out, self.n_features_in

    def __len__(self):
        return self.n_filters

    def __getitem__(self, key):
        return Filter(self.G, self._kernels[key])

    def __add__(self, other):
        return Filter(self.G, self._kernels + other._kernels) if isinstance(other, Filter) else NotImplemented

    def __matmul__(self, other):
        return self.filter(other)

    def __repr__(self):
        return "{}(in={}, out={})".format(type(self).__name__, self.n_features_in, self.n_features_out)

    def evaluate(self, x):
        """Frequency response of every kernel at `x`: shape (Nf,) + x.shape (filter.py:112-144)."""
        at = np.asanyarray(x)
        return np.stack([np.broadcast_to(g(at), at.shape) for g in self._kernels]).astype(np.float64)

    def filter(self, s, method="chebyshev", order=30, devices=None, evaluation=None):
        """Filter signals (analysis or synthesis), filter.py:146-328.

        Shapes follow the reference exactly: `s` is (N,), (N, Nsig) or (N, Nsig, Nfeat) with
        Nfeat in {1, Nf}; a trailing dimension equal to Nf means synthesis.  The result is
        squeezed.  This engine's additions: `devices`, a list of GPU ids to split the signal columns over;
        `s` may be an engine.DeviceArray (G.to_device(x)), and then so is the result (see filter_signals);
        `evaluation` ('recurrence' | 'newton' | 'auto'): how a single filter's polynomial is evaluated in an
        analysis call (default: filters.EVALUATION, see set_evaluation and newton_guard).
        """
        return filter_signals(self, s, method, order, devices, evaluation=evaluation)

    def filter_vjp(self, s, cotangent, order=30):
        """(grad_s, grad_coefficients) of ``self.filter(s, 'chebyshev', order)`` for a cotangent of the shape that
        call returns, in analysis and in synthesis (filter_signals_vjp): how a loss that reads the filtered signals
        changes with `s` and with the bank's (Nf, order + 1) Chebyshev coefficients."""
        return filter_signals_vjp(self, s, cotangent, order)

    def filter_vjp_weights(self, s, cotangent, order=30, pairs=None):
        """The gradient of a loss that reads ``self.filter(s, 'chebyshev', order)`` with respect to the graph's edge
        weights, at fixed G.lmax, for a cotangent of the shape that call returns, in analysis and in synthesis
        (filter_signals_vjp_weights, cheby_op_vjp_weights): (P,) float64, one entry per pair of `pairs` ((2, P),
        edges or not) or per edge of ``G.get_edge_list()``."""
        return filter_signals_vjp_weights(self, s, cotangent, order, pairs)

    def analyze(self, s, method="chebyshev", order=30, devices=None):
        shape = _shape_of(s)
        if len(shape) == 3 and shape[-1] != 1:
            raise ValueError("Last dimension (#features) should be 1, got {}.".format(shape))
        return self.filter(s, method, order, devices=devices)

    def synthesize(self, s, method="chebyshev", order=30, devices=None):
        shape = _shape_of(s)
        if shape[-1] != self.Nf:
            raise ValueError("Last dimension (#features) should be the number of filters "
                             "Nf = {}, got {}.".format(self.Nf, shape))
        return self.filter(s, method, order, devices=devices)

    def tune_placement(self, n_signals, order=30, candidates=32, stride_mb=8000):
        """One-off set-up for a serving loop of single-filter analysis calls of `n_signals` columns at `order`: draw
        `candidates` physical backings for the context's streamed workspaces, run that call (on scratch panels) on each
        and keep the fastest (engine.DeviceGraph.tune_placement; on MI355X the same call runs 0.54-0.60 of 8 TB/s
        depending on which pages back its work panels - profiles/r06_placement.md).  The defaults - 32 candidates with
        8 GB held between two draws - sample the whole card, which is what finds a fast zone on every card measured
        (5-13 s, what bench.py does in its set-up); stride_mb=0 with a handful of candidates takes half a second and
        only helps where fast and slow pages are mixed at the start of the memory.  Results of later calls are
        bit-identical whichever backing is kept.  Returns the report {"launch_ms": [...], "kept": index}."""
        return tune_placement(self, n_signals, order, candidates, stride_mb=stride_mb)

    def localize(self, i, **kwargs):
        """The kernel(s) localised at vertex i: sqrt(N) * filter(delta_i)  (filter.py:350-391)."""
        delta = np.zeros(self.G.N)
        delta[i] = 1.0
        return self.filter(delta, **kwargs) * np.sqrt(self.G.N)

    def compute_frame(self, **kwargs):
        """The (Nf*N, N) matrix whose rows are the localised kernels (filter.py:506-600): the bank applied
        to every delta, i.e. to the identity - N signals, produced on the device panel by panel
        (no N x N identity is ever held or shipped; see frame_panels)."""
        method, order = kwargs.pop("method", "chebyshev"), kwargs.pop("order", 30)
        if kwargs:
            raise TypeError("unexpected arguments {}".format(sorted(kwargs)))
        if method != "chebyshev":
            return self.filter(np.identity(self.G.N), method=method, order=order).T.reshape(-1, self.G.N)
        return frame_panels(self, order)


def tune_placement(bank, n_signals, order=30, candidates=32, coefficients=None, stride_mb=8000):
    """Filter.tune_placement for any object with the reference's Filter attributes (the mirror class or, through
    pygsp_amd.plugin.tune_placement, the real pygsp.filters.Filter): one filter only."""
    from . import engine
    if bank.Nf != 1:
        raise ValueError("placement tuning times a single-filter analysis call (Nf = 1), got Nf = {}".format(bank.Nf))
    coeffs = _as_coeff_matrix((coefficients or compute_cheby_coeff)(bank, m=order))
    dev = _device_graph_of(bank.G)
    x = engine.DeviceArray.from_host(dev.ctx, np.full((bank.G.N, int(n_signals)), 0.7183), dev.dtype)
    y = engine.DeviceArray.empty(dev.ctx, (bank.G.N, int(n_signals), 1), dev.dtype)
    try:
        return dev.tune_placement(coeffs[0], x.ptr, y.ptr, int(n_signals), bank.G.lmax, candidates, stride_mb)
    finally:
        x.free()
        y.free()


def frame_panels(bank, order=30, panel=1024, coefficients=None):
    """compute_frame without the dense identity.  The reference filters np.identity(N) and returns
    ``filter(I).T.reshape(-1, N)`` (filter.py:599-600): row f N + j of the frame is p_f(L) delta_j.  Here columns
    [j0, j0 + w) of the identity are written on the device (gspx_identity_panel_dev), filtered there in one call
    per panel, and only the result crosses PCIe - no N x N identity is built or shipped.  `panel` signals per
    call keep the workspace bounded (w = N would need K+1 panels of N x N).  `bank`: the mirror Filter or the
    real pygsp one (plugin.install(wrap_filter=True)), `coefficients` its compute_cheby_coeff."""
    G, Nf = bank.G, bank.Nf
    coeffs = _as_coeff_matrix((coefficients or compute_cheby_coeff)(bank, m=order))
    dev = _device_graph_of(G)
    frame = np.empty((Nf, G.N, G.N))  # [filter][delta j][vertex]
    total_ms = 0.0
    on_device = hasattr(dev, "ctx") and hasattr(dev, "cheby_filter_dev")
    if on_device:
        elt = np.dtype(dev.dtype).itemsize
        width = min(panel, G.N)
        bx, by = dev.ctx.alloc(max(G.N * width * elt, 16)), dev.ctx.alloc(max(Nf * G.N * width * elt, 16))
    try:
        for j0 in range(0, G.N, panel):
            w = min(panel, G.N - j0)
            if on_device:
                dev.ctx.identity_panel(bx, G.N, j0, w, dev.dtype)
                total_ms += dev.cheby_filter_dev(coeffs, bx.ptr, by.ptr, w, G.lmax)
                y = by.download((Nf, G.N, w), dev.dtype)
            else:  # a stand-in device object (tests): host panel through its array interface
                deltas = np.zeros((G.N, w))
                deltas[j0 + np.arange(w), np.arange(w)] = 1
                y, ms = dev.cheby_filter(coeffs, deltas, G.lmax, _capi.ANALYSIS)
                total_ms += ms
            frame[:, j0:j0 + w, :] = np.swapaxes(y, 1, 2)
    finally:
        if on_device:
            bx.free()
            by.free()
    _record_timing(G, total_ms)
    return frame.reshape(Nf * G.N, G.N)


def frame_norms(bank, order=30, panel=1024, coefficients=None):
    """The squared l2 norms of the frame's rows without the frame: (Nf, N), [f, j] = ||p_f(L) delta_j||^2, i.e. row
    f N + j of compute_frame() squared and summed (features.compute_norm_tig, compute_spectrogram).  Identity panels of
    `panel` columns are written on the device as in frame_panels and leave as their Nf x w squared column norms
    (gspx_cheby_sqnorms_dev): neither the frame nor any Nf x N x w output is formed.  `bank`, `coefficients`: as
    frame_panels."""
    G, Nf = bank.G, bank.Nf
    coeffs = _as_coeff_matrix((coefficients or compute_cheby_coeff)(bank, m=order))
    dev = _device_graph_of(G)
    norms = np.empty((Nf, G.N))
    total_ms = 0.0
    on_device = hasattr(dev, "ctx") and hasattr(dev, "cheby_sqnorms_dev")
    if on_device:
        width = max(1, min(panel, G.N))
        bx = dev.ctx.alloc(max(G.N * width * np.dtype(dev.dtype).itemsize, 16))
    try:
        for j0 in range(0, G.N, panel):
            w = min(panel, G.N - j0)
            if on_device:
                dev.ctx.identity_panel(bx, G.N, j0, w, dev.dtype)
                s, ms = dev.cheby_sqnorms_dev(coeffs, bx.ptr, w, G.lmax)
            else:  # a stand-in device object (tests): host panel through its array interface, squared here
                deltas = np.zeros((G.N, w))
                deltas[j0 + np.arange(w), np.arange(w)] = 1
                y, ms = dev.cheby_filter(coeffs, deltas, G.lmax, _capi.ANALYSIS)
                y = np.asarray(y, dtype=np.float64).reshape(Nf, G.N, w)
                s = np.einsum("fnw,fnw->fw", y, y)
            norms[:, j0:j0 + w] = s
            total_ms += ms
    finally:
        if on_device:
            bx.free()
    _record_timing(G, total_ms)
    return norms


class _HeatKernel:
    """min(exp(-tau x / lmax), 1) / norm; lmax is read from the graph when the kernel is evaluated."""

    def __init__(self, graph, tau, norm=1.0):
        self.graph, self.tau, self.norm = graph, tau, norm

    def __call__(self, x):
        return np.minimum(np.exp(-self.tau * x / self.graph.lmax), 1) / self.norm


class Heat(Filter):
    """Heat kernels g(x) = min(exp(-scale x / lmax), 1), optionally normalised to unit l2 norm over the
    spectrum G.e (heat.py:102-119).  `scale` is one diffusion time or a list of them."""

    def __init__(self, G, scale=10, normalize=False):
        self.scale = list(scale) if hasattr(scale, "__iter__") else [scale]
        self.normalize = normalize
        kernels = []
        for tau in self.scale:
            g = _HeatKernel(G, tau)
            if normalize:
                g.norm = np.linalg.norm(g(G.e))
            kernels.append(g)
        super().__init__(G, kernels)


def compute_log_scales(lmin, lmax, Nscales, t1=1, t2=2):
    """utils.py:312-339: Nscales scales, logarithmically spaced from t2 / lmin down to t1 / lmax."""
    return np.exp(np.linspace(np.log(t2 / lmin), np.log(t1 / lmax), Nscales))


class _MexicanLowPass:
    """1.2 / e * exp(-(x / (0.4 lmin))^4), the scaling-function kernel of the bank."""

    def __init__(self, lmin):
        self.lmin = lmin

    def __call__(self, x):
        return 1.2 * np.exp(-1) * np.exp(-((x / 0.4 / self.lmin) ** 4))


class _MexicanBandPass:
    """t x exp(-t x) (times sqrt(t) when normalised): the scaled Mexican-hat wavelet kernel."""

    def __init__(self, t, normalize):
        self.t, self.gain = t, (np.sqrt(t) if normalize else 1)

    def __call__(self, x):
        return self.gain * (self.t * x) * np.exp(-(self.t * x))


class MexicanHat(Filter):
    """Mexican-hat wavelet bank (mexicanhat.py:55-84): one low-pass 1.2/e * exp(-(x / (0.4 lmin))^4) with
    lmin = lmax / lpfactor fixed at construction, and Nf - 1 band-passes t x exp(-t x) at log-spaced
    scales t."""

    def __init__(self, G, Nf=6, lpfactor=20, scales=None, normalize=False):
        self.lpfactor, self.normalize = lpfactor, normalize
        lmin = G.lmax / lpfactor
        self.scales = compute_log_scales(lmin, G.lmax, Nf - 1) if scales is None else scales
        if len(self.scales) != Nf - 1:
            raise ValueError("len(scales) should be Nf-1.")
        bank = [_MexicanLowPass(lmin)]
        bank.extend(_MexicanBandPass(t, normalize) for t in self.scales)
        super().__init__(G, bank)


# ---- banks defined through the exact path: one kernel moved to every graph frequency -----------------------------
def _check_mother_kernel(graph, kernel):
    if kernel.n_filters != 1:
        raise ValueError("A kernel must be one filter. The passed "
                         "filter bank {} has {}.".format(kernel, kernel.n_filters))
    if kernel.G is not graph:
        raise ValueError("The graph passed to this filter bank must "
                         "be the one used to build the mother kernel.")


def modulation_localized(bank, s, panel=1024, coefficients=None):
    """``Modulation.filter`` with localisation first (modulation.py:170-177), the windowed graph Fourier transform:
    row i of the result is sqrt(N) gft(s * kernel.localize(i)).  The reference loops over the vertices (N Chebyshev
    localisations and N transforms); as matrices it is Y = sqrt(N) (diag(s) T)^T U with T[:, i] = kernel.localize(i)
    = sqrt(N) p(L) delta_i, p the order-30 Chebyshev polynomial ``localize`` uses by default.  Here p(L) of identity
    panels of `panel` columns comes from the Chebyshev path on the float64 device graph (as frame_panels), and each
    panel goes through one Gram against the device copy of U with row scale s (gspx_panel_gram_to_dev), both
    factors sqrt(N) folded into its alpha.  `bank`: the mirror Modulation or the real pygsp one (plugin.install(
    exact=True)), `coefficients` its compute_cheby_coeff.  Returns the (N, N) array, row i = vertex i."""
    from . import fourier
    G, kernel = bank.G, bank._kernels
    s = np.asarray(G._check_signal(s))
    if s.shape != (G.N,):
        raise ValueError("Modulation.filter with localisation first takes one signal of shape ({},), got {}."
                         .format(G.N, s.shape))
    if np.iscomplexobj(s):
        raise TypeError("complex signals are not supported by the exact path")
    if len(G.e) < G.N:
        raise ValueError("Modulation needs the full Fourier basis, but the cached basis has {} of {} vectors; "
                         "call compute_fourier_basis() for the full one".format(len(G.e), G.N))
    coeffs = _as_coeff_matrix((coefficients or compute_cheby_coeff)(kernel, m=30))
    dev, U = _exact_basis(G)
    ctx, N = dev.ctx, G.N
    root = float(np.sqrt(N))
    width = max(1, min(int(panel), N))
    ms = 0.0
    with ctx._temporaries() as tmp:
        deltas, atoms = tmp.alloc(N * width * 8), tmp.alloc(N * width * 8)
        out, scale = tmp.alloc(N * N * 8), tmp.upload(np.ascontiguousarray(s, dtype=np.float64))
        for j0 in range(0, N, width):
            w = min(width, N - j0)
            ctx.identity_panel(deltas, N, j0, w, np.float64)
            ms += dev.cheby_filter_dev(coeffs, deltas.ptr, atoms.ptr, w, G.lmax)
            ms += fourier.panel_gram_to(ctx, N, atoms.ptr, w, w, U.ptr, U.ld, N, out.ptr + 8 * j0 * N, N,
                                        rowscale_ptr=scale.ptr, alpha=root * root)
        y = out.download((N, N), np.float64)
    _record_timing(G, ms, "exact")
    return y


class Modulation(Filter):
    """One mother kernel modulated to every graph frequency (modulation.py:7-177): filter k is the kernel multiplied,
    in the vertex domain, by eigenvector u_k.  Filtering a signal gives its vertex-frequency picture S[i, k]:
    with ``modulation_first=False`` (default) the windowed graph Fourier transform - localise the kernel at vertex i,
    window the signal with it, transform - computed by modulation_localized on the device; with
    ``modulation_first=True`` the N-filter bank ``evaluate`` describes, applied by the exact path.  ``evaluate``
    always describes the modulated (not localised) bank and is defined at the eigenvalues only: NaN elsewhere.
    Needs the full Fourier basis, so graphs up to a few ten thousand vertices."""

    def __init__(self, graph, kernel, modulation_first=False):
        _check_mother_kernel(graph, kernel)
        self.G, self._kernels, self._modulation_first = graph, kernel, modulation_first

    @property
    def n_features_out(self):
        return self.G.n_vertices

    def _response(self):
        """(N, N): row k holds the response of every filter at eigenvalue e[k] (host arithmetic, as the reference's:
        the kernel's inverse transform, times sqrt(N) u_f, transformed back)."""
        if not hasattr(self, "_coefficients"):
            G = self.G
            atom = G.igft(np.squeeze(self._kernels.evaluate(G.e)))
            self._coefficients = G.gft(np.sqrt(G.n_vertices) * G.U * atom[:, np.newaxis])
        return self._coefficients

    def evaluate(self, x):
        table = self._response()
        first = {}
        for k, lam in enumerate(self.G.e):
            first.setdefault(lam, k)
        at = np.asanyarray(x)
        y = np.full((self.n_features_out, at.size), np.nan)
        for i, lam in enumerate(at.ravel()):
            k = first.get(lam)
            if k is not None:
                y[:, i] = table[k]
        return y.reshape((self.n_features_out,) + at.shape)

    def filter(self, s, method="exact", order=None):
        """The vertex-frequency transform of `s` (method and order are accepted and ignored, as in the reference:
        this bank is only defined through the exact path)."""
        if self._modulation_first:
            return super().filter(s, method="exact")
        return modulation_localized(self, s)


class Gabor(Filter):
    """One mother kernel centred at every graph frequency (gabor.py:6-92): filter k is x -> kernel(x - e[k]).  A bank
    of N filters applied by the exact path (whatever `method` says, as in the reference); needs the full Fourier
    basis."""

    def __init__(self, graph, kernel):
        _check_mother_kernel(graph, kernel)
        super().__init__(graph, [lambda x, k=k: kernel.evaluate(x - graph.e[k])[0] for k in range(graph.n_vertices)])

    def filter(self, s, method="exact", order=None):
        return super().filter(s, method="exact")
