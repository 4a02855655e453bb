"""What the numpy restatements of the two FISTA solvers share (learning_helpers.solve, prox_tv_helpers.solve; the device
side is csrc/gspx_fista.hip.h): the momentum step, the stopping rule, and the two tools that keep a comparison of
iteration counts between two implementations meaningful."""
import math

import numpy as np

CRITERIA = ("ATOL", "DTOL", "RTOL", "XTOL", "MAXIT")


def momentum(t):
    """(t_{k+1}, b_{k+1}) from t_k: t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, b_{k+1} = (t_k - 1) / t_{k+1}."""
    tn = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
    return tn, (t - 1.0) / tn


def relative_denominator(cur, prev):
    """What rtol divides by: the current objective, the previous one where that is 0, 1 where both are."""
    return cur if cur != 0 else (prev if prev != 0 else 1.0)


def stopping_rule(cur, prev, dx, it, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200):
    """The name of the first criterion that holds at iteration it >= 1, in the order ATOL, DTOL, RTOL, XTOL, MAXIT,
    or None.  cur, prev: obj_it and obj_{it-1}; dx: ||X_it - X_{it-1}||_F / sqrt(entries); a tolerance of None is
    off."""
    diff = abs(cur - prev)
    if atol is not None and cur < atol:
        return "ATOL"
    if dtol is not None and diff < dtol:
        return "DTOL"
    if rtol is not None and diff / relative_denominator(cur, prev) < rtol:
        return "RTOL"
    if xtol is not None and dx < xtol:
        return "XTOL"
    if it >= maxit:
        return "MAXIT"
    return None


def threshold_between(values, k0):
    """A threshold that values[k0] falls below by a relative 1e-6 and that no value lies within 1e-9 of (relative): a
    criterion 'value < threshold' then fires at the same index on both sides of a comparison."""
    th = values[k0] * (1 + 1e-6)
    assert np.min(np.abs(np.asarray(values) - th)) > 1e-9 * th
    return th


def assert_rule_is_decisive(info, rtol=1e-3, atol=None, dtol=None, xtol=None, maxit=200, margin=1e-6):
    """A condition on the INPUTS of a comparison: at the stopping iteration and at every earlier one, each quantity an
    enabled criterion compares lies at least a relative `margin` away from its threshold, so that rounding
    differences between two implementations cannot move niter or crit.  threshold_between puts a threshold at
    value * (1 + 1e-6), which is that margin exactly up to the rounding of the product: the distance is therefore
    measured against threshold / (1 + margin), with 1e-9 of slack for that rounding."""
    obj, dx = info["objective"], info["dx"]
    for k in range(1, info["niter"] + 1):
        diff = abs(obj[k] - obj[k - 1])
        den = relative_denominator(obj[k], obj[k - 1])
        for value, th in ((obj[k], atol), (diff, dtol), (diff / den, rtol), (dx[k - 1], xtol)):
            if th is not None:
                assert abs(value - th) >= margin * (1 - 1e-9) * abs(th) / (1 + margin), (k, value, th)
