"""The stopping rule that the numpy restatements of both FISTA solvers share (tests/fista_helpers.py), on hand-built
values: the precedence of the criteria, the denominator of the relative one, tolerances that are off, the iteration
cap, and the momentum sequence.  No device."""
import math

import fista_helpers as fh


def test_precedence_when_several_criteria_hold():
    # cur = 1, prev = 1.5: diff = 0.5, diff / cur = 0.5; dx = 0.1; it = maxit
    every = dict(atol=2.0, dtol=1.0, rtol=0.75, xtol=0.2, maxit=7)
    held = ["ATOL", "DTOL", "RTOL", "XTOL", "MAXIT"]
    assert tuple(held) == fh.CRITERIA
    for name, key in zip(held, ("atol", "dtol", "rtol", "xtol")):
        assert fh.stopping_rule(1.0, 1.5, 0.1, 7, **every) == name
        every[key] = None  # switch the winner off: the next in line takes over
    assert fh.stopping_rule(1.0, 1.5, 0.1, 7, **every) == "MAXIT"
    every["maxit"] = 8
    assert fh.stopping_rule(1.0, 1.5, 0.1, 7, **every) is None


def test_each_criterion_compares_strictly():
    assert fh.stopping_rule(1.0, 1.5, 0.1, 1, rtol=None, atol=1.0) is None
    assert fh.stopping_rule(1.0, 1.5, 0.1, 1, rtol=None, dtol=0.5) is None
    assert fh.stopping_rule(1.0, 1.5, 0.1, 1, rtol=0.5) is None
    assert fh.stopping_rule(1.0, 1.5, 0.1, 1, rtol=None, xtol=0.1) is None
    assert fh.stopping_rule(1.0, 1.5, 0.1, 1, rtol=0.5 * (1 + 1e-12)) == "RTOL"


def test_relative_criterion_falls_back_on_the_previous_objective_then_on_one():
    assert fh.relative_denominator(4.0, 2.0) == 4.0
    assert fh.relative_denominator(0.0, 2.0) == 2.0
    assert fh.relative_denominator(0.0, 0.0) == 1.0
    # cur = 0, prev = 2: diff / prev = 1
    assert fh.stopping_rule(0.0, 2.0, 1.0, 1, rtol=1.5) == "RTOL"
    assert fh.stopping_rule(0.0, 2.0, 1.0, 1, rtol=0.9) is None
    # both 0: diff / 1 = 0 is below every positive rtol, and below none that is 0
    assert fh.stopping_rule(0.0, 0.0, 1.0, 1, rtol=1e-300) == "RTOL"
    assert fh.stopping_rule(0.0, 0.0, 1.0, 1, rtol=0.0) is None


def test_a_tolerance_of_none_never_fires():
    # values every numeric tolerance would accept: objective and differences of zero
    assert fh.stopping_rule(0.0, 0.0, 0.0, 1, rtol=None, atol=None, dtol=None, xtol=None, maxit=2) is None
    assert fh.stopping_rule(-1e300, -1e300, 0.0, 1, rtol=None, atol=None, dtol=None, xtol=None, maxit=2) is None
    assert fh.stopping_rule(0.0, 0.0, 0.0, 1, rtol=None, atol=None, dtol=None, xtol=1e-9, maxit=2) == "XTOL"


def test_iteration_cap():
    off = dict(rtol=None, atol=None, dtol=None, xtol=None)
    assert fh.stopping_rule(3.0, 5.0, 1.0, 4, maxit=5, **off) is None
    assert fh.stopping_rule(3.0, 5.0, 1.0, 5, maxit=5, **off) == "MAXIT"
    assert fh.stopping_rule(3.0, 5.0, 1.0, 6, maxit=5, **off) == "MAXIT"


def test_momentum_sequence():
    t, b = fh.momentum(1.0)
    assert (t, b) == ((1.0 + math.sqrt(5.0)) / 2.0, 0.0)
    t2, b2 = fh.momentum(t)
    assert t2 == (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0 and b2 == (t - 1.0) / t2
    for k in range(2, 52):  # t_k >= (k + 2) / 2 (Beck & Teboulle 2009, lemma 4.3) and t_k < t_{k-1} + 1
        tp, (t, b) = t, fh.momentum(t)
        assert (k + 2) / 2.0 <= t < tp + 1.0 and b == (tp - 1.0) / t
