"""Host-side checks of what the program tests on the GPU rest on (tests/test_gpu_o_programs_on_tiles.py): the product
forms of program_helpers.POLYNOMIALS still have the step shapes they were chosen for, and the numpy restatement of a
program agrees with the oracle's recurrence.  No GPU.

Measured here (float64, worst over the three random graphs, both Laplacian types and the eight polynomials): product
form 1.2e-13, Newton form 1.3e-14 of max |reference|; the bar is 1e-12.  In float32 (product form) 2.5e-6."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import cheby_oracle as orc
from program_helpers import POLYNOMIALS, RANDOM_GRAPHS, program_shape, random_case, run_program, shapes_for
from pygsp_amd import filters

NAMES = sorted(POLYNOMIALS(2.0))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("lmax", [2.0, 37.3, 700.0])
def test_polynomials_keep_their_program_shapes(dtype, lmax):
    """A change in cheb_to_product (trimming, ordering of the factors) must not thin out what the GPU tests cover:
    steps, two-pass and three-pass steps, whether the first factor is a pair, the kind of the last step - and the
    guard clears every polynomial in both dtypes."""
    polys = POLYNOMIALS(lmax)
    assert sorted(polys) == sorted(shapes_for(dtype)) == NAMES and len(NAMES) == 8
    for name, c in polys.items():
        prog = filters.cheb_to_product(c, dtype)
        assert program_shape(prog) == shapes_for(dtype)[name], (name, program_shape(prog))
        assert prog[0, 2] == 0.0 and np.all(np.isfinite(prog))
        ok, m = filters.product_guard(c, dtype)
        assert ok, (name, m)
    # what the shapes are for: S = 1, a first and a last step of either kind, a program without any three-pass step
    shapes = shapes_for(dtype)
    assert shapes["heat5/1"][0] == 1
    assert {s[3] for s in shapes.values()} == {True, False} and {s[4] for s in shapes.values()} == {True, False}
    assert shapes["real7"][2] == 0 and shapes["heat7/25"][2] >= 7


@pytest.mark.parametrize("lap_type", ["combinatorial", "normalized"])
@pytest.mark.parametrize("graph", sorted(RANDOM_GRAPHS))
def test_restatement_matches_the_oracle(graph, lap_type):
    W, L, lmax = random_case(graph, lap_type)
    x = np.random.default_rng(5).standard_normal((W.shape[0], 3))
    worst = {"product": 0.0, "newton": 0.0}
    for name, c in POLYNOMIALS(lmax).items():
        ref = orc.cheby_op(L, lmax, c, x)
        e = rel_err(run_program(L, lmax, filters.cheb_to_product(c, np.float64), x), ref)
        worst["product"] = max(worst["product"], e)
        assert e < 1e-12, (name, "product", e)
        e = rel_err(run_program(L, lmax, filters.newton_program(*filters.cheb_to_newton(c)), x, old_is_x=True), ref)
        worst["newton"] = max(worst["newton"], e)
        assert e < 1e-12, (name, "newton", e)
    print("restatement against cheby_op, %s %s: product %.2e newton %.2e" % (graph, lap_type, worst["product"], worst["newton"]))


def test_restatement_in_float32_sits_inside_the_gpu_bar():
    """The GPU tests hold float32 results to 2e-4: the same steps in numpy float32 stay 50 times and more below it, so
    the bar leaves room for the device's order of summation and nothing else."""
    worst = 0.0
    for graph in sorted(RANDOM_GRAPHS):
        W, L, lmax = random_case(graph, "combinatorial")
        x = np.random.default_rng(6).standard_normal((W.shape[0], 2)).astype(np.float32)
        for name, c in POLYNOMIALS(lmax).items():
            y = run_program(L, lmax, filters.cheb_to_product(c, np.float32), x, dtype=np.float32)
            assert y.dtype == np.float32
            worst = max(worst, rel_err(y, orc.cheby_op(L, lmax, c, x.astype(np.float64))))
    print("float32 restatement against cheby_op: %.2e" % worst)
    assert worst < 4e-6


def test_gamma_of_the_first_step_is_ignored_in_product_form_only():
    W, L, lmax = random_case("rand65", "combinatorial")
    x = np.random.default_rng(7).standard_normal((65, 2))
    prog = np.array([[0.5, 0.1, 0.7], [0.4, -0.2, 0.3]])
    zeroed = prog.copy()
    zeroed[0, 2] = 0.0
    assert np.array_equal(run_program(L, lmax, prog, x), run_program(L, lmax, zeroed, x))
    assert not np.array_equal(run_program(L, lmax, prog, x, old_is_x=True), run_program(L, lmax, zeroed, x, old_is_x=True))
