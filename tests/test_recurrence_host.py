"""Host-side checks of what the recurrence tests on the GPU rest on (tests/test_gpu_p_recurrence_on_tiles.py): the numpy
restatement of the three-term recurrence with one accumulator per filter and of the vector-coefficient Clenshaw
synthesis (recurrence_helpers), computed in the compute dtype, agrees with the oracle on the graphs and polynomials of
that module; the synthesis inputs and their reference are what they claim to be; the restated rule of which launches
take the tile kernel gives the counts worked out by hand from gspx_poly.hip.h.  No GPU.

The GPU module's bar is gpu_helpers.TOL * 10 = 1e-10 (float64) / 2e-4 (float32) of max |reference|; the restatement
must stay within a twentieth of it, 5e-12 / 1e-5.  Measured here (worst over the eight graphs and seven polynomials,
analysis and synthesis; the module prints them with -s): float64 6.7e-15, float32 2.2e-6."""
import numpy as np
import pytest

from conftest import rel_err
from gpu_helpers import TOL
from oracle import cheby_oracle as orc
from recurrence_helpers import (POLYNOMIALS, SINGLE, run_clenshaw, run_recurrence, steps, synthesis_inputs,
                                synthesis_reference)
from tile_helpers import BAND_GRAPHS, GRAPHS, expected_kinds_recurrence, graph_matrix

NSIG = 4
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for dt, (err, where) in sorted(_WORST.items()):
        print("\nworst restatement against the oracle, {:<8s} {:.2e} of max |ref| at {}".format(dt, err, where), end="")
    print()


def hold(dtype, y, ref, where):
    """Within a twentieth of the GPU module's bar."""
    dt = np.dtype(dtype)
    assert y.dtype == dt and y.shape == ref.shape, where
    err = rel_err(y.astype(np.float64), ref)
    if err >= _WORST.get(dt.name, (-1.0, None))[0]:
        _WORST[dt.name] = (err, where)
    assert err < TOL[dt] * 10 / 20, (where, err)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("graph", GRAPHS + BAND_GRAPHS)
def test_restatement_matches_the_oracle(graph, dtype):
    W, lap, L, lmax, _, _ = graph_matrix(graph)
    n = W.shape[0]
    x = np.random.default_rng(11).standard_normal((n, NSIG)).astype(np.float32).astype(np.float64)
    for name, c in POLYNOMIALS(lmax).items():
        nf = c.shape[0]
        ref = orc.cheby_op(L, lmax, c, x).reshape(nf, n, NSIG)
        hold(dtype, run_recurrence(L, lmax, c, x, dtype), ref, (graph, name, "analysis"))
        if nf > 1:
            s = synthesis_inputs(x, nf)
            sref = sum(orc.cheby_op(L, lmax, c[f], s[f]) for f in range(nf))  # filter.py:317-321
            hold(dtype, run_clenshaw(L, lmax, c, s, dtype), sref, (graph, name, "synthesis"))


def test_single_filter_clenshaw_is_the_filter():
    """One filter: the Clenshaw recurrence evaluates the same polynomial as the three-term recurrence."""
    W, lap, L, lmax, _, _ = graph_matrix("rand65")
    x = np.random.default_rng(12).standard_normal((65, 3))
    for name in SINGLE:
        c = POLYNOMIALS(lmax)[name]
        assert rel_err(run_clenshaw(L, lmax, c, x[None]), run_recurrence(L, lmax, c, x)[0]) < 1e-13, name


def test_synthesis_inputs_and_their_reference():
    """Panel f is 2^-f times x rotated by 7 f columns - exact in float32 -, the first w columns of every panel are a
    slice of it, and the reference made from the analysis equals the oracle's synthesis of those panels."""
    W, lap, L, lmax, _, _ = graph_matrix("rand65")
    x = np.random.default_rng(13).standard_normal((65, 24)).astype(np.float32).astype(np.float64)
    c = POLYNOMIALS(lmax)["bank3"]
    s = synthesis_inputs(x, 3)
    assert s.shape == (3, 65, 24) and np.array_equal(s.astype(np.float32).astype(np.float64), s)
    assert np.array_equal(s[0], x) and np.array_equal(s[1][:, 0], x[:, 7] / 2) and np.array_equal(s[2][:, 20], x[:, 10] / 4)
    assert len({s[f][:, :5].tobytes() for f in range(3)}) == 3
    direct = sum(orc.cheby_op(L, lmax, c[f], s[f]) for f in range(3))
    made = synthesis_reference(orc.cheby_op(L, lmax, c, x).reshape(3, 65, 24))
    assert rel_err(made, direct) < 1e-15
    assert orc.cheby_op(L, lmax, c[1], s[1][:, :5]).tobytes() == orc.cheby_op(L, lmax, c[1], s[1])[:, :5].tobytes()


def test_polynomials_have_their_step_counts():
    p = POLYNOMIALS(3.7)
    assert [steps(p[name]) for name in SINGLE] == [1, 2, 3, 7, 30] and all(p[name].shape[0] == 1 for name in SINGLE)
    assert p["bank3"].shape == (3, 13) and p["bank2"].shape == (2, 2) and len(p) == 7


def test_the_restated_rule_of_the_recurrence():
    """expected_kinds_recurrence against counts worked out by hand from work_panels, batch_width and the step counts of
    run_batch / run_synthesis_batch (gspx_poly.hip.h)."""
    ek = expected_kinds_recurrence
    # one batch: analysis K steps, Clenshaw K + 1, the per-filter loop nf K
    assert ek(8, 8, 1, 29) == {"tile": 29, "plain": 0}
    assert ek(8, 8, 3, 12) == {"tile": 12, "plain": 0}                                    # deferred combine
    assert ek(8, 8, 3, 12, combine=1) == {"tile": 0, "plain": 12}                         # fused flush of 3 filters
    assert ek(8, 8, 3, 12, combine=2) == {"tile": 12, "plain": 0}
    assert ek(8, 8, 1, 12, combine=1) == {"tile": 12, "plain": 0}                         # one filter: fused on tiles
    assert ek(8, 8, 3, 12, "synthesis") == {"tile": 13, "plain": 0}
    assert ek(8, 8, 3, 12, "synthesis", synthesis=1) == {"tile": 36, "plain": 0}
    assert ek(8, 8, 3, 12, "synthesis", combine=1) == {"tile": 13, "plain": 0}            # (combine: analysis only)
    assert ek(8, 8, 3, 12, "synthesis", tile_gather=0) == {"tile": 0, "plain": 13}
    assert ek(8, 8, 3, 12, "synthesis", synthesis=1, tiles=False) == {"tile": 0, "plain": 36}
    # rows that are not whole pieces: padded, unless tile_pad = 0 - or one column on a small matrix with tile_pad = 1
    for w, elt in ((3, 8), (5, 8), (33, 8), (2, 4), (6, 4), (66, 4)):
        assert ek(w, elt, 1, 6) == {"tile": 6, "plain": 0}, (w, elt)
        assert ek(w, elt, 1, 6, tile_pad=2) == {"tile": 6, "plain": 0}, (w, elt)
        assert ek(w, elt, 1, 6, tile_pad=0) == {"tile": 0, "plain": 6}, (w, elt)
    for elt in (8, 4):
        assert ek(1, elt, 1, 6) == {"tile": 0, "plain": 6}
        assert ek(1, elt, 3, 12, "synthesis") == {"tile": 0, "plain": 13}
        assert ek(1, elt, 1, 6, tile_pad=2) == {"tile": 6, "plain": 0}
        assert ek(1, elt, 1, 6, big_matrix=True) == {"tile": 6, "plain": 0}
        assert ek(1, elt, 1, 6, tile_pad=0, big_matrix=True) == {"tile": 0, "plain": 6}
    assert ek(2, 4, 1, 6, tile_min_row=32) == {"tile": 0, "plain": 6}                     # padded to 16 bytes: too narrow
    # y eight bytes into its buffer: no 16-byte stores into it, so padded work panels of the same pitch
    assert ek(8, 8, 1, 6, y_offset=8) == {"tile": 6, "plain": 0}
    assert ek(8, 8, 1, 6, y_offset=8, tile_pad=0) == {"tile": 0, "plain": 6}
    # column batches of 20 float64 / 40 float32 signals
    assert ek(20, 8, 1, 29, max_batch=2) == {"tile": 290, "plain": 0}                     # ten 16-byte batches
    assert ek(40, 4, 1, 29, max_batch=2) == {"tile": 580, "plain": 0}                     # twenty 8-byte ones, padded
    assert ek(40, 4, 1, 29, max_batch=2, tile_pad=0) == {"tile": 0, "plain": 580}
    assert ek(20, 8, 1, 29, max_batch=8) == {"tile": 87, "plain": 0}                      # 8 + 8 + 4
    assert ek(40, 4, 3, 12, max_batch=8) == {"tile": 60, "plain": 0}                      # five batches, deferred
    assert ek(40, 4, 3, 12, "synthesis", max_batch=8) == {"tile": 65, "plain": 0}
    assert ek(20, 8, 3, 12, "synthesis", max_batch=20) == {"tile": 13, "plain": 0}
    assert ek(20, 8, 3, 12, "synthesis", synthesis=1, max_batch=8) == {"tile": 108, "plain": 0}
    assert ek(21, 8, 1, 6, max_batch=8) == {"tile": 18, "plain": 0}                       # 8 + 8 + 5 into odd rows of y: all padded
    assert ek(21, 8, 1, 6, max_batch=8, tile_pad=0) == {"tile": 0, "plain": 18}
    assert ek(17, 8, 1, 6, max_batch=8) == {"tile": 12, "plain": 6}                       # 8 + 8 + 1: the single column stays plain
