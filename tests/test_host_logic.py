"""Host-side logic of the product that needs no GPU: coefficient quadrature, kernel designs,
filterbank handler, shape algebra (with a stubbed device call), generators, vertex ordering."""
import os

import numpy as np
import pytest
from scipy import sparse

from conftest import csr_from, rel_err
from oracle import cheby_oracle as orc
from pygsp_amd import engine, filters, graphs


class StubGraph:
    """What the host-side filter code reads from a Graph."""

    def __init__(self, L, lmax):
        self.L = L
        self.N = L.shape[0]
        self.lmax = lmax
        self.e = None

    def _check_signal(self, s):
        s = np.asanyarray(s)
        if s.shape[0] != self.N:
            raise ValueError("First dimension must be the number of vertices")
        return s


def test_coefficients_match_reference(golden_logo, golden_sensor123):
    G = StubGraph(csr_from(golden_logo, "L"), float(golden_logo["lmax_bounds"]))
    c = filters.compute_cheby_coeff(filters.Heat(G, scale=50), m=30)
    assert isinstance(c, np.ndarray) and c.shape == (31,)
    np.testing.assert_allclose(c, golden_logo["coeff_bounds"], rtol=1e-13, atol=1e-17)
    G2 = StubGraph(csr_from(golden_sensor123, "Lcomb"), float(golden_sensor123["lmax"]))
    mh = filters.MexicanHat(G2, Nf=6)
    cl = filters.compute_cheby_coeff(mh, m=40)
    assert isinstance(cl, list) and len(cl) == 6  # filterbank_handler: list for Nf > 1
    np.testing.assert_allclose(np.array(cl), golden_sensor123["mh6_c"], rtol=1e-12, atol=1e-16)
    c3 = filters.compute_cheby_coeff(mh, m=40, i=3)
    np.testing.assert_allclose(c3, golden_sensor123["mh6_c"][3], rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(filters.compute_log_scales(1, 10, 3), [2.0, 0.4472136, 0.1], rtol=1e-7)
    with pytest.raises(ValueError):
        filters.MexicanHat(G2, Nf=4, scales=[1.0])


def test_heat_reads_lmax_lazily():
    """heat.py:111-112: lmax is read when the kernel is evaluated, not at construction."""
    G = StubGraph(sparse.identity(4, format="csr"), 2.0)
    h = filters.Heat(G, scale=[1, 5])
    assert h.Nf == 2 and len(h) == 2
    y1 = h.evaluate(np.array([0.0, 1.0, 2.0]))
    G.lmax = 4.0
    y2 = h.evaluate(np.array([0.0, 1.0, 2.0]))
    assert y1.shape == (2, 3) and not np.allclose(y1, y2)
    np.testing.assert_allclose(y2[1], np.exp(-5 * np.array([0.0, 1.0, 2.0]) / 4.0))
    assert isinstance(h[0], filters.Filter) and (h + h).Nf == 4


def test_filter_shape_algebra_with_stubbed_device(monkeypatch, golden_sensor123):
    """Filter.filter's shape rules and synthesis wiring, with the device call replaced by the
    oracle (test-only stub): must reproduce the reference's outputs exactly in shape and value."""
    g = golden_sensor123
    L, lmax = csr_from(g, "Lcomb"), float(g["lmax"])
    G = StubGraph(L, lmax)

    class StubDev:
        def cheby_filter(self, c, x, lm, mode=0):
            if mode == 0:
                r = orc.cheby_op(L, lm, c, x)
                return r.reshape(c.shape[0], G.N, -1), 0.0
            out = sum(orc.cheby_op(L, lm, c[f], x[f]) for f in range(c.shape[0]))
            return out, 0.0

    monkeypatch.setattr(filters, "_device_graph_of", lambda G_: StubDev())
    mh = filters.MexicanHat(G, Nf=6)
    a = mh.filter(g["signals5"], order=40)
    assert a.shape == (123, 5, 6) and rel_err(a, g["mh6_analysis"]) < 1e-13
    assert rel_err(mh.filter(g["mh6_analysis"], order=40), g["mh6_synthesis"]) < 1e-13
    assert rel_err(mh.synthesize(g["mh6_analysis1"], order=40), g["mh6_synthesis1"]) < 1e-13
    h2 = filters.Heat(G, scale=[8, 9])
    assert rel_err(h2.compute_frame(order=30), g["heat89_frame"]) < 1e-13
    with pytest.raises(TypeError):
        filters.Heat(G, 10).filter(g["signal"], order=0)
    with pytest.raises(TypeError):
        filters.cheby_op(G, np.ones(5), g["signal"] * 1j)
    with pytest.raises(ValueError):
        filters.cheby_op(G, np.ones(5), np.ones(124))
    with pytest.raises(NotImplementedError):
        filters.Heat(G, 10).filter(g["signal"], method="exact")
    with pytest.raises(ValueError):
        filters.Heat(G, 10).filter(g["signal"], method="lanczos")


def test_sensor_generator_reproduces_reference_graph(golden_sensor123, golden_doctest):
    """Same RNG stream, same kNN rule, same weights: identical W to graphs.Sensor(N, seed=42)."""
    W, coords = graphs.sensor_weights(123, k=6, seed=42)
    ref = csr_from(golden_sensor123, "W")
    np.testing.assert_array_equal(coords, golden_sensor123["coords"])
    assert (W != ref).nnz == 0 or abs(W - ref).max() < 1e-15
    W30, _ = graphs.sensor_weights(30, k=6, seed=42)
    assert abs(W30 - csr_from(golden_doctest, "W")).max() < 1e-15


def test_sbm_and_er_samplers():
    N, k = 4000, 4
    p, q = 0.02, 0.002
    W, z = graphs.sbm_weights(N, k, p=p, q=q, seed=1)
    assert W.dtype == np.int64 and (W != W.T).nnz == 0 and W.diagonal().sum() == 0
    assert W.max() == 1  # distinct pairs: no duplicate edges
    same = z[:, None] == z[None, :]
    A = W.toarray().astype(bool)
    iu = np.triu_indices(N, 1)
    p_hat = A[iu][same[iu]].mean()
    q_hat = A[iu][~same[iu]].mean()
    assert abs(p_hat - p) < 0.1 * p and abs(q_hat - q) < 0.15 * q
    We, _ = graphs.sbm_weights(3000, 1, np.zeros(3000, dtype=np.int64), 0.01, 0, seed=2)
    deg = np.ravel(We.sum(0))
    assert abs(deg.mean() - 0.01 * 2999) < 1.0


def test_locality_order_is_a_permutation_and_local():
    W, coords = graphs.sensor_weights(5000, k=6, seed=3)
    perm = engine.locality_order(W, coords)
    assert sorted(perm.tolist()) == list(range(5000))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(5000)
    coo = W.tocoo()
    before = np.median(np.abs(coo.row - coo.col))
    after = np.median(np.abs(inv[coo.row] - inv[coo.col]))
    assert after < before / 50  # Morton order: neighbours become close in index
    rcm = engine.locality_order(W, None)
    assert sorted(rcm.tolist()) == list(range(5000))


def test_newton_form_is_the_same_polynomial(golden_sensor123):
    """cheb_to_newton: exact change of basis - checked at random points against the Chebyshev
    series (evaluated in exact rational arithmetic), and end to end against the oracle with a
    numpy Horner evaluation."""
    from fractions import Fraction
    lmax = float(golden_sensor123["lmax"])
    L = csr_from(golden_sensor123, "Lcomb")
    for scale, K in ((10, 30), (50, 30), (50, 50), (200, 40), (3, 1), (3, 2)):
        c = orc.compute_cheby_coeff(orc.heat_kernel(scale, lmax), lmax, K)
        nodes, d = filters.cheb_to_newton(c)
        assert nodes.shape == (K,) and d.shape == (K + 1,)
        assert len(set(nodes.tolist())) == K and np.all(np.abs(nodes) <= 1)
        for t in (Fraction(-1), Fraction(1, 3), Fraction(7, 8), Fraction(-5, 9)):
            t0, t1 = Fraction(1), t
            ref = Fraction(float(c[0])) / 2 + Fraction(float(c[1])) * t1
            for k in range(2, K + 1):
                t0, t1 = t1, 2 * t * t1 - t0
                ref += Fraction(float(c[k])) * t1
            val, prod = Fraction(0), Fraction(1)
            for j in range(K + 1):
                val += Fraction(float(d[j])) * prod
                if j < K:
                    prod *= t - Fraction(float(nodes[j]))
            scale_ref = max(abs(ref), Fraction(1, 10 ** 12))
            assert abs(val - ref) / scale_ref < Fraction(1, 10 ** 9) or abs(val - ref) < Fraction(1, 10 ** 13)
        # Horner evaluation with the actual matrix, float64
        N = L.shape[0]
        Lt = (L - (lmax / 2) * sparse.eye(N)) / (lmax / 2)
        x = golden_sensor123["signals5"]
        h = d[K] * x
        for j in range(K - 1, -1, -1):
            h = Lt.dot(h) - nodes[j] * h + d[j] * x
        assert rel_err(h, orc.cheby_op(L, lmax, c, x)) < 1e-13
    with pytest.raises(TypeError):
        filters.cheb_to_newton(np.array([1.0]))
    with pytest.raises(ValueError):
        filters.set_evaluation("fancy")


def test_jackson_coefficients(golden_sensor123):
    g = golden_sensor123
    b = list(g["rect_bounds"])
    keep = list(b)
    ch, jch = filters.compute_jackson_cheby_coeff(b, [0, float(g["lmax"])], 30)
    np.testing.assert_allclose(ch, g["jackson_ch"], rtol=1e-13, atol=1e-16)
    np.testing.assert_allclose(jch, g["jackson_jch"], rtol=1e-13, atol=1e-16)
    assert b == keep  # the caller's list is left alone
    with pytest.raises(ValueError):
        filters.compute_jackson_cheby_coeff([0.1, 5.0], [0.0, 2.0], 10)
    with pytest.raises(ValueError):
        filters.cheby_rect(None, [1.0], np.ones(3))


def test_auto_order_keeps_already_local_graphs():
    W, coords = graphs.sensor_weights(20000, k=6, seed=5)
    assert engine.auto_order(W, coords) is not None          # random vertex order -> Morton
    assert engine.auto_order(W, None) is not None            # no coordinates -> RCM helps
    perm = engine.locality_order(W, coords)
    Wm = W[perm][:, perm].tocsr()                            # already Morton-ordered graph
    assert engine.auto_order(Wm, None) is None               # RCM would not improve it
    assert engine.locality_score(Wm) > 0.95 > engine.locality_score(W) + 0.3


def test_use_backend_patches_and_restores_both_lookup_sites(monkeypatch):
    """plugin.use_backend / install / uninstall on a pygsp-shaped module: the function looked up at call time
    (filter.py:309, 319 -> approximations.cheby_op) and the import-time alias (filters/__init__.py:115) are
    both replaced and both restored; PYGSP_AMD_BACKEND is honoured at import.  No device is touched."""
    import importlib
    import sys
    import types

    from pygsp_amd import plugin

    def make():
        mod = types.ModuleType("pygsp")
        mod.filters = types.ModuleType("pygsp.filters")
        mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
        orig = lambda G, c, s, **kw: "reference"  # noqa: E731
        mod.filters.approximations.cheby_op = orig
        mod.filters.cheby_op = orig
        return mod, orig

    mod, orig = make()
    plugin.use_backend("gspx", mod)
    assert mod.filters.approximations.cheby_op is filters.cheby_op and mod.filters.cheby_op is filters.cheby_op
    plugin.use_backend("reference", mod)
    assert mod.filters.approximations.cheby_op is orig and mod.filters.cheby_op is orig
    plugin.use_backend("reference", mod)  # idempotent
    with pytest.raises(ValueError):
        plugin.use_backend("scipy", mod)
    with pytest.raises(ValueError):
        plugin.install(mod, laplacian="elsewhere")
    # environment switch, read when the module is imported
    mod2, orig2 = make()
    monkeypatch.setitem(sys.modules, "pygsp", mod2)
    monkeypatch.setenv("PYGSP_AMD_BACKEND", "gspx")
    importlib.reload(plugin)
    try:
        assert mod2.filters.approximations.cheby_op is filters.cheby_op
    finally:
        plugin.uninstall(mod2)
        monkeypatch.delenv("PYGSP_AMD_BACKEND")
        importlib.reload(plugin)
    assert mod2.filters.cheby_op is orig2


def test_bench_refuses_gpus_it_cannot_see():
    """`python bench.py --gpus 2` on a box that cannot provide two devices (here: none) exits non-zero with a
    one-line reason instead of reporting a smaller run under a larger n_gpus."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1"], cwd=root, env=env,
                         capture_output=True, text=True, timeout=300)
    from pygsp_amd import _capi
    if _capi.device_count() >= 2:
        pytest.skip("two devices visible here")
    assert res.returncode != 0 and "refusing" in res.stderr
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith("{")]


def test_bench_plain_run_leaves_the_extras_to_full(monkeypatch):
    """A plain `bench.py` run skips every extra, as if each --no-* option had been given; --full runs them all unless
    a --no-* option says otherwise; --no-headline (configs only) is part of --full."""
    import subprocess
    import sys

    import bench
    extras = ("no_cpu", "no_gather", "no_newton", "no_mix", "no_e2e", "no_configs", "no_f32", "no_chain", "no_live_traffic")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and all(getattr(a, k) for k in extras) and a.cpu_all_cores == 0
    assert (a.steps, a.warmup, a.tune_candidates, a.evaluation) == (4, 2, 32, "recurrence")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-f32"])
    a = bench.parse()
    assert a.full and a.no_f32 and not any(getattr(a, k) for k in extras if k != "no_f32") and a.cpu_all_cores == -1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--no-headline", "--only-config", "c1"], cwd=root,
                         env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--full" in res.stderr
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith("{")]


def test_expander_like_tells_random_graphs_from_embedded_ones():
    """engine.expander_like: balls of a random graph (ER, SBM) grow by the mean degree per hop, those of a k-NN graph
    or a grid by a factor near 2 - the test that lets random graphs skip the reverse Cuthill-McKee pass."""
    W_er, _ = graphs.sbm_weights(60000, k=1, p=10 / 60000, seed=0)
    W_sbm, _ = graphs.sbm_weights(60000, k=8, p=8 * 12 / 60000, q=4.0 * 8 / (60000 * 7), seed=0)
    W_knn, _ = graphs.sensor_weights(60000, k=8, seed=1)
    assert engine.expander_like(W_er) and engine.expander_like(W_sbm)
    assert not engine.expander_like(W_knn)
    perm = np.random.default_rng(1).permutation(60000)
    assert not engine.expander_like(W_knn[perm][:, perm].tocsr())  # a scrambled vertex order does not fool it
    n = 200
    idx = np.arange(n * n).reshape(n, n)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    grid = sparse.csr_matrix((np.ones(r.size), (r, c)), shape=(n * n, n * n))
    assert not engine.expander_like(sparse.csr_matrix(grid + grid.T))
    assert not engine.expander_like(sparse.csr_matrix((100, 100)))  # empty / tiny graphs: no opinion


def test_graph_keeps_a_device_adjacency_until_w_is_read(monkeypatch):
    """Host logic of the generator hand-over (graphs.Graph with an engine.DeviceAdjacency; the device calls replaced by
    stand-ins): the set-up runs on the handle, facts that do not need the matrix (N, edge count, directedness) come
    from its report, G.W downloads exactly once and releases the handle; a W the device route declines (directed)
    is downloaded first and takes the ordinary constructor."""
    W = sparse.csr_matrix(np.array([[0, 1, 2.0], [1, 0, 0], [2, 0, 0]]))
    downloads = []

    class FakeAdjacency(engine.DeviceAdjacency):
        def __init__(self, host):
            self._h, self.ctx, self.shape, self.nnz, self.weights, self._host = None, None, host.shape, host.nnz, np.dtype(np.float64), None
            self._src = host

        def download(self):
            downloads.append(1)
            return self._src

    class FakeDev:
        ctx = None

        def auto_gather_tiles(self):
            return {"enabled": False}

    report = {"self_loops": 0, "negative": 0, "zeros": 0, "asymmetric": 0, "reordered": False, "built": True}
    monkeypatch.setattr(engine.DeviceGraph, "setup_from",
                        classmethod(lambda cls, adj, lap, dt, coords, order: (FakeDev(), dict(report))))
    G = graphs.Graph(FakeAdjacency(W))
    assert G._adj_dev is not None and downloads == [] and G.N == 3 and G.n_edges == 2 and not G.is_directed()
    assert abs(G.W - W).nnz == 0 and downloads == [1] and G._adj_dev is None
    assert G.W is G.W and downloads == [1]
    # declined by the device route: the matrix is fetched and the host route builds the graph
    monkeypatch.setattr(engine.DeviceGraph, "setup_from", classmethod(lambda cls, *a: (None, dict(report))))
    built = []
    monkeypatch.setattr(graphs.Graph, "_setup_on_device", lambda self, adj: False)
    monkeypatch.setattr(graphs.Graph, "compute_laplacian", lambda self, lap_type="combinatorial": built.append(lap_type))
    downloads.clear()
    H = graphs.Graph(FakeAdjacency(W))
    assert downloads == [1] and H._adj_dev is None and H.n_edges == 2 and built == ["combinatorial"]


def test_cube_shape_truth_table():
    """filters._cube_shape = the shape rules of Filter.filter (filter.py:267-290; SURVEY 8(b) truth table, N = 40) on
    shapes alone - what the wrapped real Filter.filter and the DeviceArray path decide analysis / synthesis with."""
    N = 40

    class G:
        pass

    G.N = N
    table = [((N,), (N, 1, 1), (N, 1, 1)), ((N, 1), (N, 1, 1), (N, 1, 1)), ((N, 1, 1), (N, 1, 1), (N, 1, 1)),
             ((N, 4), (N, 4, 1), (N, 4, 1)), ((N, 4, 1), (N, 4, 1), (N, 4, 1)),
             ((N, 6), (N, 6, 1), (N, 1, 6)), ((N, 1, 6), ValueError, (N, 1, 6)), ((N, 4, 6), ValueError, (N, 4, 6)),
             ((N, 6, 6), ValueError, (N, 6, 6)), ((N, 6, 1), (N, 6, 1), (N, 6, 1)), ((N, 4, 3), ValueError, ValueError),
             ((N, 2, 2, 1), ValueError, ValueError), ((N + 1,), ValueError, ValueError), ((), ValueError, ValueError),
             ((N, 0), (N, 0, 1), (N, 0, 1))]
    for shape, one, six in table:
        for nf, expect in ((1, one), (6, six)):
            if expect is ValueError:
                with pytest.raises(ValueError):
                    filters._cube_shape(G, nf, shape)
            else:
                assert filters._cube_shape(G, nf, shape) == expect, (shape, nf)
    with pytest.raises(ValueError, match="At most 3 dimensions"):
        filters._cube_shape(G, 1, (N, 2, 2, 1))
    with pytest.raises(ValueError, match="First dimension must be the number of vertices"):
        filters._cube_shape(G, 6, (N + 1, 6))
    with pytest.raises(ValueError, match="Third dimension"):
        filters._cube_shape(G, 6, (N, 4, 3))
    # _shape_of never touches the data of an object that carries its shape (a DeviceArray would be downloaded)

    class Shaped:
        shape = (N, 3)

        def __array__(self, *a, **k):
            raise AssertionError("downloaded")

    assert filters._shape_of(Shaped()) == (N, 3) and filters._shape_of([[1, 2], [3, 4]]) == (2, 2)


def test_device_array_views_without_a_device():
    """engine.DeviceArray's shape bookkeeping (no device needed: a stand-in buffer): cube vs squeezed shape, the
    as-given shape of an upload, and that a tensor is handed out as-is when the call reads it the way it is stored."""
    class Buf:
        ctx = object()
        nbytes = 0

        def free(self):
            self.freed = True

    a = engine.DeviceArray(Buf(), (40, 1, 6), np.float64)
    assert a.shape == (40, 6) and a.ndim == 2 and a.size == 240 and a.nbytes == 1920 and len(a) == 40
    b = engine.DeviceArray(Buf(), (40, 5, 1), np.float32)
    assert b.shape == (40, 5) and b.nbytes == 800
    assert engine.DeviceArray(Buf(), (40, 1, 1), np.float64).shape == (40,)
    with pytest.raises(ValueError):
        a.planes(4, 2)  # 6 elements per vertex cannot be read as 4 x 2
    buf = a._buf
    a.free()
    assert buf.freed and a._buf is None
    with pytest.raises(ValueError):
        a.ptr


def test_install_wraps_and_restores_the_filter_methods():
    """plugin.install(wrap_filter=...) on a pygsp-shaped module (no device needed: nothing is filtered): the secondary
    seam replaces Filter.filter / Filter.compute_frame, wrap_filter=False and uninstall() put the package's own methods
    back, repeated installs keep the ORIGINAL methods (not a wrapper of a wrapper), and a package without a Filter
    class (or without compute_cheby_coeff) gets the primary seam alone."""
    import types

    from pygsp_amd import plugin

    def make(with_filter=True):
        mod = types.ModuleType("pygsp")
        mod.filters = types.ModuleType("pygsp.filters")
        mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
        mod.filters.approximations.cheby_op = mod.filters.cheby_op = lambda G, c, s, **kw: "reference"
        mod.filters.approximations.compute_cheby_coeff = lambda f, m=30: np.ones(m + 1)
        if with_filter:
            class Filter:
                def filter(self, s, method="chebyshev", order=30):
                    return "own filter"

                def compute_frame(self, **kwargs):
                    return "own frame"
            mod.filters.Filter = Filter
        return mod

    mod = make()
    own_filter, own_frame = mod.filters.Filter.filter, mod.filters.Filter.compute_frame
    try:
        plugin.install(mod)
        assert mod.filters.Filter.filter is plugin._filter_on_device
        assert mod.filters.Filter.compute_frame is plugin._compute_frame_on_device
        plugin.install(mod, dtype=np.float32)  # again: the saved originals are still the package's own
        plugin.install(mod, wrap_filter=False)
        assert mod.filters.Filter.filter is own_filter and mod.filters.Filter.compute_frame is own_frame
        assert mod.filters.approximations.cheby_op is filters.cheby_op  # the primary seam stays
        plugin.install(mod)
        # everything but Chebyshev is answered by the package's own code, through the wrapper
        assert mod.filters.Filter().filter(np.zeros(3), method="exact") == "own filter"
        assert mod.filters.Filter().compute_frame(method="exact") == "own frame"
        plugin.uninstall(mod)
        assert mod.filters.Filter.filter is own_filter and mod.filters.Filter.compute_frame is own_frame
        assert mod.filters.cheby_op(None, None, None) == "reference"
        bare = make(with_filter=False)
        plugin.install(bare)
        assert bare.filters.cheby_op is filters.cheby_op and not hasattr(bare.filters, "Filter")
        plugin.uninstall(bare)
        # two pygsp-shaped modules patched at once: each keeps and gets back ITS OWN originals, a wrapped
        # method answers with its own package's code and coefficients, and uninstalling one leaves the other patched
        one, two = make(), make()
        two.filters.Filter.filter = lambda self, s, method="chebyshev", order=30: "filter of two"
        two.filters.approximations.compute_cheby_coeff = lambda f, m=30: np.full(m + 1, 2.0)
        own_one, own_two = one.filters.Filter.filter, two.filters.Filter.filter
        ref_one, ref_two = one.filters.approximations.cheby_op, two.filters.approximations.cheby_op
        plugin.install(one)
        plugin.install(two)
        assert one.filters.Filter().filter(None, method="exact") == "own filter"
        assert two.filters.Filter().filter(None, method="exact") == "filter of two"
        assert plugin._reference_coefficients(one.filters.Filter(), 3).tolist() == [1.0] * 4
        assert plugin._reference_coefficients(two.filters.Filter(), 3).tolist() == [2.0] * 4
        plugin.uninstall(one)
        assert one.filters.Filter.filter is own_one and one.filters.approximations.cheby_op is ref_one
        assert two.filters.Filter.filter is plugin._filter_on_device and two.filters.cheby_op is filters.cheby_op
        plugin.uninstall()  # no argument: the module patched last that is still patched
        assert two.filters.Filter.filter is own_two and two.filters.approximations.cheby_op is ref_two
        assert not plugin._installed
        plugin.uninstall(two)  # nothing left to restore: a no-op
    finally:
        plugin.uninstall(mod)
        plugin._config.update(dtype=np.dtype(np.float64))


def test_install_flags_patch_and_restore_every_seam_through_one_table():
    """plugin.install() on a pygsp-shaped module with every seam (no device needed: nothing is called): each optional
    seam - lanczos_op, features, learning, compute_fourier_basis, estimate_lmax - follows its flag from one install to
    the next while cheby_op and Filter.filter stay patched, and uninstall() after any sequence of installs leaves every
    touched object with the package's own attributes and without a save table."""
    import itertools
    import types

    from pygsp_amd import plugin

    def make(with_lanczos=True):
        mod = types.ModuleType("pygsp")
        mod.filters = types.ModuleType("pygsp.filters")
        approx = mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
        approx.cheby_op = mod.filters.cheby_op = lambda G, c, s, **kw: "reference"
        approx.compute_cheby_coeff = lambda f, m=30: np.ones(m + 1)
        if with_lanczos:
            approx.lanczos_op = mod.filters.lanczos_op = lambda f, s, order=30: "reference lanczos"

        class Filter:
            def filter(self, s, method="chebyshev", order=30):
                return "own filter"

            def compute_frame(self, **kwargs):
                return "own frame"

        class Graph:
            def estimate_lmax(self, method="lanczos"):
                return "own lmax"

            def compute_fourier_basis(self, n_eigenvectors=None):
                return "own basis"

        mod.filters.Filter = Filter
        mod.graphs = types.ModuleType("pygsp.graphs")
        mod.graphs.Graph = Graph
        mod.features = types.ModuleType("pygsp.features")
        mod.features.compute_tig = lambda g, **k: "own tig"
        mod.features.compute_norm_tig = lambda g, **k: "own norm tig"
        mod.features.compute_spectrogram = lambda G, atom=None, M=100, **k: "own spectrogram"
        mod.learning = types.ModuleType("pygsp.learning")
        mod.learning.regression_tikhonov = lambda G, y, M, tau=0: "own regression"
        mod.learning.classification_tikhonov_simplex = lambda G, y, M, tau=0.1, **k: "own simplex"
        mod.learning.classification_tikhonov = lambda G, y, M, tau=0: "own classification"
        return mod

    def touched(mod):
        return (mod.filters.approximations, mod.filters, mod.filters.Filter, mod.graphs.Graph, mod.features,
                mod.learning)

    def attributes(mod):
        return {(i, n): v for i, obj in enumerate(touched(mod)) for n, v in vars(obj).items() if callable(v)}

    def assert_untouched(mod, own):
        now = attributes(mod)
        assert now.keys() == own.keys()
        for key in own:
            assert now[key] is own[key], key
        for obj in touched(mod):
            assert plugin._SAVED not in vars(obj), obj

    mod = make()
    own = attributes(mod)
    approx, Graph, feats, learn = mod.filters.approximations, mod.graphs.Graph, mod.features, mod.learning
    optional = ((approx, "lanczos_op"), (mod.filters, "lanczos_op"), (feats, "compute_norm_tig"),
                (feats, "compute_spectrogram"), (learn, "regression_tikhonov"),
                (learn, "classification_tikhonov_simplex"), (Graph, "compute_fourier_basis"), (Graph, "estimate_lmax"))
    try:
        plugin.install(mod, lanczos=True, features=True, learning=True, fourier=True, lmax="device")
        assert approx.lanczos_op is filters.lanczos_op and mod.filters.lanczos_op is filters.lanczos_op
        assert Graph.compute_fourier_basis is plugin._compute_fourier_basis_on_device
        assert Graph.estimate_lmax is plugin._estimate_lmax_on_device
        for obj, name in optional:
            assert getattr(obj, name) is not own[touched(mod).index(obj), name], name
        plugin.install(mod)  # the defaults: each of the five goes back to the package's own object ...
        for obj, name in optional:
            assert getattr(obj, name) is own[touched(mod).index(obj), name], name
        for obj in (Graph, feats, learn):
            assert plugin._SAVED not in vars(obj)
        # ... while the primary and the secondary seam stay
        assert approx.cheby_op is filters.cheby_op and mod.filters.cheby_op is filters.cheby_op
        assert mod.filters.Filter.filter is plugin._filter_on_device
        assert mod.filters.Filter.compute_frame is plugin._compute_frame_on_device
        assert mod.filters.Filter().filter(None, method="exact") == "own filter"
        plugin.uninstall(mod)
        assert_untouched(mod, own)
        # any sequence of installs, then one uninstall
        flag_sets = [dict(lanczos=a, features=b, learning=c, fourier=d, lmax=e, wrap_filter=f)
                     for a, b, c, d, e, f in itertools.product((False, True), (False, True), (False, True),
                                                               (False, True), ("reference", "device"), (True, False))]
        for first, second in ((0, 63), (63, 0), (21, 42), (42, 21), (63, 63), (5, 58), (36, 27)):
            plugin.install(mod, **flag_sets[first])
            plugin.install(mod, **flag_sets[second])
            plugin.uninstall(mod)
            assert_untouched(mod, own)
        for flags in flag_sets:
            plugin.install(mod, **flags)
        plugin.uninstall(mod)
        assert_untouched(mod, own)
        plugin.uninstall(mod)  # nothing left to restore: a no-op
        assert_untouched(mod, own)
        # a package without lanczos_op: there is no original to put back, and no table stays behind either
        bare = make(with_lanczos=False)
        own_bare = attributes(bare)
        plugin.install(bare, lanczos=True)
        assert bare.filters.approximations.lanczos_op is filters.lanczos_op
        plugin.install(bare)
        plugin.uninstall(bare)
        for obj in touched(bare):
            assert plugin._SAVED not in vars(obj)
        now = attributes(bare)
        for key in own_bare:
            assert now[key] is own_bare[key], key
    finally:
        plugin.uninstall(mod)


def test_device_array_pool_is_locked_and_gives_way_to_allocations():
    """the recycled-buffer pool of a Context (take / give) is mutated from DeviceArray.__del__ and from
    user threads - one lock - and must never be the reason an allocation fails: Context.call() empties it and runs a
    failed call once more.  No device needed: the pool logic with stand-in buffers."""
    import threading
    from pygsp_amd import _capi, engine
    ctx = engine.Context.__new__(engine.Context)  # no device: only the pool is exercised
    ctx._h = None
    ctx._init_pool()

    class Buf:
        def __init__(self, n):
            self._h, self.ctx, self.nbytes, self.freed = 1, ctx, n, False

        def free(self):
            self.freed, self._h = True, None

    b = Buf(100)
    ctx.give(b)
    assert ctx.pooled_bytes() == 100 and ctx.take(100) is b and ctx.pooled_bytes() == 0
    big = Buf(ctx.POOL_BYTES + 1)
    ctx.give(big)  # beyond the cap: freed, not kept
    assert big.freed and ctx.pooled_bytes() == 0
    # a failing allocation with buffers in the pool: pool emptied, call repeated once
    kept = [Buf(64), Buf(64), Buf(32)]
    for k in kept:
        ctx.give(k)
    calls = []

    def alloc(*args):
        calls.append(args)
        return _capi.ERR_OOM if len(calls) == 1 else _capi.OK
    ctx.call(alloc, 1, 2)
    assert calls == [(1, 2), (1, 2)] and ctx.pooled_bytes() == 0 and all(k.freed for k in kept)
    # nothing in the pool: no second attempt, the failure surfaces as the library's exception
    calls.clear()
    with pytest.raises(_capi.GspxError):
        ctx.call(lambda *a: calls.append(a) or _capi.ERR_OOM)
    assert len(calls) == 1
    # a HIP failure that is not an allocation failure is never retried (the call may have written already: ADVICE r5)
    ctx.give(Buf(8))
    calls.clear()
    with pytest.raises(_capi.GspxError):
        ctx.call(lambda *a: calls.append(a) or _capi.ERR_HIP)
    assert len(calls) == 1 and ctx.pooled_bytes() == 8
    ctx.clear_pool()
    # argument errors are never retried
    ctx.give(Buf(8))
    calls.clear()
    with pytest.raises(ValueError):
        ctx.call(lambda *a: calls.append(a) or _capi.ERR_INVALID)
    assert len(calls) == 1 and ctx.pooled_bytes() == 8
    ctx.clear_pool()
    # many threads giving and taking: the byte count stays exact
    def take_or_new(n):  # Context.take without the device allocation behind it
        with ctx._pool_lock:
            stack = ctx._pool.get(n)
            if stack:
                ctx._pooled -= n
                return stack.pop()
        return Buf(n)

    def worker(seed):
        mine = []
        for i in range(300):
            if mine and (i + seed) % 3 == 0:
                ctx.give(mine.pop())
            else:
                mine.append(take_or_new(16))
        for m in mine:
            ctx.give(m)
    ts = [threading.Thread(target=worker, args=(s,)) for s in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    with ctx._pool_lock:
        assert ctx._pooled == 16 * sum(len(v) for v in ctx._pool.values())
    ctx.clear_pool()
    assert ctx.pooled_bytes() == 0


def test_newton_guard_and_auto_evaluation(golden_sensor123, monkeypatch):
    """VERDICT r5 "Next 2c/2d": the host-side guard of the Newton evaluation and evaluation='auto'.  The guard clears
    the Heat / Mexican-hat polynomials on Leja-ordered nodes, trips on overflow (fp32 at order 200: d_j ~ 2^j) and on
    a constructed ill-conditioned Newton form (the same nodes in sorted order - the textbook unstable case -, where
    the Horner evaluation really is wrong by orders of magnitude more than the threshold); 'auto' takes Newton only
    for one filter, analysis, one device, a panel beyond the launch-bound sizes, and a cleared polynomial."""
    lmax = 22.1
    for kern in [orc.heat_kernel(50, lmax), orc.heat_kernel(10, lmax)] + orc.mexican_hat_kernels(lmax, 6):
        for order in (30, 50, 100, 200):
            c = orc.compute_cheby_coeff(kern, lmax, order)
            ok64, m64 = filters.newton_guard(c, np.float64)
            assert ok64 and m64["grid_err"] < 1e-14 and m64["amplification"] < 200, m64
            ok32, m32 = filters.newton_guard(c, np.float32)
            if order <= 100:
                assert ok32 and m32["grid_err"] < 5e-6, m32
            else:
                assert not ok32 and m32["reason"] == "overflow", m32
    # the constructed ill-conditioned case: Newton form on SORTED Chebyshev nodes
    c = orc.compute_cheby_coeff(orc.heat_kernel(50, lmax), lmax, 60)
    nodes, d = filters.cheb_to_newton(c, ordering="sorted")
    bad = filters.newton_stability(c, np.float64, nodes, d)
    assert bad["finite"] and bad["grid_err"] > 1e-8 and bad["eps_amplification"] > 1e-6, bad
    good = filters.newton_stability(c, np.float64)
    assert good["grid_err"] < 1e-14 and good["eps_amplification"] < 1e-13, good
    # ... and the guard's verdict on it, through the same thresholds newton_guard applies
    lim_grid, lim_amp = filters.NEWTON_GUARD[np.dtype(np.float64)]
    assert bad["grid_err"] > lim_grid and 8 * bad["eps_amplification"] > lim_amp
    monkeypatch.setattr(filters, "cheb_to_newton", lambda cc, ordering="leja": (nodes, d))
    filters._guard_cache.clear()
    ok, m = filters.newton_guard(c, np.float64)
    assert not ok and m["reason"] in ("grid", "amplification")
    monkeypatch.undo()
    filters._guard_cache.clear()
    assert not filters.newton_guard(np.array([1.0, np.nan, 0.5]), np.float64)[0]
    # choose_evaluation
    c1, c6 = np.atleast_2d(c), np.tile(c, (6, 1))
    big = (1000000, 64)
    assert filters.choose_evaluation("auto", c1, np.float64, *big) == "product"          # (order 60 Heat(50): both cleared)
    monkeypatch.setattr(filters, "product_guard", lambda cc, dt=np.float64: (False, {"reason": "test"}))
    assert filters.choose_evaluation("auto", c1, np.float64, *big) == "newton"             # product refused: Newton
    monkeypatch.undo()
    assert filters.choose_evaluation("auto", c6, np.float64, *big) == "recurrence"          # a bank
    assert filters.choose_evaluation("auto", c1, np.float64, 100000, 1) == "recurrence"     # launch-bound: hipGraph replay
    assert filters.choose_evaluation("auto", c1, np.float64, *big, split=True) == "recurrence"
    assert filters.choose_evaluation("recurrence", c1, np.float64, *big) == "recurrence"
    assert filters.choose_evaluation("newton", c1, np.float64, 100, 1) == "newton"           # explicit: always
    # (a series that has NOT converged by its order - the Mexican-hat low-pass: all 200 terms count; Heat(50) at order
    # 200 is 41 terms to 'auto', in every form: filters.effective_coefficients)
    c200 = np.atleast_2d(orc.compute_cheby_coeff(orc.mexican_hat_kernels(lmax, 6)[0], lmax, 200))
    assert filters.effective_coefficients(c200[0], np.float32).size == 201
    heat200 = orc.compute_cheby_coeff(orc.heat_kernel(50, lmax), lmax, 200)
    assert filters.effective_coefficients(heat200, np.float64).size < 50 > filters.effective_coefficients(heat200, np.float32).size
    assert filters.effective_coefficients(np.array([1.0, 1e-30]), np.float64).size == 2  # (c_0, c_1 always stay)
    assert filters.choose_evaluation("auto", c200, np.float32, *big) == "recurrence"       # product refused, Newton overflows
    assert filters.choose_evaluation("auto", c200, np.float64, *big) == "newton"
    with pytest.raises(ValueError, match="not representable"):
        filters.choose_evaluation("newton", c200, np.float32, *big)
    with pytest.raises(ValueError, match="single-device"):
        filters.choose_evaluation("newton", c1, np.float64, *big, split=True)
    with pytest.raises(ValueError, match="evaluation must be"):
        filters.choose_evaluation("horner", c1, np.float64, *big)
    # through Filter.filter with a stubbed device: 'auto' reaches newton_filter only when the rule says so
    g = golden_sensor123
    L, lm = csr_from(g, "Lcomb"), float(g["lmax"])
    G = StubGraph(L, lm)
    calls = []

    class StubDev:
        dtype = np.dtype(np.float64)

        def cheby_filter(self, cc, x, lmx, mode=0):
            calls.append("recurrence")
            return orc.cheby_op(L, lmx, cc, x).reshape(cc.shape[0], G.N, -1), 0.0

        def program_filter(self, prog, x, lmx, old_is_x=False):
            calls.append("newton" if old_is_x else "product")
            t = (2.0 / lmx) * L - sparse.identity(G.N)
            h_prev, h = np.zeros_like(x), x
            for s_, (sc, be, ga) in enumerate(prog):
                o = x if old_is_x else (h_prev if s_ else 0.0 * x)
                h_prev, h = h, (2 * sc) * t.dot(h) + be * h + ga * o
            return h, 0.0

        def newton_filter(self, nd, dc, x, lmx):
            calls.append("newton")
            t = (2.0 / lmx) * L - sparse.identity(G.N)
            h = dc[-1] * x
            for j in range(len(nd) - 1, -1, -1):
                h = t.dot(h) - nd[j] * h + dc[j] * x
            return h, 0.0

    monkeypatch.setattr(filters, "_device_graph_of", lambda G_: StubDev())
    heat = filters.Heat(G, scale=10)
    y = heat.filter(g["signals5"], order=30, evaluation="auto")  # 123 x 5: launch-bound -> recurrence
    assert calls == ["recurrence"] and rel_err(y, g["heat10_y5"]) < 1e-13
    monkeypatch.setattr(filters, "AUTO_MIN_PANEL_BYTES", 0)
    y = heat.filter(g["signals5"], order=30, evaluation="auto")
    assert calls[-1] == "product" and rel_err(y, g["heat10_y5"]) < 1e-12 and G._gspx_last_evaluation == "product"
    heat.filter(g["signals5"], order=30, evaluation="product")     # (an explicit choice)
    assert calls[-1] == "product"
    y = heat.filter(g["signals5"], order=30, evaluation="newton")
    assert calls[-1] == "newton" and rel_err(y, g["heat10_y5"]) < 1e-13 and G._gspx_last_evaluation == "newton"
    filters.MexicanHat(G, Nf=6).filter(g["signals5"], order=40, evaluation="auto")
    assert calls[-1] == "recurrence"
    try:
        filters.set_evaluation("auto")
        heat.filter(g["signal"], order=30)
        assert calls[-1] == "product"
    finally:
        filters.set_evaluation("recurrence")
    heat.filter(g["signal"], order=30)
    assert calls[-1] == "recurrence"
    with pytest.raises(ValueError):
        filters.set_evaluation("horner")


def test_product_form_and_its_guard():
    """The product form (round 6): p(t) = C prod sigma_j (t - r_j) from the roots of the Chebyshev series - real roots
    one step, conjugate pairs two - as a program of (scale, beta, gamma) rows.  The scalar program reproduces the
    Chebyshev sum; converged series are trimmed to their effective degree; the guard clears what the device then
    computes to 1e-13 and refuses what it computes badly (measured on the device: Mexican-hat low-pass at order 100
    reads 5e-8 in fp64 and 25 in fp32)."""
    from numpy.polynomial import chebyshev as npcheb
    lmax = 22.1
    kernels = {"heat50": orc.heat_kernel(50, lmax), "heat10": orc.heat_kernel(10, lmax)}
    kernels.update({"mh%d" % i: k for i, k in enumerate(orc.mexican_hat_kernels(lmax, 6))})
    grid = np.cos(np.linspace(0, np.pi, 401))
    for name, kern in kernels.items():
        for order in (2, 3, 30, 50, 100):
            c = orc.compute_cheby_coeff(kern, lmax, order)
            prog = filters.cheb_to_product(c, np.float64)
            assert prog.shape[1] == 3 and 1 <= prog.shape[0] <= order and prog[0, 2] == 0.0
            h_prev, h = np.zeros_like(grid), np.ones_like(grid)
            for s, (sc, be, ga) in enumerate(prog):
                h_prev, h = h, (2 * sc) * grid * h + be * h + (ga if s else 0.0) * h_prev
            cc = c.copy()
            cc[0] /= 2
            p = npcheb.chebval(grid, cc)
            assert np.max(np.abs(h - p)) < 2e-11 * np.max(np.abs(p)), (name, order)
            ok, m = filters.product_guard(c, np.float64)
            assert m["finite"] and m["grid_err"] < 2e-11 and 1.0 <= m["panel_passes_per_order"] * order / prog.shape[0] <= 3.0
            assert ok == (8 * m["eps_amplification"] <= filters.PRODUCT_GUARD[np.dtype(np.float64)][1])
    # the headline polynomial: 30 factors, 18 of them real roots (the interpolant oscillates about zero where the
    # kernel is below its error), 2.2 panel passes per order; cleared in fp64
    c = orc.compute_cheby_coeff(kernels["heat50"], lmax, 30)
    ok, m = filters.product_guard(c, np.float64)
    assert ok and m["S"] == 30 and abs(m["panel_passes_per_order"] - 2.2) < 0.05 and m["amplification"] < 1e3
    # a converged series is trimmed: order 100 of Heat(10) is 22 factors in fp64 and fewer in fp32
    c = orc.compute_cheby_coeff(kernels["heat10"], lmax, 100)
    assert filters.cheb_to_product(c, np.float64).shape[0] < 30 > filters.cheb_to_product(c, np.float32).shape[0]
    assert filters.product_guard(c, np.float64)[0] and filters.product_guard(c, np.float32)[0]
    # refused: the Mexican-hat low-pass at order 100 (error amplification 9e11), in both dtypes
    c = orc.compute_cheby_coeff(kernels["mh0"], lmax, 100)
    for dt in (np.float64, np.float32):
        ok, m = filters.product_guard(c, dt)
        assert not ok and m["reason"] == "amplification" and m["amplification"] > 1e9
    # explicit 'product' on a polynomial that does not fit: an error, not garbage; degenerate inputs
    assert filters.choose_evaluation("product", np.atleast_2d(c), np.float64, 10, 1) == "product"  # finite: the caller's choice
    with pytest.raises(ValueError, match="single-device"):
        filters.choose_evaluation("product", np.atleast_2d(c), np.float64, 10, 1, split=True)
    with pytest.raises(TypeError):
        filters.cheb_to_product(np.array([1.0]))
    with pytest.raises(ValueError):
        filters.cheb_to_product(np.array([1.0, np.inf, 0.5]))
    assert not filters.product_guard(np.array([2.0, 0.0, 0.0]), np.float64)[0]  # a constant: no product form
