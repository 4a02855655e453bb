"""Connected components, the parts that need no GPU: the plugin's topology rows on a pygsp-shaped stand-in, the
C-ABI prototypes, the round cap (host arithmetic), and the entry points failing loudly without a device."""
import ctypes
import types

import numpy as np
import pytest
from scipy import sparse

from pygsp_amd import _capi, engine, graphs, plugin


def _standin():
    class Graph:
        _connected = None

        def is_connected(self):
            return "ref connected"

        def extract_components(self):
            return "ref components"

        def estimate_lmax(self, method="lanczos"):
            return "ref lmax"

    mod = types.ModuleType("pygsp")
    mod.graphs = types.ModuleType("pygsp.graphs")
    mod.graphs.Graph = Graph
    mod.filters = types.ModuleType("pygsp.filters")
    mod.filters.approximations = types.ModuleType("pygsp.filters.approximations")
    mod.filters.approximations.cheby_op = mod.filters.cheby_op = lambda *a, **k: "ref cheby"
    return mod


def test_plugin_topology_rows_are_opt_in_and_restored():
    mod = _standin()
    Graph = mod.graphs.Graph
    own = (Graph.is_connected, Graph.extract_components, Graph.estimate_lmax)
    assert plugin._TOPOLOGY == ("is_connected", "extract_components")
    try:
        plugin.install(mod)
        assert (Graph.is_connected, Graph.extract_components, Graph.estimate_lmax) == own
        plugin.install(mod, topology=True)
        assert Graph.is_connected is plugin._is_connected_on_device
        assert Graph.extract_components is plugin._extract_components_on_device
        assert Graph.estimate_lmax is own[2]
        assert set(plugin._TOPOLOGY) == set(vars(Graph)[plugin._SAVED])
        plugin.install(mod, topology=True)  # again: the saved originals are still the package's own
        assert vars(Graph)[plugin._SAVED]["is_connected"] is own[0]
        # a directed graph, and a graph without vertices, reach the originals
        directed = Graph()
        directed.N, directed.is_directed = 3, lambda: True
        assert directed.is_connected() == "ref connected" and directed.extract_components() == "ref components"
        empty = Graph()
        empty.N, empty.is_directed = 0, lambda: False
        assert empty.is_connected() == "ref connected"
        plugin.install(mod, topology=False, lmax="device")
        assert (Graph.is_connected, Graph.extract_components) == own[:2] and Graph.estimate_lmax is not own[2]
        plugin.install(mod, topology=True)
    finally:
        plugin.uninstall(mod)
    assert (Graph.is_connected, Graph.extract_components, Graph.estimate_lmax) == own
    assert not hasattr(Graph, plugin._SAVED)
    bare = _standin()
    del bare.graphs
    with pytest.raises(ValueError, match="topology=True"):
        plugin.install(bare, topology=True)
    plugin.uninstall(bare)


def test_capi_prototypes():
    sig = _capi.SIGNATURES
    P = ctypes.c_void_p
    outs = [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    assert sig["gspx_graph_components_dev"] == (ctypes.c_int, [P, P] + outs)
    assert sig["gspx_graph_components"] == (ctypes.c_int, [P, P] + outs)
    assert sig["gspx_components_round_cap"] == (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(ctypes.c_int)])
    assert _capi.ERR_INTERNAL == 6
    lib = _capi.load()
    for name in ("gspx_graph_components_dev", "gspx_graph_components", "gspx_components_round_cap"):
        assert hasattr(lib, name)


def test_round_cap_and_argument_errors_need_no_device():
    """The cap is 2 ceil(log2 N) + 1 (derived in gspx_components.hip.h); null handles are refused before any device
    work."""
    lib = _capi.load()
    cap = ctypes.c_int(-1)
    for N, want in ((0, 1), (1, 1), (2, 3), (3, 5), (4, 5), (1000, 21), (1 << 20, 41), (1 << 30, 61)):
        _capi.check(lib.gspx_components_round_cap(N, ctypes.byref(cap)))
        assert cap.value == want, N
    with pytest.raises(ValueError):
        _capi.check(lib.gspx_components_round_cap(-1, ctypes.byref(cap)))
    with pytest.raises(ValueError):
        _capi.check(lib.gspx_components_round_cap(5, None))
    n, rounds, ms = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0)
    labels = np.zeros(4, dtype=np.int32)
    for fn in (lib.gspx_graph_components_dev, lib.gspx_graph_components):
        with pytest.raises(ValueError, match="null graph"):
            _capi.check(fn(None, _capi.ptr(labels), ctypes.byref(n), ctypes.byref(rounds), ctypes.byref(ms)))


@pytest.mark.skipif(_capi.device_count() > 0, reason="checks the no-device behaviour")
def test_topology_fails_loudly_without_device():
    """No CPU fallback: without a HIP device an undirected graph cannot be built, let alone labelled."""
    W = sparse.csr_matrix(np.array([[0., 1., 0.], [1., 0., 0.], [0., 0., 0.]]))
    with pytest.raises(_capi.GspxError):
        graphs.Graph(W).connected_components()
    with pytest.raises(_capi.GspxError):
        graphs.Graph(W).is_connected()
    with pytest.raises(_capi.GspxError):
        engine.DeviceGraph.from_w(W).components()

    class Undirected:  # a reference-shaped graph through the plugin's rows
        def __init__(self):
            self.N, self.lap_type, self._connected, self.W = 3, "combinatorial", None, W
            self.L = sparse.csr_matrix(np.diag([1., 1., 0.])) - W

        def is_directed(self):
            return False

    for method in (plugin._is_connected_on_device, plugin._extract_components_on_device):
        with pytest.raises(_capi.GspxError):
            method(Undirected())
