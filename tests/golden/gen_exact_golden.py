#!/usr/bin/env python3
"""Generate tests/golden/exact_sensor123.npz from the REAL reference (pygsp v0.6.1, the checkout named by $PYGSP_PATH).

    PYGSP_PATH=path/to/reference python tests/golden/gen_exact_golden.py

Sensor(123, seed=42) with its full Fourier basis: the reference's own e and U (the tests inject them, so no result
depends on which eigenvectors another LAPACK picks), Filter.filter(method='exact') of Heat(10) and MexicanHat(6)
(analysis, synthesis of that analysis, localize(61)), Modulation(Heat(10)) in both orders, Gabor(Heat(10)) and the
coherence.  The fixture is committed; tests read it, never the reference.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import filters, graphs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def make(name, G):
    out = {}
    W = G.W.tocsr()
    W.sort_indices()
    out["W_indptr"], out["W_indices"], out["W_data"] = W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data
    out["W_shape"] = np.array(W.shape)
    G.compute_fourier_basis()
    out["e"], out["U"], out["lmax"] = G.e, G.U, np.float64(G.lmax)
    out["coherence"] = np.float64(G.coherence)
    rng = np.random.default_rng(11)
    x1, x5 = rng.standard_normal(G.N), rng.standard_normal((G.N, 5))
    out["x1"], out["x5"] = x1, x5
    for key, bank in (("heat10", filters.Heat(G, scale=10)), ("mexicanhat6", filters.MexicanHat(G, Nf=6))):
        for tag, x in (("1", x1), ("5", x5)):
            analysis = bank.filter(x, method="exact")
            out["{}_analysis{}".format(key, tag)] = analysis
            # (with one filter the second pass reads as an analysis again: the chain the doctest of filter.py runs)
            out["{}_synthesis{}".format(key, tag)] = bank.filter(analysis, method="exact")
        out[key + "_localize61"] = bank.localize(61, method="exact")
    heat = filters.Heat(G, scale=10)
    out["modulation_localize_first"] = filters.Modulation(G, heat, modulation_first=False).filter(x1)
    out["modulation_modulate_first"] = filters.Modulation(G, heat, modulation_first=True).filter(x1)
    out["modulation_evaluate"] = filters.Modulation(G, heat).evaluate(G.e)
    out["gabor"] = filters.Gabor(G, heat).filter(x1)
    np.savez_compressed(os.path.join(OUT, "exact_{}.npz".format(name)), **out)


if __name__ == "__main__":
    make("sensor123", graphs.Sensor(123, seed=42))
