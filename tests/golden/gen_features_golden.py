#!/usr/bin/env python3
"""Generate tests/golden/features_*.npz from the REAL reference (pygsp v0.6.1, the checkout named by $PYGSP_PATH).

    PYGSP_PATH=path/to/reference python tests/golden/gen_features_golden.py

Outputs of the reference's own pygsp.features: compute_norm_tig of Heat(10) on both Laplacians, the list that
compute_norm_tig returns for MexicanHat(Nf=6) (its first entry, and whether all Nf entries are equal) and
compute_spectrogram with its default M = 100 on Sensor(123); compute_spectrogram with M = 30 on the Logo.  lmax is the
reference's deterministic 'bounds' estimate, stored with the Laplacian it was taken on.
The fixtures are committed; tests read them, never the reference.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.environ["PYGSP_PATH"])
os.environ.setdefault("MPLBACKEND", "agg")
from pygsp import features, filters, graphs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def put_csr(out, prefix, A):
    A = A.tocsr()
    A.sort_indices()
    out[prefix + "_indptr"], out[prefix + "_indices"] = A.indptr.astype(np.int32), A.indices.astype(np.int32)
    out[prefix + "_data"], out[prefix + "_shape"] = A.data, np.array(A.shape)


def sensor123():
    G = graphs.Sensor(123, seed=42)
    out = {}
    put_csr(out, "W", G.W)
    for lap in ("combinatorial", "normalized"):
        G.compute_laplacian(lap)
        G._lmax_method = None  # (compute_laplacian drops _lmax but not the method: 'bounds' again would be a no-op)
        G.estimate_lmax("bounds")
        out["lmax_" + lap] = np.float64(G.lmax)
        put_csr(out, "L_" + lap, G.L)
        out["heat10_norm_tig_" + lap] = features.compute_norm_tig(filters.Heat(G, scale=10))
    G.compute_laplacian("combinatorial")
    G._lmax_method = None
    G.estimate_lmax("bounds")
    mh = features.compute_norm_tig(filters.MexicanHat(G, Nf=6))
    out["mh6_norm_tig"] = mh[0]
    out["mh6_list_len"] = np.int64(len(mh))
    out["mh6_all_equal"] = np.bool_(all(np.array_equal(m, mh[0]) for m in mh))
    out["spectrogram_M100"] = features.compute_spectrogram(G)
    np.savez_compressed(os.path.join(OUT, "features_sensor123.npz"), **out)


def logo():
    G = graphs.Logo()
    out = {}
    put_csr(out, "W", G.W)
    G.compute_laplacian("combinatorial")
    G.estimate_lmax("bounds")
    out["lmax_combinatorial"] = np.float64(G.lmax)
    put_csr(out, "L_combinatorial", G.L)
    out["spectrogram_M30"] = features.compute_spectrogram(G, M=30)
    np.savez_compressed(os.path.join(OUT, "features_logo.npz"), **out)


if __name__ == "__main__":
    sensor123()
    logo()
