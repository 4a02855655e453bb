"""The numpy restatement behind the autograd tests (gspx_cheby_cross_moments_dev, filters.cheby_op_vjp,
pygsp_amd.nn): cross-moments by the plain three-term recurrence with fp64 dots, the vector-Jacobian product built on
them and on the oracle's cheby_op, and a stand-in device object that computes with both."""
import numpy as np

from oracle import cheby_oracle as orc
from spectrum_helpers import slots


def cross_moments_direct(L, lmax, x, z, M):
    """(Nf, M, Nsig): sum_n z[f][n][j] (T_k(Lt) x)[n][j], one recurrence step per order.  x (N, Nsig); z (N, Nsig) -
    one plane - or (Nf, N, Nsig)."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    z = z.reshape((-1,) + x.shape)
    T = slots(L, lmax, x, M)
    return np.array([[(Tk * zf).sum(0) for Tk in T] for zf in z])


def analysis_direct(L, lmax, c, x):
    """(Nf, N, Nsig): p_f(L) x by the oracle."""
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    return orc.cheby_op(L, lmax, c, np.asarray(x, dtype=np.float64)).reshape(c.shape[0], L.shape[0], -1)


def synthesis_direct(L, lmax, c, planes):
    """(N, Nsig): sum_f p_f(L) planes[f] by the oracle, one filter at a time."""
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    return sum(orc.cheby_op(L, lmax, c[f], np.asarray(planes[f], dtype=np.float64)).reshape(L.shape[0], -1)
               for f in range(c.shape[0]))


def vjp_direct(L, lmax, c, x, cot, synthesis=False):
    """(grad_x, grad_c (Nf, M)) of the analysis forward y_f = p_f(L) x - x (N, Nsig), cot (Nf, N, Nsig) - or of the
    synthesis forward y = sum_f p_f(L) x_f - x (Nf, N, Nsig), cot (N, Nsig).  L symmetric."""
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    M = c.shape[1]
    if synthesis:
        gx = analysis_direct(L, lmax, c, cot)
        cross = cross_moments_direct(L, lmax, cot, x, M)
    else:
        gx = synthesis_direct(L, lmax, c, cot)
        cross = cross_moments_direct(L, lmax, x, cot, M)
    gc = cross.sum(axis=2)
    gc[:, 0] *= 0.5
    return gx, gc


class OracleDevice:
    """Stands in for engine.DeviceGraph where the torch layer and the vjp need one: the host-array call contract of
    cheby_filter and cheby_cross_moments, arithmetic by the oracle and the restatement above."""

    def __init__(self, L, dtype=np.float64):
        self.L, self.N, self.dtype, self.calls = L, L.shape[0], np.dtype(dtype), []

    def cheby_filter(self, coeffs, x, lmax, mode=0):
        self.calls.append("synthesis" if mode else "analysis")
        if mode == 0:
            return analysis_direct(self.L, lmax, coeffs, x), 0.0
        return synthesis_direct(self.L, lmax, coeffs, x), 0.0

    def cheby_cross_moments(self, x, z, lmax, M):
        self.calls.append("cross_moments")
        return cross_moments_direct(self.L, lmax, x, z, M), 0.0


class OracleGraph:
    """What filters and nn read from a Graph - N, lmax, device_graph(dtype), _check_signal - over an OracleDevice."""

    def __init__(self, W, lmax):
        self.W, self.L, self.N, self.lmax = W, orc.laplacian(W), W.shape[0], float(lmax)
        self.dev = OracleDevice(self.L)

    def device_graph(self, dtype=None):
        return self.dev

    def _check_signal(self, s):
        s = np.asanyarray(s)
        if s.shape[0] != self.N:
            raise ValueError("First dimension must be the number of vertices G.N = {}, got {}.".format(self.N, s.shape))
        return s
