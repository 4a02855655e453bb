"""The numpy restatement behind the Chebyshev graph convolution tests (gspx_cheby_conv_dev,
gspx_cheby_cross_grams_dev, filters.cheby_conv, pygsp_amd.nn.ChebConv): the plain three-term recurrence, then the
feature mix, one order at a time; the cross-Grams of the recurrence with a second signal; the vector-Jacobian product
built on both; and a stand-in device object that computes with them.  Everything in fp64."""
import numpy as np

from oracle import cheby_oracle as orc
from spectrum_helpers import slots


def _cube(L, X, F=None):
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(L.shape[0], -1, X.shape[-1])
    assert F is None or X.shape[2] == F, (X.shape, F)
    return X


def recurrence(L, lmax, X, M):
    """[T_0 X, .., T_{M-1} X], each (N, B, Fin): T_k(Lt) acts on the vertex index only."""
    X = _cube(L, X)
    return [T.reshape(X.shape) for T in slots(L, lmax, X.reshape(X.shape[0], -1), M)]


def conv_direct(L, lmax, X, theta):
    """(N, B, Fout): sum_k (T_k(Lt) X) theta[k] - a plain sum, theta[0] not halved.  X (N, Fin) or (N, B, Fin)."""
    theta = np.asarray(theta, dtype=np.float64)
    return sum(np.einsum("nbi,io->nbo", T, theta[k]) for k, T in enumerate(recurrence(L, lmax, X, theta.shape[0])))


def cross_grams_direct(L, lmax, X, Z, M):
    """(M, Fin, Fout): sum_{n, b} (T_k(Lt) X)[n, b, i] Z[n, b, o]."""
    Z = _cube(L, Z)
    return np.array([np.einsum("nbi,nbo->io", T, Z) for T in recurrence(L, lmax, X, M)])


def conv_vjp_direct(L, lmax, X, theta, cot):
    """(grad_X (N, B, Fin), grad_theta (M, Fin, Fout)) of <cot, conv_direct(X, theta)>, L symmetric."""
    theta = np.asarray(theta, dtype=np.float64)
    return conv_direct(L, lmax, cot, theta.transpose(0, 2, 1)), cross_grams_direct(L, lmax, X, cot, theta.shape[0])


def bridge_theta(c, F):
    """theta[k] = c_k I_F with theta[0] halved: cheby_conv with it is cheby_op with the coefficients c."""
    c = np.asarray(c, dtype=np.float64)
    theta = c[:, None, None] * np.eye(F)[None]
    theta[0] *= 0.5
    return theta


class OracleDevice:
    """Stands in for engine.DeviceGraph where filters.cheby_conv(_vjp) and the torch layer need one: the host-array
    call contract of cheby_conv and cheby_cross_grams, arithmetic by the restatement above."""

    def __init__(self, L, dtype=np.float64):
        self.L, self.N, self.dtype, self.calls = L, L.shape[0], np.dtype(dtype), []

    def cheby_conv(self, theta, x, lmax):
        self.calls.append("conv")
        return conv_direct(self.L, lmax, x, theta), 0.0

    def cheby_cross_grams(self, x, z, lmax, M):
        self.calls.append("cross_grams")
        return cross_grams_direct(self.L, lmax, x, z, M), 0.0


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
