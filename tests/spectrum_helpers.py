"""The numpy restatement behind the spectrum tests (pygsp_amd.spectrum, gspx_cheby_moments_dev)."""
import numpy as np


def slots(L, lmax, x, S):
    """T_0 .. T_{S-1} of the three-term recurrence of approximations.py:93-112 applied to x (N, Nsig)."""
    a = lmax / 2.0
    x = np.asarray(x, dtype=np.float64)
    T = [x]
    if S > 1:
        T.append((L.dot(x) - a * x) / a)
    for _ in range(2, S):
        T.append((2.0 / a) * (L.dot(T[-1]) - a * T[-1]) - T[-2])
    return T


def moments_direct(L, lmax, x, M):
    """(M, Nsig): x_j^T T_k(Lt) x_j, one recurrence step per order."""
    x = np.asarray(x, dtype=np.float64)
    return np.array([(T * x).sum(0) for T in slots(L, lmax, x, M)])


def moments_doubling(L, lmax, x, M):
    """The same from M // 2 steps by T_i T_j = (T_{i+j} + T_{|i-j|}) / 2 (L symmetric)."""
    T = slots(L, lmax, x, M // 2 + 1)
    m = np.empty((M, T[0].shape[1]))
    m[0] = (T[0] * T[0]).sum(0)
    m[1] = (T[1] * T[0]).sum(0)
    for k in range(2, M):
        i = k // 2
        m[k] = 2.0 * (T[i + 1] * T[i]).sum(0) - m[1] if k & 1 else 2.0 * (T[i] * T[i]).sum(0) - m[0]
    return m


def exact_moments(e, lmax, M):
    """(M,): mean_i T_k(2 e_i / lmax - 1), the moments of the true density of states."""
    theta = np.arccos(2.0 * np.asarray(e, dtype=np.float64) / lmax - 1.0)
    return np.cos(np.arange(M)[:, None] * theta).mean(1)
