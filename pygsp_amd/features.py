"""Localised-atom norms and the graph spectrogram (pygsp.features, features.py:27-94) on the device.

The reference builds the dense (Nf N, N) frame of every atom and keeps N numbers of it.  Here the bank is applied to
identity panels written on the device, and every panel leaves as its Nf x w squared column norms (filters.frame_norms,
gspx_cheby_sqnorms_dev): no frame, no N x N array.  A spectrogram of M shifted atoms is ONE bank of M kernels: one
recurrence sweep over the identity and one fused contraction per batch, whatever M is.

Behaviour kept from the reference on purpose:
* ``**kwargs`` are ignored: the reference's compute_tig drops them, so the filter is always Chebyshev of order 30.
* compute_norm_tig of a bank of Nf > 1 kernels returns a list of Nf identical (Nf N,) arrays (filterbank_handler maps
  compute_tig, which ignores ``i``, over the bank); Nf = 1 returns shape (N,).
* compute_spectrogram sets ``G.spectr``; its default atom is exp(-M (x / lmax)^2), shifted to linspace(0, lmax, M).
"""
import numpy as np

from . import filters

ORDER = 30  # Filter.filter's default order: what the reference's compute_frame() runs (kwargs never reach it)


@filters.filterbank_handler
def compute_tig(g, **kwargs):
    """The frame of the bank (features.py:27-42): ``g.compute_frame()``, kwargs ignored as in the reference."""
    return g.compute_frame()


def _norm_tig(g, norms, **kwargs):
    """compute_norm_tig's return convention around norms(bank) -> (Nf, N) squared norms."""
    n = np.sqrt(norms(g)).reshape(-1)  # entry f N + j: ||p_f(L) delta_j||, the norm of row f N + j of the frame
    if g.Nf <= 1 or "i" in kwargs:
        return n
    return [n.copy() for _ in range(g.Nf)]


def compute_norm_tig(g, **kwargs):
    """The l2 norms of the frame's rows (features.py:45-59), from squared column norms on the device.  Nf = 1: shape
    (N,); Nf > 1: a list of Nf identical (Nf N,) arrays, as the reference returns."""
    return _norm_tig(g, lambda bank: filters.frame_norms(bank, ORDER), **kwargs)


class ShiftedAtom:
    """atom(x - shift), the shift bound at construction: one kernel of the spectrogram's bank."""

    def __init__(self, atom, shift):
        self.atom, self.shift = atom, shift

    def __call__(self, x):
        return self.atom(x - self.shift)


def spectrogram_kernels(G, atom, M):
    """The M kernels of compute_spectrogram (features.py:80-90).  The default atom reads G.lmax when it is evaluated,
    as the reference's closure does."""
    if not atom:
        def atom(x):
            return np.exp(-M * (x / G.lmax) ** 2)
    return [ShiftedAtom(atom, shift) for shift in np.linspace(0, G.lmax, M)]


def _spectrogram(G, bank, norms):
    spectr = np.ascontiguousarray(norms(bank).T)  # (N, M): column m = ||T_i g_m||^2 for every vertex i
    G.spectr = spectr
    return spectr


def compute_spectrogram(G, atom=None, M=100, **kwargs):
    """The (N, M) squared norms of the localised atoms shifted along [0, lmax] (features.py:62-94), also stored in
    ``G.spectr``: one bank of M kernels on the device instead of M dense frames."""
    return _spectrogram(G, filters.Filter(G, spectrogram_kernels(G, atom, M)),
                        lambda bank: filters.frame_norms(bank, ORDER))
