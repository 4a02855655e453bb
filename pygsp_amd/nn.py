"""Differentiable Chebyshev filtering and graph convolution for PyTorch, on the engine's recurrence.

``cheby_filter`` (a torch.autograd.Function behind a plain function) and ``ChebyshevFilter`` (a torch.nn.Module whose
parameter is the coefficient matrix) are PER-CHANNEL filtering: scalar coefficients c[f][k], every signal column
filtered on its own, nothing mixes feature channels - fitting a filter to input / output pairs.  Forward is one
gspx_cheby_filter_dev call; backward is filters._vjp_device: one synthesis call with the same coefficients for the
signal's gradient (L is symmetric) and one gspx_cheby_cross_moments_dev call for the coefficients' gradient.

``cheby_conv`` and ``ChebConv`` are the ChebNet layer (Defferrard et al.): matrix coefficients Theta_k (Fin x Fout),
Y[n, b, :] = sum_k (T_k(Lt) X)[n, b, :] Theta_k, a plain sum.  Forward is one gspx_cheby_conv_dev call; backward is the
same call with every Theta_k transposed for the signal's gradient and one gspx_cheby_cross_grams_dev call for Theta's.
Only X is saved for backward, never the T_k X.

``WeightedGraph`` makes the graph's edge weights a parameter on a fixed pattern; ``cheby_filter`` on it has the
weights as a third differentiable input (one gspx_cheby_laplacian_grad_dev call in backward, at fixed lmax).

``graph_pool`` / ``graph_unpool`` and ``GraphPool`` / ``GraphUnpool`` move vertex signals between the levels of a
``reduction.Coarsening`` (max, mean or sum over every cluster): one gspx_segment_pool_dev call forward, one
gspx_segment_pool_vjp_dev call backward (the argmax of max pooling is recomputed from the saved input, no index tensor
is kept); no atomics, so a training step gives the same bits every time.

No second derivatives, no gradient with respect to lmax; ``cheby_conv`` has no gradient in the graph's weights.

IMPORT ORDER.  torch ships its own HIP runtime (libamdhip64.so) and libgspx links against the ROCm installation's copy
of the same SONAME.  Whichever of the two is loaded first serves both libraries: this module imports torch at its
top, before anything loads libgspx (pygsp_amd loads it lazily, at the first context or graph), so a process that
imports ``pygsp_amd.nn`` before creating a context has ONE runtime, and a tensor's ``data_ptr()`` means the same thing
to both.  A process that has already loaded libgspx when torch arrives holds TWO runtimes; a pointer of torch's is then
unknown to libgspx's, gspx_ptr_device says so, and every call is staged through host arrays instead - correct, slower,
with one warning per process.  A pointer the library's runtime does not know never reaches a kernel.
(The order to avoid, seen on the card: libgspx LOADED but not yet used, then torch imported, then the first context -
torch's bundled runtime had claimed the GPU by then and gspx_ctx_create found no device.  A process that wants both
and cannot import this module first makes one libgspx call that touches HIP, e.g. ``_capi.device_count()``, before it
imports torch; tests/test_autograd_host.py does.)

No other module of the package imports torch."""
import torch  # first: see IMPORT ORDER above

import ctypes
import warnings

import numpy as np

from . import _capi, engine, filters

_warned = False
last_path = None  # "zero_copy" | "staged": how the most recent forward or backward pass reached the engine


def _np_dtype(t):
    if t.dtype == torch.float64:
        return np.dtype(np.float64)
    if t.dtype == torch.float32:
        return np.dtype(np.float32)
    raise TypeError("the engine takes float64 or float32 signals, got {}".format(t.dtype))


def ptr_device(pointer):
    """The device ordinal of `pointer` (an int) as libgspx's HIP runtime sees it, or None when that runtime does not
    know it as device memory (gspx_ptr_device: launches nothing, touches no memory)."""
    dev = ctypes.c_int(-1)
    rc = _capi.load().gspx_ptr_device(ctypes.c_void_p(int(pointer)), ctypes.byref(dev))
    return dev.value if rc == _capi.OK else None


def _zero_copy(dev, tensors):
    """Whether the device entry points may read and write `tensors` (contiguous, on the GPU) in place: `dev` is a real
    engine.DeviceGraph and libgspx's own runtime places every pointer on the context's device.  Warns once per process
    when it does not."""
    global _warned, last_path
    last_path = "staged"
    if not hasattr(dev, "cheby_filter_dev") or not hasattr(dev, "ctx"):
        return False
    bad = [t.data_ptr() for t in tensors if ptr_device(t.data_ptr()) != dev.ctx.device]
    if not bad:
        last_path = "zero_copy"
        return True
    if not _warned:
        _warned = True
        warnings.warn("pygsp_amd.nn: the HIP runtime of libgspx does not know torch's device pointer {:#x} as memory of "
                      "device {} ({}) - the process holds two HIP runtimes because libgspx was loaded before torch, or "
                      "the tensor lives elsewhere.  Calls are staged through host arrays: correct, but slow.  Import "
                      "pygsp_amd.nn BEFORE creating a context or a device graph."
                      .format(bad[0], dev.ctx.device, _capi.last_error()), RuntimeWarning, stacklevel=3)
    return False


def _device_of(G, x):
    """The graph's device build for x's dtype; a GPU tensor must live on that build's GPU."""
    dev = G.device_graph(_np_dtype(x))
    if x.is_cuda and hasattr(dev, "ctx") and x.device.index != dev.ctx.device:
        raise ValueError("the signal lives on {} but the graph on GPU {}".format(x.device, dev.ctx.device))
    return dev


def _host(t):
    global last_path
    last_path = "staged"
    return np.ascontiguousarray(t.detach().cpu().numpy())


class _ChebyFilter(torch.autograd.Function):
    """y[n, j, f] = (p_f(L) x)[n, j],  p_f = c_f0 / 2 + sum_{k >= 1} c_fk T_k(Lt).

    ORDERING of the zero-copy path.  Before a device call the tensor's producer stream (torch's current stream on that
    GPU) is synchronised, so every input - and the freshly allocated output - is at rest.  After it nothing more is
    needed: gspx_cheby_filter_dev and gspx_cheby_cross_moments_dev each end with their own hipStreamSynchronize of the
    context's stream (run_batches, the replay branch of filter_dev_t, the download of the moments), so the call has
    finished on the device when it returns and torch may read the output from any stream."""

    @staticmethod
    def forward(ctx, coeffs, x, G, lmax, weight=None, pattern=None):
        # (weight, pattern: the Parameter and the module of a WeightedGraph whose present graph G is - the third
        # differentiable input; None for a plain graph)
        ctx.pattern = pattern
        if coeffs.dim() not in (1, 2) or x.dim() not in (1, 2):
            raise ValueError("coeffs must be (Nf, M) or (M,) and x (N,) or (N, Nsig), got {} and {}"
                             .format(tuple(coeffs.shape), tuple(x.shape)))
        dev = _device_of(G, x)
        lmax = float(G.lmax if lmax is None else lmax)
        c = np.ascontiguousarray(coeffs.detach().to("cpu", torch.float64).numpy()).reshape(-1, coeffs.shape[-1])
        Nf, N = c.shape[0], x.shape[0]
        xc = x.detach().reshape(N, -1).contiguous()
        nsig = xc.shape[1]
        ctx.save_for_backward(xc)
        ctx.call = (G, dev, lmax, c, tuple(coeffs.shape), coeffs.dtype, coeffs.device, tuple(x.shape))
        y = None
        if xc.is_cuda and xc.numel():
            y = torch.empty((Nf, N, nsig), dtype=xc.dtype, device=xc.device)
            torch.cuda.current_stream(xc.device).synchronize()
            if _zero_copy(dev, (xc, y)):
                dev.cheby_filter_dev(c, xc.data_ptr(), y.data_ptr(), nsig, lmax, _capi.ANALYSIS)
            else:
                y = None
        if y is None:
            yh, _ = dev.cheby_filter(c, _host(xc), lmax, _capi.ANALYSIS)
            y = torch.from_numpy(np.ascontiguousarray(yh).reshape(Nf, N, nsig)).to(device=xc.device, dtype=xc.dtype)
        return y.permute(1, 2, 0)  # the planes the engine writes, viewed as (vertex, signal, filter): no copy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        (xc,) = ctx.saved_tensors
        G, dev, lmax, c, c_shape, c_dtype, c_device, x_shape = ctx.call
        need_c, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = ctx.pattern is not None and ctx.needs_input_grad[4]
        Nf, M = c.shape
        N, nsig = xc.shape
        g = grad_y.detach().to(xc.dtype).permute(2, 0, 1).contiguous()  # planes [filter][vertex][signal]
        grad_c = grad_x = None
        grad_w = _weight_grad(ctx.pattern, G, dev, lmax, c, xc, g) if need_w else None
        done = False
        if xc.is_cuda and xc.numel():
            gx = torch.empty((N, nsig), dtype=xc.dtype, device=xc.device) if need_x else None
            torch.cuda.current_stream(xc.device).synchronize()
            if _zero_copy(dev, [t for t in (xc, g, gx) if t is not None]):
                grad_c, _ = filters._vjp_device(dev, lmax, c, xc.data_ptr(), g.data_ptr(),
                                                gx.data_ptr() if need_x else 0, nsig, False, need_x, need_c)
                grad_x, done = gx, True
        if not done:
            gh = _host(g)
            if need_x:
                gxh, _ = dev.cheby_filter(c, gh, lmax, _capi.SYNTHESIS)
                grad_x = torch.from_numpy(np.ascontiguousarray(gxh).reshape(N, nsig)).to(device=xc.device, dtype=xc.dtype)
            if need_c:
                cross, _ = dev.cheby_cross_moments(_host(xc), gh, lmax, M)
                grad_c = filters._grad_coefficients(cross)
        if need_c:
            grad_c = torch.from_numpy(np.ascontiguousarray(grad_c)).to(device=c_device, dtype=c_dtype).reshape(c_shape)
        if need_x:
            grad_x = grad_x.reshape(x_shape)
        return (grad_c if need_c else None), (grad_x if need_x else None), None, None, grad_w, None


def _weight_grad(pattern, G, dev, lmax, c, xc, g):
    """The gradient of the weights of a WeightedGraph's pattern (filters._weight_gradient over its pairs, so that pairs
    at weight 0 receive theirs too), as a tensor like ``pattern.weight``.  xc (N, nsig) and the cotangent planes g
    (Nf, N, nsig) as in _ChebyFilter.backward: GPU tensors go to gspx_cheby_laplacian_grad_dev by pointer when libgspx's
    runtime knows them, with the pair list and the two outputs in tensors of their own; otherwise the call is staged
    through host arrays."""
    N, nsig = xc.shape

    def call(pairs, need_diag):
        P = pairs.shape[1]
        if P == 0:  # (an empty list by pointer would read as "the graph's own edges": nothing to ask the device for)
            return (np.zeros(N) if need_diag else None), np.zeros(0), 0.0
        if xc.is_cuda and xc.numel():
            pt = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(xc.device)
            gdiag = torch.empty(N if need_diag else 0, dtype=torch.float64, device=xc.device)
            goff = torch.empty(max(P, 1), dtype=torch.float64, device=xc.device)
            torch.cuda.current_stream(xc.device).synchronize()
            if _zero_copy(dev, (xc, g, pt, goff) + ((gdiag,) if need_diag else ())):
                ms = dev.cheby_laplacian_grad_dev(c, xc.data_ptr(), g.data_ptr(), nsig, lmax, pt.data_ptr(),
                                                  pt.data_ptr() + 4 * P, P, gdiag.data_ptr() if need_diag else None,
                                                  goff.data_ptr())
                return (gdiag.cpu().numpy() if need_diag else None), goff[:P].cpu().numpy(), ms
        return dev.cheby_laplacian_grad(c, _host(xc), _host(g), lmax, pairs, need_diag)

    grad, _ = filters._weight_gradient(G, pattern.pairs, call)
    w = pattern.weight
    return torch.from_numpy(np.ascontiguousarray(grad)).to(device=w.device, dtype=w.dtype)


def cheby_filter(G, coeffs, x, lmax=None):
    """The Chebyshev filters `coeffs` of the Laplacian of `G` applied to `x`, differentiable in both.

    coeffs: tensor (Nf, M) or (M,), M >= 2, on any device (the engine reads coefficients from the host).  x: tensor
    (N,) or (N, Nsig), float64 or float32, on the CPU or on the GPU of G's context; the graph's device build of that
    dtype (``G.device_graph(dtype)``) computes.  lmax: G.lmax unless given.  Returns (N, Nsig, Nf) on x's device,
    a permuted view of the planes the engine writes.

    A GPU tensor goes in by ``data_ptr()`` and the result is written into a ``torch.empty`` tensor in place, if
    libgspx's HIP runtime knows those pointers (see the module docstring); otherwise, and for CPU tensors, the call
    is staged through host arrays.  ``backward`` (once differentiable) returns the gradient of `coeffs` in its dtype
    and on its device and the gradient of `x`; only the device calls of the gradients that are needed run.

    `G` may be a WeightedGraph: its ``weight`` is then a third differentiable input.  The forward pass filters on
    ``G.graph()``; backward adds one gspx_cheby_laplacian_grad_dev call on the module's pattern (when ``weight``
    requires a gradient) and the chain rule of filters.cheby_op_vjp_weights, at fixed lmax."""
    if isinstance(G, WeightedGraph):
        return _ChebyFilter.apply(coeffs, x, G.graph(), lmax, G.weight, G)
    return _ChebyFilter.apply(coeffs, x, G, lmax)


class WeightedGraph(torch.nn.Module):
    """The edge weights of a graph as a parameter on a fixed pattern: ``weight`` is a float64 Parameter of shape (P,),
    one entry per pair of the pattern - `G`'s edge list (``G.get_edge_list()``) or the (2, P) integer array `pairs` of
    unique unordered pairs s != t - initialised from G's weights, 0 where a pair is no edge of G.  ``graph()`` is the
    graphs.Graph of the present values, with G's lap_type, coordinates and compute dtype; ``cheby_filter(module, c, x)``
    filters on it and differentiates with respect to ``weight`` too.

    ``graph()`` rebuilds only after ``weight`` has changed (its ``_version`` counter); the rebuild goes through the
    host: P doubles down, a scipy CSR, the one-call device set-up.  Pairs at weight 0 are not stored in W but stay in the
    pattern and receive their gradient.  A negative or non-finite weight raises ValueError: clamp after the optimiser
    step (``with torch.no_grad(): module.weight.clamp_(min=0)``)."""

    def __init__(self, G, pairs=None):
        super().__init__()
        if G.is_directed():
            raise ValueError("WeightedGraph needs an undirected graph (one weight per unordered pair)")
        self.G = G
        W = G.W.tocsr()
        if pairs is None:
            if np.any(W.diagonal() != 0):
                raise ValueError("the graph has self-loops: its own edge list is not a list of pairs s != t")
            s, t, _ = G.get_edge_list()
            p = np.stack([np.asarray(s), np.asarray(t)])
        else:
            p = filters._pair_list(G, pairs)
        lo, hi = np.minimum(p[0], p[1]).astype(np.int64), np.maximum(p[0], p[1]).astype(np.int64)
        if np.unique(lo * G.N + hi).size != lo.size:
            raise ValueError("the pairs of a WeightedGraph must be unique as unordered pairs")
        self.pairs = np.ascontiguousarray(p, dtype=np.int32)
        start = np.asarray(W[self.pairs[0], self.pairs[1]], dtype=np.float64).ravel() if lo.size else np.zeros(0)
        self.weight = torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(start)))
        self._graph, self._built = None, None

    def _build(self, W):
        """The graph of adjacency W (scipy CSR), like self.G in everything but its weights."""
        from . import graphs
        G = self.G
        return graphs.Graph(W, lap_type=G.lap_type, coords=getattr(G, "coords", None), compute_dtype=G.compute_dtype,
                            device=G.device, reorder=G.reorder, tiles=G.tiles, ctx=G._ctx)

    def graph(self):
        """The graph of the present weights; rebuilt only when ``weight`` has changed since the last call."""
        version = (self.weight._version, id(self.weight))
        if self._graph is None or self._built != version:
            from scipy import sparse
            w = self.weight.detach().to("cpu", torch.float64).numpy()
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError("WeightedGraph: a weight is negative or not finite (clamp after the optimiser step)")
            N, keep = self.G.N, w != 0
            s, t, w = self.pairs[0][keep], self.pairs[1][keep], w[keep]
            W = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([s, t]), np.concatenate([t, s]))),
                                  shape=(N, N)).tocsr()
            W.sort_indices()
            self._graph, self._built = self._build(W), version
        return self._graph

    def extra_repr(self):
        return "pairs={}, lap_type={}".format(self.pairs.shape[1], self.G.lap_type)


class ChebyshevFilter(torch.nn.Module):
    """A learnable bank of `n_filters` Chebyshev filters of order `order` on `G`: one float64 Parameter ``coeffs`` of
    shape (n_filters, order + 1), ``forward(x)`` = ``cheby_filter(G, coeffs, x)``.  `init`: a filters.Filter bank of
    n_filters kernels whose compute_cheby_coeff values start the coefficients; without it every filter starts as the
    identity (c_0 = 2: the series reads c_0 / 2)."""

    def __init__(self, G, n_filters=1, order=30, init=None):
        super().__init__()
        self.G, self.order = G, int(order)
        if self.order < 1:
            raise ValueError("order must be at least 1")
        if init is None:
            start = np.zeros((int(n_filters), self.order + 1))
            start[:, 0] = 2.0
        else:
            start = filters._as_coeff_matrix(filters.compute_cheby_coeff(init, m=self.order))
            if start.shape[0] != int(n_filters):
                raise ValueError("init holds {} filters, n_filters is {}".format(start.shape[0], n_filters))
        # float64 whatever torch's default dtype: the engine reads coefficients as float64 on the host for both compute
        # dtypes, and an alternating Chebyshev series does not forgive rounding them (``.float()`` converts as usual)
        self.coeffs = torch.nn.Parameter(torch.from_numpy(start))

    @property
    def n_filters(self):
        return self.coeffs.shape[0]

    def forward(self, x):
        return cheby_filter(self.G, self.coeffs, x)

    def extra_repr(self):
        return "n_filters={}, order={}".format(self.n_filters, self.order)


class _ChebyConv(torch.autograd.Function):
    """y[n, b, :] = sum_k (T_k(Lt) x)[n, b, :] theta[k].  The zero-copy gate, the synchronisation of the producer
    stream before a device call and the staged fallback are _ChebyFilter's (see ORDERING there): both entry points end
    with their own hipStreamSynchronize of the context's stream."""

    @staticmethod
    def forward(ctx, theta, x, G, lmax):
        if theta.dim() != 3 or x.dim() not in (2, 3) or x.shape[-1] != theta.shape[1]:
            raise ValueError("theta must be (M, Fin, Fout) and x (N, Fin) or (N, B, Fin), got {} and {}"
                             .format(tuple(theta.shape), tuple(x.shape)))
        dev = _device_of(G, x)
        lmax = float(G.lmax if lmax is None else lmax)
        th = np.ascontiguousarray(theta.detach().to("cpu", torch.float64).numpy())
        M, fin, fout = th.shape
        N = x.shape[0]
        xc = x.detach().reshape(N, -1, fin).contiguous()
        batch = xc.shape[1]
        ctx.save_for_backward(xc)
        ctx.call = (dev, lmax, th, theta.dtype, theta.device, tuple(x.shape))
        y = None
        if xc.is_cuda and xc.numel():
            y = torch.empty((N, batch, fout), dtype=xc.dtype, device=xc.device)
            torch.cuda.current_stream(xc.device).synchronize()
            if _zero_copy(dev, (xc, y)):
                dev.cheby_conv_dev(th, xc.data_ptr(), y.data_ptr(), batch, lmax)
            else:
                y = None
        if y is None:
            yh, _ = dev.cheby_conv(th, _host(xc), lmax)
            y = torch.from_numpy(np.ascontiguousarray(yh).reshape(N, batch, fout)).to(device=xc.device, dtype=xc.dtype)
        return y.reshape(tuple(x.shape[:-1]) + (fout,))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        (xc,) = ctx.saved_tensors
        dev, lmax, th, th_dtype, th_device, x_shape = ctx.call
        need_th, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        M, fin, fout = th.shape
        N, batch = xc.shape[0], xc.shape[1]
        g = grad_y.detach().to(xc.dtype).reshape(N, batch, fout).contiguous()
        tht = np.ascontiguousarray(th.transpose(0, 2, 1))
        grad_th = grad_x = None
        done = False
        if xc.is_cuda and xc.numel():
            gx = torch.empty((N, batch, fin), dtype=xc.dtype, device=xc.device) if need_x else None
            torch.cuda.current_stream(xc.device).synchronize()
            if _zero_copy(dev, [t for t in (xc, g, gx) if t is not None]):
                if need_x:
                    dev.cheby_conv_dev(tht, g.data_ptr(), gx.data_ptr(), batch, lmax)
                if need_th:
                    grad_th, _ = dev.cheby_cross_grams_dev(xc.data_ptr(), g.data_ptr(), batch, fin, fout, lmax, M)
                grad_x, done = gx, True
        if not done:
            gh = _host(g)
            if need_x:
                gxh, _ = dev.cheby_conv(tht, gh, lmax)
                grad_x = torch.from_numpy(np.ascontiguousarray(gxh).reshape(N, batch, fin)).to(device=xc.device,
                                                                                                dtype=xc.dtype)
            if need_th:
                grad_th, _ = dev.cheby_cross_grams(_host(xc), gh, lmax, M)
        if need_th:
            grad_th = torch.from_numpy(np.ascontiguousarray(grad_th, dtype=np.float64)).to(device=th_device, dtype=th_dtype)
        if need_x:
            grad_x = grad_x.reshape(x_shape)
        return (grad_th if need_th else None), (grad_x if need_x else None), None, None


def cheby_conv(G, theta, x, lmax=None):
    """The Chebyshev graph convolution of `x` on `G` with the matrix coefficients `theta`, differentiable in both:
    y[n, b, :] = sum_k (T_k(Lt) x)[n, b, :] theta[k], a plain sum (theta[0] is not halved).

    theta: tensor (M, Fin, Fout), M >= 2, 1 <= Fin, Fout <= 128, on any device (the engine reads it from the host as
    float64).  x: tensor (N, Fin) or (N, B, Fin) - VERTEX first, the engine's layout - float64 or float32, on the CPU
    or on the GPU of G's context.  lmax: G.lmax unless given.  Returns (N, Fout) or (N, B, Fout) on x's device and in
    x's dtype.  GPU tensors go in by ``data_ptr()`` when libgspx's HIP runtime knows them, through host arrays
    otherwise (see the module docstring).  ``backward`` (once differentiable) returns the gradient of `theta` in its
    dtype and on its device and the gradient of `x`; only the device calls of the gradients that are needed run."""
    return _ChebyConv.apply(theta, x, G, lmax)


class ChebConv(torch.nn.Module):
    """The ChebNet layer on `G`: ``forward(x)`` = ``cheby_conv(G, theta, x) + bias`` with ``theta`` a float64 Parameter
    of shape (order + 1, in_features, out_features) and ``bias`` an (out_features,) Parameter added by torch (none with
    ``bias=False``).  theta starts Glorot-uniform over a fan-in of (order + 1) in_features (and a fan-out of
    out_features), bias at zero.

    LAYOUT: vertex first.  x is (N, in_features) or (N, B, in_features) and the result (N, out_features) or
    (N, B, out_features), on x's device and in x's dtype - the engine's layout, NOT the batch-first one of PyTorch
    Geometric; ``x.transpose(0, 1)`` of a batch-first tensor goes in (the call makes it contiguous).

    theta is float64 whatever torch's default dtype, for the reason given for ChebyshevFilter.coeffs: the engine reads
    coefficients as float64 on the host for both compute dtypes."""

    def __init__(self, G, in_features, out_features, order, bias=True):
        super().__init__()
        self.G, self.order = G, int(order)
        self.in_features, self.out_features = int(in_features), int(out_features)
        if self.order < 1:
            raise ValueError("order must be at least 1")
        if self.in_features < 1 or self.out_features < 1:
            raise ValueError("in_features and out_features must be at least 1")
        fan_in = (self.order + 1) * self.in_features
        bound = float(np.sqrt(6.0 / (fan_in + self.out_features)))
        theta = torch.empty((self.order + 1, self.in_features, self.out_features), dtype=torch.float64)
        self.theta = torch.nn.Parameter(theta.uniform_(-bound, bound))
        self.bias = torch.nn.Parameter(torch.zeros(self.out_features)) if bias else None

    def forward(self, x):
        y = cheby_conv(self.G, self.theta, x)
        return y if self.bias is None else y + self.bias.to(y.dtype)

    def extra_repr(self):
        return "in_features={}, out_features={}, order={}, bias={}".format(self.in_features, self.out_features, self.order,
                                                                          self.bias is not None)


class _SegmentPool(torch.autograd.Function):
    """y = pool of x over the Segments `seg` (unpool=False) or the copy of every segment's row to its members
    (unpool=True: the 'sum' vjp; its own backward is then the 'sum' pooling).  The zero-copy gate, the synchronisation of
    the producer stream before a device call and the staged fallback are _ChebyFilter's (see ORDERING there): both
    entry points end with their own hipStreamSynchronize of the context's stream."""

    @staticmethod
    def _run(dev, seg, mode, vjp, a, x):
        """One pooling (vjp=False: a is the fine panel) or vjp call (a the cotangent, x the pooled input for 'max') on
        contiguous 2-D tensors; returns the result on a's device."""
        rows_out = seg.n_fine if vjp else seg.n_coarse
        width, dtype = a.shape[1], _np_dtype(a)
        need_x = vjp and mode == "max"
        if a.is_cuda and a.numel():
            out = torch.empty((rows_out, width), dtype=a.dtype, device=a.device)
            torch.cuda.current_stream(a.device).synchronize()
            if _zero_copy(dev, (a, out) + ((x,) if need_x else ())):
                if vjp:
                    engine.segment_pool_vjp_dev(seg.ctx, seg, mode, dtype, width, x.data_ptr() if need_x else None,
                                                a.data_ptr(), out.data_ptr())
                else:
                    engine.segment_pool_dev(seg.ctx, seg, mode, dtype, width, a.data_ptr(), out.data_ptr())
                return out
        if vjp:
            oh = engine.segment_pool_vjp(seg.ctx, seg, _host(a), _host(x) if need_x else None, mode)
        else:
            oh = engine.segment_pool(seg.ctx, seg, _host(a), mode)
        return torch.from_numpy(np.ascontiguousarray(oh).reshape(rows_out, width)).to(device=a.device, dtype=a.dtype)

    @staticmethod
    def forward(ctx, x, coarsening, lo, hi, mode, unpool):
        if mode not in engine.POOL_MODES:
            raise ValueError("Unknown pooling mode {!r}: 'max', 'mean' or 'sum'".format(mode))
        seg = coarsening.segments(lo, hi)
        rows = seg.n_coarse if unpool else seg.n_fine
        if x.dim() not in (2, 3) or x.shape[0] != rows:
            raise ValueError("x must be ({0}, F) or ({0}, B, F), got {1}".format(rows, tuple(x.shape)))
        _np_dtype(x)
        dev = engine._float64_device_graph(coarsening.graphs[0])  # (the gate's device; pooling reads no graph)
        if x.is_cuda and x.device.index != seg.ctx.device:
            raise ValueError("the signal lives on {} but the coarsening on GPU {}".format(x.device, seg.ctx.device))
        xc = x.detach().reshape(rows, -1).contiguous()
        ctx.call = (dev, seg, mode, unpool, tuple(x.shape))
        ctx.save_for_backward(*((xc,) if mode == "max" and not unpool else ()))
        y = _SegmentPool._run(dev, seg, "sum" if unpool else mode, unpool, xc, None)
        return y.reshape((y.shape[0],) + tuple(x.shape[1:]))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        dev, seg, mode, unpool, x_shape = ctx.call
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        g = grad_y.detach().reshape(grad_y.shape[0], -1).contiguous()
        if unpool:
            gx = _SegmentPool._run(dev, seg, "sum", False, g, None)
        else:
            xc = ctx.saved_tensors[0].to(g.dtype) if mode == "max" else None
            gx = _SegmentPool._run(dev, seg, mode, True, g, xc)
        return gx.reshape(x_shape), None, None, None, None, None


def graph_pool(coarsening, x, lo=0, hi=None, mode="max"):
    """`x` on the vertices of level `lo` of the ``reduction.Coarsening`` pooled to level `hi` (default: the coarsest),
    differentiable in x: 'max', 'mean' or 'sum' over every cluster, members in ascending order.

    x: tensor (N_lo, F) or (N_lo, B, F) - VERTEX first, as ``cheby_conv`` - float64 or float32, on the CPU or on the GPU
    of the coarsening's context.  Returns (N_hi, F) or (N_hi, B, F) on x's device and in x's dtype.  GPU tensors go in
    by ``data_ptr()`` when libgspx's HIP runtime knows them, through host arrays otherwise (see the module docstring).
    ``backward`` (once differentiable) is one gspx_segment_pool_vjp_dev call: a copy for 'sum', g / size for 'mean', and
    for 'max' the cotangent goes to the first member that attains the maximum (recomputed from x, which is the only
    thing saved)."""
    return _SegmentPool.apply(x, coarsening, lo, hi, mode, False)


def graph_unpool(coarsening, y, lo=0, hi=None):
    """`y` on the vertices of level `hi` copied to every member on level `lo`, differentiable in y (backward is the
    'sum' pooling).  Shapes, dtypes and devices as ``graph_pool``."""
    return _SegmentPool.apply(y, coarsening, lo, hi, "sum", True)


class GraphPool(torch.nn.Module):
    """``forward(x)`` = ``graph_pool(coarsening, x, lo, hi, mode)``: the pooling layer between two ChebConv layers on
    ``coarsening.graphs[lo]`` and ``coarsening.graphs[hi]`` (Defferrard et al.).  Vertex first, no parameters."""

    def __init__(self, coarsening, lo=0, hi=None, mode="max"):
        super().__init__()
        if mode not in engine.POOL_MODES:
            raise ValueError("Unknown pooling mode {!r}: 'max', 'mean' or 'sum'".format(mode))
        self.coarsening, self.mode = coarsening, mode
        self.lo, self.hi = coarsening._span(lo, hi)

    def forward(self, x):
        return graph_pool(self.coarsening, x, self.lo, self.hi, self.mode)

    def extra_repr(self):
        return "lo={}, hi={}, mode={}".format(self.lo, self.hi, self.mode)


class GraphUnpool(torch.nn.Module):
    """``forward(y)`` = ``graph_unpool(coarsening, y, lo, hi)``: every cluster's row copied to its members."""

    def __init__(self, coarsening, lo=0, hi=None):
        super().__init__()
        self.coarsening = coarsening
        self.lo, self.hi = coarsening._span(lo, hi)

    def forward(self, y):
        return graph_unpool(self.coarsening, y, self.lo, self.hi)

    def extra_repr(self):
        return "lo={}, hi={}".format(self.lo, self.hi)
