r"""Weight image of the per-feature networks of the neural autoregressive flows (csrc/mnn.hip, csrc/umnn.hip).

A `MonotonicMLP(1 + S, 1, hidden, stack=F)` holds F independent networks (zuko/nn.py:356-392).  The kernel keeps ONE network in
LDS at a time, as an image of `image_floats` floats per feature:

    w0s   [T1][ks][64]        lane (j, q) of tile o, k-step s: |W0[16 o + j][1 + 4 s + q]|   (ks = ceil(S / 4): the signal columns padded
                                                                                              to the matrix instruction's K step, zeros behind S)
    w0x   [H1]                |W0[:, 0]|: the column x multiplies — also the tangent that enters the first layer
    b0    [H1]
    per further hidden layer l:
    w_l   [T_l][T_{l-1}][256]  lane (j, q), r = 0..3 of tile (o, i): |W_l[16 o + j][16 i + 4 q + r]| — the A operands of the four k-steps of a
                               16 x 16 tile as one 16-byte read per lane; k-step r multiplies units {r, 4 + r, 8 + r, 12 + r} of the input
                               tile, the order in which the accumulator registers of the layer before hold them
    b_l   [H_l]
    wl    [H_last]            |W_last[0, :]|
    bl    [4]                 b_last, three zeros

The absolute value is taken when the image is made: `index_table` addresses the concatenation of |W_0|, ..., |W_last|, b_0, ..., b_last
(`flat_parameters`), and zk_gather_f32 builds every feature's image from it on the device.  The arithmetic of `layout` is the one of
csrc/zk_mnn_common.h: mnn_layout, which both kernel families use (zk_mnn_image_floats returns its total; tests compare the two).

The integrand networks of an unconstrained monotone network (UNAF: a stacked `MLP(1 + S, 1, hidden, stack=F)` with ELU(alpha = 1), csrc/umnn.hip)
use the same image with the SIGNED weights: `flat_parameters` takes no absolute value for them, and neither does their backward image
(`backward_image_of(..., signed=True)`, csrc/umnn_backward.hip).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

LDS_MAX = 128 * 1024  # MNN_LDS_MAX of csrc/zk_mnn_common.h


@dataclass
class Layout:
    S: int
    widths: tuple
    ks: int = 0
    T: tuple = ()
    o_w0s: int = 0
    o_w0x: int = 0
    o_b0: int = 0
    o_w: list = field(default_factory=list)  # per hidden layer l >= 1
    o_b: list = field(default_factory=list)
    o_wl: int = 0
    o_bl: int = 0
    total: int = 0


def layout(S: int, widths) -> Layout | None:
    """Offsets of one feature's image, or None for a shape the kernel does not serve."""
    widths = tuple(int(w) for w in widths)
    if not (1 <= S <= 63 and 1 <= len(widths) <= 3) or any(w < 16 or w > 128 or w % 16 for w in widths):
        return None
    L = Layout(int(S), widths, ks=(S + 3) // 4, T=tuple(w // 16 for w in widths))
    o = 0
    L.o_w0s, o = o, o + L.T[0] * L.ks * 64
    L.o_w0x, o = o, o + widths[0]
    L.o_b0, o = o, o + widths[0]
    L.o_w, L.o_b = [0], [0]
    for l in range(1, len(widths)):
        L.o_w.append(o)
        o += L.T[l] * L.T[l - 1] * 256
        L.o_b.append(o)
        o += widths[l]
    L.o_wl, o = o, o + widths[-1]
    L.o_bl, o = o, o + 4
    L.total = o
    return L if 4 * o <= LDS_MAX else None


def supported(S: int, widths) -> bool:
    return layout(S, widths) is not None


def flat_offsets(S: int, widths, features: int):
    """Offsets of every parameter tensor inside `flat_parameters`: ([weights...], [biases...], total)."""
    dims = [1 + S, *widths, 1]
    w_off, b_off, o = [], [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        w_off.append(o)
        o += features * b * a
    for b in dims[1:]:
        b_off.append(o)
        o += features * b
    return w_off, b_off, o


def index_table(S: int, widths, features: int) -> np.ndarray:
    """int32 [features, image_floats]: where every float of every feature's image comes from in `flat_parameters` (-1 = zero)."""
    L = layout(S, widths)
    assert L is not None
    dims = [1 + S, *widths, 1]
    w_off, b_off, _ = flat_offsets(S, widths, features)
    idx = np.full((features, L.total), -1, dtype=np.int64)
    f = np.arange(features, dtype=np.int64)[:, None]
    lane = np.arange(64)
    j, q = lane & 15, lane >> 4

    def W(l, out, inp):  # flat index of W_l[f, out, inp] for every feature: [features, len(out)]
        return w_off[l] + (f * dims[l + 1] + out[None, :]) * dims[l] + inp[None, :]

    for o in range(L.T[0]):
        for s in range(L.ks):
            k = 4 * s + q
            src = W(0, 16 * o + j, np.minimum(1 + k, S))
            src[:, k >= S] = -1
            base = L.o_w0s + (o * L.ks + s) * 64
            idx[:, base : base + 64] = src
    u = np.arange(widths[0])
    idx[:, L.o_w0x : L.o_w0x + widths[0]] = W(0, u, np.zeros_like(u))
    idx[:, L.o_b0 : L.o_b0 + widths[0]] = b_off[0] + f * widths[0] + u[None, :]
    e = np.arange(256)
    el, er = e >> 2, e & 3
    for l in range(1, len(widths)):
        for o in range(L.T[l]):
            for i in range(L.T[l - 1]):
                base = L.o_w[l] + (o * L.T[l - 1] + i) * 256
                idx[:, base : base + 256] = W(l, 16 * o + (el & 15), 16 * i + 4 * (el >> 4) + er)
        u = np.arange(widths[l])
        idx[:, L.o_b[l] : L.o_b[l] + widths[l]] = b_off[l] + f * widths[l] + u[None, :]
    n = len(widths)
    u = np.arange(widths[-1])
    idx[:, L.o_wl : L.o_wl + widths[-1]] = W(n, np.zeros_like(u), u)
    idx[:, L.o_bl] = b_off[n] + f[:, 0]
    assert idx.max() < 2**31
    return idx.astype(np.int32)


BWD_TILES = 4  # MNN_BWD_TM of csrc/mnn_backward.hip: the adjoint keeps widths <= 64
BWD_SCRATCH = 4 * 512  # floats of per-wave transpose scratch behind the image


@dataclass
class BackwardLayout:
    """What the adjoint kernel (csrc/mnn_backward.hip: mnn_bwd_layout) adds to `Layout`: the backward image = the forward image followed by

        wT_l   [T_{l-1}][T_l][256]  lane (j, q), r of tile (i, o): |W_l[16 o + 4 q + r][16 i + j]| — the A operands of A_l^T pb, the gradient in
                                    the accumulator layout of the layer above being the B operand as it stands
        w0sT   [ts][T_0][256]       tile (i, o): |W_0[16 o + 4 q + r][1 + 16 i + j]|, zeros behind S (ts = ceil(S / 16))

    and the layout of one (row chunk, column) partial of the parameter gradients, in the accumulator layout the kernel holds them in:

        g_w0s  [T_0][ts][256]       lane (j, q), r of tile (o, i): W_0[16 o + 4 q + r][1 + 16 i + j]
        g_w0x  [H_0]   g_b0 [H_0]
        g_w_l  [T_l][T_{l-1}][256]  lane (j, q), r of tile (o, i): W_l[16 o + 4 q + r][16 i + j]      g_b_l [H_l]
        g_wl   [H_last]   g_bl [4]
    """

    fwd: Layout
    ts: int = 0
    o_wT: list = field(default_factory=list)
    o_w0sT: int = 0
    total: int = 0
    g_w0s: int = 0
    g_w0x: int = 0
    g_b0: int = 0
    g_w: list = field(default_factory=list)
    g_b: list = field(default_factory=list)
    g_wl: int = 0
    g_bl: int = 0
    g_total: int = 0


def layout_backward(S: int, widths) -> BackwardLayout | None:
    """Offsets of one feature's backward image and of one gradient partial, or None for a shape the adjoint kernel does not serve.  `layout` and
    `index_table` are untouched: the backward image begins with the forward image."""
    L = layout(S, widths)
    if L is None or any(t > BWD_TILES for t in L.T):
        return None
    B = BackwardLayout(L, ts=(L.S + 15) // 16)
    n = len(L.widths)
    o = L.total
    B.o_wT = [0]
    for l in range(1, n):
        B.o_wT.append(o)
        o += L.T[l] * L.T[l - 1] * 256
    B.o_w0sT, o = o, o + B.ts * L.T[0] * 256
    B.total = o
    g = 0
    B.g_w0s, g = g, g + L.T[0] * B.ts * 256
    B.g_w0x, g = g, g + L.widths[0]
    B.g_b0, g = g, g + L.widths[0]
    B.g_w, B.g_b = [0], [0]
    for l in range(1, n):
        B.g_w.append(g)
        g += L.T[l] * L.T[l - 1] * 256
        B.g_b.append(g)
        g += L.widths[l]
    B.g_wl, g = g, g + L.widths[-1]
    B.g_bl, g = g, g + 4
    B.g_total = g
    return B if 4 * (max(B.total, B.g_total) + BWD_SCRATCH) <= LDS_MAX else None


def _flat_index(S: int, widths, features: int):
    dims = [1 + S, *widths, 1]
    w_off, b_off, total = flat_offsets(S, widths, features)
    f = np.arange(features, dtype=np.int64)[:, None]

    def W(l, out, inp):  # flat index of W_l[f, out, inp] for every feature: [features, len(out)]
        return w_off[l] + (f * dims[l + 1] + out[None, :]) * dims[l] + inp[None, :]

    return W, b_off, f, total


def index_table_backward(S: int, widths, features: int) -> np.ndarray:
    """int32 [features, backward image floats]: `index_table` followed by the transposed sections."""
    B = layout_backward(S, widths)
    assert B is not None
    L = B.fwd
    W, _, _, _ = _flat_index(S, widths, features)
    idx = np.full((features, B.total), -1, dtype=np.int64)
    idx[:, : L.total] = index_table(S, widths, features)
    e = np.arange(256)
    j, q, r = (e >> 2) & 15, e >> 6, e & 3
    for l in range(1, len(widths)):
        for i in range(L.T[l - 1]):
            for o in range(L.T[l]):
                base = B.o_wT[l] + (i * L.T[l] + o) * 256
                idx[:, base : base + 256] = W(l, 16 * o + 4 * q + r, 16 * i + j)
    for i in range(B.ts):
        for o in range(L.T[0]):
            k = 16 * i + j
            src = W(0, 16 * o + 4 * q + r, np.minimum(1 + k, S))
            src[:, k >= S] = -1
            base = B.o_w0sT + (i * L.T[0] + o) * 256
            idx[:, base : base + 256] = src
    assert idx.max() < 2**31
    return idx.astype(np.int32)


def grad_table(S: int, widths, features: int) -> np.ndarray:
    """int32 [features, g_total]: where every float of a feature's gradient partial goes in `flat_parameters` (-1 = nowhere).  Every flat parameter
    is named exactly once: the table is the inverse of a bijection between the partial's used floats and the flat parameters."""
    B = layout_backward(S, widths)
    assert B is not None
    L = B.fwd
    n = len(widths)
    W, b_off, f, _ = _flat_index(S, widths, features)
    idx = np.full((features, B.g_total), -1, dtype=np.int64)
    e = np.arange(256)
    j, q, r = (e >> 2) & 15, e >> 6, e & 3
    for o in range(L.T[0]):
        for i in range(B.ts):
            k = 16 * i + j
            src = W(0, 16 * o + 4 * q + r, np.minimum(1 + k, S))
            src[:, k >= S] = -1
            base = B.g_w0s + (o * B.ts + i) * 256
            idx[:, base : base + 256] = src
    u = np.arange(widths[0])
    idx[:, B.g_w0x : B.g_w0x + widths[0]] = W(0, u, np.zeros_like(u))
    idx[:, B.g_b0 : B.g_b0 + widths[0]] = b_off[0] + f * widths[0] + u[None, :]
    for l in range(1, n):
        for o in range(L.T[l]):
            for i in range(L.T[l - 1]):
                base = B.g_w[l] + (o * L.T[l - 1] + i) * 256
                idx[:, base : base + 256] = W(l, 16 * o + 4 * q + r, 16 * i + j)
        u = np.arange(widths[l])
        idx[:, B.g_b[l] : B.g_b[l] + widths[l]] = b_off[l] + f * widths[l] + u[None, :]
    u = np.arange(widths[-1])
    idx[:, B.g_wl : B.g_wl + widths[-1]] = W(n, np.zeros_like(u), u)
    idx[:, B.g_bl] = b_off[n] + f[:, 0]
    assert idx.max() < 2**31
    return idx.astype(np.int32)


def _linears(network):
    return [m for m in network if hasattr(m, "weight")]


def is_signed(network) -> bool:
    """True for the integrand network of a UMNN (plain `Linear`s: signed weights), False for a MonotonicMLP (|W|)."""
    from .nn import MonotonicLinear

    return not any(isinstance(l, MonotonicLinear) for l in _linears(network))


def shape_of(network):
    """(S, hidden widths, features) of a stacked MonotonicMLP(1 + S, 1, ...) or of a stacked MLP(1 + S, 1, ...) whose activations are all
    ELU(alpha = 1) (the integrand of a UMNN), or None when it is something else."""
    import torch.nn as nn

    lins = _linears(network)
    if len(lins) < 2 or any(l.weight.dim() != 3 or l.bias is None for l in lins):
        return None
    if len(list(network)) != 2 * len(lins) - 1 or lins[-1].weight.shape[1] != 1:
        return None
    if is_signed(network) and any(type(m) is not nn.ELU or m.alpha != 1.0 for m in network if not hasattr(m, "weight")):
        return None  # (the kernel of the signed networks knows the plain ELU only)
    return lins[0].weight.shape[2] - 1, tuple(l.weight.shape[1] for l in lins[:-1]), lins[0].weight.shape[0]


def flat_parameters(network):
    lins = _linears(network)
    if is_signed(network):
        return torch.cat([l.weight.detach().reshape(-1) for l in lins] + [l.bias.detach().reshape(-1) for l in lins])
    return torch.cat([l.weight.detach().abs().reshape(-1) for l in lins] + [l.bias.detach().reshape(-1) for l in lins])


class Image:
    """Device image of a network's parameters, rebuilt when a parameter's version (or storage) changes."""

    def __init__(self, network, device):
        self.S, self.widths, self.features = shape_of(network)
        self.layout = layout(self.S, self.widths)
        self.idx = torch.from_numpy(index_table(self.S, self.widths, self.features).reshape(-1)).to(device)
        self.data = torch.empty(self.idx.numel(), dtype=torch.float32, device=device)
        self.version = None

    def refresh(self, network):
        from . import _C
        from .nn import _param_stamp

        version = _param_stamp(_linears(network))
        if version != self.version:
            flat = flat_parameters(network).float()
            _C.check(_C.lib().zk_gather_f32(flat.data_ptr(), None, self.idx.data_ptr(), self.idx.numel(), self.data.data_ptr(), _C.stream()), "zk_gather_f32")
            self.version = version
        return self.data


class BackwardImage(Image):
    """Device backward image (forward image + transposed sections) and the gradient table of the adjoint kernel."""

    def __init__(self, network, device):
        self.S, self.widths, self.features = shape_of(network)
        self.layout = layout(self.S, self.widths)
        self.backward = layout_backward(self.S, self.widths)
        self.idx = torch.from_numpy(index_table_backward(self.S, self.widths, self.features).reshape(-1)).to(device)
        self.table = torch.from_numpy(grad_table(self.S, self.widths, self.features).reshape(-1)).to(device)
        self.data = torch.empty(self.idx.numel(), dtype=torch.float32, device=device)
        w_off, b_off, total = flat_offsets(self.S, self.widths, self.features)
        self.flat_weights, self.flat_total = b_off[0], total
        self.version = None


def backward_image_of(network, device, signed: bool = False) -> BackwardImage | None:
    """The cached backward image of a MonotonicMLP stack (`signed`: of the integrand networks of a UMNN, whose weights enter as they are) on
    `device` (zuko_amd.invalidate drops it), or None for the other kind of network and outside the adjoint's envelope."""
    sh = shape_of(network)
    if sh is None or is_signed(network) != bool(signed) or layout_backward(sh[0], sh[1]) is None:
        return None
    key = (str(device), sh)
    cache = network.__dict__.get("_mnn_bwd_image_cache")
    if cache is None or cache[0] != key:
        cache = (key, BackwardImage(network, device))
        network.__dict__["_mnn_bwd_image_cache"] = cache
    return cache[1]


def image_of(network, device) -> Image | None:
    """The cached image of `network` on `device` (zuko_amd.invalidate drops it), or None for a shape the kernel does not serve."""
    sh = shape_of(network)
    if sh is None or layout(sh[0], sh[1]) is None:
        return None
    key = (str(device), sh)
    cache = network.__dict__.get("_mnn_image_cache")
    if cache is None or cache[0] != key:
        cache = (key, Image(network, device))
        network.__dict__["_mnn_image_cache"] = cache
    return cache[1]
