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
use the same image with the SIGNED weights: `flat_parameters` takes no absolute value for them.
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
