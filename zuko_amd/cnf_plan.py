r"""Weight image of the vector field of a continuous normalizing flow (csrc/cnf.hip).

The field is `MLP(2 Q + F + C, F, hidden)` with ELU(alpha = 1) on `cat(cos(freqs t), sin(freqs t), x, c)` (zuko/flows/continuous.py:79-97): Q frequencies,
F features, C context features.  Its first layer splits as W0 = [W0t | W0x | W0c]; the context's share `c W0c^T + b0` is constant over an integration
and is computed on the host side once (`pre`), so neither W0c nor b0 is in the image.  The kernel keeps the rest in LDS, `image_floats` floats:

    fr    [8]                  the frequencies (zeros behind Q)
    w0t   [T1][kt][64]         lane (j, q) of tile o, k-step s: W0[16 o + j][4 s + q]           (kt = ceil(2 Q / 4), zeros behind 2 Q)
    w0x   [T1][kx][64]         lane (j, q) of tile o, k-step s: W0[16 o + j][2 Q + 4 s + q]     (kx = ceil(F / 4), zeros behind F)
    w0c   [F][H1]              W0[:, 2 Q + i]: the tangent that enters the first layer for feature i
    per further hidden layer l:
    w_l   [T_l][T_{l-1}][256]  lane (j, q), r = 0..3 of tile (o, i): W_l[16 o + j][16 i + 4 q + r]   (the tiles of mnn_plan.py)
    b_l   [H_l]
    wo    [T_last][256]        the last layer as ONE out tile whose row m is feature 4 (m & 3) + (m >> 2) (zero rows behind F): register r of
                               lane (j, q) of its product is then feature 4 r + q, the distribution in which the kernel keeps the state
    bo    [16]                 bo[4 q + r] = b_last[4 r + q] (zeros behind F)
    wl    [F][H_last]          W_last[i, :]: the row the tangent of feature i meets for the trace

`index_table` addresses `flat_parameters` = the weights, the biases, then the `freqs` buffer; zk_gather_f32 builds the image from it on the
device.  The arithmetic of `layout` is the one of csrc/cnf.hip: cnf_layout (zk_cnf_image_floats returns its total; tests compare the two).
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

LDS_MAX = 128 * 1024  # MNN_LDS_MAX of csrc/zk_mnn_common.h
FEATURES_MAX = 16
FREQS_MAX = 8


@dataclass
class Layout:
    F: int
    Q: int
    widths: tuple
    kt: int = 0
    kx: int = 0
    T: tuple = ()
    o_fr: int = 0
    o_w0t: int = 0
    o_w0x: int = 0
    o_w0c: int = 0
    o_w: list = field(default_factory=list)  # per hidden layer l >= 1
    o_b: list = field(default_factory=list)
    o_wo: int = 0
    o_bo: int = 0
    o_wl: int = 0
    total: int = 0


def layout(F: int, Q: int, widths) -> Layout | None:
    """Offsets of the image, or None for a shape the kernel does not serve."""
    widths = tuple(int(w) for w in widths)
    if not (1 <= F <= FEATURES_MAX and 1 <= Q <= FREQS_MAX and 1 <= len(widths) <= 3) or any(w < 16 or w > 128 or w % 16 for w in widths):
        return None
    L = Layout(int(F), int(Q), widths, kt=(2 * Q + 3) // 4, kx=(F + 3) // 4, T=tuple(w // 16 for w in widths))
    o = 0
    L.o_fr, o = o, o + 8
    L.o_w0t, o = o, o + L.T[0] * L.kt * 64
    L.o_w0x, o = o, o + L.T[0] * L.kx * 64
    L.o_w0c, o = o, o + F * widths[0]
    L.o_w, L.o_b = [0], [0]
    for l in range(1, len(widths)):
        L.o_w.append(o)
        o += L.T[l] * L.T[l - 1] * 256
        L.o_b.append(o)
        o += widths[l]
    L.o_wo, o = o, o + L.T[-1] * 256
    L.o_bo, o = o, o + 16
    L.o_wl, o = o, o + F * widths[-1]
    L.total = o
    return L if 4 * o <= LDS_MAX else None


def flat_offsets(F: int, Q: int, C: int, widths):
    """Offsets of every parameter tensor inside `flat_parameters`: ([weights...], [biases...], freqs, total)."""
    dims = [2 * Q + F + C, *widths, F]
    w_off, b_off, o = [], [], 0
    for a, b in zip(dims[:-1], dims[1:]):
        w_off.append(o)
        o += b * a
    for b in dims[1:]:
        b_off.append(o)
        o += b
    return w_off, b_off, o, o + Q


def index_table(F: int, Q: int, C: int, widths) -> np.ndarray:
    """int32 [image_floats]: where every float of the image comes from in `flat_parameters` (-1 = zero)."""
    L = layout(F, Q, widths)
    assert L is not None
    widths = L.widths
    dims = [2 * Q + F + C, *widths, F]
    w_off, b_off, f_off, _ = flat_offsets(F, Q, C, widths)
    idx = np.full(L.total, -1, dtype=np.int64)
    lane = np.arange(64)
    j, q = lane & 15, lane >> 4

    def W(l, out, inp):
        return w_off[l] + out * dims[l] + inp

    idx[L.o_fr : L.o_fr + Q] = f_off + np.arange(Q)
    for o in range(L.T[0]):
        for s in range(L.kt):
            k = 4 * s + q
            base = L.o_w0t + (o * L.kt + s) * 64
            idx[base : base + 64] = np.where(k < 2 * Q, W(0, 16 * o + j, np.minimum(k, 2 * Q - 1)), -1)
        for s in range(L.kx):
            k = 4 * s + q
            base = L.o_w0x + (o * L.kx + s) * 64
            idx[base : base + 64] = np.where(k < F, W(0, 16 * o + j, 2 * Q + np.minimum(k, F - 1)), -1)
    u = np.arange(widths[0])
    for i in range(F):
        idx[L.o_w0c + i * widths[0] : L.o_w0c + (i + 1) * widths[0]] = W(0, u, 2 * Q + i)
    e = np.arange(256)
    el, er = e >> 2, e & 3
    ej, eq = el & 15, el >> 4
    for l in range(1, len(widths)):
        for o in range(L.T[l]):
            for i in range(L.T[l - 1]):
                base = L.o_w[l] + (o * L.T[l - 1] + i) * 256
                idx[base : base + 256] = W(l, 16 * o + ej, 16 * i + 4 * eq + er)
        idx[L.o_b[l] : L.o_b[l] + widths[l]] = b_off[l] + np.arange(widths[l])
    n = len(widths)
    feat = 4 * (ej & 3) + (ej >> 2)  # the feature in row m = ej of the last layer's one out tile
    for i in range(L.T[-1]):
        base = L.o_wo + i * 256
        idx[base : base + 256] = np.where(feat < F, W(n, np.minimum(feat, F - 1), 16 * i + 4 * eq + er), -1)
    m = np.arange(16)
    fb = 4 * (m & 3) + (m >> 2)
    idx[L.o_bo : L.o_bo + 16] = np.where(fb < F, b_off[n] + np.minimum(fb, F - 1), -1)
    u = np.arange(widths[-1])
    for i in range(F):
        idx[L.o_wl + i * widths[-1] : L.o_wl + (i + 1) * widths[-1]] = W(n, i, u)
    assert idx.max() < 2**31
    return idx.astype(np.int32)


WIDTH_MAX_BACKWARD = 64  # MNN_BWD_TM tiles of csrc/zk_mnn_bwd_common.h: the adjoint keeps every weight's gradient in registers
SCRATCH_BACKWARD = 4 * (512 + 512)  # transpose scratch and column sums of a block's four wavefronts (floats)


@dataclass
class BackwardLayout:
    """The BACKWARD image of csrc/cnf_backward.hip — the forward image followed by the transposed tiles — and one row chunk's partial:

        wT_l   [T_{l-1}][T_l][256]  lane (j, q), r of tile (i, o): W_l[16 o + 4 q + r][16 i + j]                       (l = 1, 2)
        woT    [T_last][kx][64]     lane (j, q) of tile o, k-step s: W_last[4 s + q][16 o + j]                         (zeros behind F)
        w0xT   [T_0][256]           lane (j, q), r of tile i: W0x[16 i + 4 q + r][feature 4 (j & 3) + (j >> 2)]        (zeros behind F)

    partial (g_*): every weight tile as lane (j, q), r -> [16 o + 4 q + r][16 i + j]; for w0t the column is the embedding's entry j, for w0x
    the feature j, for wo the row is feature j and the column unit 16 o + 4 q + r; biases in unit order; bo as the image's bo."""

    fwd: Layout
    o_wT: list = field(default_factory=list)
    o_woT: int = 0
    o_w0xT: int = 0
    total: int = 0
    g_w0t: int = 0
    g_w0x: int = 0
    g_w: list = field(default_factory=list)
    g_b: list = field(default_factory=list)
    g_wo: int = 0
    g_bo: int = 0
    g_total: int = 0


def layout_backward(F: int, Q: int, widths) -> BackwardLayout | None:
    """Offsets of the backward image and of a partial (csrc/cnf_backward.hip: cnf_adj_layout), or None for a shape the adjoint does not serve."""
    L = layout(F, Q, widths)
    if L is None or any(w > WIDTH_MAX_BACKWARD for w in L.widths):
        return None
    T, n = L.T, len(L.widths)
    B = BackwardLayout(L)
    o = L.total
    B.o_wT = [0]
    for l in range(1, n):
        B.o_wT.append(o)
        o += T[l] * T[l - 1] * 256
    B.o_woT, o = o, o + T[-1] * L.kx * 64
    B.o_w0xT, o = o, o + T[0] * 256
    B.total = o
    g = 0
    B.g_w0t, g = g, g + T[0] * 256
    B.g_w0x, g = g, g + T[0] * 256
    B.g_w, B.g_b = [0], [0]
    for l in range(1, n):
        B.g_w.append(g)
        g += T[l] * T[l - 1] * 256
        B.g_b.append(g)
        g += L.widths[l]
    B.g_wo, g = g, g + T[-1] * 256
    B.g_bo, g = g, g + 16
    B.g_total = g
    return B if 4 * (max(B.total, B.g_total) + SCRATCH_BACKWARD) <= LDS_MAX else None


def index_table_backward(F: int, Q: int, C: int, widths) -> np.ndarray:
    """int32 [backward image floats]: `index_table` followed by the transposed tiles' sources."""
    B = layout_backward(F, Q, widths)
    assert B is not None
    L = B.fwd
    widths = L.widths
    dims = [2 * Q + F + C, *widths, F]
    w_off, _, _, _ = flat_offsets(F, Q, C, widths)
    idx = np.full(B.total, -1, dtype=np.int64)
    idx[: L.total] = index_table(F, Q, C, widths)

    def W(l, out, inp):
        return w_off[l] + out * dims[l] + inp

    e = np.arange(256)
    el, er = e >> 2, e & 3
    ej, eq = el & 15, el >> 4
    n = len(widths)
    for l in range(1, n):
        for i in range(L.T[l - 1]):
            for o in range(L.T[l]):
                base = B.o_wT[l] + (i * L.T[l] + o) * 256
                idx[base : base + 256] = W(l, 16 * o + 4 * eq + er, 16 * i + ej)
    lane = np.arange(64)
    j, q = lane & 15, lane >> 4
    for o in range(L.T[-1]):
        for s in range(L.kx):
            k = 4 * s + q
            base = B.o_woT + (o * L.kx + s) * 64
            idx[base : base + 64] = np.where(k < F, W(n, np.minimum(k, F - 1), 16 * o + j), -1)
    feat = 4 * (ej & 3) + (ej >> 2)
    for i in range(L.T[0]):
        base = B.o_w0xT + i * 256
        idx[base : base + 256] = np.where(feat < F, W(0, 16 * i + 4 * eq + er, 2 * Q + np.minimum(feat, F - 1)), -1)
    assert idx.max() < 2**31
    return idx.astype(np.int32)


def grad_table(F: int, Q: int, C: int, widths) -> np.ndarray:
    """int32 [partial floats]: where every float of a partial goes in the flat gradient (-1 = nowhere: padding).  Every parameter the kernel owns —
    all but the context's columns of W0 and b0 — has exactly one position."""
    B = layout_backward(F, Q, widths)
    assert B is not None
    L = B.fwd
    widths = L.widths
    dims = [2 * Q + F + C, *widths, F]
    w_off, b_off, _, _ = flat_offsets(F, Q, C, widths)
    tab = np.full(B.g_total, -1, dtype=np.int64)

    def W(l, out, inp):
        return w_off[l] + out * dims[l] + inp

    e = np.arange(256)
    el, er = e >> 2, e & 3
    ej, eq = el & 15, el >> 4
    n = len(widths)
    for o in range(L.T[0]):
        unit = 16 * o + 4 * eq + er
        tab[B.g_w0t + o * 256 : B.g_w0t + (o + 1) * 256] = np.where(ej < 2 * Q, W(0, unit, np.minimum(ej, 2 * Q - 1)), -1)
        tab[B.g_w0x + o * 256 : B.g_w0x + (o + 1) * 256] = np.where(ej < F, W(0, unit, 2 * Q + np.minimum(ej, F - 1)), -1)
    for l in range(1, n):
        for o in range(L.T[l]):
            for i in range(L.T[l - 1]):
                base = B.g_w[l] + (o * L.T[l - 1] + i) * 256
                tab[base : base + 256] = W(l, 16 * o + 4 * eq + er, 16 * i + ej)
        tab[B.g_b[l] : B.g_b[l] + widths[l]] = b_off[l] + np.arange(widths[l])
    for o in range(L.T[-1]):
        tab[B.g_wo + o * 256 : B.g_wo + (o + 1) * 256] = np.where(ej < F, W(n, np.minimum(ej, F - 1), 16 * o + 4 * eq + er), -1)
    m = np.arange(16)
    fb = 4 * (m & 3) + (m >> 2)
    tab[B.g_bo : B.g_bo + 16] = np.where(fb < F, b_off[n] + np.minimum(fb, F - 1), -1)
    assert tab.max() < 2**31
    return tab.astype(np.int32)


def _linears(ode):
    return [m for m in ode if hasattr(m, "weight")]


def shape_of(module):
    """(features, context, hidden widths, freqs) of an `FFJTransform` whose field the kernel knows — a plain MLP (linear, ELU(alpha = 1))* linear with
    biases — or None when it is something else."""
    import torch.nn as nn

    ode, freqs = module.ode, module.freqs
    mods = list(ode)
    lins = _linears(ode)
    if len(lins) < 2 or len(mods) != 2 * len(lins) - 1 or any(l.weight.dim() != 2 or l.bias is None for l in lins):
        return None
    if any(hasattr(m, "weight") != (i % 2 == 0) for i, m in enumerate(mods)):
        return None
    if any(type(m) is not nn.ELU or m.alpha != 1.0 for m in mods[1::2]):
        return None
    F, Q = lins[-1].weight.shape[0], int(freqs.numel())
    C = lins[0].weight.shape[1] - 2 * Q - F
    if C < 0 or any(a.weight.shape[0] != b.weight.shape[1] for a, b in zip(lins[:-1], lins[1:])):
        return None
    return F, C, tuple(l.weight.shape[0] for l in lins[:-1]), Q


def flat_parameters(module):
    lins = _linears(module.ode)
    return torch.cat([l.weight.detach().reshape(-1) for l in lins] + [l.bias.detach().reshape(-1) for l in lins] + [module.freqs.detach().reshape(-1)])


class Image:
    """Device image of the field's parameters, rebuilt when a parameter's (or the frequencies') version or storage changes."""

    def __init__(self, module, device):
        self.F, self.C, self.widths, self.Q = shape_of(module)
        self.layout = layout(self.F, self.Q, self.widths)
        self.idx = torch.from_numpy(index_table(self.F, self.Q, self.C, self.widths)).to(device)
        self.data = torch.empty(self.idx.numel(), dtype=torch.float32, device=device)
        self.version = None

    def refresh(self, module):
        from . import _C
        from .nn import _param_stamp

        version = (_param_stamp(_linears(module.ode)), module.freqs.data_ptr(), module.freqs._version)
        if version != self.version:
            flat = flat_parameters(module).float()
            _C.check(_C.lib().zk_gather_f32(flat.data_ptr(), None, self.idx.data_ptr(), self.idx.numel(), self.data.data_ptr(), _C.stream()), "zk_gather_f32")
            self.version = version
        return self.data


def image_of(module, device) -> Image | None:
    """The cached image of an `FFJTransform` on `device` (zuko_amd.invalidate drops it), or None for a field the kernel does not serve."""
    sh = shape_of(module)
    if sh is None or layout(sh[0], sh[3], sh[2]) is None:
        return None
    key = (str(device), sh)
    cache = module.__dict__.get("_cnf_image_cache")
    if cache is None or cache[0] != key:
        cache = (key, Image(module, device))
        module.__dict__["_cnf_image_cache"] = cache
    return cache[1]


class BackwardImage:
    """Device image of the adjoint kernel (csrc/cnf_backward.hip) and its gradient table, rebuilt like `Image`."""

    def __init__(self, module, device):
        self.F, self.C, self.widths, self.Q = shape_of(module)
        self.layout = layout_backward(self.F, self.Q, self.widths)
        self.idx = torch.from_numpy(index_table_backward(self.F, self.Q, self.C, self.widths)).to(device)
        self.table = torch.from_numpy(grad_table(self.F, self.Q, self.C, self.widths)).to(device)
        self.data = torch.empty(self.idx.numel(), dtype=torch.float32, device=device)
        self.flat_total = flat_offsets(self.F, self.Q, self.C, self.widths)[2]  # weights and biases: the flat gradient's length
        self.version = None

    refresh = Image.refresh


def backward_image_of(module, device) -> BackwardImage | None:
    """The cached backward image of an `FFJTransform` on `device` (zuko_amd.invalidate drops it), or None for a field the adjoint kernel does not
    serve."""
    sh = shape_of(module)
    if sh is None or layout_backward(sh[0], sh[3], sh[2]) is None:
        return None
    key = (str(device), sh)
    cache = module.__dict__.get("_cnf_bwd_image_cache")
    if cache is None or cache[0] != key:
        cache = (key, BackwardImage(module, device))
        module.__dict__["_cnf_bwd_image_cache"] = cache
    return cache[1]
