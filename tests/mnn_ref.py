"""Independent torch restatement of the monotone networks of a neural autoregressive flow: value with a forward-mode tangent, and the
bisection inverse — the float32 / float64 reference of the GPU tests (tests/test_mnn_host.py pins it to the fixtures the reference wrote,
tests/golden/make_golden_naf.py).

weights / biases: the stacked parameters of a MonotonicMLP(1 + S, 1, hidden, stack=F) in layer order, weights[l] [F, out, in],
biases[l] [F, out].  x [N, D], signal [N, D, S]; `feat` (a list / LongTensor of D indices, None = all F in order) picks the network of
every column.  Everything runs in the dtype of x.
"""

from __future__ import annotations

import math

import torch


def two_way_elu(p: torch.Tensor):
    """(act(p), act'(p)) over the last axis: ELU on the first ceil(H / 2) units, -ELU(-.) on the others (torch.chunk's split)."""
    H = p.shape[-1]
    first = torch.arange(H, device=p.device) < (H + 1) // 2
    s = torch.where(first, p, -p)
    a = torch.where(s > 0, s, torch.expm1(s))
    d = torch.where(s > 0, torch.ones_like(s), torch.exp(s))
    return torch.where(first, a, -a), d


def _select(weights, biases, feat, like):
    W = [w.to(like).abs() for w in weights]
    B = [b.to(like) for b in biases]
    if feat is not None:
        idx = torch.as_tensor(feat, dtype=torch.long, device=like.device)
        W, B = [w.index_select(0, idx) for w in W], [b.index_select(0, idx) for b in B]
    return W, B


def forward(weights, biases, x, signal, feat=None, tangent: bool = True):
    """(y, ladj) [N, D] each (ladj None without tangent)."""
    W, B = _select(weights, biases, feat, x)
    w0x = W[0][:, :, 0]  # [D, H1]: the column x multiplies, and the tangent that enters
    pre = w0x * x[..., None] + torch.einsum("dhs,nds->ndh", W[0][:, :, 1:], signal) + B[0]
    a, d = two_way_elu(pre)
    t = d * w0x if tangent else None
    for Wl, Bl in zip(W[1:-1], B[1:-1]):
        a, d = two_way_elu(torch.einsum("doh,ndh->ndo", Wl, a) + Bl)
        if tangent:
            t = d * torch.einsum("doh,ndh->ndo", Wl, t)
    y = torch.einsum("doh,ndh->ndo", W[-1], a)[..., 0] + B[-1][:, 0]
    if not tangent:
        return y, None
    return y, torch.einsum("doh,ndh->ndo", W[-1], t)[..., 0].log()


def inverse(weights, biases, y, signal, feat=None, bound: float = 10.0, eps: float = 1e-6):
    """n = ceil(log2(2 bound / eps)) bisection steps on [-bound, bound]: c = (a + b) / 2, f(c) < y ? a = c : b = c; returns (a + b) / 2."""
    lo, hi = torch.full_like(y, -bound), torch.full_like(y, bound)
    for _ in range(math.ceil(math.log2(2 * bound / eps))):
        c = (lo + hi) / 2
        below = forward(weights, biases, c, signal, feat, tangent=False)[0] < y
        lo, hi = torch.where(below, c, lo), torch.where(below, hi, c)
    return (lo + hi) / 2


def params_of(g: dict, device="cpu", dtype=torch.float32):
    """(weights, biases) of a fixture written by make_golden_naf.py (keys w0, b0, w1, ...)."""
    n = sum(1 for k in g if k[0] == "w" and k[1:].isdigit())
    as_t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    return [as_t(g[f"w{l}"]) for l in range(n)], [as_t(g[f"b{l}"]) for l in range(n)]
