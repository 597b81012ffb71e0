"""Independent torch restatement of the unconstrained monotone networks of an unconstrained neural autoregressive flow: the Gauss-Legendre
integral of exp(squash(h)), its log-derivative and the bisection inverse — the float32 / float64 reference of the GPU tests
(tests/test_umnn_host.py pins it to the fixtures the reference wrote, tests/golden/make_golden_unaf.py).

weights / biases: the stacked parameters of an MLP(1 + S, 1, hidden, stack=F) with ELU in layer order, weights[l] [F, out, in], biases[l]
[F, out].  x [N, D], signal [N, D, S], constant [N, D] | None; `feat` (a list / LongTensor of D indices, None = all F in order) picks the
network of every column.  Everything runs in the dtype of x.
"""

from __future__ import annotations

import math

import numpy as np
import torch


def rule(n: int, like: torch.Tensor):
    """(nodes, weights) of the n-point Gauss-Legendre rule on [0, 1]: numpy's float64 rule rounded to the dtype of `like`."""
    t, w = np.polynomial.legendre.leggauss(n)
    return torch.as_tensor((t + 1) / 2, dtype=like.dtype, device=like.device), torch.as_tensor(w / 2, dtype=like.dtype, device=like.device)


def _select(weights, biases, feat, like):
    W = [w.to(like) for w in weights]
    B = [b.to(like) for b in biases]
    if feat is not None:
        idx = torch.as_tensor(feat, dtype=torch.long, device=like.device)
        W, B = [w.index_select(0, idx) for w in W], [b.index_select(0, idx) for b in B]
    return W, B


def elu(p: torch.Tensor) -> torch.Tensor:
    return torch.where(p > 0, p, torch.expm1(torch.clamp(p, max=0)))


def squash(h: torch.Tensor) -> torch.Tensor:
    return h / (1 + (h / 7).abs())


def integrand_log(W, B, u, signal):
    """squash(h(u, signal)) [..., N, D] for u [..., N, D] with the selected parameters W, B: the logarithm of the integrand."""
    c0 = torch.einsum("dhs,nds->ndh", W[0][:, :, 1:], signal) + B[0]
    a = elu(W[0][:, :, 0] * u[..., None] + c0)
    for Wl, Bl in zip(W[1:-1], B[1:-1]):
        a = elu(torch.einsum("doh,...ndh->...ndo", Wl, a) + Bl)
    return squash(torch.einsum("doh,...ndh->...ndo", W[-1], a)[..., 0] + B[-1][:, 0])


def integral(W, B, x, signal, n: int):
    """x sum_i w_i g(t_i x), the sum in the order i = 0, 1, ..."""
    t, w = rule(n, x)
    acc = torch.zeros_like(x)
    for i in range(n):
        acc = acc + w[i] * torch.exp(integrand_log(W, B, t[i] * x, signal))
    return x * acc


def forward(weights, biases, x, signal, constant=None, feat=None, n: int = 32):
    """(y, ladj) [N, D] each."""
    W, B = _select(weights, biases, feat, x)
    y = integral(W, B, x, signal, n)
    return (y if constant is None else y + constant), integrand_log(W, B, x, signal)


def inverse(weights, biases, y, signal, constant=None, feat=None, n: int = 32, bound: float = 10.0, eps: float = 1e-6):
    """ceil(log2(2 bound / eps)) bisection steps on [-bound, bound] for f(x) = y - constant: c = (a + b) / 2, f(c) < target ? a = c : b = c;
    returns (a + b) / 2."""
    W, B = _select(weights, biases, feat, y)
    target = y if constant is None else y - constant
    lo, hi = torch.full_like(y, -bound), torch.full_like(y, bound)
    for _ in range(math.ceil(math.log2(2 * bound / eps))):
        c = (lo + hi) / 2
        below = integral(W, B, c, signal, n) < target
        lo, hi = torch.where(below, c, lo), torch.where(below, hi, c)
    return (lo + hi) / 2


def params_of(g: dict, device="cpu", dtype=torch.float32):
    """(weights, biases) of a fixture written by make_golden_unaf.py (keys w0, b0, w1, ...)."""
    n = sum(1 for k in g if k[0] == "w" and k[1:].isdigit())
    as_t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    return [as_t(g[f"w{l}"]) for l in range(n)], [as_t(g[f"b{l}"]) for l in range(n)]
