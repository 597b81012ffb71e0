"""Torch restatement of the continuous flow's arithmetic, independent of zuko_amd and of autograd: the field and the trace of its Jacobian in closed
form, one Dormand-Prince step with the per-row error ratio, and the adaptive controller.  float32 or float64, any device.  tests/test_cnf_host.py
pins it to the reference's fixtures (tests/golden/make_golden_cnf.py); the GPU tests use it where no fixture exists."""

from __future__ import annotations

import math

import torch

TRACE_SCALE = 1e-2
NODES = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
STAGES = (
    (),
    (1 / 5,),
    (3 / 40, 9 / 40),
    (44 / 45, -56 / 15, 32 / 9),
    (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
    (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
    (35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84),
)
FOURTH = (5179 / 57600, 0, 7571 / 16695, 393 / 640, -92097 / 339200, 187 / 2100, 1 / 40)

ACTS = {
    "elu": (torch.nn.functional.elu, lambda p: torch.where(p > 0, torch.ones_like(p), p.exp())),
    "tanh": (torch.tanh, lambda p: 1 - torch.tanh(p) ** 2),
}


def params_of(g: dict, dtype=torch.float64, device="cpu"):
    """(W, B, freqs) of a fixture: lists of the layers' weights and biases."""
    n = sum(1 for k in g if k.startswith("w") and k[1:].isdigit())
    cast = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)
    return [cast(g[f"w{i}"]) for i in range(n)], [cast(g[f"b{i}"]) for i in range(n)], cast(g["freqs"])


def field(W, B, freqs, t, x, c=None, act="elu", eps=None):
    """(f(t, x | c), the trace of df/dx) of MLP(cat(cos(freqs t), sin(freqs t), x, c)).  Forward mode: T_1 = D_1 o W0x, T_{l+1} = D_{l+1} o (W_l T_l),
    J = W_last T.  With `eps` [N, F] the trace is Hutchinson's estimate eps^T J eps instead."""
    fn, dfn = ACTS[act]
    Q, F = freqs.numel(), x.shape[-1]
    arg = freqs * t
    emb = torch.cat((arg.cos(), arg.sin())).expand(x.shape[:-1] + (2 * Q,))
    h = torch.cat((emb, x) if c is None else (emb, x, c.expand(x.shape[:-1] + c.shape[-1:])), dim=-1)
    T = None  # [N, H_l, F]
    for l, (w, b) in enumerate(zip(W, B)):
        p = h @ w.T + b
        lin = w[:, 2 * Q : 2 * Q + F].expand(x.shape[:-1] + (w.shape[0], F)) if l == 0 else w @ T
        if l + 1 < len(W):
            h, T = fn(p), dfn(p).unsqueeze(-1) * lin
        else:
            h, T = p, lin
    if eps is None:
        return h, torch.diagonal(T, dim1=-2, dim2=-1).sum(dim=-1)
    return h, torch.einsum("...i,...ij,...j->...", eps, T, eps)


def step(W, B, freqs, t, dt, x, l=None, c=None, atol=1e-6, rtol=1e-5, act="elu", eps=None):
    """One attempted step from (t, x, l): (x_next, l_next | None, per-row ratio).  The sums add their terms left to right, a term at a time, as the
    reference writes them; l = None integrates the value alone."""
    t, dt = torch.as_tensor(t, dtype=x.dtype, device=x.device), torch.as_tensor(dt, dtype=x.dtype, device=x.device)
    kx, kl = [], []

    def combine(x0, row, ks):
        for a, k in zip(row, ks):
            if a != 0:
                x0 = x0 + a * k
        return x0

    xs = x
    for s in range(7):
        xs = combine(x, STAGES[s], kx)
        if s == 6:
            x_next = xs
            l_next = None if l is None else combine(l, STAGES[6], kl)
        f, tr = field(W, B, freqs, t + NODES[s] * dt, xs, c, act, eps)
        kx.append(dt * f)
        if l is not None:
            kl.append(dt * (tr * TRACE_SCALE))
    ratio = (abs(x_next - combine(x, FOURTH, kx)) / (atol + rtol * torch.max(abs(x), abs(x_next)))).max(dim=-1).values
    if l is not None:
        ratio = torch.max(ratio, abs(l_next - combine(l, FOURTH, kl)) / (atol + rtol * torch.max(abs(l), abs(l_next))))
    return x_next, l_next, ratio


def integrate(W, B, freqs, x, c=None, t0=0.0, t1=1.0, with_l=True, atol=1e-6, rtol=1e-5, act="elu", eps=None):
    """The reference's controller around `step`: (x(t1), l(t1) | None, attempts [A, 3] = (t, dt, accepted))."""
    t0, t1 = torch.as_tensor(t0, dtype=x.dtype), torch.as_tensor(t1, dtype=x.dtype)
    l = torch.zeros_like(x[..., 0]) if with_l else None
    t, dt = t0, t1 - t0
    sign = torch.sign(dt)
    attempts = []
    while sign * (t1 - t) > 0:
        dt = sign * torch.min(abs(dt), abs(t1 - t))
        while True:
            y, ln, ratio = step(W, B, freqs, t, dt, x, l, c, atol, rtol, act, eps)
            r = ratio.max().clip(min=1e-9).item()
            assert math.isfinite(r)
            attempts.append((t.item(), dt.item(), float(r < 1.0)))
            if r < 1.0:
                x, l, t = y, ln, t + dt
            dt = dt * min(10.0, max(0.1, 0.9 / r ** (1 / 5)))
            if r < 1.0:
                break
    return x, l, torch.tensor(attempts, dtype=torch.float64).reshape(-1, 3)
