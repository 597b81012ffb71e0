"""Reference gradients of the unconstrained monotone networks of an unconstrained neural autoregressive flow, for the tests of zk_umnn_backward.

Two independent routes to the gradients of  sum(gy * y) + sum(gl * ladj)  with (y, ladj) of tests/umnn_ref.py: forward:

  * `autograd`: tests/umnn_ref.py under autograd with the reference's semantics (GaussLegendre.backward, zuko/utils.py:282-326): the integral is
    taken at x.detach() — the nodes t_i x carry no gradient to x — and the integrand at the upper limit, gy * g(x), is added to gx; ladj =
    integrand_log(x) is differentiated as it stands.  On the CPU in float32 it is the yardstick, in float64 the truth.
  * `closed_form`: the reverse sweep the kernel implements (csrc/umnn_backward.hip), in torch ops without autograd.

weights / biases as tests/umnn_ref.py: weights[l] [F, out, in] (signed), biases[l] [F, out]; x [N, D], signal [N, D, S]; `feat` picks the network of
every column (None = all F in order, every feature at most once).  gy [N, D] or None, gl [N, D] / [N] or None.  Both return
{"gx": [N, D], "gsignal": [N, D, S], "gW": [...], "gB": [...]} with parameter gradients of the FULL stacks (zeros for features not selected).  The
constant's gradient is gy itself and is not returned.
"""

from __future__ import annotations

import torch

import umnn_ref
from mnn_adjoint_ref import _idx, _up, all_finite, flat  # noqa: F401  (the same conventions; `flat` and `all_finite` are part of this module's interface)


def autograd(weights, biases, x, signal, gy, gl, feat=None, n: int = 32, dtype=torch.float32):
    W = [w.detach().to(dtype).clone().requires_grad_() for w in weights]
    B = [b.detach().to(dtype).clone().requires_grad_() for b in biases]
    x, signal = x.detach().to(dtype).clone().requires_grad_(), signal.detach().to(dtype).clone().requires_grad_()
    idx = _idx(feat, W[0].shape[0], x.device)
    Ws, Bs = [w.index_select(0, idx) for w in W], [b.index_select(0, idx) for b in B]
    y = umnn_ref.integral(Ws, Bs, x.detach(), signal, n)
    ladj = umnn_ref.integrand_log(Ws, Bs, x, signal)
    gy, gl = _up(gy, gl, y)
    g = torch.autograd.grad((gy * y).sum() + (gl * ladj).sum(), [x, signal, *W, *B])
    k = len(W)
    return {"gx": g[0] + gy * torch.exp(ladj.detach()), "gsignal": g[1], "gW": list(g[2 : 2 + k]), "gB": list(g[2 + k :])}


def closed_form(weights, biases, x, signal, gy, gl, feat=None, n: int = 32, dtype=torch.float64):
    W = [w.detach().to(dtype) for w in weights]
    B = [b.detach().to(dtype) for b in biases]
    x, signal = x.detach().to(dtype), signal.detach().to(dtype)
    idx = _idx(feat, W[0].shape[0], x.device)
    A = [w.index_select(0, idx) for w in W]  # [D, out, in]
    b = [v.index_select(0, idx) for v in B]
    gy, gl = _up(gy, gl, x)
    nh = len(W) - 1
    t, w = umnn_ref.rule(n, x)
    q0 = torch.einsum("dhs,nds->ndh", A[0][:, :, 1:], signal) + b[0]
    gA = [torch.zeros_like(a) for a in A]
    gb = [torch.zeros_like(v) for v in b]
    P0 = torch.zeros_like(q0)
    gx = None
    for i in range(n + 1):  # the nodes in order, then x itself
        node = i < n
        u = t[i] * x if node else x
        p = [A[0][:, :, 0] * u[..., None] + q0]
        a = [umnn_ref.elu(p[0])]
        for l in range(1, nh):
            p.append(torch.einsum("doh,ndh->ndo", A[l], a[-1]) + b[l])
            a.append(umnn_ref.elu(p[l]))
        wl = A[nh][:, 0, :]  # [D, H]
        h = (wl * a[-1]).sum(-1) + b[nh][:, 0]
        den = 1 + h.abs() / 7
        g = torch.exp(h / den)
        hb = (gy * x * w[i] * g if node else gl) / den**2
        gA[nh][:, 0, :] += (hb[..., None] * a[-1]).sum(0)
        gb[nh][:, 0] += hb.sum(0)
        ab = hb[..., None] * wl
        for l in range(nh - 1, 0, -1):
            pb = ab * torch.where(p[l] > 0, torch.ones_like(p[l]), torch.exp(p[l].clamp(max=0)))
            gA[l] += torch.einsum("ndo,ndi->doi", pb, a[l - 1])
            gb[l] += pb.sum(0)
            ab = torch.einsum("doi,ndo->ndi", A[l], pb)
        pb = ab * torch.where(p[0] > 0, torch.ones_like(p[0]), torch.exp(p[0].clamp(max=0)))
        gA[0][:, :, 0] += (pb * u[..., None]).sum(0)
        P0 = P0 + pb
        if not node:
            gx = gy * g + (A[0][:, :, 0] * pb).sum(-1)
    gb[0] = P0.sum(0)
    gA[0][:, :, 1:] = torch.einsum("ndo,ndi->doi", P0, signal)
    gs = torch.einsum("doi,ndo->ndi", A[0][:, :, 1:], P0)
    gW = [torch.zeros_like(v).index_copy_(0, idx, ga) for v, ga in zip(W, gA)]
    gB = [torch.zeros_like(v).index_copy_(0, idx, g_) for v, g_ in zip(B, gb)]
    return {"gx": gx, "gsignal": gs, "gW": gW, "gB": gB}
