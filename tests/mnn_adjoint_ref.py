"""Reference gradients of the monotone networks of a neural autoregressive flow, for the tests of zk_mnn_backward.

Two independent routes to the gradients of  sum(gy * y) + sum(gl * ladj)  with (y, ladj = log dy/dx) of the per-feature networks:

  * `autograd`: a torch restatement of the network on `torch.nn.functional.elu` (as the reference's TwoWayELU, zuko/nn.py), differentiated by
    autograd — the derivative dy/dx by torch.autograd.grad(create_graph=True), as zuko/transforms.py:623-637 takes it.  On the CPU in float32 it
    is the yardstick, in float64 the truth.  (tests/mnn_ref.py: two_way_elu is NOT differentiated: its torch.where(s > 0, s, expm1(s)) gives NaN
    gradients once expm1 overflows in the branch that is not selected.)
  * `closed_form`: the reverse sweep the kernel implements (csrc/mnn_backward.hip), in torch ops without autograd.

weights / biases as tests/mnn_ref.py: weights[l] [F, out, in] SIGNED (the network uses |W|), biases[l] [F, out]; x [N, D], signal [N, D, S]; `feat`
picks the network of every column (None = all F in order, every feature at most once).  gy [N, D] or None, gl [N, D] / [N] or None.  Both return
{"gx": [N, D], "gsignal": [N, D, S], "gW": [...], "gB": [...]} with parameter gradients of the FULL stacks (zeros for features not selected).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F


def two_way_elu(p: torch.Tensor) -> torch.Tensor:
    h = (p.shape[-1] + 1) // 2
    return torch.cat((F.elu(p[..., :h]), -F.elu(-p[..., h:])), dim=-1)


def _idx(feat, n, device):
    return torch.arange(n, device=device) if feat is None else torch.as_tensor(list(feat), dtype=torch.long, device=device)


def _up(gy, gl, like):
    gy = torch.zeros_like(like) if gy is None else gy.to(like)
    gl = torch.zeros_like(like) if gl is None else gl.to(like)
    return gy, (gl[:, None].expand_as(like) if gl.dim() == 1 else gl)


def network(W, B, x, signal, idx):
    h = torch.cat((x[..., None], signal), dim=-1)
    for l, (w, b) in enumerate(zip(W, B)):
        h = torch.einsum("doi,ndi->ndo", w.abs().index_select(0, idx), h) + b.index_select(0, idx)
        if l < len(W) - 1:
            h = two_way_elu(h)
    return h[..., 0]


def autograd(weights, biases, x, signal, gy, gl, feat=None, dtype=torch.float32):
    W = [w.detach().to(dtype).clone().requires_grad_() for w in weights]
    B = [b.detach().to(dtype).clone().requires_grad_() for b in biases]
    x, signal = x.detach().to(dtype).clone().requires_grad_(), signal.detach().to(dtype).clone().requires_grad_()
    idx = _idx(feat, W[0].shape[0], x.device)
    y = network(W, B, x, signal, idx)
    dy = torch.autograd.grad(y, x, torch.ones_like(y), create_graph=True)[0]
    gy, gl = _up(gy, gl, y)
    g = torch.autograd.grad((gy * y).sum() + (gl * dy.log()).sum(), [x, signal, *W, *B])
    n = len(W)
    return {"gx": g[0], "gsignal": g[1], "gW": list(g[2 : 2 + n]), "gB": list(g[2 + n :])}


def closed_form(weights, biases, x, signal, gy, gl, feat=None, dtype=torch.float64):
    W = [w.detach().to(dtype) for w in weights]
    B = [b.detach().to(dtype) for b in biases]
    x, signal = x.detach().to(dtype), signal.detach().to(dtype)
    idx = _idx(feat, W[0].shape[0], x.device)
    A = [w.abs().index_select(0, idx) for w in W]  # [D, out, in]
    b = [v.index_select(0, idx) for v in B]
    gy, gl = _up(gy, gl, x)
    nh = len(W) - 1

    def sigma(H):
        return torch.where(torch.arange(H, device=x.device) < (H + 1) // 2, 1.0, -1.0).to(dtype)

    u = torch.cat((x[..., None], signal), dim=-1)
    p, pd, v, t = [], [], [], []
    for l in range(nh):
        if l == 0:
            p.append(torch.einsum("doi,ndi->ndo", A[0], u) + b[0])
            pd.append(A[0][:, :, 0].expand_as(p[0]))
        else:
            p.append(torch.einsum("doi,ndi->ndo", A[l], v[-1]) + b[l])
            pd.append(torch.einsum("doi,ndi->ndo", A[l], t[-1]))
        sg = sigma(p[l].shape[-1])
        s = sg * p[l]
        v.append(sg * torch.where(s > 0, s, torch.expm1(s.clamp(max=0))))
        t.append(torch.where(s > 0, torch.ones_like(s), torch.exp(s.clamp(max=0))) * pd[l])
    aL = A[nh][:, 0, :]  # [D, H]
    dy = (aL * t[-1]).sum(-1)
    k = gl / dy
    gA = [torch.zeros_like(a) for a in A]
    gb = [torch.zeros_like(v_) for v_ in b]
    vb, tb = gy[..., None] * aL, k[..., None] * aL
    gA[nh][:, 0, :] = (gy[..., None] * v[-1] + k[..., None] * t[-1]).sum(0)
    gb[nh][:, 0] = gy.sum(0)
    gx = gs = None
    for l in range(nh - 1, -1, -1):
        sg = sigma(p[l].shape[-1])
        s = sg * p[l]
        e = torch.exp(s.clamp(max=0))
        d1 = torch.where(s > 0, torch.ones_like(s), e)
        d2 = torch.where(s > 0, torch.zeros_like(s), sg * e)
        pb = vb * d1 + tb * d2 * pd[l]
        pdb = tb * d1
        gb[l] = pb.sum(0)
        if l >= 1:
            gA[l] = torch.einsum("ndo,ndi->doi", pb, v[l - 1]) + torch.einsum("ndo,ndi->doi", pdb, t[l - 1])
            vb, tb = torch.einsum("doi,ndo->ndi", A[l], pb), torch.einsum("doi,ndo->ndi", A[l], pdb)
        else:
            gA[0] = torch.einsum("ndo,ndi->doi", pb, u)
            gA[0][:, :, 0] += pdb.sum(0)
            gx = (A[0][:, :, 0] * pb).sum(-1)
            gs = torch.einsum("doi,ndo->ndi", A[0][:, :, 1:], pb)
    gW = [torch.zeros_like(w).index_copy_(0, idx, torch.sign(w.index_select(0, idx)) * ga) for w, ga in zip(W, gA)]
    gB = [torch.zeros_like(v_).index_copy_(0, idx, g_) for v_, g_ in zip(B, gb)]
    return {"gx": gx, "gsignal": gs, "gW": gW, "gB": gB}


def flat(g: dict) -> torch.Tensor:
    """The parameter gradients in the order of zuko_amd.mnn_plan.flat_parameters: weights, then biases."""
    return torch.cat([w.reshape(-1) for w in g["gW"]] + [b.reshape(-1) for b in g["gB"]])


def all_finite(g: dict) -> bool:
    return all(bool(torch.isfinite(t).all()) for t in (g["gx"], g["gsignal"], *g["gW"], *g["gB"]))
