"""Torch restatement of the adjoint of the continuous flow, independent of zuko_amd and of autograd: (a) the closed-form reverse sweep of one field
evaluation, (b) the six-stage reverse Dormand-Prince step of the augmented system (x, a, g_phi), (c) the whole backward over a list of accepted
steps.  float32 or float64, any device.  tests/test_cnf_adjoint_host.py pins all three to autograd on tests/cnf_ref.py: field in float64; the GPU
tests compare zk_cnf_adjoint_step with (b) and (c)."""

from __future__ import annotations

import torch

from cnf_ref import NODES, STAGES, TRACE_SCALE


def sweep(W, B, freqs, t, x, a, beta=None, c=None):
    """The vector-Jacobian products of Phi = sum_n a_n . f(t, x_n | c_n) + beta_n trace(df/dx)(t, x_n | c_n), in closed form:
    (f, dPhi/dx [N, F], [dPhi/dW_l], [dPhi/db_l], dPhi/dpre [N, H_1], dPhi/dc [N, C] | None).  beta = None: the value term alone.

    With p_l the pre-activations, D_l = ELU'(p_l), D'_l = ELU''(p_l) = (p_l > 0 ? 0 : D_l):
      trace, all features at once ([N, H_l, F]):  T_1 = D_1 o W0x, Z_{l+1} = W_{l+1} T_l, T_{l+1} = D_{l+1} o Z_{l+1};
             Tb_L = beta W_last^T, Db_l += sum_i Tb_l o Z_l, Zb_l = Tb_l o D_l, Tb_{l-1} = W_l^T Zb_l
      value  hb_L = W_last^T a, pb_l = D_l o hb_l + Db_l o D'_l, hb_{l-1} = W_l^T pb_l."""
    Q, F, n = freqs.numel(), x.shape[-1], len(W) - 1
    arg = freqs * t
    emb = torch.cat((arg.cos(), arg.sin())).expand(x.shape[0], 2 * Q)
    h = torch.cat((emb, x) if c is None else (emb, x, c.expand(x.shape[0], -1)), dim=-1)
    hs, ps, Ds = [h], [], []
    for l in range(n):
        p = hs[-1] @ W[l].T + B[l]
        ps.append(p)
        Ds.append(torch.where(p > 0, torch.ones_like(p), p.exp()))
        hs.append(torch.where(p > 0, p, torch.expm1(p)))
    f = hs[-1] @ W[n].T + B[n]
    gW = [torch.zeros_like(w) for w in W]
    Db = [torch.zeros_like(p) for p in ps]
    if beta is not None:
        Z = [W[0][:, 2 * Q : 2 * Q + F].expand(x.shape[0], -1, -1)]
        T = [Ds[0].unsqueeze(-1) * Z[0]]
        for l in range(1, n):
            Z.append(W[l] @ T[-1])
            T.append(Ds[l].unsqueeze(-1) * Z[-1])
        gW[n] += torch.einsum("n,nhi->ih", beta, T[-1])
        Tb = beta[:, None, None] * W[n].T
        for l in range(n - 1, -1, -1):
            Db[l] += (Tb * Z[l]).sum(dim=-1)
            Zb = Tb * Ds[l].unsqueeze(-1)
            if l > 0:
                gW[l] += torch.einsum("nhi,nki->hk", Zb, T[l - 1])
                Tb = torch.einsum("hk,nhi->nki", W[l], Zb)
            else:
                gW[0][:, 2 * Q : 2 * Q + F] += Zb.sum(dim=0)
    gW[n] += a.T @ hs[-1]
    gB = [None] * n + [a.sum(dim=0)]
    hb = a @ W[n]
    pb = None
    for l in range(n - 1, -1, -1):
        pb = Ds[l] * hb + Db[l] * torch.where(ps[l] > 0, torch.zeros_like(ps[l]), Ds[l])
        gW[l] += pb.T @ hs[l]
        gB[l] = pb.sum(dim=0)
        hb = pb @ W[l]
    return f, hb[:, 2 * Q : 2 * Q + F], gW, gB, pb, (None if c is None else hb[:, 2 * Q + F :])


def _combine(x0, row, ks):
    for a, k in zip(row, ks):
        if a != 0:
            x0 = x0 + a * k
    return x0


def reverse_step(W, B, freqs, t, dt, x, ax, al=None, c=None):
    """One reverse step from the checkpoint (x, t, dt) AFTER a forward step: (ax_next, [g W_l], [g b_l], g pre [N, H_1], g c [N, C] | None), the
    gradients being this step's INCREMENTS.  Six stages of size -dt, the sums left to right as dopri45 writes them; stage s adds
    b_s (-dt) (-(a_s^T df/dphi + al s d trace/dphi)) to every parameter component."""
    t, dt = torch.as_tensor(t, dtype=x.dtype, device=x.device), torch.as_tensor(dt, dtype=x.dtype, device=x.device)
    h = -dt
    beta = None if al is None else al * TRACE_SCALE
    kx, ka, kW, kB, kpre, kc = [], [], [], [], [], []
    for s in range(6):
        xs, as_ = _combine(x, STAGES[s], kx), _combine(ax, STAGES[s], ka)
        f, v, gW, gB, gpre, gc = sweep(W, B, freqs, t + NODES[s] * h, xs, as_, beta, c)
        kx.append(h * f)
        ka.append(h * (-v))
        kW.append([h * (-g) for g in gW])
        kB.append([h * (-g) for g in gB])
        kpre.append(h * (-gpre))
        kc.append(None if gc is None else h * (-gc))
    zero = lambda like: torch.zeros_like(like)
    fifth = STAGES[6]
    return (_combine(ax, fifth, ka),
            [_combine(zero(w), fifth, [k[l] for k in kW]) for l, w in enumerate(W)],
            [_combine(zero(b), fifth, [k[l] for k in kB]) for l, b in enumerate(B)],
            _combine(zero(kpre[0]), fifth, kpre),
            None if c is None else _combine(zero(kc[0]), fifth, kc))


def backward(W, B, freqs, steps, ax, al=None, c=None):
    """The whole backward over the accepted steps [(x_after, t_after, dt)], taken in reverse: (ax(t0), [g W_l], [g b_l], g pre, g c | None)."""
    gW, gB = [torch.zeros_like(w) for w in W], [torch.zeros_like(b) for b in B]
    gpre, gc = None, None
    for x, t, dt in reversed(list(steps)):
        ax, dW, dB, dpre, dc = reverse_step(W, B, freqs, t, dt, x, ax, al, c)
        gW, gB = [g + d for g, d in zip(gW, dW)], [g + d for g, d in zip(gB, dB)]
        gpre = dpre if gpre is None else gpre + dpre
        gc = dc if (gc is None or dc is None) else gc + dc
    return ax, gW, gB, gpre, gc
