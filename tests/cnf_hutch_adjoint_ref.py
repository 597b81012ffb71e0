"""Torch restatement of the adjoint of the continuous flow under Hutchinson's estimator, independent of zuko_amd and of autograd: tests/cnf_adjoint_ref.py
with the trace of df/dx replaced by eps^T (df/dx) eps for a probe eps [N, F] that is constant along the integration and has no gradient — (a) the
closed-form reverse sweep of one field evaluation, (b) the six-stage reverse Dormand-Prince step, (c) the whole backward over a list of accepted
steps.  float32 or float64, any device.  tests/test_cnf_hutch_host.py pins all three to autograd on tests/cnf_ref.py: field(..., eps=) in float64; the
GPU tests compare zk_cnf_adjoint_step_v2 with (b) and (c)."""

from __future__ import annotations

import torch

from cnf_ref import NODES, STAGES, TRACE_SCALE


def sweep(W, B, freqs, t, x, a, beta=None, eps=None, c=None):
    """The vector-Jacobian products of Phi = sum_n a_n . f(t, x_n | c_n) + beta_n eps_n^T (df/dx)(t, x_n | c_n) eps_n, in closed form:
    (f, dPhi/dx [N, F], [dPhi/dW_l], [dPhi/db_l], dPhi/dpre [N, H_1], dPhi/dc [N, C] | None).  beta = None: the value term alone (eps is not read).

    With p_l the pre-activations, D_l = ELU'(p_l), D'_l = ELU''(p_l) = (p_l > 0 ? 0 : D_l):
      probe, ONE tangent ([N, H_l]):  Z_1 = W0x eps, T_l = D_l o Z_l, Z_{l+1} = W_{l+1} T_l;
             Tb_L = beta W_last^T eps, Db_l += Tb_l o Z_l, Zb_l = Tb_l o D_l, Tb_{l-1} = W_l^T Zb_l
             g W_last += beta eps T_L^T, g W_l += Zb_l T_{l-1}^T, g W0x += Zb_1 eps^T
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
        Z = [eps @ W[0][:, 2 * Q : 2 * Q + F].T]
        T = [Ds[0] * Z[0]]
        for l in range(1, n):
            Z.append(T[-1] @ W[l].T)
            T.append(Ds[l] * Z[-1])
        gW[n] += (beta[:, None] * eps).T @ T[-1]
        Tb = beta[:, None] * (eps @ W[n])
        for l in range(n - 1, -1, -1):
            Db[l] += Tb * Z[l]
            Zb = Tb * Ds[l]
            if l > 0:
                gW[l] += Zb.T @ T[l - 1]
                Tb = Zb @ W[l]
            else:
                gW[0][:, 2 * Q : 2 * Q + F] += Zb.T @ eps
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


def reverse_step(W, B, freqs, t, dt, x, ax, al=None, eps=None, c=None):
    """One reverse step from the checkpoint (x, t, dt) AFTER a forward step: (ax_next, [g W_l], [g b_l], g pre [N, H_1], g c [N, C] | None), the
    gradients being this step's INCREMENTS.  Six stages of size -dt, the sums left to right as dopri45 writes them; stage s adds
    b_s (-dt) (-(a_s^T df/dphi + al s d(eps^T (df/dx) eps)/dphi)) to every parameter component.  The probe is the same at every stage."""
    t, dt = torch.as_tensor(t, dtype=x.dtype, device=x.device), torch.as_tensor(dt, dtype=x.dtype, device=x.device)
    h = -dt
    beta = None if al is None else al * TRACE_SCALE
    kx, ka, kW, kB, kpre, kc = [], [], [], [], [], []
    for s in range(6):
        xs, as_ = _combine(x, STAGES[s], kx), _combine(ax, STAGES[s], ka)
        f, v, gW, gB, gpre, gc = sweep(W, B, freqs, t + NODES[s] * h, xs, as_, beta, eps, c)
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


def backward(W, B, freqs, steps, ax, al=None, eps=None, c=None):
    """The whole backward over the accepted steps [(x_after, t_after, dt)], taken in reverse: (ax(t0), [g W_l], [g b_l], g pre, g c | None)."""
    gW, gB = [torch.zeros_like(w) for w in W], [torch.zeros_like(b) for b in B]
    gpre, gc = None, None
    for x, t, dt in reversed(list(steps)):
        ax, dW, dB, dpre, dc = reverse_step(W, B, freqs, t, dt, x, ax, al, eps, c)
        gW, gB = [g + d for g, d in zip(gW, dW)], [g + d for g, d in zip(gB, dB)]
        gpre = dpre if gpre is None else gpre + dpre
        gc = dc if (gc is None or dc is None) else gc + dc
    return ax, gW, gB, gpre, gc
