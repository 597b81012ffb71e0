"""Host: the adjoint of the continuous flow.  tests/cnf_adjoint_ref.py against autograd on tests/cnf_ref.py: field in float64 — the closed-form sweep,
the six-stage reverse step and the whole backward, the last two against the reference's algorithm (the `adjoint` of zuko/utils.py:572-585 under
dopri45) restated with autograd; the backward image's plan against the library; the argument block's refusals; the support predicate."""

import ctypes

import numpy as np
import pytest
import torch

import cnf_adjoint_ref as ref
import cnf_ref
from cnf_ref import NODES, STAGES, TRACE_SCALE

SHAPES = [(3, 2, (64, 64), 3), (5, 0, (64, 64), 3), (1, 0, (16,), 3), (16, 3, (16, 48, 64), 2), (6, 1, (32,), 8)]
BAR = 1e-10  # relative to the largest entry, float64


def _net(F, C, widths, Q, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    dims = [2 * Q + F + C, *widths, F]
    W = [(torch.rand(b, a, generator=g, dtype=torch.float64) * 2 - 1) * scale / a**0.5 for a, b in zip(dims[:-1], dims[1:])]
    B = [(torch.rand(b, generator=g, dtype=torch.float64) * 2 - 1) * 0.5 for b in dims[1:]]
    fr = torch.arange(1, Q + 1, dtype=torch.float64) * torch.pi
    N = 9
    x = torch.randn(N, F, generator=g, dtype=torch.float64)
    c = torch.randn(N, C, generator=g, dtype=torch.float64) if C else None
    a = torch.randn(N, F, generator=g, dtype=torch.float64)
    al = torch.randn(N, generator=g, dtype=torch.float64)
    return W, B, fr, x, c, a, al


def _close(got, want, what):
    scale = float(want.abs().max())
    d = float((got - want).abs().max())
    assert d <= BAR * max(scale, 1e-300), f"{what}: {d:.3e} against a largest entry of {scale:.3e}"


def _autograd_vjp(W, B, fr, t, x, c, a, beta):
    """(f, d/dx, [d/dW], [d/db], d/dc) of sum(a . f) + sum(beta trace) on cnf_ref.field, by autograd."""
    leaves = [x.clone().requires_grad_(), *[w.clone().requires_grad_() for w in W], *[b.clone().requires_grad_() for b in B]] + ([] if c is None else [c.clone().requires_grad_()])
    n = len(W)
    xx, WW, BB, cc = leaves[0], leaves[1 : 1 + n], leaves[1 + n : 1 + 2 * n], (None if c is None else leaves[-1])
    f, tr = cnf_ref.field(WW, BB, fr, t, xx, cc)
    phi = (a * f).sum() + (0 if beta is None else (beta * tr).sum())
    g = torch.autograd.grad(phi, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if v is None else v for v, l in zip(g, leaves)]
    return f.detach(), g[0], g[1 : 1 + n], g[1 + n : 1 + 2 * n], (None if c is None else g[-1])


@pytest.mark.parametrize("F,C,widths,Q", SHAPES)
def test_closed_form_sweep_equals_autograd(F, C, widths, Q):
    """x, every W and b, and c; the weights are scaled so that the rows have pre-activations on both sides of 0 in every layer."""
    W, B, fr, x, c, a, al = _net(F, C, widths, Q, seed=F + Q, scale=2.0)
    t = torch.tensor(0.37, dtype=torch.float64)
    h = torch.cat((torch.cat(((fr * t).cos(), (fr * t).sin())).expand(x.shape[0], -1), x) if c is None else (torch.cat(((fr * t).cos(), (fr * t).sin())).expand(x.shape[0], -1), x, c), dim=-1)
    for l in range(len(widths)):
        p = h @ W[l].T + B[l]
        assert bool((p > 0).any()) and bool((p < 0).any()), f"layer {l}: one-sided pre-activations"
        h = torch.nn.functional.elu(p)
    for beta in (al * TRACE_SCALE, None):
        f0, gx0, gW0, gB0, gc0 = _autograd_vjp(W, B, fr, t, x, c, a, beta)
        f, gx, gW, gB, gpre, gc = ref.sweep(W, B, fr, t, x, a, beta, c)
        _close(f, f0, "f")
        _close(gx, gx0, "d/dx")
        for l in range(len(W)):
            _close(gW[l], gW0[l], f"d/dW{l}")
            _close(gB[l], gB0[l], f"d/db{l}")
        _close(gpre.sum(dim=0), gB0[0], "d/dpre summed over the rows = d/db0")
        if c is not None:
            _close(gc, gc0, "d/dc")


def _reference_reverse(W, B, fr, steps, ax, al, c):
    """The reference's backward restated with autograd: dopri45(adjoint, (x, a, g_phi), t, -dt) over the steps in reverse, adjoint(t, state) =
    (f_aug, grad(f_aug, (x, phi), -a)) with f_aug = (f, trace * TRACE_SCALE) of cnf_ref.field; a's log-determinant component is constant."""
    phi = [*W, *B] + ([] if c is None else [c])
    n = len(W)

    def adjoint(t, state):
        x, a = state[0], state[1]
        xx = x.clone().requires_grad_()
        pp = [p.clone().requires_grad_() for p in phi]
        f, tr = cnf_ref.field(pp[:n], pp[n : 2 * n], fr, t, xx, None if c is None else pp[-1])
        outs, cots = [f], [-a]
        if al is not None:
            outs.append(tr * TRACE_SCALE)
            cots.append(-al)
        g = torch.autograd.grad(outs, [xx, *pp], cots, allow_unused=True)
        return [f.detach()] + [torch.zeros_like(l) if v is None else v for v, l in zip(g, [xx, *pp])]

    def combine(s0, row, ks):
        for a, k in zip(row, ks):
            if a != 0:
                s0 = [u + a * v for u, v in zip(s0, k)]
        return s0

    grads = [torch.zeros_like(p) for p in phi]
    for x, t, dt in reversed(steps):
        t, h = torch.as_tensor(t, dtype=x.dtype), -torch.as_tensor(dt, dtype=x.dtype)
        state, ks = [x, ax, *grads], []
        for s in range(6):
            ks.append([h * v for v in adjoint(t + NODES[s] * h, combine(state, STAGES[s], ks))])
        state = combine(state, STAGES[6], ks)
        ax, grads = state[1], state[2:]
    return ax, grads[:n], grads[n : 2 * n], (None if c is None else grads[-1])


@pytest.mark.parametrize("F,C,widths,Q", SHAPES)
def test_reverse_step_and_backward_equal_the_references_algorithm(F, C, widths, Q):
    W, B, fr, x, c, a, al = _net(F, C, widths, Q, seed=11 * F + Q)
    steps = [(x, 0.3, 0.3), (x + 0.05, 0.55, 0.25), (x * 0.9, 1.0, 0.45)]
    for with_l in (True, False):
        l = al if with_l else None
        # (b) one step
        ax0, gW0, gB0, gc0 = _reference_reverse(W, B, fr, steps[1:2], a, l, c)
        ax, gW, gB, gpre, gc = ref.reverse_step(W, B, fr, steps[1][1], steps[1][2], steps[1][0], a, l, c)
        _close(ax, ax0, "step: ax_next")
        for k in range(len(W)):
            _close(gW[k], gW0[k], f"step: g W{k}")
            _close(gB[k], gB0[k], f"step: g b{k}")
        _close(gpre.sum(dim=0), gB0[0], "step: g pre")
        if c is not None:
            _close(gc, gc0, "step: g c")
            Q2 = 2 * Q
            _close(gpre @ W[0][:, Q2 + F :], gc0, "step: g c from g pre")
            _close(gpre.T @ c, gW0[0][:, Q2 + F :], "step: the context's columns of g W0 from g pre")
        # (c) the whole backward
        ax0, gW0, gB0, gc0 = _reference_reverse(W, B, fr, steps, a, l, c)
        ax, gW, gB, gpre, gc = ref.backward(W, B, fr, steps, a, l, c)
        _close(ax, ax0, "backward: ax")
        for k in range(len(W)):
            _close(gW[k], gW0[k], f"backward: g W{k}")
            _close(gB[k], gB0[k], f"backward: g b{k}")
        if c is not None:
            _close(gc, gc0, "backward: g c")


def _floats(lib, F, Q, widths):
    w = list(widths) + [0, 0]
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.zk_cnf_adjoint_floats(F, Q, len(widths), w[0], w[1], w[2], ctypes.byref(a), ctypes.byref(b))
    return rc, a.value, b.value


def test_new_symbols_and_the_backward_plan_agree_with_the_library():
    import zuko_amd._C as C
    from zuko_amd import cnf_plan, ops

    lib, EINVAL = C.lib(), 1
    text = open(C._HEADER).read()
    for sym in ("zk_cnf_adjoint_step", "zk_cnf_adjoint_floats", "zk_cnf_adjoint_geometry", "zk_cnf_adjoint_workspace_floats"):
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym)
    assert "zk_cnf_adj_args_v1" in C.STRUCTS
    assert hasattr(ops, "CnfIntegrateFn") and hasattr(ops, "cnf_backward_supported") and ops.CNF_ADJOINT is False
    for F, C_, widths, Q in SHAPES + [(16, 0, (64, 64, 64), 8), (2, 0, (16, 16), 1)]:
        B = cnf_plan.layout_backward(F, Q, widths)
        assert B is not None and _floats(lib, F, Q, widths) == (0, B.total, B.g_total)
        assert B.total % 4 == 0 and B.g_total % 4 == 0
        idx, tab = cnf_plan.index_table_backward(F, Q, C_, widths), cnf_plan.grad_table(F, Q, C_, widths)
        assert idx.shape == (B.total,) and tab.shape == (B.g_total,)
        assert np.array_equal(idx[: B.fwd.total], cnf_plan.index_table(F, Q, C_, widths))
        w_off, b_off, flat, _ = cnf_plan.flat_offsets(F, Q, C_, widths)
        own = tab[tab >= 0]
        # every parameter but b0 and the context's columns of W0 has exactly one position in a partial
        want = np.ones(flat, dtype=bool)
        want[b_off[0] : b_off[0] + widths[0]] = False
        W0 = np.arange(widths[0] * (2 * Q + F + C_)).reshape(widths[0], -1)
        want[w_off[0] + W0[:, 2 * Q + F :].reshape(-1)] = False
        assert len(set(own.tolist())) == own.size and np.array_equal(np.sort(own), np.flatnonzero(want))
        # the transposed tiles hold the weights the forward tiles hold
        srcs = lambda lo, hi: set(idx[lo:hi][idx[lo:hi] >= 0].tolist())
        for l in range(1, len(widths)):
            n = B.fwd.T[l] * B.fwd.T[l - 1] * 256
            assert srcs(B.o_wT[l], B.o_wT[l] + n) == srcs(B.fwd.o_w[l], B.fwd.o_w[l] + n)
        assert srcs(B.o_woT, B.o_w0xT) == srcs(B.fwd.o_wo, B.fwd.o_bo) and srcs(B.o_w0xT, B.total) == srcs(B.fwd.o_w0x, B.fwd.o_w0c)
    assert cnf_plan.layout_backward(3, 3, (16, 48, 128)) is None and _floats(lib, 3, 3, (16, 48, 128))[0] == EINVAL
    assert cnf_plan.layout_backward(3, 3, (30, 30)) is None and _floats(lib, 3, 3, (30, 30))[0] == EINVAL
    # geometry: a pure function of N; chunks of a multiple of 64 rows
    rows, chunks = ctypes.c_int(), ctypes.c_int()
    for N, want in ((1, (64, 1)), (64, (64, 1)), (65, (64, 2)), (129, (64, 3)), (1 << 14, (64, 256)), ((1 << 14) + 1, (128, 129)), (1 << 16, (256, 256))):
        assert lib.zk_cnf_adjoint_geometry(N, ctypes.byref(rows), ctypes.byref(chunks)) == 0 and (rows.value, chunks.value) == want, N
    assert lib.zk_cnf_adjoint_geometry(0, ctypes.byref(rows), ctypes.byref(chunks)) == EINVAL
    n = ctypes.c_int64(-1)
    assert lib.zk_cnf_adjoint_workspace_floats(0, 3, 3, 2, 64, 64, 0, ctypes.byref(n)) == 0 and n.value == 0
    B = cnf_plan.layout_backward(3, 3, (64, 64))
    assert lib.zk_cnf_adjoint_workspace_floats(129, 3, 3, 2, 64, 64, 0, ctypes.byref(n)) == 0 and n.value >= 3 * B.g_total and n.value % 4 == 0
    assert lib.zk_cnf_adjoint_workspace_floats(129, 3, 3, 2, 64, 128, 0, ctypes.byref(n)) == EINVAL


def test_adjoint_step_rejects_foreign_blocks_and_unsupported_arguments_without_a_device():
    import zuko_amd._C as C

    lib, EINVAL = C.lib(), 1
    fn = lib.zk_cnf_adjoint_step
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    _, image, grad = _floats(lib, 5, 3, (64, 64))

    def block(N, **kw):
        base = dict(features=5, freqs=3, n_hidden=2, width0=64, width1=64, width2=0, image_floats=image, grad_floats=grad, N=N, ldx=5, ld_ax=5, ld_ax_next=5, ld_pre=64,
                    ld_gpre=64, flat_total=1, t=1.0, dt=0.25, trace_scale=1e-2, ax=p, ax_next=p)
        if N > 0:
            base.update(x=p, al=p, pre=p, image=p, grad_table=p, gpre=p, gparams=p, work=p)
        base.update(kw)
        return C.args("zk_cnf_adj_args_v1", **base)

    assert fn(block(0), None) == 0 and fn(block(0, ld_pre=0), None) == 0  # (N = 0 launches nothing)
    for N in (0, 4):
        for delta in (-8, 8):
            bad = block(N)
            bad.struct_size += delta
            assert fn(bad, None) == EINVAL
        bad = block(N)
        bad.version = 2
        assert fn(bad, None) == EINVAL
        i128, g128 = lib.zk_cnf_image_floats(5, 3, 2, 64, 128, 0), grad
        for kw in (dict(width1=128, image_floats=i128, grad_floats=g128), dict(n_hidden=3, width2=128), dict(ax=None), dict(ax_next=None), dict(ld_gpre=66), dict(ld_gpre=60),
                   dict(ld_pre=66), dict(ldx=4), dict(ld_ax=4), dict(ld_ax_next=4), dict(image_floats=image - 4), dict(grad_floats=grad + 4), dict(t=float("nan")),
                   dict(dt=float("inf")), dict(trace_scale=0.0), dict(features=17), dict(freqs=9)):
            assert fn(block(N, **kw), None) == EINVAL, (N, kw)
    assert fn(None, None) == EINVAL and fn(block(-1), None) == EINVAL
    for kw in (dict(x=None), dict(pre=None), dict(image=None), dict(gpre=None), dict(work=None), dict(grad_table=None), dict(pre=p + 4), dict(gpre=p + 8), dict(work=p + 4)):
        assert fn(block(4, **kw), None) == EINVAL, kw  # (rows, but a pointer is missing or not 16-byte aligned)


def test_backward_supported_truth_table():
    import torch.nn as nn

    from zuko_amd import ops

    yes = [dict(features=3, context=2), dict(features=5, context=0, hidden_features=(64, 64)), dict(features=1, hidden_features=(16,)),
           dict(features=16, context=3, hidden_features=(16, 48, 64), freqs=2), dict(features=6, context=1, hidden_features=(32,), freqs=8),
           dict(features=16, hidden_features=(64, 64, 64), freqs=8), dict(features=3, activation=nn.ELU)]
    no = [dict(features=3, hidden_features=(16, 48, 128)), dict(features=3, hidden_features=(128,)), dict(features=3, hidden_features=(80, 64)),
          dict(features=3, hidden_features=(30, 30)), dict(features=17), dict(features=3, freqs=9), dict(features=3, hidden_features=(16, 16, 16, 16)),
          dict(features=3, activation=nn.Tanh), dict(features=3, activation=lambda: nn.ELU(alpha=0.5)), dict(features=3, context=-1)]
    for kw in yes:
        assert ops.cnf_backward_supported(**kw) and ops.cnf_supported(**kw), kw
    for kw in no:
        assert not ops.cnf_backward_supported(**kw), kw
    assert ops.cnf_supported(3, 0, (16, 48, 128))  # (the forward's envelope is wider)


def test_invalidate_drops_the_backward_image():
    import zuko_amd
    from zuko_amd.flows import CNF

    flow = CNF(3, 2)
    flow.transform.__dict__["_cnf_bwd_image_cache"] = ("key", object())
    zuko_amd.invalidate(flow)
    assert "_cnf_bwd_image_cache" not in flow.transform.__dict__
