"""Host: the continuous flow under Hutchinson's estimator.  tests/cnf_hutch_adjoint_ref.py against float64 autograd on tests/cnf_ref.py:
field(..., eps=) — the closed-form sweep, the six-stage reverse step and the whole backward — and against tests/cnf_adjoint_ref.py where no trace term
enters; the reference's fixture (tests/golden/make_golden_cnf_hutch.py) pins cnf_ref.integrate(..., eps=) and the package's torch-op path; the
switch's default and the v2 argument blocks as the header declares them."""

import ctypes

import numpy as np
import pytest
import torch

import cnf_adjoint_ref
import cnf_hutch_adjoint_ref as ref
import cnf_ref
from cnf_ref import NODES, STAGES, TRACE_SCALE
from conftest import T, golden, sd_hash
from parity import C_NOISE
from test_cnf_adjoint_host import SHAPES, _close, _net

FLOW_KW, FLOW_SEED = dict(features=3, context=2, exact=False), 17


def _probe(x, seed):
    return torch.randn(x.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _autograd_vjp(W, B, fr, t, x, c, a, beta, eps):
    """(f, d/dx, [d/dW], [d/db], d/dc) of sum(a . f) + sum(beta eps^T (df/dx) eps) on cnf_ref.field(..., eps=), by autograd."""
    leaves = [x.clone().requires_grad_(), *[w.clone().requires_grad_() for w in W], *[b.clone().requires_grad_() for b in B]] + ([] if c is None else [c.clone().requires_grad_()])
    n = len(W)
    xx, WW, BB, cc = leaves[0], leaves[1 : 1 + n], leaves[1 + n : 1 + 2 * n], (None if c is None else leaves[-1])
    f, est = cnf_ref.field(WW, BB, fr, t, xx, cc, eps=eps)
    phi = (a * f).sum() + (0 if beta is None else (beta * est).sum())
    g = torch.autograd.grad(phi, leaves, allow_unused=True)
    g = [torch.zeros_like(l) if v is None else v for v, l in zip(g, leaves)]
    return f.detach(), g[0], g[1 : 1 + n], g[1 + n : 1 + 2 * n], (None if c is None else g[-1])


@pytest.mark.parametrize("F,C,widths,Q", SHAPES)
def test_closed_form_sweep_with_a_probe_equals_autograd(F, C, widths, Q):
    W, B, fr, x, c, a, al = _net(F, C, widths, Q, seed=F + Q, scale=2.0)
    eps = _probe(x, 100 + F)
    t = torch.tensor(0.37, dtype=torch.float64)
    beta = al * TRACE_SCALE
    f0, gx0, gW0, gB0, gc0 = _autograd_vjp(W, B, fr, t, x, c, a, beta, eps)
    f, gx, gW, gB, gpre, gc = ref.sweep(W, B, fr, t, x, a, beta, eps, c)
    _close(f, f0, "f")
    _close(gx, gx0, "d/dx")
    for l in range(len(W)):
        _close(gW[l], gW0[l], f"d/dW{l}")
        _close(gB[l], gB0[l], f"d/db{l}")
    _close(gpre.sum(dim=0), gB0[0], "d/dpre summed over the rows = d/db0")
    if c is not None:
        _close(gc, gc0, "d/dc")
    # the estimate along the unit probes adds up to the exact trace's sweep (the estimator is linear in eps eps^T)
    parts = [ref.sweep(W, B, fr, t, x, torch.zeros_like(a), beta, torch.eye(F, dtype=torch.float64)[i].expand_as(x), c) for i in range(F)]
    exact = cnf_adjoint_ref.sweep(W, B, fr, t, x, torch.zeros_like(a), beta, c)
    _close(sum(p[1] for p in parts), exact[1], "sum over the unit probes: d/dx")
    for l in range(len(W)):
        _close(sum(p[2][l] for p in parts), exact[2][l], f"sum over the unit probes: d/dW{l}")


def _reference_reverse(W, B, fr, steps, ax, al, c, eps):
    """The reference's backward restated with autograd (as in tests/test_cnf_adjoint_host.py), the trace being cnf_ref.field's estimate along eps."""
    phi = [*W, *B] + ([] if c is None else [c])
    n = len(W)

    def adjoint(t, state):
        x, a = state[0], state[1]
        xx = x.clone().requires_grad_()
        pp = [p.clone().requires_grad_() for p in phi]
        f, tr = cnf_ref.field(pp[:n], pp[n : 2 * n], fr, t, xx, None if c is None else pp[-1], eps=eps)
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
def test_reverse_step_and_backward_with_a_probe_equal_the_references_algorithm(F, C, widths, Q):
    W, B, fr, x, c, a, al = _net(F, C, widths, Q, seed=11 * F + Q)
    eps = _probe(x, 200 + F)
    steps = [(x, 0.3, 0.3), (x + 0.05, 0.55, 0.25), (x * 0.9, 1.0, 0.45)]
    # (b) one step
    ax0, gW0, gB0, gc0 = _reference_reverse(W, B, fr, steps[1:2], a, al, c, eps)
    ax, gW, gB, gpre, gc = ref.reverse_step(W, B, fr, steps[1][1], steps[1][2], steps[1][0], a, al, eps, c)
    _close(ax, ax0, "step: ax_next")
    for k in range(len(W)):
        _close(gW[k], gW0[k], f"step: g W{k}")
        _close(gB[k], gB0[k], f"step: g b{k}")
    _close(gpre.sum(dim=0), gB0[0], "step: g pre")
    if c is not None:
        _close(gc, gc0, "step: g c")
        _close(gpre @ W[0][:, 2 * Q + F :], gc0, "step: g c from g pre")
        _close(gpre.T @ c, gW0[0][:, 2 * Q + F :], "step: the context's columns of g W0 from g pre")
    # (c) the whole backward
    ax0, gW0, gB0, gc0 = _reference_reverse(W, B, fr, steps, a, al, c, eps)
    ax, gW, gB, gpre, gc = ref.backward(W, B, fr, steps, a, al, eps, c)
    _close(ax, ax0, "backward: ax")
    for k in range(len(W)):
        _close(gW[k], gW0[k], f"backward: g W{k}")
        _close(gB[k], gB0[k], f"backward: g b{k}")
    if c is not None:
        _close(gc, gc0, "backward: g c")
    assert float((ax - cnf_adjoint_ref.backward(W, B, fr, steps, a, al, c)[0]).abs().max()) > 1e-6  # (the probe was used)
    # without al no trace term enters: the probe is not read and every result is cnf_adjoint_ref's, bit for bit
    for got, want in ((ref.reverse_step(W, B, fr, 0.55, 0.25, x, a, None, eps, c), cnf_adjoint_ref.reverse_step(W, B, fr, 0.55, 0.25, x, a, None, c)),
                      (ref.backward(W, B, fr, steps, a, None, None, c), cnf_adjoint_ref.backward(W, B, fr, steps, a, None, c))):
        flat = lambda r: [r[0], *r[1], *r[2], r[3]] + ([] if r[4] is None else [r[4]])
        assert all(torch.equal(u, v) for u, v in zip(flat(got), flat(want)))


def _fixture_flow(dtype=torch.float32):
    from zuko_amd.flows import CNF

    torch.manual_seed(FLOW_SEED)
    return CNF(**FLOW_KW).to(dtype)


def _spread(g, key):
    """The largest distance of the three float32 reference runs from the float64 truth."""
    truth = g[key + "_truth"]
    return max(float(np.abs(g[key + tag].astype(np.float64) - truth).max()) for tag in ("32", "32_098", "32_102"))


def test_the_fixture_pins_cnf_ref_with_a_probe_and_the_torch_op_path(monkeypatch):
    """Both in float32 at default tolerances with the fixture's probe: z, ladj and log_prob within C_NOISE x the fixture's own spread of the truth; in
    float64 at the truth's tolerances they are the truth."""
    from zuko_amd import ops

    g = golden("flow_cnf_hutch.npz")
    flow = _fixture_flow().eval()
    assert sd_hash(flow.state_dict()) == bytes(g["hash"]).decode() and g["x"].shape == (67, 3) and g["eps"].shape == (67, 3)
    lins = [m for m in flow.transform.ode if hasattr(m, "weight")]
    x, c, eps = T(g["x"]), T(g["c"]), T(g["eps"])
    base = lambda z: -0.5 * (z**2).sum(-1) - 0.5 * z.shape[-1] * np.log(2 * np.pi)

    def restated(dtype, **tol):
        cast = lambda v: v.detach().to(dtype)
        z, l, _ = cnf_ref.integrate([cast(m.weight) for m in lins], [cast(m.bias) for m in lins], cast(flow.transform.freqs), cast(x), cast(c), eps=cast(eps), **tol)
        return z, l / TRACE_SCALE

    def torch_ops(dtype, **tol):
        f = _fixture_flow(dtype).eval()
        f.transform.atol, f.transform.rtol = tol.get("atol", f.transform.atol), tol.get("rtol", f.transform.rtol)
        with torch.no_grad():
            out = f.transform(c.to(dtype)).call_and_ladj(x.to(dtype), eps=eps.to(dtype))
        assert ops.CNF_STATS["path"] == "torch"
        return out

    monkeypatch.setattr(ops, "_require_device", lambda *ts: None)  # (the torch-op path is device-agnostic; the product refuses CPU tensors by policy)
    for what, run in (("cnf_ref.integrate", restated), ("the torch-op path", torch_ops)):
        z, ladj = run(torch.float32)
        for key, got in (("z", z), ("ladj", ladj), ("lp", base(z) + ladj)):
            d, bar = float((got.double() - T(g[key + "_truth"])).abs().max()), C_NOISE * _spread(g, key)
            print(f"{what}: |{key} - truth| {d:.3e}, bar {bar:.3e}")
            assert d <= bar, f"{what}: |{key} - truth| = {d:.3e} > {bar:.3e}"
        # float64 at the truth's tolerances: two correct integrations differ by what the controller allows — 1e-10 + 1e-9 |state| per step, times
        # 1 / trace_scale = 100 on ladj, over the 200 and more steps such a run takes: up to 1e-8 a step, 1e-5 is above their sum and fifty times
        # below the float32 spread
        z, ladj = run(torch.float64, atol=1e-10, rtol=1e-9)
        assert torch.allclose(z, T(g["z_truth"]), rtol=1e-7, atol=1e-7) and torch.allclose(ladj, T(g["ladj_truth"]), rtol=1e-5, atol=1e-5), what


def test_the_switch_is_off_and_the_v2_blocks_extend_the_v1_blocks():
    import zuko_amd._C as C
    from zuko_amd import ops

    assert ops.CNF_HUTCHINSON is False and ops.CNF_ADJOINT is False
    text = open(C._HEADER).read()
    for sym in ("zk_cnf_step_v2", "zk_cnf_adjoint_step_v2"):
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym)
    for v1, v2 in (("zk_cnf_args_v1", "zk_cnf_args_v2"), ("zk_cnf_adj_args_v1", "zk_cnf_adj_args_v2")):
        a, b = C.STRUCTS[v1], C.STRUCTS[v2]
        n = len(a._fields_)
        assert [f for f, _ in b._fields_] == [f for f, _ in a._fields_] + ["eps", "ld_eps"]
        for (name, typ), (name2, typ2) in zip(a._fields_, b._fields_[:n]):
            assert typ is typ2 and getattr(a, name).offset == getattr(b, name2).offset and getattr(a, name).size == getattr(b, name2).size, name
        assert b.eps.offset == ctypes.sizeof(a) and b.ld_eps.offset == ctypes.sizeof(a) + 8 and ctypes.sizeof(b) == ctypes.sizeof(a) + 16
        assert C._VERSION[v1] == 1 and C._VERSION[v2] == 2


def test_v2_blocks_are_refused_without_a_device_like_v1_blocks():
    """Refusals come before any launch: a foreign size or version, the probe on a call without the trace, a probe stride below the features; a v2 block
    without a probe passes exactly the checks of the v1 block (N = 0 launches nothing)."""
    import zuko_amd._C as C

    lib, EINVAL = C.lib(), 1
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    image = lib.zk_cnf_image_floats(5, 3, 2, 64, 64, 0)
    ia, ga = ctypes.c_int(), ctypes.c_int()
    assert lib.zk_cnf_adjoint_floats(5, 3, 2, 64, 64, 0, ctypes.byref(ia), ctypes.byref(ga)) == 0

    def fwd(N, struct="zk_cnf_args_v2", **kw):
        base = dict(features=5, freqs=3, n_hidden=2, width0=64, width1=64, width2=0, image_floats=image, n_tangents=5, N=N, ldx=5, ldy=5, ld_pre=64, t=0.0, dt=0.25, atol=1e-6,
                    rtol=1e-5, trace_scale=1e-2)
        if N > 0:
            base.update(x=p, l=p, pre=p, image=p, y=p, l_next=p, err=p)
        base.update(kw)
        return C.args(struct, **base)

    def adj(N, struct="zk_cnf_adj_args_v2", **kw):
        base = dict(features=5, freqs=3, n_hidden=2, width0=64, width1=64, width2=0, image_floats=ia.value, grad_floats=ga.value, N=N, ldx=5, ld_ax=5, ld_ax_next=5, ld_pre=64,
                    ld_gpre=64, flat_total=1, t=1.0, dt=0.25, trace_scale=1e-2, ax=p, ax_next=p)
        if N > 0:
            base.update(x=p, al=p, pre=p, image=p, grad_table=p, gpre=p, gparams=p, work=p)
        base.update(kw)
        return C.args(struct, **base)

    for fn, fn1, block, v1 in ((lib.zk_cnf_step_v2, lib.zk_cnf_step, fwd, "zk_cnf_args_v1"), (lib.zk_cnf_adjoint_step_v2, lib.zk_cnf_adjoint_step, adj, "zk_cnf_adj_args_v1")):
        assert fn(block(0), None) == 0 and fn(block(0, eps=p, ld_eps=5), None) == 0 and fn(None, None) == EINVAL
        for N in (0, 4):
            for delta in (-16, -8, 8):
                bad = block(N)
                bad.struct_size += delta
                assert fn(bad, None) == EINVAL
            for version in (1, 3):
                bad = block(N)
                bad.version = version
                assert fn(bad, None) == EINVAL
            assert fn(block(N, features=17), None) == EINVAL and fn(block(N, ldx=4), None) == EINVAL  # (the v1 checks hold on a v2 block)
        assert fn(block(4, eps=p, ld_eps=4), None) == EINVAL
        assert fn1(block(0, struct=v1), None) == 0
        wrong = block(0, struct=v1)
        wrong.version = 2
        assert fn1(wrong, None) == EINVAL  # (the v1 entry points take v1 blocks only)
    assert lib.zk_cnf_step_v2(fwd(4, eps=p, ld_eps=5, n_tangents=0, l=None, l_next=None), None) == EINVAL  # (the probe needs the traced call)
    assert lib.zk_cnf_step_v2(fwd(4, eps=p, ld_eps=5, l=None), None) == EINVAL
