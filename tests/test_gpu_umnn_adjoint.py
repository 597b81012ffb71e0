"""GPU: the adjoint of the unconstrained monotone-network kernel (zk_umnn_backward) through the C ABI against the float32 / float64 CPU references
of tests/umnn_adjoint_ref.py, its independence and determinism properties, the argument block's variants, the autograd node of ops.umnn_forward and
the unconstrained neural autoregressive flow trained on it.  Bar: tests/parity.py: assert_parity with C_NOISE, for every gradient tensor."""

import copy
import ctypes

import numpy as np
import pytest
import torch

import umnn_adjoint_ref as ref
import umnn_ref
from conftest import T, golden, sd_hash
from mnn_nets import draw_inputs, draw_params
from parity import assert_parity

pytestmark = pytest.mark.gpu

UNAF_KW, UNAF_SEED = dict(features=5, context=3, transforms=2), 11
SEEDED = {"S1-16": (1, (16,)), "S7-16x48x64": (7, (16, 48, 64)), "S63-64x64x64": (63, (64, 64, 64)), "S16-64x64": (16, (64, 64))}


class BwdNet:
    """Per-feature integrand networks behind zk_umnn_backward: the backward image of the SIGNED weights and the gradient table built as the product
    builds them, and the quadrature table."""

    def __init__(self, W, B, dev, n_quad=32):
        import zuko_amd._C as C
        from zuko_amd import mnn_plan

        self.dev, self.n_quad = dev, n_quad
        self.Wc, self.Bc = [w.float().cpu() for w in W], [b.float().cpu() for b in B]
        self.W, self.B = [w.to(dev) for w in self.Wc], [b.to(dev) for b in self.Bc]
        self.S, self.widths, self.F = self.W[0].shape[2] - 1, tuple(w.shape[1] for w in self.W[:-1]), self.W[0].shape[0]
        self.L, self.Bl = mnn_plan.layout(self.S, self.widths), mnn_plan.layout_backward(self.S, self.widths)
        idx = torch.from_numpy(mnn_plan.index_table_backward(self.S, self.widths, self.F).reshape(-1)).to(dev)
        self.table = torch.from_numpy(mnn_plan.grad_table(self.S, self.widths, self.F).reshape(-1)).to(dev)
        self.flat = torch.cat([w.reshape(-1) for w in self.W] + [b.reshape(-1) for b in self.B])
        self.flat_weights = sum(w.numel() for w in self.W)
        self.image = torch.empty(idx.numel(), dtype=torch.float32, device=dev)
        C.check(C.lib().zk_gather_f32(self.flat.data_ptr(), None, idx.data_ptr(), idx.numel(), self.image.data_ptr(), C.stream()), "zk_gather_f32")
        t, w = np.polynomial.legendre.leggauss(n_quad)
        self.quad = torch.from_numpy(np.concatenate([(t + 1) / 2, w / 2]).astype(np.float32)).to(dev)
        torch.cuda.synchronize()

    def with_quad(self, n_quad):
        return BwdNet(self.Wc, self.Bc, self.dev, n_quad)

    def workspace(self, N, D):
        import zuko_amd._C as C

        v = ctypes.c_int64(-1)
        w = list(self.widths) + [0, 0]
        C.check(C.lib().zk_umnn_backward_workspace_floats(N, D, self.S, len(self.widths), w[0], w[1], w[2], ctypes.byref(v)), "workspace")
        return v.value

    def backward(self, x, sig, gy, gl, feat=None, want=(True, True, True), gx=None, gs=None):
        """x [N, D] (unit inner stride), sig [N, D, S] (unit inner stride, any column and row stride); gy [N, D] | None; gl [N, D] | [N] | None; gx / gs:
        output views to write into (any row stride) instead of fresh ones.  Returns (gx, gsignal [N, D * S], gparams flat), None where not wanted."""
        import zuko_amd._C as C

        N, D = x.shape
        assert x.stride(1) == 1 and sig.stride(2) == 1 and sig.shape == (N, D, self.S)
        if want[0] and gx is None:
            gx = torch.full((N, D), float("nan"), device=self.dev)
        if want[1] and gs is None:
            gs = torch.full((N, D * self.S), float("nan"), device=self.dev)
        gp = torch.full((self.flat.numel(),), float("nan"), device=self.dev) if want[2] else None
        work = torch.full((max(1, self.workspace(N, D)),), float("nan"), device=self.dev) if want[2] else None
        ft = None if feat is None else torch.as_tensor(list(feat), dtype=torch.int32, device=self.dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        w = list(self.widths) + [0, 0]
        ld_col = sig.stride(1) if D > 1 else self.S
        a = C.args("zk_umnn_bwd_args_v1", S=self.S, n_hidden=len(self.widths), width0=w[0], width1=w[1], width2=w[2], n_features=self.F, image_floats=self.Bl.total,
                   grad_floats=self.Bl.g_total, gl_reduced=int(gl is not None and gl.dim() == 1), n_quad=self.n_quad, N=N, Dsel=D, ldx=x.stride(0) if N > 1 else D,
                   ld_signal=sig.stride(0) if N > 1 else (D - 1) * ld_col + self.S, ld_col=ld_col, ld_gx=D if gx is None else gx.stride(0),
                   ld_gsignal=D * self.S if gs is None else gs.stride(0), flat_total=self.flat.numel(), flat_weights=self.flat_weights, x=x.data_ptr(),
                   signal=sig.data_ptr(), image=self.image.data_ptr(), quad=self.quad.data_ptr(), feat=ptr(ft), gy=ptr(gy), gl=ptr(gl),
                   grad_table=self.table.data_ptr() if want[2] else None, gx=ptr(gx) if want[0] else None, gsignal=ptr(gs) if want[1] else None, gparams=ptr(gp),
                   work=ptr(work))
        C.check(C.lib().zk_umnn_backward(a, C.stream()), "zk_umnn_backward")
        torch.cuda.synchronize()
        return (gx if want[0] else None), (gs if want[1] else None), gp

    def refs(self, x, sig, gy, gl, feat=None):
        """(float32, float64) CPU autograd references on CPU copies of device inputs; both all finite."""
        c = lambda t: None if t is None else t.detach().cpu()
        args = (self.Wc, self.Bc, c(x), c(sig), c(gy), c(gl))
        r32 = ref.autograd(*args, feat=feat, n=self.n_quad, dtype=torch.float32)
        r64 = ref.autograd(*args, feat=feat, n=self.n_quad, dtype=torch.float64)
        assert ref.all_finite(r32) and ref.all_finite(r64), "the reference gradients must be finite"
        return r32, r64


def check(net, got, r32, r64, what):
    gx, gs, gp = got
    if gx is not None:
        assert_parity(gx, r32["gx"], r64["gx"], f"{what}: gx")
    if gs is not None:
        assert_parity(gs.reshape(r32["gsignal"].shape), r32["gsignal"], r64["gsignal"], f"{what}: gsignal")
    if gp is not None:
        o = 0
        for kind in ("gW", "gB"):
            for l, (a, b) in enumerate(zip(r32[kind], r64[kind])):
                assert_parity(gp[o : o + a.numel()].reshape(a.shape), a, b, f"{what}: {kind}{l}")
                o += a.numel()
        assert o == gp.numel()


def upstream(N, D, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(N, D, generator=gen).to(dev), torch.randn(N, D, generator=gen).to(dev)


def seeded(shape, dev, F=3, N=67, seed=21, n_quad=32):
    """A seeded network and inputs [N, F] / [N, F, S]; rows with x = 0, 10 and -10 are written in."""
    S, widths = shape
    net = BwdNet(*draw_params(S, widths, F, seed=seed), dev, n_quad)
    x, sig, _ = draw_inputs(N, F, S, seed=seed + 1)
    if N >= 8:
        x[2], x[4], x[6] = 0.0, 10.0, -10.0
    return net, x.to(dev), sig.to(dev)


@pytest.mark.parametrize("name", ["umnn_a", "umnn_b", "umnn_e"])
def test_fixture_gradients_through_the_c_abi(dev, name):
    g = golden(name + ".npz")
    net = BwdNet(*umnn_ref.params_of(g), dev)
    x, sig = T(g["x"], dev), T(g["signal"], dev)
    gy, gl = upstream(*x.shape, dev, seed=31)
    check(net, net.backward(x, sig, gy, gl), *net.refs(x, sig, gy, gl), name)


@pytest.mark.parametrize("name", list(SEEDED))
def test_seeded_networks_through_the_c_abi(dev, name):
    net, x, sig = seeded(SEEDED[name], dev)
    gy, gl = upstream(*x.shape, dev, seed=32)
    check(net, net.backward(x, sig, gy, gl), *net.refs(x, sig, gy, gl), name)


@pytest.mark.parametrize("n_quad", [1, 2, 7, 33, 64])
def test_quadrature_sizes(dev, n_quad):
    net, x, sig = seeded(SEEDED["S7-16x48x64"], dev, n_quad=n_quad, seed=35)
    gy, gl = upstream(*x.shape, dev, seed=36)
    check(net, net.backward(x, sig, gy, gl), *net.refs(x, sig, gy, gl), f"n_quad {n_quad}")


@pytest.fixture(scope="module")
def edge(dev):
    """One row more than a whole number of row chunks (the geometry query names it), and the gradients of that run."""
    import zuko_amd._C as C

    N, D = 193, 3
    rows, chunks = ctypes.c_int(), ctypes.c_int()
    C.check(C.lib().zk_umnn_backward_geometry(N, D, ctypes.byref(rows), ctypes.byref(chunks)), "geometry")
    assert (N - 1) % rows.value == 0 and chunks.value == (N - 1) // rows.value + 1 and chunks.value > 1
    net, x, sig = seeded((7, (16, 48, 64)), dev, F=D, N=N, seed=41, n_quad=7)
    gy, gl = upstream(N, D, dev, seed=42)
    return net, x, sig, gy, gl, net.backward(x, sig, gy, gl)


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 193])
def test_row_edges_independence_and_determinism(dev, edge, N):
    net, x, sig, gy, gl, (gx_all, gs_all, _) = edge
    cut = lambda t: t[:N].contiguous()
    got = net.backward(cut(x), cut(sig), cut(gy), cut(gl))
    assert torch.equal(got[0], gx_all[:N]) and torch.equal(got[1], gs_all[:N]), "an element's gx / gsignal depend on that element only"
    check(net, got, *net.refs(cut(x), cut(sig), cut(gy), cut(gl)), f"rows {N}")
    for _ in range(2):
        again = net.backward(cut(x), cut(sig), cut(gy), cut(gl))
        assert all(torch.equal(a, b) for a, b in zip(again, got)), "the same inputs give the same bits"


@pytest.mark.parametrize("shape", [(3, (32,)), (7, (16, 48, 64))], ids=["S3", "S7"])
def test_strides_and_the_signal_read_in_place_from_the_packed_block(dev, shape):
    net, x, sig = seeded(shape, dev, F=4, N=130, seed=51, n_quad=7)
    N, D = x.shape
    S = net.S
    gy, gl = upstream(N, D, dev, seed=52)
    plain = net.backward(x, sig, gy, gl)
    nan = float("nan")
    # padded rows of x, gx and gsignal; the signal inside the conditioner's packed phi [N, D, S + 1] with the constant in the last column
    xp = torch.full((N, D + 3), nan, device=dev)
    xp[:, :D] = x
    phi = torch.randn(N, D, S + 1, device=dev)
    phi[:, :, :S] = sig
    gxp, gsp = torch.full((N, D + 2), nan, device=dev), torch.full((N, D * S + 7), nan, device=dev)
    packed = phi[:, :, :S]
    assert packed.stride(1) == S + 1
    got = net.backward(xp[:, :D], packed, gy, gl, gx=gxp[:, :D], gs=gsp[:, : D * S])
    assert torch.equal(gxp[:, :D], plain[0]) and torch.equal(gsp[:, : D * S], plain[1]) and torch.equal(got[2], plain[2])
    assert bool(torch.isnan(gxp[:, D:]).all()) and bool(torch.isnan(gsp[:, D * S :]).all()), "the padding is untouched"
    # padded signal rows as well
    sp = torch.full((N, D * S + 5), nan, device=dev)
    sp[:, : D * S] = sig.reshape(N, -1)
    got = net.backward(x, sp[:, : D * S].unflatten(1, (D, S)), gy, gl)
    assert all(torch.equal(a, b) for a, b in zip(got, plain))
    assert bool(torch.isfinite(plain[1]).all()) and bool(torch.isfinite(plain[2]).all())
    check(net, plain, *net.refs(x, sig, gy, gl), f"S{shape[0]} strides")


def test_interface_variants(dev):
    net, x, sig = seeded((16, (64, 64)), dev, F=5, N=97, seed=61, n_quad=7)
    N, D = x.shape
    S = net.S
    gy, gl = upstream(N, D, dev, seed=62)
    full = net.backward(x, sig, gy, gl)
    # a permuted subset of the features
    cols = [3, 0, 4]
    xs, ss = x[:, cols].contiguous(), sig[:, cols].contiguous()
    gys, gls = gy[:, cols].contiguous(), gl[:, cols].contiguous()
    sub = net.backward(xs, ss, gys, gls, feat=cols)
    assert torch.equal(sub[0], full[0][:, cols]) and torch.equal(sub[1].reshape(N, 3, S), full[1].reshape(N, D, S)[:, cols])
    r32, r64 = net.refs(xs, ss, gys, gls, feat=cols)
    check(net, sub, r32, r64, "feat subset")
    o = 0
    for kind, tensors in (("gW", net.W), ("gB", net.B)):
        for l, t in enumerate(tensors):
            per = t.numel() // net.F
            gsub, gfull = sub[2][o : o + t.numel()].reshape(net.F, per), full[2][o : o + t.numel()].reshape(net.F, per)
            assert not bool(gsub[[1, 2]].any()), "unselected features receive exact zeros"
            assert_parity(gsub[cols], gfull[cols], r64[kind][l].reshape(net.F, per)[cols], f"feat subset vs the full run: {kind}{l}")
            o += t.numel()
    # ladj's gradient given per row
    glr = gl[:, 0].contiguous()
    red = net.backward(x, sig, gy, glr)
    same = net.backward(x, sig, gy, glr[:, None].expand(N, D).contiguous())
    assert all(torch.equal(a, b) for a, b in zip(red, same))
    check(net, red, *net.refs(x, sig, gy, glr), "gl reduced")
    # either upstream gradient absent
    check(net, net.backward(x, sig, None, gl), *net.refs(x, sig, None, gl), "gy NULL")
    check(net, net.backward(x, sig, gy, None), *net.refs(x, sig, gy, None), "gl NULL")
    # every output can be left out; the others keep their bits
    for want in [(False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, False, False)]:
        part = net.backward(x, sig, gy, gl, want=want)
        for k in range(3):
            assert (part[k] is None) == (not want[k])
            assert part[k] is None or torch.equal(part[k], full[k]), want


def test_zero_rows_zero_the_parameter_gradients(dev):
    net, x, sig = seeded((3, (32,)), dev, F=2, N=4, seed=71)
    _, _, gp = net.backward(x[:0], sig[:0], None, None, want=(False, False, True))
    assert gp.numel() == net.flat.numel() and not bool(gp.any())


def _module_for(W, B, dev):
    from zuko_amd.flows import UMNN

    m = UMNN(signal=W[0].shape[2] - 1, stack=W[0].shape[0], hidden_features=tuple(w.shape[1] for w in W[:-1]))
    with torch.no_grad():
        for lin, w, b in zip([l for l in m.integrand if hasattr(l, "weight")], W, B):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    return m.to(dev)


def _module_grads(m, x, leaves, split, gy, gl, reduce=False, n=32):
    """Gradients of sum(gy y) + sum(gl ladj) through the module: `leaves` are made to require gradients, `split(*leaves)` -> (signal, constant)."""
    m.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    leaves = [t.clone().requires_grad_() for t in leaves]
    sig3, cst = split(*leaves)
    t = m(sig3, cst)
    t.n = n
    y, ladj = t.call_and_ladj_reduced(x) if reduce else t.call_and_ladj(x)
    ((gy * y).sum() + (gl * ladj).sum()).backward()
    lins = [l for l in m.integrand if hasattr(l, "weight")]
    return y, ladj, x.grad, [t.grad for t in leaves], torch.cat([l.weight.grad.reshape(-1) for l in lins] + [l.bias.grad.reshape(-1) for l in lins])


def test_autograd_node_equals_the_c_abi_and_the_switch_restores_the_torch_path(dev, monkeypatch):
    from zuko_amd import ops

    net, x, sig = seeded((16, (64, 64)), dev, F=4, N=97, seed=81)
    N, D = x.shape
    S = net.S
    gy, gl = upstream(N, D, dev, seed=82)
    m = _module_for(net.W, net.B, dev)
    direct = net.backward(x, sig, gy, gl)
    # signal and constant cut from one packed phi [N, D, S + 1]
    phi = torch.cat((sig, torch.randn(N, D, 1, device=dev)), dim=-1)
    cut = lambda p: (p[..., :S], p[..., S])
    y, ladj, gx, (gphi,), gp = _module_grads(m, x, [phi], cut, gy, gl)
    assert "UmnnForwardFn" in type(y.grad_fn).__name__ and "UmnnForwardFn" in type(ladj.grad_fn).__name__
    assert torch.equal(gx, direct[0]) and torch.equal(gphi[..., :S].reshape(N, -1), direct[1]) and torch.equal(gphi[..., S], gy) and torch.equal(gp, direct[2])
    with torch.no_grad():
        y0, ladj0 = m(*cut(phi)).call_and_ladj(x)
    assert torch.equal(y.detach(), y0) and torch.equal(ladj.detach(), ladj0)
    # a constant broadcast over the rows: autograd sums its gradient
    cst = torch.randn(D, device=dev)
    y_b, ladj_b, gx_b, (gs_b, gc_b), gp_b = _module_grads(m, x, [sig, cst], lambda s, c: (s, c), gy, gl)
    assert "UmnnForwardFn" in type(y_b.grad_fn).__name__ and tuple(gc_b.shape) == (D,)
    assert torch.equal(gx_b, direct[0]) and torch.equal(gs_b.reshape(N, -1), direct[1]) and torch.equal(gp_b, direct[2]) and torch.equal(gc_b, gy.sum(0))
    # reduced: ladj [N], its gradient given per row
    glr = gl[:, 0].contiguous()
    y_r, ladj_r, gx_r, (gphi_r,), gp_r = _module_grads(m, x, [phi], cut, gy, glr, reduce=True)
    assert "UmnnForwardFn" in type(ladj_r.grad_fn).__name__ and tuple(ladj_r.shape) == (N,)
    direct_r = net.backward(x, sig, gy, glr)
    assert torch.equal(gx_r, direct_r[0]) and torch.equal(gphi_r[..., :S].reshape(N, -1), direct_r[1]) and torch.equal(gp_r, direct_r[2])
    # double backward through the node raises
    xg = x.clone().requires_grad_()
    yy, _ = m(*cut(phi)).call_and_ladj(xg)
    (g1,) = torch.autograd.grad(yy.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()
    # the switch: the torch-op path, at the same bar
    r32, r64 = net.refs(x, sig, gy, gl)
    monkeypatch.setattr(ops, "UMNN_ADJOINT", False)
    y_t, ladj_t, gx_t, (gphi_t,), gp_t = _module_grads(m, x, [phi], cut, gy, gl)
    assert "UmnnForwardFn" not in type(y_t.grad_fn).__name__
    check(net, (gx_t, gphi_t[..., :S].reshape(N, -1), gp_t), r32, r64, "UMNN_ADJOINT = False")
    monkeypatch.setattr(ops, "UMNN_ADJOINT", True)
    check(net, (gx, gphi[..., :S].reshape(N, -1), gp), r32, r64, "autograd node")


def test_bfloat16_trains_on_float32_copies(dev):
    """bfloat16 operands under autograd run the float32 kernels on widened copies: y is rounded once to bfloat16, ladj stays float32, and every
    gradient is the float32 one rounded to the leaf's bfloat16."""
    net, x, sig = seeded((16, (64, 64)), dev, F=3, N=40, seed=85)
    N, D = x.shape
    bf = torch.bfloat16
    mb = _module_for([w.to(bf) for w in net.W], [b.to(bf) for b in net.B], dev).to(bf)
    mf = _module_for([w.to(bf).float() for w in net.W], [b.to(bf).float() for b in net.B], dev)
    xb, sb, cb = x.to(bf), sig.to(bf), torch.randn(N, D, device=dev).to(bf)
    gy, gl = upstream(N, D, dev, seed=86)
    gy = gy.to(bf).float()  # (the gradient that reaches a bfloat16 y is rounded to it)
    same = lambda s, c: (s, c)
    yf, lf, gxf, (gsf, gcf), gpf = _module_grads(mf, xb.float(), [sb.float(), cb.float()], same, gy, gl)
    yb, lb, gxb, (gsb, gcb), gpb = _module_grads(mb, xb, [sb, cb], same, gy, gl)
    assert "UmnnForwardFn" in type(lb.grad_fn).__name__
    assert yb.dtype == bf and lb.dtype == torch.float32 and gxb.dtype == bf and gsb.dtype == bf and gcb.dtype == bf and gpb.dtype == bf
    assert torch.equal(yb, yf.to(bf)) and torch.equal(lb, lf)
    assert torch.equal(gxb, gxf.to(bf)) and torch.equal(gsb, gsf.to(bf)) and torch.equal(gcb, gcf.to(bf)) and torch.equal(gpb, gpf.to(bf))


@pytest.mark.parametrize("case", ["30x30", "umnn_c", "n_quad 65"])
def test_outside_the_envelope_takes_the_torch_path(dev, case):
    from zuko_amd import ops

    S, widths, n = {"30x30": (16, (30, 30), 32), "umnn_c": (7, (16, 48, 128), 32), "n_quad 65": (16, (64, 64), 65)}[case]
    assert not ops.umnn_backward_supported(S, widths, n)
    F, N = 3, 33
    W, B = draw_params(S, widths, F, seed=91)
    x, sig, _ = draw_inputs(N, F, S, seed=92)
    m = _module_for(W, B, dev)
    gy, gl = upstream(N, F, dev, seed=93)
    y, ladj, gx, (gs,), gp = _module_grads(m, x.to(dev), [sig.to(dev)], lambda s: (s, None), gy, gl, n=n)
    assert "UmnnForwardFn" not in type(y.grad_fn).__name__
    r32 = ref.autograd(W, B, x, sig, gy.cpu(), gl.cpu(), n=n, dtype=torch.float32)
    r64 = ref.autograd(W, B, x, sig, gy.cpu(), gl.cpu(), n=n, dtype=torch.float64)
    assert ref.all_finite(r32) and ref.all_finite(r64)
    assert_parity(gx, r32["gx"], r64["gx"], f"{case}: torch path gx")
    assert_parity(gs, r32["gsignal"], r64["gsignal"], f"{case}: torch path gsignal")
    assert_parity(gp, ref.flat(r32), ref.flat(r64), f"{case}: torch path parameters")


@pytest.fixture(scope="module")
def unaf(dev):
    import zuko_amd.flows as F

    g = golden("flow_unaf_small.npz")
    torch.manual_seed(UNAF_SEED)
    flow = F.UNAF(**UNAF_KW)
    assert sd_hash(flow.state_dict()) == bytes(g["hash"]).decode()
    return g, flow.to(dev)


def test_flow_gradients_kernel_path_against_the_torch_path(dev, unaf, monkeypatch):
    import zuko_amd._C as C
    from zuko_amd import ops

    g, flow = unaf
    x, c = T(g["x"], dev), T(g["c"], dev)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(ops, "UMNN_ADJOINT", on)
        monkeypatch.setattr(C, "PROFILE", {})
        f = copy.deepcopy(flow).train()
        f(c).log_prob(x).mean().backward()
        grads[on] = {k: p.grad for k, p in f.named_parameters()}
        calls = len(C.PROFILE.get("zk_umnn_backward", []))
        assert calls >= 2 if on else calls == 0, f"UMNN_ADJOINT = {on}: {calls} zk_umnn_backward calls"
    monkeypatch.setattr(C, "PROFILE", None)
    for k in grads[True]:
        r64 = T(g["grad/" + k]).double()
        assert bool(torch.isfinite(r64).all())
        assert_parity(grads[True][k], grads[False][k], r64, f"unaf_small: grad {k}")


def test_flow_trains_on_the_kernel_path(dev, unaf):
    g, flow = unaf
    flow = copy.deepcopy(flow).train()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(256, 5, generator=gen)
    x = torch.stack([x[:, 0], x[:, 0] * x[:, 1], x[:, 2] + 0.5 * x[:, 0], x[:, 3] ** 2, x[:, 4]], dim=1).to(dev)
    c = torch.randn(256, 3, generator=gen).to(dev)
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    losses = []
    for _ in range(30):
        loss = -flow(c).log_prob(x).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_capture_step_replays_a_unaf_training_step(dev):
    import zuko_amd
    import zuko_amd.flows as F

    torch.manual_seed(3)
    flow = F.UNAF(3, 2, transforms=2).to(dev)
    twin = copy.deepcopy(flow)
    gen = torch.Generator(device=dev).manual_seed(4)
    batches = [(torch.randn(64, 3, device=dev, generator=gen), torch.randn(64, 2, device=dev, generator=gen)) for _ in range(3)]
    opt_a = torch.optim.Adam(flow.parameters(), lr=1e-3, capturable=True)
    opt_b = torch.optim.Adam(twin.parameters(), lr=1e-3, capturable=True)
    WARM = 2
    step = zuko_amd.capture_step(flow, opt_a, *batches[0], warmup=WARM)
    losses_a = [step(*b).item() for b in batches]
    losses_b = []
    for i, (x, c) in enumerate([batches[0]] * WARM + batches):
        loss = -twin(c).log_prob(x).mean()
        opt_b.zero_grad(set_to_none=False)
        loss.backward()
        opt_b.step()
        if i >= WARM:
            losses_b.append(loss.item())
    assert_parity(torch.tensor(losses_a), torch.tensor(losses_b), torch.tensor(losses_b).double(), "unaf capture_step: losses")
    for (k, p), q in zip(flow.named_parameters(), twin.parameters()):
        assert_parity(p, q, q.double(), f"unaf capture_step: {k}")
