"""CPU: the continuous normalizing flow's host side — the torch restatement the GPU tests use as reference (tests/cnf_ref.py) pinned to the
reference's fixtures (tests/golden/make_golden_cnf.py), module tree / state_dict / seeds, the envelope predicate, the weight image walked in the
kernel's order by a numpy emulator, the torch-op integrator against the restatement, and the argument-block checks of zk_cnf_step.  No kernel is
launched."""

import ctypes

import numpy as np
import pytest
import torch

import cnf_ref
from conftest import T, golden, sd_hash
from parity import assert_parity

CASES = {"cnf_a": (3, 2, (64, 64), 3, 41), "cnf_b": (5, 0, (64, 64), 3, 42), "cnf_c": (16, 3, (16, 48, 128), 2, 43), "cnf_d": (1, 0, (16,), 3, 44),
         "cnf_e": (4, 2, (30, 30), 3, 45)}
FLOW_KW, FLOW_SEED = dict(features=3, context=2), 17


def _operands(g, dtype):
    W, B, fr = cnf_ref.params_of(g, dtype)
    c = T(g["c"]).to(dtype) if "c" in g else None
    return W, B, fr, c


@pytest.mark.parametrize("name", list(CASES))
def test_cnf_ref_reproduces_the_pinned_steps_and_sequences(name):
    """One step at the three pinned attempts (result, log-determinant state, per-row ratio) and the state after the accepted sequence, forward with
    the trace and backward without: 1e-12 in float64, the suite's parity bar in float32."""
    g = golden(name + ".npz")
    for mode, with_l in (("fwd", True), ("inv", False)):
        att = g[f"{mode}_att32"]
        res = {}
        for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
            W, B, fr, c = _operands(g, dtype)
            for k, i in enumerate(g[f"{mode}_pin"]):
                x = T(g[f"{mode}_pin{k}_x"]).to(dtype)
                l = T(g[f"{mode}_pin{k}_l"]).to(dtype) if with_l else None
                y, ln, r = cnf_ref.step(W, B, fr, att[i, 0], att[i, 1], x, l, c)
                res[f"pin{k}_y{tag}"], res[f"pin{k}_r{tag}"] = y, r
                if with_l:
                    res[f"pin{k}_l{tag}"] = ln
            x = T(g["x" if mode == "fwd" else "zin"]).to(dtype)
            l = torch.zeros_like(x[:, 0]) if with_l else None
            for t, dt, ok in att:
                if ok:
                    x, l, _ = cnf_ref.step(W, B, fr, t, dt, x, l, c)
            res[f"y{tag}"] = x
            if with_l:
                res[f"l{tag}"] = l
        for key in [k[:-2] for k in res if k.endswith("64")]:
            got64, got32 = res[key + "64"], res[key + "32"]
            ref64, ref32 = T(g[f"{mode}_{key}64"]), T(g[f"{mode}_{key}32"])
            d = float((got64 - ref64).abs().max())
            print(f"{name} {mode} {key}: f64 max |d| {d:.3e}, f32 max |d| {float((got32 - ref32).abs().max()):.3e}")
            assert got64.dtype == torch.float64 and torch.allclose(got64, ref64, rtol=1e-12, atol=1e-12), f"{name} {mode} {key}64: {d:.3e}"
            assert_parity(got32, ref32, ref64, f"cnf_ref {name} {mode} {key}")
        assert g[f"{mode}_pin0_r32"].max() > 1 and g[f"{mode}_pin2_r32"].max() < 1  # (a rejected and an accepted attempt are among the pinned ones)


@pytest.mark.parametrize("name", list(CASES))
def test_cnf_ref_controller_reproduces_the_attempted_steps(name):
    g = golden(name + ".npz")
    W, B, fr, c = _operands(g, torch.float64)
    for mode, start, t0, t1, with_l in (("fwd", "x", 0.0, 1.0, True), ("inv", "zin", 1.0, 0.0, False)):
        y, l, att = cnf_ref.integrate(W, B, fr, T(g[start]).double(), c, t0, t1, with_l)
        ref = g[f"{mode}_att64"]
        assert att.shape == ref.shape, f"{name} {mode}: {len(att)} attempts, the reference made {len(ref)}"
        assert np.array_equal(att[:, 2].numpy(), ref[:, 2]) and np.allclose(att[:, :2].numpy(), ref[:, :2], rtol=1e-9, atol=1e-12)
        assert float(att[-1, 0] + att[-1, 1]) == t1
        if mode == "fwd":
            assert torch.allclose(y, T(g["z64"]), rtol=1e-10, atol=1e-10)
            base = -0.5 * (y**2).sum(-1) - 0.5 * y.shape[-1] * np.log(2 * np.pi)
            assert torch.allclose(base + l / cnf_ref.TRACE_SCALE, T(g["lp64"]), rtol=1e-9, atol=1e-9)


def test_odeint_in_torch_ops_equals_the_restatement_and_differentiates():
    """zuko_amd.utils.odeint / dopri45 on the CPU in float64 around cnf_ref's closed-form field: the same steps as cnf_ref.integrate, and the adjoint's
    gradient with respect to the initial state against the one autograd takes through an unrolled integration over the same accepted steps."""
    from zuko_amd.utils import dopri45, odeint

    g = golden("cnf_a.npz")
    W, B, fr, c = _operands(g, torch.float64)
    x = T(g["x"]).double()[:9]
    c = c[:9]

    def f(t, x, l):
        dx, tr = cnf_ref.field(W, B, fr, t, x, c)
        return dx, tr * cnf_ref.TRACE_SCALE

    with torch.no_grad():
        y, l = odeint(f, (x, torch.zeros_like(x[:, 0])), 0.0, 1.0)
        y_ref, l_ref, att = cnf_ref.integrate(W, B, fr, x, c)
        assert torch.allclose(y, y_ref, rtol=1e-12, atol=1e-12) and torch.allclose(l, l_ref, rtol=1e-12, atol=1e-14)
        one, err = dopri45(lambda t, v: cnf_ref.field(W, B, fr, t, v, c)[0], x, torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.25, dtype=torch.float64), error=True)
        y1, _, r1 = cnf_ref.step(W, B, fr, 0.0, 0.25, x, None, c)
        assert torch.allclose(one, y1, rtol=1e-13, atol=1e-13)
        assert torch.allclose((err / (1e-6 + 1e-5 * torch.max(abs(x), abs(one)))).max(-1).values, r1, rtol=1e-9, atol=1e-12)
    h = lambda t, v: cnf_ref.field(W, B, fr, t, v, c)[0]
    xg = x.clone().requires_grad_()
    odeint(h, xg, 0.0, 1.0).square().sum().backward()
    xu = x.clone().requires_grad_()
    v = xu
    _, _, att = cnf_ref.integrate(W, B, fr, x, c, with_l=False)
    for t, dt, ok in att:
        if ok:
            v = dopri45(h, v, t, dt)
    v.square().sum().backward()
    # (the adjoint integrates the continuous adjoint equation one Dormand-Prince step per accepted step: it meets the unrolled steps' gradient to
    #  the integration's tolerance, not to rounding)
    assert float((xg.grad - xu.grad).abs().max()) <= 2e-4 * float(xu.grad.abs().max())
    with pytest.raises(RuntimeError, match="non-finite error estimate"):
        odeint(lambda t, v: v * float("nan"), x, 0.0, 1.0)


def test_cnf_module_tree_state_dict_and_seed_match_the_reference():
    import torch.nn as nn

    import zuko_amd.flows as F
    import zuko_amd.transforms as ZT
    from torch.distributions import constraints
    from zuko_amd.flows import CNF, FFJTransform
    from zuko_amd.nn import MLP, Linear

    g = golden("flow_cnf_small.npz")
    torch.manual_seed(FLOW_SEED)
    flow = CNF(**FLOW_KW)
    sd = flow.state_dict()
    assert sd_hash(sd) == bytes(g["hash"]).decode()
    assert [k for k, _ in flow.named_parameters()] == list(g["param_names"])
    assert list(sd) == ["transform.times", "transform.freqs", "transform.ode.0.weight", "transform.ode.0.bias", "transform.ode.2.weight", "transform.ode.2.bias",
                        "transform.ode.4.weight", "transform.ode.4.bias", "base.loc", "base.scale"]
    assert "CNF" in F.__all__ and "FFJTransform" in F.__all__ and "FreeFormJacobianTransform" in ZT.__all__
    t = flow.transform
    assert type(t) is FFJTransform and type(t.ode) is MLP and [type(m) for m in t.ode] == [Linear, nn.ELU, Linear, nn.ELU, Linear]
    assert tuple(sd["transform.ode.0.weight"].shape) == (64, 3 + 2 + 6) and (t.atol, t.rtol, t.exact) == (1e-6, 1e-5, True)
    assert torch.equal(t.times, torch.tensor([0.0, 1.0])) and torch.allclose(t.freqs, torch.arange(1, 4) * np.pi)
    r = repr(flow)
    assert "FFJTransform(" in r and "(ode): MLP(" in r and "Linear(in_features=11, out_features=64, bias=True)" in r and "ELU(alpha=1.0)" in r
    for name, (Fe, C, hidden, Q, seed) in CASES.items():
        torch.manual_seed(seed)
        assert sd_hash(CNF(Fe, C, hidden_features=hidden, freqs=Q).state_dict()) == bytes(golden(name + ".npz")["hash"]).decode(), name
    torch.manual_seed(FLOW_SEED + 100)
    other = CNF(**FLOW_KW)
    assert sd_hash(other.state_dict()) != sd_hash(sd)
    other.load_state_dict(sd)
    assert sd_hash(other.state_dict()) == sd_hash(sd)
    # the transformation a context makes: phi follows the mode, the inverse swaps the times
    c = torch.randn(4, 2)
    tr = flow.eval().transform(c)
    assert type(tr) is ZT.FreeFormJacobianTransform and tr.phi == () and tr.trace_scale == 1e-2 and tr.exact
    assert tr.domain is constraints.real_vector and tr.codomain is constraints.real_vector and tr.bijective
    assert float(tr.t0) == 0.0 and float(tr.t1) == 1.0 and float(tr.inv.t0) == 1.0 and float(tr.inv.t1) == 0.0 and tr.inv.kernel is tr.kernel
    tr = flow.train().transform(c.requires_grad_())
    assert len(tr.phi) == 7 and tr.phi[0] is c
    assert len(flow.transform().phi) == 6 and len(flow.eval().transform().phi) == 0
    assert CNF(3, 0, exact=False, atol=1e-4, freqs=5, hidden_features=(32,), activation=nn.Tanh).transform.freqs.numel() == 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        flow.eval()(c.detach()).log_prob(torch.randn(4, 3))
    # the field in torch ops is cnf_ref's
    ga = golden("cnf_a.npz")
    torch.manual_seed(CASES["cnf_a"][4])
    fa = CNF(3, 2, hidden_features=(64, 64)).double()
    W, B, fr, ca = _operands(ga, torch.float64)
    x = T(ga["x"]).double()
    with torch.no_grad():
        assert torch.allclose(fa.transform.f(torch.tensor(0.3, dtype=torch.float64), x, ca), cnf_ref.field(W, B, fr, 0.3, x, ca)[0], rtol=1e-12, atol=1e-12)


def test_training_gradients_of_the_torch_op_path_equal_the_references(monkeypatch):
    """train() mode, float64, on the CPU (the torch-op path is device-agnostic; the product refuses CPU tensors by policy, lifted here): the gradient of
    log_prob.mean() through the exact trace (grad of grad) and the checkpoint adjoint, against the reference's."""
    from zuko_amd import ops
    from zuko_amd.flows import CNF

    g = golden("flow_cnf_small.npz")
    monkeypatch.setattr(ops, "_require_device", lambda *ts: None)
    torch.manual_seed(FLOW_SEED)
    flow = CNF(**FLOW_KW).double().train()
    x, c = T(g["x"]).double(), T(g["c"]).double()
    lp = flow(c).log_prob(x)
    assert ops.CNF_STATS["path"] == "torch" and torch.allclose(lp.detach(), T(g["lp64"]), rtol=1e-9, atol=1e-9)
    lp.mean().backward()
    for k, p in flow.named_parameters():
        ref = T(g["grad/" + k]).double()
        d = float((p.grad - ref).abs().max())
        print(f"{k}: max |d| {d:.3e} of {float(ref.abs().max()):.3e}")
        assert d <= 2e-4 * float(ref.abs().max()), k
    with torch.no_grad():
        d = flow.eval()(c)
        z = d.transform(x)
        assert torch.allclose(z, T(g["z64"]), rtol=1e-10, atol=1e-10) and torch.allclose(d.transform.inv(z), T(g["inv64"]), rtol=1e-10, atol=1e-10)


def test_supported_predicate_over_the_envelopes_edges_agrees_with_the_library():
    import torch.nn as nn

    import zuko_amd._C as C
    from zuko_amd import cnf_plan, ops

    lib = C.lib()
    assert ops.CNF_KERNEL is True
    ELU = nn.ELU
    for F, ctx, hidden, Q, act, want in [(3, 2, (64, 64), 3, ELU, True), (16, 0, (64, 64), 3, ELU, True), (17, 0, (64, 64), 3, ELU, False), (1, 0, (16,), 1, ELU, True),
                                         (0, 0, (16,), 3, ELU, False), (4, 900, (128, 128), 3, ELU, True), (4, 2, (30, 30), 3, ELU, False), (4, 2, (144,), 3, ELU, False),
                                         (4, 2, (64, 64, 64, 64), 3, ELU, False), (4, 2, (), 3, ELU, False), (4, 2, (16, 48, 128), 8, ELU, True), (4, 2, (64, 64), 9, ELU, False),
                                         (4, 2, (64, 64), 0, ELU, False), (4, 2, (64, 64), 3, nn.Tanh, False), (4, 2, (64, 64), 3, lambda: nn.ELU(alpha=0.5), False),
                                         (4, 2, (64, 64), 3, nn.ELU(), True), (4, 2, (64, 64), 3, None, True), (16, 0, (128, 128, 128), 8, ELU, False),
                                         (8, 0, (128, 128, 64), 3, ELU, True), (16, 0, (128, 128, 64), 8, ELU, False)]:  # (the last one: an image above 128 KiB)
        assert ops.cnf_supported(F, ctx, hidden, Q, act) == want, (F, ctx, hidden, Q, act)
        w = list(hidden[:3]) + [0] * (3 - min(3, len(hidden)))
        n = lib.zk_cnf_image_floats(F, Q, len(hidden), *w)
        lay = cnf_plan.layout(F, Q, hidden)
        assert (n > 0) == (lay is not None) and (lay is None or lay.total == n), (F, hidden, Q)
        if type(act) is type and act is ELU:
            assert (n > 0) == want
    assert lib.zk_cnf_image_floats(4, 3, 2, 64, 0, 0) <= 0 and lib.zk_cnf_image_floats(4, 3, 1, 64, 64, 0) <= 0  # (widths and n_hidden must agree)


def _emulate(img, L, fr, t, x, pre):
    """(f, trace) from the image alone, read where the kernel reads it: lane (j, q) fragments of the first layer, 256-float tiles of the hidden
    layers, the permuted rows of the last layer, the plain tangent columns and trace rows."""
    Q, F, widths = L.Q, L.F, L.widths
    lane = np.arange(64)
    j, q = lane & 15, lane >> 4
    arg = img[L.o_fr : L.o_fr + Q] * t
    emb = np.concatenate([np.cos(arg), np.sin(arg), np.zeros(16)])
    xin = np.concatenate([x, np.zeros(16)])
    p = pre.copy()
    for o in range(L.T[0]):
        for s in range(L.kt):
            frag = img[L.o_w0t + (o * L.kt + s) * 64 :][:64]
            np.add.at(p, 16 * o + j, frag * emb[4 * s + q])
        for s in range(L.kx):
            frag = img[L.o_w0x + (o * L.kx + s) * 64 :][:64]
            np.add.at(p, 16 * o + j, frag * xin[4 * s + q])
    elu = lambda v: np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    delu = lambda v: np.where(v > 0, 1.0, np.exp(np.minimum(v, 0)))
    h, Tn = elu(p), delu(p)[:, None] * img[L.o_w0c : L.o_w0c + F * widths[0]].reshape(F, widths[0]).T
    e = np.arange(256)
    ej, eq, er = (e >> 2) & 15, e >> 6, e & 3

    def matrix(base, tout, tin):
        M = np.zeros((16 * tout, 16 * tin))
        for o in range(tout):
            for i in range(tin):
                M[16 * o + ej, 16 * i + 4 * eq + er] = img[base + (o * tin + i) * 256 :][:256]
        return M

    for l in range(1, len(widths)):
        M = matrix(L.o_w[l], L.T[l], L.T[l - 1])
        p = M @ h + img[L.o_b[l] : L.o_b[l] + widths[l]]
        h, Tn = elu(p), delu(p)[:, None] * (M @ Tn)
    out16 = matrix(L.o_wo, 1, L.T[-1]) @ h + np.array([img[L.o_bo + m] for m in range(16)])
    f = np.array([out16[4 * (i & 3) + (i >> 2)] for i in range(F)])  # (feature i sits in row m with 4 (m & 3) + (m >> 2) = i)
    assert all(out16[m] == 0 for m in range(16) if 4 * (m & 3) + (m >> 2) >= F)
    wl = img[L.o_wl : L.o_wl + F * widths[-1]].reshape(F, widths[-1])
    return f, sum(wl[i] @ Tn[:, i] for i in range(F))


@pytest.mark.parametrize("F,C,widths,Q", [(3, 2, (64, 64), 3), (5, 0, (32,), 1), (16, 3, (16, 48, 128), 2), (1, 0, (16,), 8), (7, 1, (128, 16), 5)])
def test_weight_image_walked_in_the_kernels_order_reproduces_cnf_ref(F, C, widths, Q):
    from zuko_amd import cnf_plan

    rng = np.random.default_rng(F + Q)
    dims = [2 * Q + F + C, *widths, F]
    W = [rng.uniform(-1, 1, (b, a)) / np.sqrt(a) for a, b in zip(dims[:-1], dims[1:])]
    B = [rng.uniform(-1, 1, b) for b in dims[1:]]
    fr = np.arange(1, Q + 1) * np.pi
    L = cnf_plan.layout(F, Q, widths)
    idx = cnf_plan.index_table(F, Q, C, widths)
    assert idx.shape == (L.total,) and L.total % 4 == 0
    w_off, b_off, f_off, total = cnf_plan.flat_offsets(F, Q, C, widths)
    flat = np.concatenate([w.reshape(-1) for w in W] + B + [fr])
    assert flat.size == total and idx.max() < total
    img = np.where(idx < 0, 0.0, flat[np.maximum(idx, 0)])
    x, c = rng.standard_normal((6, F)), rng.standard_normal((6, C))
    for n in range(6):
        pre = W[0][:, 2 * Q + F :] @ c[n] + B[0]
        f, tr = _emulate(img, L, fr, 0.37, x[n], pre)
        f_ref, tr_ref = cnf_ref.field([T(w) for w in W], [T(b) for b in B], T(fr), 0.37, T(x[n : n + 1]), T(c[n : n + 1]) if C else None)
        assert np.allclose(f, f_ref[0].numpy(), rtol=1e-12, atol=1e-12) and np.allclose(tr, tr_ref[0].numpy(), rtol=1e-12, atol=1e-12)


def test_image_of_a_module_and_invalidate():
    import torch.nn as nn

    import zuko_amd
    from zuko_amd import cnf_plan
    from zuko_amd.flows import CNF

    flow = CNF(5, 3)
    assert cnf_plan.shape_of(flow.transform) == (5, 3, (64, 64), 3)
    assert cnf_plan.flat_parameters(flow.transform).numel() == cnf_plan.flat_offsets(5, 3, 3, (64, 64))[3]
    for kw in (dict(activation=nn.Tanh), dict(activation=lambda: nn.ELU(alpha=0.5)), dict(hidden_features=(30, 30))):
        t = CNF(5, 3, **kw).transform
        assert (cnf_plan.shape_of(t) is None or cnf_plan.layout(5, 3, cnf_plan.shape_of(t)[2]) is None) and cnf_plan.image_of(t, "cpu") is None
    flow.transform.__dict__["_cnf_image_cache"] = ("key", object())
    zuko_amd.invalidate(flow)
    assert "_cnf_image_cache" not in flow.transform.__dict__


def test_cnf_step_rejects_foreign_blocks_and_unsupported_arguments_without_a_device():
    import zuko_amd._C as C

    lib, EINVAL = C.lib(), 1
    text = open(C._HEADER).read()
    for sym in ("zk_cnf_step", "zk_cnf_image_floats"):
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym)
    assert "zk_cnf_args_v1" in C.STRUCTS

    def block(**kw):
        base = dict(features=5, freqs=3, n_hidden=2, width0=64, width1=64, width2=0, image_floats=lib.zk_cnf_image_floats(5, 3, 2, 64, 64, 0), n_tangents=5, N=0,
                    ldx=5, ldy=5, ld_pre=64, t=0.0, dt=1.0, atol=1e-6, rtol=1e-5, trace_scale=1e-2)
        base.update(kw)
        return C.args("zk_cnf_args_v1", **base)

    fn = lib.zk_cnf_step
    assert fn(block(), None) == 0  # (a well-formed block over zero rows: accepted, nothing to launch — with every pointer null)
    for kw in (dict(n_tangents=0), dict(n_tangents=0, trace_scale=0.0), dict(ld_pre=0), dict(ld_pre=68), dict(ldx=9, ldy=7), dict(dt=-0.5, t=1.0), dict(atol=0.0), dict(rtol=0.0),
               dict(features=16, ldx=16, ldy=16, n_tangents=16, image_floats=lib.zk_cnf_image_floats(16, 3, 2, 64, 64, 0))):
        assert fn(block(**kw), None) == 0, kw
    for delta in (-8, 8):
        bad = block()
        bad.struct_size += delta
        assert fn(bad, None) == EINVAL
    bad = block()
    bad.version = 2
    assert fn(bad, None) == EINVAL and fn(None, None) == EINVAL
    nan, inf = float("nan"), float("inf")
    for kw in (dict(features=0), dict(features=17, ldx=17, ldy=17, n_tangents=17), dict(freqs=0), dict(freqs=9), dict(n_hidden=0), dict(n_hidden=4), dict(width0=30, width1=30),
               dict(width0=144), dict(width1=0), dict(width2=64), dict(n_hidden=3, width2=128, width0=128, width1=128), dict(image_floats=1), dict(n_tangents=4),
               dict(n_tangents=-1), dict(N=-1), dict(ldx=4), dict(ldy=4), dict(ld_pre=60), dict(ld_pre=66), dict(ld_pre=-64), dict(t=nan), dict(dt=inf), dict(atol=-1e-6),
               dict(rtol=nan), dict(atol=inf), dict(trace_scale=0.0), dict(trace_scale=nan)):
        assert fn(block(**kw), None) == EINVAL, kw
    assert fn(block(N=4), None) == EINVAL  # (rows but no pointers)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    some = dict(N=4, x=p, pre=p, image=p, y=p, err=p)
    assert fn(block(**some), None) == EINVAL  # (tangents but no l / l_next)
    assert fn(block(**dict(some, l=p, l_next=p, pre=p + 4)), None) == EINVAL and fn(block(**dict(some, l=p, l_next=p, image=p + 8)), None) == EINVAL  # (16-byte alignment)
    assert fn(block(**dict(some, N=(1 << 37) + 1, l=p, l_next=p)), None) == EINVAL  # (more blocks than a grid has)


def test_capture_refuses_a_continuous_flow():
    import zuko_amd
    from zuko_amd.flows import CNF
    from zuko_amd.graph import _refuse_continuous

    with pytest.raises(NotImplementedError, match="cannot be captured"):
        _refuse_continuous(CNF(3, 2), "capture")
    _refuse_continuous(zuko_amd.flows.MAF(3, 2, transforms=1), "capture")
