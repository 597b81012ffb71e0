"""GPU: the unconstrained-monotone-network kernels (zk_umnn_forward / zk_umnn_inverse) through the C ABI against the reference's fixtures, their
independence and determinism properties, the torch-op fallback, and the unconstrained neural autoregressive flow built on them
(tests/golden/make_golden_unaf.py wrote the fixtures).  Bars: tests/parity.py (assert_parity with its constants); gradients as tests/test_gpu_mnn.py."""

import numpy as np
import pytest
import torch

import umnn_ref
from conftest import T, golden, sd_hash
from mnn_nets import UmnnNet as Net
from parity import C_NOISE, _stats, assert_parity

pytestmark = pytest.mark.gpu

FORWARD_CASES = ["umnn_a", "umnn_b", "umnn_c", "umnn_e"]
INVERSE_CASES = ["umnn_a", "umnn_b", "umnn_c"]
UNAF_KW, UNAF_SEED = dict(features=5, context=3, transforms=2), 11


@pytest.fixture(scope="module")
def nets(dev):
    out = {}
    for name in FORWARD_CASES:
        g = golden(name + ".npz")
        out[name] = (g, Net(g, dev))
    return out


def _inputs(g, dev, key="x"):
    return T(g[key], dev), T(g["signal"], dev), T(g["constant"], dev)


def _packed(sig, cst):
    """phi [N, D, S + 1] as the conditioner emits it, and the views the layer cuts from it."""
    phi = torch.cat((sig, cst[..., None]), dim=-1).contiguous()
    return phi[..., :-1], phi[..., -1]


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_forward_parity_through_the_c_abi(dev, nets, name):
    g, net = nets[name]
    x, sig, cst = _inputs(g, dev)
    y, ladj = net.forward(x, sig, cst)
    assert_parity(y, g["y32"], g["y64"], f"{name}: umnn y")
    assert_parity(ladj, g["ladj32"], g["ladj64"], f"{name}: umnn ladj")
    y_r, ladj_r = net.forward(x, sig, cst, reduce=True)
    assert torch.equal(y_r, y)
    assert_parity(ladj_r, g["ladj32"].sum(-1, dtype=np.float32), g["ladj64"].sum(-1), f"{name}: umnn ladj reduced")
    # the row sum adds the columns left to right: exactly the fp32 sum of the per-element values in that order
    acc = torch.zeros_like(ladj_r)
    for d in range(ladj.shape[1]):
        acc = acc + ladj[:, d]
    assert torch.equal(ladj_r, acc)
    # NaN-padded row strides of x, of the signal and of the constant: the same bits
    N, D, S = sig.shape
    xp, sp, cp = (torch.full(s, float("nan"), device=dev) for s in ((N, D + 3), (N, D * S + 5), (N, D + 2)))
    xp[:, :D], sp[:, : D * S], cp[:, :D] = x, sig.reshape(N, -1), cst
    y_p, ladj_p = net.forward(xp[:, :D], sp[:, : D * S].unflatten(1, (D, S)), cp[:, :D])
    assert torch.equal(y_p, y) and torch.equal(ladj_p, ladj)
    # the conditioner's packed phi read in place (ld_col = S + 1, the constant behind every element's signal): the same bits
    sig_v, cst_v = _packed(sig, cst)
    assert sig_v.stride(1) == S + 1 and cst_v.data_ptr() == sig_v.data_ptr() + 4 * S and cst_v.stride(1) == S + 1
    y_v, ladj_v = net.forward(x, sig_v, cst_v)
    assert torch.equal(y_v, y) and torch.equal(ladj_v, ladj)
    # no constant: y - constant up to the rounding of one addition
    y_0, ladj_0 = net.forward(x, sig, None)
    assert torch.equal(ladj_0, ladj) and torch.equal(y_0 + cst, y)


def _module_for(g, dev, dtype=torch.float32, **kw):
    from zuko_amd.flows import UMNN

    W, B = umnn_ref.params_of(g)
    m = UMNN(signal=W[0].shape[2] - 1, stack=W[0].shape[0], hidden_features=tuple(w.shape[1] for w in W[:-1]), **kw)
    with torch.no_grad():
        for lin, w, b in zip([l for l in m.integrand if hasattr(l, "weight")], W, B):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    return m.to(device=dev, dtype=dtype).requires_grad_(False)


def test_unsupported_shape_runs_the_fallback_at_the_same_bar(dev):
    from zuko_amd import ops

    g = golden("umnn_d.npz")
    assert not ops.umnn_supported(16, (30, 30)) and ops.umnn_supported(16, (64, 64))
    m = _module_for(g, dev)
    x, sig, cst = _inputs(g, dev)
    t = m(sig, cst)
    with torch.no_grad():
        y, ladj = t.call_and_ladj(x)
        ladj_r = t.call_and_ladj_reduced(x)[1]
        inv = t.inv(T(g["targets"], dev))
    assert_parity(y, g["y32"], g["y64"], "umnn_d (fallback): y")
    assert_parity(ladj, g["ladj32"], g["ladj64"], "umnn_d (fallback): ladj")
    assert_parity(ladj_r, g["ladj32"].sum(-1, dtype=np.float32), g["ladj64"].sum(-1), "umnn_d (fallback): ladj reduced")
    assert_parity(inv, g["inv32"], g["inv64"], "umnn_d (fallback): inverse")


def test_another_activation_runs_the_fallback(dev):
    """A Tanh integrand is not the kernel's: the torch-op path, checked against the independent restatement with the same activation in float64."""
    import torch.nn as nn

    from zuko_amd import mnn_plan

    g = golden("umnn_b.npz")
    m = _module_for(g, dev, activation=nn.Tanh)
    assert mnn_plan.image_of(m.integrand, dev) is None
    x, sig, cst = _inputs(g, dev)
    with torch.no_grad():
        y, ladj = m(sig, cst).call_and_ladj(x)
        back = m(sig, cst).inv(y)
    W, B = umnn_ref.params_of(g, dtype=torch.float64)
    old = umnn_ref.elu
    try:
        umnn_ref.elu = torch.tanh
        refs = [umnn_ref.forward([w.to(dt) for w in W], [b.to(dt) for b in B], T(g["x"]).to(dt), T(g["signal"]).to(dt), T(g["constant"]).to(dt)) for dt in (torch.float32, torch.float64)]
    finally:
        umnn_ref.elu = old
    assert_parity(y, refs[0][0], refs[1][0], "umnn_b with Tanh (fallback): y")
    assert_parity(ladj, refs[0][1], refs[1][1], "umnn_b with Tanh (fallback): ladj")
    assert float((back - x).abs().max()) < 1e-4


@pytest.mark.parametrize("name", INVERSE_CASES)
def test_the_transform_object_runs_the_kernel_and_equals_the_c_abi(dev, nets, name):
    """UnconstrainedMonotonicNetworkTransform (ops.umnn_forward / umnn_inverse: image cache, strides, feature selection) gives the bits of the direct
    calls, also on the views of a packed phi; float64 inputs take the torch-op path and meet the float64 bar."""
    from parity import assert_f64

    g, net = nets[name]
    x, sig, cst = _inputs(g, dev)
    tg = T(g["targets"], dev)
    m = _module_for(g, dev)
    y, ladj = net.forward(x, sig, cst)
    inv = net.inverse(tg, sig, cst)
    for s_, c_ in ((sig, cst), _packed(sig, cst)):
        t = m(s_, c_)
        y_t, ladj_t = t.call_and_ladj(x)
        assert torch.equal(y_t, y) and torch.equal(ladj_t, ladj)
        assert torch.equal(t.call_and_ladj_reduced(x)[1], net.forward(x, sig, cst, reduce=True)[1])
        assert torch.equal(t.inv(tg), inv)
    sel = torch.tensor([2, 0], device=dev)
    t_sel = m(sig[:, [2, 0]], cst[:, [2, 0]], features=sel)
    assert torch.equal(t_sel(x[:, [2, 0]]), y[:, [2, 0]]) and torch.equal(t_sel.inv(tg[:, [2, 0]]), inv[:, [2, 0]])
    m64 = _module_for(g, dev, torch.float64)
    t64 = m64(sig.double(), cst.double())
    y64, ladj64 = t64.call_and_ladj(x.double())
    assert_f64(y64, g["y64"], f"{name}: float64 fallback y", 1e-11)
    assert_f64(ladj64, g["ladj64"], f"{name}: float64 fallback ladj", 1e-11)
    assert_f64(t64.inv(tg.double()), g["inv64"], f"{name}: float64 fallback inverse", 1e-11)


def test_results_do_not_depend_on_the_batch_the_columns_or_the_run(dev, nets):
    g, net = nets["umnn_a"]
    gen = torch.Generator().manual_seed(5)
    N, D, S = 1031, 5, 16
    x = ((torch.rand(N, D, generator=gen) * 2 - 1) * 9.5).to(dev)
    sig = (1.5 * torch.randn(N, D, S, generator=gen)).to(dev)
    cst = torch.randn(N, D, generator=gen).to(dev)
    y, ladj = net.forward(x, sig, cst)
    inv = net.inverse(y, sig, cst)
    ref_y, ref_l = umnn_ref.forward(net.W, net.B, x, sig, cst)
    assert torch.allclose(y, ref_y, rtol=1e-4, atol=1e-4) and torch.allclose(ladj, ref_l, rtol=1e-4, atol=1e-4)  # (a sanity bound; parity is asserted on the fixtures)
    for k in (1, 63, 64, 65, 257):
        y_k, ladj_k = net.forward(x[:k].contiguous(), sig[:k].contiguous(), cst[:k].contiguous())
        assert torch.equal(y_k, y[:k]) and torch.equal(ladj_k, ladj[:k]), f"N = {k}"
        assert torch.equal(net.inverse(y[:k].contiguous(), sig[:k].contiguous(), cst[:k].contiguous()), inv[:k]), f"inverse, N = {k}"
    cols = [3, 1]
    feat = torch.tensor(cols, dtype=torch.int32, device=dev)
    sig_c, cst_c = sig[:, cols].contiguous(), cst[:, cols].contiguous()
    y_c, ladj_c = net.forward(x[:, cols].contiguous(), sig_c, cst_c, feat=feat)
    assert torch.equal(y_c, y[:, cols]) and torch.equal(ladj_c, ladj[:, cols])
    assert torch.equal(net.inverse(y[:, cols].contiguous(), sig_c, cst_c, feat=feat), inv[:, cols])
    y2, ladj2 = net.forward(x, sig, cst)
    assert torch.equal(y2, y) and torch.equal(ladj2, ladj) and torch.equal(net.inverse(y, sig, cst), inv)


@pytest.mark.parametrize("name", INVERSE_CASES)
def test_inverse_parity_and_round_trip(dev, nets, name):
    """x = f^-1(targets) against the reference's bisection (out-of-range targets included), and the round trip |f(x) + constant - target| evaluated in
    float64: two bisections of equal depth share the interval bound, so the kernel's residual stays within the suite's noise constant of the
    float32 reference's own on the same targets."""
    g, net = nets[name]
    t, sig, cst = _inputs(g, dev, "targets")
    x = net.inverse(t, sig, cst)
    assert_parity(x, g["inv32"], g["inv64"], f"{name}: umnn inverse")
    assert torch.equal(x[:2].cpu(), T(g["inv32"])[:2]), "targets outside f(+-bound): the end of the interval the reference reaches"
    x_v = net.inverse(t, *_packed(sig, cst))
    assert torch.equal(x_v, x)
    W64, B64 = umnn_ref.params_of(g, dtype=torch.float64)
    s64, c64, t64 = T(g["signal"]).double(), T(g["constant"]).double(), T(g["targets"]).double()
    res = lambda v: (umnn_ref.forward(W64, B64, v.double().cpu(), s64, c64)[0] - t64).abs()[2:]
    r_hip, r_ref = _stats(res(x)), _stats(res(T(g["inv32"])))
    print(f"{name}: round trip |f(inv(y)) - y| max/p99.9/median  kernel {r_hip[0]:.3e}/{r_hip[1]:.3e}/{r_hip[2]:.3e}  float32 reference {r_ref[0]:.3e}/{r_ref[1]:.3e}/{r_ref[2]:.3e}")
    assert all(a <= C_NOISE * b for a, b in zip(r_hip, r_ref)), (r_hip, r_ref)


@pytest.fixture(scope="module")
def unaf(dev):
    import zuko_amd.flows as F

    g = golden("flow_unaf_small.npz")
    torch.manual_seed(UNAF_SEED)
    flow = F.UNAF(**UNAF_KW)
    assert sd_hash(flow.state_dict()) == bytes(g["hash"]).decode()
    return g, flow.to(dev)


def test_flow_log_prob_transform_and_inverse(dev, unaf):
    g, flow = unaf
    x, c = T(g["x"], dev), T(g["c"], dev)
    with torch.no_grad():
        dist = flow(c)
        lp, z = dist.log_prob(x), dist.transform(x)
        x_inv = dist.transform.inv(T(g["z32"], dev))
    assert_parity(lp, g["log_prob32"], g["log_prob64"], "unaf_small: log_prob")
    assert_parity(z, g["z32"], g["z64"], "unaf_small: transform")
    assert_parity(x_inv, g["x_inv32"], g["x_inv64"], "unaf_small: transform.inv")
    assert float((x_inv - x).abs().max()) < 1e-4


def test_flow_runs_the_kernels_under_no_grad(dev, unaf):
    """log_prob and the inverse of the flow go through zk_umnn_forward / zk_umnn_inverse (counted by the binding's per-entry timing hook)."""
    import zuko_amd._C as C

    g, flow = unaf
    x, c = T(g["x"], dev), T(g["c"], dev)
    C.PROFILE = {}
    try:
        with torch.no_grad():
            z = flow(c).transform(x)
            flow(c).transform.inv(z)
        counts = {k: len(v) for k, v in C.PROFILE.items()}
    finally:
        C.PROFILE = None
    assert counts.get("zk_umnn_forward", 0) >= 2 and counts.get("zk_umnn_inverse", 0) >= 2 * 5, counts


def test_flow_sampling(dev, unaf):
    import copy

    g, flow = unaf
    c = T(g["c"], dev)[:7]
    flow64 = copy.deepcopy(flow).double()
    with torch.no_grad():
        assert tuple(flow(c[0]).sample((7,)).shape) == (7, 5)
        assert tuple(flow(c).sample().shape) == (7, 5)
        xs, lp = flow(c).rsample_and_log_prob()
        assert tuple(xs.shape) == (7, 5) and tuple(lp.shape) == (7,) and bool(torch.isfinite(xs).all())
        assert_parity(lp, flow(c).log_prob(xs), flow64(c.double()).log_prob(xs.double()), "unaf_small: rsample_and_log_prob vs log_prob of its sample")


@pytest.mark.parametrize("randperm", [False, True])
def test_descending_and_permuted_orders_round_trip(dev, randperm):
    import zuko_amd.flows as F

    torch.manual_seed(3)
    flow = F.UNAF(6, 0, transforms=2, randperm=randperm, hidden_features=[32, 32]).to(dev)  # (transform 2 of the fixed orders is descending)
    if not randperm:
        assert flow.transform.transforms[2].order.tolist() == [5, 4, 3, 2, 1, 0]
    x = torch.randn(65, 6, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        dist = flow()
        z, ladj = dist.transform.call_and_ladj(x)
        lp = dist.log_prob(x)
        back = dist.transform.inv(z)
    assert bool(torch.isfinite(z).all() and torch.isfinite(ladj).all() and torch.isfinite(lp).all())
    assert float((back - x).abs().max()) < 1e-4, float((back - x).abs().max())


def test_gradients_of_log_prob_through_the_fallback(dev, unaf):
    """Training runs the torch-op path (no adjoint kernel): d log_prob.mean() / d parameter against the reference's float64 gradients, within 2e-4 of
    max |grad| per tensor — the bar of tests/test_gpu_mnn.py."""
    import copy

    g, flow = unaf
    flow = copy.deepcopy(flow).train()
    flow(T(g["c"], dev)).log_prob(T(g["x"], dev)).mean().backward()
    for k, p in flow.named_parameters():
        ref = T(g["grad/" + k]).double()
        assert p.grad is not None, k
        d, scale = float((p.grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
        assert d <= 2e-4 * scale, f"{k}: |d| {d:.3e} vs max |grad| {scale:.3e}"
