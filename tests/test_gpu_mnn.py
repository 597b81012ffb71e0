"""GPU: the monotone-network kernels (zk_mnn_forward / zk_mnn_inverse) through the C ABI against the reference's fixtures, their independence and
determinism properties, the torch-op fallback, and the neural autoregressive flow built on them (tests/golden/make_golden_naf.py wrote the fixtures).
Bars: tests/parity.py (assert_parity with its constants); gradients as tests/test_gpu_backward.py."""

import numpy as np
import pytest
import torch

import mnn_ref
from conftest import T, golden, sd_hash
from mnn_nets import MnnNet as Net
from parity import C_NOISE, _stats, assert_parity

pytestmark = pytest.mark.gpu

KERNEL_CASES = {"mnn_a": (16, (64, 64)), "mnn_b": (3, (32,)), "mnn_c": (7, (16, 48, 128))}
NAF_KW, NAF_SEED = dict(features=5, context=3, transforms=2), 11


@pytest.fixture(scope="module")
def nets(dev):
    out = {}
    for name in KERNEL_CASES:
        g = golden(name + ".npz")
        out[name] = (g, Net(g, dev))
    return out


def _inputs(g, dev, key="x"):
    x, sig = T(g[key], dev), T(g["signal"], dev)
    return x, sig.reshape(sig.shape[0], -1)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_forward_parity_through_the_c_abi(dev, nets, name):
    g, net = nets[name]
    x, sig = _inputs(g, dev)
    y, ladj = net.forward(x, sig)
    assert_parity(y, g["y32"], g["y64"], f"{name}: mnn y")
    assert_parity(ladj, g["ladj32"], g["ladj64"], f"{name}: mnn ladj")
    y_r, ladj_r = net.forward(x, sig, reduce=True)
    assert torch.equal(y_r, y)
    assert_parity(ladj_r, g["ladj32"].sum(-1, dtype=np.float32), g["ladj64"].sum(-1), f"{name}: mnn ladj reduced")
    # the row sum adds the columns left to right: exactly the fp32 sum of the per-element values in that order
    acc = torch.zeros_like(ladj_r)
    for d in range(ladj.shape[1]):
        acc = acc + ladj[:, d]
    assert torch.equal(ladj_r, acc)
    # padded row strides of x and of the signal: the same bits
    N, D = x.shape
    xp, sp = torch.full((N, D + 3), float("nan"), device=dev), torch.full((N, sig.shape[1] + 5), float("nan"), device=dev)
    xp[:, :D], sp[:, : sig.shape[1]] = x, sig
    y_p, ladj_p = net.forward(xp[:, :D], sp[:, : sig.shape[1]])
    assert torch.equal(y_p, y) and torch.equal(ladj_p, ladj)
    assert_parity(y_p, g["y32"], g["y64"], f"{name}: mnn y, padded strides")
    assert_parity(ladj_p, g["ladj32"], g["ladj64"], f"{name}: mnn ladj, padded strides")


def _module_for(g, dev, dtype=torch.float32):
    from zuko_amd.flows import MNN

    W, B = mnn_ref.params_of(g)
    m = MNN(signal=W[0].shape[2] - 1, stack=W[0].shape[0], hidden_features=tuple(w.shape[1] for w in W[:-1]))
    with torch.no_grad():
        for lin, w, b in zip([l for l in m.network if hasattr(l, "weight")], W, B):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    return m.to(device=dev, dtype=dtype).requires_grad_(False)


def test_unsupported_shape_runs_the_fallback_at_the_same_bar(dev):
    from zuko_amd import ops

    g = golden("mnn_d.npz")
    assert not ops.mnn_supported(16, (30, 30)) and ops.mnn_supported(16, (64, 64))
    m = _module_for(g, dev)
    t = m(T(g["signal"], dev))
    with torch.no_grad():
        y, ladj = t.call_and_ladj(T(g["x"], dev))
        ladj_r = t.call_and_ladj_reduced(T(g["x"], dev))[1]
        inv = t.inv(T(g["targets"], dev))
    assert_parity(y, g["y32"], g["y64"], "mnn_d (fallback): y")
    assert_parity(ladj, g["ladj32"], g["ladj64"], "mnn_d (fallback): ladj")
    assert_parity(ladj_r, g["ladj32"].sum(-1, dtype=np.float32), g["ladj64"].sum(-1), "mnn_d (fallback): ladj reduced")
    assert_parity(inv, g["inv32"], g["inv64"], "mnn_d (fallback): inverse")


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_the_transform_object_runs_the_kernel_and_equals_the_c_abi(dev, nets, name):
    """MonotonicNetworkTransform (ops.mnn_forward / mnn_inverse: image cache, broadcasting, feature selection) gives the bits of the direct calls;
    float64 inputs take the torch-op path and meet the float64 bar."""
    from parity import assert_f64

    g, net = nets[name]
    x, sig = _inputs(g, dev)
    m = _module_for(g, dev)
    t = m(T(g["signal"], dev))
    y, ladj = net.forward(x, sig)
    y_t, ladj_t = t.call_and_ladj(x)
    assert torch.equal(y_t, y) and torch.equal(ladj_t, ladj)
    assert torch.equal(t.call_and_ladj_reduced(x)[1], net.forward(x, sig, reduce=True)[1])
    assert torch.equal(t.inv(T(g["targets"], dev)), net.inverse(T(g["targets"], dev), sig))
    sel = torch.tensor([2, 0], device=dev)
    t_sel = m(T(g["signal"], dev)[:, [2, 0]], features=sel)
    assert torch.equal(t_sel(x[:, [2, 0]]), y[:, [2, 0]])
    m64 = _module_for(g, dev, torch.float64)
    y64, ladj64 = m64(T(g["signal"], dev).double()).call_and_ladj(x.double())
    assert_f64(y64, g["y64"], f"{name}: float64 fallback y", 1e-11)
    assert_f64(ladj64, g["ladj64"], f"{name}: float64 fallback ladj", 1e-11)


def test_results_do_not_depend_on_the_batch_the_columns_or_the_run(dev, nets):
    g, net = nets["mnn_a"]
    gen = torch.Generator().manual_seed(5)
    N, D, S = 1031, 5, 16
    x = ((torch.rand(N, D, generator=gen) * 2 - 1) * 9.5).to(dev)
    sig = (1.5 * torch.randn(N, D * S, generator=gen)).to(dev)
    y, ladj = net.forward(x, sig)
    inv = net.inverse(y, sig)
    ref_y, ref_l = mnn_ref.forward(net.W, net.B, x, sig.reshape(N, D, S))
    assert torch.allclose(y, ref_y, rtol=1e-4, atol=1e-4) and torch.allclose(ladj, ref_l, rtol=1e-4, atol=1e-4)  # (a sanity bound; parity is asserted on the fixtures)
    for k in (1, 63, 64, 65, 257):
        y_k, ladj_k = net.forward(x[:k].contiguous(), sig[:k].contiguous())
        assert torch.equal(y_k, y[:k]) and torch.equal(ladj_k, ladj[:k]), f"N = {k}"
        assert torch.equal(net.inverse(y[:k].contiguous(), sig[:k].contiguous()), inv[:k]), f"inverse, N = {k}"
    cols = [3, 1]
    feat = torch.tensor(cols, dtype=torch.int32, device=dev)
    sig_c = sig.reshape(N, D, S)[:, cols].reshape(N, -1).contiguous()
    y_c, ladj_c = net.forward(x[:, cols].contiguous(), sig_c, feat=feat)
    assert torch.equal(y_c, y[:, cols]) and torch.equal(ladj_c, ladj[:, cols])
    assert torch.equal(net.inverse(y[:, cols].contiguous(), sig_c, feat=feat), inv[:, cols])
    y2, ladj2 = net.forward(x, sig)
    assert torch.equal(y2, y) and torch.equal(ladj2, ladj) and torch.equal(net.inverse(y, sig), inv)


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_inverse_parity_and_round_trip(dev, nets, name):
    """x = f^-1(targets) against the reference's bisection (out-of-range targets included), and the round trip |f(x) - target| evaluated in float64:
    two bisections of equal depth share the interval bound, so the kernel's residual stays within the suite's noise constant of the float32
    reference's own on the same targets."""
    g, net = nets[name]
    t, sig = _inputs(g, dev, "targets")
    x = net.inverse(t, sig)
    assert_parity(x, g["inv32"], g["inv64"], f"{name}: mnn inverse")
    assert torch.equal(x[:4].cpu(), T(g["inv32"])[:4]), "targets outside f(+-bound): the end of the interval the reference reaches"
    W64, B64 = mnn_ref.params_of(g, dtype=torch.float64)
    s64, t64 = T(g["signal"]).double(), T(g["targets"]).double()
    res = lambda v: (mnn_ref.forward(W64, B64, v.double().cpu(), s64, tangent=False)[0] - t64).abs()[4:]
    r_hip, r_ref = _stats(res(x)), _stats(res(T(g["inv32"])))
    print(f"{name}: round trip |f(inv(y)) - y| max/p99.9/median  kernel {r_hip[0]:.3e}/{r_hip[1]:.3e}/{r_hip[2]:.3e}  float32 reference {r_ref[0]:.3e}/{r_ref[1]:.3e}/{r_ref[2]:.3e}")
    assert all(a <= C_NOISE * b for a, b in zip(r_hip, r_ref)), (r_hip, r_ref)


@pytest.fixture(scope="module")
def naf(dev):
    import zuko_amd.flows as F

    g = golden("flow_naf_small.npz")
    torch.manual_seed(NAF_SEED)
    flow = F.NAF(**NAF_KW)
    assert sd_hash(flow.state_dict()) == bytes(g["hash"]).decode()
    return g, flow.to(dev)


def test_flow_log_prob_transform_and_inverse(dev, naf):
    g, flow = naf
    x, c = T(g["x"], dev), T(g["c"], dev)
    with torch.no_grad():
        dist = flow(c)
        lp, z = dist.log_prob(x), dist.transform(x)
        x_inv = dist.transform.inv(T(g["z32"], dev))
    assert_parity(lp, g["log_prob32"], g["log_prob64"], "naf_small: log_prob")
    assert_parity(z, g["z32"], g["z64"], "naf_small: transform")
    assert_parity(x_inv, g["x_inv32"], g["x_inv64"], "naf_small: transform.inv")
    assert float((x_inv - x).abs().max()) < 1e-4


def test_flow_sampling(dev, naf):
    import copy

    g, flow = naf
    c = T(g["c"], dev)[:7]
    flow64 = copy.deepcopy(flow).double()
    with torch.no_grad():
        assert tuple(flow(c[0]).sample((7,)).shape) == (7, 5)
        assert tuple(flow(c).sample().shape) == (7, 5)
        xs, lp = flow(c).rsample_and_log_prob()
        assert tuple(xs.shape) == (7, 5) and tuple(lp.shape) == (7,) and bool(torch.isfinite(xs).all())
        assert_parity(lp, flow(c).log_prob(xs), flow64(c.double()).log_prob(xs.double()), "naf_small: rsample_and_log_prob vs log_prob of its sample")


@pytest.mark.parametrize("randperm", [False, True])
def test_descending_and_permuted_orders_round_trip(dev, randperm):
    import zuko_amd.flows as F

    torch.manual_seed(3)
    flow = F.NAF(6, 0, transforms=2, randperm=randperm, hidden_features=[32, 32]).to(dev)  # (transform 2 of the fixed orders is descending)
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


def test_gradients_of_log_prob_through_the_fallback(dev, naf):
    """Training runs the torch-op path (no adjoint kernel yet): d log_prob.mean() / d parameter against the reference's float64 gradients, within 2e-4 of
    max |grad| per tensor — the bar of tests/test_gpu_backward.py at these row counts."""
    import copy

    g, flow = naf
    flow = copy.deepcopy(flow).train()
    flow(T(g["c"], dev)).log_prob(T(g["x"], dev)).mean().backward()
    for k, p in flow.named_parameters():
        ref = T(g["grad/" + k]).double()
        assert p.grad is not None, k
        d, scale = float((p.grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
        assert d <= 2e-4 * scale, f"{k}: |d| {d:.3e} vs max |grad| {scale:.3e}"
