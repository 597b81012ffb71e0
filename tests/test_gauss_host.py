"""CPU: the Gaussianization flow's host side.  tests/gauss_ref.py is pinned to the fixtures recorded from the live reference
(tests/golden/make_golden_gf.py), the closed-form adjoint the kernel implements is checked against autograd, zuko_amd.flows.GF has the reference's
module tree and initial values, and the new entry points refuse sizes outside their envelope before touching a device.  No kernel is launched."""

import numpy as np
import pytest
import torch

import gauss_ref as R
from conftest import T, golden, sd_hash

CASES = ["gauss_a", "gauss_b", "gauss_c", "gauss_d", "gauss_e", "gauss_f"]
EINVAL = 1


def _eval(g, dtype):
    x, b, a = (T(g[k]).to(dtype).requires_grad_() for k in ("x", "b", "a"))
    y, ladj = R.forward(x, b, a)
    gx, gb, ga = torch.autograd.grad((y * T(g["gy"]).to(dtype) + ladj * T(g["gl"]).to(dtype)).sum(), (x, b, a))
    inv = R.inverse(T(g["y64"]).float().to(dtype), b.detach(), a.detach())
    return {"y": y.detach(), "ladj": ladj.detach(), "gx": gx, "gb": gb, "ga": ga, "inv": inv}


@pytest.mark.parametrize("name", CASES)
def test_gauss_ref_reproduces_the_fixtures(name):
    g = golden(name + ".npz")
    N, D, K, shared = (int(v) for v in g["meta"])
    assert g["x"].shape == (N, D) and g["b"].shape == ((D, K) if shared else (N, D, K))
    for k, v in g.items():
        assert v.dtype.kind != "f" or np.isfinite(v).all(), k
    got = _eval(g, torch.float32)
    for k, v in got.items():
        assert np.array_equal(v.numpy(), g[k + "32"]), f"{name}: {k} (float32) is not bitwise the reference's"
    got = _eval(g, torch.float64)
    for k, v in got.items():
        ref = T(g[k + "64"])
        assert torch.allclose(v, ref, rtol=1e-12, atol=1e-12), f"{name}: {k} (float64) max |d| {(v - ref).abs().max():.3e}"


@pytest.mark.parametrize("shape", [(13, 3, 5), (7, 2, 32)])
def test_closed_form_adjoint_matches_autograd(shape):
    N, D, K = shape
    g = torch.Generator().manual_seed(7 + K)
    x = (1.5 * torch.randn(N, D, generator=g, dtype=torch.float64)).requires_grad_()
    b = torch.randn(N, D, K, generator=g, dtype=torch.float64).requires_grad_()
    a = (0.5 * torch.randn(N, D, K, generator=g, dtype=torch.float64)).requires_grad_()
    gy, gl = torch.randn(N, D, generator=g, dtype=torch.float64), torch.randn(N, D, generator=g, dtype=torch.float64)
    y, ladj = R.forward(x, b, a)
    want = torch.autograd.grad((y * gy + ladj * gl).sum(), (x, b, a))
    got = R.backward(x.detach(), b.detach(), a.detach(), gy, gl)
    for name, w, h in zip(("gx", "gb", "ga"), want, got):
        assert torch.allclose(h, w, rtol=1e-10, atol=1e-10), f"{name}: max |d| {(h - w).abs().max():.3e}"


REF_KEYS = {
    "flow_gf_small": [f"transform.transforms.{i}.hyper.{j}.{p}" for i in (0, 2, 4) for j in (0, 2, 4) for p in ("weight", "bias")]
    + ["transform.transforms.1.A", "transform.transforms.3.A", "base.loc", "base.scale"],
    "flow_gf_uncond": ["transform.transforms.0.phi.0", "transform.transforms.0.phi.1", "transform.transforms.1.A", "transform.transforms.2.phi.0",
                       "transform.transforms.2.phi.1", "base.loc", "base.scale"],
}
FLOWS = {"flow_gf_small": dict(features=5, context=3, transforms=3, components=4), "flow_gf_uncond": dict(features=3, transforms=2, components=5)}


@pytest.mark.parametrize("name", list(FLOWS))
def test_gf_module_tree_seed_and_state_dict(name):
    import zuko_amd.flows as F
    import zuko_amd.transforms as ZT
    from zuko_amd.lazy import UnconditionalTransform

    g = golden(name + ".npz")
    torch.manual_seed(11)
    flow = F.GF(**FLOWS[name])
    assert sorted(flow.state_dict()) == sorted(REF_KEYS[name])
    assert [n for n, _ in flow.named_parameters()] == list(g["param_names"])
    assert sd_hash(flow.state_dict()) == bytes(g["hash"]).decode()
    layers = list(flow.transform.transforms)
    assert len(layers) == 2 * FLOWS[name]["transforms"] - 1
    for i, t in enumerate(layers):
        if i % 2 == 0:
            assert isinstance(t, F.ElementWiseTransform) and t.univariate is ZT.GaussianizationTransform
        else:
            assert isinstance(t, UnconditionalTransform) and t.f is ZT.RotationTransform
    assert "GaussianizationTransform" in repr(flow) and "RotationTransform" in repr(flow)
    # load_state_dict round trip into a flow built under another seed
    torch.manual_seed(3)
    other = F.GF(**FLOWS[name])
    assert sd_hash(other.state_dict()) != sd_hash(flow.state_dict())
    other.load_state_dict(flow.state_dict())
    assert sd_hash(other.state_dict()) == bytes(g["hash"]).decode()
    assert F.GF is __import__("zuko_amd").flows.GF


@pytest.mark.parametrize("name", list(FLOWS))
def test_gauss_ref_reproduces_the_module_fixtures(name):
    """gauss_ref.gf_log_prob on the seeded state_dict: the recorded log_prob (float64 to 1e-12) and the recorded float64 gradients."""
    import zuko_amd.flows as F

    g = golden(name + ".npz")
    torch.manual_seed(11)
    sd = F.GF(**FLOWS[name]).state_dict()
    x, c = T(g["x"]), (T(g["c"]) if "c" in g else None)
    with torch.no_grad():
        lp32 = R.gf_log_prob(sd, x, c)
    assert torch.allclose(lp32, T(g["log_prob32"]), rtol=1e-6, atol=1e-6)
    sd64 = {k: v.detach().double().requires_grad_(not k.startswith("base.")) for k, v in sd.items()}
    lp64 = R.gf_log_prob(sd64, x.double(), None if c is None else c.double())
    assert torch.allclose(lp64.detach(), T(g["log_prob64"]), rtol=1e-12, atol=1e-12)
    lp64.mean().backward()
    for k in g["param_names"]:
        assert torch.allclose(sd64[str(k)].grad, T(g["grad/" + str(k)]), rtol=1e-10, atol=1e-12), k


def test_cpu_tensors_raise():
    import zuko_amd.flows as F
    import zuko_amd.transforms as ZT
    from zuko_amd import ops

    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gauss_forward(torch.zeros(4, 2), torch.zeros(4, 2, 8), torch.zeros(4, 2, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gauss_inverse(torch.zeros(4, 2), torch.zeros(4, 2, 8), torch.zeros(4, 2, 8))
    with pytest.raises(RuntimeError, match="HIP device"):
        ZT.GaussianizationTransform(torch.zeros(2, 8), torch.zeros(2, 8))(torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="HIP device"):
        F.GF(3, transforms=2)().log_prob(torch.zeros(4, 3))
    old = ops.GAUSS_KERNEL
    try:
        ops.GAUSS_KERNEL = False  # the torch-op path runs on the device too, never on the CPU
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.gauss_forward(torch.zeros(4, 2), torch.zeros(4, 2, 8), torch.zeros(4, 2, 8))
    finally:
        ops.GAUSS_KERNEL = old


def test_entry_points_reject_sizes_outside_the_envelope_without_a_device():
    import zuko_amd._C as C

    lib = C.lib()
    for K, dtype, want in ((0, 0, EINVAL), (65, 0, EINVAL), (65, 1, EINVAL), (8, 2, EINVAL), (8, 7, EINVAL), (-1, 1, EINVAL)):
        assert lib.zk_gauss_forward(dtype, 4, 2, K, None, None, 2 * K * 2, 2 * K, None, 2 * K * 2, 2 * K, None, None, 0, None) == want, (K, dtype)
        assert lib.zk_gauss_inverse(dtype, 4, 2, K, 10.0, 25, None, None, 2 * K * 2, 2 * K, None, 2 * K * 2, 2 * K, None, None) == want, (K, dtype)
    for K in (0, 33, 64, -1):
        assert lib.zk_gauss_backward(4, 2, K, None, None, None, None, 0, None, None, None) == EINVAL, K
    # empty inputs inside the envelope: nothing to launch
    assert lib.zk_gauss_forward(0, 0, 2, 8, None, None, 0, 0, None, 0, 0, None, None, 0, None) == 0
    assert lib.zk_gauss_backward(0, 2, 32, None, None, None, None, 0, None, None, None) == 0


def test_gauss_supported_agrees_with_the_entry_points():
    from zuko_amd import ops

    assert ops.GAUSS_KERNEL is True and ops.GAUSS_K_MAX == 64 and ops.GAUSS_K_MAX_BWD == 32
    for K in (0, 1, 8, 32, 33, 64, 65):
        for dtype in (torch.float32, torch.float64):
            assert ops.gauss_supported(K, dtype, False) == (1 <= K <= 64)
        assert ops.gauss_supported(K, torch.float32, True) == (1 <= K <= 32)
        assert not ops.gauss_supported(K, torch.float64, True)
        assert not ops.gauss_supported(K, torch.float16, False)
