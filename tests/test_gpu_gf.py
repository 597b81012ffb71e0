"""GPU: zuko_amd.flows.GF against the module fixtures recorded from the live reference (tests/golden/flow_gf_{small,uncond}.npz): log_prob, gradients,
sampling, the rotation, a short training run.  Bars: tests/parity.py; the float64 bar is that of tests/test_gpu_gauss.py, summed over the element-wise
layers' outputs (each contributes 1e-12 max(1, exp((y^2 - 9) / 2)) (1 + |y|) to the log-determinant)."""

import pytest
import torch

import gauss_ref as R
import parity
from conftest import T, golden, sd_hash
from parity import assert_parity

pytestmark = pytest.mark.gpu

FLOWS = {"flow_gf_small": dict(features=5, context=3, transforms=3, components=4), "flow_gf_uncond": dict(features=3, transforms=2, components=5)}
_REF: dict = {}


def _flow(name):
    import zuko_amd.flows as F

    torch.manual_seed(11)
    return F.GF(**FLOWS[name])


def _reference(name):
    """Computed once per fixture on the CPU and shared: the restated reference's float32 log_prob gradients (the yardstick of the gradient test), and
    the float64 outputs of every element-wise layer (the conditioning that scales the float64 bar)."""
    if name not in _REF:
        f = golden(name + ".npz")
        flow = _flow(name)
        x, c = T(f["x"]), (T(f["c"]) if "c" in f else None)
        sd32 = {k: v.detach().clone().requires_grad_(v.is_floating_point() and not k.startswith("base.")) for k, v in flow.state_dict().items()}
        names = list(f["param_names"])
        R.gf_log_prob(sd32, x, c).mean().backward()
        trace: list = []
        sd64 = {k: v.detach().double() for k, v in flow.state_dict().items()}
        with torch.no_grad():
            lp64 = R.gf_log_prob(sd64, x.double(), None if c is None else c.double(), trace)
        _REF[name] = ({k: sd32[k].grad for k in names}, trace, lp64)
    return _REF[name]


@pytest.mark.parametrize("name", list(FLOWS))
def test_log_prob_against_the_reference(name, dev):
    f = golden(name + ".npz")
    flow = _flow(name)
    assert sd_hash(flow.state_dict()) == f["hash"].tobytes().decode()
    flow = flow.to(dev)
    x, c = T(f["x"], dev), (T(f["c"], dev) if "c" in f else None)
    with torch.no_grad():
        lp = flow(c).log_prob(x)
    assert_parity(lp, f["log_prob32"], f["log_prob64"], f"{name}: log_prob")
    _, trace, lp64 = _reference(name)
    assert torch.allclose(lp64, T(f["log_prob64"]), rtol=1e-12, atol=1e-12)  # the restatement is the recorded reference
    with torch.no_grad():
        got = flow.double()(None if c is None else c.double()).log_prob(x.double()).cpu()
    bound = sum((1e-12 * torch.clamp(torch.exp((y**2 - 9) / 2), min=1.0) * (1 + y.abs())).sum(dim=-1) for y in trace)
    d = (got - T(f["log_prob64"])).abs()
    ratio = float((d / bound).max())
    parity.REPORT.append({"what": f"{name} f64: log_prob", "n": int(d.numel()), "f64_max_abs": float(d.max()), "f64_max_over_bound": ratio, "ok": ratio <= 1.0})
    assert ratio <= 1.0, f"{name} f64: log_prob max |d| / bound = {ratio:.3f} (max |d| {float(d.max()):.3e})"


@pytest.mark.parametrize("name", list(FLOWS))
def test_gradients_against_the_reference(name, dev):
    """d log_prob.mean() / d parameter for every parameter against the float64 fixture; the yardstick is the reference's own float32 gradient."""
    f = golden(name + ".npz")
    ref32, _, _ = _reference(name)
    flow = _flow(name).to(dev)
    x, c = T(f["x"], dev), (T(f["c"], dev) if "c" in f else None)
    flow(c).log_prob(x).mean().backward()
    names = [k for k, _ in flow.named_parameters()]
    assert names == list(f["param_names"])
    failed = []
    for k, p in flow.named_parameters():
        assert p.grad is not None, k
        try:
            rec = assert_parity(p.grad, ref32[k], f["grad/" + k], f"{name}: grad {k}")
            print(f"{name}: grad {k}: strict {rec['strict_1e-5']}, ratio {rec['ratio_max']:.2f}")
        except AssertionError as e:
            print(str(e))
            failed.append(k)
    assert not failed, f"{name}: gradients outside the parity bar: {failed}"


@pytest.mark.parametrize("name", list(FLOWS))
def test_sampling_and_round_trip(name, dev):
    from zuko_amd import ops

    f = golden(name + ".npz")
    flow = _flow(name).to(dev)
    D = FLOWS[name]["features"]
    c = T(f["c"], dev)[:64] if "c" in f else None
    torch.manual_seed(5)
    with torch.no_grad():
        d = flow(c)
        s = d.sample((64,)) if c is None else d.sample()
        assert s.shape == (64, D) and bool(torch.isfinite(s).all())
        z = torch.randn(64, D, device=dev).clamp(-3, 3)
        xs = d.transform.inv(z)
        back = d.transform(xs)
    # z -> x -> z: the element-wise layers invert by bisection to 2 * 10 / 2^25 in x; held to the reference's own float32 round trip
    sd = {k: v.detach().cpu() for k, v in flow.state_dict().items()}
    zc, cc = z.cpu(), (None if c is None else c.cpu())
    ref = _round_trip_reference(sd, zc, cc)
    assert_parity(back, ref, zc.double(), f"{name}: transform(transform.inv(z))")
    # rsample: gradients reach every parameter (the rotations' through torch ops, the maps' through zk_inverse_seed + zk_gauss_backward)
    d = flow(c)
    r = d.rsample((64,)) if c is None else d.rsample()
    assert r.requires_grad and r.shape == (64, D)
    r.square().mean().backward()
    for k, p in flow.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def _round_trip_reference(sd, z, c):
    """The restated reference's float32 forward(inverse(z)) through the whole transform, on the CPU."""
    layers = sorted({int(k.split(".")[2]) for k in sd if k.startswith("transform.transforms.")})

    def params(i, D):
        pre = f"transform.transforms.{i}."
        if pre + "phi.0" in sd:
            return sd[pre + "phi.0"], sd[pre + "phi.1"]
        h = c
        idx = sorted({int(k[len(pre + "hyper.") :].split(".")[0]) for k in sd if k.startswith(pre + "hyper.")})
        for j in idx:
            h = torch.nn.functional.linear(h, sd[pre + f"hyper.{j}.weight"], sd[pre + f"hyper.{j}.bias"])
            h = torch.relu(h) if j != idx[-1] else h
        return h.unflatten(-1, (D, -1)).chunk(2, dim=-1)

    def rot(i):
        A = sd[f"transform.transforms.{i}.A"]
        return torch.linalg.matrix_exp(A - A.mT)

    with torch.no_grad():
        x = z
        for i in reversed(layers):
            x = torch.einsum("...ij,...i->...j", rot(i), x) if f"transform.transforms.{i}.A" in sd else R.inverse(x, *params(i, z.shape[-1]))
        for i in layers:
            x = torch.einsum("...ij,...j->...i", rot(i), x) if f"transform.transforms.{i}.A" in sd else R.forward(x, *params(i, z.shape[-1]))[0]
    return x


def test_rotation(dev):
    import zuko_amd.transforms as ZT

    gen = torch.Generator().manual_seed(9)
    A = torch.randn(7, 7, generator=gen).to(dev).requires_grad_()
    x = torch.randn(33, 7, generator=gen).to(dev)
    t = ZT.RotationTransform(A)
    eye = torch.eye(7, device=dev)
    assert float((t.R @ t.R.mT - eye).detach().abs().max()) <= 1e-5
    y = t(x)
    assert float((t.inv(y) - x).detach().abs().max()) <= 1e-5
    ladj = t.log_abs_det_jacobian(x, y)
    assert ladj.shape == (33,) and bool((ladj == 0).all())
    assert torch.allclose(y.detach().cpu(), torch.einsum("ij,nj->ni", torch.linalg.matrix_exp((A - A.mT).detach().cpu()), x.cpu()), rtol=1e-5, atol=1e-5)
    y.square().sum().backward()  # |R x|^2 = |x|^2 for every A: the gradient is zero up to rounding, and it exists
    assert A.grad is not None and bool(torch.isfinite(A.grad).all()) and float(A.grad.abs().max()) <= 1e-3
    (ZT.RotationTransform(A)(x) * x).sum().backward()
    assert float(A.grad.abs().max()) > 1e-3


def test_training_lowers_the_loss(dev):
    import zuko_amd.flows as F

    torch.manual_seed(1)
    flow = F.GF(2, transforms=2, components=4).to(dev)
    gen = torch.Generator().manual_seed(2)
    x = (torch.randn(256, 2, generator=gen) * 0.4 + torch.where(torch.rand(256, 1, generator=gen) < 0.5, -1.2, 1.2)).to(dev)
    opt = torch.optim.Adam(flow.parameters(), lr=2e-2)
    losses = []
    for _ in range(20):
        loss = -flow().log_prob(x).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses


def test_capture_is_refused_with_a_clear_message(dev):
    import zuko_amd
    import zuko_amd.flows as F

    flow = F.GF(3, transforms=2).to(dev)
    with pytest.raises(NotImplementedError, match="Gaussianization flow"):
        zuko_amd.capture(flow, torch.zeros(8, 3, device=dev))
