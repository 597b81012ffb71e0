"""GPU: a float64 spline flow trains.  The adjoint kernels of the conditioner layer and of the spline are float32, so a float64 call that needs
gradients evaluates ops.linear / ops.rqs_forward as float64 torch ops on the device (it raised NotImplementedError before); the base density already
did.  Against float64 autograd through the CPU oracle, and — an implementation that shares no formula with either — against the float32 HIP kernels
on the same flow."""

import pytest
import torch

from oracle import zuko_oracle as O

pytestmark = pytest.mark.gpu


def _oracle_grads(flow, kind, features, x, c, uni):
    sd = {k: v.detach().cpu().clone() for k, v in flow.state_dict().items() if v is not None}
    leaves = {k: v.double().requires_grad_() for k, v in sd.items() if v.is_floating_point() and ("weight" in k or "bias" in k)}
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    sd.update(leaves)
    spec = O.spec_from_state_dict(sd, kind, uni, features)
    xr = x.double().clone().requires_grad_()
    loss = -O.flow_log_prob(spec, xr, None if c is None else c.double()).mean()
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in leaves.items()}, xr.grad


def _grads(flow, x, c):
    flow.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_()
    loss = -(flow(c) if c is not None else flow()).log_prob(xg).mean()
    loss.backward()
    return loss, {k: p.grad.detach().cpu().double() for k, p in flow.named_parameters()}, xg.grad.cpu().double()


def _flow(which):
    import zuko_amd.flows as F
    from zuko_amd.transforms import MonotonicRQSTransform

    torch.manual_seed(5)
    if which == "coupling":
        return F.NICE(16, 0, transforms=2, hidden_features=[64, 64], univariate=MonotonicRQSTransform, shapes=[(8,), (8,), (7,)]), "coupling", 16, 0
    return F.NSF(5, 3, transforms=2, bins=8, hidden_features=[64, 64]), "ar", 5, 3


@pytest.mark.parametrize("which", ["coupling", "autoregressive"])
def test_float64_spline_flow_trains(dev, which):
    """Loss and every gradient of a float64 flow: the float64 oracle's to 1e-10 of max |grad| (float64 on both sides: what separates them is the order
    of the sums), and the float32 flow's on the HIP kernels to that path's own bar against the oracle, 2e-4 of max |grad| (loss 1e-5 relative)."""
    flow, kind, D, C = _flow(which)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(64, D, generator=g) * 2.0
    c = torch.randn(64, C, generator=g) if C else None
    ref_loss, ref_grads, ref_gx = _oracle_grads(flow, kind, D, x, c, O.uni_rqs(8))
    flow = flow.to(dev)
    loss32, grads32, gx32 = _grads(flow, x.to(dev), None if c is None else c.to(dev))
    flow = flow.double()
    loss, grads, gx = _grads(flow, x.to(dev).double(), None if c is None else c.to(dev).double())
    assert loss.dtype == torch.float64 and all(p.grad is not None and p.grad.dtype == torch.float64 for p in flow.parameters())
    assert set(grads) == set(ref_grads)
    mx = lambda a, b: ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()
    assert abs(loss.item() - ref_loss.item()) < 1e-10 * abs(ref_loss.item())
    worst = max(mx(grads[k], ref_grads[k]) for k in ref_grads)
    assert worst < 1e-10 and mx(gx, ref_gx) < 1e-10, (worst, mx(gx, ref_gx))
    assert abs(loss32.item() - loss.item()) < 1e-5 * abs(loss.item())
    worst32 = max(mx(grads32[k], grads[k]) for k in grads)
    print(f"{which}: float64 path vs oracle {worst:.1e}; float32 kernels vs float64 path {worst32:.1e}, dx {mx(gx32, gx):.1e} of max |grad|")
    assert worst32 < 2e-4 and mx(gx32, gx) < 2e-4, (worst32, mx(gx32, gx))


def test_float64_flow_takes_an_optimiser_step_and_float32_is_untouched(dev):
    """Five Adam steps lower a float64 flow's loss; a float32 flow's graph still holds the kernels' autograd nodes (the float64 path is taken for
    float64 operands only)."""
    flow, _, D, _ = _flow("coupling")
    x = torch.randn(256, D, generator=torch.Generator().manual_seed(7)).to(dev)
    names, stack, seen = set(), [(-flow.to(dev)().log_prob(x).mean()).grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is not None and fn not in seen:
            seen.add(fn)
            names.add(type(fn).__name__)
            stack += [n for n, _ in fn.next_functions]
    assert "UnivariatePackedFnBackward" in names and not any("Softmax" in n or "Cumsum" in n for n in names)
    flow, x = flow.double(), x.double()
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        loss = -flow().log_prob(x).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
