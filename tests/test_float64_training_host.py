"""CPU: the float64 gradient paths of the conditioner layer and of the rational-quadratic spline (zuko_amd.ops: _linear_torch, _rqs_forward_torch —
what ops.linear / ops.rqs_forward evaluate for a float64 call that needs gradients, because their adjoint kernels are float32).  The expressions
run on any device, so they are checked here: against the oracle, and against properties that do not share the oracle's formulas."""

import torch

from oracle import zuko_oracle as O


def _params(g, shape, K):
    return [torch.randn(*shape, k, generator=g, dtype=torch.float64).requires_grad_() for k in (K, K, K - 1)]


def test_float64_spline_expressions_match_the_oracle():
    """Values and gradients against the oracle's spline, with per-element and shared parameters, a bound and a slope that are not the defaults,
    and two inputs outside the support.  Float64 on both sides: 1e-12."""
    from zuko_amd import ops

    g = torch.Generator().manual_seed(9)
    for shape_x, shape_p in (((50, 6), (50, 6)), ((50, 6), (6,)), ((7, 50, 6), (50, 6))):
        leaves = _params(g, shape_p, 8)
        x = (torch.randn(*shape_x, generator=g, dtype=torch.float64) * 2.5).requires_grad_()
        x.data.view(-1)[:2] = torch.tensor([6.0, -7.0], dtype=torch.float64)
        y, l = ops._rqs_forward_torch(x, *leaves, 3.0, 1e-2, False)
        ry, rl = O.rqs_forward(*leaves, x, bound=3.0, slope=1e-2)
        assert (y - ry).abs().max().item() < 1e-12 and (l - rl).abs().max().item() < 1e-12
        mine = torch.autograd.grad(y.sum() + (2 * l).sum(), leaves + [x], retain_graph=True)
        ref = torch.autograd.grad(ry.sum() + (2 * rl).sum(), leaves + [x])
        assert all((a - b).abs().max().item() < 1e-12 for a, b in zip(mine, ref))
        assert torch.equal(ops._rqs_forward_torch(x, *leaves, 3.0, 1e-2, True)[1], l.sum(-1))


def test_float64_spline_is_a_monotone_bijection_whose_ladj_is_its_derivative():
    """Properties that do not depend on the oracle's formulas: ladj = log dy/dx as autograd differentiates y; y is increasing in x; the map fixes
    -bound and bound and is the identity with ladj 0 outside them; the float32 oracle of the reference's golden vectors is not involved."""
    from zuko_amd import ops

    g = torch.Generator().manual_seed(10)
    for K, bound in ((4, 5.0), (8, 3.0), (13, 1.5)):
        w, h, d = _params(g, (5,), K)
        x = torch.linspace(-1.2 * bound, 1.2 * bound, 4001, dtype=torch.float64)[:, None].expand(-1, 5).clone().requires_grad_()
        y, l = ops._rqs_forward_torch(x, w, h, d, bound, 1e-3, False)
        (dy,) = torch.autograd.grad(y.sum(), x, retain_graph=True)
        assert (dy.log() - l).abs().max().item() < 1e-10
        assert bool((y[1:] > y[:-1]).all())
        out = x.abs() > bound
        assert torch.equal(y[out], x[out]) and l[out].detach().abs().max().item() == 0.0
        edge = torch.tensor([[-bound] * 5, [bound] * 5], dtype=torch.float64)
        ye, _ = ops._rqs_forward_torch(edge * (1 - 1e-15), w, h, d, bound, 1e-3, False)
        assert (ye - edge).abs().max().item() < 1e-10


def test_float64_layer_expression_and_the_predicate():
    from zuko_amd import ops

    g = torch.Generator().manual_seed(11)
    x = torch.randn(5, 4, generator=g, dtype=torch.float64, requires_grad=True)
    w, b = torch.randn(3, 4, generator=g, dtype=torch.float64), torch.randn(3, generator=g, dtype=torch.float64)
    m = torch.rand(3, 4, generator=g) > 0.5
    assert torch.equal(ops._linear_torch(x, w, b, m, 1), torch.relu(x @ (w * m).T + b))
    assert torch.equal(ops._linear_torch(x, w, None, None, 0), x @ w.T)
    assert torch.equal(ops._linear_torch(x, w, b, None, 3), torch.tanh(x @ w.T + b))
    # the paths are taken for float64 operands under autograd only: float32 and no-grad calls keep their kernels
    assert ops._f64_grad(x, w) and not ops._f64_grad(x.float(), w.float()) and not ops._f64_grad(x.detach(), w)
    with torch.no_grad():
        assert not ops._f64_grad(x, w)
