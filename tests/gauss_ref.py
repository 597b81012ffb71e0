"""The Gaussianization map and flow of the reference, restated on torch ops (a helper of the tests, not a test).

`forward` / `inverse` are what `zuko.transforms.GaussianizationTransform(shift, scale)` evaluates (call_and_ladj with the derivative by autograd, the
bisection inverse): any dtype, CPU or device, differentiable by autograd.  tests/golden/make_golden_gf.py records the live reference on the fixtures
gauss_{a..f}.npz, and tests/test_gauss_host.py pins this module to them (float64 to 1e-12, float32 bitwise), so the GPU tests can compute their
references with it at test time.

`backward` is the closed-form adjoint the HIP kernel implements (include/zuko_amd.h: zk_gauss_backward); tests/test_gauss_host.py checks it against
autograd through `forward` in float64.  `gf_log_prob` evaluates a whole GF from its state_dict.
"""

from __future__ import annotations

import math

import torch

C = 1 - 1e-6


def f(x, shift, scale):
    """y = sqrt(2) erfinv(c mean_k erf((x exp(a_k) + b_k) / sqrt(2))); shift, scale [..., K]."""
    u = x[..., None] * torch.exp(scale) + shift
    u = torch.erf(u / math.sqrt(2))
    u = torch.mean(u, dim=-1) * C
    return torch.erfinv(u) * math.sqrt(2)


def forward(x, shift, scale):
    """(y, ladj = log dy/dx), the derivative by autograd as the reference takes it; the graph is kept when an input asks for gradients."""
    graph = torch.is_grad_enabled() and (x.requires_grad or shift.requires_grad or scale.requires_grad)
    with torch.enable_grad():
        xg = x.expand(torch.broadcast_shapes(x.shape, shift.shape[:-1])).clone().requires_grad_()
        y = f(xg, shift, scale)
    jac = torch.autograd.grad(y, xg, torch.ones_like(y), create_graph=graph)[0]
    return (y if graph else y.detach()), jac.log()


def inverse(y, shift, scale, bound: float = 10.0, eps: float = 1e-6):
    """n = ceil(log2(2 bound / eps)) bisection steps on [-bound, bound] (no gradients)."""
    with torch.no_grad():
        y = y.expand(torch.broadcast_shapes(y.shape, shift.shape[:-1]))
        a, b = torch.full_like(y, -bound), torch.full_like(y, bound)
        for _ in range(math.ceil(math.log2(2 * bound / eps))):
            mid = (a + b) / 2
            below = f(mid, shift, scale) < y
            a, b = torch.where(below, mid, a), torch.where(below, b, mid)
        return (a + b) / 2


def backward(x, shift, scale, gy, gl):
    """(gx, gb, ga): the gradients of (y * gy + ladj * gl).sum() in closed form; x [...], shift / scale [..., K] of the same batch shape."""
    K = shift.shape[-1]
    s = torch.exp(scale)
    xk = x[..., None]
    u = xk * s + shift
    y = f(x, shift, scale)[..., None]
    e = torch.exp(-u * u / 2)
    S = (s * e).sum(dim=-1, keepdim=True)
    w = C * e / (K * torch.exp(-y * y / 2))
    r = s * e / S
    fp = (w * s).sum(dim=-1, keepdim=True)
    gyk, glk = gy[..., None], gl[..., None]
    gx = gyk * fp + glk * (y * fp - (r * u * s).sum(dim=-1, keepdim=True))
    gb = gyk * w + glk * (y * w - r * u)
    ga = gyk * w * xk * s + glk * (y * w * xk * s + r * (1 - u * xk * s))
    return gx[..., 0], gb, ga


def gf_log_prob(sd: dict, x, c=None, trace: list | None = None):
    """log_prob of a GF from its state_dict (keys transform.transforms.{i}.{hyper.*|phi.*|A}, base.loc, base.scale): element-wise layers at the even
    positions (parameters from the ReLU MLP of the context, or the free [D, K] tensors), rotations at the odd ones, a diagonal normal base.
    `trace` collects the output of every element-wise layer."""
    layers = sorted({int(k.split(".")[2]) for k in sd if k.startswith("transform.transforms.")})
    ladj = 0.0
    for i in layers:
        pre = f"transform.transforms.{i}."
        if pre + "A" in sd:
            A = sd[pre + "A"]
            x = torch.einsum("...ij,...j->...i", torch.linalg.matrix_exp(A - A.mT), x)
            continue
        if pre + "phi.0" in sd:
            shift, scale = sd[pre + "phi.0"], sd[pre + "phi.1"]
        else:
            h = c
            idx = sorted({int(k[len(pre + "hyper.") :].split(".")[0]) for k in sd if k.startswith(pre + "hyper.")})
            for j in idx:
                h = torch.nn.functional.linear(h, sd[pre + f"hyper.{j}.weight"], sd[pre + f"hyper.{j}.bias"])
                if j != idx[-1]:
                    h = torch.relu(h)
            phi = h.unflatten(-1, (x.shape[-1], -1))
            shift, scale = phi.chunk(2, dim=-1)
        x, l = forward(x, shift, scale)
        ladj = ladj + l.sum(dim=-1)
        if trace is not None:
            trace.append(x.detach())
    loc, sc = sd["base.loc"], sd["base.scale"]
    return torch.distributions.Normal(loc, sc, validate_args=False).log_prob(x).sum(dim=-1) + ladj
