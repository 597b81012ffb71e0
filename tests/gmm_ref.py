"""The Gaussian mixture of the reference, restated on torch ops (a helper of the tests, not a test).

`log_prob` is what `zuko.mixtures.GMM(...)(c).log_prob(x)` evaluates when the model's MLP emits `phi`: any dtype, CPU or device, differentiable by
autograd.  tests/golden/make_golden_gmm.py records the live reference on the fixtures gmm_{a..f}.npz, and tests/test_gmm_host.py pins this module to
them (float64 to 1e-12, float32 bitwise), so the GPU tests can compute their references with it at test time.

`backward` is the closed-form adjoint the HIP kernel implements (include/zuko_amd.h: zk_gmm_backward), written out with explicit substitutions;
tests/test_gmm_host.py checks it against autograd through `log_prob` in float64.
"""

from __future__ import annotations

import math

import torch

COVARIANCES = ("full", "diagonal", "spherical")


def sizes(D: int, K: int, covariance_type: str, tied: bool) -> list[int]:
    lead = 1 if tied else K
    out = [K, K * D, lead * (1 if covariance_type == "spherical" else D)]
    if covariance_type == "full":
        out.append(lead * (D * (D - 1) // 2))
    return out


def total(D: int, K: int, covariance_type: str, tied: bool) -> int:
    return sum(sizes(D, K, covariance_type, tied))


def random_phi(N: int, D: int, K: int, covariance_type: str, tied: bool, generator=None, dtype=torch.float32):
    """Rows of well-conditioned parameters: logits ~ N(0, 1), loc ~ 2 N(0, 1), diag ~ 0.5 N(0, 1), tril ~ (0.5 / sqrt(D)) N(0, 1)."""
    scales = [1.0, 2.0, 0.5, 0.5 / math.sqrt(D)]
    parts = [s * torch.randn(N, n, generator=generator, dtype=dtype) for s, n in zip(scales, sizes(D, K, covariance_type, tied))]
    return torch.cat(parts, dim=-1)


def unpack(phi, D: int, K: int, covariance_type: str, tied: bool):
    """(logits [..., K], loc [..., K, D], diag [..., Lc, Dd], tril [..., Lc, T] | None)"""
    lead = 1 if tied else K
    parts = phi.split(sizes(D, K, covariance_type, tied), dim=-1)
    batch = phi.shape[:-1]
    tril = parts[3].reshape(*batch, lead, -1) if covariance_type == "full" else None
    return parts[0], parts[1].reshape(*batch, K, D), parts[2].reshape(*batch, lead, -1), tril


def log_prob(x, phi, D: int, K: int, covariance_type: str = "full", tied: bool = False, epsilon: float = 1e-6):
    logits, loc, diag, tril = unpack(phi, D, K, covariance_type, tied)
    scale = diag.exp() + epsilon
    xk = x.unsqueeze(-2)
    if covariance_type == "full":
        factor = torch.diag_embed(scale)
        factor = factor.masked_scatter(torch.ones_like(factor, dtype=torch.bool).tril(-1), tril)
        log_p = torch.distributions.MultivariateNormal(loc, scale_tril=factor, validate_args=False).log_prob(xk)
    else:
        log_p = torch.distributions.Normal(loc, scale, validate_args=False).log_prob(xk).sum(dim=-1)
    return torch.logsumexp(torch.log_softmax(logits, dim=-1) + log_p, dim=-1)


def backward(x, phi, g, D: int, K: int, covariance_type: str = "full", tied: bool = False, epsilon: float = 1e-6):
    """(gphi [N, total], gx [N, D]) of sum(g * log_prob(x, phi)) for x [N, D], phi [N, total], g [N], by the closed form."""
    N = x.shape[0]
    logits, loc, diag, tril = unpack(phi, D, K, covariance_type, tied)
    lead, Dd = diag.shape[-2], diag.shape[-1]
    rows, cols = torch.tril_indices(D, D, offset=-1)
    e = diag.exp()
    Ld = (e + epsilon).expand(N, lead, D)  # L_ii
    L = torch.diag_embed(Ld)
    if tril is not None:
        L[..., rows, cols] = tril
    L = L.expand(N, K, D, D)
    d = x[:, None, :] - loc
    z = torch.zeros_like(d)
    for i in range(D):  # forward substitution
        acc = torch.zeros_like(d[..., 0])
        for j in range(i):
            acc = acc + L[..., i, j] * z[..., j]
        z[..., i] = (d[..., i] - acc) / L[..., i, i]
    a = torch.zeros_like(d)
    for i in reversed(range(D)):  # back substitution with L^T
        acc = torch.zeros_like(d[..., 0])
        for j in range(i + 1, D):
            acc = acc + L[..., j, i] * a[..., j]
        a[..., i] = (z[..., i] - acc) / L[..., i, i]
    logn = -0.5 * (z * z).sum(-1) - Ld.log().sum(-1).expand(N, K) - 0.5 * D * math.log(2 * math.pi)
    w = torch.softmax(logits, dim=-1)
    r = torch.softmax(torch.log_softmax(logits, dim=-1) + logn, dim=-1)
    gr = (g[:, None] * r)[..., None]  # [N, K, 1]
    glogits = g[:, None] * (r - w)
    gloc = gr * a
    gx = -(gloc.sum(dim=1))
    gdiag = gr * (a * z - 1.0 / Ld.expand(N, K, D)) * e.expand(N, lead, D).expand(N, K, D)  # [N, K, D]
    if tied:
        gdiag = gdiag.sum(dim=1, keepdim=True)
    if Dd == 1:
        gdiag = gdiag.sum(dim=-1, keepdim=True)
    parts = [glogits, gloc.reshape(N, -1), gdiag.reshape(N, -1)]
    if tril is not None:
        gL = gr[..., None] * a[..., :, None] * z[..., None, :]  # [N, K, D, D]: (i, j) = a_i z_j
        gtril = gL[..., rows, cols]
        if tied:
            gtril = gtril.sum(dim=1, keepdim=True)
        parts.append(gtril.reshape(N, -1))
    return torch.cat(parts, dim=-1), gx
