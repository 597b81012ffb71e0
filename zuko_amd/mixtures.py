r"""Mixture models: `GMM`, the Gaussian mixture of zuko/mixtures.py — a conditional density estimator in its own right (mixture density
network) and a base distribution for `Flow`.

Constructor arguments, attribute names (`hyper` / `phi`, `shapes`, `total`), state_dict keys and initial values under a seed are the
reference's.  `forward(c)` returns a `zuko_amd.distributions.GaussianMixture` over the packed parameter rows: the MLP's output as is (no
unpacking, no [N, K, D, D] scale tensor), or the concatenated parameter list for the unconditional model; its `log_prob` and the gradients are
the HIP kernels of csrc/gmm.hip.  `initialize` (a one-off) runs on torch ops.
"""

from __future__ import annotations

from math import prod

import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Distribution

from . import ops
from .distributions import GaussianMixture
from .lazy import LazyDistribution
from .nn import MLP

__all__ = ["GMM"]


class GMM(LazyDistribution):
    r"""Gaussian mixture model p(X | c) = sum_k w_k(c) N(X | mu_k(c), Sigma_k(c)).

    Arguments:
        features: The number of features.
        context: The number of context features.
        components: The number of components K.
        covariance_type: "full", "diagonal" or "spherical".
        tied: Whether the components share one covariance.
        epsilon: Added to the diagonal of the scale factor.
        kwargs: Keyword arguments passed to `zuko_amd.nn.MLP`.
    """

    def __init__(self, features: int, context: int = 0, components: int = 2, covariance_type: str = "full", tied: bool = False,
                 epsilon: float = 1e-6, **kwargs) -> None:
        super().__init__()
        self.features = features
        self.components = components
        self.covariance_type = covariance_type
        self.tied = tied
        self.epsilon = epsilon
        sizes = ops.gmm_sizes(features, components, covariance_type, tied)
        lead = 1 if tied else components
        self.shapes = [(components,), (components, features)] + [(lead, n // lead) for n in sizes[2:]]
        self.total = sum(prod(s) for s in self.shapes)
        if context > 0:
            self.hyper = MLP(context, self.total, **kwargs)
        else:
            self.phi = nn.ParameterList(torch.randn(*s) for s in self.shapes)

    def forward(self, c: Tensor | None = None) -> Distribution:
        # (one differentiable cat of the parameter list: the kernel's gradient of the row flows back to every parameter)
        phi = torch.cat([p.flatten() for p in self.phi]) if c is None else self.hyper(c)
        return GaussianMixture(phi, self.features, self.components, self.covariance_type, self.tied, self.epsilon)

    @torch.no_grad()
    def initialize(self, x: Tensor, strategy: str) -> None:
        """Sets the components from samples x [N, D]: cluster centers by `strategy` ("random", "kmeans" or "kmeans++"), every sample assigned
        to its nearest center, then the clusters' frequencies, means and covariances.  A conditional model gets them as the bias of its last
        layer, whose weight is scaled by 1e-2."""
        N, D = x.shape
        K = self.components
        assert N > K, f"The number of samples ({N}) should be larger than the number of components ({K})."
        if strategy == "random":
            centers = _centers_random(x, K)
        elif strategy == "kmeans":
            centers = _centers_kmeans(x, K)
        elif strategy == "kmeans++":
            centers = _centers_kmeans_pp(x, K)
        else:
            raise NotImplementedError(f"Unknown clustering strategy '{strategy}'.")
        member = _membership(x, centers)  # [N, K] one-hot
        count = member.sum(dim=0)
        probs = count / count.sum()
        means = _cluster_sum(x, member) / count[:, None]
        var = _cluster_cov(x, member, diagonal=self.covariance_type != "full")  # [K, D, D] or [K, D]
        if self.tied:
            var = var.mean(dim=0, keepdim=True)
        if self.covariance_type == "full":
            factor = torch.linalg.cholesky(var)
            rows, cols = torch.tril_indices(D, D, offset=-1)
            cov = (factor.diagonal(dim1=-2, dim2=-1).log(), factor[..., rows, cols])
        elif self.covariance_type == "diagonal":
            cov = (var.log(),)
        else:
            cov = (var.mean(dim=-1, keepdim=True).log(),)
        params = (probs.log(), means, *cov)
        assert all(tuple(p.shape) == tuple(s) for p, s in zip(params, self.shapes)) and len(params) == len(self.shapes)
        if hasattr(self, "hyper"):
            self.hyper[-1].weight.mul_(1e-2)
            self.hyper[-1].bias.copy_(torch.cat([p.flatten() for p in params]))
        else:
            for p, value in zip(self.phi, params):
                p.copy_(value)


def _membership(x: Tensor, centers: Tensor) -> Tensor:
    nearest = torch.cdist(x, centers).argmin(dim=-1)
    return nn.functional.one_hot(nearest, num_classes=centers.shape[0]).to(x.dtype)


def _cluster_sum(x: Tensor, member: Tensor) -> Tensor:
    return (member[:, :, None] * x[:, None, :]).sum(dim=0)  # [K, D]


def _cluster_cov(x: Tensor, member: Tensor, diagonal: bool) -> Tensor:
    """Weighted (by membership) covariance of every cluster: [K, D, D], or its diagonal [K, D]."""
    out = []
    for k in range(member.shape[1]):
        if diagonal:
            out.append(torch.stack([torch.cov(x[:, d], aweights=member[:, k]) for d in range(x.shape[1])]))
        else:
            out.append(torch.cov(x.T, aweights=member[:, k]))
    return torch.stack(out)


def _draw(weights: Tensor, n: int) -> Tensor:
    return torch.multinomial(weights, n)


def _centers_random(x: Tensor, K: int) -> Tensor:
    return x[_draw(torch.ones(x.shape[0], device=x.device), K)]


def _centers_kmeans_pp(x: Tensor, K: int) -> Tensor:
    """k-means++ seeding: each further center is a sample drawn with probability proportional to its squared distance to the nearest center
    chosen so far (samples already chosen count as distance zero)."""
    N = x.shape[0]
    first = _draw(torch.ones(N, device=x.device), K)
    centers = x[first]
    taken = torch.zeros((N, K), dtype=torch.bool, device=x.device)
    taken[first, 0] = True
    for k in range(1, K):
        dist = torch.cdist(x, centers[:k])
        dist[taken[:, :k]] = 0
        nearest = dist.min(dim=-1).values
        pick = _draw(nearest.square(), 1)
        centers[k] = x[pick]
        taken[pick, k] = True
    return centers


def _centers_kmeans(x: Tensor, K: int, iterations: int = 7) -> Tensor:
    """Lloyd iterations from a k-means++ seeding; an empty cluster restarts at a random sample."""
    N = x.shape[0]
    centers = _centers_kmeans_pp(x, K)
    for _ in range(iterations):
        member = _membership(x, centers)
        count = member.sum(dim=0)[:, None]
        restart = x[_draw(torch.ones(N, device=x.device), K)]
        centers = torch.where(count > 0, _cluster_sum(x, member) / count, restart)
    return centers
