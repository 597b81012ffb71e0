r"""Neural autoregressive flows (NAF, UNAF) and their monotone networks (MNN, UMNN).
Mirrors zuko/flows/neural.py:32-246 (constructor arguments, module tree, state_dict keys, initialisation order)."""

from __future__ import annotations

from typing import Any

import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Transform

from ..distributions import DiagNormal
from ..lazy import Flow, UnconditionalDistribution, UnconditionalTransform
from ..nn import MLP, MonotonicMLP
from ..transforms import MonotonicNetworkTransform, SoftclipTransform, UnconstrainedMonotonicNetworkTransform
from .autoregressive import MaskedAutoregressiveTransform

__all__ = ["MNN", "NAF", "UMNN", "UNAF"]


class MNN(nn.Module):
    r"""Monotone neural network: positive weights shared by all samples, modulated by a signal vector the conditioner emits per element.

    Arguments: signal (number of signal features), **kwargs for `zuko_amd.nn.MonotonicMLP` (hidden_features, stack, ...)."""

    per_feature = True  # its parameters are stacked over the features: the ordered inverse passes a sweep's feature selection along

    def __init__(self, signal: int = 16, **kwargs) -> None:
        super().__init__()
        self.network = MonotonicMLP(1 + signal, 1, **kwargs)

    def f(self, signal: Tensor, x: Tensor) -> Tensor:
        """The network in torch ops (zuko/flows/neural.py:56-60)."""
        from ..utils import broadcast

        return self.network(torch.cat(broadcast(x[..., None], signal, ignore=1), dim=-1)).squeeze(dim=-1)

    def forward(self, signal: Tensor, features=None) -> Transform:
        return MonotonicNetworkTransform(signal, self.network, features)


class UMNN(nn.Module):
    r"""Unconstrained monotone neural network: the integral of a positive integrand network whose weights are shared by all samples and which
    a signal vector the conditioner emits per element modulates; a constant the conditioner emits as well is added.

    Arguments: signal (number of signal features), **kwargs for `zuko_amd.nn.MLP` (hidden_features, stack, activation = nn.ELU, ...)."""

    per_feature = True  # its parameters are stacked over the features: the ordered inverse passes a sweep's feature selection along

    def __init__(self, signal: int = 16, **kwargs) -> None:
        super().__init__()
        kwargs.setdefault("activation", nn.ELU)
        self.integrand = MLP(1 + signal, 1, **kwargs)

    def g(self, signal: Tensor, x: Tensor) -> Tensor:
        """The integrand in torch ops (zuko/flows/neural.py:100-104): within [1e-3, 1e3]."""
        from ..utils import broadcast

        dx = self.integrand(torch.cat(broadcast(x[..., None], signal, ignore=1), dim=-1)).squeeze(dim=-1)
        return torch.exp(dx / (1 + abs(dx / 7)))

    def forward(self, signal: Tensor, constant: Tensor, features=None) -> Transform:
        return UnconstrainedMonotonicNetworkTransform(signal, constant, self.integrand, features)


class NAF(Flow):
    r"""Neural autoregressive flow: `transforms` autoregressive layers whose univariate map is a per-feature monotone network, a
    Softclip(bound=11) between consecutive layers, a standard-normal base.  Invertible for features within [-10, 10].

    Arguments (same as the reference): features, context, transforms, randperm, signal, network (kwargs for MNN), **kwargs for
    MaskedAutoregressiveTransform."""

    def __init__(self, features: int, context: int = 0, transforms: int = 3, randperm: bool = False, signal: int = 16, network: dict[str, Any] = {}, **kwargs) -> None:  # noqa: B006
        ascending = torch.arange(features)
        fixed = [ascending, torch.flipud(ascending)]
        layers: list = [
            MaskedAutoregressiveTransform(
                features=features,
                context=context,
                order=torch.randperm(features) if randperm else fixed[i % 2],
                univariate=MNN(signal=signal, stack=features, **network),
                shapes=[(signal,)],
                **kwargs,
            )
            for i in range(transforms)
        ]
        for i in range(len(layers) - 1, 0, -1):
            layers.insert(i, UnconditionalTransform(SoftclipTransform, bound=11.0))
        base = UnconditionalDistribution(DiagNormal, loc=torch.zeros(features), scale=torch.ones(features), buffer=True)
        super().__init__(layers, base)


class UNAF(Flow):
    r"""Unconstrained neural autoregressive flow: `transforms` autoregressive layers whose univariate map is the integral of a per-feature
    positive network (UMNN) plus a constant, a Softclip(bound=11) between consecutive layers, a standard-normal base.  Invertible for features
    within [-10, 10].

    Arguments (same as the reference): features, context, transforms, randperm, signal, network (kwargs for UMNN), **kwargs for
    MaskedAutoregressiveTransform."""

    def __init__(self, features: int, context: int = 0, transforms: int = 3, randperm: bool = False, signal: int = 16, network: dict[str, Any] = {}, **kwargs) -> None:  # noqa: B006
        ascending = torch.arange(features)
        fixed = [ascending, torch.flipud(ascending)]
        layers: list = [
            MaskedAutoregressiveTransform(
                features=features,
                context=context,
                order=torch.randperm(features) if randperm else fixed[i % 2],
                univariate=UMNN(signal=signal, stack=features, **network),
                shapes=[(signal,), ()],
                **kwargs,
            )
            for i in range(transforms)
        ]
        for i in range(len(layers) - 1, 0, -1):
            layers.insert(i, UnconditionalTransform(SoftclipTransform, bound=11.0))
        base = UnconditionalDistribution(DiagNormal, loc=torch.zeros(features), scale=torch.ones(features), buffer=True)
        super().__init__(layers, base)
