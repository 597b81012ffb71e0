r"""Continuous normalizing flow (CNF) and its lazy free-form Jacobian transformation.
Mirrors zuko/flows/continuous.py:23-152 (constructor arguments, module tree, state_dict keys, initialisation order)."""

from __future__ import annotations

from functools import partial
from math import pi

import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Transform

from ..distributions import DiagNormal
from ..lazy import Flow, LazyTransform, UnconditionalDistribution
from ..nn import MLP
from ..transforms import FreeFormJacobianTransform
from ..utils import broadcast

__all__ = ["CNF", "FFJTransform"]


class FFJTransform(LazyTransform):
    r"""Lazy free-form Jacobian transformation (FFJORD, Grathwohl et al., 2018): the flow of the ODE dx/dt = f(t, x | c) from t = 0 to 1, with
    f = MLP(cat(cos(k pi t), sin(k pi t), x, c)), k = 1..freqs.

    Arguments (same as the reference): features, context, freqs (time-embedding frequencies), atol, rtol (integration tolerances), exact (the exact
    trace of the Jacobian, or Hutchinson's stochastic estimate), **kwargs for `zuko_amd.nn.MLP` (hidden_features, activation = nn.ELU, ...).

    Without gradients, in float32 and with `exact=True`, a field inside the envelope of `zuko_amd.ops.cnf_supported` is integrated by the fused
    step kernel (csrc/cnf.hip); everything else — training, float64, exact=False, other activations or shapes — runs in torch ops.  With
    `zuko_amd.ops.CNF_ADJOINT = True` (off by default) training on a field of widths up to 64 runs on the kernels too (csrc/cnf_backward.hip), and
    with `zuko_amd.ops.CNF_HUTCHINSON = True` (off by default) so does `exact=False`, forward and — with both switches — training: one tangent
    along the probe per stage instead of `features`."""

    def __init__(self, features: int, context: int = 0, freqs: int = 3, atol: float = 1e-6, rtol: float = 1e-5, exact: bool = True, **kwargs) -> None:
        super().__init__()
        kwargs.setdefault("activation", nn.ELU)
        self.ode = MLP(features + context + 2 * freqs, features, **kwargs)
        self.register_buffer("times", torch.tensor((0.0, 1.0)))
        self.register_buffer("freqs", torch.arange(1, freqs + 1) * pi)
        self.atol = atol
        self.rtol = rtol
        self.exact = exact

    def f(self, t: Tensor, x: Tensor, c: Tensor | None = None) -> Tensor:
        """The field in plain torch ops, module by module — not through `MLP.forward`, whose gradient-mode route runs on once-differentiable HIP
        adjoints: the exact trace differentiates this function, and training differentiates that trace again."""
        t = self.freqs * t[..., None]
        t = torch.cat((t.cos(), t.sin()), dim=-1)
        h = torch.cat(broadcast(t, x, ignore=1) if c is None else broadcast(t, x, c, ignore=1), dim=-1)
        for m in self.ode:
            h = nn.functional.linear(h, m.weight, m.bias) if hasattr(m, "weight") else m(h)
        return h

    def forward(self, c: Tensor | None = None) -> Transform:
        if self.training:
            phi = self.parameters() if c is None else (c, *self.parameters())
        else:
            phi = () if c is None else (c,)
        return FreeFormJacobianTransform(f=partial(self.f, c=c), t0=self.times[0], t1=self.times[1], phi=phi, atol=self.atol, rtol=self.rtol,
                                         exact=self.exact, kernel=(self, c))


class CNF(Flow):
    r"""Continuous normalizing flow: one free-form Jacobian transformation and a standard-normal base.

    Arguments (same as the reference): features, context, **kwargs for `FFJTransform`."""

    def __init__(self, features: int, context: int = 0, **kwargs) -> None:
        transform = FFJTransform(features=features, context=context, **kwargs)
        base = UnconditionalDistribution(DiagNormal, loc=torch.zeros(features), scale=torch.ones(features), buffer=True)
        super().__init__(transform, base)
