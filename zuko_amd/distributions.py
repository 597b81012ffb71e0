r"""`NormalizingFlow` and `DiagNormal`: the caller of the transform hot path.

Mirrors zuko/distributions.py:39-138 and :337-363.  `log_prob` feeds z and the accumulated
log|det J| to one HIP kernel that evaluates the diagonal-normal log-density, reduces over features
and adds the ladj (zk_diag_normal_log_prob) when the base is a `DiagNormal` — or, when the last transform runs on an
operand-split static-shape autoregressive kernel, hands (loc, scale) to that transform's own launch, which then returns
the log-density and writes no z (ZUKO_AMD_NO_FUSED_BASE=1 keeps the separate launch).
"""

from __future__ import annotations

import os

import torch
from torch import Size, Tensor
from torch.distributions import Categorical, Distribution, Independent, MultivariateNormal, Normal, Transform, Uniform
from torch.distributions.utils import _sum_rightmost

from . import ops
from .transforms import ComposedTransform

__all__ = ["BoxUniform", "DiagNormal", "GaussianMixture", "NormalizingFlow"]

# the reference switches argument validation off globally (zuko/distributions.py:35-36); NaNs propagate
Distribution._validate_args = False
Distribution.arg_constraints = {}


class DiagNormal(Independent):
    """Independent(Normal(loc, scale), ndims)."""

    def __init__(self, loc: Tensor, scale: Tensor, ndims: int = 1) -> None:
        super().__init__(Normal(torch.as_tensor(loc), torch.as_tensor(scale)), ndims)

    def __repr__(self) -> str:
        return "Diag" + repr(self.base_dist)

    def expand(self, batch_shape: Size, new: Distribution | None = None) -> Distribution:
        new = self._get_checked_instance(DiagNormal, new)
        return super().expand(batch_shape, new)


class BoxUniform(Independent):
    """Independent(Uniform(lower, upper), ndims): the base of NCSF.  Mirrors zuko/distributions.py:366-396."""

    def __init__(self, lower: Tensor, upper: Tensor, ndims: int = 1) -> None:
        super().__init__(Uniform(torch.as_tensor(lower), torch.as_tensor(upper)), ndims)

    def __repr__(self) -> str:
        return "Box" + repr(self.base_dist)

    def expand(self, batch_shape: Size, new: Distribution | None = None) -> Distribution:
        new = self._get_checked_instance(BoxUniform, new)
        return super().expand(batch_shape, new)


class NormalizingFlow(Distribution):
    """p(X = x) = p(Z = f(x)) |det df/dx| for a transformation f and a base distribution p(Z)."""

    has_rsample = True

    def __init__(self, transform: Transform, base: Distribution) -> None:
        super().__init__()
        extra = transform.codomain.event_dim - len(base.event_shape)
        if extra > 0:
            base = Independent(base, extra)
        self.transform = transform
        self.base = base
        self.reinterpreted = max(-extra, 0)

    def __repr__(self) -> str:
        inner = f"(transform): {self.transform}\n(base): {self.base}".replace("\n", "\n  ")
        return f"{type(self).__name__}(\n  {inner}\n)"

    @property
    def batch_shape(self) -> Size:
        return self.base.batch_shape

    @property
    def event_shape(self) -> Size:
        return self.transform.inverse_shape(self.base.event_shape)

    def expand(self, batch_shape: Size, new: Distribution | None = None) -> Distribution:
        new = self._get_checked_instance(NormalizingFlow, new)
        new.transform = self.transform
        new.base = self.base.expand(batch_shape)
        new.reinterpreted = self.reinterpreted
        Distribution.__init__(new, validate_args=False)
        return new

    def _fusable_base(self):
        """(loc[D], scale[D]) if the base is a plain diagonal normal over the last axis."""
        b = self.base
        if isinstance(b, DiagNormal) and b.reinterpreted_batch_ndims == 1 and self.reinterpreted == 0:
            n = b.base_dist
            loc, scale = n.loc, n.scale
            D = loc.shape[-1]
            # an expanded base (context given) has stride-0 leading dims: take the underlying vector
            if loc.dim() > 1:
                if any(s != 0 for s in loc.stride()[:-1]) or any(s != 0 for s in scale.stride()[:-1]):
                    return None
                # (works for empty batch shapes too: view the last axis of the underlying vector)
                loc = loc.as_strided((D,), (loc.stride(-1),))
                scale = scale.as_strided((D,), (scale.stride(-1),))
            return loc, scale
        return None

    def log_prob(self, x: Tensor) -> Tensor:
        fused = self._fusable_base()
        if fused is not None and torch.is_grad_enabled() and (fused[0].requires_grad or fused[1].requires_grad):
            fused = None  # trainable base: its gradient flows through torch's Normal.log_prob, as in the reference
        if (fused is not None and isinstance(self.transform, ComposedTransform) and torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32
                and os.environ.get("ZUKO_AMD_NO_FUSED_BASE", "0") != "1"):
            # a last transform on an operand-split static-shape kernel adds the base's log-density in its own launch: T launches, no z
            z, ladj = self.transform.call_and_ladj(x, base=fused)
            if z is None:
                return ladj
        else:
            z, ladj = self.transform.call_and_ladj(x)
        ladj = _sum_rightmost(ladj, self.reinterpreted)
        if fused is not None and z.dtype != torch.float32 and torch.is_grad_enabled() and (z.requires_grad or (torch.is_tensor(ladj) and ladj.requires_grad)):
            fused = None  # the base's adjoint kernel is float32: a float64 call that needs gradients (a continuous flow trained in float64) takes torch's Normal
        if fused is not None and z.is_cuda and torch.is_tensor(ladj) and ladj.shape == z.shape[:-1]:
            return ops.diag_normal_log_prob(z, fused[0], fused[1], ladj)
        return self.base.log_prob(z) + ladj

    def rsample(self, shape: Size = ()) -> Tensor:
        z = self.base.rsample(shape) if self.base.has_rsample else self.base.sample(shape)
        return self.transform.inv(z)

    def rsample_and_log_prob(self, shape: Size = ()):
        z = self.base.rsample(shape) if self.base.has_rsample else self.base.sample(shape)
        x, ladj = self.transform.inv.call_and_ladj(z)
        ladj = _sum_rightmost(ladj, self.reinterpreted)
        return x, self.base.log_prob(z) - ladj


class GaussianMixture(Distribution):
    """p(X = x) = sum_k w_k N(x | loc_k, L_k L_k^T): what zuko.mixtures.GMM(...)(c) describes (a Mixture of a MultivariateNormal or DiagNormal),
    held as the packed parameter rows phi = logits | loc | diag [| tril] the model's MLP emits.  phi [total] is ONE mixture (the unconditional
    model); it stays one row under `expand`.  `log_prob` is ops.gmm_log_prob: one HIP launch that reads phi in place.  `sample` follows the
    reference on torch ops: every component is drawn, a Categorical index picks one."""

    has_rsample = False

    def __init__(self, phi: Tensor, features: int, components: int, covariance_type: str = "full", tied: bool = False, epsilon: float = 1e-6,
                 batch_shape: Size | None = None) -> None:
        total = sum(ops.gmm_sizes(features, components, covariance_type, tied))
        assert phi.shape[-1] == total, f"phi has {phi.shape[-1]} columns, expected {total}"
        self.phi, self.features, self.components = phi, features, components
        self.covariance_type, self.tied, self.epsilon = covariance_type, tied, epsilon
        super().__init__(batch_shape=Size(phi.shape[:-1] if batch_shape is None else batch_shape), event_shape=Size((features,)), validate_args=False)

    def __repr__(self) -> str:
        return f"{type(self).__name__}(components: {self.components}, features: {self.features}, covariance: {self.covariance_type}{', tied' if self.tied else ''})"

    def expand(self, batch_shape: Size, new: Distribution | None = None) -> Distribution:
        batch_shape = Size(batch_shape)
        phi = self.phi if self.phi.dim() == 1 or self.phi.shape[:-1] == batch_shape else self.phi.expand(batch_shape + self.phi.shape[-1:])
        return GaussianMixture(phi, self.features, self.components, self.covariance_type, self.tied, self.epsilon, batch_shape=batch_shape)

    def log_prob(self, x: Tensor) -> Tensor:
        lp = ops.gmm_log_prob(x, self.phi, self.components, self.covariance_type, self.tied, self.epsilon)
        shape = torch.broadcast_shapes(lp.shape, self.batch_shape)
        return lp if lp.shape == shape else lp.expand(shape)

    def _base(self) -> tuple[Distribution, Tensor]:
        """(the K component normals, batch shape self.batch_shape + (K,); the logits) as torch distributions."""
        D, K, lead = self.features, self.components, 1 if self.tied else self.components
        parts = self.phi.split(ops.gmm_sizes(D, K, self.covariance_type, self.tied), dim=-1)
        batch = self.phi.shape[:-1]
        loc = parts[1].reshape(*batch, K, D)
        scale = parts[2].reshape(*batch, lead, -1).exp() + self.epsilon
        if self.covariance_type == "full":
            factor = torch.diag_embed(scale)
            factor = factor.masked_scatter(torch.ones_like(factor, dtype=torch.bool).tril(-1), parts[3].reshape(*batch, lead, -1))
            base = MultivariateNormal(loc, scale_tril=factor, validate_args=False)
        else:
            base = DiagNormal(loc, scale.expand(loc.shape))
        return base.expand(self.batch_shape + (K,)), parts[0]

    def sample(self, shape: Size = ()) -> Tensor:
        shape = Size(shape)
        with torch.no_grad():
            base, logits = self._base()
            x = base.sample(shape)  # shape + batch + (K, D)
            i = Categorical(logits=logits).expand(self.batch_shape).sample(shape)  # shape + batch
            i = i[..., None, None].expand(*i.shape, 1, self.features)
            return x.gather(-2, i).squeeze(-2)
