r"""Gaussianization flow (Meng et al., 2020): element-wise Gaussianization layers with trainable rotations between them.
Mirrors zuko/flows/gaussianization.py:97-155 (same module tree, state_dict keys and initial values under a seed).

Each element-wise layer is one launch of csrc/elementwise.hip's Gaussianization kernel (zuko_amd.transforms.GaussianizationTransform); the
rotations and the base density run on torch ops (zuko_amd.transforms.RotationTransform).  Without a context the parameters are [features,
components] tensors shared by all rows.  By default training expands them to one packed copy per row (zuko_amd/autograd.py: UnivariateFn) and
sums the [N, features, 2 components] gradient over the rows.  With zuko_amd.ops.GAUSS_SHARED_ADJOINT = True (off by default) it reads them in
place and sums the gradient inside the adjoint kernel (GaussSharedFn / GaussSharedInverseFn on zk_gauss_backward_shared; the calls it serves:
ops.gauss_shared_supported): no tensor of batch x features x components elements is created."""

from __future__ import annotations

import torch

from ..distributions import DiagNormal
from ..lazy import Flow, UnconditionalDistribution, UnconditionalTransform
from ..transforms import GaussianizationTransform, RotationTransform
from .elementwise import ElementWiseTransform

__all__ = ["GF"]


class GF(Flow):
    r"""Gaussianization flow.  Invertibility is only guaranteed for features within [-10, 10]: standardize the data.

    Arguments:
        features: The number of features.
        context: The number of context features.
        transforms: The number of element-wise transformations.
        components: The number of mixture components in each transformation.
        kwargs: Keyword arguments passed to :class:`ElementWiseTransform`.
    """

    def __init__(self, features: int, context: int = 0, transforms: int = 3, components: int = 8, **kwargs) -> None:
        layers = [
            ElementWiseTransform(features=features, context=context, univariate=GaussianizationTransform, shapes=[(components,), (components,)], **kwargs)
            for _ in range(transforms)
        ]
        for i in reversed(range(1, len(layers))):
            layers.insert(i, UnconditionalTransform(RotationTransform, A=torch.randn(features, features)))
        base = UnconditionalDistribution(DiagNormal, loc=torch.zeros(features), scale=torch.ones(features), buffer=True)
        super().__init__(layers, base)
