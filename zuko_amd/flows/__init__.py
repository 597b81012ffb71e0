r"""Flow factories of the hot path: MAF / NSF (autoregressive), NICE / RealNVP (coupling),
SOSPF / BPF (polynomial), NAF / UNAF (monotone networks), CNF (continuous), GF (Gaussianization); GMM is an alias of zuko_amd.mixtures.GMM, as in the reference.  Same constructor signatures and module trees as zuko.flows."""

from ..mixtures import GMM
from .autoregressive import MAF, MaskedAutoregressiveTransform
from .continuous import CNF, FFJTransform
from .coupling import NICE, GeneralCouplingTransform, RealNVP
from .elementwise import ElementWiseTransform
from .gaussianization import GF
from .neural import MNN, NAF, UMNN, UNAF
from .polynomial import BPF, SOSPF
from .spline import NCSF, NSF

__all__ = [
    "BPF",
    "CNF",
    "GF",
    "GMM",
    "MAF",
    "MNN",
    "NAF",
    "NCSF",
    "NICE",
    "NSF",
    "SOSPF",
    "UMNN",
    "UNAF",
    "ElementWiseTransform",
    "FFJTransform",
    "GeneralCouplingTransform",
    "MaskedAutoregressiveTransform",
    "RealNVP",
]
