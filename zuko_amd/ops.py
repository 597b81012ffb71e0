r"""Tensor-level wrappers around the C-ABI.  PyTorch is used for device memory, streams and
shape bookkeeping only; every arithmetic result comes out of a HIP kernel in libzuko_amd.so.

All functions require tensors on a HIP device (`tensor.is_cuda`) in float32 or float64 and raise
otherwise — there is no CPU or eager-PyTorch fallback.  One documented exception: the monotone networks of a neural autoregressive
flow (mnn_forward / mnn_inverse) run as torch ops ON THE DEVICE for network shapes their kernels do not serve, for float64, for the gradient of the
bisection inverse and, under autograd, for layers wider than 64 (the adjoint kernel's envelope: mnn_backward_supported).  Likewise the Gaussian mixture density (gmm_log_prob) runs the reference's expressions as torch ops
ON THE DEVICE outside its kernels' envelope (features or components above 64, sample dimensions broadcast over a batch of mixtures).  And the
continuous flow (cnf_integrate) hands every call its step kernel does not serve — gradients (CNF_ADJOINT off), float64, Hutchinson's estimator (CNF_HUTCHINSON
off), other activations or shapes — to zuko_amd.utils.odeint, the reference's adaptive integration in torch ops.  The Gaussianization map (gauss_forward / gauss_inverse) runs the
reference's expressions as torch ops ON THE DEVICE for more than 64 components (32 with gradients), for float64 calls that need gradients and under
GAUSS_KERNEL = False.  The conditioner layer (linear) and the rational-quadratic spline (rqs_forward) evaluate the reference's expressions as torch ops ON THE DEVICE for
float64 calls that need gradients (their adjoint kernels are float32): a float64 coupling or autoregressive spline flow trains layer by layer on them.
"""

from __future__ import annotations

import ctypes
import math
from functools import lru_cache

import numpy as np
import torch
from torch import Tensor

from . import _C

ACTIVATIONS = {
    None: 0,
    torch.nn.Identity: 0,
    torch.nn.ReLU: 1,
    torch.nn.ELU: 2,
    torch.nn.Tanh: 3,
    torch.nn.SiLU: 4,
    torch.nn.GELU: 5,
    torch.nn.Sigmoid: 6,
    torch.nn.LeakyReLU: 7,
}


def _dtype_code(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return 0
    if t.dtype == torch.float64:
        return 1
    if t.dtype == torch.bfloat16:
        return 2  # storage type only (spline kernels, zk_linear_bf16): arithmetic and ladj are fp32
    raise TypeError(f"zuko_amd kernels support float32/float64 (and bfloat16 storage for splines / linear layers), got {t.dtype}")


def _require_device(*ts: Tensor) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "zuko_amd: tensors must live on a HIP device (got a CPU tensor). "
                "This package has no CPU path; use the reference implementation for CPU work."
            )


def _bf16_trains_in_f32(fn):
    """bfloat16 operands under autograd.  The reference trains in whatever dtype the module is in (zuko tests/test_flows.py:17-29);
    the adjoint kernels here are float32, so a call that needs gradients runs on float32 copies of its bf16 operands (`.float()`
    is differentiable: gradients reach bf16 leaves through the casts, as torch.autocast would arrange it) and its transformed
    values (first result) are rounded back to bf16; log-determinants stay float32, as on the bf16 inference path."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        ts = [a for a in list(args) + list(kw.values()) if isinstance(a, Tensor)]
        if torch.is_grad_enabled() and any(t.dtype == torch.bfloat16 for t in ts) and any(t.requires_grad for t in ts):
            up = lambda a: a.float() if isinstance(a, Tensor) and a.dtype == torch.bfloat16 else a
            out = fn(*[up(a) for a in args], **{k: up(v) for k, v in kw.items()})
            if isinstance(out, tuple):
                return (out[0].to(torch.bfloat16),) + tuple(out[1:])
            return out.to(torch.bfloat16)
        return fn(*args, **kw)

    return wrapped


def _no_grad_only(*ts: Tensor) -> None:
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts):
        raise NotImplementedError(
            "zuko_amd: no backward kernel for this operation yet (autograd covers log_prob of affine / RQS "
            "flows, see zuko_amd/autograd.py); call it under torch.no_grad()."
        )


def _f64_grad(*ts) -> bool:
    """A call that needs gradients with a float64 operand: the adjoint kernels are float32, so it evaluates the reference's expressions as torch ops
    ON THE DEVICE in float64 (the base density and the Gaussianization map do the same; float32 stays on the kernels, bfloat16 on float32 copies)."""
    ts = [t for t in ts if isinstance(t, Tensor)]
    return torch.is_grad_enabled() and any(t.dtype == torch.float64 for t in ts) and any(t.requires_grad for t in ts)


_ACT_MODULE = {1: torch.nn.ReLU, 2: torch.nn.ELU, 3: torch.nn.Tanh, 4: torch.nn.SiLU, 5: torch.nn.GELU, 6: torch.nn.Sigmoid, 7: torch.nn.LeakyReLU}


def _linear_torch(x: Tensor, weight: Tensor, bias: Tensor | None, mask: Tensor | None, act: int) -> Tensor:
    """act(x @ (mask * weight).T + bias) as torch ops (zuko/nn.py:217-218)."""
    w = weight if mask is None else weight * mask.to(weight.dtype)
    y = torch.nn.functional.linear(x, w, bias)
    return y if act == 0 else _ACT_MODULE[act]()(y)


def _rqs_forward_torch(x: Tensor, widths: Tensor, heights: Tensor, derivatives: Tensor, bound: float, slope: float, reduce: bool):
    """(y, ladj) of the monotonic rational-quadratic spline as torch ops (zuko/transforms.py:469-490, 499-526, 554-567): soft clip, softmax, cumulative
    knots, strict-compare bin search, the rational-quadratic value and log-derivative; the identity outside [-bound, bound]."""
    ls = math.log(slope)
    K = widths.shape[-1]
    w = torch.softmax(widths / (1 + abs(2 * widths / ls)), dim=-1)
    h = torch.softmax(heights / (1 + abs(2 * heights / ls)), dim=-1)
    d = derivatives / (1 + abs(derivatives / ls))
    pad = torch.nn.functional.pad
    hor = bound * (2 * torch.cumsum(pad(w, (1, 0), value=0), dim=-1) - 1)
    ver = bound * (2 * torch.cumsum(pad(h, (1, 0), value=0), dim=-1) - 1)
    der = torch.exp(pad(d, (1, 1), value=0))
    k = torch.sum(hor < x[..., None], dim=-1) - 1
    inside = torch.logical_and(0 <= k, k < K)
    k = (k % K)[..., None]
    shape = torch.broadcast_shapes(k.shape[:-1], hor.shape[:-1])
    k = k.expand(shape + (1,))
    hor, ver, der = (t.expand(shape + (K + 1,)) for t in (hor, ver, der))
    x0, x1 = hor.gather(-1, k).squeeze(-1), hor.gather(-1, k + 1).squeeze(-1)
    y0, y1 = ver.gather(-1, k).squeeze(-1), ver.gather(-1, k + 1).squeeze(-1)
    d0, d1 = der.gather(-1, k).squeeze(-1), der.gather(-1, k + 1).squeeze(-1)
    s = (y1 - y0) / (x1 - x0)
    z = inside * (x - x0) / (x1 - x0)
    den = s + (d0 + d1 - 2 * s) * z * (1 - z)
    y = y0 + (y1 - y0) * (s * z**2 + d0 * z * (1 - z)) / den
    jac = s**2 * (2 * s * z * (1 - z) + d0 * (1 - z) ** 2 + d1 * z**2) / den**2
    y, ladj = torch.where(inside, y, x), inside * jac.log()
    return y, (ladj.sum(-1) if reduce else ladj)


def _stream() -> int:
    return _C.stream()


def _ptr(t: Tensor | None):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lead_collapse(t: Tensor) -> tuple[Tensor, int, int]:
    """View an expanded parameter tensor of shape (*lead, D, K) as strides (sN, sD) over a
    flattened leading index, copying only if the leading strides do not collapse."""
    if t.stride(-1) != 1 and t.shape[-1] != 1:
        t = t.contiguous()
    *lead, D, _ = t.shape
    sD = t.stride(-2) if D > 1 else 0
    dims = [(n, s) for n, s in zip(lead, t.stride()[: len(lead)]) if n > 1]
    if not dims:
        return t, 0, sD
    ok = True
    for (n0, s0), (n1, s1) in zip(dims[:-1], dims[1:]):
        if s0 != s1 * n1:
            ok = False
            break
    if ok:
        return t, dims[-1][1], sD
    t = t.contiguous()
    return t, t.stride(-3) if t.dim() >= 3 else 0, t.stride(-2) if D > 1 else 0


def _bshape(x: Tensor, *params: Tensor) -> torch.Size:
    """Broadcast of x against the parameters' batch shapes (everything but their last `k` dims)."""
    return torch.broadcast_shapes(x.shape, *[p for p in params])


class _Prepared:
    """x expanded to the broadcast shape as a contiguous [N, D] block + per-parameter strides."""

    def __init__(self, x: Tensor, params: list[tuple[Tensor, int]]):
        # params: (tensor, number of trailing "parameter" dims)
        _require_device(x, *[p for p, _ in params])
        _no_grad_only(x, *[p for p, _ in params])
        dt = x.dtype
        for p, _ in params:
            if p.dtype != dt or p.device != x.device:
                raise TypeError("zuko_amd: x and parameters must share dtype and device")
        batch = torch.broadcast_shapes(x.shape, *[p.shape[: p.dim() - k] for p, k in params])
        self.shape = batch
        if len(batch) == 0:
            shape2 = (1, 1)
        else:
            shape2 = (int(math.prod(batch[:-1])), int(batch[-1]))
        self.N, self.D = shape2
        self.x = x.expand(batch).contiguous()
        self.params = []
        for p, k in params:
            tail = p.shape[p.dim() - k :]
            flat = p.reshape(p.shape[: p.dim() - k] + (int(math.prod(tail)),)) if k != 1 else p
            pe = flat.expand(batch + flat.shape[-1:])
            if len(batch) == 0:
                pe = pe.reshape(1, 1, -1)
            elif len(batch) == 1:
                pe = pe.unsqueeze(0)
            t, sN, sD = _lead_collapse(pe)
            self.params.append((t, sN, sD))
        self.code = _dtype_code(x)

    def out(self) -> Tensor:
        return torch.empty(self.shape, dtype=self.x.dtype, device=self.x.device)

    def out_ladj(self, reduced: bool) -> Tensor:
        shape = self.shape[:-1] if reduced else self.shape
        dt = torch.float32 if self.x.dtype == torch.bfloat16 else self.x.dtype  # bf16 is a storage type: ladj stays fp32
        return torch.empty(shape, dtype=dt, device=self.x.device)


# ------------------------------------------------------------------------------------------------
# RQS
# ------------------------------------------------------------------------------------------------


def _packed_ok(x: Tensor, packed: Tensor | None, total: int) -> bool:
    return packed is not None and packed.dim() >= 2 and packed.shape[-1] == total and x.dim() >= 1 and tuple(torch.broadcast_shapes(x.shape, packed.shape[:-1])) == tuple(packed.shape[:-1])


@_bf16_trains_in_f32
def rqs_forward(x: Tensor, widths: Tensor, heights: Tensor, derivatives: Tensor, bound: float = 5.0, slope: float = 1e-3,
                reduce: bool = False, want_bins: bool = False, packed: Tensor | None = None):
    """(y, ladj[, k]) — see include/zuko_amd.h:zk_rqs_forward.  `packed`: the phi[..., D, 3K-1] tensor the three parameter
    views were cut from, when the caller has it (lets autograd differentiate phi itself instead of the three views)."""
    K = widths.shape[-1]
    if heights.shape[-1] != K or derivatives.shape[-1] != K - 1:
        raise ValueError("zuko_amd: widths/heights must have K entries and derivatives K-1")
    from . import autograd as AG

    if not want_bins and AG.needs_grad(x, widths, heights, derivatives):
        _require_device(x, widths, heights, derivatives)
        if _f64_grad(x, widths, heights, derivatives):
            return _rqs_forward_torch(x, widths, heights, derivatives, bound, slope, reduce)
        if K > 64:
            raise NotImplementedError("zuko_amd: spline backward is built for up to 64 bins")
        if _packed_ok(x, packed, 3 * K - 1):
            return AG.UnivariatePackedFn.apply((1, bound, slope, (K, K, K - 1), ()), reduce, x, packed)
        return AG.UnivariateFn.apply(1, bound, slope, reduce, x, widths, heights, derivatives)
    pr = _Prepared(x, [(widths, 1), (heights, 1), (derivatives, 1)])
    if reduce and len(pr.shape) == 0:
        raise ValueError("zuko_amd: cannot reduce ladj of a 0-d input")
    y, ladj = pr.out(), pr.out_ladj(reduce)
    bins = torch.empty(pr.shape, dtype=torch.int32, device=x.device) if want_bins else None
    (w, wn, wd), (h, hn, hd), (d, dn, dd) = pr.params
    err = _C.lib().zk_rqs_forward(pr.code, pr.N, pr.D, K, bound, slope, _ptr(pr.x), _ptr(w), wn, wd, _ptr(h), hn, hd, _ptr(d), dn, dd,
                                  _ptr(y), _ptr(ladj), int(reduce), _ptr(bins), _stream())
    _C.check(err, "zk_rqs_forward")
    return (y, ladj, bins) if want_bins else (y, ladj)


@_bf16_trains_in_f32
def rqs_inverse(y: Tensor, widths: Tensor, heights: Tensor, derivatives: Tensor, bound: float = 5.0, slope: float = 1e-3, want_bins: bool = False):
    K = widths.shape[-1]
    from . import autograd as AG

    if not want_bins and AG.needs_grad(y, widths, heights, derivatives):
        _require_device(y, widths, heights, derivatives)
        if K > 64:
            raise NotImplementedError("zuko_amd: spline backward is built for up to 64 bins")
        return AG.UnivariateInverseFn.apply(1, bound, slope, (), y, widths, heights, derivatives)
    pr = _Prepared(y, [(widths, 1), (heights, 1), (derivatives, 1)])
    x = pr.out()
    bins = torch.empty(pr.shape, dtype=torch.int32, device=y.device) if want_bins else None
    (w, wn, wd), (h, hn, hd), (d, dn, dd) = pr.params
    err = _C.lib().zk_rqs_inverse(pr.code, pr.N, pr.D, K, bound, slope, _ptr(pr.x), _ptr(w), wn, wd, _ptr(h), hn, hd, _ptr(d), dn, dd,
                                  _ptr(x), _ptr(bins), _stream())
    _C.check(err, "zk_rqs_inverse")
    return (x, bins) if want_bins else x


def rqs_diag(v: Tensor, widths: Tensor, heights: Tensor, derivatives: Tensor, bound: float = 5.0, slope: float = 1e-3, inverse: bool = False):
    """Diagnostic twin of rqs_forward / rqs_inverse (fp32): (out, ladj or None, k int32, knots [..., K+1]) where `knots`
    are the knots of the searched axis exactly as the product arithmetic compared them (zk_rqs_diag)."""
    K = widths.shape[-1]
    if v.dtype != torch.float32:
        raise TypeError("zuko_amd.rqs_diag: float32 only (the fp64 path searches IEEE knots: use rqs_forward(want_bins=True))")
    pr = _Prepared(v, [(widths, 1), (heights, 1), (derivatives, 1)])
    out = pr.out()
    ladj = None if inverse else pr.out_ladj(False)
    bins = torch.empty(pr.shape, dtype=torch.int32, device=v.device)
    knots = torch.empty(tuple(pr.shape) + (K + 1,), dtype=torch.float32, device=v.device)
    (w, wn, wd), (h, hn, hd), (d, dn, dd) = pr.params
    err = _C.lib().zk_rqs_diag(int(inverse), pr.N, pr.D, K, bound, slope, _ptr(pr.x), _ptr(w), wn, wd, _ptr(h), hn, hd, _ptr(d), dn, dd, _ptr(out), _ptr(ladj),
                               _ptr(bins), _ptr(knots), _stream())
    _C.check(err, "zk_rqs_diag")
    return out, ladj, bins, knots


def rqs_from_knots(v: Tensor, horizontal: Tensor, vertical: Tensor, slopes: Tensor, inverse: bool = False):
    """Test entry: evaluate from constrained knots; returns (out, ladj, k)."""
    K = horizontal.shape[-1] - 1
    pr = _Prepared(v, [(horizontal.contiguous(), 1), (vertical.contiguous(), 1), (slopes.contiguous(), 1)])
    out, ladj = pr.out(), pr.out_ladj(False)
    bins = torch.empty(pr.shape, dtype=torch.int32, device=v.device)
    (h, hn, hd), (ve, vn, vd), (s, sn, sd) = pr.params
    if (hn, hd) != (vn, vd) or (hn, hd) != (sn, sd):
        raise ValueError("zuko_amd: knots must share strides")
    err = _C.lib().zk_rqs_from_knots(pr.code, int(inverse), pr.N, pr.D, K, _ptr(pr.x), _ptr(h), _ptr(ve), _ptr(s), hn, hd, _ptr(out), _ptr(ladj),
                                     _ptr(bins), _stream())
    _C.check(err, "zk_rqs_from_knots")
    return out, ladj, bins


# ------------------------------------------------------------------------------------------------
# affine
# ------------------------------------------------------------------------------------------------


@_bf16_trains_in_f32
def affine_forward(x: Tensor, shift: Tensor, scale: Tensor, slope: float = 1e-3, reduce: bool = False, packed: Tensor | None = None):
    from . import autograd as AG

    if AG.needs_grad(x, shift, scale):
        _require_device(x, shift, scale)
        if _packed_ok(x, packed, 2):
            return AG.UnivariatePackedFn.apply((0, 5.0, slope, (1, 1), ()), reduce, x, packed)
        return AG.UnivariateFn.apply(0, 5.0, slope, reduce, x, shift, scale)
    pr = _Prepared(x, [(shift.unsqueeze(-1), 1), (scale.unsqueeze(-1), 1)])
    y, ladj = pr.out(), pr.out_ladj(reduce)
    (s, sn, sd), (c, cn, cd) = pr.params
    err = _C.lib().zk_affine_forward(pr.code, pr.N, pr.D, slope, _ptr(pr.x), _ptr(s), sn, sd, _ptr(c), cn, cd, _ptr(y), _ptr(ladj), int(reduce), _stream())
    _C.check(err, "zk_affine_forward")
    return y, ladj


@_bf16_trains_in_f32
def affine_inverse(y: Tensor, shift: Tensor, scale: Tensor, slope: float = 1e-3) -> Tensor:
    from . import autograd as AG

    if AG.needs_grad(y, shift, scale):
        _require_device(y, shift, scale)
        return AG.UnivariateInverseFn.apply(0, 5.0, slope, (), y, shift, scale)
    pr = _Prepared(y, [(shift.unsqueeze(-1), 1), (scale.unsqueeze(-1), 1)])
    x = pr.out()
    (s, sn, sd), (c, cn, cd) = pr.params
    err = _C.lib().zk_affine_inverse(pr.code, pr.N, pr.D, slope, _ptr(pr.x), _ptr(s), sn, sd, _ptr(c), cn, cd, _ptr(x), _stream())
    _C.check(err, "zk_affine_inverse")
    return x


# ------------------------------------------------------------------------------------------------
# SOS polynomial
# ------------------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def _leggauss01(n: int):
    """Gauss-Legendre nodes / weights mapped to [0, 1] (zuko/utils.py:328-347)."""
    nodes, weights = np.polynomial.legendre.leggauss(n)
    nodes = (nodes + 1) / 2
    weights = weights / 2
    return (ctypes.c_double * n)(*nodes.tolist()), (ctypes.c_double * n)(*weights.tolist())


SOS_BOUND = 10.0
SOS_EPS = 1e-6


@_bf16_trains_in_f32
def sos_forward(x: Tensor, a: Tensor, constant: Tensor | None = None, slope: float = 1e-3, reduce: bool = False):
    from . import autograd as AG

    if AG.needs_grad(x, a, constant):
        _require_device(x, a, constant)
        return AG.UnivariateFn.apply(2, SOS_BOUND, slope, reduce, x, a, constant)
    P, L1 = a.shape[-2:]
    plist = [(a, 2)] + ([(constant.unsqueeze(-1), 1)] if constant is not None else [])
    pr = _Prepared(x, plist)
    y, ladj = pr.out(), pr.out_ladj(reduce)
    nodes, weights = _leggauss01(L1)
    (at, an, ad) = pr.params[0]
    ct, cn, cd = pr.params[1] if constant is not None else (None, 0, 0)
    err = _C.lib().zk_sos_forward(pr.code, pr.N, pr.D, P, L1, slope, nodes, weights, _ptr(pr.x), _ptr(at), an, ad, _ptr(ct), cn, cd, _ptr(y), _ptr(ladj),
                                  int(reduce), _stream())
    _C.check(err, "zk_sos_forward")
    return y, ladj


@_bf16_trains_in_f32
def sos_inverse(y: Tensor, a: Tensor, constant: Tensor | None = None, slope: float = 1e-3) -> Tensor:
    from . import autograd as AG

    if AG.needs_grad(y, a, constant):
        _require_device(y, a, constant)
        return AG.UnivariateInverseFn.apply(2, SOS_BOUND, slope, (), y, a, constant)
    P, L1 = a.shape[-2:]
    plist = [(a, 2)] + ([(constant.unsqueeze(-1), 1)] if constant is not None else [])
    pr = _Prepared(y, plist)
    x = pr.out()
    nodes, weights = _leggauss01(L1)
    n_bisect = math.ceil(math.log2(2 * SOS_BOUND / SOS_EPS))  # transforms.py:615
    (at, an, ad) = pr.params[0]
    ct, cn, cd = pr.params[1] if constant is not None else (None, 0, 0)
    err = _C.lib().zk_sos_inverse(pr.code, pr.N, pr.D, P, L1, slope, nodes, weights, n_bisect, _ptr(pr.x), _ptr(at), an, ad, _ptr(ct), cn, cd, _ptr(x),
                                  _stream())
    _C.check(err, "zk_sos_inverse")
    return x


# ------------------------------------------------------------------------------------------------
# Bernstein polynomial
# ------------------------------------------------------------------------------------------------

BERN_EPS = 1e-6
BERN_NC_MAX = 72  # ZK_BERN_NCMAX of csrc/zk_univariate.h


@_bf16_trains_in_f32
def bernstein_forward(x: Tensor, theta: Tensor, bounded: bool, bound: float = 5.0, reduce: bool = False, eps: float = BERN_EPS):
    """`eps`: margin (in [0, 1] coordinates) beyond which the polynomial is continued linearly (zuko/transforms.py:594, :742-760)."""
    from . import autograd as AG

    if AG.needs_grad(x, theta):
        _require_device(x, theta)
        return AG.BernsteinFn.apply((bool(bounded), float(eps)), bound, reduce, x, theta)
    M = theta.shape[-1]
    pr = _Prepared(x, [(theta, 1)])
    y, ladj = pr.out(), pr.out_ladj(reduce)
    (t, tn, td) = pr.params[0]
    err = _C.lib().zk_bernstein_forward(pr.code, pr.N, pr.D, M, int(bounded), bound, float(eps), _ptr(pr.x), _ptr(t), tn, td, _ptr(y), _ptr(ladj), int(reduce), _stream())
    _C.check(err, "zk_bernstein_forward")
    return y, ladj


@_bf16_trains_in_f32
def bernstein_inverse(y: Tensor, theta: Tensor, bounded: bool, bound: float = 5.0, eps: float = BERN_EPS) -> Tensor:
    """Bisection on [-B, B] to the precision `eps` of the reference (n = ceil(log2(2B / eps)) steps, zuko/transforms.py:609-617)."""
    from . import autograd as AG

    if AG.needs_grad(y, theta):
        _require_device(y, theta)
        return AG.UnivariateInverseFn.apply(3, bound, 0.0, (bool(bounded), float(eps)), y, theta)
    M = theta.shape[-1]
    pr = _Prepared(y, [(theta, 1)])
    x = pr.out()
    n_bisect = math.ceil(math.log2(2 * bound / eps))  # transforms.py:615
    (t, tn, td) = pr.params[0]
    err = _C.lib().zk_bernstein_inverse(pr.code, pr.N, pr.D, M, int(bounded), bound, float(eps), n_bisect, _ptr(pr.x), _ptr(t), tn, td, _ptr(x), _stream())
    _C.check(err, "zk_bernstein_inverse")
    return x


# ------------------------------------------------------------------------------------------------
# conditioner layer, base density, reduction
# ------------------------------------------------------------------------------------------------


@_bf16_trains_in_f32
def linear(x: Tensor, weight: Tensor, bias: Tensor | None = None, mask: Tensor | None = None, act: int = 0) -> Tensor:
    """act(x @ (mask * weight).T + bias) over the last dim of x (zuko/nn.py:217-218)."""
    _require_device(x, weight, bias, mask)
    from . import autograd as AG

    if AG.needs_grad(x, weight, bias):
        if _f64_grad(x, weight, bias):
            return _linear_torch(x, weight, bias, mask, act)
        if act not in AG.BACKWARD_ACTS:
            raise NotImplementedError("zuko_amd: this activation cannot be fused when gradients are required")
        return AG.LinearFn.apply(x, weight, bias, mask, act)
    out_f, in_f = weight.shape
    if x.shape[-1] != in_f:
        raise ValueError(f"zuko_amd.linear: expected last dim {in_f}, got {x.shape[-1]}")
    if x.dtype == torch.bfloat16:
        w = weight if mask is None else weight * mask  # one pass over the parameters, not over the batch
        return linear_bf16(x, w, bias, None, act)
    x2 = x.reshape(-1, in_f)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    w = weight.contiguous()
    m = None
    if mask is not None:
        m = mask.contiguous()
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
        elif m.dtype != torch.uint8:
            raise TypeError("zuko_amd.linear: mask must be bool or uint8")
    b = None if bias is None else bias.contiguous()
    y = torch.empty((x2.shape[0], out_f), dtype=x.dtype, device=x.device)
    err = _C.lib().zk_linear(_dtype_code(x), x2.shape[0], in_f, out_f, _ptr(x2), x2.stride(0) if x2.shape[0] > 1 else in_f, _ptr(w), _ptr(m), _ptr(b), act,
                             _ptr(y), out_f, _stream())
    _C.check(err, "zk_linear")
    return y.reshape(x.shape[:-1] + (out_f,))


def linear_bf16(x: Tensor, weight_masked: Tensor, bias: Tensor | None, tile_live: Tensor | None, act: int = 0) -> Tensor:
    """bf16 act(x @ weight_masked.T + bias) with fp32 accumulation (zk_linear_bf16).  `tile_live`: int64
    [ceil(out/256)] bit masks (zuko_amd.nn.live_tile_masks), bit k clear where the 256 x 64 weight tile is entirely zero."""
    _require_device(x, weight_masked, bias, tile_live)
    _no_grad_only(x, weight_masked, bias)
    out_f, in_f = weight_masked.shape
    if x.dtype != torch.bfloat16 or weight_masked.dtype != torch.bfloat16 or (bias is not None and bias.dtype != torch.bfloat16):
        raise TypeError("zuko_amd.linear_bf16: x, weight and bias must be bfloat16")
    if in_f % 64 != 0:
        raise ValueError(f"zuko_amd.linear_bf16: in_features must be a multiple of 64 (got {in_f}); pad the conditioner input")
    if tile_live is not None and (tile_live.dtype != torch.int64 or tile_live.numel() != -(-out_f // 256) or in_f > 4096):
        raise ValueError("zuko_amd.linear_bf16: tile_live must be int64 [ceil(out / 256)] (and in_features <= 4096)")
    x2 = x.reshape(-1, in_f)
    if x2.stride(-1) != 1 or (x2.shape[0] > 1 and x2.stride(0) % 8 != 0) or x2.data_ptr() % 16 != 0:
        x2 = x2.contiguous()
    w = weight_masked.contiguous()
    b = None if bias is None else bias.contiguous()
    y = torch.empty((x2.shape[0], out_f), dtype=x.dtype, device=x.device)
    err = _C.lib().zk_linear_bf16(x2.shape[0], in_f, out_f, _ptr(x2), x2.stride(0) if x2.shape[0] > 1 else in_f, _ptr(w), _ptr(tile_live), _ptr(b), act,
                                  _ptr(y), out_f, _stream())
    _C.check(err, "zk_linear_bf16")
    return y.reshape(x.shape[:-1] + (out_f,))


def linear_bf16_rqs(h: Tensor, weight_panels: Tensor, bias_panels: Tensor | None, tile_live: Tensor | None, x: Tensor, K: int, bound: float = 5.0,
                    slope: float = 1e-3, lanes: bool = False):
    """(y bf16 [N, D], ladj fp32 [N]) of a bf16 autoregressive spline layer whose last conditioner layer and spline run
    in one kernel: h [N, in] last hidden activation, x [N, D] transform input, weights in feature panels — of 256 rows
    (zuko_amd.nn._Bf16Plan.spline_panels, zk_linear_bf16_rqs) or, with lanes=True, of 192 rows in the lane-owned order
    (spline_lane_panels, zk_linear_bf16_rqs_lanes)."""
    _require_device(h, weight_panels, bias_panels, tile_live, x)
    _no_grad_only(h, weight_panels, bias_panels, x)
    rows, in_f = weight_panels.shape
    panels = rows // (192 if lanes else 256)
    N, D = x.shape
    if h.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or weight_panels.dtype != torch.bfloat16:
        raise TypeError("zuko_amd.linear_bf16_rqs: bfloat16 tensors expected")
    h2 = h if (h.stride(-1) == 1 and h.stride(0) % 8 == 0 and h.data_ptr() % 16 == 0) else h.contiguous()
    x2 = x if x.stride(-1) == 1 else x.contiguous()
    y = torch.empty((N, D), dtype=torch.bfloat16, device=x.device)
    ladj = torch.empty(N, dtype=torch.float32, device=x.device)
    partial = torch.empty((2 * panels if lanes else panels, N), dtype=torch.float32, device=x.device)
    fn = _C.lib().zk_linear_bf16_rqs_lanes if lanes else _C.lib().zk_linear_bf16_rqs
    err = fn(N, in_f, panels, _ptr(h2), h2.stride(0) if N > 1 else in_f, _ptr(weight_panels), _ptr(tile_live), _ptr(bias_panels), K, D,
             bound, slope, _ptr(x2), x2.stride(0) if N > 1 else D, _ptr(y), D, _ptr(partial), _ptr(ladj), _stream())
    _C.check(err, "zk_linear_bf16_rqs_lanes" if lanes else "zk_linear_bf16_rqs")
    return y, ladj


def diag_normal_log_prob(z: Tensor, loc: Tensor, scale: Tensor, ladj: Tensor | None = None) -> Tensor:
    _require_device(z, loc, scale, ladj)
    from . import autograd as AG

    if AG.needs_grad(z, ladj):
        if z.dtype == torch.bfloat16:  # (bf16 module under autograd: float32 copies, gradients flow back through the casts)
            z, loc, scale = z.float(), loc.float(), scale.float()
            ladj = None if ladj is None else ladj.float()
        return AG.DiagNormalLogProbFn.apply(z, loc, scale, ladj)
    if z.dtype == torch.bfloat16:  # bf16 is a storage type here: the density is evaluated and returned in fp32
        z, loc, scale = z.float(), loc.float(), scale.float()
        ladj = None if ladj is None else ladj.float()
    D = z.shape[-1]
    z2 = z.reshape(-1, D).contiguous()
    out = torch.empty(z2.shape[0], dtype=z.dtype, device=z.device)
    la = None if ladj is None else ladj.expand(z.shape[:-1]).reshape(-1).contiguous()
    err = _C.lib().zk_diag_normal_log_prob(_dtype_code(z), z2.shape[0], D, _ptr(z2), _ptr(loc.contiguous()), _ptr(scale.contiguous()), _ptr(la), _ptr(out), _stream())
    _C.check(err, "zk_diag_normal_log_prob")
    return out.reshape(z.shape[:-1])


def sum_f64(v: Tensor, scale: float = 1.0) -> Tensor:
    """scale * sum(v) accumulated in float64; returns a 0-d float64 device tensor."""
    _require_device(v)
    v1 = v.reshape(-1).contiguous()
    ws = torch.empty(1024, dtype=torch.float64, device=v.device)
    out = torch.empty((), dtype=torch.float64, device=v.device)
    err = _C.lib().zk_sum_f64(_dtype_code(v), v1.numel(), _ptr(v1), scale, _ptr(ws), _ptr(out), _stream())
    _C.check(err, "zk_sum_f64")
    return out


# ------------------------------------------------------------------------------------------------
# monotone neural network (NAF): zk_mnn_forward / zk_mnn_inverse, torch ops when the kernel does not serve the call
# ------------------------------------------------------------------------------------------------

MNN_BOUND = 10.0
MNN_EPS = 1e-6
MNN_KERNEL = True  # False: every call takes the torch-op path (scripts/bench_naf.py measures the kernels against it)
MNN_ADJOINT = True  # False: calls that need gradients take the torch-op path (double backward through ATen), as before zk_mnn_backward existed


def mnn_supported(S: int, widths) -> bool:
    """True when zk_mnn_forward / zk_mnn_inverse serve per-feature networks (1 + S) -> widths -> 1: 1 <= S <= 63, one to three hidden
    layers, every width a multiple of 16 and <= 128, and a weight image of at most 128 KiB (zuko_amd/mnn_plan.py: layout)."""
    from . import mnn_plan

    return mnn_plan.supported(int(S), tuple(widths))


def mnn_backward_supported(S: int, widths) -> bool:
    """True when zk_mnn_backward serves per-feature networks (1 + S) -> widths -> 1: the shapes of mnn_supported whose widths are all <= 64
    (zuko_amd/mnn_plan.py: layout_backward).  Wider layers keep the torch-op path under autograd."""
    from . import mnn_plan

    return mnn_plan.layout_backward(int(S), tuple(widths)) is not None


def _mnn_feat(network, feat, device):
    """int32 device vector of the selected features (None = all, in order); `feat` is None, a (lo, hi) run or an index tensor.  The range is checked
    here, on the host, where the indices originate (the kernel's own clamp is a memory guard).  Tables are cached per run, and per index tensor
    OBJECT: the entry holds the tensor, so neither its id nor its storage can be handed to another tensor while the entry lives, and its version.
    The price: up to 1024 index tensors and their device tables stay alive on the network until the cache is cleared (wholesale, when full, or
    by zuko_amd.invalidate), and the first use of an index tensor copies it to the host, which synchronises the stream — the sweep schedule of an
    autoregressive layer holds a handful of such tensors, made once."""
    if feat is None:
        return None
    stack = next(iter(network.parameters())).shape[0]
    cache = network.__dict__.setdefault("_mnn_feat_cache", {})
    if len(cache) > 1024:
        cache.clear()
    if isinstance(feat, tuple):
        lo, hi = int(feat[0]), int(feat[1])
        if not 0 <= lo < hi <= stack:
            raise IndexError(f"zuko_amd: monotone network: features [{lo}, {hi}) outside a stack of {stack} networks")
        key = (str(device), lo, hi)
        if key not in cache:
            cache[key] = torch.arange(lo, hi, dtype=torch.int32, device=device)
        return cache[key]
    key = (str(device), id(feat))
    entry = cache.get(key)
    if entry is None or entry[0] is not feat or entry[1] != feat._version:
        host = feat.detach().cpu()
        if host.numel() and not (0 <= int(host.min()) and int(host.max()) < stack):
            raise IndexError(f"zuko_amd: monotone network: feature indices outside a stack of {stack} networks")
        entry = (feat, feat._version, host.to(device=device, dtype=torch.int32).contiguous(), int(host.unique().numel()) == host.numel())
        cache[key] = entry
    return entry[2]


def _mnn_feat_distinct(network, feat, device) -> bool:
    """Does every feature appear at most once in `feat`?  (The adjoint kernel gives every parameter one writer.)  Answered from _mnn_feat's cache."""
    if feat is None or isinstance(feat, tuple):
        return True
    _mnn_feat(network, feat, device)
    return network.__dict__["_mnn_feat_cache"][(str(device), id(feat))][3]


def _mnn_torch_f(network, x: Tensor, signal: Tensor, feat, signed: bool = False) -> Tensor:
    """MNN.f (zuko/flows/neural.py:56-60) in torch ops, on the networks of the selected features; `signed`: the weights as they are (the
    integrand of a UMNN) instead of |W|."""
    sel = None
    if feat is not None:
        sel = torch.arange(feat[0], feat[1], device=x.device) if isinstance(feat, tuple) else feat.to(device=x.device, dtype=torch.long)
    xb, _ = torch.broadcast_tensors(x.unsqueeze(-1), signal[..., :1])
    h = torch.cat((xb, signal.expand(xb.shape[:-1] + signal.shape[-1:])), dim=-1)
    for m in network:
        if hasattr(m, "weight"):
            W, b = (m.weight if signed else m.weight.abs()), m.bias
            if sel is not None:
                W, b = W.index_select(0, sel), None if b is None else b.index_select(0, sel)
            h = torch.einsum("...ij,...j->...i", W, h)
            h = h if b is None else h + b
        else:
            h = m(h)
    return h.squeeze(-1)


def _mnn_kernel_serves(network, x: Tensor, signal: Tensor):
    """The network's weight image when the HIP kernels serve this call (fp32, supported shape, nothing asks for gradients), else None."""
    from . import mnn_plan

    params = list(network.parameters())
    if not MNN_KERNEL:
        return None
    if x.dtype != torch.float32 or signal.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
        return None
    if torch.is_grad_enabled() and (x.requires_grad or signal.requires_grad or any(p.requires_grad for p in params)):
        return None
    return mnn_plan.image_of(network, x.device)


def _mnn_prepare(x: Tensor, signal: Tensor):
    S = signal.shape[-1]
    xb, sb = torch.broadcast_tensors(x.unsqueeze(-1), signal[..., :1])
    xb, sb = xb.squeeze(-1), signal.expand(xb.shape[:-1] + (S,))  # ([..., D, 1] -> x [..., D], signal [..., D, S])
    shape = xb.shape
    D = shape[-1]
    x2, s2 = xb.reshape(-1, D), sb.reshape(-1, D * S)
    if x2.stride(-1) != 1 or (x2.shape[0] > 1 and x2.stride(0) < D):
        x2 = x2.contiguous()
    if s2.stride(-1) != 1 or (s2.shape[0] > 1 and s2.stride(0) < D * S):
        s2 = s2.contiguous()
    return shape, x2, s2


def _mnn_args(img, x2: Tensor, s2: Tensor, feat, out: Tensor, **extra):
    N, D = x2.shape
    lay = img.layout
    w = list(lay.widths) + [0, 0]
    return _C.args("zk_mnn_args_v1", S=lay.S, n_hidden=len(lay.widths), width0=w[0], width1=w[1], width2=w[2], n_features=img.features, image_floats=lay.total,
                   N=N, Dsel=D, ldx=x2.stride(0) if N > 1 else D, ld_signal=s2.stride(0) if N > 1 else D * lay.S, ldy=D, x=x2.data_ptr(), signal=s2.data_ptr(),
                   image=img.data.data_ptr(), feat=None if feat is None else feat.data_ptr(), y=out.data_ptr(), **extra)


def _mnn_check(network, x: Tensor, signal: Tensor, feat) -> None:
    _require_device(x, signal, *network.parameters())
    if x.dim() < 1 or signal.dim() < 2 or signal.shape[-2] != x.shape[-1]:
        raise ValueError(f"zuko_amd: monotone network: x [..., D] and signal [..., D, S] expected, got {tuple(x.shape)} and {tuple(signal.shape)}")
    n_sel = x.shape[-1]
    stack = next(iter(network.parameters())).shape[0]
    if (feat is None and n_sel != stack) or (isinstance(feat, tuple) and feat[1] - feat[0] != n_sel) or (isinstance(feat, Tensor) and feat.numel() != n_sel):
        raise ValueError(f"zuko_amd: monotone network: {n_sel} columns do not match the feature selection of a stack of {stack} networks")


def _mnn_launch_forward(img, network, x2: Tensor, s2: Tensor, feat, reduce: bool):
    N, D = x2.shape
    data = img.refresh(network)
    y = torch.empty((N, D), dtype=torch.float32, device=x2.device)
    ladj = torch.empty((N,) if reduce else (N, D), dtype=torch.float32, device=x2.device)
    work = torch.empty((N, D), dtype=torch.float32, device=x2.device) if reduce else None
    a = _mnn_args(img, x2, s2, _mnn_feat(network, feat, x2.device), y, ladj=ladj.data_ptr(), work=None if work is None else work.data_ptr(), ladj_reduced=int(reduce))
    _C.check(_C.lib().zk_mnn_forward(a, _stream()), "zk_mnn_forward")
    del data
    return y, ladj


def mnn_backward_launch(bimg, network, x2: Tensor, s2: Tensor, feat, gy, gl, flat, need_x: bool = True, need_signal: bool = True, need_params: bool = True):
    """zk_mnn_backward on prepared operands: x2 [N, D] and s2 [N, D S] (unit inner stride), gy [N, D] or None, gl [N, D] / [N] or None, `flat` the
    signed flat parameters (mnn_plan.flat_parameters order).  Returns (gx, gsignal, gparams), None where not asked for.  Launches on the current
    stream; nothing synchronises."""
    N, D = x2.shape
    lay, B = bimg.layout, bimg.backward
    dev = x2.device
    data = bimg.refresh(network)
    gx = torch.empty((N, D), dtype=torch.float32, device=dev) if need_x else None
    gs = torch.empty((N, D * lay.S), dtype=torch.float32, device=dev) if need_signal else None
    gp = torch.empty(bimg.flat_total, dtype=torch.float32, device=dev) if need_params else None
    work = None
    if need_params and N > 0:
        import ctypes

        rows, chunks = ctypes.c_int(0), ctypes.c_int(0)
        _C.check(_C.lib().zk_mnn_backward_geometry(N, D, ctypes.byref(rows), ctypes.byref(chunks)), "zk_mnn_backward_geometry")
        work = torch.empty(chunks.value * D * B.g_total, dtype=torch.float32, device=dev)
    w = list(lay.widths) + [0, 0]
    ft = _mnn_feat(network, feat, dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = _C.args("zk_mnn_bwd_args_v1", S=lay.S, n_hidden=len(lay.widths), width0=w[0], width1=w[1], width2=w[2], n_features=bimg.features, image_floats=B.total,
                grad_floats=B.g_total, gl_reduced=int(gl is not None and gl.dim() == 1), N=N, Dsel=D, ldx=x2.stride(0) if N > 1 else D,
                ld_signal=s2.stride(0) if N > 1 else D * lay.S, ld_gx=D, ld_gsignal=D * lay.S, flat_total=bimg.flat_total, flat_weights=bimg.flat_weights,
                x=x2.data_ptr(), signal=s2.data_ptr(), image=data.data_ptr(), feat=ptr(ft), gy=ptr(gy), gl=ptr(gl), params=ptr(flat) if need_params else None,
                grad_table=bimg.table.data_ptr() if need_params else None, gx=ptr(gx), gsignal=ptr(gs), gparams=ptr(gp), work=ptr(work))
    _C.check(_C.lib().zk_mnn_backward(a, _stream()), "zk_mnn_backward")
    del data
    return gx, gs, gp


class MnnForwardFn(torch.autograd.Function):
    """(y, ladj) of the monotone networks under autograd: zk_mnn_forward forward, ONE zk_mnn_backward call backward (the adjoint kernel and the
    chunk reduction), which recomputes the forward from x and the signal: nothing else is saved."""

    @staticmethod
    def forward(ctx, network, feat, reduce, n_lin, x2, s2, *params):
        from . import mnn_plan

        ctx.network, ctx.feat, ctx.n_lin = network, feat, n_lin
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x2, s2, *params)
        return _mnn_launch_forward(mnn_plan.image_of(network, x2.device), network, x2.detach(), s2.detach(), feat, reduce)

    @staticmethod
    @torch.autograd.function.once_differentiable  # raw-pointer HIP kernels on detached data: double backward (create_graph=True) must raise
    def backward(ctx, gy, gl):
        from . import mnn_plan

        x2, s2, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_p = any(need[6:])
        none = (None, None, None, None)
        if gy is None and gl is None:
            return none + (None,) * (2 + len(params))
        bimg = mnn_plan.backward_image_of(ctx.network, x2.device)
        flat = torch.cat([p.detach().reshape(-1) for p in params]) if need_p else None
        gx, gs, gp = mnn_backward_launch(bimg, ctx.network, x2, s2, ctx.feat, None if gy is None else gy.contiguous(), None if gl is None else gl.contiguous(), flat,
                                         need_x=need[4], need_signal=need[5], need_params=need_p)
        gparams = [None] * len(params)
        if need_p:
            o = 0
            for i, p in enumerate(params):
                gparams[i] = gp[o : o + p.numel()].view(p.shape) if need[6 + i] else None
                o += p.numel()
        return none + (gx, gs, *gparams)


def _mnn_adjoint_serves(network, x: Tensor, signal: Tensor, feat):
    """The dtype the adjoint path runs this call from (float32, or bfloat16 trained on float32 copies as _bf16_trains_in_f32 arranges it), or
    None: switches off, another dtype, a shape outside mnn_backward_supported, or a feature named twice."""
    from . import mnn_plan

    if not (MNN_KERNEL and MNN_ADJOINT):
        return None
    params = list(network.parameters())
    dt = x.dtype
    if dt not in (torch.float32, torch.bfloat16) or signal.dtype != dt or any(p.dtype != dt for p in params):
        return None
    if mnn_plan.backward_image_of(network, x.device) is None or not _mnn_feat_distinct(network, feat, x.device):
        return None
    return dt


def _mnn_forward_adjoint(x: Tensor, signal: Tensor, network, feat, reduce: bool, dt):
    from . import mnn_plan

    lins = mnn_plan._linears(network)
    params = [l.weight for l in lins] + [l.bias for l in lins]  # (the order of mnn_plan.flat_parameters)
    if dt == torch.bfloat16:
        x, signal, params = x.float(), signal.float(), [p.float() for p in params]
    shape, x2, s2 = _mnn_prepare(x, signal)  # (differentiable views: broadcast gradients are summed by autograd)
    y, ladj = MnnForwardFn.apply(network, feat, reduce, len(lins), x2, s2, *params)
    lshape = shape[:-1] if reduce else shape
    y = y if y.shape == shape else y.reshape(shape)  # (two-dimensional calls hand out the node's own outputs)
    return (y.to(dt) if dt != torch.float32 else y), (ladj if ladj.shape == lshape else ladj.reshape(lshape))


def mnn_forward(x: Tensor, signal: Tensor, network, feat=None, reduce: bool = False):
    """(y, ladj) of the per-feature monotone networks `network` (a stacked zuko_amd.nn.MonotonicMLP(1 + S, 1, ...)): x [..., D], signal
    [..., D, S]; column j uses the network of feature feat[j] (`feat`: None, a (lo, hi) run or an index tensor).  zk_mnn_forward when it
    serves the call, under autograd with zk_mnn_backward as its adjoint (MnnForwardFn: float32 and bfloat16, shapes of
    mnn_backward_supported); otherwise (unsupported shape, float64, MNN_ADJOINT = False) the reference's torch ops with torch.autograd.grad
    for the derivative (zuko/transforms.py:623-637), which can be differentiated twice."""
    _mnn_check(network, x, signal, feat)
    if torch.is_grad_enabled() and (x.requires_grad or signal.requires_grad or any(p.requires_grad for p in network.parameters())):
        dt = _mnn_adjoint_serves(network, x, signal, feat)
        if dt is not None:
            return _mnn_forward_adjoint(x, signal, network, feat, reduce, dt)
    img = _mnn_kernel_serves(network, x, signal)
    if img is None:
        create_graph = torch.is_grad_enabled() and (x.requires_grad or signal.requires_grad or any(p.requires_grad for p in network.parameters()))
        with torch.enable_grad():
            xg = x.clone().requires_grad_()
            y = _mnn_torch_f(network, xg, signal, feat)
        jac = torch.autograd.grad(y, xg, torch.ones_like(y), create_graph=create_graph)[0]
        if not create_graph:
            y = y.detach()
        ladj = jac.log()
        return y, (ladj.sum(dim=-1) if reduce else ladj)
    shape, x2, s2 = _mnn_prepare(x, signal)
    y, ladj = _mnn_launch_forward(img, network, x2, s2, feat, reduce)
    return y.reshape(shape), ladj.reshape(shape[:-1] if reduce else shape)


class _MnnBisection(torch.autograd.Function):
    """Bisection on [-bound, bound] in torch ops, gradients by implicit differentiation: dx = dy / f'(x), dphi = -f_phi(x) dy / f'(x)."""

    @staticmethod
    def forward(ctx, f, y, bound, n, *phi):
        lo, hi = torch.full_like(y, -bound), torch.full_like(y, bound)
        for _ in range(n):
            mid = (lo + hi) / 2
            below = f(mid) < y
            lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
        x = (lo + hi) / 2
        ctx.f = f
        ctx.save_for_backward(x, *phi)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x):
        x, *phi = ctx.saved_tensors
        with torch.enable_grad():
            x = x.detach().requires_grad_()
            y = ctx.f(x)
        jac = torch.autograd.grad(y, x, torch.ones_like(y), retain_graph=bool(phi))[0]
        grad_y = grad_x / jac
        grad_phi = torch.autograd.grad(y, phi, -grad_y) if phi else ()
        return (None, grad_y, None, None, *grad_phi)


def mnn_inverse(y: Tensor, signal: Tensor, network, feat=None, bound: float = MNN_BOUND, eps: float = MNN_EPS) -> Tensor:
    """x with f(x) = y by n = ceil(log2(2 bound / eps)) bisection steps on [-bound, bound] (zuko/transforms.py:609-617): zk_mnn_inverse,
    or the same loop in torch ops when the kernel does not serve the call (see mnn_forward)."""
    _mnn_check(network, y, signal, feat)
    n = math.ceil(math.log2(2 * bound / eps))
    img = _mnn_kernel_serves(network, y, signal)
    if img is None:
        phi = [p for p in (signal, *network.parameters()) if p.requires_grad] if torch.is_grad_enabled() else []
        return _MnnBisection.apply(lambda v: _mnn_torch_f(network, v, signal, feat), y, float(bound), n, *phi)
    shape, y2, s2 = _mnn_prepare(y, signal)
    data = img.refresh(network)
    x = torch.empty(y2.shape, dtype=torch.float32, device=y.device)
    a = _mnn_args(img, y2, s2, _mnn_feat(network, feat, y.device), x, n_bisect=n, bound=float(bound))
    _C.check(_C.lib().zk_mnn_inverse(a, _stream()), "zk_mnn_inverse")
    del data
    return x.reshape(shape)


# ------------------------------------------------------------------------------------------------
# Gaussianization (GF): zk_gauss_forward / zk_gauss_inverse / zk_gauss_backward, torch ops when the kernels do not serve the call
# ------------------------------------------------------------------------------------------------

GAUSS_KERNEL = True  # False: every call takes the torch-op path (scripts/bench_gf.py measures the kernels against it)
GAUSS_K_MAX = 64  # ZK_GAUSS_KMAX of csrc/zk_univariate.h
GAUSS_K_MAX_BWD = 32  # ZK_GAUSS_KMAX_BWD: the adjoint's LDS image
GAUSS_BOUND = 10.0
GAUSS_EPS = 1e-6


def gauss_supported(K: int, dtype=torch.float32, needs_grad: bool = False) -> bool:
    """Do the kernels serve K components in `dtype`?  Forward and inverse: float32 / float64, 1 <= K <= 64; with gradients: float32 (bfloat16
    trains on float32 copies), 1 <= K <= 32."""
    if needs_grad:
        return dtype in (torch.float32, torch.bfloat16) and 1 <= K <= GAUSS_K_MAX_BWD
    return dtype in (torch.float32, torch.float64) and 1 <= K <= GAUSS_K_MAX


GAUSS_SHARED_ADJOINT = False  # True: [D, K] parameters shared by all rows train on zk_gauss_backward_shared (autograd.GaussSharedFn) instead of an expanded [N, D, 2K] copy


def _gauss_shared_shapes(x: Tensor, shift: Tensor, scale: Tensor) -> bool:
    """The dtype and shape clauses of gauss_shared_supported (no device needed)."""
    return (x.dtype in (torch.float32, torch.bfloat16) and shift.dtype == x.dtype and scale.dtype == x.dtype and x.dim() >= 1 and shift.dim() == 2
            and tuple(scale.shape) == tuple(shift.shape) and shift.shape[0] == x.shape[-1] and 1 <= shift.shape[1] <= GAUSS_K_MAX_BWD)


def gauss_shared_supported(x: Tensor, shift: Tensor, scale: Tensor) -> bool:
    """Does zk_gauss_backward_shared serve this call?  Device tensors, float32 (bfloat16 trains on float32 copies), x [..., D] with at least one
    dimension, shift and scale exactly [D, K] (two-dimensional, no other broadcast), 1 <= K <= 32."""
    return x.is_cuda and shift.is_cuda and scale.is_cuda and _gauss_shared_shapes(x, shift, scale)


def gauss_shared_chunks(N: int, D: int, K: int) -> int:
    """Row chunks of zk_gauss_backward_shared's partition (one [D, 2K] partial each in its workspace); 0 for a shape it does not serve."""
    floats = _C.lib().zk_gauss_backward_shared_floats(int(N), int(D), int(K))
    return floats // (D * 2 * K) if floats > 0 else 0


def _gauss_route(x: Tensor, shift: Tensor, scale: Tensor, grad: bool, packed: Tensor | None = None) -> str:
    """The path of gauss_forward / gauss_inverse: "torch" (torch ops), "kernel" (no gradients), and under autograd "packed" (UnivariatePackedFn, forward
    only), "shared" (GaussSharedFn / GaussSharedInverseFn) or "rows" (UnivariateFn / UnivariateInverseFn on parameters expanded to every row)."""
    K = shift.shape[-1]
    if not (GAUSS_KERNEL and gauss_supported(K, x.dtype, grad)):
        return "torch"
    if not grad:
        return "kernel"
    if _packed_ok(x, packed, 2 * K):
        return "packed"
    return "shared" if GAUSS_SHARED_ADJOINT and gauss_shared_supported(x, shift, scale) else "rows"


def _gauss_torch_f(x: Tensor, shift: Tensor, scale: Tensor) -> Tensor:
    """The reference's expression tree (zuko/transforms.py:869-875)."""
    u = x[..., None] * torch.exp(scale) + shift
    return torch.erfinv(torch.erf(u / math.sqrt(2)).mean(dim=-1) * (1 - 1e-6)) * math.sqrt(2)


def _gauss_check(x: Tensor, shift: Tensor, scale: Tensor) -> int:
    _require_device(x, shift, scale)
    if shift.dim() < 1 or shift.shape[-1] != scale.shape[-1] or shift.shape[-1] < 1:
        raise ValueError(f"zuko_amd: gaussianization: shift [..., K] and scale [..., K] expected, got {tuple(shift.shape)} and {tuple(scale.shape)}")
    return shift.shape[-1]


@_bf16_trains_in_f32
def gauss_forward(x: Tensor, shift: Tensor, scale: Tensor, reduce: bool = False, packed: Tensor | None = None):
    """(y, ladj) of the Gaussianization map — see include/zuko_amd.h: zk_gauss_forward.  `packed`: the phi[..., D, 2K] = [shift | scale] tensor the
    two views were cut from, when the caller has it.  Outside the kernels' envelope (gauss_supported) and under GAUSS_KERNEL = False: the
    reference's torch ops on the device, the derivative by torch.autograd.grad (zuko/transforms.py:623-637)."""
    from . import autograd as AG

    K = _gauss_check(x, shift, scale)
    grad = AG.needs_grad(x, shift, scale)
    route = _gauss_route(x, shift, scale, grad, packed)
    if route == "torch":
        with torch.enable_grad():
            xg = x.expand(torch.broadcast_shapes(x.shape, shift.shape[:-1], scale.shape[:-1])).clone().requires_grad_()
            y = _gauss_torch_f(xg, shift, scale)
        jac = torch.autograd.grad(y, xg, torch.ones_like(y), create_graph=grad)[0]
        if not grad:
            y = y.detach()
        ladj = jac.log()
        return y, (ladj.sum(dim=-1) if reduce else ladj)
    if route == "packed":
        return AG.UnivariatePackedFn.apply((4, GAUSS_BOUND, 0.0, (K, K), ()), reduce, x, packed)
    if route == "shared":
        return AG.GaussSharedFn.apply(reduce, x, shift, scale)
    if route == "rows":
        return AG.UnivariateFn.apply(4, GAUSS_BOUND, 0.0, reduce, x, shift, scale)
    pr = _Prepared(x, [(shift, 1), (scale, 1)])
    if reduce and len(pr.shape) == 0:
        raise ValueError("zuko_amd: cannot reduce ladj of a 0-d input")
    y, ladj = pr.out(), pr.out_ladj(reduce)
    (b, bn, bd), (a, an, ad) = pr.params
    err = _C.lib().zk_gauss_forward(pr.code, pr.N, pr.D, K, _ptr(pr.x), _ptr(b), bn, bd, _ptr(a), an, ad, _ptr(y), _ptr(ladj), int(reduce), _stream())
    _C.check(err, "zk_gauss_forward")
    return y, ladj


@_bf16_trains_in_f32
def gauss_inverse(y: Tensor, shift: Tensor, scale: Tensor, bound: float = GAUSS_BOUND, eps: float = GAUSS_EPS) -> Tensor:
    """x with f(x) = y by n = ceil(log2(2 bound / eps)) bisection steps on [-bound, bound] (zuko/transforms.py:609-617): zk_gauss_inverse, its
    gradients by the inverse function theorem on the forward map's adjoint kernel; the same loop in torch ops where gauss_forward runs torch ops."""
    from . import autograd as AG

    K = _gauss_check(y, shift, scale)
    grad = AG.needs_grad(y, shift, scale)
    n = math.ceil(math.log2(2 * bound / eps))
    route = _gauss_route(y, shift, scale, grad)
    if route == "torch":
        phi = [p for p in (shift, scale) if p.requires_grad] if torch.is_grad_enabled() else []
        ye = y.expand(torch.broadcast_shapes(y.shape, shift.shape[:-1], scale.shape[:-1]))
        return _MnnBisection.apply(lambda v: _gauss_torch_f(v, shift, scale), ye, float(bound), n, *phi)
    if route == "shared":
        return AG.GaussSharedInverseFn.apply(float(bound), float(eps), y, shift, scale)
    if grad:
        return AG.UnivariateInverseFn.apply(4, float(bound), 0.0, (float(eps),), y, shift, scale)
    pr = _Prepared(y, [(shift, 1), (scale, 1)])
    x = pr.out()
    (b, bn, bd), (a, an, ad) = pr.params
    err = _C.lib().zk_gauss_inverse(pr.code, pr.N, pr.D, K, float(bound), n, _ptr(pr.x), _ptr(b), bn, bd, _ptr(a), an, ad, _ptr(x), _stream())
    _C.check(err, "zk_gauss_inverse")
    return x


# ------------------------------------------------------------------------------------------------
# unconstrained monotone neural network (UNAF): zk_umnn_forward / zk_umnn_inverse / zk_umnn_backward, torch ops when the kernels do not serve the call
# ------------------------------------------------------------------------------------------------

UMNN_KERNEL = True  # False: every call takes the torch-op path (scripts/bench_unaf.py measures the kernels against it)
UMNN_QUAD_MAX = 64  # UMNN_QUAD_MAX of csrc/umnn.hip
UMNN_ADJOINT = True  # False: calls that need gradients take the torch-op path (the quadrature re-run under autograd), as before zk_umnn_backward existed


def umnn_supported(S: int, widths) -> bool:
    """True when zk_umnn_forward / zk_umnn_inverse serve per-feature integrand networks (1 + S) -> widths -> 1: the limits of mnn_supported."""
    return mnn_supported(S, widths)


def umnn_backward_supported(S: int, widths, n: int = 32) -> bool:
    """True when zk_umnn_backward serves per-feature integrand networks (1 + S) -> widths -> 1 with an n-point rule: the shapes of
    mnn_backward_supported (widths <= 64) whose backward image, transpose scratch and quadrature table fit the LDS limit, 1 <= n <= 64."""
    from . import mnn_plan

    B = mnn_plan.layout_backward(int(S), tuple(widths))
    if B is None or not 1 <= int(n) <= UMNN_QUAD_MAX:
        return False
    return 4 * (max(B.total, B.g_total) + mnn_plan.BWD_SCRATCH + 2 * UMNN_QUAD_MAX) <= mnn_plan.LDS_MAX


@lru_cache(maxsize=None)
def _umnn_rule(n: int):
    """(nodes, weights) of the n-point Gauss-Legendre rule on [0, 1] in float64 (zuko/utils.py:328-347)."""
    nodes, weights = np.polynomial.legendre.leggauss(int(n))
    return (nodes + 1) / 2, weights / 2


_UMNN_QUAD: dict = {}


def _umnn_quad(n: int, device) -> Tensor:
    """float32 device table [2 n] of zk_umnn_*: the nodes, then the weights, rounded from float64; cached per device."""
    key = (str(device), int(n))
    t = _UMNN_QUAD.get(key)
    if t is None:
        t = torch.from_numpy(np.concatenate(_umnn_rule(n)).astype(np.float32)).to(device)
        _UMNN_QUAD[key] = t
    return t


def _umnn_squash(h: Tensor) -> Tensor:
    return h / (1 + abs(h / 7))  # log g, within (-7, 7) (zuko/flows/neural.py:104)


def _umnn_torch_g(network, u: Tensor, signal: Tensor, feat) -> Tensor:
    """UMNN.g (zuko/flows/neural.py:100-104) in torch ops, on the networks of the selected features."""
    return torch.exp(_umnn_squash(_mnn_torch_f(network, u, signal, feat, signed=True)))


def _umnn_quadrature(g, x: Tensor, n: int) -> Tensor:
    """x sum_i w_i g(t_i x) (GaussLegendre.quadrature over [0, x], zuko/utils.py:349-363; its lerp(0, x, t_i) is t_i x up to rounding)."""
    nodes, weights = (torch.as_tensor(v, dtype=x.dtype, device=x.device) for v in _umnn_rule(n))
    u = nodes.reshape((n,) + (1,) * x.dim()) * x
    return x * torch.tensordot(weights, g(u), dims=1)


class _UmnnGaussLegendre(torch.autograd.Function):
    """f(x) = int_0^x g with the reference's gradients (zuko/utils.py:282-326): g(x) grad w.r.t. the upper limit, and for the parameters the
    quadrature re-run under autograd."""

    @staticmethod
    def forward(ctx, g, x, n, *phi):
        ctx.g, ctx.n = g, n
        ctx.save_for_backward(x, *phi)
        return _umnn_quadrature(g, x, n)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_area):
        x, *phi = ctx.saved_tensors
        grad_x = ctx.g(x) * grad_area if ctx.needs_input_grad[1] else None
        grad_phi = ()
        if phi and any(ctx.needs_input_grad[3:]):
            with torch.enable_grad():
                area = _umnn_quadrature(ctx.g, x.detach(), ctx.n)
            grad_phi = torch.autograd.grad(area, phi, grad_area)
        return (None, grad_x, None, *(grad_phi or (None,) * len(phi)))


def _umnn_phi(network, signal: Tensor):
    return [p for p in (signal, *network.parameters()) if p.requires_grad] if torch.is_grad_enabled() else []


def _umnn_torch_f(network, signal: Tensor, feat, n: int):
    phi = _umnn_phi(network, signal)
    return lambda v: _UmnnGaussLegendre.apply(lambda u: _umnn_torch_g(network, u, signal, feat), v, n, *phi)


def _umnn_check(network, x: Tensor, signal: Tensor, constant, feat, n: int) -> None:
    _require_device(constant)
    _mnn_check(network, x, signal, feat)
    if constant is not None and (constant.dim() < 1 or constant.shape[-1] not in (1, x.shape[-1])):
        raise ValueError(f"zuko_amd: unconstrained monotone network: constant [..., D] expected next to x {tuple(x.shape)}, got {tuple(constant.shape)}")
    if int(n) < 1:
        raise ValueError(f"zuko_amd: unconstrained monotone network: a quadrature of {n} points")


def _umnn_kernel_serves(network, x: Tensor, signal: Tensor, constant, n: int):
    """The network's weight image when the HIP kernels serve this call (fp32, ELU networks of a supported shape, at most 64 quadrature points,
    nothing asks for gradients), else None."""
    from . import mnn_plan

    if not UMNN_KERNEL or n > UMNN_QUAD_MAX or not mnn_plan.is_signed(network):
        return None
    ts = [x, signal, *network.parameters()] + ([] if constant is None else [constant])
    if any(t.dtype != torch.float32 for t in ts):
        return None
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return None
    return mnn_plan.image_of(network, x.device)


def _umnn_prepare(x: Tensor, signal: Tensor, constant):
    """The operands as the kernel reads them, IN PLACE wherever their strides allow (the conditioner's packed phi [N, D, S + 1] is not copied to
    split it): shape, x [N, D], signal [N, D, S], constant [N, D] | None and the stride fields of the argument block."""
    S = signal.shape[-1]
    batch = torch.broadcast_shapes(x.shape[:-1], signal.shape[:-2], *(() if constant is None else (constant.shape[:-1],)))
    D = x.shape[-1]
    x2 = x.expand(batch + (D,)).reshape(-1, D)
    N = x2.shape[0]
    if x2.stride(1) != 1 or (N > 1 and x2.stride(0) < 1):
        x2 = x2.contiguous()
    s3 = signal.expand(batch + (D, S)).reshape(-1, D, S)
    if s3.stride(2) != 1 or (D > 1 and s3.stride(1) < S) or (N > 1 and s3.stride(0) < (D - 1) * s3.stride(1) + S):
        s3 = s3.contiguous()
    ld_col = s3.stride(1) if D > 1 else S
    strides = dict(ldx=x2.stride(0) if N > 1 else D, ld_signal=s3.stride(0) if N > 1 else (D - 1) * ld_col + S, ld_col=ld_col, ldy=D)
    c2 = None
    if constant is not None:
        c2 = constant.expand(batch + (D,)).reshape(-1, D)
        strides.update(ld_constant=c2.stride(0) if N > 1 else 0, ld_constant_col=c2.stride(1) if D > 1 else 0)
    return batch + (D,), x2, s3, c2, strides


def _umnn_args(img, n: int, x2: Tensor, s3: Tensor, c2, strides: dict, feat, out: Tensor, **extra):
    N, D = x2.shape
    lay = img.layout
    w = list(lay.widths) + [0, 0]
    return _C.args("zk_umnn_args_v1", S=lay.S, n_hidden=len(lay.widths), width0=w[0], width1=w[1], width2=w[2], n_features=img.features, image_floats=lay.total,
                   n_quad=n, N=N, Dsel=D, x=x2.data_ptr(), signal=s3.data_ptr(), constant=None if c2 is None else c2.data_ptr(), image=img.data.data_ptr(),
                   quad=_umnn_quad(n, x2.device).data_ptr(), feat=None if feat is None else feat.data_ptr(), y=out.data_ptr(), **strides, **extra)


def _umnn_launch_forward(img, network, n: int, x2: Tensor, s3: Tensor, c2, strides: dict, feat, reduce: bool):
    N, D = x2.shape
    data = img.refresh(network)
    y = torch.empty((N, D), dtype=torch.float32, device=x2.device)
    ladj = torch.empty((N,) if reduce else (N, D), dtype=torch.float32, device=x2.device)
    work = torch.empty((N, D), dtype=torch.float32, device=x2.device) if reduce else None
    a = _umnn_args(img, n, x2, s3, c2, strides, _mnn_feat(network, feat, x2.device), y, ladj=ladj.data_ptr(), work=None if work is None else work.data_ptr(),
                   ladj_reduced=int(reduce))
    _C.check(_C.lib().zk_umnn_forward(a, _stream()), "zk_umnn_forward")
    del data
    return y, ladj


def umnn_backward_launch(bimg, network, n: int, x2: Tensor, s3: Tensor, strides: dict, feat, gy, gl, need_x: bool = True, need_signal: bool = True,
                         need_params: bool = True):
    """zk_umnn_backward on prepared operands: x2 [N, D] and s3 [N, D, S] as _umnn_prepare hands them out with their `strides` (the signal is read in
    place), gy [N, D] or None, gl [N, D] / [N] or None (contiguous).  Returns (gx [N, D], gsignal [N, D S], gparams in mnn_plan.flat_parameters
    order), None where not asked for.  Launches on the current stream; nothing synchronises."""
    N, D = x2.shape
    lay, B = bimg.layout, bimg.backward
    dev = x2.device
    data = bimg.refresh(network)
    gx = torch.empty((N, D), dtype=torch.float32, device=dev) if need_x else None
    gs = torch.empty((N, D * lay.S), dtype=torch.float32, device=dev) if need_signal else None
    gp = torch.empty(bimg.flat_total, dtype=torch.float32, device=dev) if need_params else None
    work = None
    if need_params and N > 0:
        import ctypes

        rows, chunks = ctypes.c_int(0), ctypes.c_int(0)
        _C.check(_C.lib().zk_umnn_backward_geometry(N, D, ctypes.byref(rows), ctypes.byref(chunks)), "zk_umnn_backward_geometry")
        work = torch.empty(chunks.value * D * B.g_total, dtype=torch.float32, device=dev)
    w = list(lay.widths) + [0, 0]
    ft = _mnn_feat(network, feat, dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    a = _C.args("zk_umnn_bwd_args_v1", S=lay.S, n_hidden=len(lay.widths), width0=w[0], width1=w[1], width2=w[2], n_features=bimg.features, image_floats=B.total,
                grad_floats=B.g_total, gl_reduced=int(gl is not None and gl.dim() == 1), n_quad=n, N=N, Dsel=D, ldx=strides["ldx"], ld_signal=strides["ld_signal"],
                ld_col=strides["ld_col"], ld_gx=D, ld_gsignal=D * lay.S, flat_total=bimg.flat_total, flat_weights=bimg.flat_weights, x=x2.data_ptr(),
                signal=s3.data_ptr(), image=data.data_ptr(), quad=_umnn_quad(n, dev).data_ptr(), feat=ptr(ft), gy=ptr(gy), gl=ptr(gl),
                grad_table=bimg.table.data_ptr() if need_params else None, gx=ptr(gx), gsignal=ptr(gs), gparams=ptr(gp), work=ptr(work))
    _C.check(_C.lib().zk_umnn_backward(a, _stream()), "zk_umnn_backward")
    del data
    return gx, gs, gp


class UmnnForwardFn(torch.autograd.Function):
    """(y, ladj) of the unconstrained monotone networks under autograd: zk_umnn_forward forward, ONE zk_umnn_backward call backward (the adjoint
    kernel and the chunk reduction), which recomputes the forward from x and the signal: nothing else is saved.  The constant's gradient is gy."""

    @staticmethod
    def forward(ctx, network, feat, reduce, n, strides, x2, s3, c2, *params):
        from . import mnn_plan

        ctx.network, ctx.feat, ctx.n, ctx.strides = network, feat, n, strides
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x2, s3, *params)
        return _umnn_launch_forward(mnn_plan.image_of(network, x2.device), network, n, x2.detach(), s3.detach(), None if c2 is None else c2.detach(), strides, feat, reduce)

    @staticmethod
    @torch.autograd.function.once_differentiable  # raw-pointer HIP kernels on detached data: double backward (create_graph=True) must raise
    def backward(ctx, gy, gl):
        from . import mnn_plan

        x2, s3, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_p = any(need[8:])
        none = (None,) * 5
        if gy is None and gl is None:
            return none + (None,) * (3 + len(params))
        bimg = mnn_plan.backward_image_of(ctx.network, x2.device, signed=True)
        gy = None if gy is None else gy.contiguous()
        gx, gs, gp = umnn_backward_launch(bimg, ctx.network, ctx.n, x2, s3, ctx.strides, ctx.feat, gy, None if gl is None else gl.contiguous(),
                                          need_x=need[5], need_signal=need[6], need_params=need_p)
        gparams = [None] * len(params)
        if need_p:
            o = 0
            for i, p in enumerate(params):
                gparams[i] = gp[o : o + p.numel()].view(p.shape) if need[8 + i] else None
                o += p.numel()
        return none + (gx, None if gs is None else gs.view(s3.shape), gy if need[7] else None, *gparams)


def _umnn_adjoint_serves(network, x: Tensor, signal: Tensor, constant, feat, n: int):
    """The dtype the adjoint path runs this call from (float32, or bfloat16 trained on float32 copies), or None: nothing asks for gradients,
    switches off, another dtype, a network or rule outside umnn_backward_supported, or a feature named twice."""
    from . import mnn_plan

    if not (UMNN_KERNEL and UMNN_ADJOINT and torch.is_grad_enabled()) or n > UMNN_QUAD_MAX:
        return None
    ts = [x, signal, *network.parameters()] + ([] if constant is None else [constant])
    if not any(t.requires_grad for t in ts):
        return None
    dt = x.dtype
    if dt not in (torch.float32, torch.bfloat16) or any(t.dtype != dt for t in ts):
        return None
    bimg = mnn_plan.backward_image_of(network, x.device, signed=True)
    if bimg is None or not umnn_backward_supported(bimg.S, bimg.widths, n) or not _mnn_feat_distinct(network, feat, x.device):
        return None
    return dt


def _umnn_forward_adjoint(x: Tensor, signal: Tensor, constant, network, feat, reduce: bool, n: int, dt):
    from . import mnn_plan

    lins = mnn_plan._linears(network)
    params = [l.weight for l in lins] + [l.bias for l in lins]  # (the order of mnn_plan.flat_parameters)
    if dt == torch.bfloat16:
        x, signal, params = x.float(), signal.float(), [p.float() for p in params]
        constant = None if constant is None else constant.float()
    shape, x2, s3, c2, strides = _umnn_prepare(x, signal, constant)  # (differentiable views: broadcast gradients are summed by autograd)
    y, ladj = UmnnForwardFn.apply(network, feat, reduce, int(n), strides, x2, s3, c2, *params)
    lshape = shape[:-1] if reduce else shape
    y = y if y.shape == shape else y.reshape(shape)  # (two-dimensional calls hand out the node's own outputs)
    return (y.to(dt) if dt != torch.float32 else y), (ladj if ladj.shape == lshape else ladj.reshape(lshape))


def umnn_forward(x: Tensor, signal: Tensor, constant, network, feat=None, reduce: bool = False, n: int = 32):
    """(y, ladj) of the per-feature unconstrained monotone networks: y = x sum_i w_i g(t_i x) + constant over the n-point Gauss-Legendre rule,
    g = exp(squash(h)) with h = `network` (a stacked zuko_amd.nn.MLP(1 + S, 1, ...) with ELU), ladj = squash(h(x)) = log g(x).  x [..., D],
    signal [..., D, S], constant [..., D] | None; column j uses the network of feature feat[j] (`feat`: None, a (lo, hi) run or an index tensor).
    zk_umnn_forward when it serves the call, under autograd with zk_umnn_backward as its adjoint (UmnnForwardFn: float32 and bfloat16, shapes of
    umnn_backward_supported); otherwise (unsupported shape or activation, float64, UMNN_ADJOINT = False) the same expressions as torch ops
    with the reference's autograd semantics (zuko/utils.py:282-326)."""
    _umnn_check(network, x, signal, constant, feat, n)
    dt = _umnn_adjoint_serves(network, x, signal, constant, feat, n)
    if dt is not None:
        return _umnn_forward_adjoint(x, signal, constant, network, feat, reduce, n, dt)
    img = _umnn_kernel_serves(network, x, signal, constant, n)
    if img is None:
        y = _umnn_torch_f(network, signal, feat, n)(x)
        y = y if constant is None else y + constant
        ladj = _umnn_squash(_mnn_torch_f(network, x, signal, feat, signed=True)).expand(y.shape)
        return y, (ladj.sum(dim=-1) if reduce else ladj)
    shape, x2, s3, c2, strides = _umnn_prepare(x, signal, constant)
    y, ladj = _umnn_launch_forward(img, network, n, x2, s3, c2, strides, feat, reduce)
    return y.reshape(shape), ladj.reshape(shape[:-1] if reduce else shape)


def umnn_inverse(y: Tensor, signal: Tensor, constant, network, feat=None, bound: float = MNN_BOUND, eps: float = MNN_EPS, n: int = 32) -> Tensor:
    """x with f(x) + constant = y by ceil(log2(2 bound / eps)) bisection steps on [-bound, bound] (zuko/transforms.py:609-617): zk_umnn_inverse,
    or the same loop in torch ops when the kernel does not serve the call (see umnn_forward)."""
    _umnn_check(network, y, signal, constant, feat, n)
    steps = math.ceil(math.log2(2 * bound / eps))
    img = _umnn_kernel_serves(network, y, signal, constant, n)
    if img is None:
        target = y if constant is None else y - constant
        target = target.expand(torch.broadcast_shapes(target.shape, signal.shape[:-1]))
        return _MnnBisection.apply(_umnn_torch_f(network, signal, feat, n), target, float(bound), steps, *_umnn_phi(network, signal))
    shape, y2, s3, c2, strides = _umnn_prepare(y, signal, constant)
    data = img.refresh(network)
    x = torch.empty(y2.shape, dtype=torch.float32, device=y.device)
    a = _umnn_args(img, n, y2, s3, c2, strides, _mnn_feat(network, feat, y.device), x, n_bisect=steps, bound=float(bound))
    _C.check(_C.lib().zk_umnn_inverse(a, _stream()), "zk_umnn_inverse")
    del data
    return x.reshape(shape)


# ------------------------------------------------------------------------------------------------
# Gaussian mixture model: zk_gmm_log_prob / zk_gmm_backward, torch ops when the kernel does not serve the call
# ------------------------------------------------------------------------------------------------

GMM_KERNEL = True  # False: every call takes the torch-op path (scripts/bench_gmm.py measures the kernels against it; double backward needs it)
GMM_COVARIANCE = {"full": 0, "diagonal": 1, "spherical": 2}


def gmm_sizes(D: int, K: int, covariance_type: str, tied: bool) -> list[int]:
    """Lengths of the segments of one row of phi: logits | loc | diag [| tril] (include/zuko_amd.h: zk_gmm_args_v1)."""
    if covariance_type not in GMM_COVARIANCE:
        raise NotImplementedError(f"Unknown covariance type '{covariance_type}'.")
    lead = 1 if tied else K
    sizes = [K, K * D, lead * (1 if covariance_type == "spherical" else D)]
    if covariance_type == "full":
        sizes.append(lead * (D * (D - 1) // 2))
    return sizes


def gmm_supported(D: int, K: int, covariance_type: str, tied: bool, dtype=torch.float32) -> bool:
    """True when zk_gmm_log_prob / zk_gmm_backward serve the shape: 1 <= D <= 64, 1 <= K <= 64, float32 / float64 (bfloat16 is widened)."""
    return (covariance_type in GMM_COVARIANCE and dtype in (torch.float32, torch.float64, torch.bfloat16)
            and _C.lib().zk_gmm_total(int(D), int(K), GMM_COVARIANCE[covariance_type], int(bool(tied))) > 0)


def _gmm_torch_log_prob(x: Tensor, phi: Tensor, K: int, covariance_type: str, tied: bool, epsilon: float) -> Tensor:
    """The reference's expressions on torch ops (zuko/mixtures.py: GMM.forward, zuko/distributions.py: Mixture.log_prob): the path of every
    call the kernel does not serve, and the baseline of scripts/bench_gmm.py.  phi [..., total] broadcasts against x [..., D]."""
    D, lead, full = x.shape[-1], 1 if tied else K, covariance_type == "full"
    parts = phi.split(gmm_sizes(D, K, covariance_type, tied), dim=-1)
    batch = phi.shape[:-1]
    logits, loc = parts[0], parts[1].reshape(*batch, K, D)
    scale = parts[2].reshape(*batch, lead, -1).exp() + epsilon
    xk = x.unsqueeze(-2)
    if full:
        factor = torch.diag_embed(scale)
        below = torch.ones_like(factor, dtype=torch.bool).tril(-1)
        factor = factor.masked_scatter(below, parts[3].reshape(*batch, lead, -1))
        log_p = torch.distributions.MultivariateNormal(loc, scale_tril=factor, validate_args=False).log_prob(xk)
    else:
        log_p = torch.distributions.Normal(loc, scale, validate_args=False).log_prob(xk).sum(dim=-1)
    return torch.logsumexp(torch.log_softmax(logits, dim=-1) + log_p, dim=-1)


def _gmm_rows(t: Tensor, width: int) -> tuple[Tensor, int]:
    """t [..., width] as a [N, width] block the kernels can address (unit column stride, row stride >= width): a view where possible."""
    t2 = t.reshape(-1, width)
    if t2.stride(1) != 1 or (t2.shape[0] > 1 and t2.stride(0) < width):
        t2 = t2.contiguous()
    return t2, (t2.stride(0) if t2.shape[0] > 1 else max(t2.stride(0), width))


def _gmm_kernel_serves(x: Tensor, phi: Tensor, K: int, covariance_type: str, tied: bool) -> bool:
    D = x.shape[-1]
    return (GMM_KERNEL and x.dtype == phi.dtype and gmm_supported(D, K, covariance_type, tied, x.dtype) and x.numel() > 0
            and (phi.dim() == 1 or phi.shape[:-1] == x.shape[:-1]))


def _gmm_args(x2: Tensor, ldx: int, phi2: Tensor, ld_phi: int, K: int, covariance_type: str, tied: bool, epsilon: float, **extra):
    return _C.args("zk_gmm_args_v1", dtype=_dtype_code(x2), N=x2.shape[0], D=x2.shape[1], K=K, covariance=GMM_COVARIANCE[covariance_type], tied=int(bool(tied)),
                   epsilon=float(epsilon), x=x2.data_ptr(), ldx=ldx, phi=phi2.data_ptr(), ld_phi=ld_phi, **extra)


def _gmm_operands(x: Tensor, phi: Tensor, K: int, covariance_type: str, tied: bool):
    D = x.shape[-1]
    total = sum(gmm_sizes(D, K, covariance_type, tied))
    if phi.shape[-1] != total:
        raise ValueError(f"zuko_amd: phi has {phi.shape[-1]} columns, a {covariance_type} mixture of {K} components in {D} features needs {total}")
    x2, ldx = _gmm_rows(x, D)
    if phi.dim() == 1:
        return x2, ldx, phi.contiguous(), 0, total
    phi2, ld_phi = _gmm_rows(phi, total)
    return x2, ldx, phi2, ld_phi, total


def gmm_forward_kernel(x: Tensor, phi: Tensor, components: int, covariance_type: str, tied: bool, epsilon: float) -> Tensor:
    """One zk_gmm_log_prob launch on detached operands (the caller checked _gmm_kernel_serves)."""
    x2, ldx, phi2, ld_phi, _ = _gmm_operands(x, phi, components, covariance_type, tied)
    out = torch.empty(x2.shape[0], dtype=x.dtype, device=x.device)
    a = _gmm_args(x2, ldx, phi2, ld_phi, components, covariance_type, tied, epsilon, out=out.data_ptr())
    _C.check(_C.lib().zk_gmm_log_prob(a, _stream()), "zk_gmm_log_prob")
    return out.reshape(x.shape[:-1])


def gmm_backward(x: Tensor, phi: Tensor, g: Tensor, components: int, covariance_type: str = "full", tied: bool = False, epsilon: float = 1e-6,
                 need_x: bool = True, need_phi: bool = True, gx: Tensor | None = None, gphi: Tensor | None = None):
    """(gx, gphi) of sum(g * gmm_log_prob(x, phi)) in one zk_gmm_backward launch (plus the reduction of the partial sums when phi is one shared
    row).  gx [N, D] / gphi [N, total] may be given as views with a row stride (unit column stride); an output that is not needed is None."""
    _require_device(x, phi, g)
    if not _gmm_kernel_serves(x, phi, components, covariance_type, tied):
        raise RuntimeError("zuko_amd: zk_gmm_backward does not serve this call (shape outside 1 <= D, K <= 64, mixed dtypes, or phi not one row per row of x)")
    x2, ldx, phi2, ld_phi, total = _gmm_operands(x, phi, components, covariance_type, tied)
    N, D = x2.shape
    gc = g.expand(x.shape[:-1]).reshape(-1).contiguous()
    extra = {}
    if need_x:
        if gx is None:
            gx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        gx2, ld_gx = _gmm_rows(gx, D)
        assert gx2.data_ptr() == gx.data_ptr() and gx.dtype == x.dtype, "gx must be addressable in place"
        extra.update(gx=gx2.data_ptr(), ld_gx=ld_gx)
    work = None
    if need_phi:
        if gphi is None:
            gphi = torch.empty(phi.shape, dtype=phi.dtype, device=phi.device)
        if ld_phi == 0:
            assert gphi.is_contiguous() and gphi.numel() == total
            n = _C.lib().zk_gmm_workspace_floats(_dtype_code(x2), N, D, components, GMM_COVARIANCE[covariance_type], int(bool(tied)))
            work = torch.empty(n, dtype=x.dtype, device=x.device)
            extra.update(gphi=gphi.data_ptr(), work=work.data_ptr())
        else:
            gphi2, ld_gphi = _gmm_rows(gphi, total)
            assert gphi2.data_ptr() == gphi.data_ptr() and gphi.dtype == x.dtype, "gphi must be addressable in place"
            extra.update(gphi=gphi2.data_ptr(), ld_gphi=ld_gphi)
    a = _gmm_args(x2, ldx, phi2, ld_phi, components, covariance_type, tied, epsilon, g=gc.data_ptr(), **extra)
    _C.check(_C.lib().zk_gmm_backward(a, _stream()), "zk_gmm_backward")
    del work  # (stream-ordered allocator: the block is reused only by later work of this stream)
    return (gx if need_x else None), (gphi if need_phi else None)


def gmm_log_prob(x: Tensor, phi: Tensor, components: int, covariance_type: str = "full", tied: bool = False, epsilon: float = 1e-6) -> Tensor:
    """log p(x) of the Gaussian mixture whose parameters are the rows of phi = logits | loc | diag [| tril] (zuko/mixtures.py: _get_gmm_shapes).
    x [..., D]; phi [total] (one mixture for every row) or [..., total].  zk_gmm_log_prob (and zk_gmm_backward under autograd) when
    1 <= D, components <= 64 and phi is one row or has x's batch shape; otherwise — sample dimensions broadcast over a batch of mixtures, larger
    shapes, GMM_KERNEL = False — the reference's expressions as torch ops on the device."""
    _require_device(x, phi)
    if x.dtype == torch.bfloat16 or phi.dtype == torch.bfloat16:  # storage type only: the density is evaluated and returned in fp32
        x, phi = x.float(), phi.float()
    if not _gmm_kernel_serves(x, phi, components, covariance_type, tied):
        return _gmm_torch_log_prob(x, phi, components, covariance_type, tied, epsilon)
    from . import autograd as AG

    if AG.needs_grad(x, phi):
        return AG.GmmLogProbFn.apply(x, phi, components, covariance_type, tied, epsilon)
    return gmm_forward_kernel(x, phi, components, covariance_type, tied, epsilon)


# ------------------------------------------------------------------------------------------------
# continuous normalizing flow: zk_cnf_step driven by the adaptive controller; torch ops (zuko_amd.utils.odeint) when the kernel does not serve the call
# ------------------------------------------------------------------------------------------------

CNF_KERNEL = True  # False: every call takes the torch-op path (scripts/bench_cnf.py measures the kernel against it)
CNF_STATS: dict = {}  # the last integration: path ("kernel" | "torch"); on the kernel path also attempts, accepted, t_end (the time reached) and trace ("exact" | "hutchinson")
CNF_HUTCHINSON = False  # True: call_and_ladj of an exact=False transform integrates on the kernels too (the probe variant of zk_cnf_step_v2 / zk_cnf_adjoint_step_v2)


def cnf_supported(features: int, context: int = 0, hidden_features=(64, 64), freqs: int = 3, activation=None) -> bool:
    """True when zk_cnf_step serves the field MLP(2 freqs + features + context, features, hidden_features, activation): 1 <= features <= 16, one to
    three hidden layers whose widths are multiples of 16 up to 128, 1 <= freqs <= 8, ELU(alpha = 1) (None: the default of FFJTransform, which is
    ELU); any context width — the context enters the kernel through the first layer's product, computed once per integration."""
    from . import cnf_plan

    act = torch.nn.ELU if activation is None else activation
    if not isinstance(act, torch.nn.Module):
        try:
            act = act()
        except Exception:
            return False
    if type(act) is not torch.nn.ELU or act.alpha != 1.0 or int(context) < 0:
        return False
    return cnf_plan.layout(int(features), int(freqs), tuple(hidden_features)) is not None


def _cnf_kernel_serves(module, c, x: Tensor):
    """The field's weight image when the step kernel serves this call (fp32 on the device, a supported field, nothing asks for gradients), else None."""
    from . import cnf_plan

    if not CNF_KERNEL or not x.is_cuda:
        return None
    ts = [x, *module.ode.parameters(), module.freqs] + ([] if c is None else [c])
    if any(t.dtype != torch.float32 for t in ts):
        return None
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return None
    sh = cnf_plan.shape_of(module)
    if sh is None or x.dim() < 1 or x.shape[-1] != sh[0] or (sh[1] > 0) != (c is not None) or (c is not None and c.shape[-1] != sh[1]) or x.numel() == 0:
        return None
    return cnf_plan.image_of(module, x.device)


def cnf_step(img, x: Tensor, l, pre: Tensor, t: float, dt: float, atol: float, rtol: float, trace_scale: float, y: Tensor, l_next, err: Tensor, err_rows=None, *,
             eps=None) -> None:
    """One attempted Dormand-Prince step on zk_cnf_step: x [N, F] (unit column stride), l [N] | None (None: the value alone, no trace), pre
    [N, H1] or [H1] (one row for every x row) -> y, l_next, and the largest error ratio in `err` (one float, zeroed by the caller).  With `eps`
    [N, F] (unit column stride; needs l) the trace is Hutchinson's estimate eps^T (df/dx) eps, on zk_cnf_step_v2."""
    lay = img.layout
    w = list(lay.widths) + [0, 0]
    N, F = x.shape
    probe = {} if eps is None else dict(eps=eps.data_ptr(), ld_eps=eps.stride(0) if N > 1 else F)
    a = _C.args("zk_cnf_args_v1" if eps is None else "zk_cnf_args_v2", **probe, features=F, freqs=lay.Q, n_hidden=len(lay.widths), width0=w[0], width1=w[1], width2=w[2], image_floats=lay.total,
                n_tangents=0 if l is None else F, N=N, ldx=x.stride(0) if N > 1 else F, ldy=y.stride(0) if N > 1 else F,
                ld_pre=0 if pre.dim() == 1 else (pre.stride(0) if N > 1 else lay.widths[0]), t=t, dt=dt, atol=atol, rtol=rtol, trace_scale=trace_scale,
                x=x.data_ptr(), l=None if l is None else l.data_ptr(), pre=pre.data_ptr(), image=img.data.data_ptr(), y=y.data_ptr(),
                l_next=None if l_next is None else l_next.data_ptr(), err=err.data_ptr(), err_rows=None if err_rows is None else err_rows.data_ptr())
    if eps is None:
        _C.check(_C.lib().zk_cnf_step(a, _stream()), "zk_cnf_step")
    else:
        _C.check(_C.lib().zk_cnf_step_v2(a, _stream()), "zk_cnf_step_v2")


def _cnf_run(module, img, c, x: Tensor, t0: float, t1: float, atol: float, rtol: float, trace_scale: float, with_ladj: bool, keep: bool, eps=None):
    """The controller's loop on zk_cnf_step: (x(t1) [N, F], l(t1) [N] | None, the broadcast shape, pre, the accepted steps, the statistics).  With
    `keep` every accepted step leaves (a clone of the state after it, the time after it, its size) for the adjoint: N F floats per step.  `eps`
    [N, F]: the probe of Hutchinson's estimator, the same for every attempt."""
    from .utils import step_factor

    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("zuko_amd: a continuous flow cannot be captured into a HIP graph: its step loop reads the error estimate back after every "
                           "attempt and the number of attempts depends on the data")
    F = x.shape[-1]
    lin0 = module.ode[0]
    Q2 = 2 * img.Q
    if c is None:
        shape, pre = x.shape, lin0.bias.detach()
    else:
        shape = torch.broadcast_shapes(x.shape[:-1], c.shape[:-1]) + (F,)
        c2 = c.detach().reshape(-1, c.shape[-1])
        pre = torch.addmm(lin0.bias.detach(), c2, lin0.weight.detach()[:, Q2 + F :].t())  # once per integration: it does not depend on t or x
        if c2.shape[0] == 1:
            pre = pre[0]
        elif c.shape[:-1] != shape[:-1]:
            pre = pre.reshape(c.shape[:-1] + (-1,)).expand(shape[:-1] + (-1,)).reshape(-1, pre.shape[-1])
    pre = pre.contiguous()
    if pre.data_ptr() % 16:
        pre = pre.clone()  # (a parameter that is a view into a larger buffer: the kernel reads 16-byte pieces)
    cur = x.detach().expand(shape).reshape(-1, F).contiguous().clone()
    N = cur.shape[0]
    spare = torch.empty_like(cur)
    l_cur = torch.zeros(N, dtype=torch.float32, device=x.device) if with_ladj else None
    l_spare = torch.empty_like(l_cur) if with_ladj else None
    err = torch.zeros(1, dtype=torch.float32, device=x.device)
    data = img.refresh(module)
    f32 = np.float32
    floor = float(f32(1e-9))
    t, end = f32(t0), f32(t1)
    dt = f32(end - t)
    sign = f32(np.sign(dt))
    attempts = accepted = 0
    steps = []
    while sign * (end - t) > 0:
        rest = f32(end - t)
        dt = f32(sign * min(abs(dt), abs(rest)))
        while True:
            err.zero_()
            cnf_step(img, cur, l_cur, pre, float(t), float(dt), atol, rtol, trace_scale, spare, l_spare, err, eps=eps)
            ratio = float(err.item())
            attempts += 1
            if not math.isfinite(ratio):
                raise RuntimeError(f"zuko_amd: continuous flow: non-finite error estimate ({ratio}) at t = {float(t):g}, dt = {float(dt):g}")
            ratio = max(ratio, floor)
            ok = ratio < 1.0
            if ok:
                cur, spare, l_cur, l_spare = spare, cur, l_spare, l_cur
                t = end if dt == rest else f32(t + dt)
                accepted += 1
                if keep:
                    steps.append((cur.clone(), float(t), float(dt)))
            dt = f32(dt * f32(step_factor(ratio)))
            if ok:
                break
    del data
    stats = dict(path="kernel", attempts=attempts, accepted=accepted, t_end=float(t))
    if with_ladj:
        stats["trace"] = "exact" if eps is None else "hutchinson"
    return cur, l_cur, shape, pre, steps, stats


def _cnf_probe_ok(c, x: Tensor, eps) -> bool:
    """The estimator's call is served when x already has the broadcast batch shape (the probe is drawn like x) and a given probe is x's like."""
    if c is not None and torch.broadcast_shapes(x.shape[:-1], c.shape[:-1]) != x.shape[:-1]:
        return False
    return eps is None or (eps.shape == x.shape and eps.dtype == x.dtype and eps.device == x.device and not (torch.is_grad_enabled() and eps.requires_grad))


def cnf_integrate(module, c, x: Tensor, t0: float, t1: float, atol: float, rtol: float, trace_scale: float, with_ladj: bool, phi=(), hutchinson: bool = False, eps=None):
    """(x(t1), l(t1) | None) of the free-form Jacobian ODE of `module` (a zuko_amd.flows.FFJTransform) from x(t0) = x, l(t0) = 0, on the step kernel —
    or None when the kernel does not serve the call (the caller then integrates in torch ops).  l is the log-determinant times `trace_scale`.

    The loop is the reference's (zuko/utils.py:532-552) with t and dt carried in float32: per attempt `err` is zeroed, zk_cnf_step writes the step
    into the spare buffers, the largest ratio is read back (the one synchronisation per attempt the reference has too), dt is multiplied by
    min(10, max(0.1, 0.9 / ratio^(1/5))), and the buffers swap when ratio < 1.  The last step is clamped to the rest of the interval and ends at t1
    exactly.  A non-finite ratio raises RuntimeError (utils.odeint does likewise).

    A call that asks for gradients is served only with CNF_ADJOINT on and a field zk_cnf_adjoint_step serves (cnf_backward_supported): it goes
    through CnfIntegrateFn, which gives gradients to x and to the tensors of `phi` (the transform's: the context and, in train() mode, the
    parameters), as the reference's adjoint does.

    `hutchinson` (with_ladj, CNF_HUTCHINSON on): l integrates Hutchinson's estimate eps^T (df/dx) eps of the trace on the probe variant of the
    kernels.  The probe is `eps` [like x] or ONE torch.randn_like(x), drawn here once the call is known to be served — where the torch-op path
    draws its own — and constant over the integration; it has no gradient."""
    if hutchinson and not (CNF_HUTCHINSON and with_ladj and _cnf_probe_ok(c, x, eps)):
        return None
    img = _cnf_kernel_serves(module, c, x)
    if img is None:
        img = _cnf_adjoint_serves(module, c, x, phi)
        if img is None:
            return None
    eps = (torch.randn_like(x) if eps is None else eps.detach()).reshape(-1, x.shape[-1]).contiguous() if hutchinson else None
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in phi)):
        out = CnfIntegrateFn.apply((module, c, t0, t1, atol, rtol, trace_scale, with_ladj, eps), x, *phi)
        return (out[0], out[1]) if with_ladj else (out, None)
    cur, l_cur, shape, _, _, stats = _cnf_run(module, img, c, x, t0, t1, atol, rtol, trace_scale, with_ladj, False, eps)
    CNF_STATS.clear()
    CNF_STATS.update(stats)
    return cur.reshape(shape), (l_cur.reshape(shape[:-1]) if with_ladj else None)


# ---- training: the checkpoint adjoint on zk_cnf_adjoint_step ---------------------------------------------------------------------------

CNF_ADJOINT = False  # True: calls that ask for gradients integrate on the kernels too (CnfIntegrateFn); False: they take the torch-op path


def cnf_backward_supported(features: int, context: int = 0, hidden_features=(64, 64), freqs: int = 3, activation=None) -> bool:
    """True when zk_cnf_adjoint_step serves the field: the envelope of `cnf_supported` with every hidden width at most 64."""
    from . import cnf_plan

    if not cnf_supported(features, context, hidden_features, freqs, activation):
        return False
    return cnf_plan.layout_backward(int(features), int(freqs), tuple(hidden_features)) is not None


def _cnf_adjoint_serves(module, c, x: Tensor, phi):
    """The forward image when CnfIntegrateFn serves this call: the switch on, the conditions of `_cnf_kernel_serves` but for the gradients, a
    field the adjoint kernel serves, and a `phi` made of the context and the field's own weights and biases."""
    from . import cnf_plan

    if not (CNF_KERNEL and CNF_ADJOINT) or not x.is_cuda:
        return None
    ts = [x, *module.ode.parameters(), module.freqs] + ([] if c is None else [c])
    if any(t.dtype != torch.float32 for t in ts):
        return None
    sh = cnf_plan.shape_of(module)
    if sh is None or x.dim() < 1 or x.shape[-1] != sh[0] or (sh[1] > 0) != (c is not None) or (c is not None and c.shape[-1] != sh[1]) or x.numel() == 0:
        return None
    own = {id(p) for lin in cnf_plan._linears(module.ode) for p in (lin.weight, lin.bias)}
    if any(p is not c and id(p) not in own for p in phi):
        return None
    if cnf_plan.backward_image_of(module, x.device) is None:
        return None
    return cnf_plan.image_of(module, x.device)


def cnf_adjoint_step(bimg, x: Tensor, ax: Tensor, al, pre: Tensor, t: float, dt: float, trace_scale: float, ax_next: Tensor, gpre: Tensor, gparams, work: Tensor, *,
                     eps=None) -> None:
    """One reverse step on zk_cnf_adjoint_step: x [N, F] the checkpoint after the forward step (t, dt), ax [N, F], al [N] | None -> ax_next; gpre
    [N, H1] and gparams [flat] | None are added to.  `work`: cnf_adjoint_workspace(bimg, N) floats.  With `eps` [N, F] (unit column stride), the
    probe of the forward steps, the trace term is that of Hutchinson's estimate, on zk_cnf_adjoint_step_v2 (al = None: the probe is not read)."""
    lay = bimg.layout
    w = list(lay.fwd.widths) + [0, 0]
    N, F = x.shape
    probe = {} if eps is None else dict(eps=eps.data_ptr(), ld_eps=eps.stride(0) if N > 1 else F)
    a = _C.args("zk_cnf_adj_args_v1" if eps is None else "zk_cnf_adj_args_v2", **probe, features=F, freqs=lay.fwd.Q, n_hidden=len(lay.fwd.widths), width0=w[0], width1=w[1], width2=w[2], image_floats=lay.total,
                grad_floats=lay.g_total, N=N, ldx=x.stride(0) if N > 1 else F, ld_ax=ax.stride(0) if N > 1 else F, ld_ax_next=ax_next.stride(0) if N > 1 else F,
                ld_pre=0 if pre.dim() == 1 else (pre.stride(0) if N > 1 else w[0]), ld_gpre=gpre.stride(0) if N > 1 else w[0],
                flat_total=0 if gparams is None else gparams.numel(), t=t, dt=dt, trace_scale=trace_scale, x=x.data_ptr(), ax=ax.data_ptr(),
                al=None if al is None else al.data_ptr(), pre=pre.data_ptr(), image=bimg.data.data_ptr(), grad_table=bimg.table.data_ptr(), ax_next=ax_next.data_ptr(),
                gpre=gpre.data_ptr(), gparams=None if gparams is None else gparams.data_ptr(), work=work.data_ptr())
    if eps is None:
        _C.check(_C.lib().zk_cnf_adjoint_step(a, _stream()), "zk_cnf_adjoint_step")
    else:
        _C.check(_C.lib().zk_cnf_adjoint_step_v2(a, _stream()), "zk_cnf_adjoint_step_v2")


def cnf_adjoint_workspace(bimg, N: int) -> int:
    lay = bimg.layout
    w = list(lay.fwd.widths) + [0, 0]
    n = ctypes.c_int64(0)
    _C.check(_C.lib().zk_cnf_adjoint_workspace_floats(N, lay.fwd.F, lay.fwd.Q, len(lay.fwd.widths), w[0], w[1], w[2], ctypes.byref(n)), "zk_cnf_adjoint_workspace_floats")
    return int(n.value)


class CnfIntegrateFn(torch.autograd.Function):
    """x(t1) (and l(t1)) on zk_cnf_step, keeping every accepted step; backward makes one zk_cnf_adjoint_step per kept step in reverse — no host
    synchronisation — and turns gpre into the gradients of b0, the context's columns of W0 and the context.  Inputs: the settings, x, and the
    transform's phi; gradients go to x and to exactly those tensors.  The settings end with the probe of Hutchinson's estimator ([N, F] | None):
    the node keeps it (N F floats) and gives it to every reverse step."""

    @staticmethod
    def forward(ctx, cfg, x, *phi):
        from . import cnf_plan

        module, c, t0, t1, atol, rtol, trace_scale, with_ladj, eps = cfg
        img = cnf_plan.image_of(module, x.device)
        cur, l_cur, shape, pre, steps, stats = _cnf_run(module, img, c, x, t0, t1, atol, rtol, trace_scale, with_ladj, True, eps)
        ctx.set_materialize_grads(False)
        ctx.cfg, ctx.steps, ctx.pre, ctx.shape, ctx.x_shape, ctx.phi = cfg, steps, pre, shape, x.shape, phi
        CNF_STATS.clear()
        CNF_STATS.update(stats)
        y = cur.reshape(shape)
        return (y, l_cur.reshape(shape[:-1])) if with_ladj else y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy, gl=None):
        from . import cnf_plan

        module, c, _, _, _, _, trace_scale, with_ladj, eps = ctx.cfg
        shape, pre, phi = ctx.shape, ctx.pre, ctx.phi
        F = shape[-1]
        dev = pre.device
        bimg = cnf_plan.backward_image_of(module, dev)
        data = bimg.refresh(module)
        N = math.prod(shape[:-1])
        ax = torch.zeros(N, F, dtype=torch.float32, device=dev) if gy is None else gy.float().expand(shape).reshape(N, F).contiguous().clone()
        al = None if (not with_ladj or gl is None) else gl.float().expand(shape[:-1]).reshape(N).contiguous()
        spare = torch.empty_like(ax)
        H0 = bimg.widths[0]
        gpre = torch.zeros(N, H0, dtype=torch.float32, device=dev)
        want_params = any(p is not c for p in phi)
        gparams = torch.zeros(bimg.flat_total, dtype=torch.float32, device=dev) if want_params else None
        work = torch.empty(max(cnf_adjoint_workspace(bimg, N), 4), dtype=torch.float32, device=dev)
        for xs, t, dt in reversed(ctx.steps):
            cnf_adjoint_step(bimg, xs, ax, al, pre, t, dt, trace_scale, spare, gpre, gparams, work, eps=eps)
            ax, spare = spare, ax
        del data
        CNF_STATS["adjoint_steps"] = len(ctx.steps)
        gx = ax.reshape(shape).sum_to_size(ctx.x_shape) if ctx.needs_input_grad[1] else None
        lins = cnf_plan._linears(module.ode)
        Q2, C = 2 * bimg.Q, bimg.C
        w_off, b_off, _, _ = cnf_plan.flat_offsets(F, bimg.Q, C, bimg.widths)
        where = {}
        for l, lin in enumerate(lins):
            where[id(lin.weight)] = ("w", l)
            where[id(lin.bias)] = ("b", l)
        out = []
        for k, p in enumerate(phi):
            if not ctx.needs_input_grad[2 + k]:
                out.append(None)
            elif p is c:
                gc = gpre @ lins[0].weight.detach()[:, Q2 + F :]
                out.append(gc.reshape(shape[:-1] + (C,)).sum_to_size(c.shape))
            else:
                kind, l = where[id(p)]
                if kind == "b":
                    out.append(gpre.sum(dim=0) if l == 0 else gparams[b_off[l] : b_off[l] + p.numel()].clone())
                else:
                    g = gparams[w_off[l] : w_off[l] + p.numel()].reshape(p.shape).clone()
                    if l == 0 and C > 0:
                        g[:, Q2 + F :] = gpre.t() @ c.detach().expand(shape[:-1] + (C,)).reshape(N, C)
                    out.append(g)
        return (None, gx, *out)
