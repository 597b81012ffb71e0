r"""Shape helpers shared by the flow factories (host-side logic, no arithmetic), and the adaptive ODE integrator of the continuous flow in torch ops
(`odeint`, `dopri45`: the path of every CNF call that the step kernel csrc/cnf.hip does not serve)."""

from __future__ import annotations

import math
from typing import Any, Callable, Sequence

import torch
import torch.nn as nn
from torch import Tensor

__all__ = ["Partial", "broadcast", "dopri45", "odeint", "unpack"]


def broadcast(*tensors: Tensor, ignore: int | Sequence[int] = 0) -> list[Tensor]:
    """Expand the leading dims of `tensors` to a common shape, leaving the last `ignore` dims of
    each untouched (same contract as zuko/utils.py:212-244)."""
    skip = [ignore] * len(tensors) if isinstance(ignore, int) else list(ignore)
    cut = [t.dim() - s for t, s in zip(tensors, skip)]
    lead = torch.broadcast_shapes(*[t.shape[:c] for t, c in zip(tensors, cut)])
    return [t.expand(lead + t.shape[c:]) for t, c in zip(tensors, cut)]


def unpack(x: Tensor, shapes: Sequence[Sequence[int]]) -> tuple[Tensor, ...]:
    """Split the last dim of a packed tensor into views of the given shapes
    (same contract as zuko/utils.py:596-622); the pieces alias `x`, which is what lets the
    kernels recognise the packed phi[N, D, total] layout."""
    sizes = [math.prod(s) for s in shapes]
    return tuple(_shape_tail(piece, s) for piece, s in zip(x.split(sizes, -1), shapes))


def _shape_tail(piece: Tensor, shape: Sequence[int]) -> Tensor:
    shape = tuple(shape)
    if len(shape) == 0:
        return piece.squeeze(-1)
    if len(shape) == 1:
        return piece
    return piece.unflatten(-1, shape)


class Partial(nn.Module):
    """`functools.partial` as a module: tensor arguments become buffers or parameters so they move
    with `.to(device)` and appear in the state_dict under `_0, _1, ...` / their keyword
    (key layout of zuko/utils.py:26-115, e.g. `base._0`... NOTE: flows register `loc`/`scale`)."""

    def __init__(self, f: Callable, /, *args: Any, buffer: bool = False, **kwargs: Any) -> None:
        super().__init__()
        self.f = f
        self._nargs = len(args)
        self._keys = list(kwargs)
        for name, value in [(f"_{i}", a) for i, a in enumerate(args)] + list(kwargs.items()):
            if torch.is_tensor(value):
                if buffer:
                    self.register_buffer(name, value)
                else:
                    self.register_parameter(name, nn.Parameter(value))
            else:
                setattr(self, name, value)

    @property
    def args(self) -> list:
        return [getattr(self, f"_{i}") for i in range(self._nargs)]

    @property
    def kwargs(self) -> dict:
        return {k: getattr(self, k) for k in self._keys}

    def extra_repr(self) -> str:
        return "" if isinstance(self.f, nn.Module) else f"(f): {self.f}"

    def forward(self, *args: Any, **kwargs: Any) -> Any:
        return self.f(*self.args, *args, **self.kwargs, **kwargs)


# ------------------------------------------------------------------------------------------------
# adaptive Dormand-Prince 5(4) integration with the adaptive-checkpoint adjoint (same contract as zuko/utils.py:366-593)
# ------------------------------------------------------------------------------------------------

# Butcher tableau (https://wikipedia.org/wiki/Dormand-Prince_method): stage s is evaluated at t + node dt on x + sum_m row[m] k_m.  A None entry is
# a term the sum does not have; the terms are added left to right.
_DP_STAGES = (
    (1 / 5, (1 / 5,)),
    (3 / 10, (3 / 40, 9 / 40)),
    (4 / 5, (44 / 45, -56 / 15, 32 / 9)),
    (8 / 9, (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729)),
    (1, (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656)),
)
_DP_FIFTH = (35 / 384, None, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)
_DP_FOURTH = (5179 / 57600, None, 7571 / 16695, 393 / 640, -92097 / 339200, 187 / 2100, 1 / 40)


class _Bundle(tuple):
    """Several tensors integrated as one state (the adjoint's x, dL/dx, dL/dphi...): sums and scalings go tensor by tensor."""

    def __add__(self, other):
        return _Bundle(a + b for a, b in zip(self, other, strict=True))

    def __sub__(self, other):
        return _Bundle(a - b for a, b in zip(self, other, strict=True))

    def __rmul__(self, factor):
        return _Bundle(factor * a for a in self)


def _dp_sum(x, row, ks):
    for a, k in zip(row, ks):
        if a is not None:
            x = x + a * k
    return x


def dopri45(f: Callable, x, t: Tensor, dt: Tensor, error: bool = False):
    """One Dormand-Prince step from (t, x): the fifth-order result, and with `error` also |fifth - fourth| of the embedded pair."""
    ks = [dt * f(t, x)]
    for node, row in _DP_STAGES:
        ks.append(dt * f(t + node * dt, _dp_sum(x, row, ks)))
    x_next = _dp_sum(x, _DP_FIFTH, ks)
    if not error:
        return x_next
    ks.append(dt * f(t + dt, x_next))
    return x_next, abs(x_next - _dp_sum(x, _DP_FOURTH, ks))


def step_factor(ratio: float) -> float:
    """The controller's factor on dt after an attempt whose largest error-to-tolerance ratio is `ratio` (>= 1e-9)."""
    return min(10.0, max(0.1, 0.9 / ratio ** (1 / 5)))


class _CheckpointAdjoint(torch.autograd.Function):
    """x(t1) by adaptive steps; under grad mode the accepted steps (state after, time after, size) are kept, and backward re-integrates every one of
    them in reverse with the adjoint state (x, dL/dx, dL/dphi), obtaining the vector-Jacobian products from autograd (Zhuang et al., 2020)."""

    @staticmethod
    def forward(ctx, settings, f, x, t0, t1, *phi):
        atol, rtol, keep = settings
        ctx.f, ctx.steps = f, []
        ctx.save_for_backward(x, t0, t1, *phi)
        t, dt = t0, t1 - t0
        sign = torch.sign(dt)
        while sign * (t1 - t) > 0:
            dt = sign * torch.min(abs(dt), abs(t1 - t))  # never past t1
            accepted = False
            while not accepted:
                y, err = dopri45(f, x, t, dt, error=True)
                ratio = torch.max(err / (atol + rtol * torch.max(abs(x), abs(y)))).clip(min=1e-9).item()
                if not math.isfinite(ratio):
                    # (the reference's loop never ends here: NaN < 1 is false for ever, and an infinite ratio keeps shrinking dt by 0.1 x)
                    raise RuntimeError(f"zuko_amd.utils.odeint: non-finite error estimate ({ratio}) at t = {float(t):g}, dt = {float(dt):g}")
                accepted = ratio < 1.0
                if accepted:
                    x, t = y, t + dt
                    if keep:
                        ctx.steps.append((x, t, dt))
                dt = dt * step_factor(ratio)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_x):
        f = ctx.f
        x0, t0, t1, *phi = ctx.saved_tensors
        grad_t1 = torch.sum(f(t1, ctx.steps[-1][0]) * grad_x) if ctx.needs_input_grad[4] else None
        grad_phi = [torch.zeros_like(p) for p in phi]

        def adjoint(t, state):
            with torch.enable_grad():
                x = state[0].detach().requires_grad_()
                dx = f(t, x)
            grads = torch.autograd.grad(dx, (x, *phi), -state[1], allow_unused=True)
            return _Bundle((dx, *[torch.zeros_like(p) if g is None else g for g, p in zip(grads, (x, *phi))]))

        for x, t, dt in reversed(ctx.steps):
            _, grad_x, *grad_phi = dopri45(adjoint, _Bundle((x, grad_x, *grad_phi)), t, -dt)
        grad_t0 = torch.sum(f(t0, x0) * grad_x) if ctx.needs_input_grad[3] else None
        return (None, None, grad_x, grad_t0, grad_t1, *grad_phi)


def odeint(f: Callable, x, t0, t1, phi=(), atol: float = 1e-6, rtol: float = 1e-5):
    """x(t1) = x(t0) + int f(t, x) dt with adaptive Dormand-Prince 5(4) steps, in torch ops.  `x` is a tensor or a sequence of tensors (f then takes
    and returns that many).  A step is accepted when max(err / (atol + rtol max(|x|, |y|))) < 1; the ratio is clipped below at 1e-9, and dt is
    multiplied by min(10, max(0.1, 0.9 / ratio^(1/5))) after every attempt and clamped to what is left of the interval; t and dt are carried in
    the state's dtype.  Gradients reach x, t0, t1 and `phi` (the parameters of f) through the adaptive-checkpoint adjoint.

    One departure from the reference: a non-finite error estimate raises RuntimeError (the reference's loop never terminates then)."""
    settings = (atol, rtol, torch.is_grad_enabled())
    if torch.is_tensor(x):
        x0, g, shapes = x, f, None
    else:
        shapes = [v.shape for v in x]
        sizes = [math.prod(s) for s in shapes]

        def split(v):
            return [p.reshape(s) for p, s in zip(v.split(sizes), shapes)]

        def g(t, v):
            return torch.cat([p.flatten() for p in f(t, *split(v))])

        x0 = torch.cat([v.flatten() for v in x])
    t0 = torch.as_tensor(t0, dtype=x0.dtype, device=x0.device)
    t1 = torch.as_tensor(t1, dtype=x0.dtype, device=x0.device)
    assert not t0.shape and not t1.shape, "'t0' and 't1' must be scalars"
    x1 = _CheckpointAdjoint.apply(settings, g, x0, t0, t1, *phi)
    return x1 if shapes is None else tuple(split(x1))
