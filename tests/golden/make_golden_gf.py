r"""Generate the fixtures of the Gaussianization flow from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_gf.py

gauss_{a..f}.npz: x ~ 1.5 N(0, 1), shift b ~ N(0, 1), unconstrained scale a ~ 0.5 N(0, 1) (case d: 1.0 / 0.5 / 0.3), weights gy, gl ~ N(0, 1), and what
the reference's GaussianizationTransform(b, a) makes of them in float32 and float64: y, ladj = call_and_ladj(x), the gradients gx, gb, ga of
(y * gy + ladj * gl).sum(), and inv = the bisection inverse of float32(y64).  In case f the parameters are [D, K], shared by all rows, and their
gradients are summed over the rows.  `meta` holds N, D, K, shared.  Every recorded value must be finite: a seed that produces one that is not is
changed, not masked.
flow_gf_small.npz: GF(features=5, context=3, transforms=3, components=4) under seed 11: the state_dict's hash (weights are re-created from the seed),
x, c, log_prob in both precisions and the float64 gradient of log_prob.mean() for every parameter.  flow_gf_uncond.npz: the same for the
unconditional GF(features=3, transforms=2, components=5).
"""

from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ZUKO_REFERENCE"])

import zuko  # noqa: E402  (the real reference)
from zuko.flows import GF  # noqa: E402
from zuko.transforms import GaussianizationTransform  # noqa: E402

CASES = {  # name: (N, D, K, shared, (scale of x, b, a), seed)
    "gauss_a": (67, 5, 8, False, (1.5, 1.0, 0.5), 41),
    "gauss_b": (33, 64, 8, False, (1.5, 1.0, 0.5), 42),
    "gauss_c": (19, 70, 4, False, (1.5, 1.0, 0.5), 43),
    "gauss_d": (97, 3, 1, False, (1.0, 0.5, 0.3), 44),
    "gauss_e": (23, 2, 32, False, (1.5, 1.0, 0.5), 45),
    "gauss_f": (131, 6, 8, True, (1.5, 1.0, 0.5), 46),
}


def sd_hash(sd: dict) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        v = sd[k]
        if v is None:
            continue
        h.update(k.encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def finite(name: str, out: dict) -> None:
    for k, v in out.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), f"{name}: {k} has a non-finite value: change the seed"


def kernel_case(name: str) -> None:
    N, D, K, shared, (sx, sb, sa), seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = sx * torch.randn(N, D, generator=g)
    pshape = (D, K) if shared else (N, D, K)
    b, a = sb * torch.randn(pshape, generator=g), sa * torch.randn(pshape, generator=g)
    gy, gl = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
    out = {"x": x.numpy(), "b": b.numpy(), "a": a.numpy(), "gy": gy.numpy(), "gl": gl.numpy(), "meta": np.array([N, D, K, int(shared)], dtype=np.int64)}
    for tag, cast in (("32", lambda t: t.clone()), ("64", lambda t: t.double())):
        xt, bt, at = cast(x).requires_grad_(), cast(b).requires_grad_(), cast(a).requires_grad_()
        y, ladj = GaussianizationTransform(bt, at).call_and_ladj(xt)
        gx, gb, ga = torch.autograd.grad((y * cast(gy) + ladj * cast(gl)).sum(), (xt, bt, at))
        out["y" + tag], out["ladj" + tag] = y.detach().numpy(), ladj.detach().numpy()
        out["gx" + tag], out["gb" + tag], out["ga" + tag] = gx.numpy(), gb.numpy(), ga.numpy()
    y_in = torch.from_numpy(out["y64"]).float()
    with torch.no_grad():
        out["inv32"] = GaussianizationTransform(b, a).inv(y_in).numpy()
        out["inv64"] = GaussianizationTransform(b.double(), a.double()).inv(y_in.double()).numpy()
    finite(name, out)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    ay = np.abs(out["y64"])
    print(name, (N, D, K), f"max |y| {ay.max():.2f}  share |y| > 3: {(ay > 3).mean():.4f}  |y32 - y64| {np.abs(out['y32'] - out['y64']).max():.2e}  "
          f"|ladj32 - ladj64| {np.abs(out['ladj32'] - out['ladj64']).max():.2e}  |inv32 - inv64| {np.abs(out['inv32'] - out['inv64']).max():.2e}  "
          f"{os.path.getsize(os.path.join(HERE, name + '.npz'))} bytes")


def module_case(name: str, kw: dict, seed: int = 11) -> None:
    torch.manual_seed(seed)
    m32 = GF(**kw)
    torch.manual_seed(seed)
    m64 = GF(**kw).double()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(96, kw["features"], generator=g)
    c = torch.randn(96, kw["context"], generator=g) if kw.get("context", 0) else None
    out = {"hash": np.frombuffer(sd_hash(m32.state_dict()).encode(), dtype=np.uint8), "x": x.numpy()}
    if c is not None:
        out["c"] = c.numpy()
    with torch.no_grad():
        out["log_prob32"] = m32(c).log_prob(x).numpy()
        out["log_prob64"] = m64(None if c is None else c.double()).log_prob(x.double()).numpy()
    m64(None if c is None else c.double()).log_prob(x.double()).mean().backward()
    names = []
    for k, p in m64.named_parameters():
        names.append(k)
        out["grad/" + k] = p.grad.numpy()
    out["param_names"] = np.array(names)
    finite(name, out)
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    print(name, names, f"|log_prob32 - 64| {np.abs(out['log_prob32'] - out['log_prob64']).max():.2e}")


if __name__ == "__main__":
    print("zuko", zuko.__version__)
    for name in CASES:
        kernel_case(name)
    module_case("flow_gf_small", dict(features=5, context=3, transforms=3, components=4))
    module_case("flow_gf_uncond", dict(features=3, transforms=2, components=5))
