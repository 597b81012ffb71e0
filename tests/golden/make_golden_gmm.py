r"""Generate the fixtures of the Gaussian mixture model from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_gmm.py

gmm_{a..f}.npz: x ~ 2.5 N(0, 1), rows of parameters phi (logits ~ N(0, 1), loc ~ 2 N(0, 1), diag ~ 0.5 N(0, 1), tril ~ (0.5 / sqrt(D)) N(0, 1)),
weights g ~ N(0, 1), and what the reference makes of them in float32 and float64: log_prob = GMM(...)(c).log_prob(x) with phi standing in for the
output of the model's MLP, and gphi, gx = the gradients of (log_prob * g).sum().  `meta` holds N, D, K, covariance (0 full, 1 diagonal,
2 spherical), tied.
flow_gmm_small.npz: GMM(features=5, context=3, components=4) under seed 11: the state_dict's hash (weights are re-created from the seed), x, c,
log_prob in both precisions and the float64 gradient of log_prob.mean() for every parameter.  flow_gmm_uncond.npz: the same for the
unconditional GMM(features=3, components=5).
"""

from __future__ import annotations

import hashlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ZUKO_REFERENCE"])

import zuko  # noqa: E402  (the real reference)
from zuko.mixtures import GMM  # noqa: E402

COV = {"full": 0, "diagonal": 1, "spherical": 2}
CASES = {  # name: (N, D, K, covariance, tied, seed)
    "gmm_a": (67, 8, 4, "full", False, 31),
    "gmm_b": (67, 8, 4, "full", True, 32),
    "gmm_c": (97, 5, 4, "diagonal", False, 33),
    "gmm_d": (97, 5, 4, "spherical", True, 34),
    "gmm_e": (97, 1, 1, "full", False, 35),
    "gmm_f": (97, 2, 3, "full", False, 36),
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


class Rows(torch.nn.Module):
    """Stands in for the MLP of a conditional GMM: returns the given parameter rows."""

    def __init__(self, phi):
        super().__init__()
        self.rows = phi

    def forward(self, c):
        return self.rows


def kernel_case(name: str) -> None:
    N, D, K, cov, tied, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    model = GMM(features=D, context=1, components=K, covariance_type=cov, tied=tied)
    scales = [1.0, 2.0, 0.5, 0.5 / math.sqrt(D)]
    phi = torch.cat([s * torch.randn(N, math.prod(shape), generator=g) for s, shape in zip(scales, model.shapes)], dim=-1)
    assert phi.shape[-1] == model.total
    x = 2.5 * torch.randn(N, D, generator=g)
    w = torch.randn(N, generator=g)
    out = {"x": x.numpy(), "phi": phi.numpy(), "g": w.numpy(), "meta": np.array([N, D, K, COV[cov], int(tied)], dtype=np.int64)}
    for tag, cast in (("32", lambda t: t.clone()), ("64", lambda t: t.double())):
        xt, pt = cast(x).requires_grad_(), cast(phi).requires_grad_()
        model.hyper = Rows(pt)
        lp = model(xt[:, :1]).log_prob(xt)
        gp, gx = torch.autograd.grad((lp * cast(w)).sum(), (pt, xt))
        out["log_prob" + tag], out["gphi" + tag], out["gx" + tag] = lp.detach().numpy(), gp.numpy(), gx.numpy()
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    print(name, {k: v.shape for k, v in out.items()}, f"|lp32 - lp64| {np.abs(out['log_prob32'] - out['log_prob64']).max():.2e}  max |lp| {np.abs(out['log_prob64']).max():.1f}")


def module_case(name: str, kw: dict, seed: int = 11) -> None:
    torch.manual_seed(seed)
    m32 = GMM(**kw)
    torch.manual_seed(seed)
    m64 = GMM(**kw).double()
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
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    print(name, names, f"|log_prob32 - 64| {np.abs(out['log_prob32'] - out['log_prob64']).max():.2e}")


if __name__ == "__main__":
    print("zuko", zuko.__version__)
    for name in CASES:
        kernel_case(name)
    module_case("flow_gmm_small", dict(features=5, context=3, components=4))
    module_case("flow_gmm_uncond", dict(features=3, components=5))
