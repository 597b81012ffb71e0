r"""Generate the fixtures of the unconstrained neural autoregressive flow from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_unaf.py

umnn_{a,b,c,d,e}.npz: the stacked weights of `zuko.flows.neural.UMNN(signal=S, stack=D, hidden_features=hidden)` under a fixed seed
(w0, b0, w1, ...), x uniform in +-9.5, signal ~ 1.5 N(0, 1), constant ~ N(0, 1), and what the reference makes of them in float32 and
float64: y, ladj (call_and_ladj of the transform UMNN.forward returns) and inv (its bisection inverse) of `targets` — the float32 y with
rows 0 and 1 replaced by f(+-10) + constant +- 1 (the bisection then runs into an end of the interval).  umnn_d has widths the kernel does
not serve.  umnn_e has its last layer's weight and bias multiplied by 30: the integrand's logarithm leaves the linear part of the squash on
both sides; its inverse is ill-conditioned and is not stored.
flow_unaf_small.npz: UNAF(features=5, context=3, transforms=2) under seed 11: the state_dict's hash (weights are re-created from the
seed), x, c, log_prob, z = transform(x), x_inv = transform.inv(z) in both precisions, and the float64 gradient of log_prob.mean() for every
parameter (stored rounded to float32: the tests' bar is 2e-4 of the largest entry).
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
from zuko.flows.neural import UMNN, UNAF  # noqa: E402

CASES = {  # name: (N, D, S, hidden, seed, factor of the last layer)
    "umnn_a": (257, 5, 16, (64, 64), 31, 1.0),
    "umnn_b": (130, 8, 3, (32,), 32, 1.0),
    "umnn_c": (67, 3, 7, (16, 48, 128), 33, 1.0),
    "umnn_d": (33, 4, 16, (30, 30), 34, 1.0),
    "umnn_e": (130, 4, 16, (64, 64), 35, 30.0),
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


def network(S: int, D: int, hidden, seed: int, factor: float, double: bool):
    torch.manual_seed(seed)
    m = UMNN(signal=S, stack=D, hidden_features=hidden).eval()
    with torch.no_grad():
        last = [l for l in m.integrand if hasattr(l, "weight")][-1]
        last.weight.mul_(factor)
        last.bias.mul_(factor)
    for p in m.parameters():
        p.requires_grad_(False)
    return m.double() if double else m


def umnn_case(name: str) -> None:
    N, D, S, hidden, seed, factor = CASES[name]
    m32 = network(S, D, hidden, seed, factor, False)
    x = (torch.rand(N, D) * 2 - 1) * 9.5  # (drawn behind the network's initialisation, from the same stream)
    signal = 1.5 * torch.randn(N, D, S)
    constant = torch.randn(N, D)
    m64 = network(S, D, hidden, seed, factor, True)
    out = {"x": x.numpy(), "signal": signal.numpy(), "constant": constant.numpy()}
    for i, l in enumerate(l for l in m32.integrand if hasattr(l, "weight")):
        out[f"w{i}"], out[f"b{i}"] = l.weight.numpy(), l.bias.numpy()
    with torch.no_grad():
        t32, t64 = m32(signal, constant), m64(signal.double(), constant.double())
        y32, l32 = t32.call_and_ladj(x)
        y64, l64 = t64.call_and_ladj(x.double())
        out.update(y32=y32.numpy(), ladj32=l32.numpy(), y64=y64.numpy(), ladj64=l64.numpy())
        report = f"|y32 - y64| {np.abs(out['y32'] - out['y64']).max():.2e} (|y| <= {np.abs(out['y64']).max():.3g})  |ladj| {np.abs(out['ladj32'] - out['ladj64']).max():.2e}"
        if factor == 1.0:
            targets = y32.clone()
            ends = torch.full_like(x[:1], 10.0)
            targets[0] = m32(signal[0:1], constant[0:1])(ends)[0] + 1.0
            targets[1] = m32(signal[1:2], constant[1:2])(-ends)[0] - 1.0
            inv32, inv64 = t32.inv(targets), t64.inv(targets.double())
            out.update(targets=targets.numpy(), inv32=inv32.numpy(), inv64=inv64.numpy())
            report += f"  |inv| {np.abs(out['inv32'] - out['inv64']).max():.2e}  ends {inv32[0, 0].item()}, {inv32[1, 0].item()}"
        else:
            h = torch.log(m64.g(signal.double(), x.double()))
            report += f"  log g in [{h.min().item():.2f}, {h.max().item():.2f}]"
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    print(name, {k: v.shape for k, v in out.items()}, report)


def flow_case() -> None:
    seed, kw = 11, dict(features=5, context=3, transforms=2)
    torch.manual_seed(seed)
    f32 = UNAF(**kw)
    torch.manual_seed(seed)
    f64 = UNAF(**kw).double()
    g = torch.Generator().manual_seed(seed + 1)
    x, c = torch.randn(96, 5, generator=g), torch.randn(96, 3, generator=g)
    out = {"hash": np.frombuffer(sd_hash(f32.state_dict()).encode(), dtype=np.uint8), "x": x.numpy(), "c": c.numpy()}
    for tag, flow, cast in (("32", f32, lambda t: t), ("64", f64, lambda t: t.double())):
        with torch.no_grad():
            d = flow(cast(c))
            z = d.transform(cast(x))
            out["log_prob" + tag], out["z" + tag], out["x_inv" + tag] = d.log_prob(cast(x)).numpy(), z.numpy(), d.transform.inv(z).numpy()
    f64(c.double()).log_prob(x.double()).mean().backward()
    names = []
    for k, p in f64.named_parameters():
        names.append(k)
        out["grad/" + k] = p.grad.numpy().astype(np.float32)
    out["param_names"] = np.array(names)
    np.savez(os.path.join(HERE, "flow_unaf_small.npz"), **out)
    print("flow_unaf_small", len(names), "parameters,", f"|log_prob32 - 64| {np.abs(out['log_prob32'] - out['log_prob64']).max():.2e}")


if __name__ == "__main__":
    print("zuko", zuko.__version__)
    for name in CASES:
        umnn_case(name)
    flow_case()
