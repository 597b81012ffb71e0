r"""Generate the fixtures of the neural autoregressive flow from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_naf.py

mnn_{a,b,c,d}.npz: the stacked weights of `zuko.flows.neural.MNN(signal=S, stack=D, hidden_features=hidden)` under a fixed seed
(w0, b0, w1, ...), x uniform in +-9.5, signal ~ 1.5 N(0, 1), and what the reference makes of them in float32 and float64:
y, ladj (MonotonicTransform.call_and_ladj) and inv (its bisection inverse) of `targets` — the float32 y with rows 0..3 replaced by
values outside f(+-bound) (the bisection then runs into an end of the interval).  mnn_d has widths the kernel does not serve.
flow_naf_small.npz: NAF(features=5, context=3, transforms=2) under seed 11: the state_dict's hash (weights are re-created from
the seed), x, c, log_prob, z = transform(x), x_inv = transform.inv(z) in both precisions, and the float64 gradient of
log_prob.mean() for every parameter (stored rounded to float32: the tests' bar is 2e-4 of the largest entry).
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
from zuko.flows.neural import MNN, NAF  # noqa: E402

CASES = {  # name: (N, D, S, hidden, seed)
    "mnn_a": (257, 5, 16, (64, 64), 21),
    "mnn_b": (130, 8, 3, (32,), 22),
    "mnn_c": (67, 3, 7, (16, 48, 128), 23),
    "mnn_d": (33, 4, 16, (30, 30), 24),
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


def mnn_case(name: str) -> None:
    N, D, S, hidden, seed = CASES[name]
    torch.manual_seed(seed)
    m32 = MNN(signal=S, stack=D, hidden_features=hidden).eval()
    for p in m32.parameters():
        p.requires_grad_(False)
    x = (torch.rand(N, D) * 2 - 1) * 9.5
    signal = 1.5 * torch.randn(N, D, S)
    torch.manual_seed(seed)
    m64 = MNN(signal=S, stack=D, hidden_features=hidden).eval().double()
    for p in m64.parameters():
        p.requires_grad_(False)
    out = {"x": x.numpy(), "signal": signal.numpy()}
    lins = [l for l in m32.network if hasattr(l, "weight")]
    for i, l in enumerate(lins):
        out[f"w{i}"], out[f"b{i}"] = l.weight.numpy(), l.bias.numpy()
    t32, t64 = m32(signal), m64(signal.double())
    y32, l32 = t32.call_and_ladj(x)
    y64, l64 = t64.call_and_ladj(x.double())
    targets = y32.detach().clone()
    ends = torch.full_like(x[:1], 10.0)
    hi, lo = m32.f(signal[0:1], ends), m32.f(signal[1:2], -ends)
    targets[0], targets[1] = hi[0] + 1.0, lo[0] - 1.0
    targets[2], targets[3] = m32.f(signal[2:3], ends)[0] + 100.0, m32.f(signal[3:4], -ends)[0] - 100.0
    with torch.no_grad():
        inv32, inv64 = t32.inv(targets), t64.inv(targets.double())
    out.update(y32=y32.detach().numpy(), ladj32=l32.detach().numpy(), y64=y64.detach().numpy(), ladj64=l64.detach().numpy(), targets=targets.numpy(),
               inv32=inv32.numpy(), inv64=inv64.numpy())
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    print(name, {k: v.shape for k, v in out.items()}, f"|y32 - y64| {np.abs(out['y32'] - out['y64']).max():.2e}  |ladj| {np.abs(out['ladj32'] - out['ladj64']).max():.2e}"
          f"  |inv| {np.abs(out['inv32'] - out['inv64']).max():.2e}")


def flow_case() -> None:
    seed, kw = 11, dict(features=5, context=3, transforms=2)
    torch.manual_seed(seed)
    f32 = NAF(**kw)
    torch.manual_seed(seed)
    f64 = NAF(**kw).double()
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
    np.savez(os.path.join(HERE, "flow_naf_small.npz"), **out)
    print("flow_naf_small", len(names), "parameters,", f"|log_prob32 - 64| {np.abs(out['log_prob32'] - out['log_prob64']).max():.2e}")


if __name__ == "__main__":
    print("zuko", zuko.__version__)
    for name in CASES:
        mnn_case(name)
    flow_case()
