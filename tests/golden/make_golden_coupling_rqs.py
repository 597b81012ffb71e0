r"""Generate the fixture of the spline coupling flow from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_coupling_rqs.py

flow_nice_rqs_small.npz: NICE(5, 3, transforms=3, hidden_features=[32, 32], univariate=MonotonicRQSTransform, shapes=[(8,), (8,), (7,)]) under seed 21 —
the coupling form of a neural spline flow.  It holds the state dict (`sd/<key>`), 64 rows of x = 2.5 N(0, 1) (so that some values lie in the identity
tails outside [-5, 5]) and of the context c ~ N(0, 1), and what the reference makes of them in float32: z, ladj = transform.call_and_ladj(x),
log_prob(x) and inv = transform.inv(z).  Every recorded value must be finite: a seed that produces one that is not is changed, not masked.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ZUKO_REFERENCE"])

import zuko  # noqa: E402  (the real reference)
from zuko.flows import NICE  # noqa: E402
from zuko.transforms import MonotonicRQSTransform  # noqa: E402

K, SEED = 8, 21

if __name__ == "__main__":
    print("zuko", zuko.__version__)
    torch.manual_seed(SEED)
    flow = NICE(5, 3, transforms=3, hidden_features=[32, 32], univariate=MonotonicRQSTransform, shapes=[(K,), (K,), (K - 1,)])
    g = torch.Generator().manual_seed(SEED + 1)
    x, c = 2.5 * torch.randn(64, 5, generator=g), torch.randn(64, 3, generator=g)
    out = {"sd/" + k: v.detach().numpy() for k, v in flow.state_dict().items() if v is not None}
    with torch.no_grad():
        t = flow(c).transform
        z, ladj = t.call_and_ladj(x)
        out.update(x=x.numpy(), c=c.numpy(), z=z.numpy(), ladj=ladj.numpy(), log_prob=flow(c).log_prob(x).numpy(), inv=t.inv(z).numpy())
    for k, v in out.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), f"{k} has a non-finite value: change the seed"
    path = os.path.join(HERE, "flow_nice_rqs_small.npz")
    np.savez_compressed(path, **out)
    print(f"share |x| > 5: {(np.abs(out['x']) > 5).mean():.4f}  mean |ladj| {np.abs(out['ladj']).mean():.3f}  max |inv - x| {np.abs(out['inv'] - out['x']).max():.2e}  "
          f"{os.path.getsize(path)} bytes")
