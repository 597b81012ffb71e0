r"""Generate the fixture of the continuous flow under Hutchinson's estimator from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_cnf_hutch.py

flow_cnf_hutch.npz: `zuko.flows.CNF(3, 2, exact=False)` under seed 17 (the weights of flow_cnf_small.npz: `exact` does not enter the initialisation),
67 rows of x, c ~ N(0, 1), and

  * `eps` [67, 3]: the probe the reference drew for the first call — recorded by wrapping `torch.randn_like` around `call_and_ladj` — and which every
    other run below is GIVEN through the same wrapper (cast to the run's precision), so that all of them estimate the same quantity;
  * z32 / ladj32: `call_and_ladj(x)` in float32 at default tolerances; z32_098 / ladj32_098, z32_102 / ladj32_102: both tolerances scaled by 0.98 and
    1.02 — stand-ins for a step sequence that differs at a borderline decision; z_truth / ladj_truth: float64 at atol = 1e-10, rtol = 1e-9;
    lp<tag> = Normal(0, 1).log_prob(z).sum(-1) + ladj for every tag (what tests/test_gpu_cnf.py: _distances reads);
  * `grad/<name>` (float64, stored rounded to float32) and `grad32/<name>`: the gradients of -(base.log_prob(z) + ladj).mean() for every parameter in
    train() mode with that probe; `param_names`; the state_dict's hash.
"""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.environ["ZUKO_REFERENCE"])

import zuko  # noqa: E402  (the real reference)
from make_golden_cnf import TRUTH, sd_hash  # noqa: E402
from zuko.flows import CNF  # noqa: E402

SEED, KW, ROWS = 17, dict(features=3, context=2, exact=False), 67


class Probe:
    """Wraps torch.randn_like: the first draw is recorded, every later one returns it in the precision asked for."""

    def __init__(self):
        self.eps, self.draws, self._randn_like = None, 0, torch.randn_like

    def __enter__(self):
        def randn_like(x, *args, **kw):
            self.draws += 1
            if self.eps is None:
                self.eps = self._randn_like(x, *args, **kw)
            assert self.eps.shape == x.shape
            return self.eps.to(x.dtype)

        torch.randn_like = randn_like
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._randn_like


def flow_of(dtype, train=False):
    torch.manual_seed(SEED)
    flow = CNF(**KW).to(dtype)
    return flow.train() if train else flow.eval()


def main() -> None:
    g = torch.Generator().manual_seed(SEED + 1)
    x, c = torch.randn(ROWS, 3, generator=g), torch.randn(ROWS, 2, generator=g)
    f32, f64 = flow_of(torch.float32), flow_of(torch.float64)
    out = {"hash": np.frombuffer(sd_hash(f32.state_dict()).encode(), dtype=np.uint8), "x": x.numpy(), "c": c.numpy()}

    def run(flow, dtype, scale=1.0, **tol):
        tr = flow.transform
        keep = tr.atol, tr.rtol
        tr.atol, tr.rtol = tol.get("atol", keep[0]) * scale, tol.get("rtol", keep[1]) * scale
        try:
            with torch.no_grad():
                d = flow(c.to(dtype))
                z, ladj = d.transform.call_and_ladj(x.to(dtype))
                lp = d.base.log_prob(z) + ladj
        finally:
            tr.atol, tr.rtol = keep
        return z.numpy(), ladj.numpy(), lp.numpy()

    torch.manual_seed(SEED + 2)
    with Probe() as probe:
        for tag, flow, dtype, kw in (("32", f32, torch.float32, {}), ("32_098", f32, torch.float32, dict(scale=0.98)), ("32_102", f32, torch.float32, dict(scale=1.02)),
                                     ("_truth", f64, torch.float64, TRUTH)):
            out["z" + tag], out["ladj" + tag], out["lp" + tag] = run(flow, dtype, **kw)
        out["eps"] = probe.eps.numpy()
        names = []
        for tag, dtype in (("grad/", torch.float64), ("grad32/", torch.float32)):
            train = flow_of(dtype, train=True)
            d = train(c.to(dtype))
            z, ladj = d.transform.call_and_ladj(x.to(dtype))
            (-(d.base.log_prob(z) + ladj).mean()).backward()
            names = [k for k, _ in train.named_parameters()]
            for k, p in train.named_parameters():
                out[tag + k] = p.grad.numpy().astype(np.float32)
        assert probe.draws == 6
    out["param_names"] = np.array(names)
    np.savez(os.path.join(HERE, "flow_cnf_hutch.npz"), **out)
    d = lambda a, b: float(np.abs(out[a].astype(np.float64) - out[b]).max())
    rel = max(float(np.abs(out["grad32/" + k].astype(np.float64) - out["grad/" + k]).max() / np.abs(out["grad/" + k]).max()) for k in names)
    print("flow_cnf_hutch", f"|lp32 - truth| {d('lp32', 'lp_truth'):.2e}, 0.98: {d('lp32_098', 'lp_truth'):.2e}, 1.02: {d('lp32_102', 'lp_truth'):.2e};",
          f"|z32 - truth| {d('z32', 'z_truth'):.2e}; float32 gradients {rel:.2e} of the largest entry from the float64 ones;", os.path.getsize(os.path.join(HERE, "flow_cnf_hutch.npz")), "bytes")


if __name__ == "__main__":
    print("zuko", zuko.__version__)
    torch.set_num_threads(8)
    main()
