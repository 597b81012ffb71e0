r"""NICE(64, transforms=8, hidden_features=[256] * 3) with the 8-bin rational-quadratic spline as univariate map — the coupling form of a neural
spline flow — on one GPU at batch 2^18: `log_prob` and `rsample_and_log_prob`, on the fused launch (zk_coupling_forward_v2 / zk_coupling_inverse_v2:
one launch per transform) and layer by layer (ZUKO_AMD_NO_FUSED_COUPLING=1), alternating in one process.  Device events over >= 0.5 s of work per
measurement after a warm-up.  On a commit without the fused spline launch both columns take the layer-wise path (the line says so: `fused_launches` 0).

    python scripts/bench_coupling_rqs.py                 # prints one JSON line
    rocprofv3 --kernel-trace --stats -- python scripts/bench_coupling_rqs.py --trace     # a few fused calls of each kind, for per-launch kernel times

Roofline: the launch is bound by the f32 matrix instruction; FLOP per sample and transform = 2 x the conditioner's weights, as
bench.py's model_flops counts a coupling flow, against 157.3 TFLOP/s."""

from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import zuko_amd
from zuko_amd import _C
from zuko_amd.flows import NICE
from zuko_amd.transforms import MonotonicRQSTransform

PEAK_F32_MFMA = 157.3e12
D, T, K, HIDDEN, N = 64, 8, 8, [256] * 3, 2**18
ENTRIES = ("zk_coupling_forward_v2", "zk_coupling_inverse_v2")


def timed(fn, min_seconds: float = 0.5, warmup: int = 3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    total = 0.0
    while total < min_seconds or len(times) < 5:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
        total += times[-1]
    times.sort()
    return {"median_ms": 1e3 * times[len(times) // 2], "min_ms": 1e3 * times[0], "max_ms": 1e3 * times[-1], "calls": len(times)}


def layerwise(fn):
    def run():
        os.environ["ZUKO_AMD_NO_FUSED_COUPLING"] = "1"
        try:
            return fn()
        finally:
            os.environ.pop("ZUKO_AMD_NO_FUSED_COUPLING", None)

    return run


def main() -> None:
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    flow = NICE(D, transforms=T, hidden_features=HIDDEN, univariate=MonotonicRQSTransform, shapes=[(K,), (K,), (K - 1,)]).to(dev)
    x = (2.5 * torch.randn(N, D, generator=torch.Generator().manual_seed(1))).to(dev)

    def log_prob():
        with torch.no_grad():
            return flow().log_prob(x)

    def sample():
        with torch.no_grad():
            return flow().rsample_and_log_prob((N,))

    if "--trace" in sys.argv:
        for _ in range(3):
            log_prob()
            sample()
        torch.cuda.synchronize()
        return
    out = {"workload": f"NICE({D}, transforms={T}, hidden_features={HIDDEN}, univariate=MonotonicRQSTransform, bins={K})", "batch": N}
    a, b = log_prob(), layerwise(log_prob)()
    out["log_prob_max_abs_diff_fused_vs_layerwise"] = float((a - b).abs().max())
    del a, b
    runs = {}
    # alternate the two paths (two rounds each): neither sees a systematically warmer or cooler device
    for rnd in range(2):
        for name, wrap in (("fused", lambda f: f), ("layerwise", layerwise)):
            runs.setdefault(("log_prob", name), []).append(timed(wrap(log_prob)))
            runs.setdefault(("rsample_and_log_prob", name), []).append(timed(wrap(sample)))
    for (what, name), rs in runs.items():
        best = min(rs, key=lambda r: r["median_ms"])
        out[f"{what}_{name}"] = best | {"medians_ms": [round(r["median_ms"], 3) for r in rs], "samples_per_s": N / (best["median_ms"] * 1e-3)}
    for what in ("log_prob", "rsample_and_log_prob"):
        out[f"{what}_speedup"] = out[f"{what}_layerwise"]["median_ms"] / out[f"{what}_fused"]["median_ms"]
    # per-launch times by events around the entry points, and the launch as a share of the f32 matrix peak
    flop = 2 * sum(m.weight.numel() for m in flow.transform.transforms[0].hyper if hasattr(m, "weight"))
    out["flop_per_sample_and_transform"] = flop
    _C.PROFILE = {}
    log_prob()
    sample()
    torch.cuda.synchronize()
    prof, _C.PROFILE = _C.PROFILE, None
    out["fused_launches"] = {sym: len(prof.get(sym, [])) for sym in ENTRIES}
    for sym in ENTRIES:
        ts = sorted(a.elapsed_time(b) * 1e-3 for a, b, _ in prof.get(sym, []))
        if ts:
            t = ts[len(ts) // 2]
            out[f"{sym}_event_ms"] = round(1e3 * t, 4)
            out[f"{sym}_tflops"] = N * flop / t / 1e12
            out[f"{sym}_share_of_f32_matrix_peak"] = N * flop / t / PEAK_F32_MFMA
    out["version"] = zuko_amd.__version__
    print(json.dumps(out))


if __name__ == "__main__":
    main()
