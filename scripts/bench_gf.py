r"""GF(features=64, transforms=3, components=8), unconditional (parameters [64, 8] shared by all rows) and conditional (context=16: the MLP emits one
packed [shift | scale] row per element), on one GPU: `log_prob` at batch 2^18 and one Adam training step at batch 2^16, the Gaussianization kernels
(zk_gauss_forward / zk_gauss_backward) against the torch-op restatement of the reference's expressions (zuko_amd.ops.GAUSS_KERNEL = False),
alternating in one process.  Device events over >= 0.5 s of work per measurement after a warm-up.

    python scripts/bench_gf.py                 # prints one JSON line
    rocprofv3 --kernel-trace --stats -- python scripts/bench_gf.py --trace     # per-launch kernel times (kernel path, few calls, a sample() for the inverse)
    python scripts/bench_gf.py --rows DIR      # the Gaussianization kernels' dispatches in the *_kernel_trace.csv under DIR, grouped (no GPU needed)
    python scripts/bench_gf.py --shared-adjoint   # the same line, plus the unconditional training step with ops.GAUSS_SHARED_ADJOINT on and off
                                                  # (step time, peak memory, zk_gauss_backward_shared per launch); with --trace: three such steps more

Rooflines.  Conditional forward: 4 + 8 K + 4 bytes per element (x, the packed parameters, y; ladj is one float per row) against 8 TB/s
of HBM.  Shared parameters: 2 K floats per feature stay in cache, the kernel is bound by its arithmetic: per element and component one exp (the scale), one
erfc and one exp (the log-sum-exp), reported as component evaluations per second."""

from __future__ import annotations

import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import zuko_amd
from zuko_amd import _C, ops
from zuko_amd.flows import GF

PEAK_HBM = 8.0e12
D, C, T, K = 64, 16, 3, 8
N_LOG_PROB, N_TRAIN = 2**18, 2**16
KERNELS = ("GaussOp", "gauss_backward", "gauss_shared_reduce")


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


def with_kernel(on, fn):
    def run():
        ops.GAUSS_KERNEL = on
        try:
            return fn()
        finally:
            ops.GAUSS_KERNEL = True

    return run


def workload(context: int, dev):
    torch.manual_seed(0)
    flow = GF(D, context=context, transforms=T, components=K).to(dev)
    opt = torch.optim.Adam(flow.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N_LOG_PROB, D, generator=g).to(dev)
    c = torch.randn(N_LOG_PROB, context, generator=g).to(dev) if context else None
    xt, ct = x[:N_TRAIN].contiguous(), (None if c is None else c[:N_TRAIN].contiguous())

    def log_prob():
        with torch.no_grad():
            return flow(c).log_prob(x)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = -flow(ct).log_prob(xt).mean()
        loss.backward()
        opt.step()
        return loss

    def sample():
        with torch.no_grad():
            return flow(ct).sample() if ct is not None else flow().sample((N_TRAIN,))

    return flow, log_prob, step, sample


def with_shared(on, fn):
    def run():
        ops.GAUSS_SHARED_ADJOINT = on
        try:
            return fn()
        finally:
            ops.GAUSS_SHARED_ADJOINT = False

    return run


def shared_adjoint(dev) -> dict:
    """--shared-adjoint: the unconditional training step with ops.GAUSS_SHARED_ADJOINT on and off, alternating (two rounds each); one step's peak of
    allocated memory over the level before it; the adjoint launches by events around the entry points."""
    _, _, step, _ = workload(0, dev)
    names = {True: "shared_on", False: "shared_off"}
    runs = {True: [], False: []}
    for rnd in range(2):
        for on in (True, False):
            runs[on].append(timed(with_shared(on, step)))
    res = {}
    for on, rs in runs.items():
        res[f"train_step_{names[on]}"] = min(rs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in rs]}
    res["train_step_shared_speedup"] = res["train_step_shared_off"]["median_ms"] / res["train_step_shared_on"]["median_ms"]
    for on in (True, False):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with_shared(on, step)()
        torch.cuda.synchronize()
        res[f"train_step_{names[on]}_peak_bytes"] = torch.cuda.max_memory_allocated()
        res[f"train_step_{names[on]}_peak_bytes_over_start"] = torch.cuda.max_memory_allocated() - before
        _C.PROFILE = {}
        with_shared(on, step)()
        torch.cuda.synchronize()
        prof, _C.PROFILE = _C.PROFILE, None
        for sym in ("zk_gauss_backward_shared", "zk_gauss_backward"):
            ts = [a.elapsed_time(b) * 1e-3 for a, b, _ in prof.get(sym, [])]
            if ts:
                res[f"{sym}_event_ms"] = round(1e3 * min(ts), 4)
                res[f"{sym}_component_evaluations_per_s"] = N_TRAIN * D * K * 2 / min(ts)
    return res


def kernel_rows(stats_dir: str) -> list:
    """The Gaussianization kernels' dispatches in a rocprofv3 --kernel-trace output directory, grouped by (kernel, grid): the grid tells the 2^18-row
    inference call from the 2^16-row training step; `us` keeps the dispatch order (--trace runs the unconditional flow first)."""
    groups = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if not any(k in r["Kernel_Name"] for k in KERNELS):
                    continue
                key = (r["Kernel_Name"], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0))
                groups.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3))
    out = []
    for (name, grid), calls in sorted(groups.items()):
        out.append({"kernel": name, "grid_threads": grid, "calls": len(calls), "us": [round(us, 2) for _, us in sorted(calls)]})
    return out


def main() -> None:
    if "--rows" in sys.argv:
        print(json.dumps(kernel_rows(sys.argv[sys.argv.index("--rows") + 1])))
        return
    dev = torch.device("cuda:0")
    if "--trace" in sys.argv:
        for context in (0, C):
            _, log_prob, step, sample = workload(context, dev)
            for _ in range(3):
                log_prob()
                step()
                sample()
                if "--shared-adjoint" in sys.argv and not context:
                    with_shared(True, step)()
        torch.cuda.synchronize()
        return
    out = {"workload": f"GF(features={D}, transforms={T}, components={K})", "log_prob_batch": N_LOG_PROB, "train_batch": N_TRAIN}
    for context in (0, C):
        flow, log_prob, step, sample = workload(context, dev)
        res = {"context": context}
        lp_k, lp_t = with_kernel(True, log_prob)(), with_kernel(False, log_prob)()
        res["log_prob_max_abs_diff_kernel_vs_torch"] = float((lp_k - lp_t).abs().max())
        del lp_k, lp_t
        runs = {}
        # alternate the two paths (two rounds each): neither sees a systematically warmer or cooler device
        for rnd in range(2):
            for name, on in (("kernel", True), ("torch", False)):
                runs.setdefault(("log_prob", name), []).append(timed(with_kernel(on, log_prob)))
                runs.setdefault(("train_step", name), []).append(timed(with_kernel(on, step)))
        for (what, name), rs in runs.items():
            res[f"{what}_{name}"] = min(rs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in rs]}
        for what in ("log_prob", "train_step"):
            res[f"{what}_speedup"] = res[f"{what}_torch"]["median_ms"] / res[f"{what}_kernel"]["median_ms"]
        # per-launch times by events around the entry points (the kernel-trace run gives the same without the launch gap)
        _C.PROFILE = {}
        log_prob()
        step()
        sample()
        torch.cuda.synchronize()
        prof, _C.PROFILE = _C.PROFILE, None
        for sym, n in (("zk_gauss_forward", N_LOG_PROB), ("zk_gauss_backward", N_TRAIN), ("zk_gauss_inverse", N_TRAIN)):
            ts = [a.elapsed_time(b) * 1e-3 for a, b, _ in prof.get(sym, [])]
            if not ts:
                continue
            # the first T zk_gauss_forward calls are the 2^18-row inference call; the training step's own forwards (2^16 rows) follow
            t = min(ts[:T]) if sym == "zk_gauss_forward" else min(ts)
            res[f"{sym}_event_ms"] = round(1e3 * t, 4)
            res[f"{sym}_component_evaluations_per_s"] = n * D * K * (25 if sym == "zk_gauss_inverse" else 2 if sym == "zk_gauss_backward" else 1) / t
            if context and sym != "zk_gauss_inverse":
                per_element = (4 + 8 * K + 4) if sym == "zk_gauss_forward" else (4 + 8 * K + 4 + 4 + 8 * K)  # backward: x, phi, gy in; gx, gphi out (gl per row)
                res[f"{sym}_event_share_of_hbm_peak"] = per_element * n * D / t / PEAK_HBM
        out["conditional" if context else "unconditional"] = res
        del flow
        torch.cuda.empty_cache()
    if "--shared-adjoint" in sys.argv:
        out["unconditional"]["shared_adjoint"] = shared_adjoint(dev)
    out["version"] = zuko_amd.__version__
    print(json.dumps(out))


if __name__ == "__main__":
    main()
