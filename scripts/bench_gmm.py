r"""GMM(features=8, context=16, components=8, hidden_features=(256, 256)), full and diagonal covariance, on one GPU: `log_prob` at batch 2^18 and one
Adam training step at batch 2^16, the mixture kernels (zk_gmm_log_prob / zk_gmm_backward) against the torch-op restatement of the reference's
expressions (zuko_amd.ops.GMM_KERNEL = False), alternating in one process.  Device events over >= 0.5 s of work per measurement after a warm-up.

    python scripts/bench_gmm.py                 # prints one JSON line
    rocprofv3 --kernel-trace --stats -- python scripts/bench_gmm.py --trace [full | diagonal]     # per-launch kernel times (kernel path, few calls)
    python scripts/bench_gmm.py --rows DIR      # the gmm kernels' dispatches in the *_kernel_trace.csv under DIR, grouped, with their bandwidth (no GPU needed)

Traffic model, bytes per row in float32: zk_gmm_log_prob reads phi and x once and writes one value, 4 (total + D + 1);
zk_gmm_backward reads phi twice (the pass that finds the responsibilities, the pass that writes gradients), x and g once, and writes gphi and gx:
4 (3 total + 2 D + 1).  Full covariance at D = K = 8: total = 360, 1 476 B and 4 388 B per row.  Peak HBM bandwidth: 8 TB/s."""

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
from zuko_amd.mixtures import GMM

PEAK_HBM = 8.0e12
D, C, K, HIDDEN = 8, 16, 8, (256, 256)
N_LOG_PROB, N_TRAIN = 2**18, 2**16


def bytes_per_row(total: int, backward: bool) -> int:
    return 4 * (3 * total + 2 * D + 1) if backward else 4 * (total + D + 1)


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
        ops.GMM_KERNEL = on
        try:
            return fn()
        finally:
            ops.GMM_KERNEL = True

    return run


def workload(cov: str, dev):
    torch.manual_seed(0)
    model = GMM(features=D, context=C, components=K, covariance_type=cov, hidden_features=HIDDEN).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(1)
    x, c = torch.randn(N_LOG_PROB, D, generator=g).to(dev), torch.randn(N_LOG_PROB, C, generator=g).to(dev)
    xt, ct = x[:N_TRAIN].contiguous(), c[:N_TRAIN].contiguous()

    def log_prob():
        with torch.no_grad():
            return model(c).log_prob(x)

    def density_only(phi):
        with torch.no_grad():
            return ops.gmm_log_prob(x, phi, K, cov, False, 1e-6)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = -model(ct).log_prob(xt).mean()
        loss.backward()
        opt.step()
        return loss

    return model, log_prob, density_only, step, (x, c)


def kernel_rows(stats_dir: str) -> list:
    """The gmm kernels' dispatches in a rocprofv3 --kernel-trace output directory, grouped by (kernel, grid): the grid tells the 2^18-row inference call
    from the 2^16-row training step.  The trace does not report dynamic LDS, so nothing in a row tells full from diagonal covariance: --trace runs full
    covariance first, and `us` keeps the dispatch order (or trace one covariance at a time: --trace full / --trace diagonal)."""
    groups = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                if "gmm_" not in r["Kernel_Name"]:
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
        rest = sys.argv[sys.argv.index("--trace") + 1 :]
        for cov in rest[:1] if rest and rest[0] in ("full", "diagonal") else ("full", "diagonal"):
            _, log_prob, _, step, _ = workload(cov, dev)
            for _ in range(3):
                log_prob()
                step()
        torch.cuda.synchronize()
        return
    out = {"workload": f"GMM(features={D}, context={C}, components={K}, hidden_features={HIDDEN})", "log_prob_batch": N_LOG_PROB, "train_batch": N_TRAIN}
    for cov in ("full", "diagonal"):
        model, log_prob, density_only, step, (x, c) = workload(cov, dev)
        res = {"total": model.total, "bytes_per_row_log_prob": bytes_per_row(model.total, False), "bytes_per_row_backward": bytes_per_row(model.total, True)}
        lp_k, lp_t = with_kernel(True, log_prob)(), with_kernel(False, log_prob)()
        res["log_prob_max_abs_diff_kernel_vs_torch"] = float((lp_k - lp_t).abs().max())
        with torch.no_grad():
            phi = model.hyper(c)
        runs = {}
        # alternate the two paths (two rounds each): neither sees a systematically warmer or cooler device
        for rnd in range(2):
            for name, on in (("kernel", True), ("torch", False)):
                runs.setdefault(("log_prob", name), []).append(timed(with_kernel(on, log_prob)))
                runs.setdefault(("density_only", name), []).append(timed(with_kernel(on, lambda: density_only(phi))))
                runs.setdefault(("train_step", name), []).append(timed(with_kernel(on, step)))
        for (what, name), rs in runs.items():
            res[f"{what}_{name}"] = min(rs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in rs]}
        for what in ("log_prob", "density_only", "train_step"):
            res[f"{what}_speedup"] = res[f"{what}_torch"]["median_ms"] / res[f"{what}_kernel"]["median_ms"]
        # per-launch times by events around the entry points (the kernel-trace run gives the same without the launch gap)
        _C.PROFILE = {}
        log_prob()
        step()
        torch.cuda.synchronize()
        for sym, n, bwd in (("zk_gmm_log_prob", N_LOG_PROB, False), ("zk_gmm_backward", N_TRAIN, True)):
            ts = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get(sym, [])]
            # the first zk_gmm_log_prob is the 2^18 inference call; the training step's own forward (2^16 rows) follows it
            if ts:
                t = ts[0] if not bwd else min(ts)
                res[f"{sym}_event_ms"] = round(1e3 * t, 4)
                res[f"{sym}_event_share_of_hbm_peak"] = bytes_per_row(model.total, bwd) * n / t / PEAK_HBM
        _C.PROFILE = None
        out[cov] = res
        del model, phi
    out["version"] = zuko_amd.__version__
    print(json.dumps(out))


if __name__ == "__main__":
    main()
