r"""CNF(features=5, context=3), hidden (64, 64): `log_prob` at batch 2^16 and sampling at batch 2^14 on one GPU, the fused Dormand-Prince step kernel
(zk_cnf_step) against the torch-op path of the same integration (zuko_amd.ops.CNF_KERNEL = False: what a call that needs gradients runs — seven
field evaluations per attempted step, each with a batched autograd Jacobian for the trace), alternating in one process.  Device events over
>= 0.5 s of work per measurement after a warm-up.  The kernel path's attempt counts are in the output.

    python scripts/bench_cnf.py                 # prints one JSON line
    rocprofv3 --kernel-trace --stats -- python scripts/bench_cnf.py --trace     # per-launch kernel times (kernel path only, few calls)
    python scripts/bench_cnf.py --train         # one JSON line: an Adam step at batch 2^14 and 2^16 with ops.CNF_ADJOINT on and off
    rocprofv3 --kernel-trace --stats -- python scripts/bench_cnf.py --train --trace   # per-launch times of the adjoint kernel (kernel path only)
    python scripts/bench_cnf.py --exact-false [--train] [--trace]     # Hutchinson's estimator (exact=False): see below

`--exact-false`: CNF(5, 3) and the 16-feature CNF(16, 3, hidden (64, 64)) with exact=False, `log_prob` at batch 2^16 (with `--train`: an Adam step at
batch 2^14 and 2^16), three ways in one process: ops.CNF_HUTCHINSON on (with `--train` ops.CNF_ADJOINT too: the probe variant of the kernels), both
switches off (the torch-op path an exact=False flow takes by default, and took before the switch existed), and the exact=True flow of the same shape on
the exact kernels.  ZUKO_AMD_BENCH_ROOT=<another checkout> measures that checkout's package instead; one without the switch reports the two rows it has.

`--train`: the loss is -log_prob(x).mean(); a step is zero_grad, forward, backward, Adam.  With the switch on the forward runs on zk_cnf_step and the
backward makes one zk_cnf_adjoint_step per accepted step; with it off (the default) both run in torch ops — the code path of the parent commit.

FLOP per row and attempted step from the shapes, seven stages each: the value 2 [(2 Q + F) H1 + sum_l H_l H_{l+1} + H_last F] (the context's share
of the first layer is one GEMM per integration, not counted) and F tangents of 2 [sum_l H_l H_{l+1} + H_last] each (a tangent enters the first
layer as a column, and meets one row of the last) = 362 880 for F = 5, Q = 3, hidden (64, 64).  The f32 matrix instruction's peak is 157.3
TFLOP/s; a row moves 120 bytes plus its 256-byte `pre` row per step, so the bound is compute."""

from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.environ.get("ZUKO_AMD_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import zuko_amd
from zuko_amd import _C, ops
from zuko_amd.flows import CNF

PEAK_F32_MATRIX = 157.3e12


def flop_per_row_step(F: int, Q: int, hidden, tangents: bool = True) -> int:
    h = list(hidden)
    inner = sum(a * b for a, b in zip(h[:-1], h[1:]))
    value = 2 * ((2 * Q + F) * h[0] + inner + h[-1] * F)
    return 7 * (value + (F * 2 * (inner + h[-1]) if tangents else 0))


def timed(fn, min_seconds: float = 0.5, warmup: int = 2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    total = 0.0
    while total < min_seconds or len(times) < 3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
        total += times[-1]
    times.sort()
    return {"median_ms": 1e3 * times[len(times) // 2], "min_ms": 1e3 * times[0], "max_ms": 1e3 * times[-1], "calls": len(times)}


def train_main() -> None:
    dev = torch.device("cuda:0")
    F, C, Q, hidden = 5, 3, 3, (64, 64)
    g = torch.Generator().manual_seed(1)
    X, Cx = torch.randn(2**16, F, generator=g).to(dev), torch.randn(2**16, C, generator=g).to(dev)

    def stepper(on: bool, n: int):
        torch.manual_seed(0)
        flow = CNF(F, C).to(dev).train()
        opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
        x, c = X[:n], Cx[:n]
        stats = {}

        def step():
            ops.CNF_ADJOINT = on
            try:
                opt.zero_grad(set_to_none=True)
                loss = -flow(c).log_prob(x).mean()
                stats.update(ops.CNF_STATS)
                loss.backward()
                stats.update(ops.CNF_STATS)
                opt.step()
            finally:
                ops.CNF_ADJOINT = False
            return loss

        return flow, step, stats

    if "--trace" in sys.argv:
        for n in (2**14, 2**16):
            _, step, _ = stepper(True, n)
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        return
    out = {"workload": f"Adam step of CNF({F}, {C}), freqs {Q}, hidden {hidden}, loss -log_prob.mean(), weights as initialised (seed 0)", "version": zuko_amd.__version__}
    for n in (2**14, 2**16):
        key = f"batch_{n}"
        # the first step's gradients of the two paths on the same weights and data
        grads = {}
        for on in (True, False):
            flow, step, stats = stepper(on, n)
            ops.CNF_ADJOINT = on
            try:
                (-flow(Cx[:n]).log_prob(X[:n]).mean()).backward()
            finally:
                ops.CNF_ADJOINT = False
            grads[on] = torch.cat([p.grad.reshape(-1) for p in flow.parameters()])
        out[key + "_grad_max_abs_diff_over_max_abs"] = float((grads[True] - grads[False]).abs().max() / grads[False].abs().max())
        runs = {}
        steppers = {on: stepper(on, n) for on in (True, False)}
        for rnd in range(2):  # alternate the two paths: neither sees a systematically warmer or cooler device
            for on in (True, False):
                runs.setdefault(on, []).append(timed(steppers[on][1], min_seconds=1.0, warmup=2))
        for on, name in ((True, "adjoint_on"), (False, "adjoint_off")):
            best = min(runs[on], key=lambda r: r["median_ms"])
            st = steppers[on][2]
            out[f"{key}_{name}"] = best | {"medians_ms": [round(r["median_ms"], 3) for r in runs[on]], "path": st.get("path"),
                                           "last_step": {k: st[k] for k in ("attempts", "accepted", "adjoint_steps") if k in st}}
        out[key + "_speedup"] = out[f"{key}_adjoint_off"]["median_ms"] / out[f"{key}_adjoint_on"]["median_ms"]
        # events around the entry points over one step on the kernel path
        _C.PROFILE = {}
        steppers[True][1]()
        torch.cuda.synchronize()
        prof, _C.PROFILE = _C.PROFILE, None
        for sym in ("zk_cnf_step", "zk_cnf_adjoint_step"):
            ts = [a.elapsed_time(b) for a, b, _ in prof.get(sym, [])]
            out[f"{key}_{sym}_launch_ms"] = {"launches": len(ts), "mean": sum(ts) / max(len(ts), 1), "min": min(ts, default=0.0), "max": max(ts, default=0.0)}
    print(json.dumps(out))


def hutch_main() -> None:
    """exact=False on the probe kernels, on the torch-op path, and exact=True on the exact kernels, at two shapes."""
    dev = torch.device("cuda:0")
    train, trace = "--train" in sys.argv, "--trace" in sys.argv
    has_switch = hasattr(ops, "CNF_HUTCHINSON")
    g = torch.Generator().manual_seed(1)
    out = {"workload": ("Adam step, loss -log_prob.mean()" if train else "log_prob") + " of CNF(F, 3), freqs 3, hidden (64, 64), weights as initialised (seed 0)",
           "version": zuko_amd.__version__, "has_switch": has_switch}
    for F in (5, 16):
        X, Cx = torch.randn(2**16, F, generator=g).to(dev), torch.randn(2**16, 3, generator=g).to(dev)

        def runner(exact: bool, on: bool, n: int):
            torch.manual_seed(0)
            flow = CNF(F, 3, exact=exact).to(dev)
            flow = flow.train() if train else flow.eval().requires_grad_(False)
            opt = torch.optim.Adam(flow.parameters(), lr=1e-3) if train else None
            x, c = X[:n], Cx[:n]
            stats = {}

            def run():
                keep = ops.CNF_ADJOINT, getattr(ops, "CNF_HUTCHINSON", False)
                ops.CNF_ADJOINT = on and train
                if has_switch:
                    ops.CNF_HUTCHINSON = on
                try:
                    if not train:
                        with torch.no_grad():
                            lp = flow(c).log_prob(x)
                        stats.update(ops.CNF_STATS)
                        return lp
                    opt.zero_grad(set_to_none=True)
                    loss = -flow(c).log_prob(x).mean()
                    stats.update(ops.CNF_STATS)
                    loss.backward()
                    stats.update(ops.CNF_STATS)
                    opt.step()
                    return loss
                finally:
                    ops.CNF_ADJOINT = keep[0]
                    if has_switch:
                        ops.CNF_HUTCHINSON = keep[1]

            return run, stats

        for n in ((2**14, 2**16) if train else (2**16,)):
            rows = {"exact_kernels": (True, True), "hutchinson_off": (False, False)} | ({"hutchinson_on": (False, True)} if has_switch else {})
            if trace:  # the probe kernels alone, a few calls
                run, _ = runner(False, True, n)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                continue
            runs = {name: runner(exact, on, n) for name, (exact, on) in rows.items()}
            res = {}
            for rnd in range(2):  # alternate the paths: none sees a systematically warmer or cooler device
                for name, (run, _) in runs.items():
                    res.setdefault(name, []).append(timed(run, min_seconds=0.5, warmup=2))
            key = f"features_{F}_batch_{n}"
            for name, (run, st) in runs.items():
                best = min(res[name], key=lambda r: r["median_ms"])
                out[f"{key}_{name}"] = best | {"medians_ms": [round(r["median_ms"], 3) for r in res[name]],
                                               "last_call": {k: st[k] for k in ("path", "trace", "attempts", "accepted", "adjoint_steps") if k in st}}
            if has_switch:
                on = out[f"{key}_hutchinson_on"]["median_ms"]
                out[f"{key}_off_over_on"] = out[f"{key}_hutchinson_off"]["median_ms"] / on
                out[f"{key}_exact_over_on"] = out[f"{key}_exact_kernels"]["median_ms"] / on
                _C.PROFILE = {}
                runs["hutchinson_on"][0]()
                torch.cuda.synchronize()
                prof, _C.PROFILE = _C.PROFILE, None
                for sym in ("zk_cnf_step_v2", "zk_cnf_adjoint_step_v2"):
                    ts = [a.elapsed_time(b) for a, b, _ in prof.get(sym, [])]
                    if ts:
                        out[f"{key}_{sym}_launch_ms"] = {"launches": len(ts), "mean": sum(ts) / len(ts), "min": min(ts), "max": max(ts)}
    if not trace:
        print(json.dumps(out))


def main() -> None:
    if "--exact-false" in sys.argv:
        return hutch_main()
    if "--train" in sys.argv:
        return train_main()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    F, C, Q, hidden = 5, 3, 3, (64, 64)
    flow = CNF(F, C).to(dev).eval().requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    x, c = torch.randn(2**16, F, generator=g).to(dev), torch.randn(2**16, C, generator=g).to(dev)
    n_sample = 2**14
    cs = c[:n_sample]

    def log_prob():
        with torch.no_grad():
            return flow(c).log_prob(x)

    def sample():
        with torch.no_grad():
            return flow(cs).sample()

    def with_kernel(on, fn):
        def run():
            ops.CNF_KERNEL = on
            try:
                return fn()
            finally:
                ops.CNF_KERNEL = True

        return run

    if "--trace" in sys.argv:
        for _ in range(3):
            log_prob()
        sample()
        torch.cuda.synchronize()
        return
    out = {"workload": f"CNF({F}, {C}), freqs {Q}, hidden {hidden}, weights as initialised (seed 0)", "log_prob_batch": x.shape[0], "sample_batch": n_sample}
    lp_k = with_kernel(True, log_prob)()
    out["log_prob_attempts_kernel"] = {k: ops.CNF_STATS[k] for k in ("attempts", "accepted")}
    lp_t = with_kernel(False, log_prob)()
    out["log_prob_max_abs_diff_kernel_vs_torch"] = float((lp_k - lp_t).abs().max())
    # alternate the two paths (two rounds each): neither sees a systematically warmer or cooler device
    res = {}
    for rnd in range(2):
        for name, on in (("kernel", True), ("torch", False)):
            res.setdefault(("log_prob", name), []).append(timed(with_kernel(on, log_prob)))
    for name, on in (("kernel", True), ("torch", False)):
        res[("sample", name)] = [timed(with_kernel(on, sample), warmup=1)]
    with_kernel(True, sample)()
    out["sample_attempts_kernel"] = {k: ops.CNF_STATS[k] for k in ("attempts", "accepted")}
    for (what, name), runs in res.items():
        out[f"{what}_{name}"] = min(runs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in runs]}
    out["log_prob_speedup"] = out["log_prob_torch"]["median_ms"] / out["log_prob_kernel"]["median_ms"]
    out["sample_speedup"] = out["sample_torch"]["median_ms"] / out["sample_kernel"]["median_ms"]
    # per-launch time of the step kernel by events around the entry point (the kernel-trace run gives the same without the launch gap)
    _C.PROFILE = {}
    log_prob()
    torch.cuda.synchronize()
    launches = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_cnf_step", [])]
    _C.PROFILE = None
    flop = flop_per_row_step(F, Q, hidden) * x.shape[0]
    out["flop_per_row_step"] = flop_per_row_step(F, Q, hidden)
    out["zk_cnf_step_launch_ms"] = [round(1e3 * t, 4) for t in launches]
    if launches:
        out["zk_cnf_step_tflops"] = flop / min(launches) / 1e12
        out["zk_cnf_step_share_of_f32_matrix_peak"] = flop / min(launches) / PEAK_F32_MATRIX
    out["bound"] = "compute (363 kFLOP against under 400 B per row and step)"
    out["version"] = zuko_amd.__version__
    print(json.dumps(out))


if __name__ == "__main__":
    main()
