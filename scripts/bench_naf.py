r"""NAF(64, transforms=3): `log_prob` at batch 2^16 and sampling at batch 2^14 on one GPU, the monotone-network kernels (zk_mnn_forward /
zk_mnn_inverse) against the torch-op restatement of the same expressions (zuko_amd.ops.MNN_KERNEL = False), alternating in one process.  Device events over >= 0.5 s of work per measurement after a warm-up.

    python scripts/bench_naf.py                 # prints one JSON line
    rocprofv3 --kernel-trace --stats -- python scripts/bench_naf.py --trace     # per-launch kernel times (kernel path only, few calls)
    python scripts/bench_naf.py --train [--out FILE]      # the training step: Adam at batch 2^14 and 2^16, the adjoint kernel (zk_mnn_backward)
                                                          # against ops.MNN_ADJOINT = False (the torch-op double backward), alternating
    rocprofv3 --kernel-trace --stats -- python scripts/bench_naf.py --trace-train    # per-launch times of the training step's kernels

FLOP per forward element from the shapes: 2 [(1 + S) H1 + 2 sum_l H_l H_{l+1} + 2 H_last] (value and tangent share |W_l|; the tangent skips
the first layer) = 18 816 for S = 16, hidden (64, 64).  The f32 matrix instruction's peak is 157.3 TFLOP/s; the kernel moves 72 bytes per
element, so its bound is compute.

FLOP per adjoint element: the forward again (it is recomputed), per hidden-to-hidden layer two outer products and two transposed products of
2 H_l H_{l+1} each, the signal's outer product and transposed product of 2 S H1 each, and the first layer's x column and the last layer
(4 H1 + 6 H_last) = 18 816 + 8 * 4096 + 4 * 16 * 64 + 256 + 384 = 56 320 for the default network."""

from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import zuko_amd
from zuko_amd import _C, ops
from zuko_amd.flows import NAF

PEAK_F32_MATRIX = 157.3e12


def flop_per_element(S: int, hidden) -> int:
    h = list(hidden)
    return 2 * ((1 + S) * h[0] + 2 * sum(a * b for a, b in zip(h[:-1], h[1:])) + 2 * h[-1])


def adjoint_flop_per_element(S: int, hidden) -> int:
    h = list(hidden)
    return flop_per_element(S, hidden) + 8 * sum(a * b for a, b in zip(h[:-1], h[1:])) + 4 * S * h[0] + 4 * h[0] + 6 * h[-1]


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


def train(trace: bool) -> None:
    """One optimisation step (loss, zero_grad, backward, Adam) of NAF(64, transforms=3) at batch 2^14 and 2^16: the adjoint kernel against
    ops.MNN_ADJOINT = False, which is what every call that needs gradients ran before zk_mnn_backward existed."""
    dev = torch.device("cuda:0")
    D, T, S, hidden = 64, 3, 16, (64, 64)
    torch.manual_seed(0)
    flow = NAF(D, transforms=T).to(dev)
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(1)
    data = {n: torch.randn(n, D, generator=g).to(dev) for n in (2**14, 2**16)}

    def step(n, on):
        def run():
            ops.MNN_ADJOINT = on
            try:
                loss = -flow().log_prob(data[n]).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss
            finally:
                ops.MNN_ADJOINT = True

        return run

    if trace:
        for n in data:
            for _ in range(3):
                step(n, True)()
        torch.cuda.synchronize()
        return
    out = {"workload": f"training step (Adam) of NAF({D}, transforms={T}), signal {S}, hidden {hidden}", "batches": list(data)}
    # the two paths' gradients on the same parameters
    grads = {}
    for on in (True, False):
        ops.MNN_ADJOINT = on
        flow.zero_grad(set_to_none=True)
        (-flow().log_prob(data[2**14]).mean()).backward()
        grads[on] = [p.grad.clone() for p in flow.parameters()]
    ops.MNN_ADJOINT = True
    out["grad_max_abs_diff_over_max_abs_grad"] = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads[True], grads[False]))
    for n in data:
        res = {}
        for rnd in range(2):  # alternate: neither path sees a systematically warmer or cooler device
            for name, on in (("kernel", True), ("torch", False)):
                res.setdefault(name, []).append(timed(step(n, on)))
        for name, runs in res.items():
            out[f"step_{n}_{name}"] = min(runs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in runs]}
        out[f"step_{n}_speedup"] = out[f"step_{n}_torch"]["median_ms"] / out[f"step_{n}_kernel"]["median_ms"]
        out[f"step_{n}_kernel_samples_per_s"] = n / (out[f"step_{n}_kernel"]["median_ms"] * 1e-3)
        # per-call time of the adjoint by events around the entry point (kernel + memset + chunk reduction; the kernel-trace run separates them)
        _C.PROFILE = {}
        step(n, True)()
        torch.cuda.synchronize()
        calls = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_mnn_backward", [])]
        _C.PROFILE = None
        flop = adjoint_flop_per_element(S, hidden) * n * D
        out[f"zk_mnn_backward_{n}_call_ms"] = [round(1e3 * t, 4) for t in calls]
        if calls:
            out[f"zk_mnn_backward_{n}_tflops"] = flop / min(calls) / 1e12
            out[f"zk_mnn_backward_{n}_share_of_f32_matrix_peak"] = flop / min(calls) / PEAK_F32_MATRIX
    out["adjoint_flop_per_element"] = adjoint_flop_per_element(S, hidden)
    # the other instantiations of the adjoint (three hidden layers, a wide signal) at batch 2^14: medians of two alternating rounds per path
    del flow, opt
    other = {}
    for S2, hidden2 in [(16, (64, 64, 64)), (63, (64, 64, 64)), (63, (64, 64))]:
        torch.manual_seed(0)
        flow2 = NAF(D, transforms=T, signal=S2, network={"hidden_features": hidden2}).to(dev)
        opt2 = torch.optim.Adam(flow2.parameters(), lr=1e-3)

        def step2(on):
            def run():
                ops.MNN_ADJOINT = on
                try:
                    loss = -flow2().log_prob(data[2**14]).mean()
                    opt2.zero_grad()
                    loss.backward()
                    opt2.step()
                finally:
                    ops.MNN_ADJOINT = True

            return run

        res = {}
        for rnd in range(2):
            for name, on in (("kernel", True), ("torch", False)):
                res.setdefault(name, []).append(round(timed(step2(on))["median_ms"], 3))
        other[f"signal {S2}, hidden {hidden2}"] = res | {"speedup": min(res["torch"]) / min(res["kernel"])}
    out["step_16384_other_shapes_medians_ms"] = other
    out["peak_memory_gib"] = torch.cuda.max_memory_allocated() / 2**30
    out["version"] = zuko_amd.__version__
    line = json.dumps(out)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    print(line)


def main() -> None:
    if "--train" in sys.argv or "--trace-train" in sys.argv:
        return train("--trace-train" in sys.argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    D, T, S, hidden = 64, 3, 16, (64, 64)
    flow = NAF(D, transforms=T).to(dev).requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2**16, D, generator=g).to(dev)
    n_sample = 2**14

    def log_prob():
        with torch.no_grad():
            return flow().log_prob(x)

    def sample():
        with torch.no_grad():
            return flow().sample((n_sample,))

    def with_kernel(on, fn):
        def run():
            ops.MNN_KERNEL = on
            try:
                return fn()
            finally:
                ops.MNN_KERNEL = True

        return run

    if "--trace" in sys.argv:
        for _ in range(3):
            log_prob()
        sample()
        torch.cuda.synchronize()
        return
    out = {"workload": f"NAF({D}, transforms={T}), signal {S}, hidden {hidden}", "log_prob_batch": x.shape[0], "sample_batch": n_sample}
    lp_k, lp_t = with_kernel(True, log_prob)(), with_kernel(False, log_prob)()
    out["log_prob_max_abs_diff_kernel_vs_torch"] = float((lp_k - lp_t).abs().max())
    # alternate the two paths (two rounds each): neither sees a systematically warmer or cooler device
    res = {}
    for rnd in range(2):
        for name, on in (("kernel", True), ("torch", False)):
            res.setdefault(("log_prob", name), []).append(timed(with_kernel(on, log_prob)))
    for name, on in (("kernel", True), ("torch", False)):
        res[("sample", name)] = [timed(with_kernel(on, sample), warmup=1)]
    for (what, name), runs in res.items():
        out[f"{what}_{name}"] = min(runs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in runs]}
    out["log_prob_speedup"] = out["log_prob_torch"]["median_ms"] / out["log_prob_kernel"]["median_ms"]
    out["sample_speedup"] = out["sample_torch"]["median_ms"] / out["sample_kernel"]["median_ms"]
    # per-launch time of the forward kernel by events around the entry point (the kernel-trace run gives the same without the launch gap)
    _C.PROFILE = {}
    log_prob()
    torch.cuda.synchronize()
    launches = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_mnn_forward", [])]
    _C.PROFILE = None
    flop = flop_per_element(S, hidden) * x.shape[0] * D
    out["flop_per_element"] = flop_per_element(S, hidden)
    out["zk_mnn_forward_launch_ms"] = [round(1e3 * t, 4) for t in launches]
    if launches:
        out["zk_mnn_forward_tflops"] = flop / min(launches) / 1e12
        out["zk_mnn_forward_share_of_f32_matrix_peak"] = flop / min(launches) / PEAK_F32_MATRIX
    out["bound"] = "compute (18.8 kFLOP against 72 B per element)"
    out["version"] = zuko_amd.__version__
    print(json.dumps(out))


if __name__ == "__main__":
    main()
