r"""UNAF(64, transforms=3): `log_prob` at batch 2^16 and sampling at batch 2^12 on one GPU, the unconstrained-monotone-network kernels
(zk_umnn_forward / zk_umnn_inverse) against the torch-op restatement of the same expressions (zuko_amd.ops.UMNN_KERNEL = False: the
reference's algorithm on ATen kernels, what a call that needs gradients runs), alternating in one process.  Device events after a warm-up.

    python scripts/bench_unaf.py                 # prints one JSON line
    rocprofv3 --kernel-trace --stats -- python scripts/bench_unaf.py --trace     # per-launch kernel times (kernel path only, few calls)
    python scripts/bench_unaf.py --train [--out FILE]     # the training step: Adam at batch 2^14 and 2^16, the adjoint kernel (zk_umnn_backward)
                                                          # against ops.UMNN_ADJOINT = False (the quadrature under autograd), alternating
    rocprofv3 --kernel-trace --stats -- python scripts/bench_unaf.py --trace-train   # per-launch times of the training step's kernels

FLOP per element from the shapes: the signal's share of the first layer once, 2 S H1, and per evaluation of the integrand network
2 (H1 + sum_l H_l H_{l+1} + H_last); for S = 16, hidden (64, 64): 2 048 + 33 x 8 448 forward (32 nodes and the log-derivative's point),
2 048 + 25 x 32 x 8 448 inverse.  The f32 matrix instruction's peak is 157.3 TFLOP/s; the forward kernel moves 80 bytes per element, so its
bound is compute.  The torch-op path of `log_prob` holds [32, N, D, H] activations: where it does not fit the device at the full batch it is
measured at a smaller one and scaled by rows (recorded in the output); the training step follows the same rule.

FLOP per adjoint element: the signal's product three times (forward, outer product, transposed product), 6 S H1, and per point (32 nodes and x)
the forward again plus, per hidden-to-hidden layer, one outer product and one transposed product of 2 H_l H_{l+1} each:
6 S H1 + 33 [2 (H1 + sum_l H_l H_{l+1} + H_last) + 4 sum_l H_l H_{l+1}] = 2 048 x 3 + 33 x (8 448 + 2 x 8 192) = 825 600 for the default network
(the first layer's x column and the last layer's gradient, 6 H per point, are left out)."""

from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import zuko_amd
from zuko_amd import _C, ops
from zuko_amd.flows import UNAF

PEAK_F32_MATRIX = 157.3e12


def flop_per_element(S: int, hidden, evaluations: int) -> int:
    h = list(hidden)
    return 2 * S * h[0] + evaluations * 2 * (h[0] + sum(a * b for a, b in zip(h[:-1], h[1:])) + h[-1])


def adjoint_flop_per_element(S: int, hidden, evaluations: int) -> int:
    h = list(hidden)
    return flop_per_element(S, hidden, evaluations) + 4 * S * h[0] + evaluations * 4 * sum(a * b for a, b in zip(h[:-1], h[1:]))


def timed(fn, min_seconds: float = 0.5, warmup: int = 1, min_calls: int = 3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    total = 0.0
    while total < min_seconds or len(times) < min_calls:
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
    """One optimisation step (loss, zero_grad, backward, Adam) of UNAF(64, transforms=3) at batch 2^14 and 2^16: the adjoint kernel against
    ops.UMNN_ADJOINT = False, which is what every call that needs gradients ran before zk_umnn_backward existed."""
    dev = torch.device("cuda:0")
    D, T, S, hidden, n_quad = 64, 3, 16, (64, 64), 32
    g = torch.Generator().manual_seed(1)
    data = {n: torch.randn(n, D, generator=g).to(dev) for n in (2**14, 2**16)}

    def stepper(flow, opt):
        def step(n, on, rows=None):
            def run():
                ops.UMNN_ADJOINT = on
                try:
                    loss = -flow().log_prob(data[n] if rows is None else data[n][:rows]).mean()
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
                    return loss
                finally:
                    ops.UMNN_ADJOINT = True

            return run

        return step

    def torch_rows(step, n):
        """The batch the torch-op step runs at: n, or the largest power of two below it that fits the device."""
        rows = n
        while True:
            try:
                step(n, False, rows)()
                torch.cuda.synchronize()
                return rows
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
                rows //= 2

    torch.manual_seed(0)
    flow = UNAF(D, transforms=T).to(dev)
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    step = stepper(flow, opt)
    if trace:
        for n in data:
            for _ in range(3):
                step(n, True)()
        torch.cuda.synchronize()
        return
    out = {"workload": f"training step (Adam) of UNAF({D}, transforms={T}), signal {S}, hidden {hidden}, {n_quad} nodes", "batches": list(data)}
    # the two paths' gradients on the same parameters
    grads = {}
    rows_grad = torch_rows(step, 2**14)
    for on in (True, False):
        ops.UMNN_ADJOINT = on
        flow.zero_grad(set_to_none=True)
        (-flow().log_prob(data[2**14][:rows_grad]).mean()).backward()
        grads[on] = [p.grad.clone() for p in flow.parameters()]
    ops.UMNN_ADJOINT = True
    out["grad_rows"] = rows_grad
    out["grad_max_abs_diff_over_max_abs_grad"] = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(grads[True], grads[False]))
    del grads
    for n in data:
        rows = torch_rows(step, n)
        out[f"step_{n}_torch_rows"] = rows
        res = {}
        for rnd in range(2):  # alternate: neither path sees a systematically warmer or cooler device
            res.setdefault("kernel", []).append(timed(step(n, True), warmup=2))
            res.setdefault("torch", []).append(timed(step(n, False, rows), min_seconds=0.0, warmup=0, min_calls=2))
        for name, runs in res.items():
            out[f"step_{n}_{name}"] = min(runs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in runs]}
        out[f"step_{n}_torch_scaled_to_full_batch_ms"] = out[f"step_{n}_torch"]["median_ms"] * (n / rows)
        out[f"step_{n}_speedup"] = out[f"step_{n}_torch_scaled_to_full_batch_ms"] / out[f"step_{n}_kernel"]["median_ms"]
        out[f"step_{n}_kernel_samples_per_s"] = n / (out[f"step_{n}_kernel"]["median_ms"] * 1e-3)
        # per-call time of the adjoint by events around the entry point (kernel + memset + chunk reduction; the kernel-trace run separates them)
        _C.PROFILE = {}
        step(n, True)()
        torch.cuda.synchronize()
        calls = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_umnn_backward", [])]
        fwd = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_umnn_forward", [])]
        _C.PROFILE = None
        flop = adjoint_flop_per_element(S, hidden, n_quad + 1) * n * D
        out[f"zk_umnn_backward_{n}_call_ms"] = [round(1e3 * t, 4) for t in calls]
        out[f"zk_umnn_forward_{n}_call_ms"] = [round(1e3 * t, 4) for t in fwd]
        if calls:
            out[f"zk_umnn_backward_{n}_tflops"] = flop / min(calls) / 1e12
            out[f"zk_umnn_backward_{n}_share_of_f32_matrix_peak"] = flop / min(calls) / PEAK_F32_MATRIX
    out["adjoint_flop_per_element"] = adjoint_flop_per_element(S, hidden, n_quad + 1)
    # the other instantiations of the adjoint (three hidden layers, a wide signal) at batch 2^14: medians of two alternating rounds per path
    del flow, opt, step
    torch.cuda.empty_cache()
    other = {}
    for S2, hidden2 in [(16, (64, 64, 64)), (63, (64, 64, 64)), (63, (64, 64))]:
        torch.manual_seed(0)
        flow2 = UNAF(D, transforms=T, signal=S2, network={"hidden_features": hidden2}).to(dev)
        step2 = stepper(flow2, torch.optim.Adam(flow2.parameters(), lr=1e-3))
        n = 2**14
        rows = torch_rows(step2, n)
        res = {"torch_rows": rows}
        for rnd in range(2):
            res.setdefault("kernel", []).append(round(timed(step2(n, True), warmup=2)["median_ms"], 3))
            res.setdefault("torch", []).append(round(timed(step2(n, False, rows), min_seconds=0.0, warmup=0, min_calls=2)["median_ms"] * (n / rows), 3))
        other[f"signal {S2}, hidden {hidden2}"] = res | {"speedup": min(res["torch"]) / min(res["kernel"])}
        del flow2, step2
        torch.cuda.empty_cache()
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
    D, T, S, hidden, n_quad, n_bisect = 64, 3, 16, (64, 64), 32, 25
    flow = UNAF(D, transforms=T).to(dev).requires_grad_(False)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2**16, D, generator=g).to(dev)
    n_sample = 2**12

    def log_prob(rows=None):
        with torch.no_grad():
            return flow().log_prob(x if rows is None else x[:rows])

    def sample():
        with torch.no_grad():
            return flow().sample((n_sample,))

    def with_kernel(on, fn):
        def run():
            ops.UMNN_KERNEL = on
            try:
                return fn()
            finally:
                ops.UMNN_KERNEL = True

        return run

    if "--trace" in sys.argv:
        for _ in range(3):
            log_prob()
        sample()
        torch.cuda.synchronize()
        return
    out = {"workload": f"UNAF({D}, transforms={T}), signal {S}, hidden {hidden}, {n_quad} nodes", "log_prob_batch": x.shape[0], "sample_batch": n_sample}
    # the torch-op path at the full batch, or at the largest power of two below it that fits the device
    rows = x.shape[0]
    while True:
        try:
            lp_t = with_kernel(False, lambda: log_prob(rows))()
            torch.cuda.synchronize()
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            rows //= 2
    out["log_prob_torch_rows"] = rows
    lp_k = with_kernel(True, log_prob)()
    out["log_prob_max_abs_diff_kernel_vs_torch"] = float((lp_k[:rows] - lp_t).abs().max())
    del lp_t
    # alternate the two paths (two rounds each): neither sees a systematically warmer or cooler device
    res = {}
    for rnd in range(2):
        res.setdefault(("log_prob", "kernel"), []).append(timed(with_kernel(True, log_prob)))
        res.setdefault(("log_prob", "torch"), []).append(timed(with_kernel(False, lambda: log_prob(rows)), min_seconds=0.0, warmup=0, min_calls=2))
    res[("sample", "kernel")] = [timed(with_kernel(True, sample))]
    res[("sample", "torch")] = [timed(with_kernel(False, sample), min_seconds=0.0, warmup=0, min_calls=2)]
    for (what, name), runs in res.items():
        out[f"{what}_{name}"] = min(runs, key=lambda r: r["median_ms"]) | {"medians_ms": [round(r["median_ms"], 3) for r in runs]}
    scale = x.shape[0] / rows  # (1 when the torch-op path ran at the full batch)
    out["log_prob_torch_scaled_to_full_batch_ms"] = out["log_prob_torch"]["median_ms"] * scale
    out["log_prob_speedup"] = out["log_prob_torch_scaled_to_full_batch_ms"] / out["log_prob_kernel"]["median_ms"]
    out["sample_speedup"] = out["sample_torch"]["median_ms"] / out["sample_kernel"]["median_ms"]
    # per-launch times by events around the entry points (the kernel-trace run gives the same without the launch gap)
    _C.PROFILE = {}
    log_prob()
    sample()
    torch.cuda.synchronize()
    fwd = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_umnn_forward", [])]
    inv = [a.elapsed_time(b) * 1e-3 for a, b, _ in _C.PROFILE.get("zk_umnn_inverse", [])]
    _C.PROFILE = None
    f_fwd, f_inv = flop_per_element(S, hidden, n_quad + 1), flop_per_element(S, hidden, n_bisect * n_quad)
    out["flop_per_element_forward"], out["flop_per_element_inverse"] = f_fwd, f_inv
    out["zk_umnn_forward_launch_ms"] = [round(1e3 * t, 4) for t in fwd]
    if fwd:
        out["zk_umnn_forward_tflops"] = f_fwd * x.shape[0] * D / min(fwd) / 1e12
        out["zk_umnn_forward_share_of_f32_matrix_peak"] = out["zk_umnn_forward_tflops"] * 1e12 / PEAK_F32_MATRIX
    if inv:
        inv.sort()
        med = inv[len(inv) // 2]  # (one launch per feature of a sweep: n_sample x 1 elements)
        out["zk_umnn_inverse_launches"], out["zk_umnn_inverse_launch_median_ms"] = len(inv), round(1e3 * med, 4)
        out["zk_umnn_inverse_tflops"] = f_inv * n_sample / med / 1e12
        out["zk_umnn_inverse_share_of_f32_matrix_peak"] = out["zk_umnn_inverse_tflops"] * 1e12 / PEAK_F32_MATRIX
    out["bound"] = "compute (281 kFLOP against 80 B per forward element)"
    out["version"] = zuko_amd.__version__
    print(json.dumps(out))


if __name__ == "__main__":
    main()
