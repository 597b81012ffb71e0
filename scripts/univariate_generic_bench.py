"""Device-event timing of the run-time-count paths of the stand-alone univariate kernels at 2^16 x 64 (float32, packed parameters):
RQS K = 5, Bernstein NC = 9 (unbounded M = 7) and SOS 2 x 3, forward and inverse; and of the float32 backward of the K = 8 spline and the affine map.

    python scripts/univariate_generic_bench.py [--root DIR] [--repeats R]      # DIR: the checkout whose zuko_amd is imported (default: this one)

Prints one JSON line: per entry the median, minimum and maximum of R timed launches (ms) after 3 warm-up launches."""

import json
import os
import sys


def main(root: str, repeats: int) -> None:
    sys.path.insert(0, root)
    import torch

    from zuko_amd import ops
    from zuko_amd.utils import unpack

    dev = torch.device("cuda:0")
    N, D = 2**16, 64
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(N, D, generator=g) * 2.0).to(dev)
    phi5 = torch.randn(N, D, 14, generator=g).to(dev)
    w5, h5, d5 = unpack(phi5, [(5,), (5,), (4,)])
    theta = torch.randn(N, D, 7, generator=g).to(dev)
    a = torch.randn(N, D, 2, 3, generator=g).to(dev)
    phi8 = torch.randn(N, D, 23, generator=g).to(dev)
    phi2 = torch.randn(N, D, 2, generator=g).to(dev)
    gy, gl = torch.randn(N, D, generator=g).to(dev), torch.randn(N, D, generator=g).to(dev)

    def backward_of(phi, split, fwd):
        p = phi.clone().requires_grad_()
        xx = x.clone().requires_grad_()
        y, ladj = fwd(xx, p, split(p))
        loss = (y * gy).sum() + (ladj * gl).sum()
        return lambda: torch.autograd.grad(loss, (xx, p), retain_graph=True)

    entries = {
        "rqs_K5_forward": lambda: ops.rqs_forward(x, w5, h5, d5),
        "rqs_K5_inverse": lambda: ops.rqs_inverse(x, w5, h5, d5),
        "bern_NC9_forward": lambda: ops.bernstein_forward(x, theta, False),
        "bern_NC9_inverse": lambda: ops.bernstein_inverse(x, theta, False),
        "sos_2x3_forward": lambda: ops.sos_forward(x, a),
        "sos_2x3_inverse": lambda: ops.sos_inverse(x, a),
        "rqs_K8_backward_autograd": backward_of(phi8, lambda p: unpack(p, [(8,), (8,), (7,)]), lambda xx, p, s: ops.rqs_forward(xx, *s, packed=p)),
        "affine_backward_autograd": backward_of(phi2, lambda p: (p[..., 0], p[..., 1]), lambda xx, p, s: ops.affine_forward(xx, *s, packed=p)),
    }
    out = {}
    for name, fn in entries.items():
        with torch.set_grad_enabled(name.endswith("autograd")):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[name] = {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}
    print(json.dumps({"shape": [N, D], "repeats": repeats, "root": root, "entries": out}))


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = sys.argv[1:]
    root = os.path.abspath(args[args.index("--root") + 1]) if "--root" in args else here
    repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 10
    main(root, repeats)
