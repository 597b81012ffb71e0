"""Cases of tests/test_gpu_half_gaps.py, shared by the test and by the child process that evaluates them on a build of the two-part kernels
with the gap switches off (csrc/fused_ar_half_impl.h: ARH_SPLIT_GAPS):

    python tests/half_gaps_cases.py <dir>      builds the cases' kernels with -DARH_SPLIT_GAPS=0 into <dir>/ars (static_ar.build_half_variant),
                                               evaluates every case on them and writes <dir>/outputs.pt

Flows: T = 2 and 3 of MAF(16, [128, 128]) (four in pairs, a pass of three chunks), T = 2 of the cfg2 conditioner NSF(64, [256] * 3, 8 bins) and T = 2 of
MAF(16, [112, 112]) (seven hidden tiles: the last in pair is half zeros).  Rows: 129 (a second tile with one live row) and 32 897 (257 tiles on a grid of 256
workgroups).  Row 100 holds a NaN; row 77 a value above the two-part kernel's overflow bound 65520 x 2^90 (its sample becomes NaN)."""

import os
import sys

import torch

ROWS = [129, 256 * 128 + 129]
NMAX = ROWS[-1]
BAD, OVER = 100, 77
CASES = [("maf16", 2), ("maf16", 3), ("nsf_cfg2", 2), ("maf112", 2)]
MAF112 = ("affine", 16, 0, (112, 112), 0)  # not among the prebuilt kernels: the test builds it into a cache directory of its own
VARIANT_CONFIGS = [("affine", 16, 0, (128, 128), 0), ("rqs", 64, 0, (256, 256, 256), 8), MAF112]  # (zuko_amd.static_ar.build_half_variant)
OFF_FLAGS = ["-DARH_SPLIT_GAPS=0"]


def build_flow(name: str, T: int):
    """(flow on the CPU, features): the same weights in every process."""
    import zuko_amd.flows as F

    torch.manual_seed(17 + T)
    if name == "nsf_cfg2":
        return F.NSF(features=64, context=0, transforms=T, bins=8, hidden_features=[256] * 3), 64
    return F.MAF(16, 0, transforms=T, hidden_features=[128, 128] if name == "maf16" else [112, 112]), 16


def inputs(D: int) -> torch.Tensor:
    x = torch.randn(NMAX, D, generator=torch.Generator().manual_seed(37)) * 1.2
    x[BAD, D // 2] = float("nan")
    x[OVER, 3] = 1e32
    return x


def evaluate(flow, xn):
    """log_prob, y and the log-determinant of the flow launch."""
    with torch.no_grad():
        lp = flow().log_prob(xn)
        y, ladj = flow().transform.call_and_ladj(xn)
    return lp, y, ladj


def served_by_two_part_kernels(flow, dev) -> bool:
    return all(t.fused_state(dev).half is not None and t.fused_state(dev).half_ok for t in flow.transform.transforms)


def main(out: str) -> None:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import zuko_amd
    from zuko_amd import static_ar as sa

    sa.build_half_variant(VARIANT_CONFIGS, out, OFF_FLAGS)
    os.environ["ZUKO_AMD_CACHE_DIR"] = os.path.abspath(out)
    sa.rescan()
    zuko_amd.set_matmul_precision("f16x2")
    dev = torch.device("cuda:0")
    res = {}
    for name, T in CASES:
        flow, D = build_flow(name, T)
        flow = flow.to(dev)
        x = inputs(D).to(dev)
        for N in ROWS:
            res[(name, T, N)] = tuple(t.cpu() for t in evaluate(flow, x[:N]))
        assert served_by_two_part_kernels(flow, dev), (name, T)
    torch.cuda.synchronize()
    ars = os.path.join(os.path.abspath(out), "ars")
    half = [so for n, so in sa.loaded_kernels().items() if n.startswith(("arh_", "arhf_"))]
    assert half and all(os.path.dirname(so) == ars for so in half), f"kernels that are not the variant's served a case: {half}"
    torch.save(res, os.path.join(out, "outputs.pt"))


if __name__ == "__main__":
    main(sys.argv[1])
