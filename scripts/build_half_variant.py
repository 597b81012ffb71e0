#!/usr/bin/env python
"""Probe builds of the two-part fused autoregressive kernels (csrc/fused_ar_half_impl.h: arh_kernel, arht_kernel, arhf_kernel) under extra compiler flags:

    python scripts/build_half_variant.py <dir> <config>[,<config>...] [-DARH_SPLIT_GAPS=0 ...]      ->  <dir>/ars/arh_<sig>.so, arhf_<sig>.so

<config>: cfg2 (NSF(64, [256] * 3, 8 bins)), cfg3 (MAF(64, [256] * 3)), maf16 (MAF(16, [128, 128])), or kind:features:context:h1xh2x..:bins.
Both feature orders' units and the flow unit are built.  Run with ZUKO_AMD_CACHE_DIR=<dir> (searched before zuko_amd/lib/ars) to use them:
bench.py, tests/test_gpu_half_gaps.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMED = {"cfg2": ("rqs", 64, 0, (256, 256, 256), 8), "cfg3": ("affine", 64, 0, (256, 256, 256), 0), "maf16": ("affine", 16, 0, (128, 128), 0)}


def parse(c: str):
    if c in NAMED:
        return NAMED[c]
    kind, features, context, hidden, bins = c.split(":")
    return kind, int(features), int(context), tuple(int(h) for h in hidden.split("x")), int(bins)


def main(out: str, configs: list, flags: list) -> list:
    from zuko_amd import static_ar

    return static_ar.build_half_variant(configs, out, flags)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    print("\n".join(main(sys.argv[1], [parse(c) for c in sys.argv[2].split(",")], sys.argv[3:])))
