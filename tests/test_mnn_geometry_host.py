"""CPU: the launch-geometry queries of the monotone-network kernels (zk_mnn_launch_geometry / zk_umnn_launch_geometry: host-only, the one statement of
the launchers' heuristic), and that the shapes the GPU tests launch (tests/mnn_nets.py: GEOMETRY_SHAPES) reach every geometry the heuristic can
produce.  If the heuristic changes, this test says which geometry the GPU tests no longer run.  No kernel is launched."""

import ctypes

import pytest

from mnn_nets import GEOMETRY_SHAPES, geometry

FAMILIES = ["mnn", "umnn"]


def _reachable(family):
    """Every (rows_per_block, feats_per_block) the query returns over a sweep of the two sizes: powers of two and their neighbours up to 2^22 rows
    and 2^12 columns, and the sizes around the heuristic's own thresholds (512 tiles of 64 rows x 4 columns; 1024 blocks)."""
    Ns = sorted({max(1, (1 << k) + d) for k in range(0, 23) for d in (-1, 0, 1)} | {n for n in range(1, 70000, 997)} | {n for (n, _) in GEOMETRY_SHAPES})
    Ds = sorted({max(1, (1 << k) + d) for k in range(0, 13) for d in (-1, 0, 1)} | set(range(1, 70)))
    return {geometry(N, D, family) for N in Ns for D in Ds}


@pytest.mark.parametrize("family", FAMILIES)
def test_the_gpu_tests_shapes_reach_every_launch_geometry(family):
    got = {shape: geometry(*shape, family) for shape in GEOMETRY_SHAPES}
    assert got == GEOMETRY_SHAPES, got
    reachable = _reachable(family)
    assert reachable == {(r, f) for r in (64, 128, 256) for f in (1, 4)}, f"the heuristic changed: {sorted(reachable)}"
    assert set(got.values()) == reachable, f"geometries no GPU test launches: {sorted(reachable - set(got.values()))}"
    # more than 64 rows per block with one feature per block: only through the roundings of the rule (ceil(Dsel / 4) counts the (tile, column group)
    # pairs, Dsel the blocks), at few rows and hundreds of columns
    assert geometry(64, 1024, family) == (256, 1) and geometry(65, 1024, family)[1] == 4 and geometry(64, 2045, family)[1] == 4


@pytest.mark.parametrize("family", FAMILIES)
def test_the_query_is_the_launchers_and_rejects_what_they_reject(family):
    import zuko_amd._C as C

    fn = getattr(C.lib(), f"zk_{family}_launch_geometry")
    text = open(C._HEADER).read()
    assert f"zk_{family}_launch_geometry" in text and f"zk_{family}_launch_geometry" in C.SIGNATURES
    r, f = ctypes.c_int(-7), ctypes.c_int(-7)
    EINVAL = 1
    for N, D in ((0, 5), (-1, 5), (64, 0), (64, (1 << 20) + 1)):
        assert fn(N, D, ctypes.byref(r), ctypes.byref(f)) == EINVAL and (r.value, f.value) == (-7, -7), (N, D)
    assert fn(64, 5, None, ctypes.byref(f)) == EINVAL and fn(64, 5, ctypes.byref(r), None) == EINVAL
    assert fn(1, 1, ctypes.byref(r), ctypes.byref(f)) == 0 and (r.value, f.value) == (64, 1)
    assert fn(1 << 40, 1 << 20, ctypes.byref(r), ctypes.byref(f)) == 0 and (r.value, f.value) == (256, 4)
    # the two families share the rule
    assert all(geometry(N, D, "mnn") == geometry(N, D, "umnn") for N in (1, 63, 1031, 16389, 100037, 131149) for D in (1, 5, 6, 8, 64))
