"""CPU: version 2 of the coupling argument block (include/zuko_amd.h: zk_coupling_args_v2) and what its two entries refuse before any HIP call."""

import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

EINVAL = 1  # hipErrorInvalidValue
ENTRIES = ("zk_coupling_forward_v2", "zk_coupling_inverse_v2")


def test_v2_block_has_the_c_compilers_size(tmp_path):
    import zuko_amd._C as C

    cls = C.STRUCTS["zk_coupling_args_v2"]
    header = os.path.join(ROOT, "include", "zuko_amd.h")
    src = tmp_path / "size.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void) {{ printf("%zu %zu %zu %zu %zu\\n", sizeof(zk_coupling_args_v2), '
                   "offsetof(zk_coupling_args_v2, bound), offsetof(zk_coupling_args_v2, uni_kind), offsetof(zk_coupling_args_v2, bins), sizeof(zk_coupling_args_v1)); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    size, o_bound, o_kind, o_bins, size_v1 = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == ctypes.sizeof(cls)
    assert (o_bound, o_kind, o_bins) == (cls.bound.offset, cls.uni_kind.offset, cls.bins.offset)
    # the v1 fields lead the block, at v1's offsets
    v1 = C.STRUCTS["zk_coupling_args_v1"]
    assert size_v1 == ctypes.sizeof(v1) == o_bound
    assert [(f, getattr(cls, f).offset) for f, _ in v1._fields_] == [(f, getattr(v1, f).offset) for f, _ in v1._fields_]


def _spline_block(**over):
    import zuko_amd._C as C

    fields = dict(uni_kind=1, bins=8, bound=5.0, slope=1e-3, static_ok=0)
    special = {k: over.pop(k) for k in ("struct_size", "version") if k in over}
    fields.update(over)
    a = C.args("zk_coupling_args_v2", **fields)
    for k, v in special.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("entry", ENTRIES)
def test_v2_entries_refuse_bad_blocks_without_touching_a_device(entry):
    import zuko_amd._C as C

    fn = getattr(C.lib(), entry)
    size = ctypes.sizeof(C.STRUCTS["zk_coupling_args_v2"])
    assert fn(_spline_block(struct_size=size - 8), None) == EINVAL
    assert fn(_spline_block(struct_size=ctypes.sizeof(C.STRUCTS["zk_coupling_args_v1"])), None) == EINVAL
    assert fn(_spline_block(version=1), None) == EINVAL
    assert fn(_spline_block(version=3), None) == EINVAL
    assert fn(_spline_block(uni_kind=2), None) == EINVAL
    assert fn(_spline_block(bins=5), None) == EINVAL
    assert fn(_spline_block(bins=32), None) == EINVAL
    for static_ok in (1, 2, 3):
        assert fn(_spline_block(static_ok=static_ok), None) == EINVAL
    assert fn(_spline_block(bound=0.0), None) == EINVAL
    assert fn(_spline_block(slope=0.0), None) == EINVAL
    # a well-formed block with no rows is accepted (nothing is launched): the refusals above are the fields', not the entry's
    for bins in (4, 8, 16):
        assert fn(_spline_block(bins=bins), None) == 0
    assert fn(_spline_block(uni_kind=0, bins=0, bound=0.0), None) == 0  # the affine map: the v1 launch, bins / bound not examined
