"""Static guard on the code the compiler emits for the FLOW instantiation of the two-part fused autoregressive kernel (csrc/fused_ar_half_impl.h:
arhf_kernel — the T transforms of a composed flow in one persistent launch; no GPU needed: hipcc cross-compiles).

The flow kernel instantiates the same pass as arh_kernel / arht_kernel (arh_pass) inside a loop over the transforms that is NOT unrolled: one pass
body in the instruction stream, whatever T — but for the first layer (24 of 600 blocks), which is there twice: the two feature orders of an alternating
flow mirror the input tiles, so their first layers take different in pairs (S::B_IP_ALT).  The unit is a generated unit of its own (zuko_amd/static_ar.py:
ARHF) for the conditioner tests/test_codegen_half.py compiles (NSF(64, hidden 256 x 3, 8 bins)); that test's unit and its two arh_kernel instantiations are
untouched."""

import collections
import hashlib
import os
import re
import subprocess

import pytest

from test_codegen_half import CFG2, ROOT, _check_raw_reads

NIT = 4  # 16-column groups of a 64-feature row: the vector loads / stores of a lane's share of a tile's rows
_ISA: dict = {}


def _isa() -> str:
    """ISA of the flow unit of the cfg2 flow (ascending, descending, ascending, ... feature order), cached per source + header hash under zuko_amd/lib/."""
    if "s" in _ISA:
        return _ISA["s"]
    from zuko_amd import static_ar

    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    tabs = [static_ar.half_tables(plan, lay.kind, 1)[0] for plan, lay, _ in static_ar._plans_for(*CFG2)]
    tf, flags = static_ar.flow_tables(tabs)
    assert flags == [0, 1] and tf["FLOW_ALT"] == 1, "the two feature orders of cfg2 differ in the first layer's in pairs"
    src = static_ar.emit(static_ar.ARHF, tf)
    h = hashlib.sha256((src + static_ar._half_digest()).encode()).hexdigest()[:16]
    out = os.path.join(ROOT, "zuko_amd", "lib", f"arhf_isa.{h}.s")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        hip = out[:-2] + ".hip"
        with open(hip, "w") as f:
            f.write(src)
        tmp = out + f".{os.getpid()}"
        subprocess.run([hipcc, *static_ar.hipcc_flags(), "--cuda-device-only", "-S", hip, "-o", tmp], check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, out)
    _ISA["s"] = open(out).read()
    return _ISA["s"]


def _kernel(s: str):
    names = re.findall(r"^(_ZN2zk11arhf_kernel\S+):", s, flags=re.M)
    assert len(names) == 1, names
    i = s.index(names[0] + ":")
    lines = [x.strip() for x in s[i : s.index(".Lfunc_end", i)].split("\n")]
    k = s.index(".amdhsa_kernel " + names[0])
    return [l for l in lines if l and not l.startswith((";", "//", "."))], s[k : s.index(".end_amdhsa_kernel", k)]


def test_flow_kernel_instruction_mix():
    ops, desc = _kernel(_isa())
    count = collections.Counter(l.split()[0] for l in ops)
    mfma = sum(n for k, n in count.items() if "mfma" in k)
    valu = sum(n for k, n in count.items() if k.startswith("v_") and "mfma" not in k)
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
    print(f"flow kernel: {len(ops)} instructions, {mfma} MFMA, {valu} other VALU, {vgpr} VGPRs")
    assert mfma == 1800 + 72, "one pass body (600 blocks, three partial products each) and the first layer's 24 blocks a second time: the loop over the transforms is not unrolled"
    assert ".amdhsa_private_segment_fixed_size 0" in desc, "scratch in the flow kernel: its raw LDS reads do not survive a spill"
    assert vgpr <= 256, f"{vgpr} VGPRs: two wavefronts per SIMD need 256 or fewer"
    assert valu <= 4500, f"{valu} vector instructions besides the matrix ones (the per-transform product kernel: 4 150 at most; the flow pass adds the row tile's reads, the per-pass feature ids and the second first layer's descales)"


def test_flow_kernel_stores_once_per_tile():
    """y and the log-derivative leave the kernel behind the LAST transform's epilogue only: NIT row stores and one ladj store in the whole kernel, all
    behind the pass's last matrix instruction; the next tile's rows are the only plain vector loads of the pass."""
    ops, _ = _kernel(_isa())
    stores = [i for i, l in enumerate(ops) if l.startswith(("global_store", "flat_store", "buffer_store"))]
    last_mfma = max(i for i, l in enumerate(ops) if "v_mfma" in l)
    assert len(stores) == NIT + 1, [ops[i] for i in stores]
    assert all(i > last_mfma for i in stores), "a global store in front of the pass's last matrix instruction"
    assert not [l for l in ops if l.startswith(("scratch_", "buffer_load"))]
    bars = [i for i, l in enumerate(ops) if l.startswith("s_barrier")]
    assert len(bars) == 1 + 50 + 2, f"{len(bars)} barriers: the staging barrier, one per chunk of a pass, and those of the first layer's two chunks a second time"
    # the ring's DMA: three pieces per chunk and the three chunks of the prologue, plus the next pass's bias image (one request in a scalar loop)
    dma = [l for l in ops if l.startswith("global_load_lds_dwordx4")]
    assert len(dma) == 3 * (3 + 50 + 2) + 1, len(dma)
    # the rows' barrier waits for vmcnt(NIT) in the tile's last pass and for vmcnt(0) in the others: both forms are there, once each
    waits = [l for l in ops if re.fullmatch(r"s_waitcnt vmcnt\(\d+\)", l)]
    assert sum(1 for w in waits if w == f"s_waitcnt vmcnt({NIT})") == 1, [w for w in waits if w != "s_waitcnt vmcnt(0)"]


def test_flow_kernel_raw_lds_reads_are_never_touched_before_their_wait():
    stats = _check_raw_reads(_isa(), "_ZN2zk11arhf_kernel")
    assert len(stats) == 1 and all(m == 1872 and r >= 1248 for r, m in stats), stats
