"""Static guard on the code the compiler emits for the TWO-PART fused autoregressive kernel bench.py measures (no GPU needed:
hipcc cross-compiles).

csrc/fused_ar_half_impl.h pins the vector work between the matrix instructions: the operand split is two v_fma_mix*_f16 per
value, the ReLU one v_max_f32, the sample maximum one v_max3_f32 per pair, the last layer's descale one fma per parameter.  Left
to the compiler the same source costs 500 vector instructions more per launch (the split converts its high part back to f32,
the vectoriser gathers register pairs with v_mov) and spills.  The test generates the kernel of NSF(64, hidden 256 x 3, 8 bins)
as zuko_amd/static_ar.py does, compiles it to ISA with the flags of static_ar._build_so (static_ar.hipcc_flags; cached per source + header hash under
zuko_amd/lib/) and bounds the instruction mix of the product instantiation (DIAG = false)."""

import collections
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zuko_amd", "csrc")
CFG2 = ("rqs", 64, 0, (256, 256, 256), 8)


def _isa() -> str:
    from zuko_amd import static_ar

    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    (plan, lay, _), _ = static_ar._plans_for(*CFG2)
    src = static_ar.emit(static_ar.ARH, static_ar.half_tables(plan, lay.kind, 1)[0])
    h = hashlib.sha256((src + static_ar._half_digest()).encode()).hexdigest()[:16]
    out = os.path.join(ROOT, "zuko_amd", "lib", f"arh_isa.{h}.s")
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        hip = out[:-2] + ".hip"
        with open(hip, "w") as f:
            f.write(src)
        tmp = out + f".{os.getpid()}"
        subprocess.run([hipcc, *static_ar.hipcc_flags(), "--cuda-device-only", "-S", hip, "-o", tmp], check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, out)
    return open(out).read()


def _check_raw_reads(s: str, prefix: str):
    """For every kernel whose mangled name starts with `prefix`: between an inline-assembly `ds_read_b128` and an
    `s_waitcnt lgkmcnt(n)` that covers it (LDS operations of a wave complete in order: a wait lgkmcnt(n) covers every read
    except the youngest n) no instruction may mention the destination registers.  Returns [(asm reads, MFMAs)] per kernel."""

    def regs(t):
        out = set()
        for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", t):
            if m.group(1):
                out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
            else:
                out.add(int(m.group(3)))
        return out

    stats = []
    for k in [m.start() for m in re.finditer(r"^" + prefix + r"[^\n]*:", s, flags=re.M)]:
        body = s[k : s.index("s_endpgm", k)].split("\n")
        pending, in_asm, n_reads, mfma = [], False, 0, 0
        for line in body:
            t = line.strip()
            if t.startswith(";;#ASMSTART"):
                in_asm = True
                continue
            if t.startswith(";;#ASMEND"):
                in_asm = False
                continue
            if not t or t[0] in ";.":
                continue
            mfma += "v_mfma" in t
            m = re.match(r"ds_read_b128 (v\[\d+:\d+\]), ", t)
            if m and in_asm:
                pending.append(regs(m.group(1)))
                n_reads += 1
                continue
            w = re.match(r"s_waitcnt .*lgkmcnt\((\d+)\)", t)
            if w:
                n = int(w.group(1))
                pending = pending[len(pending) - n :] if 0 < n < len(pending) else ([] if n == 0 else pending)
                continue
            used = regs(t)
            assert not any(used & r for r in pending), f"'{t}' touches a weight tile whose LDS read has not been waited for"
        stats.append((n_reads, mfma))
    return stats


def test_two_part_kernel_instruction_mix():
    s = _isa()
    names = re.findall(r"^(_ZN2zk10arh_kernel\S+):", s, flags=re.M)
    product = [n for n in names if n.endswith("ELb0EEEvNS_6ArArgsE")]  # <Shape, UniRqs<8, false>, DIAG = false>
    assert len(names) == 2 and len(product) == 1, names
    name = product[0]
    i = s.index(name + ":")
    j = s.index(".Lfunc_end", i)
    ops = collections.Counter(l.split()[0] for l in (x.strip() for x in s[i:j].split("\n")) if l and not l.startswith((";", "//", ".")))
    mfma = sum(n for k, n in ops.items() if "mfma" in k)
    valu = sum(n for k, n in ops.items() if k.startswith("v_") and "mfma" not in k)
    back = sum(n for k, n in ops.items() if k.startswith("v_cvt_f32_f16"))
    vmov = sum(n for k, n in ops.items() if k.startswith("v_mov_b32"))
    print(f"two-part kernel: {sum(ops.values())} instructions, {mfma} MFMA, {valu} other VALU, {back} v_cvt_f32_f16, {vmov} v_mov_b32, {ops['s_nop']} s_nop")
    assert mfma == 1800  # 600 blocks of two images, three partial products each
    k = s.index(".amdhsa_kernel " + name)
    desc = s[k : s.index(".end_amdhsa_kernel", k)]
    assert ".amdhsa_private_segment_fixed_size 0" in desc, "scratch (VGPR spill) in the two-part kernel: its raw LDS reads do not survive a spill"
    assert valu <= 4150, f"{valu} vector instructions besides the matrix ones (4 572 before the epilogue was pinned)"
    assert back <= 40, f"{back} v_cvt_f32_f16: the split converts its high part back to f32 again"
    assert vmov <= 150, f"{vmov} v_mov_b32: register pairs are being gathered for packed instructions again"


def test_two_part_kernel_raw_lds_reads_are_never_touched_before_their_wait():
    stats = _check_raw_reads(_isa(), "_ZN2zk10arh_kernel")
    assert len(stats) == 2 and all(m == 1800 and r >= 1200 for r, m in stats), stats  # (1 200 weight images + the bias tiles read raw)
