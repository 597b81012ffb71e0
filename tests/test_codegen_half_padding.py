"""Static guard on the s_nop padding and the wait states of the TWO-PART fused autoregressive kernel (csrc/fused_ar_half_impl.h; no GPU needed:
hipcc cross-compiles).

The compiler pads an inline-assembly statement that defines a register and an instruction that reads it.  An out tile's ReLU with its entry
into the sample maximum (arh_relu_max) and an operand split (arh_split) are therefore ONE statement each: no s_nop stands in front of a
v_max3_f32 any more.  This test reads the ISA of tests/test_codegen_half.py (product and terminal kernel) and tests/test_codegen_flow.py (flow
kernel) and checks, per kernel: no pad between a counted wait and a matrix instruction, none in front of a v_max3_f32, at most 450 s_nop in the
product kernel, and — statically — at least 8 wait states between every matrix instruction and the first other instruction that reads or
writes its destination.

A block is the compiler's own wait (__builtin_amdgcn_s_waitcnt: the one wait state the compiler wants between the raw reads' statements and
a statement that uses what they defined) and ONE statement of three matrix instructions behind it (arh_wait_block); the wait states the
compiler no longer places stand in that string.  Measured on this build: 0 padded waits (the parent: 600 / 600 / 624 in the product /
terminal / flow kernel by this count), 296 s_nop in the product kernel (1 032), 13 wait states at least on the walk (8).  The earlier forms
and their counts: profiles/half_blocks/README.md."""

import re

import pytest

import test_codegen_flow
import test_codegen_half


def _regs(t: str) -> set:
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", t):
        if m.group(1):
            out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.add(int(m.group(3)))
    return out


def _body(s: str, name: str) -> list:
    """The instructions of kernel `name`, in order (labels, directives and comments dropped)."""
    i = s.index("\n" + name + ":")
    lines = (x.strip() for x in s[i : s.index(".Lfunc_end", i)].split("\n")[2:])
    return [l for l in lines if l and not l.startswith((";", "//", ".")) and not l.endswith(":")]


def _kernels():
    half = test_codegen_half._isa()
    flow = test_codegen_flow._isa()
    product = [n for n in re.findall(r"^(_ZN2zk10arh_kernel\S+):", half, flags=re.M) if n.endswith("ELb0EEEvNS_6ArArgsE")]
    term = re.findall(r"^(_ZN2zk11arht_kernel\S+):", half, flags=re.M)
    fl = re.findall(r"^(_ZN2zk11arhf_kernel\S+):", flow, flags=re.M)
    assert len(product) == 1 and len(term) == 1 and len(fl) == 1, (product, term, fl)
    return {"product": (half, product[0]), "terminal": (half, term[0]), "flow": (flow, fl[0])}


@pytest.fixture(scope="module")
def kernels():
    return {k: (_body(s, n), s, n) for k, (s, n) in _kernels().items()}


KINDS = ("product", "terminal", "flow")


@pytest.mark.parametrize("kind", KINDS)
def test_no_pad_between_a_counted_wait_and_a_matrix_instruction(kernels, kind):
    ops = kernels[kind][0]
    hits = [i for i in range(len(ops) - 2) if re.match(r"s_waitcnt lgkmcnt\(\d+\)$", ops[i]) and ops[i + 1].startswith("s_nop") and ops[i + 2].startswith("v_mfma")]
    print(f"{kind}: {len(hits)} x (s_waitcnt lgkmcnt(n); s_nop; v_mfma)   (579 while the wait and the block were two statements)")
    assert not hits, f"{len(hits)} blocks with a pad between their wait and their first matrix instruction, e.g. instruction {hits[0]}"


@pytest.mark.parametrize("kind", KINDS)
def test_no_pad_in_front_of_a_max3(kernels, kind):
    ops = kernels[kind][0]
    hits = [i for i in range(1, len(ops)) if ops[i].startswith("v_max3_f32") and ops[i - 1].startswith("s_nop")]
    print(f"{kind}: {len(hits)} s_nop directly in front of a v_max3_f32 of {sum(o.startswith('v_max3_f32') for o in ops)}   (55 while every max was a statement of its own)")
    assert not hits


def test_product_kernel_pad_count(kernels):
    ops = kernels["product"][0]
    nops = [o for o in ops if o.startswith("s_nop")]
    print(f"product: {len(nops)} s_nop, {sum(o == 's_nop 0' for o in nops)} of them s_nop 0   (1 032 / 947 before)")
    assert len(nops) <= 450


@pytest.mark.parametrize("kind", KINDS)
def test_matrix_results_are_read_after_their_wait_states(kernels, kind):
    """Every matrix instruction: scan forward to the first instruction that is not a matrix instruction and mentions one of its destination
    registers, counting wait states (s_nop N = N + 1, any other instruction 1; branches do not occur between a block and the tile's end).  A
    matrix instruction that takes exactly the destination as its SrcC continues the accumulation and needs none."""
    ops = kernels[kind][0]
    least, n_checked = None, 0
    for i, o in enumerate(ops):
        if not o.startswith("v_mfma"):
            continue
        dst = o.split()[1].rstrip(",")
        d = _regs(dst)
        states, j = 0, i + 1
        while j < len(ops):
            t = ops[j]
            if t.startswith("v_mfma"):
                args = [a.strip() for a in t.split(None, 1)[1].split(",")]
                if args[3] == dst and not (_regs(args[1]) | _regs(args[2])) & d:
                    break  # (accumulate chain: the next reader is found from THAT instruction)
                assert not (_regs(args[0]) | _regs(args[1]) | _regs(args[2]) | _regs(args[3])) & d, f"'{t}' overlaps the destination of '{o}' without being its accumulate chain"
            elif _regs(t) & d:
                n_checked += 1
                least = states if least is None else min(least, states)
                assert states >= 8, f"'{t}' touches {dst} {states} wait states behind '{o}' (instruction {i})"
                break
            m = re.match(r"s_nop (\d+)", t)
            states += int(m.group(1)) + 1 if m else 1
            j += 1
    print(f"{kind}: least distance between a matrix instruction and the first other instruction on its destination: {least} wait states ({n_checked} tile ends)")
    assert n_checked > 0


@pytest.mark.parametrize("kind", KINDS)
def test_registers_and_scratch(kernels, kind):
    _, s, name = kernels[kind]
    k = s.index(".amdhsa_kernel " + name)
    desc = s[k : s.index(".end_amdhsa_kernel", k)]
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
    print(f"{kind}: {vgpr} VGPRs")
    assert vgpr <= 256, f"{vgpr} VGPRs: two wavefronts per SIMD need 256 or fewer"
    assert ".amdhsa_private_segment_fixed_size 0" in desc, "scratch: the kernel's raw LDS reads do not survive a spill"
