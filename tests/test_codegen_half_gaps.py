"""Static guard on WHERE the operand splits of the two-part fused autoregressive kernel stand (csrc/fused_ar_half_impl.h: ARH_SPLIT_GAPS; no GPU
needed: hipcc cross-compiles).

A v_mfma_f32_16x16x32_f16 holds its SIMD's vector issue for half of its time.  With both wavefronts of a SIMD issuing matrix instructions, one
instruction of issue cost 8 (v_fma_mix*_f16, transcendentals) or two of cost 4 (v_fma_f32, v_max_f32, v_cndmask_b32) behind a matrix instruction cost
1.8 cycles per matrix instruction together; a second v_fma_mix*_f16 costs 6.5 more, one packed f32 instruction 13.6 (scripts/probes/gap_fill_probe.hip,
profiles/half_gaps/gap_fill_probe.txt).  So the budget of a gap is 8, and the sixteen v_fma_mix*_f16 of in pair p >= 1 of a consuming layer (hidden
layers 1, 2 and the last layer) stand ONE per gap in the blocks in front of the pair's first reader; where the pattern leaves too few blocks, the rest
of the pair stands in front of that reader as before.  arh_gap_plan is the table; `plan` below is the same table from the Python tables.

The test reads the ISA of tests/test_codegen_half.py (product and terminal kernel) and tests/test_codegen_flow.py (flow kernel) of cfg2, built with the
shipped defaults, and checks per kernel and consuming layer: the v_fma_mix*_f16 directly behind the layer's matrix instructions are as many as the table
says (16 x 7 in the last layer, where every pair finds its blocks); no gap inside a block — everything there is pinned — carries more than the budget,
counted with the probe's costs, and no packed f32 instruction; no split instruction reads its f32 value or its scale from a register that one of the
sixteen split instructions in front of it wrote (a split's registers are matrix operands to the layer's end; a statement whose operands say less
than it does lets the compiler put an output where an input still lives); no vector instruction writes an A or B operand of a matrix instruction
fewer than two wait states in front of it (the matrix instructions stand inside strings, where the compiler's hazard recogniser places nothing: a
register copy in front of a block must not stand behind the block's wait); no VGPR is spilled.  The spline of group g under the matrix
instructions of group g + 1 is not built: the count of spline transcendentals in matrix gaps is pinned at the shipped build's 0 and printed beside
the upper bound from GOFF."""

import re

import pytest

import test_codegen_flow
import test_codegen_half
from test_codegen_half_padding import KINDS, _body, _kernels, _regs

BUDGET = 8  # issue cycles of vector work behind one matrix instruction (the probe)
COST8 = ("v_fma_mix", "v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32")


def _cost(op: str) -> int:
    if op.startswith("v_pk_") and op.split()[0].endswith("_f32"):
        return 100  # (13.6 cycles for ONE: never in a gap)
    return 8 if op.startswith(COST8) else 4


def _tables():
    from zuko_amd import static_ar

    (plan, lay, _), _ = static_ar._plans_for(*test_codegen_half.CFG2)
    return static_ar.half_tables(plan, lay.kind, 1)[0], plan.layout.nt


def plan(t: dict, L: int, nt: int) -> list:
    """arh_gap_plan<S, L, NT>: per block of consuming layer L (NH: the last layer) the number of split instructions it carries."""
    NH, last = t["NH"], L == t["NH"]
    off = sum(t["NB"][:L])
    nblk = t["GOFF"][-1] * nt if last else t["NB"][L]
    reader = (lambda b: t["G_IP"][b // nt]) if last else (lambda b: t["B_IP"][off + b])
    carried, cursor = [0] * nblk, 0
    for p in range(1, (t["HT"][L - 1] + 1) // 2):
        lim = next((b for b in range(nblk) if reader(b) == p), nblk)
        if not last:
            for tile in (2 * p, 2 * p + 1):
                blocks = [b for b in range(nblk) if t["B_OT"][off + b] == tile]
                lim = min(lim, nblk if tile >= t["HT"][L] else (blocks[-1] if blocks else 0))
        f = 1
        while f <= 6 and cursor < lim:
            carried[cursor] = 3 if f < 6 else 1
            cursor, f = cursor + 1, f + 1
    return carried


@pytest.fixture(scope="module")
def kernels():
    return {k: (_body(s, n), s, n) for k, (s, n) in _kernels().items()}


def _behind(ops: list) -> list:
    """Per matrix instruction, in program order: the vector instructions that stand directly behind it."""
    out = []
    for i, o in enumerate(ops):
        if o.startswith("v_mfma"):
            j = i + 1
            while j < len(ops) and ops[j].startswith("v_") and not ops[j].startswith("v_mfma"):
                j += 1
            out.append(ops[i + 1 : j])
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_splits_stand_among_the_matrix_instructions_of_the_consuming_layer(kernels, kind):
    t, nt = _tables()
    behind = _behind(kernels[kind][0])
    extra = len(behind) - 1800  # (the flow kernel holds the first layer's 24 blocks twice, in front of everything else)
    assert extra in (0, 72) and extra % 3 == 0
    pairs = (t["HT"][0] + 1) // 2
    first = extra // 3 + t["NB"][0]
    total = 0
    for L in range(1, t["NH"] + 1):
        carried = plan(t, L, nt)
        want = sum(carried)
        got_blocks = []
        for b in range(len(carried)):
            runs = behind[3 * (first + b) : 3 * (first + b) + 3]
            # the two gaps inside the block: every split instruction in them counts (more than one is over the budget and fails the table too); behind
            # the block's last matrix instruction: the leading one only — a rest-of-a-split statement in front of the next block may follow it
            mix = [[o for o in r if o.startswith("v_fma_mix")] for r in runs[:2]] + [[o for o in runs[2][:1] if o.startswith("v_fma_mix")]]
            got_blocks.append(sum(len(m) for m in mix))
        print(f"{kind}, layer {L}: {sum(got_blocks)} v_fma_mix*_f16 among the layer's matrix instructions; the table: {want} of {16 * (pairs - 1)} ({len(carried)} blocks)")
        assert got_blocks == carried, f"layer {L}: the blocks carry {got_blocks}, the table says {carried}"
        if L == t["NH"]:
            assert want == 16 * (pairs - 1), "the last layer's first steps read pair 0 only: every later pair finds six blocks in front of its first reader"
        first += len(carried)
        total += want
    assert first == len(behind) // 3
    ops = kernels[kind][0]
    all_mix = sum(o.startswith("v_fma_mix") for o in ops)
    led = sum(o.startswith("v_fma_mix") and ops[i - 1].startswith("v_mfma") for i, o in enumerate(ops))
    print(f"{kind}: {total} of {all_mix} v_fma_mix*_f16 stand in matrix gaps")
    # nothing falls between this test and the budget test: every split instruction that follows a matrix instruction directly is one the table placed
    # (none in the first layer, none twice in a gap), and the rest of the 416 stand in front of a layer or of a pair's first reader
    assert led == total and all_mix == 416, (led, total, all_mix)


@pytest.mark.parametrize("kind", KINDS)
def test_no_gap_inside_a_block_is_over_the_budget(kernels, kind):
    behind = _behind(kernels[kind][0])
    worst = 0
    for i, run in enumerate(behind):
        if i % 3 == 2:
            run = run[:1] if run and run[0].startswith("v_fma_mix") else []  # (behind a block's last matrix instruction: the carried instruction only; the rest belongs to what follows the block)
        cost = sum(_cost(o) for o in run)
        worst = max(worst, cost)
        assert cost <= BUDGET, f"matrix instruction {i}: {run} behind it cost {cost} issue cycles (budget {BUDGET})"
        assert not [o for o in run if o.startswith("v_pk_")], f"matrix instruction {i}: a packed instruction in its gap: {run}"
    print(f"{kind}: the fullest gap inside a block carries {worst} issue cycles of vector work (budget {BUDGET})")


SPLINE_WINDOW = 0.67  # share of the spline's issue time that has a window under the next group's matrix instructions (profiles/half_gaps/README.md: GOFF, the probe's costs)
TRANSCENDENTAL = COST8[1:]


@pytest.mark.parametrize("kind", KINDS)
def test_spline_work_in_matrix_gaps_is_what_the_shipped_build_places(kernels, kind):
    """The spline of group g under the matrix instructions of group g + 1 is NOT built (profiles/half_gaps/README.md): the shipped build places no
    spline transcendental in a matrix gap, and the count is pinned there.  Whatever vector work the compiler puts directly behind a matrix instruction
    of the last layer, no packed f32 instruction — 13.6 cycles in a gap by the probe — may be among it."""
    t, nt = _tables()
    behind = _behind(kernels[kind][0])
    n_last = t["GOFF"][-1] * nt * 3
    last = behind[len(behind) - n_last :]
    inside = [r for i, r in enumerate(last) if i % 3 != 2]
    trans = sum(o.startswith(TRANSCENDENTAL) for r in inside for o in r)
    every = sum(o.startswith(TRANSCENDENTAL) for o in kernels[kind][0])
    print(f"{kind}: {trans} of {every} transcendentals stand in the last layer's matrix gaps; upper bound from GOFF: {SPLINE_WINDOW:.0%} of the spline's issue time")
    assert trans == 0
    assert not [o for r in inside for o in r if o.startswith("v_pk_")], "a packed f32 instruction in a matrix gap of the last layer"


@pytest.mark.parametrize("kind", KINDS)
def test_no_split_instruction_reads_what_its_split_wrote(kernels, kind):
    recent, n = [], 0
    for o in kernels[kind][0]:
        if not o.startswith("v_fma_mix"):
            continue
        dst, val, scale = (a.strip() for a in o.split(None, 1)[1].split(",")[:3])
        assert val not in recent and scale not in recent, f"'{o}' reads a register that one of the sixteen split instructions in front of it wrote"
        recent = (recent + [dst])[-16:]
        n += 1
    assert n == 416  # 26 pairs: two of the input, eight of each hidden layer's output


@pytest.mark.parametrize("kind", KINDS)
def test_no_vector_write_to_a_matrix_operand_directly_in_front_of_it(kernels, kind):
    ops = kernels[kind][0]
    for i, o in enumerate(ops):
        if not o.startswith("v_mfma"):
            continue
        args = [a.strip() for a in o.split(None, 1)[1].split(",")]
        ab = _regs(args[1]) | _regs(args[2])
        states, j = 0, i - 1
        while states < 2 and j >= 0:
            t = ops[j]
            m = re.match(r"s_nop (\d+)", t)
            if t.startswith("v_") and not t.startswith("v_mfma"):
                assert not _regs(t.split(None, 1)[1].split(",")[0]) & ab, f"'{t}' writes an operand of '{o}' {states} wait states in front of it"
            states += int(m.group(1)) + 1 if m else 1
            j -= 1


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_spills(kernels, kind):
    _, s, name = kernels[kind]
    k = s.index(".amdhsa_kernel " + name)
    desc = s[k : s.index(".end_amdhsa_kernel", k)]
    meta = s[s.index(".name:", s.index("amdhsa.kernels")) :]
    m = meta[meta.index(name) :]
    spill = int(re.search(r"\.vgpr_spill_count:\s*(\d+)", m).group(1))
    vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1))
    print(f"{kind}: {vgpr} VGPRs, {spill} spilled")
    assert spill == 0 and ".amdhsa_private_segment_fixed_size 0" in desc and vgpr <= 256
