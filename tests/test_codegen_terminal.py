"""Static guard on the TERMINAL instantiation of the two-part fused autoregressive kernel (csrc/fused_ar_half_impl.h: arht_kernel), the last launch
of a no-grad `log_prob`: same matrix work as the product kernel, no scratch, no y rows stored, the base's table entries read from LDS once per
feature slot.  Shares the compiled ISA of tests/test_codegen_half.py (no GPU needed)."""

import collections
import re

from test_codegen_half import _check_raw_reads, _isa


def _ops(s: str, name: str):
    i = s.index("\n" + name + ":")
    j = s.index(".Lfunc_end", i)
    return collections.Counter(l.split()[0] for l in (x.strip() for x in s[i:j].split("\n")[2:]) if l and not l.startswith((";", "//", ".")) and not l.endswith(":"))


def test_terminal_kernel_instruction_mix():
    s = _isa()
    term = re.findall(r"^(_ZN2zk11arht_kernel\S+):", s, flags=re.M)
    product = [n for n in re.findall(r"^(_ZN2zk10arh_kernel\S+):", s, flags=re.M) if n.endswith("ELb0EEEvNS_6ArArgsE")]
    assert len(term) == 1 and len(product) == 1, (term, product)
    t, p = _ops(s, term[0]), _ops(s, product[0])
    mfma = sum(n for k, n in t.items() if "mfma" in k)
    valu = sum(n for k, n in t.items() if k.startswith("v_") and "mfma" not in k)
    valu_p = sum(n for k, n in p.items() if k.startswith("v_") and "mfma" not in k)
    stores = sum(n for k, n in t.items() if k.startswith("global_store"))
    print(f"terminal kernel: {sum(t.values())} instructions, {mfma} MFMA, {valu} other VALU (product: {valu_p}), {stores} global stores")
    assert mfma == 1800
    k = s.index(".amdhsa_kernel " + term[0])
    desc = s[k : s.index(".end_amdhsa_kernel", k)]
    assert ".amdhsa_private_segment_fixed_size 0" in desc, "scratch in the terminal kernel: its raw LDS reads do not survive a spill"
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)) <= 256  # two wavefronts per SIMD
    assert t["global_store_dwordx4"] == 0 and stores == 1, "the terminal kernel stores the log-density only: no y rows"
    # 16 feature slots per lane and tile, each at most: clamp of the feature id, LDS address, subtract, square, fma, add; the table staging of the
    # prologue (a division and a logarithm, expanded inline) within 40
    assert valu <= valu_p + 16 * 6 + 40, f"{valu} vector instructions against the product kernel's {valu_p}"


def test_terminal_kernel_raw_lds_reads_are_never_touched_before_their_wait():
    stats = _check_raw_reads(_isa(), "_ZN2zk11arht_kernel")
    assert len(stats) == 1 and all(m == 1800 and r >= 1200 for r, m in stats), stats
