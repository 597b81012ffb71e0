"""Per-kernel instruction census of device ISA files (hipcc --cuda-device-only -S), parent beside branch, as a markdown table.

    python scripts/isa_census.py PARENT_DIR BRANCH_DIR [name.s ...]

Every kernel symbol (.amdhsa_kernel) of every file present in both directories gets one row: instructions, matrix instructions, other VALU, LDS
reads / writes, global loads / stores, barriers, waits, s_nop, next_free_vgpr and scratch bytes.  Opcodes are counted generically by prefix."""

import collections
import os
import re
import subprocess
import sys

COLS = ("instr", "mfma", "valu", "ds_read", "ds_write", "global_load", "global_store", "s_barrier", "s_waitcnt", "s_nop", "vgpr", "scratch")


# kernel template -> position of its DIAG argument among the template arguments (the diagnostic twins get the lenient gate); a kernel that is not
# listed here has no twin and gets the product gate
DIAG_ARG = {"zk::ar_kernel": 4, "zk::ar_gsplit_kernel": 2, "zk::arx_kernel": 3, "zk::arh_kernel": 2}


def is_twin(pretty: str) -> bool:
    m = re.match(r"void (zk::\w+)<(.*)>\(zk::ArArgs\)$", pretty)
    if not m or m.group(1) not in DIAG_ARG:
        return False
    args, depth, cur = [], 0, ""
    for ch in m.group(2):  # split the template arguments at top-level commas
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    args.append(cur.strip())
    pos = DIAG_ARG[m.group(1)]
    return len(args) > pos and args[pos] == "true"


def census(path: str) -> dict:
    s = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", s, flags=re.M):
        i = s.index("\n" + name + ":")
        j = s.index(".Lfunc_end", i)
        ops = collections.Counter(l.split()[0] for l in (x.strip() for x in s[i:j].split("\n")[2:]) if l and not l.startswith((";", "//", ".")) and not l.endswith(":"))
        k = s.index(".amdhsa_kernel " + name)
        desc = s[k : s.index(".end_amdhsa_kernel", k)]
        pre = lambda p: sum(n for o, n in ops.items() if o.startswith(p))
        mfma = sum(n for o, n in ops.items() if "mfma" in o)
        out[name] = dict(instr=sum(ops.values()), mfma=mfma, valu=pre("v_") - mfma, ds_read=pre("ds_read"), ds_write=pre("ds_write"), global_load=pre("global_load"),
                         global_store=pre("global_store"), s_barrier=pre("s_barrier"), s_waitcnt=pre("s_waitcnt"), s_nop=pre("s_nop"),
                         vgpr=int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", desc).group(1)), scratch=int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc).group(1)))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, r))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(parent: str, branch: str, files) -> int:
    files = files or sorted(f for f in os.listdir(branch) if f.endswith(".s") and os.path.exists(os.path.join(parent, f)))
    bad = 0
    for f in files:
        a, b = census(os.path.join(parent, f)), census(os.path.join(branch, f))
        pretty = demangle(sorted(set(a) | set(b)))
        print(f"\n### {f}\n\n| kernel | " + " | ".join(COLS) + " | gate |\n|---|" + "---|" * (len(COLS) + 1))
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                one = a.get(name) or b[name]  # (a kernel that was renamed or replaced: its own counts, so that the two sides can be read next to each other)
                print(f"| `{pretty[name]}` | " + " | ".join(str(one[c]) for c in COLS) + f" | only in {'parent' if name in a else 'branch'} |")
                bad += 1
                continue
            pa, br = a[name], b[name]
            diag = is_twin(pretty[name])
            if diag:
                ok = br["vgpr"] <= pa["vgpr"] and br["scratch"] <= pa["scratch"]
            else:
                ok = (all(br[c] == pa[c] for c in ("mfma", "ds_read", "global_load", "global_store", "s_barrier")) and br["vgpr"] <= pa["vgpr"] and br["valu"] <= pa["valu"]
                      and (br["scratch"] == 0 or pa["scratch"] != 0))
            bad += not ok
            cells = [(str(pa[c]) if pa[c] == br[c] else f"{pa[c]} → {br[c]}") for c in COLS]
            print(f"| `{pretty[name]}`{' (diagnostic twin)' if diag else ''} | " + " | ".join(cells) + f" | {'ok' if ok else '**FAIL**'} |")
    print(f"\n{bad} kernel(s) miss the gate" if bad else "\nevery kernel passes the gate")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
