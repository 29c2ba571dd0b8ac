#!/usr/bin/env python3
"""CPU: are the kernels of one translation unit instruction for instruction the same in two device listings?  What
profiles/dev_common_isa.txt was made with -- per unit, before and after a change that should not touch device code:
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S polypolish_amd/csrc/pp_gate.hip -o after/pp_gate.s
    python tools/isa_same.py before/pp_gate.s after/pp_gate.s
One line per kernel: unit, name, instructions before, after, same yes/no; then the kernels that went away and those that came.
A listing is split at the kernel symbols; directives and comments are dropped, branch labels lose their function number,
mangled names their spelling and string constants their number within the unit, so that only the instructions and where the
branches go are compared.  Exit status 1 if a kernel
differs or a new one appears."""
import os
import re
import sys

# a kernel that took another name on the way: the name before -> the name after
RENAMED = {"k_gate_scan3": "k_colscan<3>", "k_bam_scan3": "k_colscan<3>", "k_nm_scan2": "k_colscan<2>",
           "k_dfmt_scan1": "k_colscan<1>"}
ARG = {"y": "u64", "j": "u32", "Lb0": "false", "Lb1": "true"}


def kernel_name(sym):
    """_ZN12_GLOBAL__N_17k_tscanIyEEvPKjyPT_ -> k_tscan<u64>"""
    m = re.match(r"_ZN(?:12_GLOBAL__N_1|2pp)(\d+)", sym)
    if not m:
        return sym
    at = m.end()
    name, rest = sym[at:at + int(m.group(1))], sym[at + int(m.group(1)):]
    t = re.match(r"I([A-Za-z0-9]+?)EE", rest)
    if t:
        a = t.group(1)
        name += "<%s>" % ARG.get(a, a[2:] if re.match(r"L[jiym]\d+$", a) else a)
    return name


def kernels(path):
    """{name: [normalised instruction and label lines]}"""
    out, cur = {}, None
    text = open(path).read()
    functions = set(re.findall(r"^\s*\.type\s+(_Z\w+),@function", text, re.M))  # (a table in constant memory is no kernel)
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        s = line.strip()
        m = re.match(r"(_Z\w+):$", s)
        if m:
            cur = out.setdefault(kernel_name(m.group(1)), []) if m.group(1) in functions else None
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or (s.startswith(".") and not s.endswith(":")):
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        s = re.sub(r"_Z\w+", "SYM", s)
        s = re.sub(r"\.str(\.\d+)?@", ".str@", s)  # (string constants are numbered per unit, in the order of their first use)
        cur.append(" ".join(s.split()))
    return out


def main(before_path, after_path):
    unit = os.path.splitext(os.path.basename(after_path))[0]
    before, after = kernels(before_path), kernels(after_path)
    bad, seen = False, set()
    for old, body in before.items():
        new = RENAMED.get(old, old) if old not in after else old
        if new not in after:
            continue
        seen.add(new)
        count = lambda b: sum(1 for l in b if not l.endswith(":"))
        same = body == after[new]
        bad |= not same
        print(f"{unit:14s} {old + (' -> ' + new if new != old else ''):44s} {count(body):5d} {count(after[new]):5d}  {'yes' if same else 'NO'}")
    gone = [k for k in before if RENAMED.get(k, k) not in seen and k not in seen]
    came = [k for k in after if k not in seen]
    print(f"{unit:14s} went away: {', '.join(gone) if gone else '-'}")
    print(f"{unit:14s} appeared:  {', '.join(came) if came else '-'}")
    return 1 if bad or came else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
