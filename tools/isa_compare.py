"""Per-kernel comparison of two device-assembly listings of the same source file (a refactor's proof that device code did not move).

    hipcc <the FLAGS of __graft_entry__.py> --cuda-device-only -S csrc/FILE.hip -o DIR/FILE.s        (old tree, new tree)
    python tools/isa_compare.py OLD_DIR NEW_DIR FILE.s [FILE.s ...] [--may-differ REGEX] [--rename REGEX=REPL ...]

For every kernel the function text, the .amdhsa_kernel block (registers, scratch, LDS, occupancy inputs) and the metadata entry
are compared.  Kernels are matched by demangled name WITHOUT their parameter list, so that a renamed argument struct does not count;
block labels are renumbered per kernel (the order of instantiation may change) and the __hip_cuid_ symbol is ignored.
Each --rename rewrites the OLD listing's demangled kernel names (re.sub) before matching, for a kernel the change renamed or merged.
Kernels whose name matches --may-differ are reported with the registers, scratch and LDS of both sides but do not fail the run.
Exit status 1 on any other difference.
"""
import argparse
import os
import re
import subprocess
import sys

CXXFILT = os.environ.get("CXXFILT", "c++filt")


def demangle(syms):
    out = subprocess.run([CXXFILT], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    names = {}
    for s, d in zip(syms, out):
        depth, i = 0, len(d)
        while d.endswith(")"):   # drop the trailing parameter list (matching parenthesis from the end)
            i -= 1
            depth += (d[i] == ")") - (d[i] == "(")
            if depth == 0:
                d = d[:i]
        names[s] = re.sub(r"^void ", "", d)
    return names


def kernels_of(path, renames=()):
    text = open(path).read()
    syms = sorted(set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)), key=len, reverse=True)
    names = demangle(syms)
    for pat, repl in renames:
        names = {s: re.sub(pat, repl, d) for s, d in names.items()}
    assert len(set(names.values())) == len(syms), "kernel names collide once their parameter lists are dropped"
    for s in syms:   # longest first: no symbol is a prefix of a later one
        text = text.replace(s, "<" + names[s] + ">")
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", text)
    text = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", text)
    text = re.sub(r"(?<![A-Za-z0-9_])(\.L)?BB\d+_(\d+)", r"\1BB_\2", text)   # block labels and the loop comments that name them: drop the function's index
    res = {}
    for s in syms:
        n = re.escape("<" + names[s] + ">")
        body = re.search(r"^%s:.*?^\s*\.end_amdhsa_kernel" % n, text, re.M | re.S)
        meta = re.search(r"^  - \.agpr_count:(?:(?!^  - \.agpr_count:).)*?\.name:\s+'?%s'?\n.*?(?=^  - \.agpr_count:|^amdhsa\.target)" % n, text, re.M | re.S)
        assert body and meta, names[s]
        res[names[s]] = (body.group(0), meta.group(0))
    return res


def resources(body):
    """vgpr / sgpr / scratch / LDS of a kernel, from its .amdhsa block"""
    keys = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))
    return " ".join(name + "=" + re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1) for name, k in keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--may-differ", default=None)
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    bad = 0
    for f in a.files:
        old, new = kernels_of(os.path.join(a.old_dir, f), renames), kernels_of(os.path.join(a.new_dir, f))
        print(f"{f}: {len(old)} kernels before, {len(new)} after; appeared: {sorted(set(new) - set(old)) or 'none'}; vanished: {sorted(set(old) - set(new)) or 'none'}")
        bad += len(set(old) ^ set(new))
        for k in sorted(set(old) & set(new)):
            diff = [what for what, o, n in (("code + .amdhsa block", old[k][0], new[k][0]), ("metadata", old[k][1], new[k][1])) if o != n]
            allowed = bool(diff) and a.may_differ and re.search(a.may_differ, k)
            regs = re.search(r"\.amdhsa_next_free_vgpr (\d+)", new[k][0]).group(1)
            print(f"  {k}: " + ("identical" if not diff else "differs: " + ", ".join(diff) + (" (allowed)" if allowed else "")) + f"  [{new[k][0].count(chr(10))} lines, vgpr {regs}]")
            if diff:
                print(f"    before: {resources(old[k][0])}\n    after:  {resources(new[k][0])}")
            bad += bool(diff) and not allowed
    print("verdict:", "DIFFERENCES" if bad else "every kernel outside --may-differ identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
