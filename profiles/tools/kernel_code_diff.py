#!/usr/bin/env python3
"""Did a change of the source change the code of a kernel?  Compares two builds of one translation unit kernel by kernel:
the figures of -Rpass-analysis=kernel-resource-usage and the instruction streams of the gfx950 assembly.

  cd smallvcm_amd/csrc        (in the parent's tree and in this one; FLAGS are the Makefile's)
  hipcc $FLAGS --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o api.s vcm_api.hip 2> api.remarks
  python3 profiles/tools/kernel_code_diff.py parent/api.s parent/api.remarks new/api.s new/api.remarks [old=new ...]

Kernels are matched by demangled name without the parameter list; `old=new` (substrings of such names, applied in the
order given) renames the parent's kernels first.  A stream is the kernel's lines from its label to its end without
comments, labels and directives, with the function's number taken out of the block labels that branches name."""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for m, d in zip(names, out):
        d = d.replace("void ", "", 1).replace("vcm::", "")
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):   # the parameter list: the first '(' outside template brackets
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        res[m] = d[:cut]
    return res


def resources(path):
    res, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return res


def streams(path, wanted):
    """mangled name -> list of instruction lines, for the kernels in `wanted`"""
    res, cur = {}, None
    for line in open(path, errors="replace"):
        s = line.split(";", 1)[0].strip()
        if cur is None:
            if line[0] == "_" and s.endswith(":") and s[:-1] in wanted:
                cur = res.setdefault(s[:-1], [])
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.endswith(":") or s.startswith("."):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return res


def main():
    ps, pr, ns, nr = sys.argv[1:5]
    renames = [a.split("=", 1) for a in sys.argv[5:]]
    rp, rn = resources(pr), resources(nr)
    dp, dn = demangle(sorted(rp)), demangle(sorted(rn))
    for m in dp:
        for a, b in renames:
            if a in dp[m]:
                dp[m] = dp[m].replace(a, b)
                break
    byname_p, byname_n = {d: m for m, d in dp.items()}, {d: m for m, d in dn.items()}
    assert len(byname_p) == len(dp) and len(byname_n) == len(dn), "two kernels share a name"
    sp, sn = streams(ps, set(rp)), streams(ns, set(rn))
    print("kernels parent %d, new %d; only in parent %d, only in new %d" % (len(dp), len(dn), len(set(byname_p) - set(byname_n)), len(set(byname_n) - set(byname_p))))
    for d in sorted(set(byname_p) - set(byname_n)):
        print("  only in parent: " + d)
    for d in sorted(set(byname_n) - set(byname_p)):
        print("  only in new: " + d)
    common = sorted(set(byname_p) & set(byname_n))
    fmt = lambda r: " ".join("%s %s" % (f.split(" ")[0], r.get(f, "?")) for f in FIELDS)   # noqa: E731
    res_diff = [d for d in common if rp[byname_p[d]] != rn[byname_n[d]]]
    code_diff = [d for d in common if sp[byname_p[d]] != sn[byname_n[d]]]
    print("kernels of both: %d; with any differing figure %d; with a differing instruction stream %d; with scratch (new build) %d"
          % (len(common), len(res_diff), len(code_diff), sum(1 for r in rn.values() if r.get(FIELDS[3]) != "0")))
    for d in sorted(set(res_diff) | set(code_diff)):
        p, n = byname_p[d], byname_n[d]
        print("%s\n    %s, %d instructions\n -> %s, %d instructions" % (d, fmt(rp[p]), len(sp[p]), fmt(rn[n]), len(sn[n])))
    named = [d for d in common if any(a in dn[byname_n[d]] for _, a in renames)]
    if named:
        print("# the renamed kernels and those that share their new names")
        for d in named:
            p, n = byname_p[d], byname_n[d]
            print("%s\n    %s, %d instructions, %s" % (d, fmt(rn[n]), len(sn[n]), "stream and figures equal" if d not in res_diff and d not in code_diff else "DIFFERS (above)"))


if __name__ == "__main__":
    main()
