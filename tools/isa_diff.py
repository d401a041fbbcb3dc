#!/usr/bin/env python3
"""Did a change move any device code?  Compares two directories of gfx950 assembly listings (same file names, made with
build.py's FLAGS + FILE_FLAGS and ``-S --cuda-device-only``, as tests/test_isa_cpu.py makes them), function by function.

    python tools/isa_diff.py BEFORE_DIR AFTER_DIR [regex for a function whose signature changed ...]

A function's instruction stream is its listing without comments, directives and the numbers of its labels.  Every
function present on both sides must be identical, except those named on the command line (a regex that matches the
mangled name up to where the parameter types begin, e.g. 'cpq_cost_loss_kernelILb[01]E': the two sides are paired by the
text up to the end of the match): for them the registers, scratch, loads and wait groups of both sides are printed
(tools/isa_loads.py scan).  Exit status 1 if an unnamed function differs, appears or disappears, or a named one gains
scratch.
"""
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_loads import scan  # noqa: E402


def functions(path):
    """{mangled name: (instruction lines, kernel-descriptor lines, SGPR count)} of one listing."""
    out, name, last, sgprs = {}, None, None, {}
    desc, in_desc = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            name = last = m.group(1)
            out[name] = []
            continue
        m = re.match(r'\s*\.amdhsa_kernel\s+(\w+)', ln)
        if m:
            in_desc = m.group(1)
            desc[in_desc] = []
            continue
        if in_desc:
            if '.end_amdhsa_kernel' in ln:
                in_desc = None
            else:
                desc[in_desc].append(ln.strip())
            continue
        m = re.search(r';\s*TotalNumSgprs:\s*(\d+)', ln)  # (the "Kernel info" comment block follows the function's end label)
        if m and last:
            sgprs[last] = int(m.group(1))
        if name is None:
            continue
        if re.match(r'^\.Lfunc_end', ln):
            name = None
            continue
        code = ln.split(';')[0].strip()
        if not code or (code.startswith('.') and not code.endswith(':')):
            continue
        out[name].append(re.sub(r'\.(LBB\d+_|Lpost_getpc)\d+', r'.L', code))  # (long-branch labels are numbered per file)
    return {k: (v, desc.get(k, []), sgprs.get(k, 0)) for k, v in out.items()}


def main():
    before, after, changed = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0

    def key(name):  # a function whose signature changed: its name without the parameter types
        for c in changed:
            m = re.search(c, name)
            if m:
                return name[:m.end()], True
        return name, False

    def keyed(table):
        return {key(k)[0]: v for k, v in table.items()}
    for f in sorted(os.listdir(before)):
        if not f.endswith('.s'):
            continue
        fb, fa = keyed(functions(os.path.join(before, f))), keyed(functions(os.path.join(after, f)))
        sb, sa = keyed(scan(os.path.join(before, f))), keyed(scan(os.path.join(after, f)))
        same = same_p = 0
        for k in sorted(set(fb) | set(fa)):
            if k not in fb or k not in fa:
                print(f"{f}: {k} only {'before' if k in fb else 'after'}")
                bad += 1
            elif key(k)[1]:
                print(f"{f}: {k} (signature changed)")
                for tag, s, fn in (("before", sb, fb), ("after ", sa, fa)):
                    r = s[k]
                    print(f"    {tag}: vgprs {r['vgprs']:3d}  sgprs {fn[k][2]:3d}  scratch {r['scratch']}  loads {r['loads']:3d}"
                          f"  wait groups {r['waits']:3d}  instructions {len(fn[k][0])}")
                bad += sa[k]['scratch'] > sb[k]['scratch']
            elif fb[k][0] != fa[k][0] or fb[k][1] != fa[k][1]:
                print(f"{f}: {k} DIFFERS")
                for d in list(difflib.unified_diff(fb[k][0] + fb[k][1], fa[k][0] + fa[k][1], 'before', 'after', n=1, lineterm=''))[:60]:
                    print("    " + d)
                bad += 1
            else:
                same += 1
                same_p += '_kernel_p' in k
        print(f"{f}: {same} functions identical (instructions and kernel descriptor), {same_p} of them _p kernels")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
