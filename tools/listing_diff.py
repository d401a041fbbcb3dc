"""Per-kernel comparison of two directories of device listings (`hipcc -S --cuda-device-only`, one NAME.s per source).

Per kernel: whether the code text is identical, the instruction count, and VGPRs, SGPRs, scratch, LDS and occupancy from
the metadata comments behind the kernel, on both sides.  Text and metadata only.

usage: python tools/listing_diff.py DIR_A DIR_B [--json OUT] [--all]     (the table lists differing kernels; --all: every)
"""
import json
import os
import re
import subprocess
import sys

META = {"vgpr": "TotalNumVgprs", "sgpr": "TotalNumSgprs", "scratch": "ScratchSize", "lds": "LDSByteSize", "occ": "Occupancy"}


def kernels(path):
    """{kernel symbol: (code lines, {resource: int})} of one listing"""
    lines = open(path, errors="replace").read().split("\n")
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel (\S+)", ln))]
    out = {}
    for name in names:
        i = next(k for k, ln in enumerate(lines) if ln.startswith(name + ":"))
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        # a label carries the function's ordinal in its file (.LBB12_3): not part of the comparison
        code = [re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", ln) for ln in lines[i + 1:j]]
        res = {}
        for ln in lines[j:]:
            if ln.startswith("\t.section\t.text") and res:
                break
            for key, tag in META.items():
                if (m := re.match(r"; %s: (\d+)" % tag, ln)) and key not in res:
                    res[key] = int(m.group(1))
        out[name] = (code, res)
    return out


def n_instr(code):
    return sum(1 for ln in code if re.match(r"\t[a-z]\w+", ln))


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", o) for o in out]


def compare(dir_a, dir_b):
    rows = []
    for f in sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b))):
        if not f.endswith(".s"):
            continue
        ka, kb = (kernels(os.path.join(d, f)) if os.path.exists(os.path.join(d, f)) else {} for d in (dir_a, dir_b))
        syms = sorted(set(ka) | set(kb))
        for sym, name in zip(syms, demangle(syms)):
            (ca, ra), (cb, rb) = ka.get(sym, ([], {})), kb.get(sym, ([], {}))
            rows.append({"file": f, "kernel": name, "identical": ca == cb and ra == rb, "instr": [n_instr(ca), n_instr(cb)],
                         "instr_delta": n_instr(cb) - n_instr(ca), **{k: [ra.get(k), rb.get(k)] for k in META}})
    return rows


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = compare(args[0], args[1])
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump({"kernels": len(rows), "identical": sum(r["identical"] for r in rows),
                       "differing": [r for r in rows if not r["identical"]],
                       "identical_by_file": {f: sum(r["identical"] for r in rows if r["file"] == f)
                                             for f in sorted({r["file"] for r in rows})}}, f, indent=1)
            f.write("\n")
    print(f"{'file':14s} {'kernel':64s} {'same':>4s} {'instr':>13s} {'vgpr':>9s} {'sgpr':>9s} {'scratch':>9s} {'lds':>13s} {'occ':>5s}")
    for r in rows:
        if r["identical"] and "--all" not in sys.argv:
            continue
        pair = lambda k: "%s/%s" % tuple(r[k])
        print(f"{r['file']:14s} {r['kernel'][:64]:64s} {'yes' if r['identical'] else 'NO':>4s} {pair('instr'):>13s} "
              f"{pair('vgpr'):>9s} {pair('sgpr'):>9s} {pair('scratch'):>9s} {pair('lds'):>13s} {pair('occ'):>5s}")
    print(f"{sum(r['identical'] for r in rows)} of {len(rows)} kernels identical")
