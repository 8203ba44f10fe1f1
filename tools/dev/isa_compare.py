#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device listings of the same source file (no GPU needed): registers, scratch, spills and instruction
count per kernel, and whether the instruction streams are identical once basic-block labels are renumbered.  For kernels that differ
it also compares the opcode sequence of the largest basic block and the counts of the fp64 / reciprocal and of the load opcodes.
Listings:  hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --offload-device-only -S -o new.s turbomesh_amd/csrc/tm_kernels.hip
usage: isa_compare.py parent.s new.s [name filter ...]   (filters select the kernels listed one by one; the rest is summarised)"""
import collections, re, subprocess, sys


def kernels(path):
    """name -> {vgpr, sgpr, scratch, spills, blocks: [[instruction, ...], ...]} with labels renumbered in order of appearance"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:(.*?)^; COMPUTE_PGM_RSRC2:SCRATCH_EN", text, re.S | re.M):
        name, body, info = m.group(1), m.group(2), m.group(3)
        if ".amdhsa_kernel" not in body:
            continue   # a device function, not a kernel
        labels, blocks = {}, [[]]
        for line in body.split("\n"):
            line = line.split(";")[0].rstrip()
            lab = re.match(r"^(\.LBB\d+_\d+):", line)
            if lab:
                blocks.append([])
                continue
            if not re.match(r"^\t[a-z]", line):
                continue   # directives, blank lines
            ins = re.sub(r"\.LBB\d+_\d+", lambda t: "L%d" % labels.setdefault(t.group(0), len(labels)), " ".join(line.split()))
            blocks[-1].append(ins)
        g = lambda key: int(re.search(r"; %s: (\d+)" % key, info).group(1))
        out[name] = dict(vgpr=g("NumVgprs"), sgpr=g("TotalNumSgprs"), scratch=g("ScratchSize"), blocks=blocks)
    for entry in text.split("- .agpr_count")[1:]:   # the metadata note: spill counts
        sym = re.search(r"\.symbol:\s+(\S+)\.kd", entry)
        if sym and sym.group(1) in out:
            out[sym.group(1)]["spills"] = sum(int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", entry))
    return out


def flat(k):
    return [i for b in k["blocks"] for i in b]


def opcodes(instrs):
    return [i.split()[0] for i in instrs]


def counts(k, pred):
    return collections.Counter(o for o in opcodes(flat(k)) if pred(o))


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    filters = sys.argv[3:]
    names = sorted(set(old) & set(new))
    dem = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")))
    short = lambda n: dem[n].split("(")[0].replace("void ", "").replace("tmh::", "")
    print(f"{len(old)} kernels in the parent, {len(new)} in the new listing, {len(names)} by the same name"
          + "".join(f"\n  only in the parent: {n}" for n in sorted(set(old) - set(new))) + "".join(f"\n  only in the new listing: {n}" for n in sorted(set(new) - set(old))))
    print(f"{'kernel':58s} {'VGPRs':>9s} {'SGPRs':>9s} {'scratch':>9s} {'spills':>7s} {'instructions':>13s}  (parent/new)")
    rest_same, rest_diff = 0, []
    for n in names:
        a, b = old[n], new[n]
        same = flat(a) == flat(b)
        if filters and not any(f in short(n) for f in filters):
            rest_same += same
            if not same:
                rest_diff.append(short(n))
            continue
        pair = lambda key: f"{a[key]}/{b[key]}"
        line = f"{short(n)[:58]:58s} {pair('vgpr'):>9s} {pair('sgpr'):>9s} {pair('scratch'):>9s} {pair('spills'):>7s} {len(flat(a)):>6d}/{len(flat(b)):<6d}  "
        if same:
            print(line + "identical")
            continue
        big = lambda k: opcodes(max(k["blocks"], key=len))
        f64 = lambda o: (o.startswith("v_") and "f64" in o) or o.startswith("v_rcp")
        load = lambda o: "load" in o
        verdict = [f"largest block ({len(big(a))}/{len(big(b))} instructions) " + ("same opcodes" if big(a) == big(b) else "DIFFERS"),
                   "fp64/rcp counts " + ("same" if counts(a, f64) == counts(b, f64) else "DIFFER"),
                   "load counts " + ("same" if counts(a, load) == counts(b, load) else "DIFFER")]
        print(line + "differs: " + ", ".join(verdict))
        delta = collections.Counter(opcodes(flat(b)))
        delta.subtract(collections.Counter(opcodes(flat(a))))
        print(" " * 8 + "opcode count changes: " + " ".join(f"{o}{d:+d}" for o, d in sorted(delta.items()) if d))
    if filters:
        print(f"other kernels: {rest_same} identical, {len(rest_diff)} differ" + "".join(f"\n  differs: {n}" for n in rest_diff))


if __name__ == "__main__":
    main()
