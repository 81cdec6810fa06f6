"""Kernel by kernel, the gfx950 ISA of two builds of one translation unit: tools/isa_diff.py parent.s branch.s [substring]
(the .s files from `hipcc ... --cuda-device-only -S`). Prints the kernels only one side has, and per kernel on both sides
whether the instruction text is identical (block labels renumbered, comments and directives dropped), with line count,
VGPRs, SGPRs, scratch and occupancy where it differs or where `substring` selects it. Exit status 1 if the symbol sets or
any ISA differ. (tools/isa_loops.py gives the loops of one kernel, for the ones that differ.)"""
import re
import sys


def kernels(path):
    out, name, body, meta = {}, None, [], {}
    for ln in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body, meta = m.group(1), [], {}
            continue
        if name is None:
            continue
        if ln.startswith(".Lfunc_end"):
            out[name] = [body, meta]
            name = None
            continue
        t = ln.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body.append(re.sub(r"\.?LBB\d+_", "LBB_", t))
    # the resource comments follow .Lfunc_end
    cur = None
    for ln in open(path).read().split("\n"):
        m = re.match(r"^\s*\.size\s+(_Z\w+),", ln)
        if m:
            cur = m.group(1)
        m = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m and cur in out:
            out[cur][1][m.group(1)] = int(m.group(2))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pick = sys.argv[3] if len(sys.argv) > 3 else None
    bad = 0
    for k in sorted(set(a) ^ set(b)):
        print("only in", "parent" if k in a else "branch", k)
        bad = 1
    same = 0
    for k in sorted(set(a) & set(b)):
        eq = a[k][0] == b[k][0]
        same += eq
        bad |= not eq
        if not eq or (pick and pick in k):
            print(f"{'identical' if eq else 'DIFFERENT'} {k}\n    parent {len(a[k][0])} lines {a[k][1]}\n    branch {len(b[k][0])} lines {b[k][1]}")
    print(f"{sys.argv[2]}: {len(a)} / {len(b)} kernels, {same} identical")
    sys.exit(bad)


if __name__ == "__main__":
    main()
