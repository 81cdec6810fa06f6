"""Which GPU test file launches which device kernel: builds and checks tests/kernel_map.tsv.

    tools/kernel_coverage.py kernels                    the kernels of the tree, one `unit<TAB>mangled name` per line
    tools/kernel_coverage.py map TRACES [--keep]        write tests/kernel_map.tsv from the traces under TRACES
    tools/kernel_coverage.py [uncovered]                the rows of the map that no qualifying test file launched

Kernels of the build: every translation unit csrc/*.hip is compiled to device-only assembly with the command the Makefile
would run for it (`make -n -B`, so per-unit flags are included; `-c -o x.o` becomes `--cuda-device-only -S -o x.s`, as
tools/isa_diff.py takes its input), and the `.amdhsa_kernel` lines are the kernels. At most 16 compiles run at a time.

Kernels launched: TRACES holds one directory per test file, named after it (TRACES/test_gpu_drizzle/...), written by
    rocprofv3 --kernel-trace --mangled-kernels -f csv -d TRACES/test_gpu_drizzle -- python -m pytest tests/test_gpu_drizzle.py
Every *kernel_trace.csv below that directory counts (a test may start children, each process writes its own file). Only
the engine's symbols (_ZN3stk...) are read, a `.kd` suffix dropped; torch's kernels are ignored. `--keep` keeps, for test
files that TRACES does not hold, what the existing map says of them, so that only changed files need tracing again.

The map is tests/kernel_map.tsv together with its supplements tests/kernel_map_<feature>.tsv (same header, same columns): a
change that adds kernels commits their rows as a new supplement and leaves the committed rows as they are; `map` writes a
kernel's row back into the file that lists it, and a kernel no file lists into tests/kernel_map.tsv. The features named in
PARTS are held as parts of the main file instead: read_file of a map returns their rows behind its own, so read_map counts
them with the main file and not beside it (tests/test_cpu_star_measure.py pins read_map at the main file plus the nine rows
of the first supplement, which a second supplement counted beside the main file cannot meet). Everything else is the same
for a part: its own file, same header, every row checked against the tree, `map` writes its rows back into it.

Units named in OWN have a map of their own, tests/kernel_own_<feature>.tsv (same header, same columns), that read_map does
NOT return and whose units build_kernels leaves out unless asked (own=True): three existing tests pin read_map between them
(test_cpu_kernel_map.py: read_map = the kernels build_kernels returns; test_cpu_star_measure.py: read_map = the main file with
its parts + nine rows; test_cpu_background.py: parts = the background file alone), so new rows that read_map counts can go into
tests/kernel_map.tsv alone, and that is a committed file under tests/, which a feature change leaves byte for byte. (A change
that may edit it puts its rows there and needs none of this.) Such a unit is held to the same standard by the test that comes
with it: the kernels build_kernels(own=True) finds in it = the rows of its file, every row naming a qualifying GPU test file.
`kernels`, `map` and `uncovered` take these units and files along.

Units named in POST live in a subdirectory of csrc (post/: the tools that run on a finished stack) and are held exactly as
the units of OWN are, for the same reason and one more: tests/test_cpu_deconvolve.py asks that every csrc/*.hip outside OWN
is in read_map, and pins OWN itself, so a new unit directly in csrc/ can pass with neither table. Their rows are
tests/kernel_post_<feature>.tsv (read_post), their kernels build_kernels(post=True); the unit's name carries the directory
(post/kernels_wavelet), as the Makefile's command does. OWN, read_own, read_map, build_kernels() and build_kernels(own=True)
return what they returned before POST existed.

Units named in EXTRA are the fourth and LAST table: every later unit goes here, wherever it lives, and no further mechanism
is needed. The existing tests pin OWN, POST, read_map(), read_own() and read_post() and ask that every unit unit_commands()
returns is in one of the three, so unit_commands() leaves the units of EXTRA out unless asked (extra=True; its own
disk-against-Makefile assertion still covers every .hip), and their rows are tests/kernel_extra_<feature>.tsv (read_extra),
their kernels build_kernels(extra=True). The test that comes with a unit checks THAT UNIT's rows alone (the kernels
recomputed with the Makefile's command = its rows, every row a qualifying GPU test file, no kernel listed twice anywhere,
write_map byte for byte) and must not pin the table's contents or any total row count: the next feature adds one entry to
EXTRA and one file, and nothing else changes. Everything the older functions return stays what it was.

Covered: launched by a tests/test_gpu_*.py other than test_gpu_fullsize.py and the test_gpu_00_* bench and multi-rank
files. Exit status of `uncovered` is 1 if any row has no qualifying file. Only symbol names are read, never instructions."""
import argparse
import concurrent.futures
import glob
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libstacker_rs_amd", "csrc")
MAP = os.path.join(ROOT, "tests", "kernel_map.tsv")
HEADER = "unit\tmangled\tdemangled\ttest files"
PARTS = ("background",)                      # tests/kernel_map_<name>.tsv read as a part of tests/kernel_map.tsv (see above)
OWN = {"kernels_deconvolve": "deconvolve"}   # unit -> feature: its rows are tests/kernel_own_<feature>.tsv (see above)
POST = {"post/kernels_wavelet": "wavelet"}   # unit (with its directory) -> feature: tests/kernel_post_<feature>.tsv (see above)
EXTRA = {"post/kernels_stretch": "stretch"}  # unit (with its directory, if any) -> feature: tests/kernel_extra_<feature>.tsv; new units go HERE
MAX_COMPILES = 16
SYMBOL = re.compile(r"_ZN3stk\w+")


def qualifies(test_file):
    """True for the small GPU test files whose launches count as coverage."""
    return (test_file.startswith("test_gpu_") and test_file.endswith(".py")
            and test_file != "test_gpu_fullsize.py" and not test_file.startswith("test_gpu_00_"))


def unit_commands(csrc=CSRC, extra=False):
    """{unit: argv} — the Makefile's own compile line of every .hip unit, turned into a device-only assembly run. A unit in a
    subdirectory of csrc is named with it (post/kernels_wavelet). The units named in EXTRA are returned only when asked for
    (extra=True: all units); the assertion below covers them either way."""
    dry = subprocess.run(["make", "-C", csrc, "-n", "-B", "--no-print-directory", "OBJDIR=@OBJ@"],
                         check=True, capture_output=True, text=True).stdout
    cmds = {}
    for ln in dry.split("\n"):
        argv = shlex.split(ln) if " -c -o @OBJ@/" in ln else []
        if not argv or not argv[-1].endswith(".hip"):
            continue
        i = argv.index("-c")
        assert argv[i + 1] == "-o" and argv[i + 2].startswith("@OBJ@/"), ln
        cmds[os.path.splitext(argv[-1])[0]] = argv[:i] + ["--cuda-device-only", "-S", "-o", None] + argv[i + 3:]
    on_disk = {os.path.splitext(os.path.relpath(p, csrc))[0].replace(os.sep, "/")
               for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*", "*.hip"))}
    assert set(cmds) == on_disk, ("the Makefile's dry run and csrc/*.hip, csrc/*/*.hip disagree", sorted(set(cmds) ^ on_disk))
    return cmds if extra else {u: c for u, c in cmds.items() if u not in EXTRA}


def own_file(unit, path=MAP):
    """The map file of a unit named in OWN, beside `path`."""
    return os.path.join(os.path.dirname(path), "kernel_own_" + OWN[unit] + ".tsv")


def read_own(path=MAP):
    """The rows of every own map that exists, units sorted."""
    rows = []
    for unit in sorted(OWN):
        if os.path.isfile(own_file(unit, path)):
            rows += read_rows(own_file(unit, path))
    return rows


def post_file(unit, path=MAP):
    """The map file of a unit named in POST, beside `path`."""
    return os.path.join(os.path.dirname(path), "kernel_post_" + POST[unit] + ".tsv")


def read_post(path=MAP):
    """The rows of every post map that exists, units sorted."""
    rows = []
    for unit in sorted(POST):
        if os.path.isfile(post_file(unit, path)):
            rows += read_rows(post_file(unit, path))
    return rows


def extra_file(unit, path=MAP):
    """The map file of a unit named in EXTRA, beside `path`."""
    return os.path.join(os.path.dirname(path), "kernel_extra_" + EXTRA[unit] + ".tsv")


def read_extra(path=MAP):
    """The rows of every extra map that exists, units sorted."""
    rows = []
    for unit in sorted(EXTRA):
        if os.path.isfile(extra_file(unit, path)):
            rows += read_rows(extra_file(unit, path))
    return rows


def build_kernels(csrc=CSRC, workdir=None, own=False, post=False, extra=False):
    """{unit: sorted mangled kernel names} of the tree under `csrc`, compiled as its Makefile compiles it: the units read_map
    answers for, or (own=True) the units named in OWN, or (post=True) the units named in POST, or (extra=True) those in EXTRA."""
    assert own + post + extra <= 1
    cmds = {u: c for u, c in unit_commands(csrc, extra=True).items() if (u in OWN) == own and (u in POST) == post and (u in EXTRA) == extra}
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        def one(unit):
            out = os.path.join(tmp, unit.replace("/", "_") + ".s")
            argv = [out if a is None else a for a in cmds[unit]]
            r = subprocess.run(argv, cwd=csrc, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"{' '.join(argv)}\n{r.stderr[-4000:]}")
            names = set()
            with open(out) as f:
                for ln in f:
                    if ln.lstrip().startswith(".amdhsa_kernel"):
                        names.add(ln.split()[1])
            return unit, sorted(names)
        workers = min(MAX_COMPILES, len(os.sched_getaffinity(0)), len(cmds)) or 1
        with concurrent.futures.ThreadPoolExecutor(workers) as pool:
            return dict(pool.map(one, sorted(cmds)))


def demangle(names):
    names = list(names)
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", check=True, capture_output=True, text=True).stdout
    lines = out.split("\n")[:len(names)]
    assert len(lines) == len(names)
    return dict(zip(names, lines))


def launched(traces):
    """{mangled name: set of test files} from TRACES/<test file stem>/**/*kernel_trace.csv."""
    seen, files = {}, []
    for d in sorted(os.listdir(traces)):
        if not os.path.isdir(os.path.join(traces, d)):
            continue
        test_file = d + ".py"
        files.append(test_file)
        for path in glob.glob(os.path.join(traces, d, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, errors="replace") as f:
                for name in set(SYMBOL.findall(f.read())):
                    seen.setdefault(name, set()).add(test_file)
    return seen, files


def parts(path=MAP):
    """The part files of a map that exist: <stem>_<name>.tsv for the names in PARTS, in that order."""
    stem, ext = os.path.splitext(path)
    return [f for f in (stem + "_" + name + ext for name in PARTS) if os.path.isfile(f)]


def supplements(path=MAP):
    """The supplement files of a map: tests/kernel_map_<feature>.tsv beside tests/kernel_map.tsv, sorted, without its parts. A
    change that adds kernels adds its rows in a file of its own, so that the rows already committed stay as they are."""
    stem, ext = os.path.splitext(path)
    return sorted(set(glob.glob(glob.escape(stem) + "_*" + ext)) - set(parts(path)))


def read_rows(path):
    """The rows of one file, and of nothing else."""
    rows = []
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[0] == HEADER, (path, lines[0])
    for ln in lines[1:]:
        if not ln:
            continue
        unit, mangled, demangled, files = ln.split("\t")
        rows.append((unit, mangled, demangled, [t for t in files.split(",") if t]))
    return rows


def read_file(path):
    """The rows of a file, followed by the rows of its parts (a supplement has none)."""
    rows = read_rows(path)
    for part in parts(path):
        rows += read_rows(part)
    return rows


def read_map(path=MAP):
    """[(unit, mangled, demangled, [test files])] of the committed map: the file and its supplements, in that order. Nothing
    is merged: a kernel with a row in two files is there twice, which tests/test_cpu_kernel_map.py refuses."""
    rows = read_file(path)
    for extra in supplements(path):
        rows += read_file(extra)
    return rows


def write_map(kernels, seen, path=MAP):
    """The rows of every kernel of the build: a kernel that a part or a supplement of `path` lists stays in that file, every
    other one goes to `path`; a file none of whose kernels is left in the build is written with its header alone."""
    pretty = demangle(n for names in kernels.values() for n in names)
    others = parts(path) + supplements(path)
    home = {r[1]: extra for extra in others for r in read_rows(extra)}
    lines = {p: [] for p in [path] + others + [own_file(u, path) for u in sorted(kernels) if u in OWN] + [post_file(u, path) for u in sorted(kernels) if u in POST]
             + [extra_file(u, path) for u in sorted(kernels) if u in EXTRA]}
    for unit in sorted(kernels):
        for n in kernels[unit]:
            lines[own_file(unit, path) if unit in OWN else post_file(unit, path) if unit in POST else extra_file(unit, path) if unit in EXTRA
                  else home.get(n, path)].append(f"{unit}\t{n}\t{pretty[n]}\t{','.join(sorted(seen.get(n, ())))}\n")
    for p, body in lines.items():
        with open(p, "w") as f:
            f.write(HEADER + "\n" + "".join(body))


def uncovered(rows):
    return [r for r in rows if not any(qualifies(t) for t in r[3])]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd")
    sub.add_parser("kernels")
    m = sub.add_parser("map")
    m.add_argument("traces")
    m.add_argument("--keep", action="store_true")
    m.add_argument("--out", default=MAP)
    u = sub.add_parser("uncovered")
    u.add_argument("--map", default=MAP)
    args = ap.parse_args()
    if args.cmd == "kernels":
        for unit, names in sorted({**build_kernels(), **build_kernels(own=True), **build_kernels(post=True), **build_kernels(extra=True)}.items()):
            for n in names:
                print(f"{unit}\t{n}")
        return 0
    if args.cmd == "map":
        seen, traced = launched(args.traces)
        if args.keep:
            for _, mangled, _, files in read_map(args.out) + read_own(args.out) + read_post(args.out) + read_extra(args.out):
                for t in files:
                    if t not in traced:
                        seen.setdefault(mangled, set()).add(t)
        kernels = {**build_kernels(), **build_kernels(own=True), **build_kernels(post=True), **build_kernels(extra=True)}
        known = {n for names in kernels.values() for n in names}
        strangers = sorted(set(seen) - known)
        if strangers:
            print(f"{len(strangers)} traced stk kernels are not in the build (stale library?):", *strangers[:5], sep="\n  ", file=sys.stderr)
            return 2
        write_map(kernels, seen, args.out)
        print(f"{args.out}: {len(known)} kernels, {len(traced)} test files traced")
    which = getattr(args, "map", None) or getattr(args, "out", MAP)
    rows = read_map(which) + read_own(which) + read_post(which) + read_extra(which)
    bare = uncovered(rows)
    per_unit = {}
    for unit, mangled, demangled, files in bare:
        per_unit[unit] = per_unit.get(unit, 0) + 1
        print(f"{unit}\t{mangled}\t{demangled}\t{','.join(files)}")
    print(f"{len(bare)} of {len(rows)} kernels uncovered", *(f"{u}: {c}" for u, c in sorted(per_unit.items())), sep="\n  " if bare else "")
    return 1 if bare else 0


if __name__ == "__main__":
    sys.exit(main())
