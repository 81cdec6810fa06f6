"""tests/kernel_map.tsv is the tree's: every device kernel the Makefile builds has a row, every row names a GPU test file that
launched it (tools/kernel_coverage.py). The kernel set is recomputed here the way the tool computes it — each
csrc/*.hip unit to device-only assembly with the Makefile's own command, in a temporary directory — so a kernel that is
added, removed or renamed without a mapped test fails the CPU suite. Only kernel symbol names are read."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
kc = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kc)


@pytest.fixture(scope="module")
def rows():
    return kc.read_map()


def test_no_row_is_empty_and_none_repeats(rows):
    assert rows
    for unit, mangled, demangled, files in rows:
        assert unit and mangled.startswith("_ZN3stk") and "stk::" in demangled and files, (unit, mangled)
        assert files == sorted(set(files)), (mangled, files)
    assert len({r[1] for r in rows}) == len(rows)


def test_every_row_names_a_qualifying_gpu_test_file(rows):
    """A qualifying file: tests/test_gpu_*.py, not the full-size or the test_gpu_00_* files, present and marked gpu."""
    marked = {}

    def has_gpu_mark(name):
        if name not in marked:
            path = os.path.join(TESTS, name)
            marked[name] = os.path.isfile(path) and re.search(r"pytest\.mark\.gpu\b", open(path).read()) is not None
        return marked[name]
    bare = [(unit, demangled) for unit, _, demangled, files in rows if not any(kc.qualifies(t) and has_gpu_mark(t) for t in files)]
    assert not bare, f"{len(bare)} kernels without a small GPU test that launches them: {bare[:10]}"
    named = {t for r in rows for t in r[3]}
    assert all(os.path.isfile(os.path.join(TESTS, t)) for t in named), sorted(t for t in named if not os.path.isfile(os.path.join(TESTS, t)))


def test_the_map_lists_the_kernels_of_the_tree(rows, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is None:
        pytest.skip(f"no hipcc at {hipcc}: the kernel set of the tree cannot be recomputed")
    built = {(unit, n) for unit, names in kc.build_kernels(workdir=str(tmp_path)).items() for n in names}
    mapped = {(r[0], r[1]) for r in rows}
    assert built == mapped, (f"{len(built - mapped)} kernels of the tree have no row in tests/kernel_map.tsv, {len(mapped - built)} rows name no "
                             f"kernel of the tree; trace the tests that launch them and run tools/kernel_coverage.py map",
                             sorted(built - mapped)[:5], sorted(mapped - built)[:5])
