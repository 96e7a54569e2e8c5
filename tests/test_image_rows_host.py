"""The partition's arithmetic on the host (csrc/jpt_image.cpp: rows_of_rank, max_rows_of_any_rank, scatter_rows), by
tests/cpp/image_rows_test.cpp: heights 0, 1, 7, 8, 9, 20, 24 and 65 under worlds 1, 2, 3 and 5 at widths 1 and 3.  The program checks that
the shares sum to the height, that the scatter writes each image row exactly once and from the right local row, and that the piece is
the largest share; the rows it prints are compared here with gdpathtracing_amd/partition.py, which the gathers use.  CPU only."""
import os
import re
import subprocess

import pytest

from gdpathtracing_amd import capi, partition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
with open(os.path.join(capi.CSRC, "Makefile")) as _f:   # the host layer's own flags
    CXXFLAGS = re.search(r"^CXXFLAGS\s*:=\s*(.+)$", _f.read(), re.M).group(1).split()

HEIGHTS, WORLDS, WIDTHS = (0, 1, 7, 8, 9, 20, 24, 65), (1, 2, 3, 5), (1, 3)


@pytest.fixture(scope="module")
def printed(hiplib, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows") / "image_rows_test")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call([HIPCC] + CXXFLAGS + ["-x", "c++", os.path.join(ROOT, "tests", "cpp", "image_rows_test.cpp"), "-o", exe,
                                                 "-L", libdir, "-ljpt_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows, pieces = {}, {}
    for text in out.stdout.splitlines():
        key, _, rest = text.partition(":")
        kind, *numbers = key.split()
        numbers = tuple(int(n) for n in numbers)
        assert numbers not in (rows if kind == "rows" else pieces), text
        if kind == "rows":
            rows[numbers] = [int(y) for y in rest.split()]
        else:
            assert kind == "piece", text
            pieces[numbers] = int(rest)
    return rows, pieces


def test_every_case_is_printed(printed):
    rows, pieces = printed
    assert sorted(pieces) == sorted((h, world, w) for h in HEIGHTS for world in WORLDS for w in WIDTHS)
    assert sorted(rows) == sorted((h, world, w, r) for h in HEIGHTS for world in WORLDS for w in WIDTHS for r in range(world))


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_the_rows_are_partition_py_s(printed, h, world):
    rows, pieces = printed
    for w in WIDTHS:
        for r in range(world):
            assert rows[(h, world, w, r)] == partition.rows_of_rank(h, r, world).tolist()
        assert pieces[(h, world, w)] == partition.max_local_rows(h, world)


def test_the_ragged_shape_of_the_gpu_tests(printed):
    """16 x 20 under world 2 (tests/test_gpu_image_restarts.py): strips of 8, 8 and 4 rows; rank 0 holds 12 rows, rank 1 holds 8."""
    rows, pieces = printed
    assert rows[(20, 2, 3, 0)] == list(range(0, 8)) + list(range(16, 20))
    assert rows[(20, 2, 3, 1)] == list(range(8, 16))
    assert pieces[(20, 2, 3)] == 12
