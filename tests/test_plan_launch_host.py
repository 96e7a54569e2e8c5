"""jpt::plan_launch (csrc/jpt_render.cpp) -- every measured scheduling rule of a render's launch shape: the route, the slots (4, 6 where six
queues run side by side, the host's cap, 2 past 24 GiB), the chain (1, 2 or 4), frame groups from 12 Mi paths, the lone-async fallback after
three idle renders -- against a fake device, by tests/cpp/plan_launch_test.cpp on host-only contexts.  The expected values are the rules as
written, not the program's output.  CPU only."""
import os
import re
import subprocess

import pytest

from gdpathtracing_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
with open(os.path.join(capi.CSRC, "Makefile")) as _f:   # the host layer's own flags
    CXXFLAGS = re.search(r"^CXXFLAGS\s*:=\s*(.+)$", _f.read(), re.M).group(1).split()


def line(route, slot=0, slots=0, groups=1, chain=1, six=0, idle=0, slot_stream=0, group_streams=0, asked_for=0, last_pipe_slots=0, idle_streak=0):
    return ("%s slot %d slots %d groups %d chain %d | asked six %d idle %d slot_stream %d group_streams %d (for %d) | last_pipe_slots %d idle_streak %d"
            % (route, slot, slots, groups, chain, six, idle, slot_stream, group_streams, asked_for, last_pipe_slots, idle_streak))


ASKED_ONCE = dict(six=1, idle=1, slot_stream=1)
ROW_3 = dict(groups=1, chain=2)   # the blocking shape of a small native render
ROWS = {
    "1": line("kReference"),
    "2": line("kReference"),
    "3": line("kStream", last_pipe_slots=7, idle_streak=2, **ROW_3),
    "4": line("kStream", chain=1),
    "5": line("kStream", groups=2, chain=2, group_streams=1, asked_for=2),
    "6": line("kStream", groups=1, chain=1, group_streams=1, asked_for=2),
    "7": line("kStream", groups=1, chain=1),
    "8": line("kStream", groups=1, chain=1),
    "9": line("kSlot", slot=1, slots=4, chain=4, last_pipe_slots=4, **ASKED_ONCE),
    "10": line("kSlot", slot=5, slots=6, chain=4, last_pipe_slots=6, **ASKED_ONCE),
    "11": line("kSlot", slot=0, slots=1, chain=1, last_pipe_slots=1, idle=1, slot_stream=1),
    "12": line("kStream", six=1, last_pipe_slots=4, idle_streak=2, **ROW_3),
    "13": line("kStream", last_pipe_slots=4, **ASKED_ONCE, **ROW_3),
    "14a": line("kSlot", slot=1, slots=4, chain=4, last_pipe_slots=4, idle_streak=1, six=1, idle=1, slot_stream=1),
    "14b": line("kSlot", slot=1, slots=4, chain=4, last_pipe_slots=4, idle_streak=2, six=2, idle=2, slot_stream=2),
    "14c": line("kStream", last_pipe_slots=4, idle_streak=3, six=3, idle=3, slot_stream=2, **ROW_3),
    "14d": line("kStream", last_pipe_slots=4, idle_streak=4, six=4, idle=4, slot_stream=2, **ROW_3),
    "14e": line("kSlot", slot=1, slots=4, chain=4, last_pipe_slots=4, idle_streak=0, six=5, idle=5, slot_stream=3),
    "15": line("kSlot", slot=1, slots=2, chain=1, last_pipe_slots=2, idle=1, slot_stream=1),
}


@pytest.fixture(scope="module")
def planned(hiplib, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_launch_test")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call([HIPCC] + CXXFLAGS + ["-x", "c++", os.path.join(ROOT, "tests", "cpp", "plan_launch_test.cpp"), "-o", exe,
                                                 "-L", libdir, "-ljpt_hip", "-Wl,-rpath," + libdir])
    env = {k: v for k, v in os.environ.items() if k not in ("JPT_PIPELINE", "JPT_PIPE_SLOTS", "JPT_GROUPS")}
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr
    got = {}
    for text in out.stdout.splitlines():
        row, _, rest = text.partition(": ")
        assert row not in got, text
        got[row] = rest
    return got


def test_every_row_is_printed(planned):
    assert sorted(planned) == sorted(list(ROWS) + ["15 size"])


@pytest.mark.parametrize("row", list(ROWS))
def test_the_plan_of_each_row(planned, row):
    assert planned[row] == ROWS[row]


def test_row_15_is_planned_at_a_size_past_24_gib(planned):
    assert planned["15 size"] == "huge 1"
