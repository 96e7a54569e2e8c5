"""The scene on the host through the C ABI alone, by tests/cpp/host_scene_test.cpp: begin, commit, set transform and update with each
builder; a native and an as-given upload, each with an accepted and a rejected jpt_scene_update_reference_tlas; jpt_scene_share; destroy.
The program prints every step's return code, tree kind and upload note and the size and a checksum of each of the nine reference
buffers; what it prints is compared, line for line, with the recording made with the library as it was before the host scene got a
file of its own (tests/golden/host_scene_test.txt).  Host-only contexts, CPU only."""
import os
import re
import subprocess

import pytest

from gdpathtracing_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
with open(os.path.join(capi.CSRC, "Makefile")) as _f:   # the host layer's own flags
    CXXFLAGS = re.search(r"^CXXFLAGS\s*:=\s*(.+)$", _f.read(), re.M).group(1).split()


@pytest.fixture(scope="module")
def printed(hiplib, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_scene") / "host_scene_test")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call([HIPCC] + CXXFLAGS + ["-x", "c++", os.path.join(ROOT, "tests", "cpp", "host_scene_test.cpp"), "-o", exe,
                                                 "-L", libdir, "-ljpt_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "host_scene_test.txt")) as f:
        return f.read().splitlines()


def test_every_step_prints_what_was_recorded(printed, recorded):
    assert printed == recorded


def test_the_recording_holds_every_step(recorded):
    steps = [text.split(":")[0] for text in recorded if not text.startswith(" ") and ":" in text]
    want = ["%s %s" % (s, b) for b in ("exact", "sah", "watertight") for s in ("commit", "set transform", "update")]
    want += ["%s %s" % (s, m) for m in ("native", "as given") for s in ("upload", "accepted update", "rejected update")]
    want += ["share from sah", "the source after it", "update of the copy", "share from native upload"]
    assert steps == want and recorded[-1] == "destroyed"
    rcs = {text.split(":")[0]: int(text.split(" rc ")[1].split()[0]) for text in recorded if " rc " in text}
    assert [s for s, rc in rcs.items() if rc != 0] == ["rejected update native", "rejected update as given"]


def test_a_rejected_update_prints_the_buffers_of_the_accepted_one(recorded):
    def block(step):
        i = next(k for k, text in enumerate(recorded) if text.startswith(step + ":"))
        return recorded[i + 1:i + 10]
    for mode in ("native", "as given"):
        assert block("rejected update " + mode) == block("accepted update " + mode) != block("upload " + mode)
