"""The compiled form of a tracing round, second part (CPU: hipcc cross-compiles to ISA without a GPU; compile, flags and helpers
of tests/test_round_isa.py).  In the tracing launches the walk's flags `have` and `in_blas` are two wave-uniform lane masks in
scalars and the stack position is the LDS address of the lane's next entry (walk_round_masked, trace_queue: jpt_kernels_wf2.hip;
Traversal::Masked, push_at / pop_at: jpt_trace_core.h).  What that buys is pinned here, for both instantiations the renders run:

 - no ballot of a flag or a conjunction is left (0 v_cndmask_b32 0/1 + v_cmp_ne_u32 pairs; 2 before);
 - no flag lives as a 0/1 byte in a VGPR: no `v_and_b32 v, 1, v` + `v_cmp_eq_u32 1, v` test and no v_cmp_ne_u16_sdwa ballot;
 - a pop is the decrement of the address, at most ONE more address instruction (the clamp to the last LDS row) and the read;
 - the masks did not cost the round SGPR spills (no v_writelane)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_wf2.hip")

KERNELS = ["9wf2_traceILb0ELb1ELb0E", "9wf2_traceILb0ELb1ELb1E"]
STRIDE_BYTES = 256 * 4   # one stack entry up or down a lane's column: kTraceBlock words


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc in this environment")
    out = str(tmp_path_factory.mktemp("isa") / "wf2.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]   # csrc/Makefile's
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return open(out).read()


def body_of(isa, kernel):
    return re.search(r"\n_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*:.*?s_endpgm", isa, re.S).group(0).splitlines()


def instructions(lines):
    """[(mnemonic, [operands])] of the body, labels kept as ("label", [name]) so that a search can stop at a block's start"""
    out = []
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):", l)
        if m:
            out.append(("label", [m.group(1)]))
            continue
        m = re.match(r"^\s+([a-z]\w+)\s*(.*?)\s*(?:;.*)?$", l)
        if m:
            out.append((m.group(1), [o.strip() for o in m.group(2).split(",")] if m.group(2) else []))
    return out


def ballot_pairs(lines):
    """v_cndmask_b32 vN, 0, 1, mask followed within a few lines by v_cmp_ne_u32 .., 0, vN (tests/test_round_isa.py)"""
    n = 0
    for i, l in enumerate(lines):
        m = re.match(r"\s*v_cndmask_b32(?:_e64)?\s+(v\d+), 0, 1,", l)
        if m and any(re.match(r"\s*v_cmp_ne_u32(?:_e32|_e64)?\s+.*\b0, %s\b" % m.group(1), l2) for l2 in lines[i + 1:i + 6]):
            n += 1
    return n


def flag_tests(lines):
    """v_and_b32 vN, 1, vM followed within a few lines by v_cmp_eq_u32 .., 1, vN: the test of a flag kept as a 0/1 byte"""
    n = 0
    for i, l in enumerate(lines):
        m = re.match(r"\s*v_and_b32(?:_e32|_e64)?\s+(v\d+), 1, v\d+", l)
        if m and any(re.match(r"\s*v_cmp_eq_u32(?:_e32|_e64)?\s+.*\b1, %s\b" % m.group(1), l2) for l2 in lines[i + 1:i + 6]):
            n += 1
    return n


def is_decrement(mn, ops):
    """one entry down: v_add_u32 v, 0xfffffc00, v  /  v_subrev_u32 v, 0x400, v  /  v_sub_u32 v, v, 0x400 (any encoding suffix)"""
    base = re.sub(r"_(e32|e64)$", "", mn)
    consts = [o.lower() for o in ops[1:]]
    if base == "v_add_u32":
        return any(c in ("0x%x" % (2 ** 32 - STRIDE_BYTES), str(-STRIDE_BYTES)) for c in consts)
    if base in ("v_sub_u32", "v_subrev_u32"):
        return any(c in ("0x%x" % STRIDE_BYTES, str(STRIDE_BYTES)) for c in consts)
    return False


def pops(lines):
    """[VALU instructions between the decrement and the read] of every ds_read_b32 of the body (the stack's pops are its only
    LDS reads); None where the read's block has no decrement in front of it"""
    ins = instructions(lines)
    out = []
    for i, (mn, ops) in enumerate(ins):
        if mn != "ds_read_b32":
            continue
        between, found = 0, None
        for mn2, ops2 in reversed(ins[:i]):
            if mn2 == "label":
                break
            if is_decrement(mn2, ops2):
                found = between
                break
            if mn2.startswith("v_"):
                between += 1
        out.append(found)
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_ballot_of_a_flag_or_a_conjunction_is_left(isa, kernel):
    pairs = ballot_pairs(body_of(isa, kernel))
    print(kernel, "v_cndmask 0/1 + v_cmp_ne pairs:", pairs)
    assert pairs == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_flag_lives_as_a_byte_in_a_vgpr(isa, kernel):
    body = body_of(isa, kernel)
    tests, sdwa = flag_tests(body), sum("v_cmp_ne_u16_sdwa" in l for l in body)
    print(kernel, "v_and 1 + v_cmp_eq 1 tests:", tests, "v_cmp_ne_u16_sdwa:", sdwa)
    assert tests == 0 and sdwa == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_pop_is_a_decrement_one_clamp_and_the_read(isa, kernel):
    found = pops(body_of(isa, kernel))
    print(kernel, "VALU instructions between a pop's decrement and its ds_read_b32:", found)
    assert len(found) >= 2, "the record loop pops in two places (the pop, and the entry under a sentinel)"
    assert all(n is not None and n <= 1 for n in found)


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_masks_cost_no_sgpr_spills(isa, kernel):
    body = body_of(isa, kernel)
    assert not any(re.match(r"\s*v_writelane_b32", l) for l in body)
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n.*?\.sgpr_spill_count:\s+(\d+)", isa, re.S)
    assert m and int(m.group(1)) == 0
