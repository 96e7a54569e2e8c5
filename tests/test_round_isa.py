"""The compiled form of a tracing round (CPU: hipcc cross-compiles to ISA without a GPU; compile and flags of
tests/test_register_budgets.py).  wf2_trace is bound by VALU issue, and two kinds of per-round vector work served no ray:

 - the world ray's slab constants (three v_rcp_f32, three v_med3_f32, three v_mul_f32), which the compiler hoisted out of pop_next's
   rarely taken restore into the pre-header of the record loop, where the whole wave paid them in every round.  They now stay inside
   the loop, in the block that needs them (pop_next<true>, jpt_trace_core.h);
 - ballots of flags and conjunctions, which compile to v_cndmask_b32 0/1 + v_cmp_ne_u32 each: 8 pairs per round before the wave's
   bookkeeping moved to scalar lane masks (walk_round_masked, trace_queue: jpt_kernels_wf2.hip), 2 since -- the record loop's `want`,
   once in its peeled first turn and once in the loop.

Registers and scratch stay at or below what the kernels used before that change (read from the ISA of the commit before it)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gdpathtracing_amd", "csrc", "jpt_kernels_wf2.hip")

# kernel (mangled-name fragment) -> (most ballot pairs, most VGPRs, most bytes of scratch per lane, most scratch instructions).
# Pairs: 8 and 10 before the change; registers and scratch: the figures before the change.
KERNELS = {
    "9wf2_traceILb0ELb1ELb0E": (2, 71, 320, 11),
    "9wf2_traceILb0ELb1ELb1E": (2, 72, 944, 72),
}


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


def blocks_of(lines):
    """[(label, annotation, [mnemonics])]: basic blocks with the loop comments the compiler writes beside and below their labels"""
    blocks = []
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):(.*)$", l)
        if m:
            blocks.append([m.group(1).lstrip(".L").replace("; %bb.", "bb."), m.group(2), []])
        elif blocks and not blocks[-1][2] and re.match(r"^\s+;", l):
            blocks[-1][1] += " " + l.strip()
        elif blocks and re.match(r"^\s+[a-z]\w+", l):
            blocks[-1][2].append(l.split()[0])
    return blocks


def depth2_loops(lines):
    """{header label: [mnemonics of all its blocks]} of the loops at depth 2 (blocks of loops nested deeper included)"""
    loops = {}
    for label, note, ins in blocks_of(lines):
        heads = re.findall(r"(?:Header=|Parent Loop )(BB\d+_\d+) Depth=2", note)
        if re.search(r"Loop Header: Depth=2", note):
            heads.append(label)
        for h in set(heads):
            loops.setdefault(h, []).extend(ins)
    return loops


def ballot_pairs(lines):
    """v_cndmask_b32 vN, 0, 1, mask followed within a few lines by v_cmp_ne_u32 .., 0, vN: a ballot of something that is not one comparison"""
    n = 0
    for i, l in enumerate(lines):
        m = re.match(r"\s*v_cndmask_b32(?:_e64)?\s+(v\d+), 0, 1,", l)
        if m and any(re.match(r"\s*v_cmp_ne_u32(?:_e32|_e64)?\s+.*\b0, %s\b" % m.group(1), l2) for l2 in lines[i + 1:i + 6]):
            n += 1
    return n


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_the_world_rays_constants_are_restored_inside_the_record_loop(isa, kernel):
    loops = {h: ins for h, ins in depth2_loops(body_of(isa, kernel)).items() if any(i.startswith("v_cvt_f32_ubyte0") for i in ins)}
    assert loops, "no depth-2 loop with a record step (v_cvt_f32_ubyte0) in " + kernel
    for h, ins in loops.items():
        rcp = sum(i.startswith("v_rcp_f32") for i in ins)
        print(kernel, "record loop", h, "v_rcp_f32 inside:", rcp)
        assert rcp >= 3, "%s: the restore's three v_rcp_f32 are not in the record loop %s (hoisted into its pre-header?)" % (kernel, h)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_a_round_ballots_no_conjunctions(isa, kernel):
    pairs = ballot_pairs(body_of(isa, kernel))
    print(kernel, "v_cndmask 0/1 + v_cmp_ne pairs:", pairs)
    assert pairs <= KERNELS[kernel][0]


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_registers_and_scratch_did_not_grow(isa, kernel):
    _, vgprs, scratch, scratch_ops = KERNELS[kernel]
    m = re.search(r"\.name:\s+_ZN3jpt12_GLOBAL__N_1" + kernel + r"\S*\n\s+\.private_segment_fixed_size: (\d+).*?\.vgpr_count:\s+(\d+)", isa, re.S)
    assert m, "kernel not found in the ISA: " + kernel
    got = (int(m.group(2)), int(m.group(1)), len(re.findall(r"\bscratch_(?:load|store)", "\n".join(body_of(isa, kernel)))))
    print(kernel, "vgprs %d scratch %d B scratch instructions %d" % got)
    assert got[0] <= vgprs and got[1] <= scratch and got[2] <= scratch_ops
