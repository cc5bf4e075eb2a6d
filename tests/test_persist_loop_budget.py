"""Build-time budget of the persistent stage loops (no GPU needed: hipcc cross-compiles gfx950).  One wave's stream is priced per
ISSUED instruction, bookkeeping included, and three (four) waves share a SIMD's issue slots: what the loop issues besides its fp64
arithmetic is what the reverse sweep of a wide ensemble pays for (profiles/r14_persist_lean.txt).  The loops take a lean context
(PersistCtx), step their addresses and fetch their coefficients as one row per stage (dfx_persist_api.h) so that nothing is spilled
to vector lanes and re-read, and nothing but that row is loaded from the argument segment, inside a stage.  This test reads the ISA
of dfx_persist.hip, compiled as the Makefile compiles it, and holds the stage loop of k_adj_persist<1,1,4> and k_fwd_persist<1,1,4>
to that -- and to the instruction totals the lean loops were measured with.

                                 k_adj_persist<1,1,4>          k_fwd_persist<1,1,4>
    one pass of the stage loop   before    lean                before    lean
    all instructions             1 054     853                 956       861
    fp64 arithmetic                373     371                 371       371
    SALU (branches apart)          274     153                 249       191
    branches                        52      36                  39        35
    v_readlane / v_writelane     48 / 0    0 / 0               9 / 0     0 / 0
    s_load (groups, as below)    10 (2)    3 (1)               7 (2)     3 (1)
    rest of the step loop           91     100                 379        39
"""
import json
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FINGERPRINTS = os.path.join(ROOT, "tests", "golden", "schedule_fingerprints.json")

# (kernel, ceiling on all instructions of one pass of the stage loop, ceiling on the rest of the enclosing step loop): what this build has
CEILINGS = {
    "_ZN12_GLOBAL__N_113k_adj_persistILi1ELi1ELi4E": (853, 100),
    "_ZN12_GLOBAL__N_113k_fwd_persistILi1ELi1ELi4E": (861, 39),
}
# v_readlane_b32 inside a stage loop that does NOT reload a spilled scalar register, by what it reads (none today: a wave-uniform value
# a lane holds would be read with v_readfirstlane_b32, which is not counted)
NOT_A_SPILL = {}


def _body(txt, prefix):
    """Instructions and block labels of the kernel whose mangled name starts with `prefix`, in layout order."""
    m = re.search(r"\n(" + re.escape(prefix) + r"\S*):", txt)
    assert m, prefix
    out = []
    for line in txt[m.end():txt.index(".Lfunc_end", m.end())].split("\n"):
        line = line.strip()
        if not line or line.startswith(";"):
            continue
        if re.match(r"\.LBB\d+_\d+:", line):
            out.append(line.split(":")[0] + ":")
        elif not line.startswith((".", "_")):
            out.append(re.sub(r"\s*;.*$", "", line))
    return out


def _loops(lines):
    """(first, last) line of every backward branch's span."""
    labels = {line[:-1]: n for n, line in enumerate(lines) if line.endswith(":")}
    spans = []
    for n, line in enumerate(lines):
        m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", line)
        if m and labels.get(m.group(1), len(lines)) < n:
            spans.append((labels[m.group(1)], n))
    return spans


def _stage_loop(lines):
    """The innermost backward branch that encloses the ring accesses of a stage (the poll's sc1 loads AND the publishing sc1 store: the
    poll's own spin loop holds the loads only), and the innermost one around it: the step loop."""
    spans = _loops(lines)
    ring = [(a, b) for a, b in spans
            if any(re.match(r"global_load_dwordx4 .* sc1", x) for x in lines[a:b + 1]) and any(re.match(r"global_store_dwordx4 .* sc1", x) for x in lines[a:b + 1])]
    assert ring
    stage = min(ring, key=lambda t: t[1] - t[0])
    outer = [t for t in spans if t[0] <= stage[0] and t[1] >= stage[1] and t != stage]
    assert outer
    return stage, min(outer, key=lambda t: t[1] - t[0])


def _instructions(seg):
    return [x for x in seg if not x.endswith(":")]


def _toolchain():
    return subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()[1].strip()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_stage_loops_issue_no_spill_traffic_and_one_coefficient_fetch(tmp_path):
    want = json.load(open(FINGERPRINTS))["toolchain"]
    if want != _toolchain():
        pytest.skip(f"the loop budgets were taken with {want!r}, this is {_toolchain()!r}")
    mk = open(os.path.join(ROOT, "difflexmm_amd", "csrc", "Makefile")).read()
    cxxflags = shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))
    kflags = shlex.split(re.search(r"^KFLAGS = (.*)$", mk, re.M).group(1))
    assert "-disable-machine-licm" in kflags, kflags
    out = tmp_path / "persist.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950"] + cxxflags + kflags + ["-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(ROOT, "difflexmm_amd", "csrc", "dfx_persist.hip")], stderr=subprocess.DEVNULL)
    txt = out.read_text()
    for name, (ceiling, ceiling_step) in CEILINGS.items():
        lines = _body(txt, name)
        (a, b), (oa, ob) = _stage_loop(lines)
        loop = _instructions(lines[a:b + 1])
        step_rest = _instructions(lines[oa:a] + lines[b + 1:ob + 1])
        f64 = sum(x.split()[0].startswith("v_") and "f64" in x.split()[0] for x in loop)
        print(f"{name}: stage loop {len(loop)} instructions ({f64} fp64 arithmetic), rest of the step loop {len(step_rest)}")
        assert not [x for x in loop if x.startswith("v_writelane_b32")], name
        spills = [x for x in loop if x.startswith("v_readlane_b32") and x not in NOT_A_SPILL]
        assert not spills, (name, spills)
        # one group of scalar loads per stage: the coefficient row, nothing between its loads but other instructions that do not wait for them
        groups, open_group = 0, False
        for x in loop:
            if x.startswith(("s_load_", "s_buffer_load_")):
                groups += not open_group
                open_group = True
            elif x.startswith("s_waitcnt") and "lgkmcnt" in x:
                open_group = False
        assert groups <= 1, (name, groups, [x for x in loop if x.startswith("s_load_")])
        assert not [x for x in loop if x.startswith("scratch_")], name
        assert len(loop) <= ceiling, (name, len(loop), ceiling)
        assert len(step_rest) <= ceiling_step, (name, len(step_rest), ceiling_step)
        assert f64 >= 300, (name, f64)            # (the loop found really is the stage: it holds the ligament arithmetic)
