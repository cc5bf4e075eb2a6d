"""The member-ranked issue priority of the persistent stage loops, pinned without a GPU.

The rule (difflexmm_amd/csrc/dfx_persist_prio.h, persist_prio) is one pure function: a g++ program around the header prints it over
mode {0, 1} x workgroups per compute unit {1, 2, 3, 8} x member 0 .. 23 x both placements (waves packed densely; one member per XCD).
A wave calls it with its member's number only, so every wave of a member has the same value by construction; the table shows that the
value is a function of (mode, member, per_cu, placement) alone by evaluating it twice.  The members that can share a SIMD are
consecutive ones in the dense packing and, with one member per XCD, members eight apart (member 8 * mi + x sits on XCD x:
persist_wave, dfx_persist.h) -- those must differ wherever two workgroups share a compute unit.

Where the waves set it (dfx_persist.h) is read off the ISA of dfx_persist.hip, compiled as the Makefile compiles it, in the stage loop
of k_adj_persist<1,1,4> and k_fwd_persist<1,1,4>: a wave is back at priority 0 in front of the ring's polling load (a spinning wave
never outranks a computing one) and raises itself behind it; and the angle contact is evaluated only beyond the culling bound --
between the compare against kap_safe and the end of that block no angle is wrapped (v_rndne_f64) outside a block a wave without
such a lane skips."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

from .test_persist_loop_budget import _body, _instructions, _stage_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difflexmm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("_ZN12_GLOBAL__N_113k_adj_persistILi1ELi1ELi4E", "_ZN12_GLOBAL__N_113k_fwd_persistILi1ELi1ELi4E")

HARNESS = r"""
#include <cstdio>
#include "dfx_persist_prio.h"
int main() {
  const int per_cu[] = {1, 2, 3, 8};
  for (int mode = 0; mode < 2; ++mode)
    for (int p : per_cu)
      for (int xcd_wg = 0; xcd_wg < 2; ++xcd_wg)
        for (int ml = 0; ml < 32; ++ml)
          printf("%d %d %d %d %d %d\n", mode, p, xcd_wg, ml, dfx_persist::persist_prio(mode, ml, p, xcd_wg * 5),
                 dfx_persist::persist_prio(mode, ml, p, xcd_wg * 5));
  static_assert(dfx_persist::persist_prio(1, 1, 3, 0) == 2, "usable in constant expressions");
  return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("persist_prio")
    src, exe = d / "prio.cpp", d / "prio"
    src.write_text(HARNESS)
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert len(rows) == 2 * 4 * 2 * 32
    assert all(r[4] == r[5] for r in rows)          # every wave of a member: the same call, the same value
    return {r[:4]: r[4] for r in rows}


def test_rule_is_off_without_co_resident_workgroups_or_when_switched_off(table):
    for (mode, per_cu, xcd, ml), v in table.items():
        assert 0 <= v <= 3, (mode, per_cu, xcd, ml, v)
        if mode == 0 or per_cu == 1:
            assert v == 0, (mode, per_cu, xcd, ml, v)


@pytest.mark.parametrize("per_cu", [2, 3, 8])
def test_members_that_can_share_a_simd_differ(table, per_cu):
    n = min(per_cu, 4)
    for ml in range(24):
        assert table[(1, per_cu, 0, ml)] != table[(1, per_cu, 0, ml + 1)], ("dense", per_cu, ml)
        assert table[(1, per_cu, 0, ml)] == 3 - ml % n
        # one member per XCD: the eight members of a round sit on eight XCDs; the next round's member on the same XCD differs
        assert table[(1, per_cu, 1, ml)] != table[(1, per_cu, 1, ml + 8)], ("xcd", per_cu, ml)
        assert table[(1, per_cu, 1, ml)] == 3 - (ml >> 3) % n
    # any `n` members in a row of the dense packing (the most a SIMD holds, up to four) are pairwise different
    for ml in range(24):
        assert len({table[(1, per_cu, 0, ml + i)] for i in range(n)}) == n
    # the first member of a launch is the one that runs at its solo pace
    assert table[(1, per_cu, 0, 0)] == 3 and table[(1, per_cu, 1, 5)] == 3


@pytest.fixture(scope="module")
def persist_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cxxflags = shlex.split(re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1))
    kflags = shlex.split(re.search(r"^KFLAGS = (.*)$", mk, re.M).group(1))
    out = tmp_path_factory.mktemp("persist_prio_isa") / "persist.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950"] + cxxflags + kflags + ["-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "dfx_persist.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


def _stage(txt, name):
    lines = _body(txt, name)
    (a, b), _ = _stage_loop(lines)
    return lines[a:b + 1]


@pytest.mark.parametrize("name", KERNELS)
def test_a_wave_polls_at_priority_zero_and_computes_at_its_rank(persist_isa, name):
    loop = _stage(persist_isa, name)
    polls = [n for n, x in enumerate(loop) if re.match(r"global_load_dwordx4 .* sc1", x)]
    assert polls, name
    before = [x for x in loop[:polls[0]] if x.startswith("s_setprio")]
    assert before and before[-1].split() == ["s_setprio", "0"], (name, before)
    after = [x for x in loop[polls[-1]:] if x.startswith("s_setprio")]
    assert any(x.split()[1] != "0" for x in after), (name, after)
    # every raise stands alone behind a scalar compare and branch: s_setprio ignores EXEC, a lane-masked one would raise every wave
    for n, x in enumerate(loop):
        if x.startswith("s_setprio") and x.split()[1] != "0":
            prev = _instructions(loop[:n])[-2:]
            assert prev[0].startswith("s_cmp") and prev[1].startswith("s_cbranch_scc"), (name, x, prev)


@pytest.mark.parametrize("name", KERNELS)
def test_angle_contact_is_evaluated_only_beyond_the_culling_bound(persist_isa, name):
    """The culling compare is  !(|theta_o - theta_p| <= kap_safe)  -- the loop's one not-less-or-equal fp64 compare of an absolute value
    against a scalar register.  From there to the end of the block it stands in (the next s_or_b64 exec that closes a block opened earlier)
    every angle wrap (v_rndne_f64: twrap of the two void angles) lies inside a block opened behind the compare that a wave with no lane
    beyond the bound skips (s_and_saveexec + s_cbranch_execz): lanes inside the bound no longer evaluate a stand-in angle."""
    loop = _instructions(_stage(persist_isa, name))
    cmps = [n for n, x in enumerate(loop) if re.match(r"v_cmp_nle_f64\S* \S+ \|v\[\d+:\d+\]\|, s\[\d+:\d+\]$", x)]
    assert len(cmps) == 1, (name, [loop[n] for n in cmps])
    open_blocks, wraps = [], 0
    for n in range(cmps[0] + 1, len(loop)):
        x = loop[n]
        m = re.match(r"s_andn?2?_saveexec_b64 (s\[\d+:\d+\])", x)
        if m and loop[n + 1].startswith("s_cbranch_execz"):
            open_blocks.append(m.group(1))
        elif x.startswith("s_or_b64 exec, exec, "):
            if not open_blocks:
                break                     # the end of the block the compare stands in
            assert x.endswith(open_blocks.pop()), (name, n, x)
        elif x.startswith("v_rndne_f64"):
            assert open_blocks, (name, n, "an angle is wrapped on lanes inside the culling bound")
            wraps += 1
    else:
        raise AssertionError((name, "the block of the culling compare does not end inside the stage loop"))
    assert wraps == 2, (name, wraps)
