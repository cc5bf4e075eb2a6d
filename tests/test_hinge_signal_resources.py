"""The two kernels of the hinge-force signal channels -- k_signal_hinge_channels (difflexmm_amd/csrc/dfx_objective.h; every bond model, with
and without the angle contact) and k_tan_hinge_channels (difflexmm_amd/csrc/dfx_tangent.h; the same builds at chunk widths 1, 2 and 4) --
report no scratch and no spilled registers in the compiler's resource usage for gfx950, in the manner of test_signal_xcorr_resources.py.
So do k_signal_cotangent and k_signal_explicit, which gained the hinge seeds.  Only ScratchSize and the spill counts are checked; the
register counts are printed.  Seen: k_signal_hinge_channels at most 58 VGPRs, k_signal_cotangent 90, k_signal_explicit 144,
k_tan_hinge_channels 256 VGPRs and 28 AGPRs in its widest nonlinear build with the angle contact; no scratch, nothing spilled."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
BUILDS = {(m, c) for m in range(4) for c in (0, 1)}


def resource_usage(source, pattern):
    """{template arguments: dict} of the kernels whose mangled name matches ``pattern`` (its groups: name, template arguments)"""
    csrc = os.path.join(ROOT, "difflexmm_amd", "csrc")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-disable-machine-licm", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(csrc, source)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    seen = {}
    for m in re.finditer(r"Function Name: " + pattern + r"\w*(.*?)LDS Size", p.stdout, re.S):
        get = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(3)).group(1))     # noqa: E731
        args = tuple(int(x) for x in re.findall(r"Li(\d)E", m.group(2)))
        seen[(m.group(1),) + args] = dict(scratch=get("ScratchSize"), vgprs=get(r" VGPRs"), agprs=get("AGPRs"), sgprs=get("TotalSGPRs"),
                                          vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"))
    for key in sorted(seen):
        v = seen[key]
        print(f"[hinge signal] {key[0]}<{', '.join(str(x) for x in key[1:])}>: scratch {v['scratch']} bytes/lane, {v['vgprs']} VGPRs, {v['agprs']} AGPRs, "
              f"{v['sgprs']} SGPRs, {v['vgpr_spill']} VGPRs and {v['sgpr_spill']} SGPRs spilled")
    return seen


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_reverse_mode_hinge_kernels_report_no_scratch_and_no_spills():
    seen = resource_usage("engine_objective.hip", r"_ZN\d+_GLOBAL__N_1\d+(k_signal_hinge_channels|k_signal_cotangent|k_signal_explicit)I((?:Li\d+E)+)E")
    for name in ("k_signal_hinge_channels", "k_signal_cotangent", "k_signal_explicit"):
        assert {k[1:] for k in seen if k[0] == name} == BUILDS, (name, sorted(seen))
    bad = {k: v for k, v in seen.items() if v["scratch"] != 0 or v["vgpr_spill"] != 0 or v["sgpr_spill"] != 0}
    assert not bad, bad


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_forward_mode_hinge_kernel_reports_no_scratch_and_no_spills():
    seen = resource_usage("engine_tangent.hip", r"_ZN3dfx\d+(k_tan_hinge_channels)I((?:Li\d+E)+)E")
    assert {k[1:] for k in seen} == {(m, c, w) for m, c in BUILDS for w in (1, 2, 4)}, sorted(seen)
    bad = {k: v for k, v in seen.items() if v["scratch"] != 0 or v["vgpr_spill"] != 0 or v["sgpr_spill"] != 0}
    assert not bad, bad
