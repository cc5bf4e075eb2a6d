"""The four kernels of the signal spectral ratios (difflexmm_amd/csrc/dfx_objective.h: k_signal_spectrum_forms, k_signal_spectrum_reduce,
k_signal_spectrum_weights, k_signal_spectrum_residual) report no scratch and no spilled registers in the compiler's resource usage for
gfx950, in the manner of test_signal_xcorr_resources.py.  Only ScratchSize and the spill counts are checked; the register counts are
printed (recorded in profiles/spectrum_worst_cases.txt)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("k_signal_spectrum_forms", "k_signal_spectrum_reduce", "k_signal_spectrum_weights", "k_signal_spectrum_residual")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_spectrum_kernels_report_no_scratch_and_no_spills():
    csrc = os.path.join(ROOT, "difflexmm_amd", "csrc")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-disable-machine-licm", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(csrc, "engine_objective.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    seen = {}
    for m in re.finditer(r"Function Name: _ZN\d+_GLOBAL__N_1\d+(k_signal_spectrum\w*?)E\w*(.*?)LDS Size", p.stdout, re.S):
        get = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(2)).group(1))     # noqa: E731
        seen[m.group(1)] = dict(scratch=get("ScratchSize"), vgprs=get(r" VGPRs"), agprs=get("AGPRs"), sgprs=get("TotalSGPRs"),
                                vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"))
    for name in sorted(seen):
        v = seen[name]
        print(f"[signal spectrum] {name}: scratch {v['scratch']} bytes/lane, {v['vgprs']} VGPRs, {v['agprs']} AGPRs, {v['sgprs']} SGPRs, "
              f"{v['vgpr_spill']} VGPRs and {v['sgpr_spill']} SGPRs spilled")
    assert set(seen) == set(KERNELS), sorted(seen)
    bad = {k: v for k, v in seen.items() if v["scratch"] != 0 or v["vgpr_spill"] != 0 or v["sgpr_spill"] != 0}
    assert not bad, bad
