"""The shipped instances of k_tan_signal_channels (difflexmm_amd/csrc/dfx_tangent.h; chunk widths 1, 2 and 4, every bond model, with and
without the angle contact) report no scratch in the compiler's resource usage for gfx950, in the manner of
test_kernel_isa.py::test_tile_kernels_have_no_scratch_and_no_barrier and test_tangent_multi_host.py's check of the stage kernel: a
dual-number ligament evaluation that spills would pay for every epsilon part in memory traffic.  Seen: the widest nonlinear build with the
angle contact takes 256 vector registers and 12 accumulation registers, no scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_signal_channel_kernels_report_no_scratch():
    csrc = os.path.join(ROOT, "difflexmm_amd", "csrc")
    src = open(os.path.join(csrc, "engine_tangent.hip")).read()
    widths = sorted(int(w) for w in re.search(r"constexpr int kWidths\[\] = \{([^}]*)\}", src).group(1).split(","))
    assert widths == [1, 2, 4]
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-disable-machine-licm", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, os.path.join(csrc, "engine_tangent.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    seen = {}
    for m in re.finditer(r"Function Name: _ZN3dfx21k_tan_signal_channelsILi(\d)ELi(\d)ELi(\d)EEE\w*(.*?)LDS Size", p.stdout, re.S):
        model, contact, kc = (int(x) for x in m.groups()[:3])
        get = lambda key: int(re.search(key + r"[^:\n]*: (\d+)", m.group(4)).group(1))     # noqa: E731
        seen[(model, contact, kc)] = (get("ScratchSize"), get(r" VGPRs"), get("AGPRs"), get("VGPRs Spill"))
    for key in sorted(seen):
        print(f"[signal tangent] k_tan_signal_channels<model {key[0]}, contact {key[1]}, KC {key[2]}>: scratch {seen[key][0]} bytes/lane, "
              f"{seen[key][1]} VGPRs, {seen[key][2]} AGPRs, {seen[key][3]} spilled")
    assert set(seen) == {(m, c, w) for m in range(4) for c in (0, 1) for w in widths}, sorted(seen)
    bad = {k: v for k, v in seen.items() if v[0] != 0 or v[3] != 0}
    assert not bad, bad
