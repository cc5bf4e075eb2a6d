"""Is the device code of two source trees the same?  For host-side refactors: every .hip file of difflexmm_amd/csrc of both trees is compiled
for the device alone (hipcc -S --cuda-device-only, the Makefile's flags: KFLAGS, ADJFLAGS for stage_builds_adj.hip) and compared.

    python tools/compare_device_asm.py <parent tree> <branch tree> [work dir]

Per file: "identical" (after dropping the lines of the __hip_cuid_ symbol, which hashes the file's path), or -- where the order of the
functions moved -- whether the set of kernels is the same and how many kernel bodies and kernel descriptors differ (labels and comments carry
the ordinal of the function in the file: normalised).  profiles/r17_dispatch_refactor.txt is its output."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = "/opt/rocm/bin/hipcc"
CXX = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
KFLAGS = ["-mllvm", "-disable-machine-licm"]
ADJFLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp", "-DDFX_ADJ_OCC=__attribute__((amdgpu_waves_per_eu(4)))"]


def flags(name):
    return CXX + ([] if name == "dfx_comm" else KFLAGS) + (ADJFLAGS if name == "stage_builds_adj" else [])


def compile_tree(tree, out):
    csrc = os.path.join(tree, "difflexmm_amd", "csrc")
    names = sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".hip"))
    os.makedirs(out, exist_ok=True)

    def one(n):
        subprocess.check_call([HIPCC] + flags(n) + ["-S", "--cuda-device-only", "-o", os.path.join(out, n + ".s"), n + ".hip"], cwd=csrc,
                              stderr=subprocess.DEVNULL)
    with ThreadPoolExecutor(4) as ex:
        list(ex.map(one, names))
    return names


def load(path):
    return [line for line in open(path) if "__hip_cuid_" not in line]


def norm(lines):
    out = []
    for line in lines:
        line = re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+", r".\1N", line)
        out.append(re.sub(r"\s+", " ", re.sub(r"\bBB\d+_", "BBN_", line)))
    return out


def pieces(lines):
    """function bodies (label .. .Lfunc_end) and kernel descriptors (.amdhsa_kernel .. .end_amdhsa_kernel) by name"""
    bodies, desc, cur, kd = {}, {}, None, None
    for line in lines:
        m = re.match(r"^(\w+):\s", line)
        if cur is None and kd is None and m and not m.group(1).startswith("."):
            cur = m.group(1)
            bodies[cur] = []
        if cur is not None:
            bodies[cur].append(line)
            if line.startswith(".Lfunc_end"):
                cur = None
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kd = m.group(1)
            desc[kd] = []
        if kd is not None:
            desc[kd].append(line)
            if ".end_amdhsa_kernel" in line:
                kd = None
    return bodies, desc


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else "device_asm_work"
    names = compile_tree(parent, os.path.join(work, "parent"))
    assert names == compile_tree(branch, os.path.join(work, "branch")), "the trees do not hold the same .hip files"
    bad = 0
    for n in names:
        a, b = load(os.path.join(work, "parent", n + ".s")), load(os.path.join(work, "branch", n + ".s"))
        if a == b:
            print(f"{n}.hip: identical ({len(a)} lines)")
            continue
        (ba, da), (bb, db) = pieces(a), pieces(b)
        same_set = set(ba) == set(bb) and set(da) == set(db)
        n_body = sum(norm(ba[k]) != norm(bb[k]) for k in ba if k in bb)
        n_desc = sum(norm(da[k]) != norm(db[k]) for k in da if k in db)
        bad += (not same_set) + n_body + n_desc
        print(f"{n}.hip: order of functions differs; {len(da)} kernels ({len(ba)} functions), same set of names: {same_set}; "
              f"bodies that differ: {n_body}; kernel descriptors that differ: {n_desc}")
    print("DEVICE CODE UNCHANGED" if not bad else "DEVICE CODE DIFFERS")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
