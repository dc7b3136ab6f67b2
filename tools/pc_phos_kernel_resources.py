"""resources of every k_pc_phos_rhs<E>, k_pc_phos_combine<E> and k_pc_phos_finish<E> instantiation (E = levels per lane, 1 .. 8) of a
built nk2d_precond.o, from the AMDGPU metadata of its gfx950 code object, by the recipe of tools/frozen_kernel_resources.py
(llvm-objcopy --dump-section=.hip_fatbin, clang-offload-bundler --unbundle, llvm-readelf --notes): VGPRs (vector + accumulation
registers) / SGPRs / scratch bytes per lane / VGPRs spilled / static LDS bytes.

    python tools/pc_phos_kernel_resources.py newton-krylov_ooc_amd/csrc/nk2d_precond.o        (no GPU needed)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")
KERNELS = ("k_pc_phos_rhs", "k_pc_phos_combine", "k_pc_phos_finish")


def resources(obj):
    """{(kernel, E): (vgprs, sgprs, scratch, spilled, lds)}"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                        "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"(%s)ILi(\d+)EE" % "|".join(KERNELS), name)
        if not m:
            continue
        field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))     # noqa: E731
        out[(m.group(1), int(m.group(2)))] = (field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size"),
                                              field("vgpr_spill_count"), field("group_segment_fixed_size"))
    return out


if __name__ == "__main__":
    res = resources(sys.argv[1])
    print("# kernel               E | vgprs sgprs scratch spilled    lds")
    for key in sorted(res):
        print("%-20s %3d | %5d %5d %7d %7d %6d" % (key + res[key]))
    missing = [(k, e) for k in KERNELS for e in range(1, 9) if (k, e) not in res]
    print("# %d instantiations; missing: %s" % (len(res), missing or "none"))
