"""resources of every k_frozen_persistent<E, KIND, TEAM, PIECES, LEAN> and k_frozen_persistent_w2<E, PIECES> instantiation of a built
nk2d_frozen.o -- and of every k_frozen_persistent_d<E, KIND, PIECES> of a built nk2d_frozen_d.o --, from the AMDGPU metadata of its gfx950 code object (llvm-objcopy --dump-section=.hip_fatbin, clang-offload-bundler
--unbundle, llvm-readelf --notes): VGPRs (vector + accumulation registers) / scratch bytes per lane / VGPRs spilled / static LDS
bytes / code bytes / scalar registers spilled into vector lanes.  With two objects: a table before | after | same, the way profiles/r10_frozen_phosphorus_kernel_resources.log was made.

    python tools/frozen_kernel_resources.py AFTER.o [BEFORE.o]        (no GPU needed)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")


def resources(obj):
    """{(entry, template arguments): (vgprs, scratch, spilled, lds, code bytes, sgprs spilled)}"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                        "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], check=True, capture_output=True, text=True).stdout
    size = {f[7]: int(f[2]) for f in (line.split() for line in syms.splitlines()) if len(f) == 8 and f[3] == "FUNC"}
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.match(r"_Z\d+(k_frozen_persistent(?:_w2|_d)?)I((?:Li\d+E)+)E", name)
        if not m:
            continue
        field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))     # noqa: E731
        args = tuple(int(v) for v in re.findall(r"Li(\d+)E", m.group(2)))
        out[(m.group(1), args)] = (field("vgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count"),
                                   field("group_segment_fixed_size"), size.get(name, -1), field("sgpr_spill_count"))
    return out


def fmt(r):
    return "%5d %5d %5d %6d %7d %5d" % r if r else "%5s %5s %5s %6s %7s %5s" % ("-", "-", "-", "-", "-", "-")


if __name__ == "__main__":
    after = resources(sys.argv[1])
    before = resources(sys.argv[2]) if len(sys.argv) > 2 else None
    for entry, width, head in (("k_frozen_persistent", 5, "#  E KIND TEAM PIECES LEAN"), ("k_frozen_persistent_w2", 2, "#  E PIECES (k_frozen_persistent_w2)"),
                              ("k_frozen_persistent_d", 3, "#  E KIND PIECES (k_frozen_persistent_d)")):
        if not any(k[0] == entry for k in after):
            continue
        print(head + (" | %38s | %38s | same" % ("before", "after") if before is not None else " | vgprs scratch spilled lds code sgpr-spills"))
        for key in sorted(k for k in after if k[0] == entry):
            args = "".join("%4d " % v for v in key[1])
            if before is None:
                print(args + "| " + fmt(after[key]))
            else:
                same = "yes" if before.get(key) == after[key] else ("NEW" if key not in before else "NO")
                print(args + "| " + fmt(before.get(key)) + " | " + fmt(after[key]) + " | " + same)
    if before is not None:
        gone = sorted(k for k in before if k not in after)
        changed = [k for k in before if k in after and before[k] != after[k]]
        print("# %d instantiations before, %d after; %d changed, %d gone, %d new" % (len(before), len(after), len(changed), len(gone),
                                                                                  len([k for k in after if k not in before])))
