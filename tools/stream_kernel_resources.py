"""resources of every k_stream<E, KIND, TAPE, XL> and k_stream_w2<E, KIND, TAPE, XL> instantiation of built objects of the command-stream
kernel (nk2d_stream.o, nk2d_stream_xl.o), from the AMDGPU metadata of their gfx950 code objects (llvm-objcopy
--dump-section=.hip_fatbin, clang-offload-bundler --unbundle, llvm-readelf --notes): VGPRs (vector + accumulation registers) / SGPRs /
scratch bytes per lane / VGPRs spilled / static LDS bytes.  A kernel of a build from before the template parameter XL counts as XL = 0.
The table has one row per (entry, E, KIND, TAPE): the parent's kernel, this build's XL = 0 kernel, whether the two are equal, this
build's XL flavour, and whether that one needs more scratch than its XL = 0 sibling.

    python tools/stream_kernel_resources.py --before PARENT_nk2d_stream.o -- nk2d_stream.o nk2d_stream_xl.o        (no GPU needed)"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")


def resources(objs):
    """{(entry, E, KIND, TAPE, XL): (vgprs, sgprs, scratch, spilled, lds)}"""
    out = {}
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
            subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")], check=True)
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co,
                            "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH], check=True)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            block = ".agpr_count:" + block
            name = re.search(r"\.name:\s+(\S+)", block).group(1)
            m = re.match(r"_Z\d+(k_stream(?:_w2)?)ILi(\d+)ELi(\d+)ELb([01])E(?:Li(\d+)E)?Ev", name)
            if not m:
                continue
            field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))     # noqa: E731
            key = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5) or 0))
            out[key] = (field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count"),
                        field("group_segment_fixed_size"))
    return out


def fmt(r):
    return "%4d %4d %5d %5d %5d" % r if r else "%4s %4s %5s %5s %5s" % ("-", "-", "-", "-", "-")


if __name__ == "__main__":
    args = sys.argv[1:]
    before = None
    if args and args[0] == "--before":
        cut = args.index("--")
        before, args = resources(args[1:cut]), args[cut + 1:]
    after = resources(args)
    xls = sorted({k[4] for k in after if k[4] != 0})
    print("# vgprs sgprs scratch spilled lds")
    print("# entry        E KIND TAPE | %26s | %26s | same | %26s | more scratch" % ("parent", "this build, XL = 0", "this build, XL = %s" % (xls or "-")))
    changed = more = 0
    for key in sorted(k for k in after if k[4] == 0):
        b = before.get(key) if before is not None else None
        x = next((after[key[:4] + (v,)] for v in xls if key[:4] + (v,) in after), None)
        same = "-" if before is None else ("yes" if b == after[key] else "NO")
        worse = "-" if x is None else ("MORE" if x[2] > after[key][2] else "no")
        changed += same == "NO"
        more += worse == "MORE"
        print("%-11s %3d %4d %4d | %s | %s | %4s | %s | %s" % (key[:4] + (fmt(b), fmt(after[key]), same, fmt(x), worse)))
    print("# %d kernels with XL = 0 (%s of the parent's changed), %d with the XL flavour, %d of those with more scratch than their sibling"
          % (len([k for k in after if k[4] == 0]), changed if before is not None else "-", len([k for k in after if k[4] != 0]), more))
