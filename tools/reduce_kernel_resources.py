"""Reduce the remarks of `hipcc ... -Rpass-analysis=kernel-resource-usage` (on stderr) to one line per mangled function name:
registers, scratch, occupancy, spills, LDS.  Sorted, so that two builds of a translation unit compare with `diff`.

    python tools/reduce_kernel_resources.py build.log > reduced.txt"""
import re
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def reduce(text):
    out, name, vals = [], None, {}
    for line in text.splitlines():
        m = re.search(r"remark:\s+([A-Za-z][^:]*):\s+(\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            if name is not None:
                out.append(name + " " + " ".join(f"{k.split(' [')[0].replace(' ', '')}={vals[k]}" for k in FIELDS))
            name, vals = val, {}
        else:
            vals[key] = val
    if name is not None:
        out.append(name + " " + " ".join(f"{k.split(' [')[0].replace(' ', '')}={vals[k]}" for k in FIELDS))
    return sorted(out)


if __name__ == "__main__":
    print("\n".join(reduce(open(sys.argv[1]).read())))
