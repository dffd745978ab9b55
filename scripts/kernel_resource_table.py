"""One line per kernel from hipcc's -Rpass-analysis=kernel-resource-usage remarks, and the difference between two such logs.

    python scripts/kernel_resource_table.py NEW.log                 the table of NEW.log
    python scripts/kernel_resource_table.py PARENT.log NEW.log      kernels of PARENT.log whose figures changed in NEW.log, kernels only
                                                                    in one of them; exit status 1 when a kernel of PARENT.log changed

The logs come from, per translation unit,
    hipcc <the Makefile's flags> --cuda-device-only -c X.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2> X.log
No GPU is needed."""
import re
import subprocess
import sys

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds"))


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    table, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+%s: (\d+)" % re.escape(label), line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return table


def row(name, f):
    return "%-110s vgpr %3d sgpr %3d agpr %d scratch %d spills %d/%d lds %5d occupancy %d" % (
        name, f["vgpr"], f["sgpr"], f["agpr"], f["scratch"], f["sspill"], f["vspill"], f["lds"], f["occ"])


def main(argv):
    if len(argv) == 2:
        t = parse(argv[1])
        names = demangle(sorted(t))
        for k in sorted(t, key=lambda k: names[k]):
            print(row(names[k], t[k]))
        return 0
    old, new = parse(argv[1]), parse(argv[2])
    names = demangle(sorted(set(old) | set(new)))
    changed = 0
    for k in sorted(old, key=lambda k: names[k]):
        if k not in new:
            print("GONE     " + row(names[k], old[k]))
            changed += 1
        elif old[k] != new[k]:
            print("CHANGED  " + row(names[k], old[k]))
            print("     ->  " + row(names[k], new[k]))
            changed += 1
    print("%d kernels in the parent log, %d of them unchanged, %d changed or gone" % (len(old), len(old) - changed, changed))
    for k in sorted(new, key=lambda k: names[k]):
        if k not in old:
            print("NEW      " + row(names[k], new[k]))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
