"""Compares two rocprofv3 kernel traces of scratch/asm_plan_launches.py or scratch/smooth_plan_bits.py (dev tool): per build, the
ordered list of (kernel, grid, workgroup, LDS bytes) -- for the batched call, whose builds run on several host threads, the sorted list.
usage: compare_launches.py parent_kernel_trace.csv new_kernel_trace.csv labels.txt [what was traced] > profiles/asm_plan_launches.txt"""
import csv
import sys


def segments(path):
    rows = list(csv.DictReader(open(path, newline="")))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lds = [k for k in rows[0] if k.lower().startswith("lds")][0]
    segs, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        key = (name, tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"), int(r[lds]))
        if "cos_kernel" in name:      # the separator
            cur = []
            segs.append(cur)
        elif cur is not None:
            cur.append(key)
    return segs


a, b = segments(sys.argv[1]), segments(sys.argv[2])
labels = [l.rstrip("\n") for l in open(sys.argv[3])]
what = sys.argv[4] if len(sys.argv) > 4 else "the sorted-grid builds, parent commit against the plan walkers: scratch/asm_plan_launches.py"
print("# Kernel launches of %s under" % what)
print("# rocprofv3 --kernel-trace, one run per library build on one MI355X.  Per build: the ordered list of (kernel name, grid,")
print("# workgroup size, LDS bytes); the batched call's builds run on several host threads: compared as a sorted list.")
print("# segments: parent %d, new %d, labels %d" % (len(a), len(b), len(labels)))
ndiff = 0
kinds = set()
print("%-110s | launches | verdict" % "build")
for i, lab in enumerate(labels):
    if lab == "end":
        break
    sa, sb = a[i], b[i]
    asm = lambda s: [k for k in s if "ibh" in k[0]]
    sa, sb = asm(sa), asm(sb)
    if "unordered" in lab:
        sa, sb = sorted(sa), sorted(sb)
    same = sa == sb
    ndiff += 0 if same else 1
    kinds.update(sb)
    print("%-110s | %8d | %s" % (lab, len(sb), "identical" if same else "DIFFERENT"))
    if not same:
        for x, y in zip(sa, sb):
            if x != y:
                print("    parent %s\n    new    %s" % (x, y))
                break
        if len(sa) != len(sb):
            print("    parent %d launches, new %d" % (len(sa), len(sb)))
print("# %d builds, %d differ; %d distinct (kernel, grid, workgroup, LDS) launches seen" % (len(labels) - 1, ndiff, len(kinds)))
