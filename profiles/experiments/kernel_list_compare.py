"""Kernel names and launch counts of two rocprofv3 --kernel-trace --stats runs (their -d directories): equal or not.
torch's own fill / copy kernels are in the lists too: the whole process is traced.

    python profiles/experiments/kernel_list_compare.py PARENT_DIR THIS_DIR
"""
import csv, glob, sys


def load(d):
    f = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
    assert len(f) == 1, f
    return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(f[0]))}


a, b = load(sys.argv[1]), load(sys.argv[2])
print(f"parent: {len(a)} kernel names, {sum(a.values())} launches; this tree: {len(b)} names, {sum(b.values())} launches")
diff = {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)}
print("identical kernel list and launch counts" if not diff else f"DIFFERENCES: {diff}")
