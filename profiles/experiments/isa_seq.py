"""One kernel of a `hipcc -S` listing reduced to its ds_read / s_waitcnt / v_mfma / branch / scratch sequence, block labels kept
(the view behind profiles/r09_a_wgrad_parent.txt).  usage: isa_seq.py <file.s> <mangled kernel name>"""
import re
import sys

src = open(sys.argv[1]).read().split("\n")
key = sys.argv[2]
start = next(i for i, l in enumerate(src) if l.startswith(key + ":"))
keep = ("ds_read", "ds_load", "s_waitcnt", "v_mfma", "s_cbranch", "s_branch", "s_barrier", "s_nop", "scratch_")
for l in src[start + 1:]:
    t = l.strip()
    if t.startswith(".Lfunc_end"):
        break
    if re.match(r"^\.LBB\d+_\d+:", t):
        print(t.split(";")[0].strip())
    elif t and t[0] not in ";." and t.split()[0].startswith(keep):
        print("   " + t.split(";")[0].strip())
