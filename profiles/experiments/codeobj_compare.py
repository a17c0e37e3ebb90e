"""Kernel by kernel, two `hipcc -S` listings of one source file (old, new): registers, LDS, scratch, waves per SIMD and the
global / LDS access instructions by width.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S old/bn.hip -o old.s     (same for new)
    python profiles/experiments/codeobj_compare.py old.s new.s [old_name=new_name ...]

Kernels are paired by demangled name; renamed ones through the old=new arguments (names without "void " and parameters)."""
import collections
import re
import subprocess
import sys


def demangle(n):          # __bf16 (DF16b) is unknown to older demanglers; builtin types take no substitution slot
    out = subprocess.run(["c++filt", n.replace("DF16b", "f")], capture_output=True, text=True).stdout.strip()
    out = out.replace("<float", "<__bf16", 1) if "DF16b" in n else out
    return out.split("(")[0].replace("void ", "")


def parse(path):
    txt, ks = open(path).read(), {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\s*s_endpgm", txt, re.S | re.M):
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in m.group(2).split("\n")]
        ks[m.group(1)] = {"ins": [i for i in ins if i and not i.endswith(":") and not i.startswith(".")]}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        if m.group(1) in ks:
            for key, field in (("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size"),
                               ("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr")):
                ks[m.group(1)][key] = int(re.search(rf"\.amdhsa_{field} (\d+)", m.group(2)).group(1))
    return {demangle(n): k for n, k in ks.items()}


def waves(vgpr):          # 512 VGPRs per SIMD lane, allocated in eights, at most 8 waves
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


def ops(k):
    return collections.Counter(i.split()[0] for i in k["ins"])


def mem(k):
    c = collections.Counter()
    for op, n in ops(k).items():
        if re.match(r"(global|buffer|flat|scratch)_(load|store|atomic)", op):
            c[re.sub(r"^(global|buffer|flat)_", "", op)] += n
        elif op.startswith("ds_"):
            c["ds_*"] += n
    return " ".join(f"{o}:{n}" for o, n in sorted(c.items()))


old, new = parse(sys.argv[1]), parse(sys.argv[2])
ren = dict(a.split("=") for a in sys.argv[3:])
back = {v: k for k, v in ren.items()}
for n in sorted(new):
    k, q = new[n], old.get(back.get(n, n))
    if q is None:
        print(f"{n}\n    NEW KERNEL"); continue
    if k["ins"] == q["ins"]:
        isa = "identical"
    else:
        d = ops(k); d.subtract(ops(q))
        d = ", ".join(f"{o} {v:+d}" for o, v in sorted(d.items()) if v)
        isa = f"{len(q['ins'])} -> {len(k['ins'])} instructions; " + (d if d else "same opcodes, other order / registers")
    print(f"{n}   (was {back.get(n, n)})" if n in back else n)
    print(f"    VGPR {q['vgpr']} -> {k['vgpr']} (waves/SIMD {waves(q['vgpr'])} -> {waves(k['vgpr'])})  SGPR {q['sgpr']} -> {k['sgpr']}  "
          f"LDS {q['lds']} -> {k['lds']}  scratch {q['scratch']} -> {k['scratch']}")
    print(f"    access old: {mem(q)}\n    access new: {mem(k)}" + ("" if mem(q) == mem(k) else "      <-- DIFFERS"))
    print(f"    ISA: {isa}")
gone = sorted(set(old) - {back.get(n, n) for n in new})
print("old kernels without a successor:", gone if gone else "none")
