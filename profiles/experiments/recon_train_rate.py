"""fit_device over a ReconDataset (this tree) against fit_device over a DeviceDataset run from another checkout (the parent
commit's tree, built), 5 alternating epochs of 50 000 entries; two child processes, one active at a time.

    python profiles/experiments/recon_train_rate.py PARENT_TREE [OUT.txt]
"""
import os, subprocess, sys, statistics
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PARENT = os.path.abspath(sys.argv[1])
out = open(sys.argv[2] if len(sys.argv) > 2 else os.devnull, "w")
def say(s):
    print(s, flush=True); out.write(s + "\n"); out.flush()
for prec, B in (("f32", 256), ("bf16", 2048)):
    kids = {}
    for side, tree in (("parent_u8", PARENT), ("recon", ROOT)):
        env = dict(os.environ, PYTHONPATH=tree)
        kids[side] = subprocess.Popen([sys.executable, os.path.join(HERE, "recon_train_child.py"), side.split("_")[0] if side == "recon" else "u8", prec, str(B)],
                                      stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=tree)
    for side, k in kids.items():
        line = k.stdout.readline().strip()
        if line != "ready":
            say(f"{side}: child failed to start ({line!r})"); sys.exit(1)
    rates = {s: [] for s in kids}
    for ep in range(5):
        for side, k in kids.items():
            k.stdin.write("go\n"); k.stdin.flush()
            rates[side].append(float(k.stdout.readline()))
    for k in kids.values():
        k.stdin.write("quit\n"); k.stdin.flush(); k.wait(timeout=60)
    for side, r in rates.items():
        say(f"{prec} B={B} {side}: epochs {' '.join(f'{x:.0f}' for x in r)} img/s; median {statistics.median(r):.0f}, spread {100 * (max(r) - min(r)) / statistics.median(r):.2f} %")
    say(f"{prec} B={B}: recon median / parent uint8 median = {statistics.median(rates['recon']) / statistics.median(rates['parent_u8']):.4f}")
