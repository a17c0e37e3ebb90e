"""This tree against a built checkout of its parent commit on the dataset path: the digests of curate_digest.py, the medians of
recon_build_rate.py over alternating fresh processes, and fit_device epochs of recon_train_child.py on the same kind of
dataset in both trees.  One process on the GPU at a time (the two training children of a pair take turns), each under a
time limit; the first failure ends the run.

    python profiles/experiments/curation_ab.py PARENT_TREE OUT.txt [ROUNDS]
"""
import os, re, statistics, subprocess, sys
HERE = os.path.dirname(os.path.abspath(__file__))
TREES = {"parent": os.path.abspath(sys.argv[1]), "this": os.path.dirname(os.path.dirname(HERE))}
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
out = open(sys.argv[2], "w")
def say(s):
    print(s, flush=True); out.write(s + "\n"); out.flush()
def run(tree, script, *args, timeout=300):
    r = subprocess.run([sys.executable, script, *args], env=dict(os.environ, PYTHONPATH=tree), cwd=tree, text=True,
                       capture_output=True, timeout=timeout)
    if r.returncode != 0:
        say(f"FAILED rc {r.returncode}: {script} in {tree}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"); sys.exit(1)
    return r.stdout

# 1. the datasets
dig = {side: [l for l in run(tree, os.path.join(HERE, "curate_digest.py"), tree).splitlines() if l.startswith("digest")]
       for side, tree in TREES.items()}
for a, b in zip(dig["parent"], dig["this"]):
    say(f"parent {a}\nthis   {b}")
say(f"digests: {len(dig['this'])} arrays, equal between the trees: {dig['parent'] == dig['this'] and len(dig['this']) == 8}")

# 2. the build rate: each tree's own recon_build_rate.py, fresh processes in turn
med = {side: {"curate_recon": [], "curate": []} for side in TREES}
for i in range(ROUNDS):
    for side, tree in TREES.items():
        for line in run(tree, os.path.join(tree, "profiles", "experiments", "recon_build_rate.py")).splitlines():
            m = re.match(r"(curate_recon|curate): runs (.*) ms; median ([0-9.]+) ms", line)
            if m:
                med[side][m.group(1)].append(float(m.group(3)))
                say(f"build {side} process {i} {m.group(1)}: runs {m.group(2)} ms; median {m.group(3)} ms")
for k in ("curate_recon", "curate"):
    p, t = med["parent"][k], med["this"][k]
    say(f"{k}: parent medians {p} ms, median {statistics.median(p):.1f}, spread (max - min) {max(p) - min(p):.1f}; this tree medians {t} ms, "
        f"median {statistics.median(t):.1f}; difference {statistics.median(t) - statistics.median(p):+.1f} ms")

# 3. fit_device, the same dataset kind in both trees
for prec, B in (("f32", 256), ("bf16", 2048)):
    for kind in ("u8", "recon"):
        kids = {side: subprocess.Popen([sys.executable, os.path.join(HERE, "recon_train_child.py"), kind, prec, str(B)], stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, text=True, env=dict(os.environ, PYTHONPATH=tree), cwd=tree)
                for side, tree in TREES.items()}
        try:
            for side, k in kids.items():
                if k.stdout.readline().strip() != "ready":
                    say(f"{side}: training child failed to start"); sys.exit(1)
            rates = {s: [] for s in kids}
            for _ in range(5):
                for side, k in kids.items():
                    k.stdin.write("go\n"); k.stdin.flush()
                    rates[side].append(float(k.stdout.readline()))
        finally:
            for k in kids.values():
                try:
                    k.stdin.write("quit\n"); k.stdin.flush(); k.wait(timeout=60)
                except Exception:
                    k.kill()
        for side, r in rates.items():
            say(f"fit_device {prec} B={B} {kind} {side}: epochs {' '.join(f'{x:.0f}' for x in r)} img/s; median {statistics.median(r):.0f}, "
                f"spread {100 * (max(r) - min(r)) / statistics.median(r):.2f} %")
        say(f"fit_device {prec} B={B} {kind}: this / parent = {statistics.median(rates['this']) / statistics.median(rates['parent']):.4f}")
