"""The headline step of this tree against a built checkout of its parent: bench.py of each, alternating, every run a process of
its own, PAIRS pairs on one box.  One line per run: tree, pair, ms/step, images/s; then the medians and spans.

    python profiles/experiments/bench_pairs.py PARENT_TREE [OUT.txt] [PAIRS]
"""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
parent = os.path.abspath(sys.argv[1])
out = sys.argv[2] if len(sys.argv) > 2 else os.devnull
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
ARGS = ["--gpus", "1", "--steps", "300", "--warmup", "30", "--no-cpu-baseline", "--no-probe", "--no-extra-configs", "--no-fwd-bwd-rate"]
lines, ms = [], {"parent": [], "this": []}
for i in range(1, pairs + 1):
    for name, tree in (("parent", parent), ("this", ROOT)):
        env = dict(os.environ, CVAE_BENCH_DETAIL=os.devnull)
        r = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + ARGS, cwd=tree, env=env, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:              # nothing more on the GPU after a failed run
            sys.exit(f"{name} run {i} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        ms[name].append(res["ms_per_step"])
        lines.append(f"{name} {i} {res['ms_per_step']} {res['value']}")
        print(lines[-1], flush=True)
for name in ("parent", "this"):
    v = ms[name]
    lines.append(f"{name}: median {statistics.median(v):.4f} ms/step ({min(v):.4f} .. {max(v):.4f}, span {max(v) - min(v):.4f})")
    print(lines[-1], flush=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
