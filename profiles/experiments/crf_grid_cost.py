"""What the CRF grid search costs: one cvae_crf_grid call for K candidates beside the route it replaces, K sequential
dense_crf + mask_counts calls as sweep_maps loops them (the baseline is that route, not the code under test), on the 68 real
frames of tests/golden/step_real_b68.npz with the difference masks of the synthetic-weight VAE, as they are (B = 68) and repeated
to an episode-sized set (B = 2 450), at the reference's CRF parameters (10 iterations).  Cases: the 13 thresholds of -thresh, a
3 x 3 (w1, w2) grid at threshold 50, and K = 1; then one pair pass per instantiation (KC = 1, 4, 8) as half the difference
between calls of 3 and of 1 iterations, beside the same of cvae_dense_crf.  HIP events around whole calls, median of 7, the
variants alternating in one process.

    python profiles/experiments/crf_grid_cost.py [OUT.txt]
"""
import os, sys, statistics
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import segment as seg, synth
from critic_vae_amd.nets import VariationalAutoencoder
dev = torch.device("cuda:0")
REPS = 7
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def window(f, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(variants, calls):
    """{name: f} -> {name: (median ms per call, all)}: one warm-up each, then REPS rounds, each round one window per variant."""
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(REPS):
        for k, f in variants.items():
            got[k].append(window(f, calls))
    return {k: (statistics.median(v), v) for k, v in got.items()}


u8_68 = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))["u8"]
fx = np.load(os.path.join(ROOT, "tests", "golden", "segment_real_b68.npz"))
vae = VariationalAutoencoder(max_batch=68, seed=0).to(dev)
vae.load_reference_params(synth.make_params(0))
_, diff68, maxv68 = seg._infer(u8_68, vae, None, fx["preds"], None)
W1, ALPHA, BETA, W2, GAMMA, IT = seg.CRF_REF
KERN = (ALPHA, BETA, GAMMA)

for B, calls in ((68, 5), (2450, 1)):
    sel = torch.arange(B, device=dev) % 68
    frames = torch.from_numpy(u8_68).to(dev)[sel].contiguous()
    gt = torch.from_numpy(fx["gt"].astype(np.uint8)).to(dev)[sel].contiguous()
    u8d, _ = seg.normalize_diffs(diff68, maxv68)                          # the normalisation of the 68 frames, repeated
    u8d = u8d[sel].contiguous()

    def separate(cands, it=IT):
        """the parent route: per candidate the thresholded mask, dense_crf, mask_counts, summed over the frames"""
        out = []
        for t, pf, w1, w2 in cands:
            crf = seg.dense_crf(frames, (u8d > t), (w1, ALPHA, BETA, w2, GAMMA, it), pf)
            out.append(seg.mask_counts(crf, gt).sum(0))
        return torch.stack(out)

    def fused(cands, it=IT):
        return seg.crf_grid(frames, gt, KERN, cands, (it,), diff_u8=u8d)[0].sum(1)

    sweep = [(t, seg.P_FLOOR, W1, W2) for t in seg.SWEEP]
    grid = [(seg.THRESHOLD, seg.P_FLOOR, a, b) for a in (11, 22, 44) for b in (4, 8, 16)]
    one = [(seg.THRESHOLD, seg.P_FLOOR, W1, W2)]
    for name, cands in (("13 thresholds", sweep), ("3 x 3 (w1, w2)", grid), ("K = 1", one)):
        a, b = separate(cands), fused(cands)
        off = int((a - b).abs().sum())
        say(f"B = {B:4d}  {name:<15} counts of the two routes differ by {off} pixels in all (of {int(a.sum())} counted; ties of Q(1) at 0.5 may fall either way)")
        res = alternate({"separate": lambda: separate(cands), "fused": lambda: fused(cands)}, calls)
        for k, (med, allv) in res.items():
            say(f"B = {B:4d}  {name:<15} {k:<9} {med:10.3f} ms per call  {med / len(cands):9.3f} ms per candidate   [{min(allv):.3f} .. {max(allv):.3f}]  "
                f"spread {(max(allv) - min(allv)) / med * 100:.1f} %")
        say(f"B = {B:4d}  {name:<15} separate / fused = {res['separate'][0] / res['fused'][0]:.2f}x")
    # one pair pass (with its Gaussian row pass) per instantiation: (3 iterations - 1 iteration) / 2
    passes = {}
    for label, cands in (("KC = 1", one), ("KC = 4", grid[:4]), ("KC = 8", sweep[:8])):
        passes[f"grid {label} it 1"] = (lambda c=cands: fused(c, 1))
        passes[f"grid {label} it 3"] = (lambda c=cands: fused(c, 3))
    passes["dense_crf it 1"] = lambda: separate(one, 1)
    passes["dense_crf it 3"] = lambda: separate(one, 3)
    res = alternate(passes, calls)
    for label in ("grid KC = 1", "grid KC = 4", "grid KC = 8", "dense_crf"):
        t1, t3 = res[label + " it 1"][0], res[label + " it 3"][0]
        k = int(label[-1]) if label.startswith("grid") else 1
        say(f"B = {B:4d}  one pass, {label:<12} {(t3 - t1) / 2:9.3f} ms  = {(t3 - t1) / 2 / k:9.3f} ms per variant   (calls: it 1 {t1:.3f} ms, it 3 {t3:.3f} ms)")

text = "\n".join(lines)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
