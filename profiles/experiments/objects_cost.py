"""What objects from masks cost: cvae_mask_objects on the thresholded masks of the 68 real fixture frames (B = 68, and repeated to
the 2 450 frames of one episode) against today's route — the masks copied to the host and labelled per frame in a Python loop
(scipy.ndimage.label plus sums and boxes where scipy is there, objects_host otherwise: the first line says which) —; one
frame-batch of the worst patterns (the one-pixel spiral; Bernoulli p = 0.593 under 4-connectivity) at both widths with their pass
counts; cvae_object_overlap at the same sizes; and `segment -video --objects` end to end against the run without the flag
(eval_maps on critic-gradient masks).  Same process, variants alternating; HIP events around 20 calls, median of 7 (the host
route and the end-to-end runs: wall time around one synchronised call, median of 7).

    python profiles/experiments/objects_cost.py [OUT.txt]
"""
import os, sys, statistics, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from critic_vae_amd import lib as cvlib
from critic_vae_amd import objects as ob
from critic_vae_amd import segment as seg
from critic_vae_amd.critic import Critic
from critic_vae_amd.objects import ObjectFilter
import objects_tools as OT
try:
    from scipy import ndimage as ndi
except ImportError:
    ndi = None
dev = torch.device("cuda:0")
N, REPS = 20, 7
GOLDEN = os.path.join(ROOT, "tests", "golden")


def events(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / N


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(fs, measures, warm=2):
    for f in fs:
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    out = [[] for _ in fs]
    for _ in range(REPS):
        for k, f in enumerate(fs):
            out[k].append(measures[k](f))
    return out


def report(lines, labels, samples, unit=1e3, name="us"):
    base = statistics.median(samples[0])
    for label, s in zip(labels, samples):
        med = statistics.median(s)
        lines.append(f"  {label:<72s} {' '.join(f'{x * unit:.1f}' for x in s)} | median {med * unit:.1f} {name} ({med / base:.2f}x), "
                     f"spread {min(s) * unit:.1f}..{max(s) * unit:.1f}")


def host_route(mask_dev, values_dev, M=32):
    """today's route: one copy to the host, then per frame label + area, box and sums of the first M objects"""
    m, v = mask_dev.cpu().numpy() != 0, values_dev.cpu().numpy()
    if ndi is None:
        return ob.objects_host(m, ObjectFilter(max_objects=M), v)
    st = np.ones((3, 3), bool)
    out = []
    for f in range(m.shape[0]):
        lab, n = ndi.label(m[f], st)
        idx = np.arange(1, min(n, M) + 1)
        out.append((n, ndi.sum(m[f], lab, idx), ndi.find_objects(lab)[:M], ndi.sum(v[f], lab, idx), ndi.center_of_mass(m[f], lab, idx)))
    return out


lines = ["host route: " + (f"scipy.ndimage {__import__('scipy').__version__}: label + sum + find_objects + center_of_mass per frame"
                           if ndi is not None else "objects_host (no scipy on this machine)")]
fx = np.load(os.path.join(GOLDEN, "segment_real_b68.npz"))
u8 = np.load(os.path.join(GOLDEN, "step_real_b68.npz"))["u8"]
cw = np.load(os.path.join(GOLDEN, "critic_real_b8.npz"))
critic = Critic(64, handle=cvlib.Handle(64, 68)).to(dev)
critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
preds, maps, maxv = seg.critic_maps(u8, critic, "grad", chunk=68)
r0 = seg.eval_maps(u8, maps, maxv, preds, fx["gt"])
thr68, d68 = r0["device"]["thr_masks"], r0["device"]["diff_u8"]
filt = ObjectFilter(min_area=4, fill_holes=True)
plain = ObjectFilter()

# ---- the real masks ----
for B in (68, 2450):
    rep = (B + 67) // 68
    m, v = thr68.repeat(rep, 1, 1)[:B].contiguous(), d68.repeat(rep, 1, 1)[:B].contiguous()
    info = ob.mask_objects(m, filt, values=v)["info"].cpu().numpy()
    lines.append(f"B = {B} thresholded masks of the real frames (critic-gradient masks, thr 50), 64 x 64: {info[:, 0].mean():.1f} components and "
                 f"{info[:, 1].mean():.1f} kept per frame, passes {info[:, 3].min()}..{info[:, 3].max()}; us per call")
    la = ob.mask_objects(m, plain, labels=True)["labels"]
    lb = ob.mask_objects(torch.from_numpy(np.tile(fx["gt"], (rep, 1, 1))[:B]).to(dev), plain, labels=True)["labels"]
    variants = [("cvae_mask_objects: labels + table, no fill or filter", lambda: ob.mask_objects(m, plain, values=v, labels=True), events),
                ("cvae_mask_objects: fill_holes, min_area 4, labels + table", lambda: ob.mask_objects(m, filt, values=v, labels=True), events),
                ("cvae_object_overlap, M = 32", lambda: ob.object_overlap(la, lb, 32), events),
                ("host route (copy + per-frame loop; wall)", lambda: host_route(m, v), wall)]
    report(lines, [x[0] for x in variants], interleaved([x[1] for x in variants], [x[2] for x in variants]))

# ---- the worst patterns: one frame-batch (B = 256) of each ----
for W in (64, 128):
    P = OT.patterns(W)
    for name, conn in (("spiral", 4), ("spiral_180", 4), ("serpentine", 4), ("bernoulli_0.593", 4), ("bernoulli_0.593", 8), ("checker", 4)):
        m = torch.from_numpy(P[name].astype(np.uint8)).to(dev).repeat(256, 1, 1).contiguous()
        for fname, f in (("no fill", ObjectFilter(connectivity=conn)), ("fill + min_area 4", ObjectFilter(connectivity=conn, fill_holes=True, min_area=4))):
            passes = int(ob.mask_objects(m, f)["info"][0, 3])
            s = interleaved([lambda: ob.mask_objects(m, f, labels=True)], [events])[0]
            lines.append(f"  W = {W} B = 256 {name} under {conn}, {fname}: passes {passes}; " + " ".join(f"{x * 1e3:.1f}" for x in s)
                         + f" | median {statistics.median(s) * 1e3:.1f} us, spread {min(s) * 1e3:.1f}..{max(s) * 1e3:.1f}")

# ---- end to end: the tail of segment -video with and without --objects, 68 frames ----
variants = [("eval_maps (segment -video, critic-grad masks), 68 frames", lambda: seg.eval_maps(u8, maps, maxv, preds, fx["gt"]), wall),
            ("eval_maps(..., objects=ObjectFilter(min_area=4, fill_holes=True))", lambda: seg.eval_maps(u8, maps, maxv, preds, fx["gt"], objects=filt), wall)]
lines.append("segment -video end to end (normalise, threshold, CRF, IoU, bins; with --objects also both masks and the ground truth as objects, "
             "overlaps, one read, PQ); ms per call, wall")
report(lines, [x[0] for x in variants], interleaved([x[1] for x in variants], [x[2] for x in variants], warm=1), unit=1.0, name="ms")

print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
