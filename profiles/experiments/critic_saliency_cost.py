"""What the critic-side masks cost: cvae_critic_forward, cvae_critic_collect, cvae_critic_saliency (steps 1 and 32) and
cvae_critic_occlusion (P = 8) at batch 128 and 2048 on the 68 real frames of tests/golden/step_real_b68.npz repeated, the
reference checkpoint's weights (critic_real_b8.npz), each beside the torch route to the same numbers on the same device: the
critic as torch.nn modules (the reference's layers), autograd for the gradients (for integrated gradients one
forward + backward per pass, accumulated), and for occlusion a loop of 65 batched forwards, one per patch.  HIP events around
20 calls, median of 7, the variants alternating in one process.  Then `segment -video --mask-source ...` end to end for an
episode-sized set (2 450 frames, host clock around calls that end in host arrays) beside the `vae` source.

    python profiles/experiments/critic_saliency_cost.py [OUT.txt]
"""
import os, sys, statistics, time
import numpy as np
import torch
from torch import nn
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import segment as seg, synth
from critic_vae_amd.critic import CRITIC_KEYS, Critic
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
dev = torch.device("cuda:0")
CALLS, REPS, IG, P = 20, 7, 32, 8


def torch_critic(w):
    """critic_net.py:15-42 in eval mode (Dropout = identity) without the Sigmoid: returns (features, crit -> logit)."""
    f = nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2),
                      nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2), nn.Identity(), nn.Conv2d(8, 16, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2),
                      nn.Identity(), nn.Conv2d(16, 32, 4), nn.ReLU())
    c = nn.Sequential(nn.Flatten(), nn.Linear(32, 32), nn.ReLU(), nn.Identity(), nn.Linear(32, 1))
    sd = {k: torch.from_numpy(w["w/" + k]) for k, _ in CRITIC_KEYS}
    f.load_state_dict({k[len("features."):]: v for k, v in sd.items() if k.startswith("features.")})
    c.load_state_dict({k[len("crit."):]: v for k, v in sd.items() if k.startswith("crit.")})
    return f.to(dev).eval().requires_grad_(False), c.to(dev).eval().requires_grad_(False)


def window(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


def alternate(variants):
    """{name: f} -> {name: (median ms per call, all)}: one warm-up each, then REPS rounds, each round one window per variant."""
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(REPS):
        for k, f in variants.items():
            got[k].append(window(f))
    return {k: (statistics.median(v), v) for k, v in got.items()}


u8 = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))["u8"]
ck = np.load(os.path.join(ROOT, "tests", "golden", "critic_real_b8.npz"))
feat, crit = torch_critic(ck)
grey = torch.tensor([0.2989, 0.5870, 0.1140], device=dev).reshape(1, 3, 1, 1)
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


for B in (128, 2048):
    h = Handle(64, B)
    critic = Critic(handle=h).to(dev)
    critic.load_state_dict({k: torch.from_numpy(ck["w/" + k]) for k, _ in CRITIC_KEYS})
    frames = torch.from_numpy(u8).to(dev).repeat(-(-B // 68), 1, 1, 1)[:B].contiguous()
    x = critic.preprocess(frames)
    fill = x.mean(dim=(0, 2, 3)).tolist()
    pred = torch.empty(B, 1, device=dev)
    emb = [torch.empty(B, *s, device=dev) for s in ((8, 32, 32), (8, 16, 16), (8, 8, 8), (16, 4, 4), (32, 1, 1))]
    mp, mx, g = torch.empty(B, 64, 64, device=dev), torch.empty(B, device=dev), torch.empty(B, 3, 64, 64, device=dev)
    drop = torch.empty(B, 64 // P, 64 // P, device=dev)

    def t_forward():
        with torch.no_grad():
            return torch.sigmoid(crit(feat(x)))

    def t_collect():
        with torch.no_grad():
            a, out = x, []
            for layer in feat:
                a = layer(a)
                if isinstance(layer, nn.MaxPool2d):
                    out.append(a)
            out.append(a)
            return torch.sigmoid(crit(a)), out

    def t_grad_of(xs):
        xs = xs.detach().requires_grad_()
        z = crit(feat(xs))
        return torch.autograd.grad(z.sum(), xs)[0], z

    def t_map(gr):
        m = (gr.abs() * grey).sum(1)
        return m, m.amax(dim=(1, 2))

    def t_saliency():
        gr, z = t_grad_of(x)
        return (torch.sigmoid(z), gr) + t_map(gr)

    def t_ig():
        acc = torch.zeros_like(x)
        for k in range(1, IG + 1):
            gr, z = t_grad_of(x * (k / IG))
            acc += gr
        gr = acc * x * (1.0 / IG)
        return (torch.sigmoid(z), gr) + t_map(gr)

    def t_occlusion():
        with torch.no_grad():
            p0 = torch.sigmoid(crit(feat(x)))
            fl = torch.tensor(fill, device=dev).reshape(1, 3, 1, 1)
            d = torch.empty(B, 64 // P, 64 // P, device=dev)
            xo = x.clone()
            for py in range(64 // P):
                for px in range(64 // P):
                    ys, xs = slice(py * P, py * P + P), slice(px * P, px * P + P)
                    xo[:, :, ys, xs] = fl
                    d[:, py, px] = (p0 - torch.sigmoid(crit(feat(xo))))[:, 0]
                    xo[:, :, ys, xs] = x[:, :, ys, xs]
            m = d.clamp_min(0).repeat_interleave(P, 1).repeat_interleave(P, 2)
            return p0, d, m, m.amax(dim=(1, 2))

    variants = {
        "forward   hip": lambda: h.critic_forward(B, x, critic.flat, pred),
        "forward   torch": t_forward,
        "collect   hip": lambda: h.critic_collect(B, x, critic.flat, pred, emb),
        "collect   torch": t_collect,
        "grad      hip": lambda: h.critic_saliency(B, x, critic.flat, 1, pred, mp, mx, grad=g),
        "grad      torch": t_saliency,
        f"ig {IG:<3}    hip": lambda: h.critic_saliency(B, x, critic.flat, IG, pred, mp, mx, grad=g),
        f"ig {IG:<3}    torch": t_ig,
        f"occl P={P}  hip": lambda: h.critic_occlusion(B, x, critic.flat, P, fill, pred, drop, mp, mx),
        f"occl P={P}  torch": t_occlusion,
    }
    # the two routes give the same numbers (torch's convolutions sum in another order)
    h.critic_saliency(B, x, critic.flat, 1, pred, mp, mx, grad=g)
    tg = t_saliency()
    gap_g = float(((g - tg[1]).abs().amax(dim=(1, 2, 3)) / tg[1].abs().amax(dim=(1, 2, 3))).max())
    h.critic_saliency(B, x, critic.flat, IG, pred, mp, mx, grad=g)
    ti = t_ig()
    gap_i = float(((g - ti[1]).abs().amax(dim=(1, 2, 3)) / ti[1].abs().amax(dim=(1, 2, 3))).max())
    h.critic_occlusion(B, x, critic.flat, P, fill, pred, drop, mp, mx)
    gap_o = float((drop - t_occlusion()[1]).abs().max())
    say(f"B = {B}: hip vs torch: gradient within {gap_g:.1e} of each frame's max, integrated gradients {gap_i:.1e} "
                 f"(a pool tie taken the other way shows here), occlusion drop {gap_o:.1e} absolute")
    res = alternate(variants)
    for k, (med, allv) in res.items():
        say(f"B = {B:4d}  {k:<18} {med:9.3f} ms per call  {B / med / 1e3:9.3f} M frames/s   [{min(allv):.3f} .. {max(allv):.3f}]")
    for k in ("forward  ", "collect  ", "grad     ", f"ig {IG:<3}   ", f"occl P={P} "):
        say(f"B = {B:4d}  {k.strip():<10} torch / hip = {res[k + ' torch'][0] / res[k + ' hip'][0]:.2f}x")

# ---- segment -video end to end, 2 450 frames ----
N = 2450
gt68 = np.load(os.path.join(ROOT, "tests", "golden", "segment_real_b68.npz"))["gt"]
sel = np.arange(N) % 68
frames, gt = u8[sel], gt68[sel]
vae = VariationalAutoencoder(max_batch=256, seed=0).to(dev)
vae.load_reference_params(synth.make_params(0))
critic = Critic(handle=Handle(64, 256)).to(dev)
critic.load_state_dict({k: torch.from_numpy(ck["w/" + k]) for k, _ in CRITIC_KEYS})


def e2e(source):
    if source == "vae":
        return seg.eval_frames(frames, vae, gt, critic=critic, chunk=256)
    p, m, v = seg.critic_maps(frames, critic, seg.MASK_SOURCES[source], steps=IG, patch=P, chunk=256)
    return seg.eval_maps(frames, m, v, p, gt)


def maps_only(source):
    if source == "vae":
        out = seg._infer(frames, vae, critic, None, 256)
    else:
        out = seg.critic_maps(frames, critic, seg.MASK_SOURCES[source], steps=IG, patch=P, chunk=256)
    torch.cuda.synchronize()
    return out


for fn, label in ((e2e, "end to end (maps, normalise, threshold, CRF, IoUs, bins; host arrays)"), (maps_only, "maps only (frames on the host -> preds, maps, maxima on the device)")):
    times = {s: [] for s in seg.MASK_SOURCES}
    for s in seg.MASK_SOURCES:
        fn(s)
    for _ in range(5):
        for s in seg.MASK_SOURCES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(s)
            times[s].append(time.perf_counter() - t0)
    for s, v in times.items():
        say(f"{N} frames, {label}: --mask-source {s:<17} {statistics.median(v) * 1e3:8.1f} ms  [{min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f}]")

text = "\n".join(lines)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
