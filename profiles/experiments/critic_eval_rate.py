"""What a held-out evaluation of the critic costs: CriticTrainer.evaluate (one cvae_critic_score launch per batch, one host read
at the end) over 50 000 frames — the 68 real frames of tests/golden/step_real_b68.npz repeated, the reference checkpoint's
weights (critic_real_b8.npz), targets cycling through [0, 1] — at batch 128 and 2048, HIP events around whole calls, median of
7, against the nearest route without it in the same process: per batch cvae_preprocess_u8_gather + cvae_critic_forward + the
torch expressions for the same sums (BCE with both logs clamped, squared and absolute error, the moments, the maximum and the
4 x 4 bin confusion counts), accumulated on the device in fp64 and read once.

    python profiles/experiments/critic_eval_rate.py [OUT.txt]
"""
import os, sys, statistics
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd.critic import CRITIC_KEYS, Critic
from critic_vae_amd.critic_train import CriticTrainer
from critic_vae_amd.episodes import DeviceDataset
from critic_vae_amd.lib import Handle
dev = torch.device("cuda:0")
N, REPS = 50_000, 7


def timed(f, reps=REPS):
    """ms per call of f: events around each whole call, after one warm-up -> (median, all)"""
    f()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), out


def bins(v):
    """episodes.value_bins on the device: 0 mid, 1 high, 2 low, 3 none"""
    mid = (v >= 0.4) & (v <= 0.6)
    return torch.where(mid, 0, torch.where(v >= 0.7, 1, torch.where(v <= 0.25, 2, 3)))


u8 = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))["u8"]
ck = np.load(os.path.join(ROOT, "tests", "golden", "critic_real_b8.npz"))
rep = -(-N // 68)
frames = torch.from_numpy(u8).to(dev).repeat(rep, 1, 1, 1)[:N].contiguous()
targets = ((torch.arange(N, device=dev) % 101).float() / 100.0).reshape(N, 1).contiguous()
ds = DeviceDataset(frames, targets, np.stack([np.arange(N) // 1000, np.arange(N) % 1000], 1))
lines = []
for B in (128, 2048):
    h = Handle(64, B)
    critic = Critic(handle=h).to(dev)
    critic.load_state_dict({k: torch.from_numpy(ck["w/" + k]) for k, _ in CRITIC_KEYS})
    tr = CriticTrainer(critic)
    x, t, p = torch.empty(B, 3, 64, 64, device=dev), torch.empty(B, 1, device=dev), torch.empty(B, 1, device=dev)
    idx = torch.arange(N, device=dev)

    def two_kernels_and_torch():
        sums = torch.zeros(10, dtype=torch.float64, device=dev)
        conf = torch.zeros(16, dtype=torch.int64, device=dev)
        worst = torch.full((), -float("inf"), device=dev)
        for b in range(0, N, B):
            nb = min(B, N - b)
            ds.gather(h, nb, idx[b:b + nb], x[:nb], t[:nb])
            h.critic_forward(nb, x[:nb], critic.flat, p[:nb])
            pv, tv = p[:nb, 0], t[:nb, 0]
            bce = -(tv * torch.log(pv).clamp_min(-100.0) + (1.0 - tv) * torch.log(1.0 - pv).clamp_min(-100.0))
            d = pv - tv
            ok = torch.isfinite(pv) & torch.isfinite(tv) & torch.isfinite(bce) & torch.isfinite(d * d)
            pd, td = pv.double(), tv.double()
            cols = torch.stack([torch.ones_like(pd), bce.double(), (d * d).double(), d.abs().double(), pd, td, pd * pd, td * td, pd * td])
            sums[:9] += torch.where(ok, cols, 0.0).sum(1)
            sums[9] += nb
            worst = torch.maximum(worst, torch.where(ok, d.abs(), -float("inf")).max())
            conf.scatter_add_(0, bins(tv) * 4 + bins(pv), ok.long())                 # no host sync, unlike bincount / a masked index
        return torch.cat([sums, worst.double().reshape(1), conf.double()]).cpu().numpy()          # the one host read

    te, ae = timed(lambda: tr.evaluate(ds, B))
    tp, ap = timed(lambda: tr.evaluate(ds, B, per_frame=True))
    tb, ab = timed(two_kernels_and_torch)
    r, old = tr.evaluate(ds, B), two_kernels_and_torch()
    same = (r["finite_frames"] == int(old[0]) and np.array_equal(r["confusion"].reshape(-1), old[11:].astype(np.int64))
            and abs(r["bce"] - old[1] / old[0]) <= 1e-6 and abs(r["mse"] - old[2] / old[0]) <= 1e-9)      # torch's log is not the kernel's logf
    f = lambda a: " ".join(f"{v:.1f}" for v in a)
    lines.append(f"B = {B}, {N} frames: evaluate {f(ae)} ms, median {te:.1f} ms = {N / te * 1e3:.0f} frames/s; with per_frame rows "
                 f"{f(ap)} ms, median {tp:.1f} ms = {N / tp * 1e3:.0f} frames/s; cvae_preprocess_u8_gather + cvae_critic_forward + torch "
                 f"sums: {f(ab)} ms, median {tb:.1f} ms = {N / tb * 1e3:.0f} frames/s; evaluate / that = {te / tb:.3f}; "
                 f"bce {r['bce']:.6f} bin agreement {r['bin_agreement']:.4f}; the two routes agree: {same}")
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text + "\n")
