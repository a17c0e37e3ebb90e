"""Rate of the critic's training step: CriticTrainer.step (keep mask drawn on the device inside the step, as torch's Dropout
draws its masks inside its step; then cvae_critic_grad + cvae_adam_step) against the same network as torch.nn modules trained
by torch on the device, same process, alternating — HIP events around 20 steps, median of 7 — at B = 128 and B = 2048; the
step with a precomputed mask is timed too, and the kernel launches of one step of each are counted with torch.profiler.
Then one CriticTrainer.fit_device epoch over 100 000 frames (gather launch + mask draw + step per batch of 128).
No threshold: the numbers are reported as they come.

    python profiles/experiments/critic_train_rate.py [OUT.txt]
"""
import os, sys, statistics, time
import numpy as np
import torch
from torch import nn
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd.critic import Critic
from critic_vae_amd.critic_train import CriticTrainer, initial_state_dict
from critic_vae_amd.episodes import DeviceDataset
from critic_vae_amd.lib import CRITIC_KEEP, Handle
dev = torch.device("cuda:0")
N, REPS, P_DROP = 20, 7, 0.3


def torch_critic():
    """critic_net.py's default network, written out (the kernel's counterpart in torch.nn)."""
    features = nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2),
                             nn.Conv2d(8, 8, 3, 1, 1), nn.ReLU(), nn.MaxPool2d(2), nn.Dropout(P_DROP), nn.Conv2d(8, 16, 3, 1, 1), nn.ReLU(),
                             nn.MaxPool2d(2), nn.Dropout(P_DROP), nn.Conv2d(16, 32, 4), nn.ReLU())
    crit = nn.Sequential(nn.Flatten(), nn.Linear(32, 32), nn.ReLU(), nn.Dropout(P_DROP), nn.Linear(32, 1), nn.Sigmoid())
    return nn.Sequential(features, crit)


def events(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / N


def interleaved(fa, fb):
    for f in (fa, fb):
        f(); f(); f()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(REPS):
        a.append(events(fa)); b.append(events(fb))
    return statistics.median(a), statistics.median(b), a, b


def launches(f):
    """device kernels of one call of f, counted by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        f()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def fmt(v):
    return " ".join(f"{x * 1e3:.0f}" for x in v)


lines = []
for B in (128, 2048):
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    pool = [(torch.rand(B, 3, 64, 64, device=dev, generator=gen), torch.rand(B, device=dev, generator=gen),
             (torch.rand(B, CRITIC_KEEP, device=dev, generator=gen) >= P_DROP).to(torch.uint8)) for _ in range(4)]
    critic = Critic(handle=Handle(64, B)).to(dev)
    critic.load_state_dict(initial_state_dict(0))
    tr = CriticTrainer(critic, dropout=P_DROP)
    net = torch_critic().to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    k = [0, 0]

    def hip_step():
        x, t, _ = pool[k[0] % 4]; k[0] += 1
        tr.step(x, t, generator=gen)

    def hip_step_given():
        x, t, keep = pool[k[0] % 4]; k[0] += 1
        tr.step(x, t, keep=keep)

    def torch_step():
        x, t, _ = pool[k[1] % 4]; k[1] += 1
        opt.zero_grad(set_to_none=True)
        nn.functional.binary_cross_entropy(net(x)[:, 0], t).backward()
        opt.step()

    th, tt, ah, at = interleaved(hip_step, torch_step)
    tg, _, ag, _ = interleaved(hip_step_given, torch_step)
    try:
        nh, ng, nt = launches(hip_step), launches(hip_step_given), launches(torch_step)
    except Exception as e:                                  # the counts are a courtesy; the times stand without them
        nh = ng = nt = f"? ({type(e).__name__})"
    lines.append(f"B = {B}: HIP step, mask drawn in the step ({nh} kernel launches) {fmt(ah)} us, median {th * 1e3:.0f} us = "
                 f"{B / th:.0f} k images/s; torch.nn + torch.optim.Adam ({nt} kernel launches) {fmt(at)} us, median {tt * 1e3:.0f} us = "
                 f"{B / tt:.0f} k images/s; HIP / torch time = {th / tt:.3f}; HIP step with the mask given ({ng} kernel launches) "
                 f"{fmt(ag)} us, median {tg * 1e3:.0f} us")
    del tr, critic, net, opt, pool

n, B = 100_000, 128
frames = torch.randint(0, 256, (n, 64, 64, 3), dtype=torch.uint8, device=dev)
ds = DeviceDataset(frames, torch.rand(n, 1, device=dev), np.zeros((n, 2), np.int64))
critic = Critic(handle=Handle(64, B)).to(dev)
critic.load_state_dict(initial_state_dict(0))
tr = CriticTrainer(critic, dropout=P_DROP)
gen = torch.Generator(device=dev); gen.manual_seed(2)
tr.fit_device(ds, B, epochs=1, generator=gen)            # warm-up epoch
torch.cuda.synchronize()
t0 = time.time()
log = tr.fit_device(ds, B, epochs=1, generator=gen)
torch.cuda.synchronize()
dt = time.time() - t0
lines.append(f"fit_device, one epoch of {n} frames at batch {B} ({log.shape[0]} steps; per step: index slice, gather launch, mask draw, "
             f"cvae_critic_grad, cvae_adam_step, loss copy): {dt:.3f} s = {n / dt / 1e3:.0f} k images/s, {dt / log.shape[0] * 1e6:.0f} us per step (wall clock)")
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in lines:
        print(line, flush=True); f.write(line + "\n")
