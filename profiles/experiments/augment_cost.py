"""What augmentation in the batch gather costs: the plain gather, the augmented gather with everything on, and the torch
route to the same tensor (plain gather, then device indexing with PRECOMPUTED index maps, a multiply and a clamp — building
the maps is not timed, which favours torch), alternating in one process — HIP events around 20 calls, median of 7 rounds —
for uint8 frames at B = 256 and B = 2048 and fp32 entries at B = 2048 (W = 64).  Then one fit_device epoch over 50 000
frames (the 68 fixture frames repeated) with and without an augmentation: FusedTrainer in fp32 at B = 256 and in bf16 mode at
B = 2048, CriticTrainer at B = 128; wall time around the epoch with a synchronize, the two alternating, median of 3.

    python profiles/experiments/augment_cost.py [OUT.txt]
"""
import os, sys, statistics, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import augment_tools as AT
from critic_vae_amd import episodes as E
from critic_vae_amd.augment import Augment
from critic_vae_amd.critic import Critic
from critic_vae_amd.critic_train import CriticTrainer, initial_state_dict
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
dev = torch.device("cuda:0")
N, REPS, W = 20, 7, 64
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def events(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        f()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / N * 1e3          # us per call


def alternate(variants):
    for _, f in variants:
        f(); f(); f()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in variants}
    for _ in range(REPS):
        for name, f in variants:
            t[name].append(events(f))
    return t


def gathers(kind, B, n_frames):
    rng = np.random.default_rng(B)
    gen = torch.Generator(device=dev); gen.manual_seed(B)
    h = Handle(W, B)
    if kind == "uint8":
        frames = torch.randint(0, 256, (n_frames, W, W, 3), dtype=torch.uint8, device=dev, generator=gen)
        ds = E.DeviceDataset(frames, torch.rand(n_frames, 1, device=dev, generator=gen), np.zeros((n_frames, 2), np.int64))
        aug = Augment(flip=0.5, shift=4, brightness=0.2, seed=1)
    else:
        frames = torch.rand(n_frames, 3, W, W, device=dev, generator=gen) * 2 - 1
        ds = E.ReconDataset(frames, torch.rand(n_frames, 1, device=dev, generator=gen), np.zeros((n_frames, 3), np.int64))
        aug = Augment(flip=0.5, shift=4, seed=1)
    idx_host = rng.integers(0, n_frames, size=B)
    idx = torch.from_numpy(idx_host).to(dev)
    x, pred, tmp = torch.empty(B, 3, W, W, device=dev), torch.empty(B, 1, device=dev), torch.empty(B, 3, W, W, device=dev)
    applied = torch.from_numpy(aug.draws(0, idx_host)).to(dev)
    rows, cols = AT.index_maps(applied, W)
    bi, ci = torch.arange(B, device=dev)[:, None, None, None], torch.arange(3, device=dev)[None, :, None, None]
    ri, co, g = rows[:, None, :, None], cols[:, None, None, :], AT.gains(applied)[:, None, None, None]
    one = torch.ones((), device=dev)
    at = aug.at(0)

    def plain():
        ds.gather(h, B, idx, x, pred)

    def augmented():
        ds.gather(h, B, idx, x, pred, aug=at)

    def torch_route():
        ds.gather(h, B, idx, tmp, pred)
        if kind == "uint8":
            torch.minimum(tmp[bi, ci, ri, co] * g, one, out=x)
        else:
            x.copy_(tmp[bi, ci, ri, co])

    augmented()
    kernel_x = x.clone()
    torch_route()
    same = torch.equal(x.view(torch.int32), kernel_x.view(torch.int32))
    t = alternate([("plain gather", plain), ("plain gather again", plain), ("augmented gather", augmented), ("torch route", torch_route)])
    base = statistics.median(t["plain gather"])
    both = t["plain gather"] + t["plain gather again"]
    say(f"{kind}, W = {W}, B = {B} ({aug!r}; x is {x.numel() * 4 / 1e6:.1f} MB; the two routes give the same bits: {same}): "
        f"plain gather median {base:.1f} us, its own repeats span {min(both):.1f} .. {max(both):.1f} us")
    for name in t:
        m = statistics.median(t[name])
        say(f"  {name}: {' '.join(f'{v:.1f}' for v in t[name])} us, median {m:.1f} us ({m - base:+.1f} us, x{m / base:.2f} against the plain gather)")
    a, r = statistics.median(t["augmented gather"]), statistics.median(t["torch route"])
    say(f"  augmented gather against the torch route: {a:.1f} us against {r:.1f} us (x{r / a:.2f})")


def epochs(name, make, ds, B, aug):
    """make(augment) -> (trainer, fit); fit() runs one epoch.  With and without, alternating, 3 times each after a warm-up."""
    runs = {"plain": make(None), "augmented": make(aug)}
    t = {k: [] for k in runs}
    for rep in range(4):
        for k, (tr, fit) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit()
            torch.cuda.synchronize()
            if rep:                                # the first epoch of each warms up
                t[k].append((time.perf_counter() - t0) * 1e3)
    steps = (len(ds) + B - 1) // B
    p, a = statistics.median(t["plain"]), statistics.median(t["augmented"])
    say(f"{name}, one fit_device epoch of {len(ds)} frames at B = {B} ({steps} steps), {aug!r}:")
    for k in t:
        m = statistics.median(t[k])
        say(f"  {k}: {' '.join(f'{v:.1f}' for v in t[k])} ms, median {m:.1f} ms = {m / steps * 1e3:.1f} us per step")
    say(f"  augmented - plain: {a - p:+.1f} ms per epoch = {(a - p) / steps * 1e3:+.1f} us per step ({(a / p - 1) * 100:+.2f} %)")


gathers("uint8", 256, 8192)
gathers("uint8", 2048, 8192)
gathers("fp32", 2048, 4096)

pool = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))["u8"]
rep = np.resize(np.arange(len(pool)), 50000)
frames = torch.from_numpy(pool).to(dev)[torch.from_numpy(rep).to(dev)].contiguous()
gen = torch.Generator(device=dev); gen.manual_seed(0)
ds = E.DeviceDataset(frames, torch.rand(50000, 1, device=dev, generator=gen), np.stack([np.zeros(50000, np.int64), rep], 1))
full = Augment(flip=0.5, shift=4, brightness=0.2, seed=1)
np.random.seed(0)


def vae_maker(precision, B):
    def make(augment):
        vae = VariationalAutoencoder(max_batch=B, seed=0, precision=precision).to(dev)
        tr = FusedTrainer(vae, augment=augment)
        return tr, lambda: tr.fit_device(ds, B, epochs=1, generator=gen)
    return make


def critic_maker(B):
    def make(augment):
        critic = Critic(handle=Handle(64, B)).to(dev)
        critic.load_state_dict(initial_state_dict(0))
        tr = CriticTrainer(critic, augment=augment)
        return tr, lambda: tr.fit_device(ds, B, epochs=1, generator=gen)
    return make


epochs("FusedTrainer fp32", vae_maker("f32", 256), ds, 256, full)
epochs("FusedTrainer bf16 mode", vae_maker("bf16", 2048), ds, 2048, full)
epochs("CriticTrainer", critic_maker(128), ds, 128, full)
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    f.write("\n".join(lines) + "\n")
