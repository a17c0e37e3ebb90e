"""curate_recon against a baseline written from the parent commit's public calls, same episodes, same process, alternating.

    python profiles/experiments/recon_build_rate.py [OUT.txt]
"""
import os, sys, time, statistics
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from critic_vae_amd import episodes as E
from critic_vae_amd.critic import Critic
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
from recon_tools import first_vae_params
dev = torch.device("cuda:0")
G = os.path.join(ROOT, "tests", "golden")
ep = np.load(os.path.join(G, "episodes_real.npz")); pool = np.load(os.path.join(G, "step_real_b68.npz"))["u8"]
cw = np.load(os.path.join(G, "critic_real_b8.npz"))
critic = Critic(handle=Handle(64, 1024)).to(dev)
critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
offs = np.concatenate([[0], np.cumsum(ep["traj_len"])])
rng = np.random.default_rng(0)
episodes = []
for c in range(16):                                   # 16 shuffled copies of the fixture's trajectories: 58 752 walked frames
    for t, n in enumerate(ep["traj_names"].tolist()):
        s = ep["traj_idx"][offs[t]:offs[t + 1]]
        episodes.append((f"{n}_{c:02d}", pool[rng.permutation(s)]))
TOTAL = 10 ** 9
vae = VariationalAutoencoder(max_batch=256, seed=7).to(dev); vae.load_reference_params(first_vae_params(7)); vae.eval()
quiet = lambda s: None

def baseline():
    """critic pass as curate() makes it, the selection in Python, vae.diff_images on every selected frame, torch indexing."""
    names = E.reference_order([n for n, _ in episodes]); by = dict(episodes)
    h = Handle(64, 1024); x = torch.empty(1024, 3, 64, 64, device=dev)
    frames, vals = [], []
    for n in names:
        a = by[n]
        if a.shape[0] == 0:
            frames.append(None); vals.append(np.zeros(0, np.float32)); continue
        d = torch.from_numpy(np.ascontiguousarray(a)).to(dev); p = torch.empty(a.shape[0], device=dev)
        E._critic_values(critic, d, p, handle=h, x=x)
        frames.append(d); vals.append(p.cpu().numpy())
    _, ent, _ = E.select_recon_host(vals, total_images=TOTAL)
    buf = torch.empty(len(ent), 3, 64, 64, device=dev)
    sel = {}
    for e, (t, i, k) in enumerate(ent):
        sel.setdefault((t, i), []).append((e, k))
    keys = list(sel)
    xb = torch.empty(256, 3, 64, 64, device=dev)
    for p0 in range(0, len(keys), 256):
        ks = keys[p0:p0 + 256]; nb = len(ks)
        u8 = torch.stack([frames[t][i] for t, i in ks])
        vae.handle.preprocess_u8(nb, u8, xb[:nb])
        pr = torch.tensor([vals[t][i] for t, i in ks], device=dev).view(nb, 1)
        one, zero, _, _ = vae.diff_images(xb[:nb], pr)
        both = torch.stack([one, zero], 1)
        rows = [(b, k, e) for b, key in enumerate(ks) for e, k in sel[key]]
        rb, rk, re_ = (torch.tensor(v, device=dev) for v in zip(*rows))
        buf[re_] = both[rb, rk]
    preds = torch.empty(len(ent), 1, device=dev)
    for p0 in range(0, len(ent), 1024):
        nb = min(1024, len(ent) - p0)
        h.critic_forward(nb, buf[p0:p0 + nb], critic.flat, preds[p0:p0 + nb])
    torch.cuda.synchronize()
    return buf, preds

def timed(f):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = f(); torch.cuda.synchronize(); return time.perf_counter() - t0, r

new = lambda: E.curate_recon(episodes, critic, vae, total_images=TOTAL, log=quiet)
plain = lambda: E.curate(episodes, critic, total_images=TOTAL, log=quiet)
timed(new); timed(baseline); timed(plain)            # warm-up
T = {"curate_recon": [], "baseline": [], "curate": []}
for _ in range(5):
    t, ds = timed(new); T["curate_recon"].append(t)
    t, (buf, bp) = timed(baseline); T["baseline"].append(t)
    t, pd = timed(plain); T["curate"].append(t)
same = torch.equal(ds.frames.view(torch.int32), buf.view(torch.int32))
walked = sum(a.shape[0] for _, a in episodes)
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in [f"{walked} walked frames, {len(ds)} entries from {ds.stats['encoded']} selected frames ({len(pd)} frames in the plain walk); baseline entries bitwise equal: {same}"] + \
            [f"{k}: runs {' '.join(f'{x * 1e3:.1f}' for x in v)} ms; median {statistics.median(v) * 1e3:.1f} ms = "
             f"{(len(pd) if k == 'curate' else len(ds)) / statistics.median(v):.0f} {'frames' if k == 'curate' else 'entries'}/s, {walked / statistics.median(v):.0f} walked frames/s"
             for k, v in T.items()]:
        print(line, flush=True); f.write(line + "\n")
