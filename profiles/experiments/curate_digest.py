"""SHA-256 of what curate() and curate_recon() build on the workload of recon_build_rate.py (16 shuffled copies of the fixture
trajectories, no cut), one line per array.  Run from any built checkout of the project: the digests of two trees that build
the same datasets are equal.

    PYTHONPATH=TREE python profiles/experiments/curate_digest.py TREE
"""
import hashlib, os, sys
import numpy as np, torch
ROOT = os.path.abspath(sys.argv[1])
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
for c in range(16):
    for t, n in enumerate(ep["traj_names"].tolist()):
        episodes.append((f"{n}_{c:02d}", pool[rng.permutation(ep["traj_idx"][offs[t]:offs[t + 1]])]))
vae = VariationalAutoencoder(max_batch=256, seed=7).to(dev); vae.load_reference_params(first_vae_params(7)); vae.eval()
for name, ds in (("curate", E.curate(episodes, critic, total_images=10 ** 9, log=lambda s: None)),
                 ("curate_recon", E.curate_recon(episodes, critic, vae, total_images=10 ** 9, log=lambda s: None))):
    for what, a in (("frames", ds.frames.cpu().numpy()), ("preds", ds.preds.cpu().numpy()), ("source", ds.source),
                    ("sizes", np.asarray(ds.sizes, np.int64))):
        print(f"digest {name}.{what} {a.shape} {hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}", flush=True)
