"""A digest of one small critic training run, to show that a change of csrc/critic_train.hip (here: its device functions moved
to critic_bwd.h) leaves the trained bits alone: CriticTrainer.fit_device on the 68 real frames of step_real_b68.npz with
seeded targets, weights from initial_state_dict(0), batch 37 (two ragged batches per epoch), 2 epochs, Dropout 0.3 with a
seeded generator, shuffling from a seeded numpy.  Prints the SHA-256 of the final 11 873 parameters and of the loss rows.
Run it on both builds (ROOT = the checkout whose package and library are used; the fixtures are this checkout's):

    python profiles/experiments/critic_train_identity.py [ROOT]
"""
import hashlib, os, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
sys.path.insert(0, ROOT)
from critic_vae_amd.critic import Critic
from critic_vae_amd.critic_train import CriticTrainer, initial_state_dict
from critic_vae_amd.episodes import DeviceDataset
from critic_vae_amd.lib import Handle, LIB_PATH
dev = torch.device("cuda:0")
u8 = np.load(os.path.join(HERE, "tests", "golden", "step_real_b68.npz"))["u8"]
rng = np.random.default_rng(20261020)
targets = torch.from_numpy(rng.random((68, 1)).astype(np.float32)).to(dev)
ds = DeviceDataset(torch.from_numpy(u8).to(dev).contiguous(), targets, np.stack([np.zeros(68, np.int64), np.arange(68)], 1))
critic = Critic(handle=Handle(64, 64)).to(dev)
critic.load_state_dict(initial_state_dict(seed=0))
np.random.seed(7)
gen = torch.Generator(device=dev)
gen.manual_seed(11)
log = CriticTrainer(critic, dropout=0.3).fit_device(ds, 37, epochs=2, generator=gen)
torch.cuda.synchronize()
flat, rows = critic.flat.cpu().numpy(), log.cpu().numpy()
assert os.path.dirname(os.path.dirname(LIB_PATH)) == ROOT and np.isfinite(flat).all() and rows.shape == (4, 4)
print(f"steps {rows.shape[0]}  losses {rows[:, 0].tolist()}")
print(f"params sha256 {hashlib.sha256(flat.tobytes()).hexdigest()}")
print(f"losses sha256 {hashlib.sha256(rows.tobytes()).hexdigest()}")
