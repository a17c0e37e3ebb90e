"""Small fits of both trainers with fixed seeds, of the source tree given as argv[1]: sha256 of everything a fit leaves
behind.  Uses only what exists before and after the trainers got their shared base (fit.py), so the output of this tree
and of a built checkout of its parent can be compared byte for byte (each in a process of its own):

    python profiles/experiments/fit_refactor_compare.py . > this.txt
    python profiles/experiments/fit_refactor_compare.py PARENT_TREE > parent.txt && cmp parent.txt this.txt

FusedTrainer: f32 and bf16 mode, guarded and not, 40 synthetic 64x64 frames at B = 16 (ragged last batch of 8), 2 epochs,
12 held-out frames evaluated every 2 steps.  CriticTrainer: guarded and not, 60 frames at B = 32, 2 epochs, 20 held-out
frames evaluated once per epoch.
"""
import hashlib, os, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import critic_vae_amd
from critic_vae_amd import synth
from critic_vae_amd.critic import Critic
from critic_vae_amd.critic_train import CriticTrainer, initial_state_dict
from critic_vae_amd.episodes import DeviceDataset
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
assert os.path.abspath(critic_vae_amd.__file__).startswith(root), critic_vae_amd.__file__
dev = torch.device("cuda:0")
GUARD = dict(skip_nonfinite=True, max_grad_norm=1.0)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def dataset(lo, hi, preds, traj):
    x, _, _ = synth.make_batch(1234, 0, hi)
    u8 = np.ascontiguousarray(np.rint(x[lo:hi] * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))
    source = np.stack([np.full(hi - lo, traj, np.int64), np.arange(hi - lo, dtype=np.int64)], 1)
    return DeviceDataset(torch.from_numpy(u8).to(dev), torch.from_numpy(preds[lo:hi].reshape(-1, 1).copy()).to(dev), source)


def report(name, tr, tensors, returned):
    for k, t in tensors:
        print(f"{name} {k} {sha(t)}")
    print(f"{name} returned {tuple(returned.shape)} {sha(returned)}")
    print(f"{name} val_history {tr.val_history!r}")
    print(f"{name} best_val {tr.best_val!r} val_stale {tr.val_stale!r} step_count {tr.step_count}")
    print(f"{name} guard_stats {tr.guard_stats() if tr.guarded else None!r}")


def seeded():
    torch.manual_seed(0)
    np.random.seed(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    return gen


preds = np.random.default_rng(7).random(80, dtype=np.float32)
for prec in ("f32", "bf16"):
    for guarded in (False, True):
        gen = seeded()
        vae = VariationalAutoencoder(max_batch=16, seed=0, precision=prec).to(dev)
        tr = FusedTrainer(vae, **(GUARD if guarded else {}))
        scal = tr.fit_device(dataset(0, 40, preds, 0), 16, epochs=2, generator=gen, val=dataset(40, 52, preds, 1), val_every=2)
        torch.cuda.synchronize()
        report(f"vae {prec} {'guarded' if guarded else 'plain'}", tr,
               [("theta", vae.theta.data), ("m", tr.m), ("v", tr.v), ("bn_state", vae.bn_state)], scal)
for guarded in (False, True):
    gen = seeded()
    critic = Critic(handle=Handle(64, 32)).to(dev)
    critic.load_state_dict(initial_state_dict(0))
    tr = CriticTrainer(critic, **(GUARD if guarded else {}))
    log = tr.fit_device(dataset(0, 60, preds, 0), 32, epochs=2, generator=gen, val=dataset(60, 80, preds, 1))
    torch.cuda.synchronize()
    report(f"critic {'guarded' if guarded else 'plain'}", tr, [("theta", tr.theta), ("m", tr.m), ("v", tr.v)], log)
