"""Three default-argument steps and one fit_device epoch of a FusedTrainer (f32) and of a CriticTrainer (B = 64, 64 frames), of
the source tree given as argv[1]: the workload of a kernel trace that shows the default trainers launch what they launched
before the optimizer options existed, on this tree and on a built checkout of its parent.  With a third argument `optim` both
trainers run under Optim(weight_decay=0.01, ema=0.999): the launch count of a step stays, the _opt kernel stands where the plain
one stood.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_A -- python profiles/experiments/optim_trace.py .
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_B -- python profiles/experiments/optim_trace.py PARENT_TREE
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_C -- python profiles/experiments/optim_trace.py . optim
    python profiles/experiments/kernel_list_compare.py OUT_B OUT_A
"""
import os, sys
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
kw = {}
if len(sys.argv) > 2 and sys.argv[2] == "optim":
    from critic_vae_amd.optim import Optim
    kw = dict(optim=Optim(weight_decay=0.01, ema=0.999))
dev = torch.device("cuda:0")
B = 64
x, pred, _ = synth.make_batch(1234, 0, B)
u8 = np.ascontiguousarray(np.rint(x * 255.0).astype(np.uint8).transpose(0, 2, 3, 1))
ds = DeviceDataset(torch.from_numpy(u8).to(dev), torch.from_numpy(pred.reshape(B, 1).copy()).to(dev),
                   np.stack([np.zeros(B, np.int64), np.arange(B, dtype=np.int64)], 1))
gen = torch.Generator(device=dev)

vae = VariationalAutoencoder(max_batch=B, seed=0).to(dev)
tr = FusedTrainer(vae, **kw)
for s in range(3):
    tr.step(*(torch.from_numpy(a).to(dev) for a in synth.make_batch(1234, s, B)))
gen.manual_seed(0)
np.random.seed(0)
tr.fit_device(ds, 16, epochs=1, generator=gen)
print("vae steps", tr.step_count, "theta sum", vae.theta.data.double().sum().item())

critic = Critic(handle=Handle(64, B)).to(dev)
critic.load_state_dict(initial_state_dict(0))
ct = CriticTrainer(critic, **kw)
gen.manual_seed(0)
for s in range(3):
    xb, target, _ = synth.make_batch(1234, s, B)
    ct.step(torch.from_numpy(xb).to(dev), torch.from_numpy(target).to(dev), generator=gen)
ct.fit_device(ds, 16, epochs=1, generator=gen)
print("critic steps", ct.step_count, "theta sum", ct.theta.double().sum().item())
