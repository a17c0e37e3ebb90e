"""Three default-argument CriticTrainer steps (B = 64) of the source tree given as argv[1]: the workload of a kernel trace
that shows which kernels the critic's default step launches, on this tree and on a built checkout of its parent.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_A -- python profiles/experiments/critic_step_trace.py .
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_B -- python profiles/experiments/critic_step_trace.py PARENT_TREE
    python profiles/experiments/kernel_list_compare.py OUT_B OUT_A
"""
import os, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import critic_vae_amd
from critic_vae_amd.critic import Critic
from critic_vae_amd.critic_train import CriticTrainer, initial_state_dict
from critic_vae_amd.lib import Handle
assert os.path.abspath(critic_vae_amd.__file__).startswith(root), critic_vae_amd.__file__
dev = torch.device("cuda:0")
B = 64
critic = Critic(handle=Handle(64, B)).to(dev)
critic.load_state_dict(initial_state_dict(0))
tr = CriticTrainer(critic)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
rng = np.random.default_rng(0)
for s in range(3):
    x = torch.from_numpy(rng.random((B, 3, 64, 64), dtype=np.float32)).to(dev)
    target = torch.from_numpy(rng.random(B, dtype=np.float32)).to(dev)
    tr.step(x, target, generator=gen)
torch.cuda.synchronize()
print("theta sum", tr.theta.double().sum().item())
