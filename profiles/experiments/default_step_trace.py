"""Three default-argument FusedTrainer steps in each of the four precisions (B = 64) of the source tree given as argv[1]: the
workload of a kernel trace that shows which kernels the default step launches, on this tree and on a built checkout of
its parent.  Prints the SHA-256 of the parameter buffer after the three steps, per precision: equal digests = the same bits.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_A -- python profiles/experiments/default_step_trace.py .
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT_B -- python profiles/experiments/default_step_trace.py PARENT_TREE
    python profiles/experiments/kernel_list_compare.py OUT_B OUT_A
"""
import hashlib, os, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch
import critic_vae_amd
from critic_vae_amd import synth
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
assert os.path.abspath(critic_vae_amd.__file__).startswith(root), critic_vae_amd.__file__
dev = torch.device("cuda:0")
B = 64
for prec in ("f32", "bf16", "bf16x9", "bf16x6"):
    vae = VariationalAutoencoder(max_batch=B, seed=0, precision=prec).to(dev)
    tr = FusedTrainer(vae)
    for s in range(3):
        x, pred, eps = (torch.from_numpy(a).to(dev) for a in synth.make_batch(1234, s, B))
        tr.step(x, pred, eps)
    torch.cuda.synchronize()
    print(prec, "theta sha256", hashlib.sha256(vae.theta.data.cpu().numpy().tobytes()).hexdigest())
