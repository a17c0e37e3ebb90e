"""2-rank worker for tests/test_gpu_sync_stats.py: FusedTrainer(global_stats=True) on the two halves of the rows of
tests/golden/trajectory_b32.npz (both ranks on device 0, gloo carrying the collectives), with the bucketed all-reduce
overlapped with backward and with the single all-reduce.  The per-step scalars are the global batch's and meet the bounds
of test_trajectory_config1_fused_trainer; afterwards both ranks hold bitwise identical parameters, BatchNorm running
statistics and Adam state."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from critic_vae_amd import dp, synth                      # noqa: E402
from critic_vae_amd.nets import VariationalAutoencoder    # noqa: E402
from critic_vae_amd.train import FusedTrainer             # noqa: E402

TOL = 1e-4
world, rank, local = dp.init()
assert world == 2
dev = torch.device("cuda", dp.device_index(local))
torch.cuda.set_device(dev)
fx = np.load(os.path.join(ROOT, "tests", "golden", "trajectory_b32.npz"))
GLOBAL_B = int(fx["batch"])
first, per = dp.shard_rows(GLOBAL_B, world, rank)
steps = int(fx["n_frames"]) // GLOBAL_B

finals = {}
for overlap in (True, False):
    vae = VariationalAutoencoder(max_batch=per, seed=0).to(dev)
    vae.load_reference_params(synth.make_params(int(fx["wseed"])))
    tr = FusedTrainer(vae, world_size=world, overlap=overlap, global_stats=True)
    assert tr.overlap == overlap and tr.global_stats
    got = []
    for s in range(steps):
        x, pred, eps = (torch.from_numpy(a).to(dev) for a in synth.make_batch(int(fx["dseed"]), s, per, first_index=first))
        got.append(tr.step(x, pred, eps)[:3].cpu().numpy().copy())
    got = np.array(got)
    err2, err = np.abs(got[:2] - fx["traj"][:2]).max(), np.abs(got - fx["traj"]).max()
    assert np.isfinite(got).all(), overlap
    assert err2 < TOL, (overlap, err2)                                   # before Adam noise can amplify
    assert err < 5e-3, (overlap, err)
    assert got[-1, 0] < 0.5 * got[0, 0], overlap                        # it trains
    torch.cuda.synchronize()
    for name, t in (("theta", vae.theta.data), ("bn_state", vae.bn_state), ("exp_avg", tr.m), ("exp_avg_sq", tr.v)):
        other = t.clone()
        dist.broadcast(other, src=0)
        assert torch.equal(other, t), f"ranks differ in {name} (overlap={overlap})"
    finals[overlap] = (vae.theta.data.clone(), err2, err)
    if rank == 0:
        print(f"overlap={overlap}: |traj - reference| first two steps {err2:.2e}, all {err:.2e}", flush=True)
assert torch.equal(finals[True][0], finals[False][0]), "bucketed and single all-reduce differ"
print(f"SYNC_GPU_OK rank {rank}", flush=True)
dist.destroy_process_group()
