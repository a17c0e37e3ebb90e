"""2-rank worker for tests/test_gpu_optim.py (both ranks on device 0, gloo carrying the collectives, as tests/dp_gpu_worker.py
does): a data-parallel FusedTrainer under an Optim with an EMA, on the real frames of step_real_b68.npz (noise frames go NaN).
Rank 1 is built from another seed; after sync_replicas and two steps it holds rank 0's parameters, Adam moments and averaged
weights bit for bit — also when rank 0 alone came out of a checkpoint with averages of its own.

The BatchNorm running statistics, and with them `aux_ema`, are compared only right after sync_replicas: without global_stats
every rank's forward writes bn_state from its OWN shard and nothing reduces it, so they differ from the first step on, as they
do without an Optim."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from critic_vae_amd import dp                             # noqa: E402
from critic_vae_amd.nets import VariationalAutoencoder    # noqa: E402
from critic_vae_amd.optim import Optim                    # noqa: E402
from critic_vae_amd.train import FusedTrainer             # noqa: E402
from test_oracle import real_frames_params                # noqa: E402

world, rank, local = dp.init()
assert world == 2
dev = torch.device("cuda", dp.device_index(local))
torch.cuda.set_device(dev)
GLOBAL_B = 8
first, per = dp.shard_rows(GLOBAL_B, world, rank)
OPT = dict(schedule="linear", warmup=1, total=8, weight_decay=0.05, ema=0.9)
fx = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))


def batch(step):
    lo = step * GLOBAL_B + first
    x = torch.from_numpy(fx["u8"][lo:lo + per].copy()).permute(0, 3, 1, 2).float().div(255.0).contiguous()
    pred = torch.from_numpy(fx["pred"][lo:lo + per].copy()).float().reshape(per, 1)
    eps = torch.randn(per, 32, generator=torch.Generator().manual_seed(100 + lo))
    return x.to(dev), pred.to(dev), eps.to(dev)


def model(seed):
    """Rank 0: the weights the real-frames fixtures train from; rank 1: fresh ones from another seed."""
    vae = VariationalAutoencoder(max_batch=per, seed=seed + rank).to(dev)
    if rank == 0:
        vae.load_reference_params(real_frames_params(fx))
    return vae


def same_as_rank0(t, what):
    r0 = t.clone()
    dist.broadcast(r0, src=0)
    assert torch.equal(r0.view(torch.int32), t.view(torch.int32)), f"{what} differs from rank 0's"


def check(tr, tag, statistics=False):
    names = [("theta", tr.vae.theta.data), ("exp_avg", tr.m), ("exp_avg_sq", tr.v), ("ema", tr.ema)]
    if statistics:
        names += [("bn_state", tr.vae.bn_state), ("aux_ema", tr.aux_ema)]
    for name, t in names:
        same_as_rank0(t, f"{tag}: {name}")
    assert torch.isfinite(tr.vae.theta.data).all() and torch.isfinite(tr.ema).all(), f"{tag}: the run went non-finite"


# replicas from different weights: no rank has averages yet, every rank starts its own from the broadcast parameters
vae = model(100)
before = vae.theta.data.clone()
tr = FusedTrainer(vae, world_size=world, optim=Optim(**OPT))
assert tr.ema is None and tr.aux_ema is None
assert rank == 0 or not torch.equal(before, vae.theta.data)
for s in range(2):
    tr.step(*batch(s))
torch.cuda.synchronize()
assert tr.ema is not None and tr.aux_ema is not None and not torch.equal(tr.ema, vae.theta.data)
check(tr, "fresh")

# rank 0 alone carries averages (a restored checkpoint): sync_replicas hands them to rank 1, statistics included
vae2 = model(200)
tr2 = FusedTrainer(vae2, world_size=world, optim=Optim(**OPT), sync=False)
if rank == 0:
    vae2.theta.data.copy_(vae.theta.data)
    vae2.bn_state.copy_(vae.bn_state)
    tr2.load_state_dict(tr.state_dict())
    assert tr2.ema is not None
else:
    assert tr2.ema is None
tr2.sync_replicas()
assert tr2.step_count == 2 and tr2.ema is not None and tr2.aux_ema is not None
check(tr2, "after sync_replicas", statistics=True)
for s in range(2, 4):
    tr2.step(*batch(s))
torch.cuda.synchronize()
check(tr2, "restored")
assert not torch.equal(tr2.ema, tr2.vae.theta.data)
print(f"OPTIM_DP_OK rank {rank}", flush=True)
dist.destroy_process_group()
