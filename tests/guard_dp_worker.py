"""2-rank worker for tests/test_gpu_guard.py::test_two_rank_guarded_step (both ranks on device 0, gloo carrying the collectives,
as tests/dp_gpu_worker.py).  Rank 0 steps on the reference's 68 real frames, rank 1 on 68 synthetic ones, both from the seed-0
weights: rank 0's gradient is NaN, the summing all-reduce hands the NaN to rank 1, and the guard — which reads the REDUCED
gradient — must take the same decision on both ranks: skip, every bit of both replicas kept.  A finite step follows."""
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

world, rank, local = dp.init()
assert world == 2
dev = torch.device("cuda", dp.device_index(local))
torch.cuda.set_device(dev)

fx = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))
B, WSEED = int(fx["batch"]), int(fx["wseed"])
assert B == 68


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def synthetic(step, first):
    return tuple(torch.from_numpy(a).to(dev) for a in synth.make_batch(1234, step, B, first_index=first))


def real_frames():
    x = (torch.from_numpy(fx["u8"]).to(torch.float32) / 255.0).permute(0, 3, 1, 2).contiguous().to(dev)
    pred = torch.from_numpy(fx["pred"]).reshape(B, 1).float().contiguous().to(dev)
    eps = torch.from_numpy(synth.make_batch(int(fx["dseed"]), int(fx["step"]), B)[2]).to(dev)
    return x, pred, eps


def model():
    return VariationalAutoencoder(max_batch=B, seed=WSEED).to(dev)


def same_on_both_ranks(t, what):
    other = t.clone()
    dist.broadcast(other, src=0)
    assert torch.equal(bits(other), bits(t)), f"{what}: the ranks differ"


first_batch = real_frames() if rank == 0 else synthetic(0, B)
second_batch = synthetic(1, 2 * B + rank * B)             # finite on both ranks, different rows on each

# the premise, with single-rank trainers: rank 0's own gradient is non-finite, rank 1's is finite
tr = FusedTrainer(model())
tr.step(*first_batch)
finite = bool(torch.isfinite(tr.grads).all())
assert finite == (rank == 1), f"rank {rank}: gradient finite = {finite}"
seen = torch.tensor([int(finite)], device=dev)
dist.all_reduce(seen)
assert seen.item() == 1                                   # exactly one rank holds a finite gradient
del tr

for kw in (dict(overlap=True), dict(overlap=False), dict(overlap=True, reduce_dtype="bf16")):
    # unguarded, today: one rank's NaN reaches every replica
    vae = model()
    start = vae.theta.data.clone()
    FusedTrainer(vae, world_size=world, **kw).step(*first_batch)
    assert torch.isnan(vae.theta.data).any(), f"rank {rank} {kw}: the unguarded replica should be NaN"
    # guarded: both ranks skip
    vae = model()
    tr = FusedTrainer(vae, world_size=world, skip_nonfinite=True, **kw)
    assert tr.overlap == kw["overlap"] and torch.equal(bits(vae.theta.data), bits(start))
    tr.step(*first_batch)
    torch.cuda.synchronize()
    assert not torch.isfinite(tr.grads).all(), f"rank {rank} {kw}: the reduced gradient carries rank 0's NaN"
    assert torch.equal(bits(vae.theta.data), bits(start)), f"rank {rank} {kw}: theta moved in a skipped step"
    assert not tr.m.any() and not tr.v.any()
    st = tr.guard_stats()
    assert (st["applied"], st["skipped"]) == (0, 1), (rank, kw, st)
    # a finite step: applied on both ranks, the replicas stay bit-identical
    tr.step(*second_batch)
    torch.cuda.synchronize()
    st = tr.guard_stats()
    assert (st["applied"], st["skipped"]) == (1, 1), (rank, kw, st)
    assert torch.isfinite(vae.theta.data).all() and not torch.equal(vae.theta.data, start)
    for t, what in ((vae.theta.data, "theta"), (tr.m, "m"), (tr.v, "v")):
        same_on_both_ranks(t, f"{kw} {what}")
    # sync_replicas carries the guard counters: a rank restored elsewhere takes rank 0's
    if rank == 1:
        tr.load_state_dict(dict(tr.state_dict(), applied=7, skipped=3))
    tr.sync_replicas()
    st = tr.guard_stats()
    assert (st["applied"], st["skipped"]) == (1, 1), (rank, kw, st)
print(f"GUARD_DP_OK rank {rank}", flush=True)
dist.destroy_process_group()
