"""Global-batch data parallelism on the GPU: the staged step (include/cvae.h, cvae_*_stage) with the fp64 BatchNorm and loss
sums exchanged between ranks.  One rank without an exchange reproduces the single-call step bit for bit; ranks emulated in
one process (their records summed in rank order, as an all-reduce would) reproduce the reference at the GLOBAL batch; two
real processes (torchrun, gloo) train identical replicas with FusedTrainer(global_stats=True)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from critic_vae_amd import layout as L
from critic_vae_amd import synth
from critic_vae_amd.lib import SYNC_DOUBLES, sync_slot
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
from decisions import is_pre_bn_bias

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
DEV = torch.device("cuda:0")


def _rank(B, width=64, precision="f32", overlap=False, wseed=0):
    vae = VariationalAutoencoder(max_batch=B, seed=wseed, width=width, precision=precision, overlap_wgrad=overlap).to(DEV)
    vae.load_reference_params(synth.make_params(wseed, width))
    return FusedTrainer(vae)


def _batch(dseed, step, n, width=64, first=0):
    return tuple(torch.from_numpy(a).to(DEV) for a in synth.make_batch(dseed, step, n, width, first_index=first))


def _fused(tr, x, pred, eps):
    """cvae_forward + cvae_loss + cvae_backward (no optimizer step)."""
    v, h, B = tr.vae, tr.h, x.shape[0]
    h.forward(B, x, pred, eps, v.theta.data, v.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=True)
    h.loss(B, x, tr.mu, tr.logvar, tr.recon, tr.ws, tr.scalars, tr.d_recon, tr.d_mu, tr.d_logvar)
    h.backward(B, x, pred, eps, v.theta.data, tr.logvar, tr.recon, tr.d_recon, tr.d_mu, tr.d_logvar, tr.ws, tr.grads)


def _staged(trs, batches, exchange=True):
    """Every rank's staged step, stage by stage; between stages each sync slot is summed over the ranks' records in rank
    order and written back to every record (what an all-reduce does).  exchange=False: no exchange at all."""
    recs = [torch.full((SYNC_DOUBLES,), float("nan"), dtype=torch.float64, device=DEV) for _ in trs]

    def ex(point):
        if not exchange:
            return
        off, n = sync_slot(point)
        tot = recs[0][off:off + n].clone()
        for r in recs[1:]:
            tot += r[off:off + n]
        for r in recs:
            r[off:off + n].copy_(tot)

    args = []
    for tr, (x, pred, eps) in zip(trs, batches):
        args.append((tr, tr.h, x.shape[0], x, pred, eps, tr.vae.theta.data))
    for k in range(5):
        for (tr, h, B, x, pred, eps, th), rec in zip(args, recs):
            h.forward_stage(k, B, x, pred, eps, th, tr.vae.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, rec)
        if k < 4:
            ex(k)
    for k in range(2):
        for (tr, h, B, x, pred, eps, th), rec in zip(args, recs):
            h.loss_stage(k, B, x, tr.mu, tr.logvar, tr.recon, tr.ws, tr.scalars, tr.d_recon, tr.d_mu, tr.d_logvar, rec)
        if k == 0:
            ex(4)
    for k in range(5):
        for (tr, h, B, x, pred, eps, th), rec in zip(args, recs):
            h.backward_stage(k, B, x, pred, eps, th, tr.logvar, tr.recon, tr.d_recon, tr.d_mu, tr.d_logvar, tr.ws, tr.grads, rec)
        if k < 4:
            ex(5 + k)
    torch.cuda.synchronize()


def _outputs(tr, B):
    return {"mu": tr.mu[:B], "logvar": tr.logvar[:B], "recon": tr.recon[:B], "scalars": tr.scalars,
            "d_recon": tr.d_recon[:B], "d_mu": tr.d_mu[:B], "d_logvar": tr.d_logvar[:B], "grads": tr.grads,
            "bn_state": tr.vae.bn_state}


@pytest.mark.parametrize("precision,width,overlap", [(p, w, False) for w in (64, 128) for p in ("f32", "bf16", "bf16x9", "bf16x6")]
                         + [("f32", 64, True), ("bf16", 64, True)])
def test_one_rank_staged_step_is_bitwise_the_single_call_step(precision, width, overlap):
    B = 6 if width == 64 else 3
    batch = _batch(1234, 1, B, width)
    a, b = _rank(B, width, precision, overlap), _rank(B, width, precision, overlap)
    b.grads.fill_(float("nan"))                   # the stages must write every gradient (the padding stays as it was)
    used = torch.zeros_like(a.grads, dtype=torch.bool)
    for off, n in a.h.layout.values():
        used[off:off + n] = True
    b.grads[~used] = 0.0
    _fused(a, *batch)
    _staged([b], [batch], exchange=False)
    torch.cuda.synchronize()
    oa, ob = _outputs(a, B), _outputs(b, B)
    assert torch.isfinite(oa["scalars"][:3]).all()
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    # a second step on the updated running statistics, and the stages accept a new step after a complete one
    _fused(a, *_batch(1234, 2, B, width))
    _staged([b], [_batch(1234, 2, B, width)], exchange=False)
    oa, ob = _outputs(a, B), _outputs(b, B)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), ("step 2", k)


def test_fused_trainer_global_stats_at_one_rank_equals_the_default_step():
    B = 8
    a, b = _rank(B), _rank(B)
    b = FusedTrainer(b.vae, global_stats=True)
    assert b.global_stats and not a.global_stats
    for s in range(3):
        batch = _batch(1234, s, B)
        sa, sb = a.step(*batch), b.step(*batch)
        torch.cuda.synchronize()
        assert torch.equal(sa, sb), s
    for ta, tb in ((a.vae.theta.data, b.vae.theta.data), (a.vae.bn_state, b.vae.bn_state), (a.m, b.m), (a.v, b.v)):
        assert torch.equal(ta, tb)


def _running_stats(bn_state):
    return {bi: (bn_state[L.BN_OFF[l]:L.BN_OFF[l] + c].cpu().numpy(), bn_state[L.BN_TOTAL + L.BN_OFF[l]:L.BN_TOTAL + L.BN_OFF[l] + c].cpu().numpy())
            for l, (bi, c) in enumerate(zip((1, 5, 9, 13), (32, 64, 128, 256)))}


def test_four_emulated_ranks_reproduce_the_reference_at_the_global_batch(golden_dir):
    fx = np.load(os.path.join(golden_dir, "step_b32.npz"))
    GB, W, R = int(fx["batch"]), int(fx["width"]), 4
    assert GB == 32 and W == 64
    per = GB // R
    shards = [_batch(int(fx["dseed"]), int(fx["step"]), per, W, first=r * per) for r in range(R)]

    def misses(trs, grad):
        """largest deviation from the fixture, over everything test_step_matches_reference_fixture_and_oracle checks"""
        e = {}
        mu = torch.cat([t.mu[:per] for t in trs]).cpu().numpy()
        lv = torch.cat([t.logvar[:per] for t in trs]).cpu().numpy()
        recon = torch.cat([t.recon[:per] for t in trs]).cpu().numpy()
        e["mu"] = np.abs(mu - fx["mu"]).max()
        e["logvar"] = np.abs(lv - fx["logvar"]).max()
        e["recon"] = np.abs(recon.reshape(-1)[::16] - fx["recon_sample"]).max()
        ref = L.native_to_ref(trs[0].h.layout, grad)
        e["grads"] = max(np.abs(ref[k].cpu().numpy().reshape(-1)[fx["grad_idx/" + k]] - fx["grad_val/" + k]).max() for k in ref)
        return e

    # global statistics: every rank's scalars are the global ones, the gradients add up to the global-batch gradient
    trs = [_rank(per) for _ in range(R)]
    _staged(trs, shards)
    g = trs[0].grads.clone()
    for t in trs[1:]:
        g += t.grads
    e = misses(trs, g)
    for k, v in e.items():
        assert v <= TOL, (k, v)
    for t in trs:
        s = t.scalars.cpu().numpy()
        assert np.abs(s[:3] - fx["losses"]).max() < TOL
        assert np.abs(s[3:8] - fx["ssim_levels"]).max() < TOL and np.abs(s[8:13] - fx["cs_levels"]).max() < TOL
        rs = _running_stats(t.vae.bn_state)
        for bi, (m, v) in rs.items():
            assert np.abs(m - fx[f"bn_running_mean/{bi}"]).max() < 1e-5, bi
            assert np.abs(v - fx[f"bn_running_var/{bi}"]).max() < 1e-5, bi
        assert torch.equal(t.vae.bn_state, trs[0].vae.bn_state)
    # teeth: the same shards with today's per-rank semantics (mean of the shard gradients) miss the fixture by far
    local = [_rank(per) for _ in range(R)]
    for t, b in zip(local, shards):
        _fused(t, *b)
    torch.cuda.synchronize()
    g = sum(t.grads for t in local) / R
    e_local = misses(local, g)
    print("global:", {k: f"{v:.2e}" for k, v in e.items()}, "per-rank:", {k: f"{v:.2e}" for k, v in e_local.items()})
    assert max(e_local["mu"], e_local["grads"]) > 100 * TOL, e_local


def _close_rel(got, want, rel):
    return float((got - want).abs().max()) <= rel * float(want.abs().max()) + 1e-30


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_ragged_shards_equal_one_handle_at_their_total_batch(precision):
    sizes, W = (5, 5, 3), 64
    B = sum(sizes)
    firsts = np.cumsum((0,) + sizes[:-1])
    shards = [_batch(1234, 3, n, W, first=int(f)) for n, f in zip(sizes, firsts)]
    whole = _rank(B, W, precision)
    _fused(whole, *_batch(1234, 3, B, W))
    trs = [_rank(n, W, precision) for n in sizes]
    _staged(trs, shards)
    g = trs[0].grads.clone()
    for t in trs[1:]:
        g += t.grads
    got = {"mu": torch.cat([t.mu[:n] for t, n in zip(trs, sizes)]), "logvar": torch.cat([t.logvar[:n] for t, n in zip(trs, sizes)]),
           "recon": torch.cat([t.recon[:n] for t, n in zip(trs, sizes)]),
           "d_mu": torch.cat([t.d_mu[:n] for t, n in zip(trs, sizes)]), "d_logvar": torch.cat([t.d_logvar[:n] for t, n in zip(trs, sizes)])}
    want = {"mu": whole.mu[:B], "logvar": whole.logvar[:B], "recon": whole.recon[:B], "d_mu": whole.d_mu[:B],
            "d_logvar": whole.d_logvar[:B]}
    ref_got, ref_want = L.native_to_ref(whole.h.layout, g), L.native_to_ref(whole.h.layout, whole.grads)
    for t in trs:
        assert torch.equal(t.scalars, trs[0].scalars) and torch.equal(t.vae.bn_state, trs[0].vae.bn_state)
    if precision == "f32":
        for k in want:
            assert _close_rel(got[k], want[k], TOL), k
        for k in ref_want:                   # a conv bias in front of BatchNorm has gradient 0 up to round-off: absolute bound
            if is_pre_bn_bias(k):
                assert float((ref_got[k] - ref_want[k]).abs().max()) <= TOL, k
            else:
                assert _close_rel(ref_got[k], ref_want[k], TOL), k
        assert _close_rel(trs[0].scalars[:13], whole.scalars[:13], TOL)
        assert _close_rel(trs[0].vae.bn_state, whole.vae.bn_state, TOL)
    else:                                  # bf16 mode: the bounds of test_gpu_bf16 (outputs 3e-2, loss 2e-3, cosine 0.995)
        for k in ("mu", "logvar", "recon"):
            assert float((got[k] - want[k]).abs().max()) < 3e-2, k
        assert abs(float(trs[0].scalars[0]) - float(whole.scalars[0])) < 2e-3
        a = torch.cat([ref_got[k].flatten() for k in sorted(ref_want)]).double()
        b = torch.cat([ref_want[k].flatten() for k in sorted(ref_want)]).double()
        cos = float(a @ b / (a.norm() * b.norm()))
        assert cos > 0.995, cos
        assert float((trs[0].vae.bn_state - whole.vae.bn_state).abs().max()) < 3e-2


def test_two_processes_train_identical_replicas_with_global_stats():
    env = dict(os.environ, CVAE_DIST_BACKEND="gloo", CVAE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nnodes=1", "--nproc-per-node=2", os.path.join(ROOT, "tests", "sync_gpu_worker.py")],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "SYNC_GPU_OK rank 0" in r.stdout and "SYNC_GPU_OK rank 1" in r.stdout
