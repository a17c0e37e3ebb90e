"""The guarded optimizer step on the GPU: the gradient-statistics pass on crafted buffers, the guarded Adam against
clip_grad_norm_ + torch.optim.Adam, and FusedTrainer(skip_nonfinite=..., max_grad_norm=...) on the batch that breaks an
unguarded run — the reference's own 68 frames with the seed-0 weights (tests/golden/step_real_b68.npz: finite loss, NaN
gradients), alone, with global-batch statistics, across two ranks, and through a save / resume."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from critic_vae_amd import lib as cvlib
from critic_vae_amd import params as P
from critic_vae_amd import synth
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
from oracle import cvae_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
LR, B1, B2 = 5e-5, 0.9, 0.999


def bits(t):
    """Bit patterns, so that NaNs compare as what they are."""
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guarded_trainer(vae, **kw):
    try:
        return FusedTrainer(vae, **kw)
    except TypeError as e:
        pytest.fail(f"FusedTrainer has no guard ({e}): whatever backward produced goes straight into Adam")


def guard_entry(H, name):
    if not hasattr(H, name):
        pytest.fail(f"the library binding has no {name}: the guarded step (cvae_grad_stats / cvae_adam_step_guarded) is missing")
    return getattr(H, name)


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return cvlib.Handle(64, 4)


def stats(H, g, scale=1.0, max_norm=INF, skip=True, state=None):
    """One statistics pass on a fresh guard state -> (record, its 64 raw bytes)."""
    if state is None:
        state = guard_entry(H, "guard_state")(g.device)
    H.grad_stats(g, state, scale, max_norm, skip, LR, B1, B2)
    rec = H.guard_record(state)
    return rec, bytes(rec)


def want(g, scale, max_norm):
    norm = torch.linalg.vector_norm(g.double().cpu() * scale).item()
    return norm, min(1.0, max_norm / (norm + 1e-6))


def host_bias(t):
    """launch_adam's host arithmetic: fp64 from the fp32 lr and betas the call receives -> (step_size, sqrt_bc2)."""
    lr, b1, b2 = (float(np.float32(x)) for x in (LR, B1, B2))
    return lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# n: one float4 | one workgroup's worth | a ragged grid-stride tail, several rounds of the capped grid | the model's flat gradient
SIZES = [4, 4096, 4 * (256 * 2048 + 3), None]


@pytest.fixture(scope="module", params=SIZES, ids=["n4", "n4096", "ragged-tail", "param-total"])
def buf(request, H):
    n = request.param if request.param is not None else H.param_total
    assert n % 4 == 0
    g = torch.Generator().manual_seed(n % 9973)
    return (torch.rand(n, generator=g) * 2 - 1).cuda()


def test_stats_random_values_norm_and_coef(H, buf):
    n = buf.numel()
    for scale, max_norm in ((1.0, INF), (0.5, 1.0), (0.5, 1e-3), (2.0, 1e4)):
        rec, _ = stats(H, buf, scale, max_norm)
        norm, coef = want(buf, scale, max_norm)
        print(f"n = {n}, scale {scale}, max_norm {max_norm}: norm {rec.norm64!r} (torch {norm!r}), coef {rec.coef!r} (torch {coef!r})")
        assert rel(rec.norm64, norm) <= 1e-6 and rel(rec.norm, norm) <= 1e-6
        assert abs(rec.coef - coef) <= 1e-6 * coef
        assert (rec.apply, rec.nonfinite, rec.t, rec.skipped, rec.ticket) == (1, 0, 1, 0, 0)
        assert rec.gscale == np.float32(scale) * np.float32(rec.coef)
        assert (rec.beta1, rec.beta2) == (np.float32(B1), np.float32(B2))
        assert rec.coef == 1.0 or max_norm != INF
        assert rec.coef < 1.0 or max_norm != 1e-3                        # both branches of the min are taken
        # launch_adam's host arithmetic at t = 1, rounded to float (one ulp for the device's pow)
        assert rel(rec.step_size, host_bias(1)[0]) <= 2.0 ** -23 and rel(rec.sqrt_bc2, host_bias(1)[1]) <= 2.0 ** -23


def test_stats_counts_steps_on_one_state_and_repeats_bit_for_bit(H, buf):
    """The same buffer gives the same record in every run (two fresh states), and a state that is used again counts on
    with the arrival ticket back at 0 each time."""
    a = stats(H, buf, 0.5, 1.0)[1]
    b = stats(H, buf, 0.5, 1.0)[1]
    assert a == b
    state = H.guard_state(buf.device)
    poisoned = buf.clone()
    poisoned[buf.numel() // 3] = float("nan")
    seen = []
    for k, g in enumerate((buf, poisoned, buf, buf)):
        rec, raw = stats(H, g, 0.5, 1.0, state=state)
        seen.append(rec)
        assert rec.ticket == 0 and rec.t + rec.skipped == k + 1
    assert [(r.apply, r.t, r.skipped) for r in seen] == [(1, 1, 0), (0, 1, 1), (1, 2, 1), (1, 3, 1)]
    assert seen[0].norm64 == seen[2].norm64 == seen[3].norm64 and seen[0].coef == seen[3].coef
    assert seen[1].step_size == 0.0                                     # a skipped step carries no bias correction
    assert rel(seen[3].step_size, host_bias(3)[0]) <= 2.0 ** -23 and rel(seen[3].sqrt_bc2, host_bias(3)[1]) <= 2.0 ** -23
    c = stats(H, poisoned, 0.5, 1.0)[1]
    assert c == stats(H, poisoned, 0.5, 1.0)[1]


def test_stats_zeros_denormals_and_huge_values(H, buf):
    n = buf.numel()
    rec, _ = stats(H, torch.zeros_like(buf), 1.0, 1.0)
    assert (rec.norm64, rec.norm, rec.coef, rec.apply, rec.nonfinite) == (0.0, 0.0, 1.0, 1, 0)
    # denormals only: every element below FLT_MIN, none flushed on the way into the fp64 sum
    den = (buf.cpu().double() * 1e-39).float().cuda()
    den[den == 0] = 1e-45
    assert (den.abs() < 1.17549435e-38).all() and (den != 0).all()
    rec, _ = stats(H, den, 1.0, 1.0)
    norm, _ = want(den, 1.0, 1.0)
    print(f"n = {n}, denormals: norm {rec.norm64!r} (torch {norm!r})")
    assert norm > 0 and rel(rec.norm64, norm) <= 1e-6 and (rec.coef, rec.apply, rec.nonfinite) == (1.0, 1, 0)
    # all elements 3e38: the squares overflow fp32, not fp64 — a finite norm, a clipped step, no skip
    huge = torch.full_like(buf, 3e38)
    rec, _ = stats(H, huge, 1.0, 1.0, skip=True)
    norm, coef = want(huge, 1.0, 1.0)
    print(f"n = {n}, 3e38: norm {rec.norm64!r} (torch {norm!r}), coef {rec.coef!r} (torch {coef!r})")
    assert math.isfinite(rec.norm64) and rel(rec.norm64, norm) <= 1e-6 and math.isinf(rec.norm)
    assert (rec.nonfinite, rec.apply, rec.t, rec.skipped) == (0, 1, 1, 0)
    # coef ~ 1e-39 .. 1e-42 is a denormal float: half a unit of 2^-149 for its rounding, 1e-6 relative for the norm
    assert 0.0 < rec.coef < 1.0 and abs(rec.coef - coef) <= 2.0 ** -150 + 1e-6 * coef
    assert rec.gscale == rec.coef


@pytest.mark.parametrize("value,where", [(float("nan"), "last"), (INF, "first"), (-INF, "middle")])
def test_stats_flags_a_single_non_finite_element(H, buf, value, where):
    n = buf.numel()
    g = buf.clone()
    g[{"last": n - 1, "first": 0, "middle": n // 2}[where]] = value
    for skip in (True, False):
        for max_norm in (INF, 1.0):
            rec, _ = stats(H, g, 1.0, max_norm, skip=skip)
            assert rec.nonfinite == 1 and rec.apply == (0 if skip else 1), (skip, max_norm)
            assert (rec.t, rec.skipped) == ((0, 1) if skip else (1, 0))
            assert not math.isfinite(rec.norm64)
            if max_norm == INF:
                assert rec.coef == 1.0                       # no clipping: the gradient flows through as it is
    # skipping off, finite max_norm (include/cvae.h): an Inf gives norm inf and coef 0, a NaN gives norm NaN and coef 1
    rec, _ = stats(H, g, 1.0, 1.0, skip=False)
    assert (rec.coef, rec.gscale) == ((1.0, 1.0) if math.isnan(value) else (0.0, 0.0))
    assert math.isnan(rec.norm64) if math.isnan(value) else rec.norm64 == INF
    # the flag comes from the exponent bits: huge finite neighbours do not set it, a finite sum does not clear it
    rec, _ = stats(H, torch.full_like(buf, 3e38), 1.0, INF)
    assert rec.nonfinite == 0


def test_guarded_adam_matches_clip_grad_norm_and_torch_adam(H):
    """test_adam_matches_torch's setup, every step clipped: clip_grad_norm_ + torch.optim.Adam on the CPU."""
    n, max_norm = 4096, 0.05
    p0 = torch.from_numpy(synth.uniform(7, "ap", (n,), -1.0, 1.0))
    g = torch.from_numpy(synth.uniform(7, "ag", (n,), -1e-2, 1e-2))
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=LR)
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    state = guard_entry(H, "guard_state")(p.device)
    for step in range(1, 6):
        gs = g * step
        p_ref.grad = gs.clone()
        total = torch.nn.utils.clip_grad_norm_([p_ref], max_norm)
        assert total.item() > max_norm                      # every step clips
        opt.step()
        gd = (gs * 2.0).cuda()
        H.grad_stats(gd, state, 0.5, max_norm, True, LR, B1, B2)
        H.adam_step_guarded(p, gd, m, v, state, eps=1e-8)
        rec = H.guard_record(state)
        assert rec.apply == 1 and rec.t == step and rec.coef < 1.0 and rel(rec.norm64, total.item()) <= 1e-6
    err = (p.cpu().double() - p_ref.detach().double()).abs().max().item()
    print(f"guarded adam vs clip_grad_norm_ + torch Adam: max|err| {err:.3e}")
    assert err <= 1e-7


def test_guarded_adam_leaves_every_bit_when_it_skips(H):
    n = 4 * (256 * 2048 + 3)
    gen = torch.Generator().manual_seed(11)
    p, m, v, g = (torch.randn(n, generator=gen).cuda() for _ in range(4))
    v = v.abs()
    g[n - 1] = INF
    before = [t.clone() for t in (p, m, v)]
    state = guard_entry(H, "guard_state")(p.device)
    H.grad_stats(g, state, 1.0, 1.0, True, LR, B1, B2)
    H.adam_step_guarded(p, g, m, v, state, eps=1e-8)
    assert all(same_bits(a, b) for a, b in zip(before, (p, m, v)))
    H.grad_stats(g, state, 1.0, 1.0, False, LR, B1, B2)       # skipping off, finite max_norm: coef = 0, the Inf element turns NaN (inf * 0)
    H.adam_step_guarded(p, g, m, v, state, eps=1e-8)
    bad = ~torch.isfinite(m)
    assert bad[n - 1] and int(bad.sum()) == 1 and torch.isnan(p[n - 1]) and torch.isfinite(p[:n - 1]).all()
    # ... and with max_norm = inf the update is cvae_adam_step's own, bit for bit, non-finite element included
    p1, m1, v1 = (t.clone() for t in before)
    p2, m2, v2 = (t.clone() for t in before)
    H.grad_stats(g, state, 0.5, INF, False, LR, B1, B2)
    H.adam_step_guarded(p1, g, m1, v1, state, eps=1e-8)
    t = H.guard_record(state).t
    H.adam_step(p2, g, m2, v2, int(t), LR, B1, B2, 1e-8, grad_scale=0.5)
    assert same_bits(p1, p2) and same_bits(m1, m2) and same_bits(v1, v2)


# ---- FusedTrainer ----
def batch(step, B, dseed=1234):
    return tuple(torch.from_numpy(a).cuda() for a in synth.make_batch(dseed, step, B))


def fresh(B, seed=0):
    return VariationalAutoencoder(max_batch=B, seed=seed).cuda()


def test_noop_guard_equals_no_guard():
    """skip_nonfinite with nothing to skip and max_grad_norm = inf: the same model as the plain trainer.  m and v do not see
    the bias correction and must agree to the bit; theta sees the device's step_size / sqrt_bc2 (fp64 pow on the device
    instead of the host's)."""
    B = 4
    va, vb = fresh(B), fresh(B)
    ta, tb = FusedTrainer(va), guarded_trainer(vb, skip_nonfinite=True, max_grad_norm=INF)
    for s in range(5):
        x, pred, eps = batch(s, B)
        ta.step(x, pred, eps)
        tb.step(x, pred, eps)
    torch.cuda.synchronize()
    assert torch.isfinite(va.theta).all()
    assert same_bits(ta.m, tb.m) and same_bits(ta.v, tb.v)
    err = (va.theta.data.double() - vb.theta.data.double()).abs().max().item()
    print(f"no-op guard vs no guard after 5 steps: theta max|diff| {err:.3e}, bit-identical: {same_bits(va.theta.data, vb.theta.data)}")
    assert err <= 1e-7
    st = tb.guard_stats()
    assert (st["applied"], st["skipped"], st["coef"]) == (5, 0, 1.0) and st["norm"] > 0
    assert ta.step_count == tb.step_count == 5 and same_bits(va.bn_state, vb.bn_state)


@pytest.fixture(scope="module")
def real(golden_dir):
    """The 68 real frames, the reference critic's values of them and eps: with the seed-`wseed` weights the loss is finite and
    every gradient through recon is NaN."""
    fx = np.load(os.path.join(golden_dir, "step_real_b68.npz"))
    B = int(fx["batch"])
    x = orc.preprocess_frames(torch.from_numpy(fx["u8"])).cuda()
    pred = torch.from_numpy(fx["pred"]).reshape(B, 1).float().contiguous().cuda()
    eps = torch.from_numpy(synth.make_batch(int(fx["dseed"]), int(fx["step"]), B)[2]).cuda()
    return dict(B=B, wseed=int(fx["wseed"]), bad=(x, pred, eps), good=batch(0, B))


@pytest.mark.parametrize("global_stats", [False, True], ids=["local", "global-stats"])
def test_real_frames_are_skipped_and_the_next_step_is_step_one(real, global_stats):
    B, kw = real["B"], dict(global_stats=global_stats)
    # today's behaviour, and this test's premise: one such batch and theta is NaN for good
    v0 = fresh(B, real["wseed"])
    start = v0.theta.data.clone()
    t0 = FusedTrainer(v0, **kw)
    scal = t0.step(*real["bad"])
    torch.cuda.synchronize()
    assert torch.isfinite(scal[:3]).all() and abs(scal[0].item() - 0.8214) < 2e-3
    n_nan = int(torch.isnan(v0.theta.data).sum())
    print(f"unguarded step on the real frames: loss {scal[0].item():.4f}, {n_nan} of {start.numel()} parameters NaN")
    assert n_nan > 0
    # guarded: the same step changes nothing
    v1 = fresh(B, real["wseed"])
    assert same_bits(v1.theta.data, start)
    t1 = guarded_trainer(v1, skip_nonfinite=True, **kw)
    t1.step(*real["bad"])
    torch.cuda.synchronize()
    assert same_bits(v1.theta.data, start) and not t1.m.any() and not t1.v.any()
    assert same_bits(t1.m, torch.zeros_like(t1.m)) and same_bits(t1.v, torch.zeros_like(t1.v))
    st = t1.guard_stats()
    assert (st["applied"], st["skipped"]) == (0, 1) and t1.step_count == 1 and v1.num_batches_tracked == 1
    # ... and the next, finite batch is Adam's step 1: bias correction for t = 1, not for step_count = 2
    t1.step(*real["good"])
    v2 = fresh(B, real["wseed"])
    t2 = FusedTrainer(v2, **kw)
    t2.step(*real["good"])
    torch.cuda.synchronize()
    assert torch.isfinite(v2.theta.data).all() and not same_bits(v2.theta.data, start)
    assert same_bits(t1.m, t2.m) and same_bits(t1.v, t2.v)
    err = (v1.theta.data.double() - v2.theta.data.double()).abs().max().item()
    print(f"step after the skip vs a first step: theta max|diff| {err:.3e}")
    assert err <= 1e-7
    st = t1.guard_stats()
    assert (st["applied"], st["skipped"]) == (1, 1) and t1.step_count == 2


def test_clipping_in_a_real_step():
    B = 4
    x, pred, eps = batch(0, B)
    va = fresh(B)
    theta0 = va.theta.data.clone()
    ta = FusedTrainer(va)
    ta.step(x, pred, eps)
    torch.cuda.synchronize()
    grads = ta.grads.cpu()
    norm = torch.linalg.vector_norm(grads.double()).item()
    vb = fresh(B)
    tb = guarded_trainer(vb, max_grad_norm=norm / 2)
    tb.step(x, pred, eps)
    st = tb.guard_stats()
    print(f"B = {B}: gradient norm {norm!r}; guarded norm {st['norm']!r}, coef {st['coef']!r}")
    assert same_bits(tb.grads, ta.grads) and rel(st["norm"], norm) <= 1e-6
    assert abs(st["coef"] - 0.5) <= 1e-6 and (st["applied"], st["skipped"]) == (1, 0)
    p_ref = theta0.cpu().clone().requires_grad_(True)
    p_ref.grad = grads.clone()
    torch.nn.utils.clip_grad_norm_([p_ref], norm / 2)
    torch.optim.Adam([p_ref], lr=P.lr, betas=P.adam_betas, eps=P.adam_eps).step()
    err = (vb.theta.data.cpu().double() - p_ref.detach().double()).abs().max().item()
    print(f"clipped step vs clip_grad_norm_ + torch Adam: theta max|err| {err:.3e}")
    assert err <= 1e-7
    assert not same_bits(vb.theta.data, va.theta.data)


def test_resume_continues_bit_for_bit(tmp_path):
    """Six guarded steps == three steps, save, a fresh VAE and trainer, load, three more.  The second batch carries an Inf, so the
    saved applied count (2) is not step_count (3): a resume that mixes them up corrects Adam's bias for the wrong step."""
    from critic_vae_amd.train import load_networks, save_networks
    try:
        from critic_vae_amd.train import load_trainer, save_trainer
    except ImportError as e:
        pytest.fail(f"no trainer checkpoint ({e}): a run that can skip cannot be restarted")
    B, kw = 4, dict(skip_nonfinite=True, max_grad_norm=1.0)
    batches = [batch(s, B) for s in range(6)]
    batches[1][0][2, 1, 5, 7] = INF

    def run(tr, steps):
        for s in steps:
            tr.step(*batches[s])

    va = fresh(B)
    ta = guarded_trainer(va, **kw)
    run(ta, range(6))
    vb = fresh(B)
    tb = FusedTrainer(vb, **kw)
    run(tb, range(3))
    sd = tb.state_dict()
    assert (sd["applied"], sd["skipped"], sd["step_count"]) == (2, 1, 3)
    save_networks(vb, str(tmp_path))
    save_trainer(tb, str(tmp_path / "trainer.pt"))
    vc = fresh(B, seed=1)
    tc = FusedTrainer(vc, **kw)
    load_networks(vc, str(tmp_path))
    load_trainer(tc, str(tmp_path / "trainer.pt"))
    assert same_bits(vc.theta.data, vb.theta.data) and same_bits(vc.bn_state, vb.bn_state)
    run(tc, range(3, 6))
    torch.cuda.synchronize()
    assert torch.isfinite(va.theta.data).all()
    for name, a, c in (("theta", va.theta.data, vc.theta.data), ("m", ta.m, tc.m), ("v", ta.v, tc.v), ("bn_state", va.bn_state, vc.bn_state)):
        assert same_bits(a, c), name
    sa, sc = ta.guard_stats(), tc.guard_stats()
    assert sa == sc and (sa["applied"], sa["skipped"]) == (5, 1)
    assert ta.step_count == tc.step_count == 6 and va.num_batches_tracked == vc.num_batches_tracked == 6


def test_two_rank_guarded_step():
    env = dict(os.environ, CVAE_DIST_BACKEND="gloo", CVAE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nnodes=1", "--nproc-per-node=2", os.path.join(ROOT, "tests", "guard_dp_worker.py")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "GUARD_DP_OK rank 0" in r.stdout and "GUARD_DP_OK rank 1" in r.stdout
