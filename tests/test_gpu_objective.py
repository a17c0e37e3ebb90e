"""cvae_loss_obj on the GPU: the configurable objective (MS-SSIM weight, MSE term, KLD weight, used-terms MS-SSIM gradient)
against cvae_loss (bit for bit at the reference objective), against the oracle composed and differentiated on the CPU, and
through FusedTrainer's schedules, checkpoints and evaluate().  Bounds: the ones test_gpu_ops.test_msssim holds the MS-SSIM
op to (scalars 2e-5, gradients 1e-4 of the tensor's largest element); the pure-MSE gradient and scalars[13] to round-off
bounds derived where they are used."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.objective import Objective, compose
from critic_vae_amd.train import FusedTrainer, load_trainer, save_trainer
from oracle import cvae_oracle as orc
from test_gpu_ops import _ms_inputs, check

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
SENTINEL = 0x5A5AA5A5          # a finite float (1.5e16) no kernel would write by chance
MS_TAIL = 832                  # floats of slab + coef + ticket at the end of the "ms" region (include/cvae.h)
GUARD = 16384                  # 64 KB of floats after d_recon
REFERENCE = (1.0, 0.0, 0.001, 0)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def nans(n):
    return torch.full((n,), float("nan"), device="cuda")


class Call:
    """One loss call with NaN-prefilled outputs and a guard band after d_recon."""

    def __init__(self, h, B, W, x, mu, logvar, recon, obj, ws=None, raw=False):
        n = B * 3 * W * W
        self.n = n
        self.ws = torch.empty(h.workspace_bytes(B) // 4, device="cuda") if ws is None else ws
        self.scal, self.buf, self.d_mu, self.d_lv = nans(16), nans(n + GUARD), nans(B * 32), nans(B * 32)
        self.d_recon = self.buf[:n]
        if obj == "cvae_loss":
            h.loss(B, x, mu, logvar, recon, self.ws, self.scal, self.d_recon, self.d_mu, self.d_lv)
        elif raw:
            o = None if obj is None else C.byref(cvlib.Objective(*obj))
            self.rc = h.lib.cvae_loss_obj(h.h, B, x.data_ptr(), mu.data_ptr(), logvar.data_ptr(), recon.data_ptr(), self.ws.data_ptr(),
                                          o, self.scal.data_ptr(), self.d_recon.data_ptr(), self.d_mu.data_ptr(),
                                          self.d_lv.data_ptr(), cvlib._stream())
        else:
            h.loss_obj(B, x, mu, logvar, recon, self.ws, obj, self.scal, self.d_recon, self.d_mu, self.d_lv)
        torch.cuda.synchronize()
        assert bool((bits(self.buf[n:]) == NAN_BITS).all()), "write past the end of d_recon"

    def outputs(self):
        return [bits(t) for t in (self.scal, self.d_recon, self.d_mu, self.d_lv)]

    def untouched(self):
        return all(bool((b == NAN_BITS).all()) for b in self.outputs())


@functools.lru_cache(maxsize=None)
def smooth_case(W, B):
    """A smooth image against a noisy copy (all level means positive) with a latent: CPU tensors, shared and never modified."""
    g = torch.Generator().manual_seed(1000 * W + B)
    x = torch.rand(B, 3, W, W, generator=g)
    recon = (0.7 * x + 0.3 * torch.rand(B, 3, W, W, generator=g)).clone()
    mu = torch.randn(B, 32, generator=g) * 0.5
    logvar = torch.randn(B, 32, generator=g) * 0.3
    return x, mu, logvar, recon


def dev(*ts):
    return [t.cuda().contiguous() for t in ts]


def raw_kld(mu, logvar):
    return torch.mean(-0.5 * torch.sum(1 + logvar - mu ** 2 - logvar.exp(), dim=1), dim=0)


MS_W = torch.tensor(orc.MS_WEIGHTS, dtype=torch.float32)


def used_terms_loss(sims, css):
    return 1 - torch.prod(css[:4] ** MS_W[:4]) * sims[4] ** (4 * MS_W[4])


# ---- 1. the reference objective is cvae_loss, bit for bit ----
@pytest.mark.parametrize("W,B", [(64, 5), (128, 2)])
def test_default_objective_is_cvae_loss_bit_for_bit(W, B):
    h = cvlib.Handle(W, B)
    args = dev(*smooth_case(W, B))
    ref = Call(h, B, W, *args, "cvae_loss").outputs()
    one = Call(h, B, W, *args, REFERENCE)
    assert all(torch.equal(a, b) for a, b in zip(ref, one.outputs()))
    assert bits(one.scal)[13:].tolist() == [0, 0, 0]
    two = Call(h, B, W, *args, REFERENCE, ws=one.ws)
    assert all(torch.equal(a, b) for a, b in zip(ref, two.outputs()))


# ---- 2. each term against the oracle ----
OBJECTIVES = [(1.0, 0.5, 0.01, 0), (0.3, 2.0, 0.0, 0), (0.0, 1.0, 0.001, 0), (1.0, 0.0, 0.001, 1)]


def _obj_id(o):
    return "ms%g-mse%g-kld%g-%s" % (o[0], o[1], o[2], "used" if o[3] else "ref")


@pytest.mark.parametrize("obj", OBJECTIVES, ids=_obj_id)
@pytest.mark.parametrize("W,B", [(64, 1), (64, 5), (64, 37), (128, 3)])
def test_terms_against_the_oracle(W, B, obj):
    """An image is 3 * W * W / 4 float4 = 3 (64 wide) or 12 (128 wide) workgroup-trips of 1024 threads, so these shapes launch
    3, 15, 111 and 36 workgroups that make ONE full trip each: every term, every scalar and the merge over several
    workgroups, but not the strided loop (test_pixel_pass_strides_over_a_clamped_grid)."""
    _terms_against_the_oracle(W, B, obj)


@pytest.mark.parametrize("obj", [OBJECTIVES[0], OBJECTIVES[2]], ids=_obj_id)          # mixed and pure MSE: the two forms of the pixel pass
@pytest.mark.parametrize("W,B", [(64, 100), (128, 24)])
def test_pixel_pass_strides_over_a_clamped_grid(W, B, obj):
    """Past one trip: the pixel pass launches min(trips, compute units, 256) workgroups of 1024 threads.  B = 100 at 64 wide is 300
    workgroup-trips and B = 24 at 128 wide 288, over the 256 workgroups of an MI355X: the grid is clamped, `idx += stride` runs,
    and 44 (32) workgroups make two trips while the others make one.  A trip is never partly filled at these widths (an image is
    a whole number of trips), so the `idx < total4` test only ever ends a thread's loop."""
    h = cvlib.Handle(W, B)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    trips = B * 3 * W * W // 4 // 1024
    grid = min(cus, 256)
    assert trips > grid and trips % grid != 0, f"{trips} trips on {cus} compute units: not a clamped grid with uneven trip counts"
    _terms_against_the_oracle(W, B, obj, h)


def _terms_against_the_oracle(W, B, obj, h=None):
    w_ms, w_mse, beta, used = obj
    x, mu0, lv0, r0 = smooth_case(W, B)
    r, mu, lv = (t.clone().requires_grad_(True) for t in (r0, mu0, lv0))
    ms, sims, css = orc.msssim(r, x)
    assert bool((sims > 0).all()) and bool((css > 0).all())      # then the used-terms gradient is autograd's
    mse, kld = F.mse_loss(r, x), raw_kld(mu, lv)
    total = w_ms * ms + w_mse * mse + beta * kld
    total.backward()
    h = cvlib.Handle(W, B) if h is None else h
    c = Call(h, B, W, *dev(x, mu0, lv0, r0), obj)
    s = c.scal.cpu()
    twice = Call(h, B, W, *dev(x, mu0, lv0, r0), obj, ws=c.ws)
    assert all(torch.equal(a, b) for a, b in zip(c.outputs(), twice.outputs())), "the same call, other bits"
    print(f"scalars {s.tolist()}")
    if w_ms != 0:
        check(s[3:8], sims, "ssim levels", 2e-5)
        check(s[8:13], css, "cs levels", 2e-5)
        check(s[1], ms, "msssim loss", 2e-5)
    else:
        assert s[1].item() == 0.0 and bits(s[3:13]).tolist() == [0] * 10
    check(s[2], beta * kld, "weighted KLD", 2e-5)
    check(s[0], total, "total", 2e-5)
    assert s[14].item() == 0.0 and s[15].item() == 0.0
    if w_mse != 0:
        # fp32 squares (relative 2^-23 each: the difference and the square round once) summed in fp64, one rounding to fp32
        mse64 = ((r0.double() - x.double()) ** 2).mean().item()
        assert abs(s[13].item() - mse64) <= 1e-6 * mse64, (s[13].item(), mse64)
    else:
        assert s[13].item() == 0.0
    shape = (B, 3, W, W)
    if w_ms == 0:
        # d = fl(r - x), s = fl(2 w / N), g = fl(d * s): three roundings of 2^-24 relative each; 4 * 2^-24 of the largest element
        want = 2.0 * w_mse * (r0.double() - x.double()) / r0.numel()
        err = (c.d_recon.view(shape).cpu().double() - want).abs().max().item()
        bound = 4 * 2.0 ** -24 * want.abs().max().item()
        print(f"pure MSE gradient: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        check(c.d_recon.view(shape), r.grad, "d_recon vs autograd", rel=True)
    else:
        check(c.d_recon.view(shape), r.grad, "d_recon", rel=True)
    if beta != 0:
        check(c.d_mu.view(B, 32), mu.grad, "d_mu", rel=True)
        check(c.d_lv.view(B, 32), lv.grad, "d_logvar", rel=True)
    else:
        assert not c.d_mu.any() and not c.d_lv.any()


# ---- 3. a zero weight skips the work ----
@pytest.mark.parametrize("tag", ["pos", "nan"])
def test_zero_msssim_weight_runs_no_pyramid(tag):
    B = 4
    h = cvlib.Handle(64, B)
    a, b = _ms_inputs(tag)
    _, mu, lv, _ = smooth_case(64, 5)
    x, mu, lv, recon = dev(b, mu[:B], lv[:B], a)
    ws = torch.empty(h.workspace_bytes(B) // 4, device="cuda")
    off, n = h.lib.cvae_ws_offset(h.h, B, b"ms"), h.op_msssim_ws_floats(B)
    assert off >= 0 and off + n <= ws.numel()
    region = ws[off:off + n].view(torch.int32)
    region.fill_(SENTINEL)
    c = Call(h, B, 64, x, mu, lv, recon, (0.0, 1.0, 0.001, 0), ws=ws)
    assert bool((region[:n - MS_TAIL] == SENTINEL).all()), "a level field, pyramid or partial was written"
    s = c.scal.cpu()
    assert s[1].item() == 0.0 and bits(s[3:13]).tolist() == [0] * 10
    assert torch.isfinite(s).all() and s[13].item() > 0 and torch.isfinite(c.d_recon).all()
    if tag == "nan":                      # the same inputs under MS-SSIM: NaN, as test_gpu_ops.test_msssim pins
        full = Call(h, B, 64, x, mu, lv, recon, (1.0, 1.0, 0.001, 0), ws=ws)
        assert torch.isnan(full.scal[1]) and torch.isnan(full.scal[0]) and torch.isfinite(full.scal[13])


def test_zero_mse_weight_runs_no_pixel_pass():
    B = 4
    h = cvlib.Handle(64, B)
    a, b = _ms_inputs("pos")
    _, mu, lv, _ = smooth_case(64, 5)
    c = Call(h, B, 64, *dev(b, mu[:B], lv[:B], a), (1.0, 0.0, 0.001, 1))
    assert bits(c.scal)[13:].tolist() == [0, 0, 0] and torch.isfinite(c.scal[:13]).all()


# ---- 4. the NaN case: the reference's real frames under seed-0 weights ----
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_real_frames_nan_gradient_and_the_used_terms_gradient(golden_dir, precision):
    fx = np.load(os.path.join(golden_dir, "step_real_b68.npz"))
    B, wseed = 5, int(fx["wseed"])
    x = orc.preprocess_frames(torch.from_numpy(fx["u8"][:B])).cuda()
    pred = torch.from_numpy(fx["pred"][:B]).reshape(B, 1).float().cuda().contiguous()
    eps = torch.from_numpy(synth.make_batch(int(fx["dseed"]), int(fx["step"]), 68)[2][:B]).cuda().contiguous()

    def model():
        vae = VariationalAutoencoder(max_batch=B, seed=wseed, precision=precision).cuda()
        vae.load_reference_params(synth.make_params(wseed))
        return vae

    vae = model()
    h = vae.handle
    mu, lv, recon = torch.empty(B, 32, device="cuda"), torch.empty(B, 32, device="cuda"), torch.empty(B, 3, 64, 64, device="cuda")
    ws = vae._workspace(B)
    h.forward(B, x, pred, eps, vae.theta.data, vae.bn_state.clone(), mu, lv, recon, ws, train=True)
    torch.cuda.synchronize()
    plain = Call(h, B, 64, x, mu, lv, recon, "cvae_loss", ws=ws)
    ref = Call(h, B, 64, x, mu, lv, recon, REFERENCE, ws=ws)
    used = Call(h, B, 64, x, mu, lv, recon, (1.0, 0.0, 0.001, 1), ws=ws)
    s = ref.scal.cpu()
    print(f"{precision}: scalars {s[:13].tolist()}")
    assert torch.isfinite(s[0]) and s[3].item() < 0 and torch.equal(bits(ref.scal), bits(plain.scal))
    assert bool(torch.isnan(ref.d_recon).all()) and bool(torch.isnan(plain.d_recon).all())
    assert torch.equal(bits(used.scal)[:13], bits(ref.scal)[:13])
    assert bool(torch.isfinite(used.d_recon).all())
    r = recon.cpu().clone().requires_grad_(True)
    _, sims, css = orc.msssim(r, x.cpu())
    used_terms_loss(sims, css).backward()
    assert bool(torch.isfinite(r.grad).all())
    check(used.d_recon.view(B, 3, 64, 64), r.grad, "used-terms d_recon", rel=True)
    # three guarded steps: every one skipped under the reference objective, every one applied under the used-terms gradient
    for objective, want in ((None, (0, 3)), (Objective(msssim_grad="used"), (3, 0))):
        tr = FusedTrainer(model(), skip_nonfinite=True, objective=objective)
        for _ in range(3):
            tr.step(x, pred, eps)
        st = tr.guard_stats()
        assert (st["applied"], st["skipped"]) == want, (objective, st)


# ---- 5. schedules, resume, evaluate ----
def _trainer(B, objective=None, **kw):
    vae = VariationalAutoencoder(max_batch=B, seed=0).cuda()
    vae.load_reference_params(synth.make_params(0))
    return (FusedTrainer(vae, objective=objective, **kw) if objective is not None or kw else FusedTrainer(vae))


def _batches(B, n):
    return [dev(*(torch.from_numpy(t) for t in synth.make_batch(77, s, B))) for s in range(n)]


def _state(tr):
    return [bits(t) for t in (tr.vae.theta.data, tr.m, tr.v, tr.scalars, tr.vae.bn_state)]


def test_schedules_equal_a_hand_loop_and_resume_exactly(tmp_path):
    B, steps = 5, 6
    objective = Objective(mse=1.0, kld_warmup=4, msssim_from=3)
    data = _batches(B, steps)
    tr = _trainer(B, Objective(mse=1.0, kld_warmup=4, msssim_from=3))
    resumed = None
    for s, (x, pred, eps) in enumerate(data):
        tr.step(x, pred, eps)
        if s == 2:
            save_trainer(tr, str(tmp_path / "trainer.pt"))
            resumed = _trainer(B, Objective())                      # the saved objective replaces this one
            resumed.vae.theta.data.copy_(tr.vae.theta.data)
            resumed.vae.bn_state.copy_(tr.vae.bn_state)
            load_trainer(resumed, str(tmp_path / "trainer.pt"))
            assert resumed.objective == objective and resumed.step_count == 3
    for x, pred, eps in data[3:]:
        resumed.step(x, pred, eps)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_state(tr), _state(resumed)))
    # the hand loop: forward / loss_obj(at(s)) / backward / Adam on buffers of its own
    hand = _trainer(B)
    v, h = hand.vae, hand.h
    for s, (x, pred, eps) in enumerate(data):
        theta = v.theta.data
        h.forward(B, x, pred, eps, theta, v.bn_state, hand.mu, hand.logvar, hand.recon, hand.ws, train=True)
        h.loss_obj(B, x, hand.mu, hand.logvar, hand.recon, hand.ws, objective.at(s), hand.scalars, hand.d_recon, hand.d_mu, hand.d_logvar)
        h.backward(B, x, pred, eps, theta, hand.logvar, hand.recon, hand.d_recon, hand.d_mu, hand.d_logvar, hand.ws, hand.grads)
        h.adam_step(theta, hand.grads, hand.m, hand.v, s + 1, hand.lr, hand.betas[0], hand.betas[1], hand.eps, grad_scale=1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(_state(tr), _state(hand)))
    sc = tr.scalars.cpu()
    assert sc[1].item() > 0 and sc[13].item() > 0            # step 5: both terms on


def test_objective_none_is_the_trainer_without_the_argument():
    B = 5
    data = _batches(B, 3)
    a, b = _trainer(B), _trainer(B, objective=None, skip_nonfinite=False)
    assert a.objective is None and b.objective is None
    for x, pred, eps in data:
        a.step(x, pred, eps)
        b.step(x, pred, eps)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(_state(a), _state(b)))


def test_evaluate_reports_the_objective_from_its_own_entries():
    from critic_vae_amd.episodes import DeviceDataset
    B, n = 5, 7
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (n, 64, 64, 3), dtype=torch.uint8, generator=g)
    ds = DeviceDataset.from_host(frames.numpy(), critic=torch.rand(n, generator=g).numpy())
    objective = Objective(msssim=0.5, mse=2.0, kld=0.004, msssim_grad="used", kld_warmup=10)
    r = _trainer(B, objective).evaluate(ds, B)
    want = 0.5 * r["recon_loss"] + 2.0 * r["mean_mse"] + 0.004 * r["kld_raw"]
    assert r["objective"] == pytest.approx(want, rel=1e-12) and r["objective"] == compose(objective, r)
    assert r["kld_raw"] == pytest.approx(r["KLD"] / 0.001, rel=1e-5)
    assert "objective" not in _trainer(B).evaluate(ds, B)


# ---- 6. errors ----
@pytest.mark.parametrize("obj", [(-1.0, 1.0, 0.001, 0), (1.0, 0.0, -0.001, 0), (float("nan"), 1.0, 0.001, 0), (1.0, float("inf"), 0.001, 0),
                                 (0.0, 0.0, 0.001, 0), (1.0, 0.0, 0.001, 2), (1.0, 0.0, 0.001, -1), None])
def test_invalid_objectives_are_rejected_before_any_device_access(obj):
    B = 2
    h = cvlib.Handle(64, B)
    c = Call(h, B, 64, *dev(*(t[:B] for t in smooth_case(64, 5))), obj, raw=True)
    assert c.rc == -1 and c.untouched(), h.lib.cvae_last_error()


def test_objective_with_the_staged_cross_rank_step_raises():
    vae = VariationalAutoencoder(max_batch=2, seed=0).cuda()
    with pytest.raises(ValueError, match="global_stats"):
        FusedTrainer(vae, global_stats=True, objective=Objective(mse=1.0))
