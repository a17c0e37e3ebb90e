"""Held-out validation on the GPU: cvae_score's per-image rows against the oracle applied to each image alone, a non-finite
image reported instead of hidden, the pooled record against cvae_loss on the whole set as one batch, determinism and memory
discipline of the call, and FusedTrainer.evaluate / fit_device(val=...) on real frames leaving the training run bit for bit
what it is without them."""
import functools
import os

import numpy as np
import pytest
import torch

from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
from oracle import cvae_oracle as orc
from ws_tools import FILLS, holds, poison, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = 8
TAIL = 16384            # floats (64 KB) behind the row buffer that the call must leave alone


def entry(obj, name):
    if not hasattr(obj, name):
        pytest.fail(f"{type(obj).__name__} has no {name}: per-image scores / held-out evaluation are missing")
    return getattr(obj, name)


@functools.lru_cache(maxsize=None)
def handle(width, max_batch, precision="f32"):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return cvlib.Handle(width, max_batch, precision=precision)


@functools.lru_cache(maxsize=None)
def inputs(width, B, a, flip=None):
    """x, recon = a x + (1 - a) u, mu, logvar (numpy fp32); flip: that image's recon becomes 1 - x."""
    x = synth.make_batch(7, 0, B, width)[0]
    recon = (np.float32(a) * x + np.float32(1 - a) * synth.uniform(11, "recon", x.shape)).astype(np.float32)
    if flip is not None:
        recon[flip] = 1 - x[flip]
    mu, logvar = synth.normal(11, "mu", (B, 32)), synth.normal(11, "logvar", (B, 32))
    return x, recon, mu, logvar


@functools.lru_cache(maxsize=None)
def oracle_rows(width, B, a):
    """Per image: the oracle's MSSIM of the image alone, its weighted KLD, float64 mse and max |recon - x|, ssim levels 0 and 4."""
    x, recon, mu, logvar = (torch.from_numpy(t) for t in inputs(width, B, a))
    out = np.zeros((B, 6), np.float64)
    for i in range(B):
        loss, sims, _ = orc.msssim(recon[i:i + 1], x[i:i + 1])
        out[i, 0], out[i, 4], out[i, 5] = loss.item(), sims[0].item(), sims[4].item()
        out[i, 1] = orc.vae_loss(x[i:i + 1], mu[i:i + 1], logvar[i:i + 1], recon[i:i + 1])["KLD"].item()
        d = recon[i].double() - x[i].double()
        out[i, 2] = (d ** 2).mean().item()
        out[i, 3] = d.abs().max().item()
    return out


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run_score(H, B, x, recon, mu, logvar, rows=True, state=None, ws=None):
    """One cvae_score; returns (rows or None, ws)."""
    if ws is None:
        ws = torch.empty(H.workspace_bytes(B) // 4, device="cuda")
    out = torch.empty(B, COLS, device="cuda") if rows else None
    entry(H, "score")(B, x, mu, logvar, recon, ws, out, state)
    return out, ws


def record(state):
    s = state.cpu().numpy()
    return dict(sums=s[:11], images=s[11], finite=s[12], sum_total=s[13], sum_msssim=s[14], sum_kld=s[15], sum_mse=s[16], worst=s[17])


CASES = [(64, 1, 5), (64, 3, 5), (64, 5, 5), (128, 1, 2), (128, 2, 2), (64, 7, 7)]      # (width, batch, max_batch); the last: B = max_batch


@pytest.mark.parametrize("a", [0.9, 0.7, 0.5])
@pytest.mark.parametrize("width,B,mb", CASES)
def test_rows_match_the_oracle_per_image(width, B, mb, a):
    H = handle(width, mb)
    rows, _ = run_score(H, B, *dev(*inputs(width, B, a)))
    got, want = rows.cpu().numpy().astype(np.float64), oracle_rows(width, B, a)
    for i in range(B):
        print(f"W {width} B {B} a {a} image {i}: msssim {got[i, 1]:.7f} (oracle {want[i, 0]:.7f}) kld {got[i, 2]:.7f} ({want[i, 1]:.7f}) "
              f"mse {got[i, 3]:.9f} ({want[i, 2]:.9f}) max {got[i, 4]:.9f}")
        assert abs(got[i, 1] - want[i, 0]) <= 1e-4
        assert abs(got[i, 2] - want[i, 1]) <= 1e-4
        assert abs(got[i, 3] - want[i, 2]) <= 1e-6 * want[i, 2]
        assert np.float32(got[i, 4]) == np.float32(want[i, 3])
        assert np.float32(got[i, 0]) == np.float32(got[i, 1]) + np.float32(got[i, 2])
        assert got[i, 7] == 0
    assert np.abs(got[:, 5:7] - want[:, 4:6]).max() <= 1e-4


def test_rows_are_per_image_not_batch_means():
    """At a = 0.5 the per-image losses spread over 0.0834..0.0885 around the batch loss 0.0859: the rows must differ."""
    H = handle(64, 12)
    rows, _ = run_score(H, 12, *dev(*inputs(64, 12, 0.5)))
    r = rows[:, 1].cpu().numpy()
    assert r.max() - r.min() > 3e-3
    want = oracle_rows(64, 12, 0.5)
    assert np.abs(r - want[:, 0]).max() <= 1e-4


def test_a_nonfinite_image_is_reported_not_hidden():
    H = handle(64, 5)
    clean, _ = run_score(H, 5, *dev(*inputs(64, 5, 0.7)))
    state = entry(H, "score_state")("cuda")
    rows, _ = run_score(H, 5, *dev(*inputs(64, 5, 0.7, flip=2)), state=state)
    r = rows.cpu().numpy()
    assert np.isnan(r[2, 0]) and np.isnan(r[2, 1])
    assert np.isfinite(r[2, 2:5]).all()
    keep = [0, 1, 3, 4]
    assert same_bits(rows[keep], clean[keep])
    rec = record(state)
    assert rec["images"] == 5 and rec["finite"] == 4
    r64 = r[keep].astype(np.float64)
    for k, c in (("sum_total", 0), ("sum_msssim", 1), ("sum_kld", 2), ("sum_mse", 3)):
        assert abs(rec[k] - r64[:, c].sum()) <= 1e-12 * abs(r64[:, c].sum()), k
    assert rec["worst"] == r64[:, 0].max()


@pytest.mark.parametrize("width", [64, 128])
def test_batch_of_one_equals_cvae_loss(width):
    H = handle(width, 5 if width == 64 else 2)
    t = dev(*inputs(width, 1, 0.7))
    rows, ws = run_score(H, 1, *t)
    scal = torch.empty(16, device="cuda")
    H.loss(1, t[0], t[2], t[3], t[1], ws, scal)
    got, want = rows[0, :3].cpu().numpy().astype(np.float64), scal[:3].cpu().numpy().astype(np.float64)
    print("row", got, "cvae_loss", want)
    assert np.abs(got - want).max() <= 1e-6


@pytest.mark.parametrize("sizes", [(5, 5, 2), (1,) * 12])
def test_pooled_record_equals_cvae_loss_on_the_whole_set(sizes):
    H = handle(64, 12)
    x, recon, mu, logvar = dev(*inputs(64, 12, 0.7))
    state = entry(H, "score_state")("cuda")
    ws = torch.empty(H.workspace_bytes(12) // 4, device="cuda")
    s = 0
    for n in sizes:
        run_score(H, n, x[s:s + n], recon[s:s + n], mu[s:s + n], logvar[s:s + n], rows=False, state=state, ws=ws)
        s += n
    pooled = torch.empty(16, device="cuda")
    H.score_finish(state, pooled)
    whole = torch.empty(16, device="cuda")
    H.loss(12, x, mu, logvar, recon, ws, whole)
    got, want = pooled[:13].cpu().numpy().astype(np.float64), whole[:13].cpu().numpy().astype(np.float64)
    print("pooled", got, "\ncvae_loss", want)
    assert np.abs(got - want).max() <= 1e-6
    assert record(state)["images"] == 12
    o = orc.vae_loss(*(torch.from_numpy(t) for t in (inputs(64, 12, 0.7)[0], inputs(64, 12, 0.7)[2], inputs(64, 12, 0.7)[3], inputs(64, 12, 0.7)[1])))
    ref = np.concatenate([[o["total_loss"].item(), o["recon_loss"].item(), o["KLD"].item()], o["ssim_levels"].numpy(), o["cs_levels"].numpy()])
    assert np.abs(got - ref).max() <= 1e-4


def test_same_bits_on_every_run_whatever_the_buffers_held():
    H = handle(64, 5)
    B = 5
    t = dev(*inputs(64, B, 0.7))
    ws = torch.empty(H.workspace_bytes(B) // 4, device="cuda")
    buf = torch.empty(B * COLS + TAIL, device="cuda")
    results = []
    for name, pattern in FILLS + (("ones again", FILLS[-1][1]),):
        poison(ws, pattern)
        poison(buf, pattern)
        state = entry(H, "score_state")("cuda")
        H.score(B, t[0], t[2], t[3], t[1], ws, buf[:B * COLS], state)
        torch.cuda.synchronize()
        assert holds(buf[B * COLS:], pattern).all(), f"{name}: the call wrote behind its {B} rows"
        results.append((name, buf[:B * COLS].clone(), state[:18].clone()))
    for name, rows, st in results[1:]:
        assert same_bits(rows, results[0][1]), f"rows differ between fills zero and {name}"
        assert same_bits(st, results[0][2]), f"record differs between fills zero and {name}"
    # either output alone
    only_rows, _ = run_score(H, B, *t, ws=ws)
    assert same_bits(only_rows.reshape(-1), results[0][1])
    state = H.score_state("cuda")
    poison(ws, FILLS[-1][1])
    run_score(H, B, *t, rows=False, state=state, ws=ws)
    assert same_bits(state[:18], results[0][2])


def test_bad_arguments_are_rejected_before_any_device_access():
    H = handle(64, 5)
    t = dev(*inputs(64, 5, 0.7))
    ws = torch.empty(H.workspace_bytes(5) // 4, device="cuda")
    rows = torch.full((5, COLS), 7.0, device="cuda")
    for B in (0, 6):
        with pytest.raises(cvlib.CvaeError):
            H.score(B, t[0], t[2], t[3], t[1], ws, rows, None)
    with pytest.raises(cvlib.CvaeError):
        H.score(5, t[0], t[2], t[3], t[1], ws, None, None)
    assert (rows == 7.0).all()


# ---- validation inside the training loop ----
@functools.lru_cache(maxsize=None)
def real_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))


def small_dataset():
    """3 trajectories of 16 + 14 + 10 frames on the device with their critic values: the first 40 of the 68 real frames of
    step_real_b68.npz (noise frames against an untrained decoder give negative cs means, a NaN loss and NaN parameters after
    one step: two NaN runs would be 'identical' whatever validation did)."""
    fx = real_fixture()
    lengths = [16, 14, 10]
    n = sum(lengths)
    source = np.stack([np.repeat(np.arange(3), lengths), np.concatenate([np.arange(k) for k in lengths])], 1)
    return E.DeviceDataset(torch.from_numpy(fx["u8"][:n].copy()).cuda(), torch.from_numpy(fx["pred"][:n].copy()).cuda(), source)


def fresh_trainer(precision):
    """The weights the real-frames fixtures train from (test_gpu_step: the loss stays finite over 200 steps)."""
    from test_oracle import real_frames_params
    fx = real_fixture()
    vae = VariationalAutoencoder(max_batch=8, seed=int(fx["wseed"]), precision=precision).to("cuda:0")
    vae.load_reference_params(real_frames_params(fx))
    return FusedTrainer(vae)


def fit(trainer, ds, **kw):
    np.random.seed(5)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    return trainer.fit_device(ds, 8, 2, generator=gen, **kw)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_validation_does_not_perturb_training(precision):
    full = small_dataset()
    train, val = entry(E, "split_by_trajectory")(full, 0.25, seed=0)
    assert len(train) + len(val) == 40 and len(val) >= 10
    assert not set(train.source[:, 0].tolist()) & set(val.source[:, 0].tolist())
    plain, watched = fresh_trainer(precision), fresh_trainer(precision)
    fit(plain, train)
    fit(watched, train, val=val, val_every=2)
    torch.cuda.synchronize()
    assert torch.isfinite(plain.vae.theta.data).all() and torch.isfinite(plain.vae.bn_state).all(), "the run itself went non-finite"
    for name, a, b in (("theta", plain.vae.theta.data, watched.vae.theta.data), ("exp_avg", plain.m, watched.m),
                       ("exp_avg_sq", plain.v, watched.v), ("bn_state", plain.vae.bn_state, watched.vae.bn_state)):
        assert same_bits(a, b), f"{name} differs once validation runs between the steps"
    steps = 2 * -(-len(train) // 8)
    assert plain.step_count == watched.step_count == steps
    assert plain.vae.num_batches_tracked == watched.vae.num_batches_tracked == steps
    assert [t for t, _ in watched.val_history] == list(range(2, steps + 1, 2)) and plain.val_history == []
    for _, r in watched.val_history:
        assert r["images"] == len(val) and np.isfinite(r["KLD"])
        print(precision, "val", r["total_loss"], r["recon_loss"], r["KLD"], r["finite_images"], r["mean_mse"], r["psnr"])
    # nothing of the trainer moves under evaluate itself
    before = [t.clone() for t in (watched.vae.theta.data, watched.m, watched.v, watched.vae.bn_state)]
    r8 = watched.evaluate(val, 8, per_image=True)
    assert all(same_bits(a, b) for a, b in zip(before, (watched.vae.theta.data, watched.m, watched.v, watched.vae.bn_state)))
    assert watched.step_count == steps and watched.vae.num_batches_tracked == steps
    assert tuple(r8["per_image"].shape) == (len(val), COLS)
    if precision == "f32":
        r3 = watched.evaluate(val, 3)
        for k in ("total_loss", "recon_loss", "KLD", "mean_total", "mean_msssim", "mean_kld", "mean_mse", "worst"):
            print(k, r8[k], r3[k])
            assert (np.isnan(r8[k]) and np.isnan(r3[k])) or abs(r8[k] - r3[k]) <= 1e-6, k
        assert np.abs(np.array(r8["ssim_levels"] + r8["cs_levels"]) - np.array(r3["ssim_levels"] + r3["cs_levels"])).max() <= 1e-6
        assert r8["images"] == r3["images"] == len(val) and r8["finite_images"] == r3["finite_images"]


def test_on_val_can_stop_the_fit():
    full = small_dataset()
    train, val = entry(E, "split_by_trajectory")(full, 0.25, seed=0)
    tr = fresh_trainer("f32")
    seen = []
    fit(tr, train, val=val, val_every=2, on_val=lambda t, r: seen.append(t.step_count) or t.step_count >= 4)
    assert tr.step_count == 4 and seen == [2, 4] and len(tr.val_history) == 2
    tr.best_val, tr.val_stale = 0.25, 1
    sd = tr.state_dict()
    assert [t for t, _ in sd["val_history"]] == [2, 4]
    other = fresh_trainer("f32")
    other.load_state_dict(sd)
    assert [t for t, _ in other.val_history] == [2, 4] and other.val_history[1][1] == tr.val_history[1][1]
    assert other.best_val == 0.25 and other.val_stale == 1 and other.step_count == 4
    del sd["val_history"], sd["best_val"], sd["val_stale"]              # a state written before validation existed still loads
    other.load_state_dict(sd)
    assert other.val_history == [] and other.best_val is None and other.val_stale == 0


# ---- end to end on real frames: tests/golden/score_real.npz (make_score_golden.py) ----
@functools.lru_cache(maxsize=None)
def score_fixture():
    path = os.path.join(ROOT, "tests", "golden", "score_real.npz")
    if not os.path.exists(path):
        pytest.fail("tests/golden/score_real.npz is missing (tests/golden/make_score_golden.py writes it)")
    return np.load(path)


@functools.lru_cache(maxsize=None)
def trained_state():
    """The fixture's training repeated here: `steps` FusedTrainer steps in fp32 on the 68 real frames as one batch, from the
    fixture's start weights and eps stream (the trained weights are too large to store).  Returns (theta, bn_state with the
    REFERENCE's stored running statistics, x, pred)."""
    from test_oracle import real_frames_params
    fx, sf = real_fixture(), score_fixture()
    x = orc.preprocess_frames(torch.from_numpy(fx["u8"])).cuda().contiguous()
    pred = torch.from_numpy(fx["pred"]).cuda()
    vae = VariationalAutoencoder(max_batch=68, seed=int(fx["wseed"])).to("cuda:0")
    vae.load_reference_params(real_frames_params(fx))
    tr = FusedTrainer(vae)
    for s in range(int(sf["steps"])):
        tr.step(x, pred, torch.from_numpy(synth.make_batch(int(sf["dseed"]), s, 68)[2]).cuda())
    bn = torch.from_numpy(np.concatenate([sf["running_mean"], sf["running_var"]])).cuda()
    print("running statistics, this run against the reference's: max |d mean|", (vae.bn_state[:480] - bn[:480]).abs().max().item(),
          "max |d var|", (vae.bn_state[480:] - bn[480:]).abs().max().item())
    return vae.theta.data.clone(), bn, x[sf["index"]].contiguous(), pred[sf["index"]].contiguous()


def scoring_vae(max_batch, precision="f32"):
    theta, bn, x, pred = trained_state()
    vae = VariationalAutoencoder(max_batch=max_batch, seed=0, precision=precision).to("cuda:0")
    vae.theta.data.copy_(theta)
    vae.bn_state.copy_(bn)
    vae.num_batches_tracked = int(score_fixture()["num_batches_tracked"])
    return vae.eval(), x, pred


def test_score_on_real_frames_matches_the_reference():
    """vae.score in fp32 against the reference's eval-mode per-image values, in pieces of 20 + 20 + 20 + 8."""
    sf = score_fixture()
    vae, x, pred = scoring_vae(20)
    bn_before, nbt = vae.bn_state.clone(), vae.num_batches_tracked
    rows = entry(vae, "score")(x, pred)
    assert tuple(rows.shape) == (68, COLS)
    assert same_bits(vae.bn_state, bn_before) and vae.num_batches_tracked == nbt
    got = rows.cpu().numpy().astype(np.float64)
    ok = ~sf["flagged"]
    used = np.concatenate([sf["cs_levels"][:, :4], sf["ssim_levels"][:, 4:5]], 1)
    decided = ok | (np.abs(used).min(1) > 1e-5)              # flagged images still agree on finite versus NaN unless within 1e-5 of zero
    assert np.array_equal(np.isnan(got[decided, 1]), np.isnan(sf["msssim"][decided]))
    err = {"msssim": np.abs(got[ok, 1] - sf["msssim"][ok]).max(), "kld": np.abs(got[ok, 2] - sf["kld"][ok]).max(),
           "ssim0": np.abs(got[ok, 5] - sf["ssim_levels"][ok, 0]).max(), "ssim4": np.abs(got[ok, 6] - sf["ssim_levels"][ok, 4]).max()}
    print("images compared", int(ok.sum()), "max errors", err)
    assert max(err.values()) <= 1e-4, err
    # the same rows whatever the piece size, and the pooled loss of the 68 as one batch
    vae68, _, _ = scoring_vae(68)
    assert np.abs(vae68.score(x, pred).cpu().numpy() - rows.cpu().numpy())[:, :7].max() <= 1e-6
    fx = real_fixture()
    ds = E.DeviceDataset(torch.from_numpy(fx["u8"][sf["index"]].copy()).cuda(), pred.clone(), np.stack([np.zeros(68, np.int64), np.arange(68)], 1))
    r = FusedTrainer(vae68).evaluate(ds, 68)
    pooled = np.array([r["total_loss"], r["recon_loss"], r["KLD"]] + r["ssim_levels"] + r["cs_levels"])
    print("pooled", pooled[:3], "reference", sf["pooled"][:3])
    assert np.abs(pooled - sf["pooled"]).max() <= 1e-4


def msssim64(recon, x):
    """MSSIM.forward in float64 (the oracle's level function on double tensors)."""
    window = orc.ms_window_2d(3).double()
    w = torch.tensor(orc.MS_WEIGHTS, dtype=torch.float64)
    a, b, sims, css = recon.double(), x.double(), [], []
    for _ in range(5):
        s, c = orc.ssim_level(a, b, window)
        sims.append(s); css.append(c)
        a, b = torch.nn.functional.avg_pool2d(a, (2, 2)), torch.nn.functional.avg_pool2d(b, (2, 2))
    sims, css = torch.stack(sims), torch.stack(css)
    return (1 - torch.prod((css ** w)[:-1] * (sims ** w)[-1])).item(), sims[0].item(), sims[4].item()


def test_score_in_bf16_mode_matches_its_own_forward():
    """The rows of a bf16-mode VAE against a float64 recomputation from the recon, mu, logvar its own eval-mode forward returned."""
    vae, x, pred = scoring_vae(68, "bf16")
    rows = entry(vae, "score")(x, pred).cpu().numpy().astype(np.float64)
    mu, logvar = torch.empty(68, 32, device="cuda"), torch.empty(68, 32, device="cuda")
    recon, zero = torch.empty(68, 3, 64, 64, device="cuda"), torch.zeros(68, 32, device="cuda")
    vae.handle.forward(68, x, pred, zero, vae.theta.data, vae.bn_state, mu, logvar, recon, vae._workspace(68), train=False)
    recon, mu, logvar, xc = recon.cpu(), mu.cpu().double(), logvar.cpu().double(), x.cpu()
    kld = (0.001 * -0.5 * (1 + logvar - mu ** 2 - logvar.exp()).sum(1)).numpy()
    want = np.array([msssim64(recon[i:i + 1], xc[i:i + 1]) for i in range(68)])
    d = (recon.double() - xc.double()).flatten(1)
    err = {"msssim": np.abs(rows[:, 1] - want[:, 0]).max(), "kld": np.abs(rows[:, 2] - kld).max(),
           "ssim0": np.abs(rows[:, 5] - want[:, 1]).max(), "ssim4": np.abs(rows[:, 6] - want[:, 2]).max(),
           "mse": np.abs(rows[:, 3] - (d ** 2).mean(1).numpy()).max()}
    print("bf16 rows against float64 of its own forward:", err)
    assert np.isfinite(want).all() and max(err.values()) <= 1e-4, err
    assert np.array_equal(rows[:, 4].astype(np.float32), d.abs().max(1).values.numpy().astype(np.float32))
