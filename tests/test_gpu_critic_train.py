"""cvae_critic_grad and CriticTrainer on the device (csrc/critic_train.hip, critic_train.py) against the torch-CPU
restatement tests/critic_train_ref.py, which tests/golden/make_critic_train_golden.py pins to the reference's own Critic
class.  Smallest shapes at which the kernel can go wrong: B = 1, 5 and 37 (ragged against any power-of-two blocking, more
than one workgroup, and — under CVAE_PERSIST_MAXWG — several images per workgroup), and B = 256, 257 and 300 around the
grid clamp at 256 workgroups: from 257 on some workgroups walk two images, the scratch holds 256 partials and not B, and the
finalize takes a second trip over the loss terms."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_train_ref as ref                                  # noqa: E402
import critic_train_tools as T                                  # noqa: E402
from critic_vae_amd import lib as cvlib                         # noqa: E402
from critic_vae_amd import synth                                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = T.DEV
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return T.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def handle():
    return T.make_handle()


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(77)
    w = synth.make_critic_params(0)
    return dict(w=w, flat=ref.flatten(w).astype(np.float32), x=rng.random((37, 3, 64, 64), dtype=np.float32),
                target=rng.random(37, dtype=np.float32), keep=(rng.random((37, cvlib.CRITIC_KEEP)) >= 0.3).astype(np.uint8))


@pytest.fixture(scope="module")
def noise300():
    """300 noise images for the batches past the grid clamp (MAX_GRID = 256 workgroups, critic_train.hip)."""
    rng = np.random.default_rng(300)
    w = synth.make_critic_params(0)
    return dict(w=w, flat=ref.flatten(w).astype(np.float32), x=rng.random((300, 3, 64, 64), dtype=np.float32),
                target=rng.random(300, dtype=np.float32), keep=(rng.random((300, cvlib.CRITIC_KEEP)) >= 0.3).astype(np.uint8))


def _inputs(fx, noise, source):
    if source == "real":
        return fx["w"], fx["flat"], fx["x"], fx["z"]["target"], fx["z"]["keep"]
    return noise["w"], noise["flat"], noise["x"], noise["target"], noise["keep"]


# (dropout_p, keep given)
MODES = {"p0.3-keep": (0.3, True), "p0.3-null": (0.3, False), "p0-null": (0.0, False), "p0-keep": (0.0, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("loss", ["bce", "mse"])
@pytest.mark.parametrize("source", ["real", "noise"])
@pytest.mark.parametrize("B", [1, 5, 37])
def test_parity_with_imposed_decisions(fx, noise, handle, B, source, loss, mode):
    """pred / loss within 1e-5, every gradient tensor within 1e-4 of its max, against the fp64 restatement following the
    kernel's own decisions; a decision that differs from the fp64 free choice must be a tie within 4 E_l."""
    w, flat, x, target, keep = _inputs(fx, noise, source)
    p, given = MODES[mode]
    k = keep[:B] if given else None
    res = T.run_kernel(handle, flat, x[:B], target[:B], k, p, loss)
    T.imposed_parity(res, w, x[:B], target[:B], k, p, loss, f"B={B} {source} {loss} {mode}")


@pytest.mark.parametrize("loss", ["bce", "mse"])
@pytest.mark.parametrize("B", [256, 257, 300])
def test_parity_past_the_grid(noise300, handle, B, loss):
    """The method and bounds of test_parity_with_imposed_decisions at the grid clamp: 256 images in 256 workgroups, 257 and
    300 in 256 workgroups of which the first B - 256 walk two images (the scratch then holds 256 partials, the loss terms
    start after them, and the finalize sums the terms in two trips).  Measured on the MI355X, worst of the six
    cases: |d pred| 5.3e-08, |d loss| 3.7e-08, gradient gap 1.1e-06 of a tensor's max, no decision flips; the fp32 CPU
    restatement's own gap to the fp64 one at B = 300 is 4.7e-08 / 2.3e-08 / 7.6e-06, so PRED_TOL and GRAD_TOL stay."""
    n = noise300
    res = T.run_kernel(handle, n["flat"], n["x"][:B], n["target"][:B], n["keep"][:B], 0.3, loss)
    if "CVAE_PERSIST_MAXWG" not in os.environ:
        assert res["partials_written"] == min(B, 256)
    if B > 256:
        assert res["partials_written"] < B
    T.imposed_parity(res, n["w"], n["x"][:B], n["target"][:B], n["keep"][:B], 0.3, loss, f"B={B} noise {loss} p0.3-keep")


@pytest.mark.parametrize("B", [1, 255, 256, 257, 300])
def test_scratch_bytes_follow_the_grid_clamp(handle, B):
    """min(B, 256) partials of 11 876 floats, then the (2, B) loss terms, rounded up to 256 bytes (host only)."""
    assert cvlib.CRITIC_TRAIN_FLOATS == 11876
    want = -(-((min(B, 256) * 11876 + 2 * B) * 4) // 256) * 256
    assert handle.critic_grad_scratch_bytes(B) == want


@pytest.mark.parametrize("loss", ["bce", "mse"])
@pytest.mark.parametrize("B", [5, 37])
def test_against_reference_fixture(fx, handle, B, loss):
    """The reference class's own train-mode step (critic_train_real.npz), when the kernel took the same decisions."""
    z = fx["z"]
    p = float(z["dropout_p"])
    res = T.run_kernel(handle, fx["flat"], fx["x"][:B], z["target"][:B], z["keep"][:B], p, loss)
    differ = int((res["decisions"] != z["decisions"][:B]).sum())
    if differ == 0:
        T.compare(res, z[f"b{B}/{loss}/pred"], z[f"b{B}/{loss}/scalars"], z[f"b{B}/{loss}/grads"], loss, f"fixture B={B} {loss}")
    else:
        T.imposed_parity(res, fx["w"], fx["x"][:B], z["target"][:B], z["keep"][:B], p, loss,
                         f"fixture B={B} {loss}: {differ} decisions differ from the fixture's, compared in the imposed form")


@pytest.mark.parametrize("source", ["real", "noise"])
def test_eval_consistency(fx, noise, handle, source):
    """keep = NULL, dropout_p = 0 is the eval-mode forward: pred agrees with cvae_critic_forward within 1e-6."""
    _, flat, x, target, _ = _inputs(fx, noise, source)
    res = T.run_kernel(handle, flat, x, target, None, 0.0, "bce", decisions=False)
    pred = torch.empty(37, 1, device=DEV)
    handle.critic_forward(37, torch.from_numpy(x).to(DEV), torch.from_numpy(flat).to(DEV), pred)
    gap = float(np.abs(res["pred"] - pred.cpu().numpy()).max())
    print(f"eval consistency ({source}): max |d pred| {gap:.2e}")
    assert gap <= 1e-6


@pytest.mark.parametrize("B", [1, 5])
def test_saturated_sigmoid(fx, handle, B):
    """crit.4.bias pushed until p == 1.0f: the BCE term is 100 (1 - t), every gradient is exactly 0 (torch's arithmetic:
    d_z = d_p * p (1 - p) with p (1 - p) == 0), nothing is NaN."""
    w = dict(fx["w"])
    w["crit.4.bias"] = np.array([64.0], np.float32)
    flat = ref.flatten(w).astype(np.float32)
    target = np.array([0.25, 0.5, 1.0, 0.0, 0.75], np.float32)[:B]             # 100 (1 - t) and its mean are exact in fp32
    for loss in ("bce", "mse"):
        res = T.run_kernel(handle, flat, fx["x"][:B], target, None, 0.3, loss)
        assert (res["pred"] == 1.0).all()
        assert np.isfinite(res["scalars"]).all() and not np.isnan(res["grads"]).any()
        assert (res["grads"] == 0).all(), f"{loss}: a saturated image contributed {np.abs(res['grads']).max():.3e}"
        assert abs(float(res["scalars"][1]) - float(np.mean(100.0 * (1.0 - target.astype(np.float64))))) <= 1e-5
        assert abs(float(res["scalars"][2]) - float(np.mean((1.0 - target.astype(np.float64)) ** 2))) <= 1e-5
    r = ref.step(w, fx["x"][:B], target, None, 0.3, "bce")                      # torch gives the same
    assert (r["flat_grads"] == 0).all() and abs(r["bce"] - float(res["scalars"][1])) <= 1e-5


@pytest.mark.parametrize("B", [37, 257])
def test_determinism_and_hygiene(fx, noise300, handle, B):
    """Same bits twice; NaN bytes in scratch, grads and decisions before the call change nothing; padding zero; 64 KB guard
    bands after grads, pred, decisions and scratch untouched.  B = 257 (noise images): the scratch is clamped to 256 partials,
    so the band starts right after the loss terms that follow them, and the terms region is NaN before the third call."""
    z, G = fx["z"], 65536
    sizes = dict(grads=cvlib.CRITIC_TRAIN_FLOATS * 4, pred=B * 4, dec=B * cvlib.CRITIC_DECISIONS,
                 scratch=handle.critic_grad_scratch_bytes(B))
    buf = {k: torch.empty(n + G, dtype=torch.uint8, device=DEV) for k, n in sizes.items()}
    if B == 37:
        src = dict(x=fx["x"], target=z["target"], keep=z["keep"], flat=fx["flat"])
    else:
        src = {k: noise300[k][:B] if k != "flat" else noise300[k] for k in ("x", "target", "keep", "flat")}
    x, target = torch.from_numpy(src["x"]).to(DEV), torch.from_numpy(src["target"]).to(DEV)
    keep, flat = torch.from_numpy(src["keep"]).to(DEV), torch.from_numpy(src["flat"]).to(DEV)
    assert x.shape[0] == target.shape[0] == keep.shape[0] == B
    scal = torch.empty(4, device=DEV)

    def call(fill):
        for k, t in buf.items():
            t[:sizes[k]] = fill
            t[sizes[k]:] = 0xA5
        scal.fill_(float("nan"))
        handle.critic_grad(B, x, target, keep, 0.3, 0, flat, buf["grads"][:sizes["grads"]].view(torch.float32),
                           buf["pred"][:sizes["pred"]].view(torch.float32), scal, buf["scratch"],
                           decisions=buf["dec"][:sizes["dec"]])
        torch.cuda.synchronize()
        for k, t in buf.items():
            assert (t[sizes[k]:] == 0xA5).all(), f"guard band after {k} was written"
        return [buf[k][:sizes[k]].cpu().numpy().copy() for k in ("grads", "pred", "dec")] + [scal.cpu().numpy().copy()]

    a, b, c = call(0x00), call(0x00), call(0xFF)             # 0xFF bytes: NaN floats
    for i, name in enumerate(("grads", "pred", "decisions", "scalars")):
        assert np.array_equal(a[i].view(np.uint8), b[i].view(np.uint8)), f"{name}: two calls differ"
        assert np.array_equal(a[i].view(np.uint8), c[i].view(np.uint8)), f"{name}: depends on what the buffers held before"
    g = a[0].view(np.float32)
    assert (g[ref.N_PARAMS:] == 0).all() and np.isfinite(g).all() and np.abs(g).max() > 0


def test_several_images_per_workgroup(fx, handle, tmp_path):
    """The grid is persistent: CVAE_PERSIST_MAXWG=8 in a fresh child process walks B = 37 in 8 workgroups (4 or 5 images
    each).  Same decisions and pred; gradients bitwise, or within 1e-4 of each tensor's max (another partial order)."""
    out = str(tmp_path / "capped.npz")
    env = dict(os.environ, CVAE_PERSIST_MAXWG="8")
    r = subprocess.run([sys.executable, os.path.join(HERE, "critic_train_worker.py"), out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    capped = np.load(out)
    z = fx["z"]
    for loss in ("bce", "mse"):
        res = T.run_kernel(handle, fx["flat"], fx["x"], z["target"], z["keep"], float(z["dropout_p"]), loss)
        # the cap took effect: the child wrote 8 per-workgroup partials into scratch (4 or 5 images each)
        assert int(capped[f"{loss}/partials_written"]) == 8, f"the child ran {int(capped[f'{loss}/partials_written'])} workgroups"
        if "CVAE_PERSIST_MAXWG" not in os.environ:
            assert res["partials_written"] == 37
        assert np.array_equal(res["decisions"], capped[f"{loss}/decisions"]) and np.array_equal(res["pred"], capped[f"{loss}/pred"])
        if not np.array_equal(res["grads"], capped[f"{loss}/grads"]):
            cap = {k: capped[f"{loss}/{k}"] for k in ("grads", "pred", "scalars")}
            T.compare(cap, res["pred"], (res["scalars"][1], res["scalars"][2]), res["grads"][:ref.N_PARAMS].astype(np.float64), loss,
                      f"8 workgroups vs 37, {loss}")


def _critic(handle, w):
    from critic_vae_amd.critic import Critic
    critic = Critic(handle=handle).to(DEV)
    critic.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()})
    return critic


def test_trajectory_against_fp64_curve(fx, handle):
    """CriticTrainer, 40 steps at B = 37 with the fixture's keep sequence: the loss curve within max(10 x the fp32 CPU
    restatement's own worst gap to the fp64 curve, 1e-5); the trained critic evaluates as the restatement does on its final
    parameters; its state_dict is the reference's checkpoint format."""
    from critic_vae_amd.critic import CRITIC_KEYS, Critic
    from critic_vae_amd.critic_train import CriticTrainer
    z = fx["z"]
    critic = _critic(handle, fx["w"])
    tr = CriticTrainer(critic, lr=float(z["lr"]), dropout=float(z["dropout_p"]), loss="bce")
    keeps = np.unpackbits(z["traj/keep_bits"], axis=1).reshape(40, 37, cvlib.CRITIC_KEEP)
    x, target = torch.from_numpy(fx["x"]).to(DEV), torch.from_numpy(z["target"]).to(DEV)
    d_keeps = torch.from_numpy(keeps).to(DEV)
    curve = torch.empty(40, 4, device=DEV)
    for s in range(40):
        curve[s].copy_(tr.step(x, target, keep=d_keeps[s]))
    curve = curve.cpu().numpy().astype(np.float64)
    bound = max(10 * float(z["traj/gap32"]), 1e-5)
    gap = float(np.abs(curve[:, 0] - z["traj/loss64"]).max())
    print(f"trajectory: loss {curve[0, 0]:.6f} -> {curve[-1, 0]:.6f}; worst gap to the fp64 curve {gap:.3e} (bound {bound:.1e})")
    assert gap <= bound
    assert tr.step_count == 40 and critic.flat.data_ptr() == tr.theta.data_ptr()
    sd = critic.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, s) for k, s in CRITIC_KEYS]
    final = {k: v.cpu().numpy() for k, v in sd.items()}
    got = critic.evaluate(x).cpu().numpy()
    e_own = float(np.abs(got - ref.eval_forward(final, fx["x"], torch.float64)).max())
    e_fix = float(np.abs(got - ref.eval_forward(ref.unflatten(z["traj/params64"], np.float64), fx["x"], torch.float64)).max())
    print(f"eval after training: vs the restatement on the device's parameters {e_own:.2e}, on the fixture's fp64 parameters {e_fix:.2e}; "
          f"max parameter gap {np.abs(ref.flatten(final) - z['traj/params64']).max():.2e}")
    assert e_own <= 1e-5 and e_fix <= 1e-5
    other = Critic(handle=handle).to(DEV)
    other.load_state_dict(sd)
    assert torch.equal(other.flat, critic.flat)
    st = tr.state_dict()
    assert st["step_count"] == 40 and torch.equal(st["flat"], critic.flat.cpu()) and st["m"].numel() == cvlib.CRITIC_TRAIN_FLOATS


def test_guarded_step_skips_nan_target(fx, handle):
    from critic_vae_amd.critic_train import CriticTrainer
    z = fx["z"]
    critic = _critic(handle, fx["w"])
    tr = CriticTrainer(critic, dropout=0.3, skip_nonfinite=True)
    x, target = torch.from_numpy(fx["x"]).to(DEV), torch.from_numpy(z["target"]).to(DEV)
    keep = torch.from_numpy(z["keep"]).to(DEV)
    tr.step(x, target, keep=keep)
    before = [t.clone() for t in (tr.theta, tr.m, tr.v)]
    bad = target.clone()
    bad[11] = float("nan")
    tr.step(x, bad, keep=keep)
    torch.cuda.synchronize()
    for was, now in zip(before, (tr.theta, tr.m, tr.v)):
        assert torch.equal(was.view(torch.int32), now.view(torch.int32))
    st = tr.guard_stats()
    assert st["applied"] == 1 and st["skipped"] == 1
    tr.step(x, target, keep=keep)
    assert tr.guard_stats()["applied"] == 2 and not torch.equal(before[0], tr.theta)


def test_fit_device_end_to_end(handle):
    """3 synthetic trajectories of 40 frames -> critic_dataset -> fit_device (batch 32, 2 epochs, ragged last batch): the
    losses are those of a hand loop of step() over the same indices and masks, bit for bit; curate() takes the trained critic."""
    from critic_vae_amd import episodes as E
    from critic_vae_amd.critic_train import CriticTrainer
    rng = np.random.default_rng(9)
    eps = [(f"t{i}", rng.integers(0, 256, (40, 64, 64, 3), dtype=np.uint8)) for i in range(3)]
    rewards = {name: (rng.random(40) < 0.1).astype(np.float64) for name, _ in eps}
    ds = E.critic_dataset(eps, rewards, seed=1, device=DEV)
    assert len(ds) == 120 and ds.preds.shape == (120, 1)
    tg = np.stack([E.discounted_targets(rewards[eps[t][0]])[f] for t, f in ds.source])
    assert np.array_equal(ds.preds.cpu().numpy()[:, 0], tg) and 0 <= tg.min() and tg.max() <= 1
    assert np.array_equal(ds.frames.cpu().numpy(), np.stack([eps[t][1][f] for t, f in ds.source]))
    w = synth.make_critic_params(3)

    critic = _critic(handle, w)
    tr = CriticTrainer(critic)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    np.random.seed(5)
    log = tr.fit_device(ds, 32, epochs=2, generator=gen).cpu().numpy()
    assert log.shape == (8, 4) and np.isfinite(log).all()

    critic2 = _critic(handle, w)
    tr2 = CriticTrainer(critic2)
    gen.manual_seed(5)
    np.random.seed(5)
    x, target, hand = torch.empty(32, 3, 64, 64, device=DEV), torch.empty(32, 1, device=DEV), []
    for _ in range(2):
        idx = np.arange(120)
        np.random.shuffle(idx)
        d_idx = torch.from_numpy(idx).to(DEV)
        for b in range(0, 120, 32):
            nb = min(32, 120 - b)
            handle.preprocess_u8_gather(nb, ds.frames, ds.preds, d_idx[b:b + nb], x[:nb], target[:nb])
            keep = tr2.draw_keep(nb, gen)
            hand.append(tr2.step(x[:nb], target[:nb], keep=keep).cpu().numpy().copy())
    assert np.array_equal(log.view(np.uint32), np.stack(hand).view(np.uint32))
    assert torch.equal(critic.flat, critic2.flat)
    curated = E.curate(eps, critic, collect=5, total_images=20, device=DEV, log=lambda *a: None)
    if len(curated):            # which frames a barely trained critic bins is not the point: its values drive the walk
        assert np.array_equal(curated.preds.cpu().numpy(), critic.evaluate(critic.preprocess(curated.frames)).cpu().numpy())


def test_critic_dataset_in_several_chunks(monkeypatch):
    """critic_dataset with the staging chunk cut to 16 frames: 120 frames travel in 7 full chunks and a ragged one through the
    two StagingSets in turn; frames and targets arrive in drawn order, as in one chunk."""
    from critic_vae_amd import episodes as E
    rng = np.random.default_rng(10)
    eps = [(f"t{i}", rng.integers(0, 256, (T, 64, 64, 3), dtype=np.uint8)) for i, T in enumerate((50, 3, 67))]
    rewards = {name: (rng.random(a.shape[0]) < 0.2).astype(np.float64) for name, a in eps}
    whole = E.critic_dataset(eps, rewards, seed=2, device=DEV)
    monkeypatch.setattr(E, "CRITIC_CHUNK", 16)
    for size in (None, 40, 16, 1):
        ds = E.critic_dataset(eps, rewards, size=size, seed=2, device=DEV)
        n = 120 if size is None else size
        assert len(ds) == n and np.array_equal(ds.source, whole.source[:n])
        assert torch.equal(ds.frames, whole.frames[:n]) and torch.equal(ds.preds, whole.preds[:n])
    assert np.array_equal(whole.frames.cpu().numpy(), np.stack([eps[t][1][f] for t, f in whole.source]))
    tg = np.stack([E.discounted_targets(rewards[eps[t][0]])[f] for t, f in whole.source])
    assert np.array_equal(whole.preds.cpu().numpy()[:, 0], tg)


def test_trainer_notices_a_moved_critic(fx, handle):
    from critic_vae_amd.critic_train import CriticTrainer
    critic = _critic(handle, fx["w"])
    tr = CriticTrainer(critic)
    critic.flat = critic.flat.clone()              # what critic.to(...) / .double() do: a new buffer
    with pytest.raises(RuntimeError, match="no longer"):
        tr.step(torch.from_numpy(fx["x"][:5]).to(DEV), torch.from_numpy(fx["z"]["target"][:5]).to(DEV))
