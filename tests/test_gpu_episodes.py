"""Dataset curation and the device batch gather on the MI355X (critic_vae_amd.episodes, dataset.hip): cvae_curate_select
against the plain restatement of load_minerl_data on adversarial critic values, curate() against what the reference's own
code selected from real frames (episodes_real.npz), the gathers bit for bit against cvae_preprocess_u8 and the critic,
addressing past 2^31 bytes, fit_device against fit_u8, and the -train --episodes CLI end to end."""
import os

import numpy as np
import pytest
import torch

from critic_vae_amd import episodes as E
from critic_vae_amd import train
from critic_vae_amd.critic import Critic
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
from dataset_ops_tools import device_select as _device_select
from recon_tools import first_vae_params

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "episodes_real.npz"))


@pytest.fixture(scope="module")
def pool(golden_dir):
    return np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]


@pytest.fixture(scope="module")
def critic_sd(golden_dir):
    cw = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    return {k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")}


def real_critic(critic_sd, handle=None):
    c = Critic(handle=handle).to(DEV)
    c.load_state_dict(critic_sd)
    return c


def fixture_trajectories(fx):
    offs = np.concatenate([[0], np.cumsum(fx["traj_len"])])
    return [fx["traj_idx"][offs[t]:offs[t + 1]] for t in range(len(fx["traj_len"]))]


# ---- 1. cvae_curate_select against the restatement ----

def _adversarial_trajectories():
    f = np.float32
    edges = [f(0.4), f(0.6), f(0.7), f(0.25)]
    vals = [v for e in edges for v in (np.nextafter(e, f(-1)), e, np.nextafter(e, f(2)))]
    vals += [f("nan"), f(0.0), f(-0.0), f(1.0), f(0.5), f(0.9), f(0.1), f(0.65)]
    vals = np.array(vals, np.float32)
    rng = np.random.default_rng(3)
    lengths = [0, 1, 149, 150, 151, 255, 256, 257, 0, 20000, 151, 1, 150, 149, 300]
    trajs = []
    for t, n in enumerate(lengths):
        if t % 3 == 2:                                   # long runs of one value: every bin reaches its cap
            a = np.repeat(rng.choice(vals, size=max(1, n // 40 + 1)), 40)[:n]
        else:
            a = rng.choice(vals, size=n)
        trajs.append(a.astype(np.float32))
    return trajs


def test_curate_select_matches_restatement():
    h = Handle(64, 1)
    trajs = _adversarial_trajectories()
    for collect in (1, 150, 10 ** 6):
        sizes_all, sel_all, _ = E.select_host(trajs, collect=collect, total_images=10 ** 9)
        boundary = sizes_all[6]                           # len(dset) exactly before trajectory 6
        for total in (0, boundary, boundary + 1, len(sel_all) + 1):
            sizes, ref_sel, ref_counts = E.select_host(trajs, collect=collect, total_images=total)
            ref_first = sizes + [-1] * (len(trajs) - len(sizes))
            for n_chunks in (1, 2, 5):
                got_sel, got_first, got_counts, running = _device_select(h, trajs, collect, total, n_chunks)
                case = (collect, total, n_chunks)
                assert got_sel == ref_sel, case
                assert got_first == ref_first, case
                np.testing.assert_array_equal(got_counts, ref_counts, err_msg=str(case))
                assert running == len(ref_sel), case


def test_curate_select_rejects_bad_arguments():
    h = Handle(64, 1)
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)          # noqa: E731
    preds = torch.zeros(4, device=DEV)
    with pytest.raises(Exception, match="collect"):
        h.curate_select(i64(2), preds, 0, 10, i64(1), i64(3), i64(1), i64(2), i64(4))
    with pytest.raises(Exception, match=">= 0"):
        h.curate_select(i64(2), preds, 1, -1, i64(1), i64(3), i64(1), i64(2), i64(4))


# ---- 2. curate() against the reference's own selection ----

@pytest.mark.parametrize("chunk_frames", [8192, 700])
def test_curate_matches_the_reference(fx, pool, critic_sd, chunk_frames):
    critic = real_critic(critic_sd)
    trajs = fixture_trajectories(fx)
    names = fx["traj_names"].tolist()
    episodes = [(n, pool[s]) for n, s in zip(names, trajs)]
    lines = []
    ds = E.curate(episodes, critic, collect=int(fx["collect"]), total_images=int(fx["total_images"]),
                  chunk_frames=chunk_frames, log=lines.append)
    assert ds.sizes == fx["sizes"].tolist()
    assert [f"total images = {s}" for s in fx["sizes"]] == [ln for ln in lines if ln.startswith("total images")]
    assert ds.names == [names[i] for i in fx["order"]][:len(fx["sizes"])]
    content = np.array([trajs[t][i] for t, i in ds.source], np.int64)
    np.testing.assert_array_equal(content, fx["dset_pool"])
    np.testing.assert_array_equal(ds.frames.cpu().numpy(), pool[content])
    # HIP critic values of the pool against the reference critic's, and the cached values are those values
    hip = E.DeviceDataset.from_host(pool, critic).preds.cpu().numpy()[:, 0]
    assert np.abs(hip - fx["pool_preds"]).max() < 2e-6
    np.testing.assert_array_equal(ds.preds.cpu().numpy()[:, 0], hip[content])


@pytest.mark.parametrize("kind", ["plain", "recon"])
def test_curate_empty_and_zero_total(pool, critic_sd, kind):
    critic = real_critic(critic_sd)
    if kind == "plain":
        def walk(eps, total):
            return E.curate(eps, critic, total_images=total, log=lambda s: None)
    else:
        vae = VariationalAutoencoder(max_batch=8, seed=7).to(DEV)
        vae.load_reference_params(first_vae_params(7))

        def walk(eps, total):
            return E.curate_recon(eps, critic, vae, total_images=total, log=lambda s: None)
    eps = [("a", pool[:0]), ("b", pool[:5])]
    assert len(walk(eps, 0)) == 0
    ds = walk([("a", pool[:0])], 10)
    assert len(ds) == 0 and ds.sizes == [0]
    if kind == "recon":
        assert ds.source.shape == (0, 3) and ds.stats == {"walked": 0, "encoded": 0, "decoded": 0}


# ---- 3. gathers ----

@pytest.mark.parametrize("w", [64, 128])
def test_preprocess_u8_gather_bitwise(w):
    rng = np.random.default_rng(w)
    n = 300
    frames = rng.integers(0, 256, size=(n, w, w, 3), dtype=np.uint8)
    preds = rng.random(n).astype(np.float32)
    ds = E.DeviceDataset.from_host(frames, preds)
    h = Handle(w, 256)
    for B in (1, 7, 128, 256, 77):
        idx = rng.integers(0, n, size=B)
        x = torch.full((B, 3, w, w), -1.0, device=DEV)
        p = torch.full((B, 1), -1.0, device=DEV)
        h.preprocess_u8_gather(B, ds.frames, ds.preds, torch.from_numpy(idx).to(DEV), x, p)
        ref = torch.empty(B, 3, w, w, device=DEV)
        h.preprocess_u8(B, torch.from_numpy(frames[idx]).to(DEV), ref)
        assert torch.equal(x.view(torch.int32), ref.view(torch.int32)), (w, B)
        np.testing.assert_array_equal(p.cpu().numpy()[:, 0], preds[idx])


def test_gathered_preds_equal_the_critic_on_the_batch(pool, critic_sd):
    critic = real_critic(critic_sd)
    ds = E.DeviceDataset.from_host(pool, critic)
    h = Handle(64, 256)
    rng = np.random.default_rng(0)
    for B in (1, 7, 128, 256, 77):
        idx = rng.integers(0, len(pool), size=B)
        x = torch.empty(B, 3, 64, 64, device=DEV)
        p = torch.empty(B, 1, device=DEV)
        h.preprocess_u8_gather(B, ds.frames, ds.preds, torch.from_numpy(idx).to(DEV), x, p)
        q = torch.empty(B, 1, device=DEV)
        h.critic_forward(B, x, critic.flat, q)
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), B


def test_gather_width_must_match_the_handle():
    ds = E.DeviceDataset.from_host(np.zeros((4, 64, 64, 3), np.uint8))
    h = Handle(128, 8)
    with pytest.raises(Exception, match="width"):
        h.preprocess_u8_gather(2, ds.frames, ds.preds, torch.zeros(2, dtype=torch.int64, device=DEV),
                               torch.empty(2, 3, 128, 128, device=DEV), torch.empty(2, 1, device=DEV))


# ---- 4. past 2^31 bytes ----

def _pattern(first, n):
    i = torch.arange(first, first + n, device=DEV, dtype=torch.int64)[:, None]
    j = torch.arange(64 * 64 * 3, device=DEV, dtype=torch.int64)[None, :]
    return ((i * 7 + j * 13 + (i * j) % 5) % 251).to(torch.uint8).view(n, 64, 64, 3)


def test_gathers_past_2_31_bytes():
    fb = 64 * 64 * 3
    n = 174763 + 40                                       # 2^31 / 12288 = 174762.67 frames
    assert n * fb > 2 ** 31
    frames = torch.empty(n, 64, 64, 3, dtype=torch.uint8, device=DEV)
    for p in range(0, n, 4096):
        frames[p:p + 4096] = _pattern(p, min(4096, n - p))
    preds = torch.arange(n, dtype=torch.float32, device=DEV).view(n, 1)
    straddle = 2 ** 31 // fb                              # the frame that holds byte 2^31
    assert straddle * fb < 2 ** 31 < (straddle + 1) * fb
    idx = np.array([n - 1, straddle, straddle - 1, straddle + 1, n - 2, 0, n - 40], np.int64)
    B = len(idx)
    h = Handle(64, 16)
    x = torch.empty(B, 3, 64, 64, device=DEV)
    p = torch.empty(B, 1, device=DEV)
    h.preprocess_u8_gather(B, frames, preds, torch.from_numpy(idx).to(DEV), x, p)
    src = torch.cat([_pattern(int(i), 1) for i in idx])
    ref = torch.empty(B, 3, 64, 64, device=DEV)
    h.preprocess_u8(B, src, ref)
    assert torch.equal(x, ref)
    assert p[:, 0].cpu().tolist() == idx.astype(np.float32).tolist()
    # gather_frames_u8 reading past 2^31 (big source) and writing past 2^31 (big destination)
    sel = torch.from_numpy(idx).to(DEV)
    span = torch.tensor([0, B], dtype=torch.int64, device=DEV)
    small = torch.zeros(B, 64, 64, 3, dtype=torch.uint8, device=DEV)
    small_p = torch.zeros(B, 1, device=DEV)
    h.gather_frames_u8(frames, preds, sel, B, span, small, small_p)
    assert torch.equal(small, src) and torch.equal(small_p[:, 0].cpu(), torch.from_numpy(idx.astype(np.float32)))
    span = torch.tensor([straddle - 2, B], dtype=torch.int64, device=DEV)
    rev = torch.arange(B - 1, -1, -1, dtype=torch.int64, device=DEV)
    h.gather_frames_u8(small, small_p, rev, B, span, frames, preds)
    assert torch.equal(frames[straddle - 2:straddle - 2 + B], src.flip(0))
    assert torch.equal(frames[straddle - 3], _pattern(straddle - 3, 1)[0])
    assert torch.equal(frames[straddle - 2 + B], _pattern(straddle - 2 + B, 1)[0])


# ---- 5. fit_device == fit_u8 ----

@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_device_equals_fit_u8(pool, critic_sd, precision):
    rng = np.random.default_rng(1)
    frames = np.concatenate([pool, pool[rng.permutation(len(pool))][:32]])      # 100 frames: batches 32, 32, 32, 4
    B = 32
    out = []
    for mode in ("u8", "device"):
        vae = VariationalAutoencoder(max_batch=B, seed=5, precision=precision).to(DEV)
        tr = FusedTrainer(vae)
        critic = real_critic(critic_sd, handle=vae.handle)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(9)
        np.random.seed(123)
        if mode == "u8":
            scal = tr.fit_u8(frames, critic, B, epochs=2, generator=gen)
        else:
            scal = tr.fit_device(E.DeviceDataset.from_host(frames, critic), B, epochs=2, generator=gen)
        torch.cuda.synchronize()
        out.append({"theta": vae.theta.detach().clone(), "m": tr.m.clone(), "v": tr.v.clone(),
                    "bn": vae.bn_state.clone(), "scal": scal.clone(), "steps": tr.step_count})
    a, b = out
    assert a["steps"] == b["steps"] == 8
    for k in ("theta", "m", "v", "bn", "scal"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ---- 6. the CLI end to end ----

def test_cli_trains_on_episodes(tmp_path, fx, pool, critic_sd, capsys):
    trajs = fixture_trajectories(fx)
    names = ["ep_a", "ep_b", "ep_c"]
    seqs = [trajs[0][:300], trajs[2][:120], trajs[6][:200]]
    d = tmp_path / "eps"
    d.mkdir()
    for n, s in zip(names, seqs):
        np.save(d / f"{n}.npy", pool[s])
    pt = tmp_path / "critic.pt"
    torch.save(critic_sd, pt)
    save = tmp_path / "out"
    total, collect = 150, 40
    train.main(["-train", "--episodes", str(d), "--critic", str(pt), "--epochs", "1", "--batch", "32",
                "--total-images", str(total), "--collect", str(collect), "--save", str(save)])
    text = capsys.readouterr().out
    order = E.reference_order(names)
    _, sel, _ = E.select_host([fx["pool_preds"][seqs[names.index(n)]] for n in order], collect=collect, total_images=total)
    assert f"curated {len(sel)} frames" in text
    vae = VariationalAutoencoder(max_batch=4, seed=99)
    enc = torch.load(save / train.ENCODER_FILE)
    dec = torch.load(save / train.DECODER_FILE)
    vae.encoder.load_state_dict(enc, strict=True)
    vae.decoder.load_state_dict(dec, strict=True)
    # bit patterns: the generator's seed-0 weights give NaN gradients on real frames, in the reference as here
    # (test_gpu_step.py), so a trained model may hold NaN
    bits = lambda t: t.detach().cpu().reshape(-1).view(torch.uint8)                       # noqa: E731
    for k, v in vae.encoder.state_dict().items():
        assert torch.equal(bits(v), bits(enc[k])), k
    for k, v in vae.decoder.state_dict().items():
        assert torch.equal(bits(v), bits(dec[k])), k
    assert set(enc) == set(VariationalAutoencoder(max_batch=4, seed=0).encoder.state_dict())
