"""The second VAE's dataset and training on the MI355X (critic_vae_amd.episodes.curate_recon, dataset.hip):
cvae_curate_select_recon against the plain restatement of the recon branch of load_minerl_data, curate_recon against what
the reference's own code built from real frames (recon_real.npz), the encoder-once structure, the cached critic values,
cvae_gather_f32 bit for bit (past 2^31 bytes too), fit_device on a ReconDataset against step(), the reference's `-second`
loss curve, save / load and the -dataset / -second / -video --second CLI end to end."""
import os

import numpy as np
import pytest
import torch

from critic_vae_amd import episodes as E
from critic_vae_amd import segment
from critic_vae_amd import synth
from critic_vae_amd import train
from critic_vae_amd.critic import Critic
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
from dataset_ops_tools import device_select_recon as _device_select_recon
from oracle import cvae_oracle as orc
from recon_tools import SAMPLE_STRIDE, first_vae_params, sample_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4                    # the project's fp32 parity bound (test_gpu_step.TOL, test_inference_path_eval_mode)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "recon_real.npz"))


@pytest.fixture(scope="module")
def ep(golden_dir):
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


def first_vae(fx, max_batch=128):
    vae = VariationalAutoencoder(max_batch=max_batch, seed=int(fx["wseed"])).to(DEV)
    vae.load_reference_params(first_vae_params(int(fx["wseed"])))
    return vae.eval()


def fixture_trajectories(ep):
    offs = np.concatenate([[0], np.cumsum(ep["traj_len"])])
    return [ep["traj_idx"][offs[t]:offs[t + 1]] for t in range(len(ep["traj_len"]))]


@pytest.fixture(scope="module")
def built(fx, ep, pool, critic_sd):
    """curate_recon on the fixture at two chunk sizes, with the frames every eval-mode forward was handed."""
    out = {}
    trajs = fixture_trajectories(ep)
    names = ep["traj_names"].tolist()
    episodes = [(n, pool[s]) for n, s in zip(names, trajs)]
    for chunk_frames in (8192, 700):
        vae = first_vae(fx)
        critic = real_critic(critic_sd)
        encoded = []
        orig = vae.handle.forward

        def counting(B, *a, _orig=orig, **k):
            encoded.append(B)
            return _orig(B, *a, **k)

        vae.handle.forward = counting
        lines = []
        ds = E.curate_recon(episodes, critic, vae, collect=int(fx["collect"]), total_images=int(fx["total_images"]),
                            chunk_frames=chunk_frames, log=lines.append)
        vae.handle.forward = orig
        out[chunk_frames] = {"ds": ds, "vae": vae, "critic": critic, "encoded": encoded, "lines": lines, "trajs": trajs,
                             "names": names}
    return out


# ---- 1. cvae_curate_select_recon against the restatement ----

def _adversarial_trajectories():
    f = np.float32
    edges = [f(0.4), f(0.6), f(0.7), f(0.25)]
    vals = [v for e in edges for v in (np.nextafter(e, f(-1)), e, np.nextafter(e, f(2)))]
    vals += [f("nan"), f(0.0), f(-0.0), f(1.0), f(0.5), f(0.9), f(0.1), f(0.65)]
    vals = np.array(vals, np.float32)
    rng = np.random.default_rng(4)
    trajs = [np.full(400, 0.5, np.float32),                # all mid, past the cap
             np.zeros(0, np.float32), np.array([0.5], np.float32), np.array([0.9], np.float32)]
    for t, n in enumerate([149, 150, 151, 255, 256, 257, 0, 20000, 151, 1, 300]):
        if t % 3 == 2:                                     # long runs of one value: every bin reaches its cap
            a = np.repeat(rng.choice(vals, size=max(1, n // 40 + 1)), 40)[:n]
        else:
            a = rng.choice(vals, size=n)
        trajs.append(a.astype(np.float32))
    return trajs


def test_curate_select_recon_matches_restatement(fx, ep):
    h = Handle(64, 1)
    walk = [fixture_trajectories(ep)[t] for t in ep["order"]]
    cases = [([ep["pool_preds"][s] for s in walk], [int(fx["collect"])], [int(fx["total_images"])])]
    adv = _adversarial_trajectories()
    sizes_all, ent_all, _ = E.select_recon_host(adv, collect=150, total_images=10 ** 9)
    # cut in the first trajectory, exactly at a boundary, one past it, never
    cases.append((adv, [1, 150, 10 ** 6], [0, 1, sizes_all[6], sizes_all[6] + 1, len(ent_all) + 1]))
    for trajs, collects, totals in cases:
        for collect in collects:
            for total in totals:
                sizes, ref_ent, ref_counts = E.select_recon_host(trajs, collect=collect, total_images=total)
                ref_first = sizes + [-1] * (len(trajs) - len(sizes))
                for n_chunks in (1, 2, 5):
                    got_ent, got_first, got_counts, running = _device_select_recon(h, trajs, collect, total, n_chunks)
                    case = (len(trajs), collect, total, n_chunks)
                    assert got_ent == ref_ent, case
                    assert got_first == ref_first, case
                    np.testing.assert_array_equal(got_counts, ref_counts, err_msg=str(case))
                    assert running == len(ref_ent), case


# ---- 2. curate_recon against the reference's own dataset ----

@pytest.mark.parametrize("chunk_frames", [8192, 700])
def test_curate_recon_matches_the_reference(fx, ep, pool, critic_sd, built, chunk_frames):
    """sizes, entry count and (pool, kind) sequence exact; every entry within 1e-4 of the reference's reconstruction (its
    fixed sample, sum, min, max); entries of equal (pool, kind) bitwise equal to each other and to vae.diff_images on that
    frame at another batch size (a frame's result does not depend on the batch it ran in)."""
    b = built[chunk_frames]
    ds, vae, trajs = b["ds"], b["vae"], b["trajs"]
    assert ds.sizes == fx["sizes"].tolist()
    assert [f"total images = {s}" for s in fx["sizes"]] == [ln for ln in b["lines"] if ln.startswith("total images")]
    assert ds.names == [b["names"][i] for i in ep["order"]][:len(fx["sizes"])]
    assert len(ds) == len(fx["dset_pool"])
    content = np.array([trajs[t][i] for t, i, _ in ds.source], np.int64)
    np.testing.assert_array_equal(content, fx["dset_pool"])
    np.testing.assert_array_equal(ds.source[:, 2], fx["dset_kind"])
    got = ds.frames.cpu().numpy()
    assert got.shape == (len(ds), 3, 64, 64) and got.dtype == np.float32
    worst = 0.0
    for e, (p, k) in enumerate(zip(content, ds.source[:, 2])):
        s, total, lo, hi = sample_of(got[e])
        worst = max(worst, np.abs(s - fx["samples"][p, k]).max(), abs(lo - fx["stats"][p, k, 1]), abs(hi - fx["stats"][p, k, 2]),
                    abs(total - fx["stats"][p, k, 0]) / got[e].size)
    print(f"curate_recon (chunk_frames {chunk_frames}): max |entry - reference| over samples / min / max / mean = {worst:.2e}")
    assert worst < TOL
    # one frame, one result: the pool frames through diff_images at batch 68
    x = torch.empty(len(pool), 3, 64, 64, device=DEV)
    vae.handle.preprocess_u8(len(pool), torch.from_numpy(pool).to(DEV), x)
    p = real_critic(critic_sd, handle=vae.handle).evaluate(x)
    one, zero, _, _ = vae.diff_images(x, p)
    want = torch.stack([one, zero], 1)[torch.from_numpy(content).to(DEV), torch.from_numpy(ds.source[:, 2]).to(DEV)]
    diff = (ds.frames - want).abs().max().item()
    print(f"curate_recon (chunk_frames {chunk_frames}): max |entry - diff_images of its frame| = {diff:.2e}")
    assert torch.equal(ds.frames.view(torch.int32), want.view(torch.int32))


def test_encoder_runs_once_per_selected_frame(fx, built):
    for chunk_frames, b in built.items():
        ds = b["ds"]
        selected = len({(t, i) for t, i, _ in ds.source.tolist()})
        assert selected < len(ds)                                  # mid frames own two entries
        assert sum(b["encoded"]) == selected == ds.stats["encoded"] == int(ds.counts.sum()), chunk_frames
        assert ds.stats["decoded"] == len(ds) and ds.stats["walked"] >= selected


def test_recon_preds_are_the_critic_on_the_entries(built, critic_sd):
    ds, critic = built[8192]["ds"], built[8192]["critic"]
    h = Handle(64, 256)
    rng = np.random.default_rng(0)
    assert float(ds.frames.min()) < 0.0                            # inputs outside [0, 1]: new ground for the critic kernel
    for B in (1, 7, 256, 77):
        idx = rng.integers(0, len(ds), size=B)
        x = torch.empty(B, 3, 64, 64, device=DEV)
        p = torch.empty(B, 1, device=DEV)
        h.gather_f32(B, ds.frames, ds.preds, torch.from_numpy(idx).to(DEV), x, p)
        q = torch.empty(B, 1, device=DEV)
        h.critic_forward(B, x, critic.flat, q)
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), B
    want = orc.critic_forward({k: v.clone() for k, v in critic_sd.items()}, ds.frames.cpu())
    gap = (ds.preds.cpu() - want).abs().max().item()
    print(f"critic on the reconstructions: max |HIP - oracle| = {gap:.2e}")
    assert gap < 2e-6


# ---- 3. cvae_gather_f32 ----

@pytest.mark.parametrize("w", [64, 128])
def test_gather_f32_bitwise(w):
    g = torch.Generator(device=DEV)
    g.manual_seed(w)
    n = 300
    frames = torch.rand(n, 3, w, w, device=DEV, generator=g) * 2 - 1
    frames.view(torch.int32)[5, 1, 2, :4] = torch.tensor([0x7fc00001, -1, 0x00000001, -2 ** 31], dtype=torch.int32, device=DEV)
    preds = torch.rand(n, 1, device=DEV, generator=g)
    h = Handle(w, 256)
    rng = np.random.default_rng(w)
    for B in (1, 7, 128, 256, 77):
        idx = rng.integers(0, n, size=B)
        idx[0] = 5
        d_idx = torch.from_numpy(idx).to(DEV)
        x = torch.full((B, 3, w, w), -3.0, device=DEV)
        p = torch.full((B, 1), -3.0, device=DEV)
        h.gather_f32(B, frames, preds, d_idx, x, p)
        assert torch.equal(x.view(torch.int32), frames[d_idx].view(torch.int32)), (w, B)
        assert torch.equal(p.view(torch.int32), preds[d_idx].view(torch.int32)), (w, B)
    # an index outside [0, n): NaN image and NaN pred, neighbours intact, nothing past the batch written
    idx = np.array([3, n, 4, -1, 0], np.int64)
    x = torch.full((6, 3, w, w), -3.0, device=DEV)
    p = torch.full((6, 1), -3.0, device=DEV)
    h.gather_f32(5, frames, preds, torch.from_numpy(idx).to(DEV), x, p)
    for b, i in enumerate(idx):
        if 0 <= i < n:
            assert torch.equal(x[b], frames[i]) and torch.equal(p[b], preds[i])
        else:
            assert torch.isnan(x[b]).all() and torch.isnan(p[b]).all()
    assert (x[5] == -3.0).all() and (p[5] == -3.0).all()


def test_gather_f32_width_must_match_the_handle():
    h = Handle(128, 8)
    with pytest.raises(Exception, match="width"):
        h.gather_f32(2, torch.zeros(4, 3, 64, 64, device=DEV), torch.zeros(4, 1, device=DEV),
                     torch.zeros(2, dtype=torch.int64, device=DEV), torch.empty(2, 3, 128, 128, device=DEV),
                     torch.empty(2, 1, device=DEV))


def _pattern(first, n):
    i = torch.arange(first, first + n, device=DEV, dtype=torch.int64)[:, None]
    j = torch.arange(3 * 64 * 64, device=DEV, dtype=torch.int64)[None, :]
    return (((i * 7 + j * 13 + (i * j) % 5) % 2039).to(torch.float32) / 1024 - 1).view(n, 3, 64, 64)


def test_gather_f32_past_2_31_bytes():
    fb = 3 * 64 * 64 * 4
    n = 2 ** 31 // fb + 1 + 1100                          # 43 691 entries hold byte 2^31; about 2.2 GB in all
    assert 2 ** 31 < n * fb < 2.21e9
    frames = torch.empty(n, 3, 64, 64, device=DEV)
    for p in range(0, n, 2048):
        frames[p:p + 2048] = _pattern(p, min(2048, n - p))
    preds = torch.arange(n, dtype=torch.float32, device=DEV).view(n, 1)
    straddle = 2 ** 31 // fb                              # the entry that holds byte 2^31
    assert straddle * fb < 2 ** 31 < (straddle + 1) * fb
    idx = np.array([n - 1, straddle, straddle - 1, straddle + 1, n - 2, 0, straddle + 700, 17], np.int64)
    B = len(idx)
    h = Handle(64, 16)
    x = torch.empty(B, 3, 64, 64, device=DEV)
    p = torch.empty(B, 1, device=DEV)
    h.gather_f32(B, frames, preds, torch.from_numpy(idx).to(DEV), x, p)
    want = torch.cat([_pattern(int(i), 1) for i in idx])
    assert torch.equal(x, want)
    assert p[:, 0].cpu().tolist() == idx.astype(np.float32).tolist()


# ---- 4. fit_device on a ReconDataset == step() on torch-indexed batches ----

@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_device_recon_equals_step(precision):
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    n, B, epochs = 100, 32, 2                             # batches 32, 32, 32, 4
    frames = torch.rand(n, 3, 64, 64, device=DEV, generator=g) * 1.8 - 0.9
    preds = torch.rand(n, 1, device=DEV, generator=g)
    ds = E.ReconDataset(frames, preds, np.zeros((n, 3), np.int64))
    out = []
    for mode in ("device", "step"):
        vae = VariationalAutoencoder(max_batch=B, seed=5, precision=precision).to(DEV)
        tr = FusedTrainer(vae)
        gen = torch.Generator(device=DEV)
        gen.manual_seed(9)
        np.random.seed(123)
        if mode == "device":
            scal = tr.fit_device(ds, B, epochs=epochs, generator=gen)
        else:
            for _ in range(epochs):
                idx = np.arange(n)
                np.random.shuffle(idx)
                d_idx = torch.from_numpy(idx).to(DEV)
                for b in range(0, n, B):
                    sl = d_idx[b:b + B]
                    eps = torch.randn(sl.numel(), 32, device=DEV, generator=gen)
                    scal = tr.step(frames[sl].contiguous(), preds[sl].contiguous(), eps)
        torch.cuda.synchronize()
        out.append({"theta": vae.theta.detach().clone(), "m": tr.m.clone(), "v": tr.v.clone(),
                    "bn": vae.bn_state.clone(), "scal": scal.clone(), "steps": tr.step_count})
    a, b = out
    assert a["steps"] == b["steps"] == 8
    for k in ("theta", "m", "v", "bn", "scal"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


# ---- 5. the reference's -second curve ----

def test_second_vae_follows_the_references_curve(fx, built):
    """HIP training (fp32 mode) of a fresh VAE on the HIP-built first 128 entries, with the HIP critic's values of them,
    against the reference's modules + torch.optim.Adam on the reference-built entries (recon_real.npz, second_*): the whole
    curve within 5e-3 (as test_training_on_the_references_real_frames_fp32_and_bf16).  If the reference's curve
    ends in a non-finite step, the same step is non-finite here."""
    ds = built[8192]["ds"]
    B, steps, bad = int(fx["second_batch"]), int(fx["second_steps"]), int(fx["second_first_nonfinite_step"])
    ref = fx["second_traj"]
    x, pred = ds.frames[:2 * B].contiguous(), ds.preds[:2 * B].contiguous()
    pgap = np.abs(pred.cpu().numpy()[:, 0] - fx["second_preds"]).max()
    vae = VariationalAutoencoder(max_batch=B, seed=int(fx["second_wseed"])).to(DEV)
    tr = FusedTrainer(vae, lr=float(fx["second_lr"]))
    n_run = steps if bad < 0 else bad + 1
    assert len(ref) == n_run
    got = torch.empty(n_run, 3, device=DEV)
    for s in range(n_run):
        lo = B * (s % 2)
        eps = torch.from_numpy(synth.make_batch(int(fx["second_dseed"]), s, B)[2]).to(DEV)
        got[s] = tr.step(x[lo:lo + B], pred[lo:lo + B], eps)[:3]
    got = got.cpu().numpy()
    finite = n_run if bad < 0 else bad
    d01 = np.abs(got[:2] - ref[:2]).max()
    dall = np.abs(got[:finite] - ref[:finite]).max()
    print(f"-second, {n_run} steps at B = {B}: reference {ref[0, 0]:.5f} -> {ref[finite - 1, 0]:.5f}, here {got[finite - 1, 0]:.5f}; "
          f"first two steps {d01:.2e}, whole curve {dall:.2e}; critic values of the entries differ by {pgap:.2e}; "
          f"first non-finite step {bad}")
    assert np.isfinite(got[:finite]).all()
    if bad >= 0:
        assert not np.isfinite(got[bad]).all()
    assert dall < 5e-3


# ---- 6. save / load, the reference's list, the CLI ----

def test_save_load_and_reference_list(tmp_path, built):
    ds = built[700]["ds"]
    path = tmp_path / "recon.npz"
    ds.save(str(path))
    assert path.exists()
    back = E.ReconDataset.load(str(path), DEV)
    assert torch.equal(back.frames.view(torch.int32), ds.frames.view(torch.int32))
    assert torch.equal(back.preds.view(torch.int32), ds.preds.view(torch.int32))
    np.testing.assert_array_equal(back.source, ds.source)
    assert back.names == ds.names and back.sizes == ds.sizes
    np.testing.assert_array_equal(back.counts, ds.counts)
    ref = ds.to_reference_list()
    assert len(ref) == len(ds) and all(a.shape == (1, 3, 64, 64) and a.dtype == np.float32 for a in ref)
    stacked = np.stack(ref).squeeze()                              # train(): np.stack(dset).squeeze(), vae.py:37
    assert stacked.shape == (len(ds), 3, 64, 64) and np.array_equal(stacked, ds.frames.cpu().numpy())


def test_cli_dataset_second_and_video(tmp_path, capsys):
    rng = np.random.default_rng(2)
    d = tmp_path / "eps"
    d.mkdir()
    lengths = {"ep_a": 40, "ep_b": 25, "ep_c": 30}
    for name, n in lengths.items():
        blocks = rng.integers(0, 256, size=(n, 8, 8, 3), dtype=np.uint8)
        np.save(d / f"{name}.npy", np.kron(blocks, np.ones((1, 8, 8, 1), np.uint8)))
    nets = tmp_path / "nets"
    first = VariationalAutoencoder(max_batch=8, seed=3).to(DEV)
    train.save_networks(first, str(nets))
    out, pk = tmp_path / "recon.npz", tmp_path / "recon-dataset.pickle"
    total, collect = 60, 10
    ds = train.main(["-dataset", "--episodes", str(d), "--critic", "synth", "--networks", str(nets), "--out", str(out),
                     "--pickle", str(pk), "--total-images", str(total), "--collect", str(collect)])
    text = capsys.readouterr().out
    # the restatement on the device critic's own values of the frames
    critic = train._load_critic("synth", Handle(64, 64), 0, DEV)
    eps = E.load_episodes([str(d)])
    order = E.reference_order([n for n, _ in eps])
    by = dict(eps)
    vals = [E.DeviceDataset.from_host(np.asarray(by[n]), critic).preds.cpu().numpy()[:, 0] for n in order]
    _, ent, _ = E.select_recon_host(vals, collect=collect, total_images=total)
    assert len(ent) > 0 and len(ds) == len(ent) and f"built {len(ent)} entries" in text
    assert out.exists() and pk.exists()
    import pickle
    with open(pk, "rb") as f:
        lst = pickle.load(f)
    assert len(lst) == len(ent) and lst[0].shape == (1, 3, 64, 64) and lst[0].dtype == np.float32
    save = tmp_path / "second"
    train.main(["-second", "--dataset", str(out), "--critic", "synth", "--batch", "16", "--epochs", "1", "--save", str(save)])
    text = capsys.readouterr().out
    assert "images/s" in text
    assert (save / "vae2_encoder.pt").exists() and (save / "vae2_decoder.pt").exists()
    assert not (save / "vae_encoder.pt").exists()
    vae2 = train.load_networks(VariationalAutoencoder(max_batch=4, seed=99), str(save), second=True)
    enc = torch.load(save / "vae2_encoder.pt")
    bits = lambda t: t.detach().cpu().reshape(-1).view(torch.uint8)                       # noqa: E731
    for k, v in vae2.encoder.state_dict().items():
        assert torch.equal(bits(v), bits(enc[k])), k
    assert not torch.equal(bits(enc["model.0.weight"]), bits(VariationalAutoencoder(max_batch=4, seed=0).encoder.state_dict()["model.0.weight"]))
    # -evalsecond: segment -video --second reads vae2_*.pt (only those exist in `save`)
    n = 5000
    X = np.kron(rng.integers(0, 256, size=(n // 50, 8, 8, 3), dtype=np.uint8), np.ones((50, 8, 8, 1), np.uint8))
    Y = np.zeros((n, 64, 64, 3), np.uint8)
    Y[:, 16:48, 16:48] = 255
    np.save(tmp_path / "X.npy", X[:n])
    np.save(tmp_path / "Y.npy", Y)
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_critic_params(0).items()}, tmp_path / "critic.pt")
    argv = ["-video", "--frames", str(tmp_path / "X.npy"), "--gt", str(tmp_path / "Y.npy"), "--networks", str(save),
            "--critic", str(tmp_path / "critic.pt")]
    assert segment.main(argv + ["--second"]) == 0
    assert "thr_iou=" in capsys.readouterr().out
    with pytest.raises(FileNotFoundError):
        segment.main(argv)
