"""Generate tests/golden/recon_real.npz from the REFERENCE's own recon-dataset builder and training step (run only where
the reference checkout exists, like make_episode_golden.py).

    python tests/golden/make_recon_golden.py            # needs /root/reference (read-only)

Block 1 — `-dataset`: the reference's load_minerl_data(critic, recon_dset=True, vae=vae) (vae_utility.py:393-443) on CPU,
with the stand-ins of make_episode_golden.py (`minerl`, `denseCRF`, the font) and the same pool (the 68 real frames of
step_real_b68.npz), trajectories, order and real critic as episodes_real.npz.  The first VAE is the reference's
VariationalAutoencoder in eval mode with the generator-defined weights and BatchNorm running statistics of
tests/recon_tools.first_vae_params(WSEED), loaded through load_state_dict.  total_images is chosen so that the cut falls
inside the trajectory list AND the visited set differs from the non-recon walk at the same total_images (mid frames count
twice); both are asserted.

Block 2 — `-second`: the first 128 entries of that dataset, the reference critic on them, a fresh reference VAE from
synth.make_params(WSEED2), K Adam steps (lr 5e-5) at batch 64: step s trains on entries [64 (s % 2), 64 (s % 2) + 64) with
eps = synth.make_batch(DSEED2, s, 64)[2].  Targets in (-1, 1) can drive a cs level negative and the reference's MS-SSIM to
NaN: WSEED2 is searched over SEED_CANDIDATES until the curve is finite for all K steps; if none is, the first
candidate's finite prefix and first non-finite step are stored.

The fixture holds data only (no frames, no reference code):
  wseed, total_images, collect      what block 1 ran with
  sizes        (V,)  int64          len(dset) printed before each visited trajectory
  dset_pool    (N,)  int64          per entry, the pool frame it reconstructs
  dset_kind    (N,)  int64          0 = vae.evaluate(obs, p), 1 = vae.evaluate(obs, 0), recovered by matching each entry
                                    bit for bit against the reference's own evaluate of the pool frames
  samples      (68, 2, 127) f32     per (pool frame, kind): every 97th value of the reconstruction (NaN where the pair
  stats        (68, 2, 3)   f64     never occurs) and its sum / min / max
  second_*                          wseed2, dseed2, steps, lr, traj (K, 3) loss triples, first_nonfinite_step (-1: none),
                                    preds (128,) the reference critic's values of the first 128 entries
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
torch.set_num_threads(8)
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REF)

from make_episode_golden import _stub_modules          # noqa: E402
from recon_tools import SAMPLE_STRIDE, first_vae_params, sample_of          # noqa: E402
from critic_vae_amd import episodes as E               # noqa: E402
from critic_vae_amd import synth                       # noqa: E402

WSEED = 7
TOTAL_IMAGES = 1000
SEED_CANDIDATES = (21, 22, 23, 24, 25, 26, 27, 28)
DSEED2 = 4321
STEPS = 40
BATCH = 64


def load_reference_vae(vae_nets, params):
    v = vae_nets.VariationalAutoencoder()
    enc = {k[len("encoder."):]: torch.from_numpy(np.array(a)) for k, a in params.items() if k.startswith("encoder.")}
    dec = {k[len("decoder."):]: torch.from_numpy(np.array(a)) for k, a in params.items() if k.startswith("decoder.")}
    missing = v.encoder.load_state_dict(enc, strict=False)
    assert not missing.unexpected_keys and all("running" in k or "num_batches" in k for k in missing.missing_keys), missing
    v.decoder.load_state_dict(dec, strict=True)
    return v


def second_curve(vae_nets, lr, entries, preds, wseed2):
    v = load_reference_vae(vae_nets, synth.make_params(wseed2))
    v.train()
    opt = torch.optim.Adam(list(v.parameters()), lr=lr)
    traj, first_bad = [], -1
    orig = torch.randn_like
    for s in range(STEPS):
        lo = BATCH * (s % 2)
        eps = torch.from_numpy(synth.make_batch(DSEED2, s, BATCH)[2])
        torch.randn_like = lambda t, *a, **k: eps.clone()
        try:
            opt.zero_grad()
            out = v(entries[lo:lo + BATCH], preds[lo:lo + BATCH])
            losses = v.vae_loss(out[0], out[1], out[2], out[3])
            losses["total_loss"].backward()
            opt.step()
        finally:
            torch.randn_like = orig
        traj.append([losses["total_loss"].item(), losses["recon_loss"].item(), losses["KLD"].item()])
        if not np.isfinite(traj[-1]).all():
            first_bad = s
            break
    return np.array(traj, np.float32), first_bad


def main():
    ep = np.load(os.path.join(HERE, "episodes_real.npz"))
    pool = np.load(os.path.join(HERE, "step_real_b68.npz"))["u8"]
    names = ep["traj_names"].tolist()
    offs = np.concatenate([[0], np.cumsum(ep["traj_len"])])
    traj_seqs = {n: ep["traj_idx"][offs[t]:offs[t + 1]] for t, n in enumerate(names)}
    _stub_modules(pool, traj_seqs)

    import critic_net                                  # noqa: E402  (the reference)
    import vae_nets                                    # noqa: E402
    import vae_parameters                              # noqa: E402
    import vae_utility as vu                           # noqa: E402
    cw = np.load(os.path.join(HERE, "critic_real_b8.npz"))
    critic = critic_net.Critic()
    critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
    critic.eval()

    vae = load_reference_vae(vae_nets, first_vae_params(WSEED))
    vae.eval(), vae.encoder.eval(), vae.decoder.eval()             # load_vae_network, vae_utility.py:359-361
    for k, a in first_vae_params(WSEED).items():
        if "running_mean" in k:
            assert np.abs(a).min() >= 0.05
        if "running_var" in k:
            assert np.abs(a - 1).min() >= 0.2

    vu.total_images = TOTAL_IMAGES
    out = io.StringIO()
    with contextlib.redirect_stdout(out), torch.no_grad():
        dset = vu.load_minerl_data(critic, recon_dset=True, vae=vae)
    sizes = [int(line.split("=")[1]) for line in out.getvalue().splitlines() if line.startswith("total images =")]

    # the reference's own evaluate of every pool frame, both kinds; every dset entry must be one of them bit for bit
    key = {}
    samples = np.full((len(pool), 2, (3 * 64 * 64 + SAMPLE_STRIDE - 1) // SAMPLE_STRIDE), np.nan, np.float32)
    stats = np.full((len(pool), 2, 3), np.nan, np.float64)
    evals = {}
    with torch.no_grad():
        for i, f in enumerate(pool):
            obs = vu.preprocess_observation(f)
            pred = critic.evaluate(obs)[0]
            assert abs(pred.item() - ep["pool_preds"][i]) < 1e-6          # CPU round-off may differ with the thread count
            for kind, p in ((0, torch.zeros(1) + pred), (1, torch.zeros(1))):
                r = vae.evaluate(obs, p).detach().cpu().numpy()
                key.setdefault(r.tobytes(), (i, kind))
                evals[(i, kind)] = r
    dset_pool, dset_kind = [], []
    for d in dset:
        assert d.shape == (1, 3, 64, 64) and d.dtype == np.float32
        i, kind = key[np.asarray(d).tobytes()]
        dset_pool.append(i)
        dset_kind.append(kind)
        s, total, lo, hi = sample_of(evals[(i, kind)])
        samples[i, kind], stats[i, kind] = s, (total, lo, hi)
    dset_pool, dset_kind = np.array(dset_pool, np.int64), np.array(dset_kind, np.int64)

    # the restatement agrees, the cut falls inside the list, and counting mid frames twice changes the visited set
    walk = [traj_seqs[names[i]] for i in ep["order"]]
    wpreds = [ep["pool_preds"][s] for s in walk]
    r_sizes, r_entries, _ = E.select_recon_host(wpreds, collect=150, total_images=TOTAL_IMAGES)
    assert r_sizes == sizes
    assert [(int(walk[t][i]), k) for t, i, k in r_entries] == list(zip(dset_pool.tolist(), dset_kind.tolist()))
    plain_sizes, _, _ = E.select_host(wpreds, collect=150, total_images=TOTAL_IMAGES)
    assert len(sizes) < len(names), "the cut must fall inside the trajectory list"
    assert len(plain_sizes) != len(sizes), "the recon walk must visit another set than the non-recon walk"
    assert {0, 1} <= set(dset_kind.tolist()) and np.abs(stats[np.isfinite(stats[:, :, 1])][:, 1:]).max() < 1.0
    print(f"[recon] sizes {sizes} ({len(plain_sizes)} trajectories in the non-recon walk) -> {len(dset)} entries, "
          f"range [{np.nanmin(stats[:, :, 1]):.3f}, {np.nanmax(stats[:, :, 2]):.3f}]")

    # block 2: -second on the first 128 entries
    entries = torch.from_numpy(np.stack(dset[:2 * BATCH]).squeeze())
    with torch.no_grad():
        preds = critic.evaluate(entries)
    chosen = None
    for wseed2 in SEED_CANDIDATES:
        traj, first_bad = second_curve(vae_nets, vae_parameters.lr, entries, preds, wseed2)
        print(f"[second] wseed2 {wseed2}: {len(traj)} steps, first non-finite {first_bad}, loss {traj[0, 0]:.5f} -> {traj[-1, 0]:.5f}")
        if chosen is None:
            chosen = (wseed2, traj, first_bad)
        if first_bad < 0:
            chosen = (wseed2, traj, first_bad)
            break
    wseed2, traj, first_bad = chosen
    if first_bad < 0:
        assert len(traj) == STEPS and np.isfinite(traj).all()
    else:
        assert np.isfinite(traj[:first_bad]).all()
    np.savez_compressed(os.path.join(HERE, "recon_real.npz"),
                        pool_source="step_real_b68.npz/u8", episodes_source="episodes_real.npz", wseed=WSEED,
                        total_images=TOTAL_IMAGES, collect=150, sizes=np.array(sizes, np.int64), dset_pool=dset_pool,
                        dset_kind=dset_kind, sample_stride=SAMPLE_STRIDE, samples=samples, stats=stats,
                        second_wseed=wseed2, second_dseed=DSEED2, second_steps=STEPS, second_batch=BATCH,
                        second_lr=np.float32(vae_parameters.lr), second_traj=traj, second_first_nonfinite_step=first_bad,
                        second_preds=preds.numpy().reshape(-1).astype(np.float32))
    print(f"[second] stored wseed2 {wseed2}: {len(traj)} steps, first non-finite step {first_bad}")


if __name__ == "__main__":
    main()
