"""cvae_critic_collect, cvae_critic_saliency and cvae_critic_occlusion on the device (csrc/critic_saliency.hip) against
cvae_critic_forward / cvae_critic_grad (the same device code: bit for bit) and the torch-CPU restatement
tests/critic_saliency_ref.py, which tests/golden/make_critic_saliency_golden.py pins to the reference's own Critic class.

Frames are the 68 real fixture frames, repeated where a batch is longer.  B = 1, 5 and 37 (ragged, more than one workgroup,
and — under CVAE_PERSIST_MAXWG in a child process — several images per workgroup) and B = 257, one past the grid of a
256-CU part, where the first workgroup walks a second image.  A frame's results depend on that frame alone, so the device
runs on the 68 frames and the fp64 restatements with the device's decisions imposed are computed once per module and every
batch is compared with their rows: bit for bit with the device's, within the parity bar with the restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_saliency_ref as sref                               # noqa: E402
import critic_saliency_tools as S                                # noqa: E402
import critic_saliency_worker as W                               # noqa: E402
import critic_train_tools as T                                   # noqa: E402
from critic_vae_amd import lib as cvlib                          # noqa: E402
from critic_vae_amd import segment as seg                        # noqa: E402
from critic_vae_amd import synth                                 # noqa: E402
from critic_vae_amd.critic import Critic                         # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = [1, 5, 37, 257]
EMBED_TOL, PRED_TOL, GRAD_TOL = 1e-5, 1e-6, 1e-4      # absolute; absolute against cvae_critic_forward; of each frame's max |gradient|
IG = 4


@pytest.fixture(scope="module")
def fx(golden_dir):
    return S.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def handle():
    return T.make_handle(64)


def rows(B):
    return np.arange(B) % 68


def rel_gap(got, want):
    """Per frame: max |got - want| over the frame / max |want| over the frame."""
    B = want.shape[0]
    g = np.abs(got.astype(np.float64) - want).reshape(B, -1).max(1)
    return g / np.abs(want).reshape(B, -1).max(1)


@pytest.fixture(scope="module")
def sal68(fx, handle):
    """steps = 1 on the 68 frames, and the fp64 restatement with the device's decisions imposed."""
    res = S.run_saliency(handle, fx["flat"], fx["x"], 1)
    return res, sref.logit_grad(fx["w"], fx["x"], torch.float64, decisions=res["decisions"])


@pytest.fixture(scope="module")
def ig68(fx, handle):
    """steps = IG on the 68 frames; the decisions of every pass from steps = 1 calls on the host-scaled frames (covered by
    the steps = 1 tests); the fp64 restatement of the sum with those decisions imposed pass by pass."""
    res = S.run_saliency(handle, fx["flat"], fx["x"], IG)
    passes = [S.run_saliency(handle, fx["flat"], sref.scaled_frames(fx["x"], k, IG), 1, grad=False)["decisions"] for k in range(1, IG + 1)]
    return res, passes, sref.integrated_gradients(fx["w"], fx["x"], IG, torch.float64, decisions=passes)


# ---------------------------------------------------------------- 1. collect ----------------------------------------------------------------
@pytest.fixture(scope="module")
def col68(fx, handle):
    return S.run_collect(handle, fx["flat"], fx["x"])


@pytest.mark.parametrize("B", BATCHES)
def test_collect_pred_is_critic_forwards_and_rows_depend_on_their_frame(fx, handle, col68, B):
    x = fx["x"][rows(B)]
    res = S.run_collect(handle, fx["flat"], x)
    assert np.array_equal(res["pred"], S.run_forward(handle, fx["flat"], x)), "pred differs from cvae_critic_forward's bits"
    for k in ("pred", "e1", "e2", "e3", "e4", "e5"):
        assert np.array_equal(res[k], col68[k][rows(B)]), k


def test_collect_embeddings_against_the_fixture_and_the_fp64_restatement(fx, col68):
    """Measured on the MI355X: see the printed gaps; the bound is the one the critic-train tests hold pred to."""
    z = fx["z"]
    pred, embeds = sref.embeddings(fx["w"], fx["x"])
    gaps = [float(np.abs(col68[f"e{i + 1}"].astype(np.float64) - e).max()) for i, e in enumerate(embeds)]
    fgaps = [float(np.abs(col68[f"e{i + 1}"][z["frames"]].astype(np.float64) - z[f"e{i + 1}"]).max()) for i in range(5)]
    gp = float(np.abs(col68["pred"] - pred.reshape(-1)).max())
    print(f"collect: |d e1..e5| vs fp64 {['%.1e' % g for g in gaps]}, vs fixture {['%.1e' % g for g in fgaps]}, |d pred| {gp:.1e}")
    assert max(gaps) <= EMBED_TOL and max(fgaps) <= EMBED_TOL and gp <= EMBED_TOL
    assert all(np.isfinite(col68[f"e{i + 1}"]).all() and (col68[f"e{i + 1}"] >= 0).all() for i in range(5))


def test_forward_collect_returns_the_references_list(fx, handle):
    """Critic.forward(X, collect=True) (critic_net.py:44-59): (pred (B,1), four pooled maps and the bottleneck)."""
    critic = Critic(handle=handle).to(S.DEV)
    critic.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx["w"].items()})
    X = S.dev(fx["x"][:5])
    pred, embeds = critic(X, collect=True)
    assert tuple(pred.shape) == (5, 1) and [tuple(e.shape) for e in embeds] == [(5, 8, 32, 32), (5, 8, 16, 16), (5, 8, 8, 8), (5, 16, 4, 4), (5, 32, 1, 1)]
    assert torch.equal(pred, critic(X)) and torch.equal(pred, critic.evaluate(X))
    _, want = sref.embeddings(fx["w"], fx["x"][:5])
    assert max(float(np.abs(e.cpu().numpy() - w).max()) for e, w in zip(embeds, want)) <= EMBED_TOL


@pytest.mark.parametrize("which", [(False,) * 5, (True, False, True, False, True), (False, True, False, True, False)])
def test_collect_null_embeddings_leave_no_write(fx, handle, col68, which):
    res = S.run_collect(handle, fx["flat"], fx["x"][:5], which)          # run_collect checks the guard bytes and the withheld buffers
    assert np.array_equal(res["pred"], col68["pred"][:5])
    for i, on in enumerate(which):
        assert not on or np.array_equal(res[f"e{i + 1}"], col68[f"e{i + 1}"][:5])


# ------------------------------------------------------- 2. saliency against cvae_critic_grad -------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_saliency_pred_and_decisions_are_critic_grads(fx, handle, sal68, B):
    x = fx["x"][rows(B)]
    res = S.run_saliency(handle, fx["flat"], x, 1)
    tr = T.run_kernel(handle, fx["flat"], x, np.zeros(B, np.float32), None, 0.0, "bce")
    assert np.array_equal(res["pred"], tr["pred"].reshape(-1)) and np.array_equal(res["decisions"], tr["decisions"])
    gap = float(np.abs(res["pred"] - S.run_forward(handle, fx["flat"], x)).max())
    print(f"B={B}: saliency pred vs cvae_critic_forward {gap:.2e}")
    assert gap <= PRED_TOL
    for k in ("pred", "decisions", "grad", "map", "max_values"):
        assert np.array_equal(res[k], sal68[0][k][rows(B)]), f"{k}: a frame's result depends on its place in the batch"


# ------------------------------------------------------------ 3. gradient and map -------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_saliency_gradient_against_the_imposed_fp64_restatement(fx, handle, sal68, B):
    """Measured on the MI355X: see the printed gap (the fp32 CPU restatement's own gap is 3.1e-7)."""
    res = S.run_saliency(handle, fx["flat"], fx["x"][rows(B)], 1)
    want = sal68[1]["grad"][rows(B)]
    rel = rel_gap(res["grad"], want)
    print(f"B={B}: gradient within {rel.max():.2e} of each frame's max |gradient| ({np.abs(want).reshape(B, -1).max(1).min():.3f} .. "
          f"{np.abs(want).reshape(B, -1).max(1).max():.3f})")
    assert np.isfinite(res["grad"]).all() and rel.max() <= GRAD_TOL
    assert float(np.abs(res["pred"] - sal68[1]["pred"][rows(B)].reshape(-1)).max()) <= 1e-5


def test_saliency_decisions_against_the_free_fp64_choices(fx, sal68):
    z, dec = fx["z"], sal68[0]["decisions"]
    n = S.check_ties(fx["w"], fx["x"][z["frames"]], dec[z["frames"]], z["decisions"], "fixture frames")
    free = sref.logit_grad(fx["w"], fx["x"], torch.float64)["decisions"]
    assert np.array_equal(free[z["frames"]], z["decisions"])
    n68 = S.check_ties(fx["w"], fx["x"], dec, free, "68 frames")
    print(f"decisions that differ from the free fp64 choices: {n} of {z['decisions'].size} (fixture), {n68} of {dec.size} (68 frames)")
    if n == 0:                                   # the same branch: the fixture's gradient is the imposed restatement's
        assert rel_gap(sal68[0]["grad"][z["frames"]], z["grad"]).max() <= GRAD_TOL


@pytest.mark.parametrize("steps", [1, IG])
def test_saliency_map_and_max_values(fx, handle, sal68, ig68, steps):
    res = (sal68 if steps == 1 else ig68)[0]
    want = sref.grey_map(res["grad"])
    gap = np.abs(res["map"].astype(np.float64) - want)
    print(f"steps={steps}: map within {float((gap / S.ulp32(want)).max()):.2f} ulp of the weights applied to grad in float64")
    assert (gap <= 4 * S.ulp32(want)).all() and (res["map"] >= 0).all()
    assert np.array_equal(res["max_values"], res["map"].reshape(68, -1).max(1)) and (res["max_values"] > 0).all()
    # grad and decisions are optional: the other outputs do not change without them
    bare = S.run_saliency(handle, fx["flat"], fx["x"][:5], steps, grad=False, decisions=False)
    assert all(np.array_equal(bare[k], res[k][:5]) for k in ("pred", "map", "max_values"))


# ------------------------------------------------------------ 4. integrated gradients ---------------------------------------------------------
@pytest.mark.parametrize("B", [5, 37, 257])
def test_integrated_gradients_against_the_imposed_fp64_restatement(fx, handle, sal68, ig68, B):
    res = S.run_saliency(handle, fx["flat"], fx["x"][rows(B)], IG)
    dev, passes, want = ig68
    rel = rel_gap(res["grad"], want["grad"][rows(B)])
    print(f"B={B}, steps={IG}: integrated gradients within {rel.max():.2e} of each frame's max")
    assert np.isfinite(res["grad"]).all() and rel.max() <= GRAD_TOL
    # pred and decisions are those of the last pass, x itself: the steps = 1 call's
    assert np.array_equal(res["pred"], sal68[0]["pred"][rows(B)]) and np.array_equal(res["decisions"], sal68[0]["decisions"][rows(B)])
    assert np.array_equal(passes[IG - 1], sal68[0]["decisions"])
    for k in ("grad", "map", "max_values"):
        assert np.array_equal(res[k], dev[k][rows(B)]), k


def test_integrated_gradients_against_the_fixture(fx, ig68):
    z = fx["z"]
    assert int(z["ig_steps"]) == IG
    dev, passes, _ = ig68
    f = z["frames"]
    free = sref.integrated_gradients(fx["w"], fx["x"][f], IG, torch.float64)
    assert float(np.abs(free["grad"] - z["ig"]).max()) <= 1e-12
    differ = 0
    for k in range(IG):
        differ += S.check_ties(fx["w"], sref.scaled_frames(fx["x"][f], k + 1, IG), passes[k][f], free["pass_decisions"][k], f"pass {k + 1}")
    rel = rel_gap(dev["grad"][f], z["ig"])
    print(f"fixture N={IG}: {differ} decisions differ over the passes; gap to the fixture {rel.max():.2e} of each frame's max")
    if differ == 0:                              # otherwise the imposed form above is the comparison, and the ties were judged here
        assert rel.max() <= GRAD_TOL


# ----------------------------------------------------------------- 5. occlusion ---------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 4])
def test_occlusion_against_host_occluded_frames(fx, P):
    h = cvlib.Handle(64, 2048)
    fill = tuple(float(v) for v in fx["z"]["occ_fill"])
    x = fx["x"][[0, 9, 23, 40, 67]]
    g = 64 // P
    res = S.run_occlusion(h, fx["flat"], x, P, fill)
    assert np.array_equal(res["pred"], S.run_forward(h, fx["flat"], x))
    host = np.concatenate([sref.occluded_frames(x[b], P, fill) for b in range(5)])
    p_host = S.run_forward(h, fx["flat"], host).reshape(5, g, g)
    assert np.array_equal(res["drop"], (res["pred"][:, None, None] - p_host).astype(np.float32)), "drop != fp32(pred - p_host)"
    clamp = np.maximum(res["drop"], np.float32(0)).repeat(P, axis=1).repeat(P, axis=2)
    assert np.array_equal(res["map"], clamp) and np.array_equal(res["max_values"], clamp.reshape(5, -1).max(1))
    assert (res["max_values"] > 0).all()                                  # no real frame without a positive drop


def test_occlusion_against_the_fixture(fx, handle):
    z = fx["z"]
    res = S.run_occlusion(handle, fx["flat"], fx["x"][z["frames"]], int(z["occ_patch"]), tuple(float(v) for v in z["occ_fill"]))
    gap = float(np.abs(res["drop"].astype(np.float64) - z["occ_drop"]).max())
    print(f"occlusion P={int(z['occ_patch'])}: |d drop| vs the reference class {gap:.2e}")
    assert gap <= 1e-5 and float(np.abs(res["pred"] - z["pred"].reshape(-1)).max()) <= 1e-5


# ------------------------------------------------------ 6. several images per workgroup -------------------------------------------------------
def test_several_images_per_workgroup(fx, handle, tmp_path):
    """CVAE_PERSIST_MAXWG=8 in a fresh child process walks B = 37 in 8 workgroups (4 or 5 images each): every output equals
    this process's, bit for bit — a border left dirty by the backward, or a patch not put back, would show in the next image."""
    out = str(tmp_path / "capped.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "critic_saliency_worker.py"), out], env=dict(os.environ, CVAE_PERSIST_MAXWG="8"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    capped = np.load(out)
    assert int(capped["workgroups"]) == 8, f"the child ran {int(capped['workgroups'])} workgroups"
    mine = W.run_all(S, handle, fx, fx["x"][:W.B])
    assert set(mine) | {"workgroups"} == set(capped.files)
    for k, v in mine.items():
        assert np.array_equal(v, capped[k]), f"{k}: differs between 8 workgroups and one workgroup per image"


def test_copies_of_one_frame_give_identical_rows(fx, handle):
    x = np.repeat(fx["x"][11:12], 37, axis=0)
    for k, v in W.run_all(S, handle, fx, x).items():
        assert (v == v[:1]).all(), k


# ----------------------------------------------------------------- 7. segment tail ------------------------------------------------------------
@pytest.fixture(scope="module")
def critic68(fx):
    critic = Critic(64, handle=cvlib.Handle(64, 32)).to("cuda")
    critic.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx["w"].items()})
    return critic


def test_eval_maps_is_eval_frames_tail(fx, golden_dir, critic68):
    from critic_vae_amd.nets import VariationalAutoencoder
    gt = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))["gt"]
    vae = VariationalAutoencoder(max_batch=32, seed=0).to("cuda")
    vae.load_reference_params(synth.make_params(0))
    r = seg.eval_frames(fx["u8"], vae, gt, critic=critic68, t=50)
    assert "device" not in r
    m = seg.eval_maps(fx["u8"], r["diff"], r["max_values"], r["preds"], gt, 50, seg.CRF_REF, seg.P_FLOOR)
    assert set(m) == set(r) | {"device"}
    for k in ("diff_u8", "thr_masks", "crf_masks", "hist", "preds", "max_values", "diff"):
        assert np.array_equal(m[k], r[k]), k
    assert m["thr_iou"] == r["thr_iou"] and m["crf_iou"] == r["crf_iou"] and m["mean_max"] == r["mean_max"] and m["bins"] == r["bins"]
    sweep = seg.sweep_maps(fx["u8"], r["diff"], r["max_values"], gt, thresholds=(0, 50))
    assert sweep[1] == (50, r["thr_iou"], r["crf_iou"]) and sweep == seg.threshold_sweep(fx["u8"], vae, gt, critic=critic68, thresholds=(0, 50))


@pytest.mark.parametrize("source", ["grad", "ig", "occlusion"])
def test_critic_maps_end_to_end(fx, golden_dir, critic68, sal68, source):
    """No IoU is asserted: the ground truth of the 68 frames is synthetic."""
    gt = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))["gt"]
    preds, maps, maxv = seg.critic_maps(fx["u8"], critic68, source, steps=8, patch=16, chunk=32)     # 68 frames in chunks of 32
    assert preds.is_cuda and tuple(preds.shape) == (68,) and tuple(maps.shape) == (68, 64, 64) and tuple(maxv.shape) == (68,)
    assert bool(torch.isfinite(maps).all()) and bool((maps >= 0).all()) and torch.equal(maxv, maps.amax(dim=(1, 2)))
    if source == "grad":                         # the chunks through preprocess_u8 are the frames the other tests ran on
        assert np.array_equal(maps.cpu().numpy(), sal68[0]["map"]) and np.array_equal(preds.cpu().numpy(), sal68[0]["pred"])
    r = seg.eval_maps(fx["u8"], maps, maxv, preds, gt)
    assert r["mean_max"] > 0 and r["diff_u8"].shape == (68, 64, 64) and r["diff_u8"].dtype == np.uint8
    assert r["thr_masks"].shape == r["crf_masks"].shape == (68, 64, 64) and r["thr_masks"].dtype == r["crf_masks"].dtype == bool
    assert r["thr_masks"].any() and 0 <= r["thr_iou"] <= 1 and 0 <= r["crf_iou"] <= 1 and r["hist"].sum() == 68 * 64 * 64
    assert r["thr_iou"] == seg.iou(gt, r["thr_masks"]) and r["crf_iou"] == seg.iou(gt, r["crf_masks"])
    print(f"{source}: mean_max {r['mean_max']:.4f}, thr_iou {r['thr_iou']}, crf_iou {r['crf_iou']} (synthetic ground truth)")


def test_cli_with_a_critic_source(fx, tmp_path, capsys):
    n = 108                                      # load_episode keeps frames 100, 102, ...: four of them
    X = fx["u8"][np.arange(n) % 68]
    Y = np.zeros((n, 64, 64, 3), np.uint8)
    Y[:, 20:40, 10:50] = 1
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "Y.npy", Y)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in fx["w"].items()}, tmp_path / "critic.pt")
    argv = ["-video", "--frames", str(tmp_path / "X.npy"), "--gt", str(tmp_path / "Y.npy"), "--critic", str(tmp_path / "critic.pt"),
            "--mask-source", "critic-grad", "--networks", str(tmp_path / "none")]
    assert seg.main(argv) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("thr_iou=") and lines[1].startswith("crf_iou=")
    assert 0 <= float(lines[0].split("=")[1]) <= 1 and 0 <= float(lines[1].split("=")[1]) <= 1
