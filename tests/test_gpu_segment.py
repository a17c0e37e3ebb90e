"""Segmentation evaluation on the MI355X (critic_vae_amd.segment, cvae_diff_normalize / cvae_mask_counts /
cvae_dense_crf): the CRF against the float64 restatement of tests/crf_ref.py, determinism, the normalisation kernel
against numpy, and eval_frames / threshold_sweep against the reference's own evaluation (segment_real_b68.npz)."""
import os
import statistics
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crf_ref import crf_ref  # noqa: E402
from segment_tools import _structured_frames  # noqa: E402

from critic_vae_amd import segment as seg  # noqa: E402
from critic_vae_amd.critic import Critic  # noqa: E402
from critic_vae_amd.lib import Handle  # noqa: E402
from critic_vae_amd.nets import VariationalAutoencoder  # noqa: E402
from critic_vae_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _real_frames(golden_dir, n):
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"][:n]
    g = u8.astype(np.int32)
    masks = ((g[..., 0] > g[..., 1]) & (g[..., 0] > 40)).astype(np.float32)       # brownish pixels: a crude trunk mask
    return u8, masks


def _check_against_ref(labels, q1, frames, masks, params, p_floor, device="cpu"):
    for i in range(frames.shape[0]):
        lr, qr = crf_ref(frames[i], masks[i], params, p_floor, device=device)
        err = np.abs(q1[i].astype(np.float64) - qr).max()
        assert err < 1e-4, (i, err)
        bad = (labels[i] != lr) & (np.abs(qr - 0.5) >= 1e-4)
        assert not bad.any(), (i, int(bad.sum()))


def test_crf_matches_float64_reference_64():
    fr_real, m_real = _real_frames(os.path.join(os.path.dirname(__file__), "golden"), 6)
    fr_syn, m_syn = _structured_frames(8, 64, 11)
    frames, masks = np.concatenate([fr_real, fr_syn]), np.concatenate([m_real, m_syn])
    for params, p_floor in ((seg.CRF_REF, 1e-5), ((5, 6, 20.0, 3, 3.0, 4), 1e-3)):
        labels, q1 = seg.dense_crf(frames, masks, params, p_floor, return_q1=True)
        _check_against_ref(labels.cpu().numpy(), q1.cpu().numpy(), frames, masks, params, p_floor, device="cuda")


def test_crf_matches_float64_reference_128():
    frames, masks = _structured_frames(1, 128, 5)
    labels, q1 = seg.dense_crf(frames, masks, seg.CRF_REF, return_q1=True)
    _check_against_ref(labels.cpu().numpy(), q1.cpu().numpy(), frames, masks, seg.CRF_REF, 1e-5, device="cuda")


def test_crf_zero_iterations_returns_the_mask():
    frames, masks = _structured_frames(3, 64, 2)
    m = (masks > 0.5).astype(np.float32)
    labels = seg.dense_crf(frames, m, (22, 12, 3.1, 8, 1.8, 0))
    assert np.array_equal(labels.cpu().numpy(), m > 0.5)


def test_crf_bitwise_deterministic_across_batch_and_runs():
    frames, masks = _structured_frames(12, 64, 3)
    B, pos = 600, 337
    sel = np.arange(B) % 12
    big_f, big_m = frames[sel], masks[sel]
    one_l, one_q = seg.dense_crf(frames[pos % 12:pos % 12 + 1], masks[pos % 12:pos % 12 + 1], return_q1=True)
    l1, q1 = seg.dense_crf(big_f, big_m, return_q1=True)
    l2, q2 = seg.dense_crf(big_f, big_m, return_q1=True)
    assert torch.equal(l1, l2) and torch.equal(q1, q2)
    assert torch.equal(one_l[0], l1[pos]) and torch.equal(one_q[0], q1[pos])
    assert torch.equal(q1[pos], q1[pos + 12 * 10])            # the same frame at another position


def _numpy_u8(diff32, mean_max, factor):
    d = diff32.astype(np.float64)
    d[d > mean_max] = mean_max
    d = d * factor
    return (d * 255).astype(np.uint8)


@pytest.mark.parametrize("w", [64, 128])
def test_diff_normalize_bitwise_and_histogram_iou(w):
    rng = np.random.default_rng(w)
    B = 37
    diff = (rng.gamma(0.8, 1.0, size=(B, w, w)) * rng.uniform(0.1, 2.0, size=(B, 1, 1))).astype(np.float32)
    diff[3] = 0
    gt = rng.random((B, w, w)) < np.linspace(0, 0.6, B)[:, None, None]
    gt[5] = False
    maxima = diff.reshape(B, -1).max(1)
    factor, mean_max = seg.diff_factor(maxima)
    ref = _numpy_u8(diff, mean_max, factor)
    h = Handle(w, 1)
    dd = torch.from_numpy(diff).cuda()
    gtd = torch.from_numpy(gt.astype(np.uint8)).cuda()
    u8 = torch.empty(B, w, w, dtype=torch.uint8, device="cuda")
    mask = torch.empty_like(u8)
    counts = torch.empty(B, 3, dtype=torch.int64, device="cuda")
    hist = torch.zeros(2, 256, dtype=torch.int64, device="cuda")
    t = 50
    h.diff_normalize(B, dd, mean_max, factor, t, gtd, u8, mask, counts, hist)
    u8n, maskn, countsn = u8.cpu().numpy(), mask.cpu().numpy().astype(bool), counts.cpu().numpy()
    assert np.array_equal(u8n, ref)
    assert np.array_equal(maskn, ref > t)
    for i in range(B):
        G, T = gt[i], ref[i] > t
        assert countsn[i].tolist() == [np.sum(G & T), np.sum(G & ~T), np.sum(~G & T)]
    hn = hist.cpu().numpy()
    assert hn.sum() == B * w * w
    for th in range(0, 256, 5):
        assert seg.iou_from_hist(hn, th) == seg.iou(gt, ref > th), th
    h.diff_normalize(B, dd, mean_max, factor, t, gtd, u8, None, None, hist)        # accumulates
    assert np.array_equal(hist.cpu().numpy(), 2 * hn)
    c2 = seg.mask_counts(mask, gtd).cpu().numpy()
    assert np.array_equal(c2, countsn)


def test_mean_max_zero_and_empty_union():
    B, w = 4, 64
    diff = torch.zeros(B, w, w, device="cuda")
    u8, m = seg.threshold_masks(diff, np.zeros(B), 0)
    assert seg.diff_factor(np.zeros(B)) == (0, 0)
    assert not u8.any() and not m.any()
    gt = np.zeros((B, w, w), bool)
    c = seg.mask_counts(m, gt).cpu().numpy()
    assert not c.any() and seg.iou_from_counts(*c.sum(0)) == 1 == seg.iou(gt, m.cpu().numpy())


def _vae_and_critic(golden_dir, max_batch):
    vae = VariationalAutoencoder(max_batch=max_batch, seed=0).to("cuda")
    vae.load_reference_params(synth.make_params(0))
    cw = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    critic = Critic(64, handle=Handle(64, max_batch)).to("cuda")
    critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
    return vae, critic


def test_eval_frames_against_reference_fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    gt = fx["gt"]
    vae, critic = _vae_and_critic(golden_dir, 32)             # 68 frames in chunks of 32
    vae.train()                                               # eval_frames must force eval mode itself
    r = seg.eval_frames(u8, vae, gt, critic=critic, t=50)
    assert np.abs(r["preds"] - fx["preds"]).max() < 1e-5
    # the measured diff error: the stored float64 difference masks and every frame's maximum
    fr_u, fr_d = list(fx["u8_frames"]), list(fx["diff_frames"])
    err = max(np.abs(r["diff"][fr_d].astype(np.float64) - fx["diff"]).max(),
              np.abs(r["max_values"].astype(np.float64) - fx["max_values"]).max())
    assert err < 1e-5, err
    mm_ref = float(fx["mean_max"])
    assert abs(r["mean_max"] - mm_ref) <= err + 1e-15
    tol = 255 * 4 * err / mm_ref
    # this library's float64 values before truncation (the kernel's arithmetic: test_diff_normalize_bitwise_...)
    f_ours, mm_ours = seg.diff_factor(r["max_values"])
    v = np.minimum(r["diff"].astype(np.float64), mm_ours) * f_ours * 255
    assert np.array_equal(v.astype(np.uint8), r["diff_u8"])
    # a uint8 value may differ from the reference's only by one, and only where the two values straddle a truncation
    # boundary, i.e. where this library's value lies within the measured error of it
    ours, ref = r["diff_u8"][fr_u], fx["diff_u8"]
    differs = ours != ref
    assert (np.abs(ours.astype(int) - ref) <= 1).all()
    assert (np.abs(v[fr_u] - np.maximum(ours, ref))[differs] <= tol).all()
    # masks of all 68 frames: a pixel may change side only within the measured error of the boundary 51 (u8 > 50)
    mdiff = r["thr_masks"] != fx["thr_masks/50"]
    assert (np.abs(v - 51)[mdiff] <= tol).all()
    if not mdiff.any():
        assert r["thr_iou"] == fx["thr_iou/50"]
    assert r["thr_iou"] == seg.iou(gt, r["thr_masks"])
    assert abs(r["thr_iou"] - fx["thr_iou/50"]) <= mdiff.sum() / max(1, (gt | fx["thr_masks/50"]).sum()) + 1e-3
    # what the reference hands densecrf: the frame, stack(1 - m, m) of its thresholded mask, and CRF_REF
    assert tuple(fx["crf_call0/img_shape"].tolist()) == (1, 64, 64, 3)      # frame 0 itself, as (1, 64, 64, 3)
    assert np.array_equal(fx["crf_call0/prob"][..., 1], fx["thr_masks/50"][0].astype(np.float32))
    assert tuple(fx["crf_call0/param"].tolist()) == seg.CRF_REF
    assert r["crf_iou"] == seg.iou(gt, r["crf_masks"])
    assert np.array_equal(r["crf_masks"], seg.dense_crf(u8, r["thr_masks"]).cpu().numpy())
    if not mdiff.any():
        assert seg.bin_info_text(r["bins"]) == str(fx["bin_info_text"])


def test_threshold_sweep_matches_separate_evaluations(golden_dir):
    fx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    vae, critic = _vae_and_critic(golden_dir, 68)
    preds = fx["preds"]
    sweep = seg.threshold_sweep(u8, vae, fx["gt"], preds=preds)
    assert [t for t, _, _ in sweep] == list(seg.SWEEP)
    for t, thr_iou, crf_iou in sweep:
        r = seg.eval_frames(u8, vae, fx["gt"], preds=preds, t=t)
        assert (thr_iou, crf_iou) == (r["thr_iou"], r["crf_iou"]), t
        if f"thr_iou/{t}" in fx.files and np.array_equal(r["thr_masks"], fx[f"thr_masks/{t}"]):
            assert thr_iou == fx[f"thr_iou/{t}"]
    assert statistics.mean(float(x) for x in fx["max_values"]) == float(fx["mean_max"])
