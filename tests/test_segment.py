"""Segmentation evaluation, host side (no GPU): the float64 CRF restatement's invariants, IoU / bins / normalisation
against the reference's own fixture (segment_real_b68.npz), load_episode, argument checks of the C-ABI entries and
the CLI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crf_ref import crf_ref  # noqa: E402

from critic_vae_amd import lib as cvlib  # noqa: E402
from critic_vae_amd import segment as seg  # noqa: E402

W = 16      # the float64 reference takes any size; small frames keep these tests fast


def _flat_frame(w=W, colour=(120, 80, 40), seed=0):
    rng = np.random.default_rng(seed)
    f = np.empty((w, w, 3), np.uint8)
    f[:] = colour
    return np.clip(f.astype(int) + rng.integers(-2, 3, size=f.shape), 0, 255).astype(np.uint8)


def _two_region():
    f = _flat_frame()
    f[:, W // 2:] = (20, 160, 220)
    m = np.zeros((W, W), np.float32)
    m[:, W // 2:] = 1
    m[3:6, 2:4] = 1 - m[3:6, 2:4]
    return f, m


def test_crf_ref_zero_iterations_returns_the_mask():
    f, m = _two_region()
    lab, q = crf_ref(f, m, (22, 12, 3.1, 8, 1.8, 0))
    assert np.array_equal(lab, m > 0.5)
    assert np.allclose(q[m > 0.5], 1 - 1e-5) and np.allclose(q[m < 0.5], 1e-5)


def test_crf_ref_without_pairwise_terms_is_the_identity():
    f, m = _two_region()
    lab, _ = crf_ref(f, m, (0, 12, 3.1, 0, 1.8, 10))
    assert np.array_equal(lab, m > 0.5)


def test_crf_ref_label_swap_swaps_the_output():
    f, m = _two_region()
    rng = np.random.default_rng(1)
    soft = np.clip(m * 0.7 + rng.random(m.shape) * 0.3, 0, 1)
    lab, q = crf_ref(f, soft)
    lab_s, q_s = crf_ref(f, 1 - soft)
    assert np.allclose(q + q_s, 1, atol=1e-12)
    tie = np.abs(q - 0.5) < 1e-9
    assert np.array_equal(lab[~tie], ~lab_s[~tie])


def test_crf_ref_removes_an_isolated_flipped_pixel():
    f = _flat_frame()
    m = np.zeros((W, W), np.float32)
    m[7, 9] = 1
    lab, _ = crf_ref(f, m)
    assert not lab.any()
    lab, _ = crf_ref(f, 1 - m)
    assert lab.all()


def test_iou_semantics():
    G = np.zeros((2, 4, 4), bool)
    assert seg.iou(G, G) == 1                       # empty union
    T = G.copy()
    G[0, 0, :3] = True
    T[0, 0, 1:] = True
    assert seg.iou(G, T) == round(2 / 4, 3) == seg.iou(T, G)
    assert seg.iou_from_counts(1, 1, 1) == 0.333
    hist = np.zeros((2, 256), np.int64)
    hist[0, 10], hist[0, 200], hist[1, 150] = 3, 5, 7
    assert seg.iou_from_hist(hist, 100) == round(5 / 15, 3)
    assert seg.iou_from_hist(hist, 0) == round(8 / 15, 3)
    assert seg.iou_from_hist(hist, 255) == 0.0


def test_normalisation_iou_and_bins_against_the_reference_fixture(golden_dir):
    fx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    factor, mean_max = seg.diff_factor(fx["max_values"])
    assert mean_max == float(fx["mean_max"]) and factor == float(fx["diff_factor"])
    fr_u, fr_d = list(fx["u8_frames"]), list(fx["diff_frames"])
    d = np.minimum(fx["diff"], mean_max) * factor
    assert np.array_equal((d * 255).astype(np.uint8), fx["diff_u8"][[fr_u.index(i) for i in fr_d]])
    for t in fx["thresholds"]:
        assert np.array_equal(fx["diff_u8"] > t, fx[f"thr_masks/{t}"][fr_u])
        assert seg.iou(fx["gt"], fx[f"thr_masks/{t}"]) == fx[f"thr_iou/{t}"]
    bins = seg.bin_info(fx["preds"], fx["gt"], fx["thr_masks/50"])
    assert seg.bin_info_text(bins) == str(fx["bin_info_text"])
    assert "bin: 1.0, iou_mean=" in str(fx["bin_info_text"]) and "iou_std=nan" in str(fx["bin_info_text"])


def test_write_bin_info(tmp_path):
    preds = np.array([0.12, 0.14, 0.31], np.float32)
    gt = np.zeros((3, 4, 4), bool)
    gt[:, 0] = True
    masks = gt.copy()
    masks[1, 0, 0] = False
    bins = seg.bin_info(preds, gt, masks)
    assert list(bins["frames"].items()) == [(0.1, 2), (0.3, 1)]
    p = tmp_path / "bin_info.txt"
    seg.write_bin_info(str(p), bins)
    txt = p.read_text()
    assert txt.startswith("ground truth pixels sorted by bin:\nbin: 0.1, pixels = 8 = 67.0%\n")
    assert "bin: 0.1, iou_mean=0.88, iou_std=0.18\nbin: 0.3, iou_mean=1.0, iou_std=nan\n" in txt


def test_load_episode_slicing(tmp_path):
    n = 5200
    X = (np.arange(n, dtype=np.int64) % 251).astype(np.uint8)[:, None, None, None] * np.ones((1, 2, 2, 3), np.uint8)
    Y = np.zeros((n, 2, 2, 3), np.uint8)
    Y[::3] = 255
    Y[::3, 0, 0, 1] = 0
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "Y.npy", Y)
    frames, gt = seg.load_episode(str(tmp_path / "X.npy"), str(tmp_path / "Y.npy"))
    idx = np.arange(100, 5000, 2)
    assert frames.shape == (2450, 2, 2, 3) and np.array_equal(frames, X[idx])
    assert gt.shape == (2450, 2, 2) and gt.dtype == bool
    assert np.array_equal(gt, np.all(Y[idx], axis=-1))
    assert gt[idx % 3 == 0][:, 0, 1].all() and not gt[:, 0, 0].any()


def test_crf_scratch_query_and_argument_rejection():
    h = cvlib.Handle(64, 1)
    lib = h.lib
    npix = 64 * 64
    assert h.crf_scratch_bytes(1) == npix * (2 * 16 + 5 * 4)
    assert h.crf_scratch_bytes(7) == 7 * h.crf_scratch_bytes(1)
    assert lib.cvae_crf_scratch_bytes(h.h, 0) < 0
    assert lib.cvae_crf_scratch_bytes(None, 1) < 0
    assert lib.cvae_crf_scratch_bytes(h.h, 2 ** 31 // 4096) < 0
    h128 = cvlib.Handle(128, 1)
    assert h128.crf_scratch_bytes(3) == 3 * 16384 * (32 + 20)
    fake = 1 << 20                                  # never dereferenced: every call below fails its host checks

    def crf(p, B=1, scratch=fake, labels=fake):
        return lib.cvae_dense_crf(h.h, B, fake, fake, C.byref(p), labels, None, scratch, None)

    good = seg.crf_params()
    bad = [dict(w1=-1.0), dict(w2=-0.5), dict(alpha=0.0), dict(beta=-3.0), dict(gamma=0.0), dict(p_floor=0.0),
           dict(p_floor=1.5), dict(iterations=-1), dict(iterations=10001), dict(w1=float("nan")),
           dict(alpha=float("inf"))]
    for change in bad:
        p = seg.crf_params()
        for k, v in change.items():
            setattr(p, k, v)
        assert crf(p) < 0, change
        assert b"cvae_dense_crf" in lib.cvae_last_error()
    assert crf(good, B=0) < 0
    assert crf(good, labels=None) < 0
    assert crf(good, scratch=fake + 4) < 0 and b"aligned" in lib.cvae_last_error()
    args = [h.h, 1, fake, 1.0, 1.0]
    assert lib.cvae_diff_normalize(*args, 256, None, fake, None, None, None, None) < 0
    assert lib.cvae_diff_normalize(*args, 50, None, fake, None, fake, None, None) < 0        # counts need gt
    assert lib.cvae_diff_normalize(*args, 50, None, fake, None, None, fake, None) < 0        # histogram needs gt
    assert lib.cvae_diff_normalize(h.h, 1, fake, -1.0, 1.0, 50, None, fake, None, None, None, None) < 0
    assert lib.cvae_diff_normalize(h.h, 1, fake, float("nan"), 1.0, 50, None, fake, None, None, None, None) < 0
    assert lib.cvae_diff_normalize(h.h, 0, fake, 1.0, 1.0, 50, None, fake, None, None, None, None) < 0
    assert lib.cvae_mask_counts(h.h, 1, fake, None, fake, None) < 0
    assert lib.cvae_mask_counts(h.h, 0, fake, fake, fake, None) < 0


def test_reference_constants():
    assert seg.CRF_REF == (22, 12, 3.1, 8, 1.8, 10)
    assert seg.THRESHOLD == 50
    assert seg.SWEEP == tuple(range(0, 130, 10))
    p = seg.crf_params()
    assert (p.w1, p.alpha, p.w2, p.iterations) == (22, 12, 8, 10)
    assert abs(p.beta - 3.1) < 1e-6 and abs(p.gamma - 1.8) < 1e-6 and abs(p.p_floor - 1e-5) < 1e-12


def test_cli_parsing():
    a = seg.parse_args(["-video", "--frames", "x.npy", "--gt", "y.npy", "--networks", "nets"])
    assert a.video and not a.thresh and a.frames == "x.npy" and a.gt == "y.npy"
    assert a.critic == os.path.join("nets", seg.CRITIC_FILE) and a.chunk == 256
    a = seg.parse_args(["-video", "-thresh", "--critic", "c.pt", "--chunk", "64"])
    assert a.thresh and a.critic == "c.pt" and a.chunk == 64
    assert a.frames == "minerl-episode/X.npy" and a.networks == "saved-networks"
    with pytest.raises(SystemExit):
        seg.parse_args([])                          # -video is the only mode
    with pytest.raises(SystemExit):
        seg.parse_args(["-video", "--chunk", "0"])
