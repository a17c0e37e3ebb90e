"""Generate tests/golden/segment_real_b68.npz from the REFERENCE's own evaluation code (run only where the reference
checkout exists, like make_golden.py).

    python tests/golden/make_segment_golden.py            # needs /root/reference (read-only)

Imports the reference's vae_utility with three stand-ins for what cannot load here: `minerl` (an empty module),
`denseCRF` (a recording stub whose densecrf returns its input mask unchanged) and PIL.ImageFont.truetype (returns
None: the reference hard-codes a font path; PIL's default font then draws the frame titles).  On the 68 real
frames of step_real_b68.npz["u8"] it runs the reference critic (critic_real_b8.npz weights) and the reference VAE in eval mode on the generator's seed-0 weights
through eval_textured_frames at t = 0, 50, 120, and get_diff_image / get_diff_and_thr_masks / get_iou directly.
The ground truth is a deterministic synthetic mask stored in the fixture (the episode's Y.npy is not available).

One deviation: the reference's save_bin_info_file calls statistics.stdev, which raises on a bin with one frame
(this set has one frame in bin 1.0).  The generator gives vae_utility a `statistics` whose stdev returns nan for
fewer than two values; critic_vae_amd.segment.bin_info_text writes nan there too.

The fixture holds data only, kept small: preds, the per-frame maxima, mean_max and diff_factor of all 68 frames; the
float64 diffs of DIFF_FRAMES and the uint8 masks of U8_FRAMES (random-looking values that compress poorly); the
thresholded masks and thr_iou of every frame per t; the bin-info text at t = 50; and what the reference handed to its
first densecrf call: the shape of img (whose values are asserted here to be frame 0), prob and param.
"""
import math
import os
import statistics
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from critic_vae_amd import synth                      # noqa: E402

THRESHOLDS = (0, 50, 120)
U8_FRAMES = tuple(range(0, 68, 4))      # frames whose uint8 masks are stored
DIFF_FRAMES = (0, 32)                   # frames whose float64 difference masks are stored (a subset of U8_FRAMES)
CRF_CALLS = []


def _stub_modules():
    sys.modules["minerl"] = types.ModuleType("minerl")
    dcrf = types.ModuleType("denseCRF")

    def densecrf(img, prob, param):
        CRF_CALLS.append((np.array(img, copy=True), np.array(prob, copy=True), tuple(param)))
        return (prob[..., 1] > 0.5).astype(np.uint8)
    dcrf.densecrf = densecrf
    sys.modules["denseCRF"] = dcrf
    from PIL import ImageFont
    real = ImageFont.truetype
    ImageFont.truetype = lambda *a, **k: None
    return real


def _stdev_or_nan(v):
    v = list(v)
    return statistics.stdev(v) if len(v) > 1 else float("nan")


def synthetic_gt(n, w=64, seed=7):
    """A deterministic 'trunk': a vertical band of random position and width per frame, with a ragged edge; every
    ninth frame has no ground truth at all."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((n, w, w), bool)
    xs = np.arange(w)
    for i in range(n):
        if i % 9 == 4:
            continue
        c, half = rng.integers(10, w - 10), rng.integers(3, 12)
        edge = rng.integers(-2, 3, size=w)
        gt[i] = np.abs(xs[None, :] - c) <= (half + edge)[:, None]
        gt[i, :rng.integers(0, 20)] = False
    return gt


def main():
    truetype = _stub_modules()
    import vae_utility as vu                           # noqa: E402  (the reference)
    import vae_nets                                    # noqa: E402
    import critic_net                                  # noqa: E402
    vu.statistics = types.SimpleNamespace(mean=statistics.mean, stdev=_stdev_or_nan)
    from PIL import ImageFont
    ImageFont.truetype = truetype                      # the None the stub gave the reference cannot draw the frame titles
    vu.font = ImageFont.load_default()

    torch.manual_seed(0)
    u8 = np.load(os.path.join(HERE, "step_real_b68.npz"))["u8"]
    cw = np.load(os.path.join(HERE, "critic_real_b8.npz"))
    critic = critic_net.Critic()
    critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
    critic.eval()
    vae = vae_nets.VariationalAutoencoder()
    params = synth.make_params(0)
    vae.encoder.load_state_dict({k[8:]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith("encoder.")},
                                strict=False)
    vae.decoder.load_state_dict({k[8:]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith("decoder.")})
    vae.eval(); vae.encoder.eval(); vae.decoder.eval()
    n = u8.shape[0]
    gt = synthetic_gt(n)

    # step 1 + 2 by hand: the float64 diffs and maxima before get_diff_and_thr_masks normalises them in place
    preds, diffs, maxima = [], [], []
    with torch.no_grad():
        for img in u8:
            frame = vu.preprocess_observation(img)
            pred = critic.evaluate(frame)
            _, _, diff, mx = vu.get_diff_image(vae, frame, pred[0])
            preds.append(pred[0].item()); diffs.append(diff); maxima.append(mx)
    diff_factor, mean_max = vu.get_diff_factor(maxima)
    fx = {"u8_source": "step_real_b68.npz/u8", "vae_wseed": 0, "gt": gt, "preds": np.array(preds, np.float32),
          "diff_frames": np.array(DIFF_FRAMES), "diff": np.array(diffs, np.float64)[list(DIFF_FRAMES)],
          "max_values": np.array(maxima, np.float64), "mean_max": mean_max, "diff_factor": diff_factor,
          "thresholds": np.array(THRESHOLDS), "u8_frames": np.array(U8_FRAMES)}
    for t in THRESHOLDS:
        du8, thr = vu.get_diff_and_thr_masks([d.copy() for d in diffs], list(maxima), thr=t)
        fx["diff_u8"] = du8.astype(np.uint8)[list(U8_FRAMES)]
        fx[f"thr_masks/{t}"] = thr
        fx[f"thr_iou/{t}"] = vu.get_iou(gt, thr)

    # the whole eval_textured_frames, which must agree with the pieces above; its densecrf calls are recorded
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        os.chdir(tmp)
        try:
            for t in THRESHOLDS:
                CRF_CALLS.clear()
                _, thr_iou, crf_iou = vu.eval_textured_frames(u8, vae, critic, gt, t=t)
                assert thr_iou == fx[f"thr_iou/{t}"] and crf_iou == thr_iou, (t, thr_iou, crf_iou, fx[f"thr_iou/{t}"])
                assert len(CRF_CALLS) == n
                if t == 50:
                    img, prob, param = CRF_CALLS[0]
                    assert img.shape == (1, 64, 64, 3) and np.array_equal(img[0], u8[0])
                    fx["crf_call0/img_shape"] = np.array(img.shape)
                    fx["crf_call0/prob"], fx["crf_call0/param"] = prob, np.array(param)
                    fx["bin_info_text"] = open("bin_info_vae1.txt").read()
        finally:
            os.chdir(cwd)
    assert math.isfinite(mean_max)
    np.savez_compressed(os.path.join(HERE, "segment_real_b68.npz"), **fx)
    print(f"[segment] mean_max {mean_max:.6f} thr_iou {[fx[f'thr_iou/{t}'] for t in THRESHOLDS]} "
          f"crf img {tuple(int(v) for v in fx['crf_call0/img_shape'])} prob {fx['crf_call0/prob'].shape} {fx['crf_call0/prob'].dtype}")


if __name__ == "__main__":
    main()
