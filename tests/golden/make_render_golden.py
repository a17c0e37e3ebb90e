"""Generate tests/golden/render_real.npz from the REFERENCE's own picture code (run only where the reference checkout
exists, like make_segment_golden.py), and hold the numpy restatement of its panel rules that the render tests use as
their oracle (importable without the reference: nothing below main() touches it).

    python tests/golden/make_render_golden.py            # needs /root/reference (read-only)

Stand-ins as in make_segment_golden.py (`minerl` empty, `denseCRF` returning its input mask, the font), and
PIL.ImageDraw.ImageDraw.text replaced by a recorder that draws nothing: the pictures come out textless and every text
call is kept as (x, y, string).  On the 68 real frames of step_real_b68.npz["u8"], seed-0 VAE weights, the reference critic
and the ground truth of segment_real_b68.npz, it runs
  * eval_textured_frames (t = 50): the 7-panel pictures of get_final_frame,
  * the body of image_evaluate (vae.py:78-108) with the reference's get_diff_image / prepare_diff / get_final_frame: the
    4-panel strips,
  * get_injected_img: the 7-panel injection strips,
asserts that compose_ref below equals every one of those 3 x 68 PIL pictures byte for byte, and stores for the K frames
chosen below the three textless pictures and the reference's fp32 recon_one, recon_zero and six injected reconstructions,
and for all 68 frames the recorded text calls.  Data only.
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
THRESHOLD = 50
K = 2                    # frames stored (chosen in main()): 780 KB; a third would pass the largest fixture committed (907 KB)


# ---- the restatement: what the reference's host code does to each kind of panel ----
def panel_f32(chw, clamp=False):
    """prepare_rgb_image (vae_utility.py:385-390): transpose to HWC, ONE float32 multiply, truncation toward zero to int32,
    the low 8 bits; NaN, +-inf and |v * 255| >= 2^31 give 0 (what (img * 255).astype(np.uint8) gives on x86 for the values a
    Tanh output takes; stated through int64 here so that no host's cast is relied on)."""
    v = np.transpose(np.asarray(chw, np.float32), (1, 2, 0)) * np.float32(255)
    ok = np.isfinite(v) & (np.abs(v) < 2147483648.0)
    q = np.trunc(np.where(ok, v, 0)).astype(np.int64)
    if clamp:
        q = np.clip(q, 0, 255)
    return (q & 255).astype(np.uint8)


def panel_u8(hwc):
    return np.asarray(hwc, np.uint8)


def panel_grey(u8):
    """Image.fromarray(uint8 (w,w)) is mode L; pasted into an RGB image it is replicated."""
    return np.repeat(np.asarray(u8, np.uint8)[..., None], 3, axis=-1)


def panel_mask(m):
    """Image.fromarray(bool (w,w)) is mode 1; pasted into an RGB image it is 255 or 0, replicated."""
    return np.repeat((np.asarray(m) != 0)[..., None], 3, axis=-1).astype(np.uint8) * np.uint8(255)


PANEL_RULES = (panel_f32, panel_u8, panel_grey, panel_mask)        # indexed by the panel kind of include/cvae.h


def compose_ref(panels, ih=0, overlay=None, atlas=None, label=None, label_xy=(0, 0), clamp=False):
    """One picture (ih + w, n * w, 3) uint8 from [(kind, array), ...]; overlay (ih + w, n * w) and atlas[label] at label_xy
    (x, y) whiten pixels, clipped at the picture's edges."""
    tiles = [panel_f32(a, clamp) if k == 0 else PANEL_RULES[k](a) for k, a in panels]
    w = tiles[0].shape[0]
    pic = np.zeros((ih + w, len(tiles) * w, 3), np.uint8)
    pic[ih:] = np.concatenate(tiles, axis=1)
    white = np.zeros(pic.shape[:2], bool)
    if overlay is not None:
        white |= np.asarray(overlay) != 0
    if atlas is not None and label is not None and 0 <= label < atlas.shape[0]:
        g = atlas[label] != 0
        x, y = label_xy
        for gy in range(g.shape[0]):
            for gx in range(g.shape[1]):
                if g[gy, gx] and 0 <= y + gy < pic.shape[0] and 0 <= x + gx < pic.shape[1]:
                    white[y + gy, x + gx] = True
    pic[white] = 255
    return pic


def main():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    from critic_vae_amd import synth

    calls = []
    sys.modules["minerl"] = types.ModuleType("minerl")
    dcrf = types.ModuleType("denseCRF")
    dcrf.densecrf = lambda img, prob, param: (prob[..., 1] > 0.5).astype(np.uint8)
    sys.modules["denseCRF"] = dcrf
    from PIL import ImageDraw, ImageFont
    ImageFont.truetype = lambda *a, **k: None
    ImageDraw.ImageDraw.text = lambda self, xy, text, *a, **k: calls.append((int(xy[0]), int(xy[1]), str(text)))
    import vae_utility as vu                           # the reference
    import vae_nets
    import critic_net
    vu.save_bin_info = lambda *a, **k: None            # writes a file; make_segment_golden.py covers it

    torch.manual_seed(0)
    u8 = np.load(os.path.join(HERE, "step_real_b68.npz"))["u8"]
    seg_fx = np.load(os.path.join(HERE, "segment_real_b68.npz"))
    gt = seg_fx["gt"]
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
    n, w = u8.shape[0], u8.shape[1]

    with torch.no_grad():
        # the pieces by hand (the reference's own calls, frame by frame), to restate the pictures from
        frames, preds, ones, zeros, diffs, maxima, injected = [], [], [], [], [], [], []
        for img in u8:
            frame = vu.preprocess_observation(img)
            pred = critic.evaluate(frame)
            ro, rz, diff, mx = vu.get_diff_image(vae, frame, pred[0])
            frames.append(frame); preds.append(pred[0]); ones.append(ro); zeros.append(rz); diffs.append(diff); maxima.append(mx)
            injected.append(np.stack([vu.to_np(r.view(-1, 3, w, w)[0]) for r in vae.inject(frame)]))
        p32 = np.array([p.item() for p in preds], np.float32)
        assert np.array_equal(p32, seg_fx["preds"])

        # 1. eval_textured_frames: the video pictures
        calls.clear()
        video, thr_iou, crf_iou = vu.eval_textured_frames(u8, vae, critic, gt, t=THRESHOLD)
        video = [np.array(im) for im in video]
        text_video = list(calls)
        assert len(text_video) == 8 * n
        du8, thr = vu.get_diff_and_thr_masks([d.copy() for d in diffs], list(maxima), thr=THRESHOLD)
        du8 = du8.astype(np.uint8)

        # 2. the body of image_evaluate (vae.py:98-108)
        calls.clear()
        diff_factor, mean_max = vu.get_diff_factor(maxima)
        strips = []
        for i in range(n):
            d = vu.prepare_diff(diffs[i].copy(), diff_factor, mean_max)
            d = (d * 255).astype(np.uint8)
            assert np.array_equal(d, du8[i])
            from PIL import Image
            strips.append(np.array(vu.get_final_frame(frames[i], ones[i], zeros[i], Image.fromarray(d), preds[i])))
        text_strip = list(calls)
        assert len(text_strip) == n

        # 3. get_injected_img
        calls.clear()
        inj_strips = [np.array(vu.get_injected_img(vae, frames[i], preds[i])) for i in range(n)]
        assert not calls

    # the restatement equals the reference's PIL pictures, all 68 frames, all three layouts
    for i in range(n):
        f = frames[i].numpy()[0]
        assert np.array_equal(panel_f32(f), u8[i])                               # the frame panel is the uint8 frame
        v = compose_ref([(0, f), (0, ones[i]), (0, zeros[i]), (2, du8[i]), (3, thr[i]), (3, thr[i]), (3, gt[i])], ih=w)
        assert np.array_equal(v, video[i]), ("video", i)
        assert np.array_equal(compose_ref([(1, u8[i]), (0, ones[i]), (0, zeros[i]), (2, du8[i])]), strips[i]), ("strip", i)
        assert np.array_equal(compose_ref([(1, u8[i])] + [(0, injected[i][r]) for r in range(6)]), inj_strips[i]), ("inject", i)
        assert np.array_equal(injected[i][0], zeros[i])                          # reward 0 is recon_zero

    # frames to store: the most extreme critic value first, then the most negative reconstruction among the rest
    extreme = int(np.argmax(np.abs(p32 - 0.5)))
    assert p32[extreme] >= 0.95 or p32[extreme] <= 0.05, p32[extreme]
    neg = [min(ones[i].min(), zeros[i].min(), injected[i].min()) for i in range(n)]
    chosen = [extreme] + [int(i) for i in np.argsort(neg) if i != extreme][:K - 1]
    for i in chosen:
        assert neg[i] < 0, (i, neg[i])                                          # wrapped pixels occur in every stored frame
    fx = {"frames": np.array(chosen), "preds": p32, "thr_iou": thr_iou, "crf_iou": crf_iou, "threshold": THRESHOLD,
          "mean_max": mean_max,
          "video": np.stack([video[i] for i in chosen]), "strip": np.stack([strips[i] for i in chosen]),
          "inject": np.stack([inj_strips[i] for i in chosen]),
          "recon_one": np.stack([ones[i] for i in chosen]), "recon_zero": np.stack([zeros[i] for i in chosen]),
          "injected": np.stack([injected[i] for i in chosen]),
          "text_video_xy": np.array([[c[:2] for c in text_video[8 * i:8 * i + 8]] for i in range(n)], np.int32),
          "text_video": np.array([[c[2] for c in text_video[8 * i:8 * i + 8]] for i in range(n)]),
          "text_strip_xy": np.array([c[:2] for c in text_strip], np.int32), "text_strip": np.array([c[2] for c in text_strip])}
    out = os.path.join(HERE, "render_real.npz")
    np.savez_compressed(out, **fx)
    print(f"[render] frames {chosen} preds {p32[chosen]} min recon {[float(neg[i]) for i in chosen]} thr_iou {thr_iou} "
          f"{os.path.getsize(out)} bytes; labels {sorted(set(fx['text_strip'].tolist()))}")


if __name__ == "__main__":
    main()
