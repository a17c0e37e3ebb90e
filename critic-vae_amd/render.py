"""The reference's pictures, composed on the MI355X (cvae_compose_frames, csrc/render.hip).

    video_frames     get_final_frame with masks (vae_utility.py:286-322): per episode frame the 7-panel picture
                     [frame | recon(pred) | recon(0) | difference | thr-mask | thr-mask + crf | ground truth], (B, 2w, 7w, 3),
                     titles and the two IoUs in the black upper half, the critic value in the frame panel.
    evaluate_strips  image_evaluate (vae.py:68-108; `python vae.py`, `-evalsecond`): [frame | recon(pred) | recon(0) |
                     difference], (B, w, 4w, 3), the difference masks normalised over the whole set.
    inject_strips    get_injected_img (vae_utility.py:240-254; `python vae.py -inject`): [frame | recon at reward 0, 0.2,
                     ..., 1], (B, w, 7w, 3), no text.

Every picture is uint8 HWC on the device.  Reconstruction panels follow prepare_rgb_image, (img * 255).astype(np.uint8):
negative values of the Tanh output wrap modulo 256, as in the reference's pictures (clamp=True saturates instead).  The
frame panel is the uint8 frame itself: ((u / 255f) * 255f).astype(uint8) == u for all 256 values.  Text is white, at the
reference's positions, in a built-in 5 x 9 bitmap font (the reference's Ubuntu TTF is not needed; glyph shapes differ).

    python -m critic_vae_amd.render [-inject] [--second] --images PATH --networks DIR --critic CKPT --out DIR

PATH: an .npy (N,64,64,3) uint8 or, with PIL, a folder of image files in os.listdir order (as the reference reads
source-images/).  Without PIL the pictures are written as one .npy.
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import segment as seg
from .lib import PANEL_F32_CHW, PANEL_MASK, PANEL_U8_GREY, PANEL_U8_HWC

TITLES = ("orig img\n+crit val", "crit val\ninjected", "crit=0\ninjected", "difference\nmask", "thr-mask\nthr={thr}",
          "thr-mask +\ncrf", "ground\ntruth")                     # titles, vae_utility.py:19
INJECT_REWARDS = (0, .2, .4, .6, .8, 1)                           # vae_nets.py:33
TEXT_XY = (2, 0)                                                  # title i at (w * i + 2, 0); the critic value at (2, ih + 2)
LABEL_XY = (2, 2)

# ---- bitmap font: 5 x 9 cells (rows 0-1 ascenders, 2-6 x-height, 7-8 descenders), bit 4 = left column ----
GLYPH_W, GLYPH_H, ADVANCE, LINE_H = 5, 9, 6, 10
_FONT = {
    " ": (0, 0, 0, 0, 0, 0, 0, 0, 0),
    "0": (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E, 0, 0), "1": (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E, 0, 0),
    "2": (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F, 0, 0), "3": (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E, 0, 0),
    "4": (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02, 0, 0), "5": (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E, 0, 0),
    "6": (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E, 0, 0), "7": (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08, 0, 0),
    "8": (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E, 0, 0), "9": (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C, 0, 0),
    "a": (0, 0, 0x0E, 0x01, 0x0F, 0x11, 0x0F, 0, 0), "b": (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x1E, 0, 0),
    "c": (0, 0, 0x0E, 0x10, 0x10, 0x11, 0x0E, 0, 0), "d": (0x01, 0x01, 0x0D, 0x13, 0x11, 0x11, 0x0F, 0, 0),
    "e": (0, 0, 0x0E, 0x11, 0x1F, 0x10, 0x0E, 0, 0), "f": (0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08, 0, 0),
    "g": (0, 0, 0x0F, 0x11, 0x11, 0x11, 0x0F, 0x01, 0x0E), "h": (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x11, 0, 0),
    "i": (0x04, 0, 0x0C, 0x04, 0x04, 0x04, 0x0E, 0, 0), "j": (0x02, 0, 0x06, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C),
    "k": (0x10, 0x10, 0x12, 0x14, 0x18, 0x14, 0x12, 0, 0), "l": (0x0C, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E, 0, 0),
    "m": (0, 0, 0x1A, 0x15, 0x15, 0x15, 0x15, 0, 0), "n": (0, 0, 0x16, 0x19, 0x11, 0x11, 0x11, 0, 0),
    "o": (0, 0, 0x0E, 0x11, 0x11, 0x11, 0x0E, 0, 0), "p": (0, 0, 0x1E, 0x11, 0x11, 0x11, 0x1E, 0x10, 0x10),
    "q": (0, 0, 0x0F, 0x11, 0x11, 0x11, 0x0F, 0x01, 0x01), "r": (0, 0, 0x16, 0x19, 0x10, 0x10, 0x10, 0, 0),
    "s": (0, 0, 0x0F, 0x10, 0x0E, 0x01, 0x1E, 0, 0), "t": (0x08, 0x08, 0x1C, 0x08, 0x08, 0x09, 0x06, 0, 0),
    "u": (0, 0, 0x11, 0x11, 0x11, 0x13, 0x0D, 0, 0), "v": (0, 0, 0x11, 0x11, 0x11, 0x0A, 0x04, 0, 0),
    "w": (0, 0, 0x11, 0x11, 0x15, 0x15, 0x0A, 0, 0), "x": (0, 0, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0, 0),
    "y": (0, 0, 0x11, 0x11, 0x11, 0x11, 0x0F, 0x01, 0x0E), "z": (0, 0, 0x1F, 0x02, 0x04, 0x08, 0x1F, 0, 0),
    ".": (0, 0, 0, 0, 0, 0x0C, 0x0C, 0, 0), "=": (0, 0, 0, 0x1F, 0, 0x1F, 0, 0, 0),
    "+": (0, 0, 0x04, 0x04, 0x1F, 0x04, 0x04, 0, 0), "-": (0, 0, 0, 0, 0x1F, 0, 0, 0, 0),
}
_BITS = {c: ((np.array(rows, np.uint8)[:, None] >> np.arange(GLYPH_W - 1, -1, -1)) & 1).astype(np.uint8) for c, rows in _FONT.items()}


def glyph_boxes(x, y, string):
    """[(char, x0, y0, x1, y1), ...]: the cell of every character but newlines of `string` drawn with its top left corner
    at (x, y); lines are LINE_H apart, characters ADVANCE."""
    out = []
    for li, line in enumerate(string.split("\n")):
        for ci, ch in enumerate(line):
            if ch not in _BITS:
                raise ValueError(f"no glyph for {ch!r} (the font has digits, lower-case letters and '. = + -')")
            x0, y0 = x + ci * ADVANCE, y + li * LINE_H
            out.append((ch, x0, y0, x0 + GLYPH_W, y0 + GLYPH_H))
    return out


def draw_text(canvas, x, y, string):
    """Set the glyph pixels of `string` in the (H, W) uint8 canvas to 255, clipped at its edges."""
    H, W = canvas.shape
    for ch, x0, y0, x1, y1 in glyph_boxes(x, y, string):
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        if cx0 < cx1 and cy0 < cy1:
            canvas[cy0:cy1, cx0:cx1] |= _BITS[ch][cy0 - y0:cy1 - y0, cx0 - x0:cx1 - x0] * np.uint8(255)
    return canvas


def title_calls(w, thr_iou=None, crf_iou=None, threshold=seg.THRESHOLD):
    """The draw.text calls of get_final_frame's title loop (vae_utility.py:311-317): [(x, y, string), ...]."""
    calls = []
    for i, title in enumerate(TITLES):
        title = title.format(thr=threshold)
        if i == 4 and thr_iou is not None:
            title += f"\niou={thr_iou}"
        elif i == 5 and crf_iou is not None:
            title += f"\niou={crf_iou}"
        calls.append((w * i + TEXT_XY[0], TEXT_XY[1], title))
    return calls


def title_overlay(w, thr_iou=None, crf_iou=None, threshold=seg.THRESHOLD):
    """(2w, 7w) uint8: the titles of the video picture, nonzero = white."""
    canvas = np.zeros((2 * w, len(TITLES) * w), np.uint8)
    for x, y, s in title_calls(w, thr_iou, crf_iou, threshold):
        draw_text(canvas, x, y, s)
    return canvas


def label_index(preds):
    """round-half-even(10 * pred) in float64, where 10 * float32 is exact: k such that f'{pred:.1f}' == f'{k / 10:.1f}'
    (Python formats the exact binary value, correctly rounded, ties to even).  numpy array or tensor of float32 in,
    int64 of the same kind out."""
    if torch.is_tensor(preds):
        return torch.round(preds.to(torch.float32).to(torch.float64) * 10).to(torch.int64)
    return np.rint(np.asarray(preds, np.float32).astype(np.float64) * 10).astype(np.int64)


def label_strings(lo=0, hi=10):
    """The strings f'{pred:.1f}' can give for label indices lo..hi: 11 of them for a critic value in [0, 1]."""
    return [f"{k / 10:.1f}" for k in range(lo, hi + 1)]


def label_atlas(strings):
    """(L, GLYPH_H, width of the longest string) uint8 atlas of one-line labels."""
    lw = max(len(s) for s in strings) * ADVANCE - (ADVANCE - GLYPH_W)
    atlas = np.zeros((len(strings), GLYPH_H, lw), np.uint8)
    for i, s in enumerate(strings):
        draw_text(atlas[i], 0, 0, s)
    return atlas


def _labels(preds, device):
    """(atlas (L, lh, lw) uint8, index (B) int32) on the device for the critic values `preds` (B) on the device."""
    k = label_index(preds.reshape(-1))
    finite = torch.isfinite(preds.reshape(-1))
    kf = torch.where(finite, k, torch.zeros_like(k))
    lo, hi = min(int(kf.min()), 0), max(int(kf.max()), 10)
    if hi - lo > 4096:
        raise ValueError(f"critic values span {lo / 10}..{hi / 10}: too many labels")
    atlas = torch.from_numpy(label_atlas(label_strings(lo, hi))).to(device)
    idx = torch.where(finite, k - lo, torch.full_like(k, -1)).to(torch.int32).contiguous()     # non-finite: no label
    return atlas, idx


def _dev(a, dtype, device="cuda"):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device, dtype).contiguous()


def compose(width, panels, row_offset=0, overlay=None, preds=None, clamp=False):
    """panels [(kind, (B, ...) device tensor), ...] -> (B, row_offset + w, len(panels) * w, 3) uint8 on the device, one launch.
    overlay: (row_offset + w, len(panels) * w) uint8 array or None; preds: critic values (B) whose f'{:.1f}' goes to
    (2, row_offset + 2), or None."""
    B, dev = panels[0][1].shape[0], panels[0][1].device
    h = seg._handle(width)
    out = torch.empty(B, row_offset + width, len(panels) * width, 3, dtype=torch.uint8, device=dev)
    desc = []
    for kind, t in panels:
        if t.shape[0] != B:
            raise ValueError(f"panel batch {t.shape[0]} != {B}")
        desc.append((kind, t, t.stride(0) if t.dim() > 1 else 0))
    ov = None if overlay is None else _dev(overlay, torch.uint8, dev)
    atlas = idx = None
    if preds is not None:
        atlas, idx = _labels(_dev(preds, torch.float32, dev), dev)
    h.compose_frames(B, [(k, _flat(t), s) for k, t, s in desc], row_offset, out, ov, atlas, idx,
                     (LABEL_XY[0], row_offset + LABEL_XY[1]), clamp)
    return out


def _flat(t):
    """The tensor's own memory from its first element on, as a contiguous 1-D view (for a batch-strided panel such as
    injected[:, r] of a (B, R, 3, w, w) tensor)."""
    if t.is_contiguous():
        return t
    base = t._base if t._base is not None else t
    assert base.is_contiguous(), "panel: a view of a contiguous tensor is needed"
    return base.reshape(-1)[t.storage_offset() - base.storage_offset():]


def video_frames(result, text=True, clamp=False, threshold=seg.THRESHOLD):
    """The 7-panel pictures (B, 2w, 7w, 3) uint8 on the device.  `result`: what segment.eval_frames(..., keep_device=True)
    returned, or a dict of the inputs themselves (arrays or tensors): frames (B,w,w,3) uint8, recon_one, recon_zero (B,3,w,w)
    fp32, diff_u8, thr_masks, crf_masks, gt (B,w,w), preds (B), and thr_iou / crf_iou for the text."""
    d = result.get("device", result)
    frames = _dev(d["frames"], torch.uint8)
    w = frames.shape[1]
    panels = [(PANEL_U8_HWC, frames), (PANEL_F32_CHW, _dev(d["recon_one"], torch.float32)),
              (PANEL_F32_CHW, _dev(d["recon_zero"], torch.float32)), (PANEL_U8_GREY, _dev(d["diff_u8"], torch.uint8)),
              (PANEL_MASK, _dev(d["thr_masks"], torch.uint8)), (PANEL_MASK, _dev(d["crf_masks"], torch.uint8)),
              (PANEL_MASK, _dev(d["gt"], torch.uint8))]
    overlay = title_overlay(w, result.get("thr_iou"), result.get("crf_iou"), threshold) if text else None
    return compose(w, panels, w, overlay, d["preds"] if text else None, clamp)


def _preprocess(frames, vae):
    B, w = frames.shape[0], frames.shape[1]
    x = torch.empty(B, 3, w, w, device=frames.device)
    for s in range(0, B, vae.max_batch):
        e = min(B, s + vae.max_batch)
        vae.handle.preprocess_u8(e - s, frames[s:e], x[s:e])
    return x


def evaluate_strips(frames_u8, vae, critic=None, preds=None, text=True, clamp=False, chunk=None, return_parts=False):
    """image_evaluate (vae.py:68-108) for a whole set at once: critic, difference masks, the mean of their maxima over the
    SET, cvae_diff_normalize, one compose launch -> (B, w, 4w, 3) uint8 on the device.  return_parts: also the dict of
    device tensors it was composed from (preds, recon_one, recon_zero, diff_u8) and mean_max."""
    p, diff, maxv, ro, rz = seg._infer(frames_u8, vae, critic, preds, chunk, keep_recons=True)
    frames = _dev(frames_u8, torch.uint8)
    u8, mean_max = seg.normalize_diffs(diff, maxv.cpu())
    pics = compose(frames.shape[1], [(PANEL_U8_HWC, frames), (PANEL_F32_CHW, ro), (PANEL_F32_CHW, rz), (PANEL_U8_GREY, u8)],
                   0, None, p if text else None, clamp)
    if return_parts:
        return pics, {"preds": p, "recon_one": ro, "recon_zero": rz, "diff_u8": u8, "mean_max": mean_max}
    return pics


def inject_strips(frames_u8, vae, rewards=INJECT_REWARDS, clamp=False, return_parts=False):
    """get_injected_img (vae_utility.py:240-254) for a whole set: (B, w, (1 + len(rewards)) w, 3) uint8 on the device."""
    vae.eval()                                   # load_vae_network (vae_utility.py:345-361)
    frames = _dev(frames_u8, torch.uint8)
    if frames.shape[1] != vae.width:
        raise ValueError(f"frames are {frames.shape[1]}x{frames.shape[1]}, the VAE is {vae.width}x{vae.width}")
    inj = vae.inject_images(_preprocess(frames, vae), rewards)
    pics = compose(frames.shape[1], [(PANEL_U8_HWC, frames)] + [(PANEL_F32_CHW, inj[:, r]) for r in range(inj.shape[1])],
                   0, None, None, clamp)
    return (pics, {"injected": inj}) if return_parts else pics


# ---- writers ----
def _pil_image():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def _host(pictures):
    a = pictures.cpu().numpy() if torch.is_tensor(pictures) else np.asarray(pictures)
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[-1] == 3, (a.dtype, a.shape)
    return a


def save_pngs(directory, pictures, pattern="image-{i:03d}.png", npy=False):
    """One PNG per picture (the reference's file names), or — without PIL, or with npy=True — DIR/pictures.npy holding the
    whole uint8 array.  Returns the paths written."""
    a = _host(pictures)
    os.makedirs(directory, exist_ok=True)
    Image = None if npy else _pil_image()
    if Image is None:
        path = os.path.join(directory, "pictures.npy")
        np.save(path, a)
        return [path]
    paths = []
    for i, pic in enumerate(a):
        paths.append(os.path.join(directory, pattern.format(i=i)))
        Image.fromarray(pic, mode="RGB").save(paths[-1], format="png")
    return paths


def save_gif(path, pictures, duration=100, loop=0, npy=False):
    """create_video (vae_utility.py:85-104): an animated GIF through PIL (its palette quantisation, on the host); without
    PIL, or with npy=True, PATH + '.npy' holding the uint8 array.  Returns the path written."""
    a = _host(pictures)
    Image = None if npy else _pil_image()
    if Image is None:
        np.save(path + ".npy", a)
        return path + ".npy"
    imgs = [Image.fromarray(pic, mode="RGB") for pic in a]
    imgs[0].save(path, format="GIF", duration=duration, save_all=True, loop=loop, append_images=imgs[1:])
    return path


def load_images(path):
    """(N,w,w,3) uint8 from an .npy, or from a folder of image files in os.listdir order (needs PIL)."""
    if os.path.isdir(path):
        Image = _pil_image()
        if Image is None:
            raise RuntimeError(f"{path} is a folder of image files: reading them needs PIL; pass an .npy (N,64,64,3) uint8")
        return np.stack([np.array(Image.open(os.path.join(path, f)).convert("RGB")) for f in os.listdir(path)])
    a = np.load(path)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3 or a.shape[1] != a.shape[2]:
        raise ValueError(f"{path}: need (N,w,w,3) uint8, got {a.dtype} {a.shape}")
    return a


# ---- CLI (vae.py without a flag, -evalsecond, -inject: image_evaluate, vae.py:68-108) ----
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m critic_vae_amd.render",
                                 description="the reference's evaluation strips of a set of images, composed on the device")
    ap.add_argument("-inject", action="store_true", help="strips [frame | recon at reward 0, 0.2, ..., 1] (vae.py -inject) "
                    "instead of [frame | recon(pred) | recon(0) | difference]")
    ap.add_argument("--second", action="store_true", help="the second VAE, NETWORKS/vae2_*.pt (the reference's -evalsecond)")
    ap.add_argument("--images", required=True, help=".npy (N,64,64,3) uint8, or a folder of image files (needs PIL)")
    ap.add_argument("--networks", default="saved-networks", help=f"directory with {seg.ENCODER_FILE} and {seg.DECODER_FILE}")
    ap.add_argument("--critic", default=None, help=f"critic checkpoint (default: NETWORKS/{seg.CRITIC_FILE})")
    ap.add_argument("--out", required=True, help="directory for image-000.png, ... (pictures.npy without PIL)")
    ap.add_argument("--chunk", type=int, default=256, help="frames per VAE launch")
    ap.add_argument("--no-text", dest="text", action="store_false", help="no critic value in the frame panel")
    ap.add_argument("--npy", action="store_true", help="write OUT/pictures.npy even where PIL is installed")
    args = ap.parse_args(argv)
    if args.chunk < 6:
        ap.error("--chunk must be >= 6 (one image's six injections go through one decoder call)")
    if args.critic is None:
        args.critic = os.path.join(args.networks, seg.CRITIC_FILE)
    return args


def main(argv=None):
    args = parse_args(argv)
    from .critic import Critic
    from .lib import Handle
    from .nets import VariationalAutoencoder
    from .train import load_networks
    images = load_images(args.images)
    vae = VariationalAutoencoder(width=images.shape[1], max_batch=args.chunk).to("cuda")
    load_networks(vae, args.networks, second=args.second)
    if args.inject:                              # the reference evaluates the critic here too, but the strip does not show it
        pics = inject_strips(images, vae)
    else:
        critic = Critic(64, handle=Handle(64, args.chunk)).to("cuda")
        critic.load_state_dict(torch.load(args.critic, map_location="cpu"))
        pics = evaluate_strips(images, vae, critic=critic, text=args.text, chunk=args.chunk)
    paths = save_pngs(args.out, pics, npy=args.npy)
    print(f"wrote {pics.shape[0]} pictures {tuple(pics.shape[1:])} to {args.out} ({len(paths)} file{'s' if len(paths) != 1 else ''})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
