"""Critic-guided segmentation: the evaluation of `python vae.py -video [-thresh]` (eval_textured_frames,
vae_utility.py:162-212) on the MI355X.

Per frame the critic value and the difference mask (VariationalAutoencoder.diff_images); over the whole set the
normalisation by the mean of the per-frame maxima, the uint8 mask and its threshold (cvae_diff_normalize), the
IoU against the ground truth, a dense CRF that refines every thresholded mask (cvae_dense_crf) and a second IoU,
and the per-critic-value-bin statistics of save_bin_info.  The 7-panel pictures of get_final_frame are composed on the
device by critic_vae_amd.render (`--out DIR` writes them, `--gif` also the GIF).

The CRF is an EXACT mean-field solution of the model SimpleCRF's denseCRF.densecrf names (include/cvae.h): every
pairwise sum runs over all pixel pairs, where the densecrf library approximates the bilateral filter with a
permutohedral lattice.  Its unary clamps probabilities at `p_floor` (default 1e-5, the `clip` default of the common
unary_from_softmax helper); whether SimpleCRF clamps a 0/1 mask the same way has not been checked against SimpleCRF.

    python -m critic_vae_amd.segment -video [-thresh] --frames X.npy --gt Y.npy --networks DIR [--critic CKPT]
                                     [--out DIR [--gif] [--no-text]] [--thr T] [--crf W1,ALPHA,BETA,W2,GAMMA,IT] [--p-floor F]
                                     [--objects [--connectivity 4|8] [--fill-holes] [--min-area A] [--keep-largest K]
                                      [--max-objects M] [--objects-out FILE.npz]]
    python -m critic_vae_amd.segment -video -search [--grid-thr 0,10,...] [--grid-w1 ...] ... [--skip N] [--top N]

`-search` is the grid search the reference's crf() is written as (lists for every parameter, the IoU per tuple): every
threshold and every (w1, w2, p_floor) of one (alpha, beta, gamma) ride on one pairwise pass (crf_search / cvae_crf_grid).

`--mask-source critic-grad | critic-ig | critic-occlusion` builds the masks from the critic alone (critic_maps: the
gradient of its logit with respect to the pixels, integrated gradients, occlusion sensitivity) and sends them through the
same tail (eval_maps / sweep_maps): the baselines that show what the VAE adds.  No pictures for these sources.

`--objects` reports the thresholded and the CRF mask as objects as well (critic_vae_amd.objects: connected components after an
optional hole fill and area filter, matched with the ground truth's components at IoU > 0.5): precision, recall and panoptic
quality per mask kind, for every mask source.
"""
import argparse
import os
import statistics
import sys
from collections import defaultdict

import numpy as np
import torch

from .lib import CrfParams, Handle

CRF_REF = (22, 12, 3.1, 8, 1.8, 10)     # (w1, alpha, beta, w2, gamma, it) of crf(), vae_utility.py:25-30
THRESHOLD = 50                          # vae_utility.py:17
P_FLOOR = 1e-5                          # unary clamp (unary_from_softmax's clip default; unverified against SimpleCRF)
SWEEP = tuple(range(0, 130, 10))        # the -thresh loop, vae.py:121
BIN_FRAMES_DENOM = 1200                 # save_bin_info_file divides frame counts by a fixed 1200 (vae_utility.py:123)
ENCODER_FILE, DECODER_FILE = "vae_encoder.pt", "vae_decoder.pt"            # vae_parameters.py:29-30
CRITIC_FILE = "critic-rewidx=1-cepochs=15-datamode=trunk-datasize=99999-shift=12-chfak=1-dropout=0.3.pt"   # vae_parameters.py:46

_handles = {}


def _handle(width):
    """A library handle for the entries that need only the frame width (none of them is capped by max_batch)."""
    dev = torch.cuda.current_device()
    h = _handles.get((width, dev))
    if h is None:
        h = _handles[(width, dev)] = Handle(width, 1)
    return h


def _cuda(a, dtype):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype).contiguous()


def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


# ---- IoU (get_iou, vae_utility.py:56-68) ----
def iou_from_counts(tp, fn, fp):
    """tp / (tp + fn + fp), 1 when the union is empty, rounded to 3 places on the host."""
    tp, fn, fp = int(tp), int(fn), int(fp)
    if tp + fn + fp == 0:
        return 1
    return round(tp / (tp + fn + fp), 3)


def iou(G, T):
    """get_iou(G, T) on boolean arrays of any (equal) shape."""
    G, T = _np(G).astype(bool), _np(T).astype(bool)
    return iou_from_counts(np.sum(G & T), np.sum(G & ~T), np.sum(~G & T))


def iou_from_hist(hist, t):
    """Set-wide IoU of the mask diff_u8 > t from the (2,256) histograms of cvae_diff_normalize (row 0: gt set,
    row 1: gt clear): a threshold sweep never re-reads the masks."""
    hist = _np(hist).astype(np.int64)
    return iou_from_counts(hist[0, t + 1:].sum(), hist[0, :t + 1].sum(), hist[1, t + 1:].sum())


# ---- normalisation + threshold (get_diff_factor / prepare_diff / get_diff_and_thr_masks) ----
def diff_factor(max_values):
    """get_diff_factor (vae_utility.py:106-110): (1 / mean_max or 0, mean_max), mean_max = statistics.mean."""
    mean_max = statistics.mean(float(m) for m in _np(max_values).reshape(-1))
    return (1.0 / mean_max if mean_max != 0 else 0), mean_max


def _normalize(diff, max_values, t=THRESHOLD, gt=None, mask=False, counts=False, hist=None):
    diff = _cuda(diff, torch.float32)
    B, W = diff.shape[0], diff.shape[-1]
    factor, mean_max = diff_factor(max_values)
    u8 = torch.empty(B, W, W, dtype=torch.uint8, device=diff.device)
    m = torch.empty_like(u8) if mask else None
    c = torch.empty(B, 3, dtype=torch.int64, device=diff.device) if counts else None
    _handle(W).diff_normalize(B, diff, mean_max, factor, t, gt, u8, m, c, hist)
    return u8, m, c, mean_max


def normalize_diffs(diff, max_values):
    """(B,W,W) float difference masks + per-frame maxima -> (diff_u8 (B,W,W) uint8 on the device, mean_max):
    trunc((min(d, mean_max) * diff_factor) * 255) in float64, as prepare_diff + astype(np.uint8)."""
    u8, _, _, mean_max = _normalize(diff, max_values)
    return u8, mean_max


def threshold_masks(diff, max_values, t=THRESHOLD):
    """get_diff_and_thr_masks (vae_utility.py:148-160): (diff_u8, diff_u8 > t), both (B,W,W) on the device."""
    u8, m, _, _ = _normalize(diff, max_values, t, mask=True)
    return u8, m.bool()


# ---- dense CRF (crf, vae_utility.py:22-54) ----
def crf_params(params=CRF_REF, p_floor=P_FLOOR):
    w1, alpha, beta, w2, gamma, it = params
    return CrfParams(float(w1), float(alpha), float(beta), float(w2), float(gamma), float(p_floor), int(it))


def dense_crf(frames_u8, prob_or_mask, params=CRF_REF, p_floor=P_FLOOR, return_q1=False):
    """frames_u8 (B,W,W,3) uint8 RGB, prob_or_mask (B,W,W): a 0/1 mask or the probability of label 1 (the
    reference passes prob = stack(1 - m, m)) -> labels (B,W,W) bool on the device [, Q(1) (B,W,W) fp32].
    One call for any B; params = (w1, alpha, beta, w2, gamma, it)."""
    frames = _cuda(frames_u8, torch.uint8)
    prob1 = _cuda(prob_or_mask, torch.float32)
    B, W = frames.shape[0], frames.shape[1]
    assert frames.shape == (B, W, W, 3) and prob1.shape == (B, W, W), (tuple(frames.shape), tuple(prob1.shape))
    h = _handle(W)
    p = crf_params(params, p_floor)
    labels = torch.empty(B, W, W, dtype=torch.uint8, device=frames.device)
    q1 = torch.empty(B, W, W, device=frames.device) if return_q1 else None
    scratch = torch.empty(h.crf_scratch_bytes(B), dtype=torch.uint8, device=frames.device)
    h.dense_crf(B, frames, prob1, p, labels, q1, scratch)
    return (labels.bool(), q1) if return_q1 else labels.bool()


def mask_counts(mask, gt):
    """per-frame (tp, fn, fp) of get_iou(gt, mask), (B,3) int64 on the device"""
    mask, gt = _cuda(mask, torch.uint8), _cuda(gt, torch.uint8)
    c = torch.empty(mask.shape[0], 3, dtype=torch.int64, device=mask.device)
    _handle(mask.shape[-1]).mask_counts(mask.shape[0], mask, gt, c)
    return c


# ---- the grid search of crf() (vae_utility.py:22-54: lists for every parameter, the IoU per tuple, a `skip`) ----
GRID_SCRATCH_LIMIT = 4 << 30            # crf_search's default frame chunk keeps a call's scratch under this many bytes
PROB1 = -1                              # a variant's thr that selects the prob1 plane instead of a threshold of diff_u8


def crf_grid(frames_u8, gt, kernel, variants, its=(CRF_REF[5],), prob1=None, diff_u8=None, labels=False, q1=False):
    """cvae_crf_grid: the dense CRF for every variant (thr, p_floor, w1, w2) of one frame set under one kernel
    (alpha, beta, gamma); thr = -1 takes `prob1` (B,W,W) fp32, thr in 0..255 the mask `diff_u8` > thr.  `its`: ascending
    iteration counts; with gt, counts (len(its), K, B, 3) int64 hold the per-frame (tp, fn, fp) after each.  Returns the counts
    (None without gt) on the device; with labels and / or q1 a tuple (counts, labels (K,B,W,W) bool, Q(1) (K,B,W,W) fp32) of
    what was asked for, both at the last of `its`."""
    frames = _cuda(frames_u8, torch.uint8)
    B, W = frames.shape[0], frames.shape[1]
    assert frames.shape == (B, W, W, 3), tuple(frames.shape)
    dev = frames.device
    gt_d = None if gt is None else _cuda(gt if torch.is_tensor(gt) else _np(gt).astype(np.uint8), torch.uint8)
    p1 = None if prob1 is None else _cuda(prob1, torch.float32)
    u8 = None if diff_u8 is None else _cuda(diff_u8, torch.uint8)
    for t in (gt_d, p1, u8):
        assert t is None or t.shape == (B, W, W), tuple(t.shape)
    variants, its = [tuple(v) for v in variants], [int(i) for i in its]
    K = len(variants)
    h = _handle(W)
    counts = torch.empty(len(its), K, B, 3, dtype=torch.int64, device=dev) if gt_d is not None else None
    lab = torch.empty(K, B, W, W, dtype=torch.uint8, device=dev) if labels else None
    q = torch.empty(K, B, W, W, device=dev) if q1 else None
    scratch = torch.empty(h.crf_grid_scratch_bytes(B, K), dtype=torch.uint8, device=dev)
    h.crf_grid(B, frames, p1, u8, gt_d, kernel, variants, its, counts, lab, q, scratch)
    if not labels and not q1:
        return counts
    return (counts,) + ((lab.bool(),) if labels else ()) + ((q,) if q1 else ())


def grid_plan(thresholds=SWEEP, w1=(CRF_REF[0],), alpha=(CRF_REF[1],), beta=(CRF_REF[2],), w2=(CRF_REF[3],),
              gamma=(CRF_REF[4],), it=(CRF_REF[5],), p_floor=(P_FLOOR,)):
    """The grid as calls of crf_grid (host only).  Returns (rows, calls): rows, in grid order (thr, p_floor, then the
    reference's nesting w1, alpha, beta, w2, gamma, it), are (thr, (w1, alpha, beta, w2, gamma, it), p_floor, call, variant,
    snapshot); calls, in order of first use, are ((alpha, beta, gamma), [(thr, p_floor, w1, w2), ...], sorted its): one per
    kernel, every thresholds x p_floor x w1 x w2 a variant, every `it` a snapshot."""
    its = sorted(set(int(i) for i in it))
    calls, call_of, var_of, rows = [], {}, [], []
    for t in thresholds:
        for pf in p_floor:
            for a in w1:
                for b in alpha:
                    for c in beta:
                        for d in w2:
                            for e in gamma:
                                kern = (float(b), float(c), float(e))
                                if kern not in call_of:
                                    call_of[kern] = len(calls)
                                    calls.append((kern, [], its))
                                    var_of.append({})
                                ci = call_of[kern]
                                var = (int(t), float(pf), float(a), float(d))
                                if var not in var_of[ci]:
                                    var_of[ci][var] = len(calls[ci][1])
                                    calls[ci][1].append(var)
                                for i in it:
                                    rows.append((t, (a, b, c, d, e, i), pf, ci, var_of[ci][var], its.index(int(i))))
    return rows, calls


def rank_rows(rows):
    """Best crf_iou first; ties of the 3-place value go to the larger unrounded tp / (tp + fn + fp) (1 for an empty union),
    then to grid order (the sort is stable).  The reference sorts ascending and discards the result."""
    def ratio(r):
        tp, fn, fp = r["counts"]
        return tp / (tp + fn + fp) if tp + fn + fp else 1.0
    return sorted(rows, key=lambda r: (-r["crf_iou"], -ratio(r)))


def _grid_chunk(h, B, K, limit=GRID_SCRATCH_LIMIT):
    per_frame = h.crf_grid_scratch_bytes(1, K)
    return max(1, min(B, (limit - 4096) // per_frame))


def crf_search(frames_u8, maps, max_values, gt, thresholds=SWEEP, w1=(CRF_REF[0],), alpha=(CRF_REF[1],), beta=(CRF_REF[2],),
               w2=(CRF_REF[3],), gamma=(CRF_REF[4],), it=(CRF_REF[5],), p_floor=(P_FLOOR,), skip=1, chunk=None):
    """The grid search of the reference's crf() over thresholds and CRF parameters, for any non-negative map (B,W,W) with its
    per-frame maxima (as sweep_maps takes them).  `skip` evaluates frames [::skip], as crf() does.  The masks are normalised
    once (thr_iou from the histograms); per (alpha, beta, gamma) and per chunk of `chunk` frames (default: as many as keep the
    scratch under 4 GiB) ONE crf_grid call serves every thresholds x p_floor x w1 x w2 as a variant and every `it` as a
    snapshot.  Counts are summed over the frames on the device and read once.  Returns a list of dicts {"thr", "params":
    (w1, alpha, beta, w2, gamma, it), "p_floor", "thr_iou", "crf_iou", "counts": (tp, fn, fp)}, best crf_iou first (rank_rows)."""
    skip = int(skip)
    if skip < 1:
        raise ValueError(f"skip {skip} must be >= 1")
    frames = _cuda(frames_u8, torch.uint8)[::skip].contiguous()
    diff = _cuda(maps, torch.float32)[::skip].contiguous()
    gt_d = _cuda(_np(gt).astype(np.uint8), torch.uint8)[::skip].contiguous()
    maxv = _cuda(max_values, torch.float32).reshape(-1)[::skip].cpu()
    B, W = frames.shape[0], frames.shape[1]
    rows, calls = grid_plan(thresholds, w1, alpha, beta, w2, gamma, it, p_floor)
    hist = torch.zeros(2, 256, dtype=torch.int64, device=frames.device)
    u8, _, _, _ = _normalize(diff, maxv, 0, gt=gt_d, hist=hist)
    h = _handle(W)
    sums = []
    for kern, variants, its in calls:
        total = torch.zeros(len(its), len(variants), 3, dtype=torch.int64, device=frames.device)
        for v0 in range(0, len(variants), 64):                            # CVAE_CRF_GRID_MAX_VARIANTS per call
            vs = variants[v0:v0 + 64]
            step = int(chunk) if chunk else _grid_chunk(h, B, len(vs))
            for s in range(0, B, step):
                e = min(B, s + step)
                total[:, v0:v0 + len(vs)] += crf_grid(frames[s:e], gt_d[s:e], kern, vs, its, diff_u8=u8[s:e]).sum(2)
        sums.append(total)
    host = torch.cat([t.reshape(-1) for t in sums] + [hist.reshape(-1)]).cpu().numpy()          # the one read
    sums = [a.reshape(t.shape) for a, t in zip(np.split(host[:-512], np.cumsum([t.numel() for t in sums])[:-1]), sums)]
    hist = host[-512:].reshape(2, 256)
    out = []
    for t, params, pf, ci, vi, si in rows:
        c = tuple(int(x) for x in sums[ci][si, vi])
        out.append({"thr": t, "params": params, "p_floor": pf, "thr_iou": iou_from_hist(hist, t), "crf_iou": iou_from_counts(*c),
                    "counts": c})
    return rank_rows(out)


# ---- per-critic-value bins (save_bin_info / save_bin_info_file, vae_utility.py:112-146) ----
def bin_info(preds, gt, thr_masks):
    """{"ious", "frames", "gts"}: dicts keyed by round(pred, 1) in first-seen order, as save_bin_info builds them."""
    preds = _np(preds).reshape(-1)
    gt, thr_masks = _np(gt).astype(bool), _np(thr_masks).astype(bool)
    ious, frames, gts = defaultdict(list), defaultdict(int), defaultdict(int)
    for i, pred in enumerate(preds):
        b = round(float(pred), 1)
        ious[b].append(iou(thr_masks[i], gt[i]))
        frames[b] += 1
        gts[b] += gt[i].sum()
    return {"ious": dict(ious), "frames": dict(frames), "gts": dict(gts)}


def bin_info_text(bins):
    """The text of save_bin_info_file.  Where the reference's statistics.stdev raises (a bin of one frame), the
    std is written as nan; a set without ground-truth pixels gives nan percentages, as numpy's division does."""
    ious, frames, gts = bins["ious"], bins["frames"], bins["gts"]
    total_gt = np.sum(list(gts.values()))
    out = ["ground truth pixels sorted by bin:\n"]
    with np.errstate(divide="ignore", invalid="ignore"):
        for b, count in gts.items():
            out.append(f"bin: {b}, pixels = {count} = {round(np.int64(count) / total_gt, 2) * 100}%\n")
    out.append("\nframes separated by bin:\n")
    for b, count in frames.items():
        out.append(f"bin: {b}, frames = {count} = {round(count / BIN_FRAMES_DENOM, 2) * 100}%\n")
    out.append("\niou-mean and std:\n")
    for b, vals in ious.items():
        mean = round(statistics.mean(vals), 2)
        std = round(statistics.stdev(vals), 2) if len(vals) > 1 else float("nan")
        out.append(f"bin: {b}, iou_mean={mean}, iou_std={std}\n")
    return "".join(out)


def write_bin_info(path, bins):
    """save_bin_info_file's file (the reference writes bin_info_vae1.txt in the working directory)."""
    with open(path, "w") as f:
        f.write(bin_info_text(bins))


# ---- the pipeline ----
def _infer(frames_u8, vae, critic, preds, chunk, keep_recons=False):
    """critic values + difference masks of every frame, in chunks of at most vae.max_batch:
    (preds (B,) fp32, diff (B,W,W) fp32 on the device, per-frame maxima (B,) fp32); with keep_recons also the two
    reconstructions (B,3,W,W) the masks came from."""
    if (critic is None) == (preds is None):
        raise ValueError("pass exactly one of critic and preds")
    vae.eval()                                   # load_vae_network (vae_utility.py:345-361)
    vae.encoder.eval()
    vae.decoder.eval()
    frames = _cuda(frames_u8, torch.uint8)
    B, W = frames.shape[0], frames.shape[1]
    if W != vae.width:
        raise ValueError(f"frames are {W}x{W}, the VAE is {vae.width}x{vae.width}")
    chunk = min(int(chunk or vae.max_batch), vae.max_batch)
    if preds is not None:
        preds = _cuda(preds, torch.float32).reshape(-1)
        if preds.shape[0] != B:
            raise ValueError(f"{preds.shape[0]} preds for {B} frames")
    out_p = torch.empty(B, device=frames.device)
    diff = torch.empty(B, W, W, device=frames.device)
    maxv = torch.empty(B, device=frames.device)
    x = torch.empty(chunk, 3, W, W, device=frames.device)
    ro = torch.empty(B, 3, W, W, device=frames.device) if keep_recons else None
    rz = torch.empty_like(ro) if keep_recons else None
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        xs = x[:e - s]
        vae.handle.preprocess_u8(e - s, frames[s:e], xs)
        if critic is not None:
            cb = critic.handle.max_batch
            for c0 in range(0, e - s, cb):
                out_p[s + c0:s + min(e - s, c0 + cb)] = critic.evaluate(xs[c0:c0 + cb]).reshape(-1)
        else:
            out_p[s:e] = preds[s:e]
        r1, r0, d, m = vae.diff_images(xs, out_p[s:e])
        diff[s:e] = d
        maxv[s:e] = m
        if keep_recons:
            ro[s:e] = r1
            rz[s:e] = r0
    return (out_p, diff, maxv, ro, rz) if keep_recons else (out_p, diff, maxv)


def _crf_counts(frames, thr_mask, gt, crf_params_, p_floor):
    crf = dense_crf(frames, thr_mask, crf_params_, p_floor)
    c = mask_counts(crf, gt).sum(0).tolist()
    return crf, iou_from_counts(*c)


MASK_SOURCES = {"vae": None, "critic-grad": "grad", "critic-ig": "ig", "critic-occlusion": "occlusion"}      # --mask-source
IG_STEPS, OCCLUSION_PATCH = 32, 8


def critic_maps(frames_u8, critic, source="grad", steps=IG_STEPS, patch=OCCLUSION_PATCH, fill=None, chunk=256):
    """Masks from the critic alone, to set beside the VAE's difference masks: (preds (B,) fp32, maps (B,64,64) fp32 >= 0,
    per-frame maxima (B,) fp32), on the device.  source "grad": the grey |d logit / d x|; "ig": the same of integrated
    gradients over `steps` passes from the black frame; "occlusion": the drop of the critic's value under a `patch` x `patch`
    cover of colour `fill` (None: the mean colour of the whole set).  Frames go through preprocess_u8 in chunks, as _infer's."""
    if source not in ("grad", "ig", "occlusion"):
        raise ValueError(f"source {source!r}: one of 'grad', 'ig', 'occlusion'")
    frames = _cuda(frames_u8, torch.uint8)
    B, W = frames.shape[0], frames.shape[1]
    if W != 64:
        raise ValueError(f"frames are {W}x{W}, the critic is 64x64 only")
    chunk = min(max(1, int(chunk or 256)), critic.handle.max_batch)       # preprocess_u8 takes at most the handle's max_batch
    if source == "occlusion" and fill is None:
        fill = (frames.sum(dim=(0, 1, 2), dtype=torch.float64) / (B * W * W * 255.0)).tolist()
    out_p = torch.empty(B, device=frames.device)
    maps = torch.empty(B, W, W, device=frames.device)
    maxv = torch.empty(B, device=frames.device)
    x = torch.empty(chunk, 3, W, W, device=frames.device)
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        xs = x[:e - s]
        critic.handle.preprocess_u8(e - s, frames[s:e], xs)
        if source == "occlusion":
            r = critic.occlusion(xs, patch=patch, fill=fill)
        else:
            r = critic.saliency(xs, steps=1 if source == "grad" else steps)
        out_p[s:e] = r["pred"].reshape(-1)
        maps[s:e] = r["map"]
        maxv[s:e] = r["max_values"]
    return out_p, maps, maxv


def object_eval(mask, gt, filt, values=None, gt_objects=None):
    """One mask kind as objects (objects.py): `mask` (B,W,W) through cvae_mask_objects under the ObjectFilter `filt` (sum_value
    over `values`), the ground truth labelled with the same connectivity and no filter (or `gt_objects`, that result, to share
    it), the overlap matrix, the matches at IoU > 0.5.  Returns {"iou": the filtered mask's pixel IoU (mask_counts), "pq", "sq",
    "rq", "precision", "recall", "tp", "fp", "fn", "truncated_frames", and on the device "mask", "labels", "info", "table",
    "gt_info", "gt_table"}."""
    from . import objects as ob
    gt_d = _cuda(gt, torch.uint8)
    if gt_objects is None:
        gt_objects = ob.mask_objects(gt_d, ob.ObjectFilter(connectivity=filt.connectivity, max_objects=filt.max_objects), labels=True)
    o = ob.mask_objects(mask, filt, values=values, labels=True)
    inter = ob.object_overlap(o["labels"], gt_objects["labels"], filt.max_objects)
    c = mask_counts(o["mask"], gt_d).sum(0)
    ta, ia, tb, ib, it, c = ob._host(o["table"], o["info"], gt_objects["table"], gt_objects["info"], inter, c)     # the one read
    r = ob.panoptic(ob.match(ta, ia[:, ob.INFO_KEPT], tb, ib[:, ob.INFO_KEPT], it))
    r["iou"] = iou_from_counts(*c.tolist())
    r.update(mask=o["mask"], labels=o["labels"], info=o["info"], table=o["table"], gt_info=gt_objects["info"],
             gt_table=gt_objects["table"])
    return r


def _objects_entry(thr, crf, gt_d, u8, filt):
    from . import objects as ob
    gto = ob.mask_objects(gt_d, ob.ObjectFilter(connectivity=filt.connectivity, max_objects=filt.max_objects), labels=True)
    return {"thr": object_eval(thr, gt_d, filt, u8, gto), "crf": object_eval(crf, gt_d, filt, u8, gto)}


def eval_maps(frames_u8, maps, max_values, preds, gt, t=THRESHOLD, crf_params=CRF_REF, p_floor=P_FLOOR, objects=None):
    """The tail of eval_frames for any non-negative per-pixel map (B,W,W) with its per-frame maxima: normalisation by the
    set-wide mean of the maxima, threshold, histograms, thr_iou, CRF, crf_iou, bins.  Returns eval_frames' dict (its "diff"
    is `maps`), and under "device" the tensors left on the device (frames, gt, preds, diff_u8, thr_masks, crf_masks; the
    masks as uint8 0/1).  objects: an objects.ObjectFilter adds one key, "objects": {"thr", "crf"}, each object_eval's dict of
    the thresholded and of the CRF mask (sum_value over diff_u8); None returns and launches exactly what it did without."""
    frames = _cuda(frames_u8, torch.uint8)
    diff = _cuda(maps, torch.float32)
    maxv = _cuda(max_values, torch.float32).reshape(-1)
    p = _cuda(preds, torch.float32).reshape(-1)
    gt_d = _cuda(_np(gt).astype(np.uint8), torch.uint8)
    hist = torch.zeros(2, 256, dtype=torch.int64, device=frames.device)
    u8, m, c, mean_max = _normalize(diff, maxv.cpu(), t, gt=gt_d, mask=True, counts=True, hist=hist)
    thr_iou = iou_from_counts(*c.sum(0).tolist())
    crf, crf_iou = _crf_counts(frames, m, gt_d, crf_params, p_floor)
    thr_np = _np(m).astype(bool)
    preds_np = _np(p)
    r = {"preds": preds_np, "diff": _np(diff), "max_values": _np(maxv), "diff_u8": _np(u8), "thr_masks": thr_np, "crf_masks": _np(crf),
         "thr_iou": thr_iou, "crf_iou": crf_iou, "bins": bin_info(preds_np, gt, thr_np), "mean_max": mean_max, "hist": _np(hist),
         "device": {"frames": frames, "gt": gt_d, "preds": p, "diff_u8": u8, "thr_masks": m, "crf_masks": crf.to(torch.uint8)}}
    if objects is not None:
        r["objects"] = _objects_entry(m, r["device"]["crf_masks"], gt_d, u8, objects)
    return r


def sweep_maps(frames_u8, maps, max_values, gt, thresholds=SWEEP, crf_params=CRF_REF, p_floor=P_FLOOR):
    """The tail of threshold_sweep for any non-negative map: normalised once (thr_iou at every threshold from its
    histograms), the CRF once per threshold.  Returns [(t, thr_iou, crf_iou), ...]."""
    frames = _cuda(frames_u8, torch.uint8)
    diff = _cuda(maps, torch.float32)
    gt_d = _cuda(_np(gt).astype(np.uint8), torch.uint8)
    hist = torch.zeros(2, 256, dtype=torch.int64, device=frames.device)
    maxv = _cuda(max_values, torch.float32).reshape(-1).cpu()
    _normalize(diff, maxv, 0, gt=gt_d, hist=hist)
    hist = _np(hist)
    out = []
    for t in thresholds:
        _, m, _, _ = _normalize(diff, maxv, t, mask=True)
        _, crf_iou = _crf_counts(frames, m, gt_d, crf_params, p_floor)
        out.append((t, iou_from_hist(hist, t), crf_iou))
    return out


def eval_frames(frames_u8, vae, gt, critic=None, preds=None, t=THRESHOLD, crf_params=CRF_REF, chunk=None,
                p_floor=P_FLOOR, keep_device=False, objects=None):
    """eval_textured_frames (vae_utility.py:162-212) without the PIL frames.  frames_u8 (B,W,W,3) uint8, gt (B,W,W)
    bool; either a critic (64x64 only, as the reference's) or explicit preds (B,).  The VAE runs in eval mode in
    chunks of at most vae.max_batch; normalisation, threshold, CRF and IoU run over the whole set at once (eval_maps).
    Returns a dict: preds, diff (fp32), max_values, diff_u8, thr_masks, crf_masks (host arrays), thr_iou, crf_iou,
    bins, mean_max, hist (the (2,256) histograms of diff_u8).  keep_device=True adds "device": what render.video_frames
    composes the pictures from, left on the device (frames, gt, preds, recon_one, recon_zero, diff_u8, thr_masks, crf_masks;
    the masks as uint8 0/1).  objects: an objects.ObjectFilter adds the key "objects", as eval_maps does."""
    p, diff, maxv, *recons = _infer(frames_u8, vae, critic, preds, chunk, keep_recons=keep_device)
    r = eval_maps(frames_u8, diff, maxv, p, gt, t, crf_params, p_floor, objects=objects)
    dev = r.pop("device")
    if keep_device:
        r["device"] = dict(dev, recon_one=recons[0], recon_zero=recons[1])
    return r


def threshold_sweep(frames_u8, vae, gt, critic=None, preds=None, thresholds=SWEEP, crf_params=CRF_REF, chunk=None,
                    p_floor=P_FLOOR):
    """The -thresh loop (vae.py:119-124): the VAE and critic run once, the masks are normalised once (thr_iou at every
    threshold from its histograms), the CRF once per threshold (sweep_maps).  Returns [(t, thr_iou, crf_iou), ...]."""
    p, diff, maxv = _infer(frames_u8, vae, critic, preds, chunk)
    return sweep_maps(frames_u8, diff, maxv, gt, thresholds, crf_params, p_floor)


def load_episode(x_npy, y_npy):
    """load_textured_minerl (vae_utility.py:70-82): frames X[100:5000:2] (N,64,64,3) uint8 and the ground truth
    np.all(Y, -1)[100:5000:2] (N,64,64) bool.  Paths or arrays.  (The reference's final squeeze() would also drop
    the frame axis of a one-frame slice; here the frame axis always stays.)"""
    X = np.load(x_npy) if isinstance(x_npy, (str, os.PathLike)) else np.asarray(x_npy)
    Y = np.load(y_npy) if isinstance(y_npy, (str, os.PathLike)) else np.asarray(y_npy)
    return X[100:5000:2], np.all(Y, axis=-1)[100:5000:2]


# ---- CLI (vae.py -video [-thresh], vae.py:108-127) ----
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m critic_vae_amd.segment",
                                 description="critic-guided segmentation masks of an episode: thr_iou and crf_iou")
    ap.add_argument("-video", action="store_true", help="evaluate the episode (the only mode)")
    ap.add_argument("-thresh", action="store_true", help="sweep thresholds 0, 10, ..., 120")
    ap.add_argument("--frames", default="minerl-episode/X.npy", help="episode frames (N,64,64,3) uint8")
    ap.add_argument("--gt", default="minerl-episode/Y.npy", help="episode ground truth (N,64,64,C)")
    ap.add_argument("--networks", default="saved-networks", help=f"directory with {ENCODER_FILE} and {DECODER_FILE}")
    ap.add_argument("--critic", default=None, help=f"critic checkpoint (default: NETWORKS/{CRITIC_FILE})")
    ap.add_argument("--chunk", type=int, default=256, help="frames per VAE launch")
    ap.add_argument("--second", action="store_true", help="evaluate the second VAE: NETWORKS/vae2_encoder.pt and "
                    "vae2_decoder.pt (written by train.py -second).  The reference's -evalsecond is the folder evaluation "
                    "of that VAE: python -m critic_vae_amd.render --second")
    ap.add_argument("--out", default=None, help="write the 7-panel pictures of get_final_frame to DIR (image-000.png, ...; "
                    "frames.npy without PIL)")
    ap.add_argument("--gif", action="store_true", help=f"with --out: also DIR/video-threshold={THRESHOLD}.gif (needs PIL)")
    ap.add_argument("--no-text", dest="text", action="store_false", help="with --out: bare panels, no titles, IoUs or critic value")
    ap.add_argument("--mask-source", choices=tuple(MASK_SOURCES), default="vae", help="where the masks come from: the VAE's "
                    "difference masks (default), or the critic alone: the gradient of its logit with respect to the pixels, "
                    "integrated gradients from the black frame, or occlusion sensitivity.  A critic source needs no --networks")
    ap.add_argument("--ig-steps", type=int, default=IG_STEPS, help="critic-ig: passes from the black frame to the frame (2..256)")
    ap.add_argument("--occlusion-patch", type=int, default=OCCLUSION_PATCH, choices=(4, 8, 16),
                    help="critic-occlusion: side of the non-overlapping cover, filled with the episode's mean colour")
    ap.add_argument("--thr", type=int, default=THRESHOLD, help="threshold of the single evaluation (0..255)")
    ap.add_argument("--crf", default=None, metavar="W1,ALPHA,BETA,W2,GAMMA,IT", help="CRF parameters of the single evaluation "
                    "and of -thresh (default: the reference's " + ",".join(str(v) for v in CRF_REF) + ")")
    ap.add_argument("--p-floor", type=float, default=P_FLOOR, help="unary floor of the single evaluation and of -thresh")
    ap.add_argument("-search", action="store_true", help="grid search over thresholds and CRF parameters (the --grid-* lists), "
                    "best crf_iou first")
    ap.add_argument("--top", type=int, default=10, help="-search: rows to print")
    ap.add_argument("--skip", type=int, default=1, help="-search: evaluate frames [::N], as the reference's crf(skip=N)")
    ap.add_argument("--grid-thr", default=",".join(str(t) for t in SWEEP), help="-search: thresholds, a comma list")
    for name, ref in zip(("w1", "alpha", "beta", "w2", "gamma", "it"), CRF_REF):
        ap.add_argument(f"--grid-{name}", default=str(ref), help=f"-search: {name} values, a comma list")
    ap.add_argument("--grid-p-floor", default=str(P_FLOOR), help="-search: unary floors, a comma list")
    ap.add_argument("--objects", action="store_true", help="also report both masks as objects: connected components after an "
                    "optional hole fill and area filter, matched with the ground truth's at IoU > 0.5 (precision, recall, PQ = SQ * RQ)")
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8), help="--objects: connectivity of the set pixels")
    ap.add_argument("--fill-holes", action="store_true", help="--objects: set every clear region that does not reach the frame border")
    ap.add_argument("--min-area", type=int, default=1, help="--objects: drop components of fewer pixels")
    ap.add_argument("--keep-largest", type=int, default=0, help="--objects: keep the K largest components per frame (0: all)")
    ap.add_argument("--max-objects", type=int, default=32, help="--objects: table rows per frame (1..64)")
    ap.add_argument("--objects-out", default=None, metavar="FILE.npz", help="--objects: write info, tables and centroids of both "
                    "masks and of the ground truth")
    args = ap.parse_args(argv)

    def numbers(text, kind, flag):
        try:
            vals = tuple(kind(v) for v in text.split(","))
        except ValueError:
            ap.error(f"{flag}: {text!r} is not a comma list of {kind.__name__} values")
        return vals
    if args.crf is None:
        args.crf = CRF_REF
    else:
        v = numbers(args.crf, float, "--crf")
        if len(v) != 6 or v[5] != int(v[5]):
            ap.error("--crf takes W1,ALPHA,BETA,W2,GAMMA,IT with an integer IT")
        args.crf = v[:5] + (int(v[5]),)
    if not 0 <= args.thr <= 255:
        ap.error("--thr must be in 0..255")
    args.grid = {"thresholds": numbers(args.grid_thr, int, "--grid-thr"), "it": numbers(args.grid_it, int, "--grid-it"),
                 "p_floor": numbers(args.grid_p_floor, float, "--grid-p-floor")}
    for name in ("w1", "alpha", "beta", "w2", "gamma"):
        args.grid[name] = numbers(getattr(args, f"grid_{name}"), float, f"--grid-{name}")
    if args.search and (args.out is not None or args.thresh):
        ap.error("-search prints the table of a grid: not with --out or -thresh")
    if args.search and (args.thr != THRESHOLD or args.crf != CRF_REF or args.p_floor != P_FLOOR):
        ap.error("-search takes its values from the --grid-* lists: not with --thr, --crf or --p-floor")
    if args.thresh and args.thr != THRESHOLD:
        ap.error("-thresh sweeps the thresholds: not with --thr")
    if args.skip < 1 or args.top < 1:
        ap.error("--skip and --top must be >= 1")
    if not args.video:
        ap.error("-video is required (-dataset and -second are modes of critic_vae_amd.train; -inject and the folder "
                 "evaluation of -evalsecond are python -m critic_vae_amd.render)")
    if args.out is None and (args.gif or not args.text):
        ap.error("--gif and --no-text need --out")
    if args.out is not None and args.thresh:
        ap.error("--out writes the pictures of one evaluation: not with -thresh")
    if args.chunk < 1:
        ap.error("--chunk must be >= 1")
    if args.mask_source != "vae" and args.out is not None:
        ap.error("--out composes the 7-panel pictures, which have reconstruction panels: not with a critic --mask-source")
    if args.mask_source != "vae" and args.second:
        ap.error("--second selects a VAE: not with a critic --mask-source")
    if not 2 <= args.ig_steps <= 256:
        ap.error("--ig-steps must be in 2..256")
    if args.critic is None:
        args.critic = os.path.join(args.networks, CRITIC_FILE)
    args.object_filter = None
    if args.objects:
        if args.search or args.thresh:
            ap.error("--objects reports the single evaluation: not with -search or -thresh")
        from .objects import ObjectFilter
        try:
            args.object_filter = ObjectFilter(args.connectivity, args.fill_holes, args.min_area, args.keep_largest, args.max_objects)
        except ValueError as e:
            ap.error(f"--objects: {e}")
    elif (args.objects_out is not None or args.fill_holes or args.connectivity != 8 or args.min_area != 1 or args.keep_largest != 0
          or args.max_objects != 32):
        ap.error("--connectivity, --fill-holes, --min-area, --keep-largest, --max-objects and --objects-out need --objects")
    return args


def print_objects(entry):
    """One line per mask kind of an "objects" entry."""
    for kind in ("thr", "crf"):
        o = entry[kind]
        print(f"objects {kind}: iou={o['iou']}, pq={o['pq']:.3f}, sq={o['sq']:.3f}, rq={o['rq']:.3f}, precision={o['precision']:.3f}, "
              f"recall={o['recall']:.3f}, tp={o['tp']}, fp={o['fp']}, fn={o['fn']}, truncated_frames={o['truncated_frames']}")


def save_objects(path, entry):
    """FILE.npz of --objects-out: per mask kind (thr, crf) and for the ground truth (gt) the info, the table and the centroids."""
    from .objects import centroids
    out = {}
    for kind in ("thr", "crf"):
        o = entry[kind]
        out[f"{kind}_info"], out[f"{kind}_table"] = _np(o["info"]), _np(o["table"])
        out[f"{kind}_centroids"] = centroids(out[f"{kind}_table"])
    out["gt_info"], out["gt_table"] = _np(entry["thr"]["gt_info"]), _np(entry["thr"]["gt_table"])
    out["gt_centroids"] = centroids(out["gt_table"])
    with open(path, "wb") as f:
        np.savez(f, **out)


def _report_objects(args, r):
    if args.object_filter is not None:
        print_objects(r["objects"])
        if args.objects_out is not None:
            save_objects(args.objects_out, r["objects"])


def print_search(rows, top):
    """The table of -search: the best `top` rows of crf_search."""
    print(f"grid search: {len(rows)} candidates, best crf_iou first")
    for r in rows[:top]:
        w1, alpha, beta, w2, gamma, it = r["params"]
        print(f"thr={r['thr']}, w1={w1:g}, alpha={alpha:g}, beta={beta:g}, w2={w2:g}, gamma={gamma:g}, it={it}, "
              f"p_floor={r['p_floor']:g}, thr_iou={r['thr_iou']}, crf_iou={r['crf_iou']}")


def main(argv=None):
    args = parse_args(argv)
    from .critic import Critic
    frames, gt = load_episode(args.frames, args.gt)
    critic = Critic(64, handle=Handle(64, args.chunk)).to("cuda")
    critic.load_state_dict(torch.load(args.critic, map_location="cpu"))
    if args.mask_source != "vae":
        preds, maps, maxv = critic_maps(frames, critic, MASK_SOURCES[args.mask_source], steps=args.ig_steps, patch=args.occlusion_patch,
                                        chunk=args.chunk)
        if args.search:
            print_search(crf_search(frames, maps, maxv, gt, skip=args.skip, **args.grid), args.top)
        elif args.thresh:
            print("testing thresholds (thr):")
            for t, thr_iou, crf_iou in sweep_maps(frames, maps, maxv, gt, crf_params=args.crf, p_floor=args.p_floor):
                print(f"thr={t}, thr_iou={thr_iou}, crf_iou={crf_iou}")
        else:
            r = eval_maps(frames, maps, maxv, preds, gt, args.thr, args.crf, args.p_floor, objects=args.object_filter)
            print(f"thr_iou={r['thr_iou']}")
            print(f"crf_iou={r['crf_iou']}")
            _report_objects(args, r)
        return 0
    from .nets import VariationalAutoencoder
    from .train import load_networks
    vae = VariationalAutoencoder(max_batch=args.chunk).to("cuda")
    load_networks(vae, args.networks, second=args.second)
    if args.search:
        _, diff, maxv = _infer(frames, vae, critic, None, args.chunk)
        print_search(crf_search(frames, diff, maxv, gt, skip=args.skip, **args.grid), args.top)
    elif args.thresh:
        print("testing thresholds (thr):")
        for t, thr_iou, crf_iou in threshold_sweep(frames, vae, gt, critic=critic, crf_params=args.crf, chunk=args.chunk,
                                                   p_floor=args.p_floor):
            print(f"thr={t}, thr_iou={thr_iou}, crf_iou={crf_iou}")
    else:
        r = eval_frames(frames, vae, gt, critic=critic, t=args.thr, crf_params=args.crf, chunk=args.chunk, p_floor=args.p_floor,
                        keep_device=args.out is not None, objects=args.object_filter)
        print(f"thr_iou={r['thr_iou']}")
        print(f"crf_iou={r['crf_iou']}")
        _report_objects(args, r)
        if args.out is not None:
            from . import render
            pictures = render.video_frames(r, text=args.text, threshold=args.thr).cpu().numpy()
            render.save_pngs(args.out, pictures)
            if args.gif:
                render.save_gif(os.path.join(args.out, f"video-threshold={args.thr}.gif"), pictures)
    return 0


if __name__ == "__main__":
    sys.exit(main())
