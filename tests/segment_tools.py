"""Host-side tools of the segmentation tests (numpy / torch on the CPU, no GPU): the CRF case table and its inputs,
deliberately wrong variants of the float64 reference (crf_ref_knockout), a float32 restatement of the kernel's
arithmetic that qualifies cases on the CPU (crf_f32), and exact references of the pixel and integer kernels.

tests/test_host_segment_tools.py checks, without a GPU, that every case of CRF_CASES is non-degenerate, that float32
arithmetic resolves it a decade below the bar, and that each knockout moves the reference a hundred bars: the GPU
comparison of tests/test_gpu_segment_ops.py then separates a right kernel from one that drops far taps, far rows, an
LDS chunk or the frame offset.
"""
import os
from contextlib import contextmanager

import numpy as np
import torch

import crf_ref as _crf_ref_module
from crf_ref import crf_ref

BAR = 1e-4                       # the bar of test_gpu_segment._check_against_ref: |Q(1) - reference| and the label margin
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (w1, alpha, beta, w2, gamma, it).  it1 / it2 are wideB with fewer trips.  narrow: its filters reach no neighbour, so each
# pixel feeds (w1 + w2) * (2Q - 1) back to itself; at weights 4 / 3 that saturates the mean field (3.7 % of pixels stay
# mid-range), at 0.6 / 0.4 it does not.  tiny_* / small_alpha / huge: the ends of the documented parameter ranges.
WIDE_B = (6, 48, 40, 4, 24, 3)
CRF_CASES = {
    "wideA": (3, 200, 200, 2, 100, 2),
    "wideB": WIDE_B,
    "wideC": (4, 64, 1e4, 3, 32, 3),
    "g_only": (0, 12, 3.1, 6, 24, 3),
    "b_only": (6, 48, 40, 0, 1.8, 3),
    "none": (0, 12, 3.1, 0, 1.8, 3),
    "it1": WIDE_B[:5] + (1,),
    "it2": WIDE_B[:5] + (2,),
    "narrow": (0.6, 0.3, 0.5, 0.4, 0.3, 3),
    "tiny_gamma": (6, 48, 40, 4, 1e-20, 3),
    "tiny_alpha": (6, 1e-20, 40, 4, 24, 3),
    "tiny_beta": (6, 48, 1e-20, 4, 24, 3),
    "small_alpha": (6, 1e-10, 40, 4, 24, 3),      # its prescale is finite in fp32, but products with it round
    "huge": (3, 1e20, 3e38, 2, 1e20, 2),
}
UNCONDITIONED = ("none", "tiny_gamma", "tiny_alpha", "tiny_beta", "small_alpha", "huge")    # conditions a-c do not apply
KNOCKOUTS = {                                                                # which knockout must bite which case
    "gauss_far": ("wideA", "wideB", "wideC", "g_only"),
    "bilateral_far_rows": ("wideA", "wideB", "wideC", "b_only"),
    "last_chunk": ("wideA", "wideB", "wideC", "b_only"),
    "frame_offset": tuple(c for c in CRF_CASES if c not in UNCONDITIONED),
}
WIDE = ("wideA", "wideB", "wideC")
CASE_P_FLOOR = 1e-5


# ---- inputs ----
def _structured_frames(n, w, seed):
    """Blocky colour regions with noise and their masks (a disk, stripes, speckle, a soft probability)."""
    rng = np.random.default_rng(seed)
    frames = np.empty((n, w, w, 3), np.uint8)
    masks = np.empty((n, w, w), np.float32)
    yy, xx = np.mgrid[0:w, 0:w]
    for i in range(n):
        cells = rng.integers(0, 256, size=(4, 4, 3))
        base = np.repeat(np.repeat(cells, w // 4, 0), w // 4, 1).astype(np.int32)
        frames[i] = np.clip(base + rng.integers(-6, 7, size=(w, w, 3)), 0, 255).astype(np.uint8)
        cx, cy, r = rng.integers(w // 4, 3 * w // 4, size=2).tolist() + [rng.integers(w // 8, w // 3)]
        m = ((xx - cx) ** 2 + (yy - cy) ** 2 < r * r).astype(np.float32)
        kind = i % 4
        if kind == 1:
            m = ((xx // 5 + i) % 3 == 0).astype(np.float32)
        elif kind == 2:
            m = np.where(rng.random((w, w)) < 0.1, 1 - m, m)
        elif kind == 3:
            m = np.clip(0.5 + 0.4 * np.sin(xx / 7.0 + i) * np.cos(yy / 5.0), 0, 1).astype(np.float32)
        masks[i] = m
    return frames, masks


def soft_prob(w, seed):
    """A smooth probability map (w,w) float32 that spans exactly [0.05, 0.95] with its median at 0.5: a few waves of
    1.5 to 4 periods per frame, short against the wide filters of CRF_CASES, so that the far-reaching messages nearly
    cancel and the mean field stays mid-range instead of collapsing to one label."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:w, 0:w] / float(w)
    s = np.zeros((w, w))
    for _ in range(4):
        f, th = rng.uniform(1.5, 4.0), rng.uniform(0, np.pi)
        s += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi * f * (np.cos(th) * xx + np.sin(th) * yy) + rng.uniform(0, 2 * np.pi))
    s -= np.median(s)
    s = np.where(s > 0, s / s.max(), s / -s.min())
    return (0.5 + 0.45 * s).astype(np.float32)


def case_frames(w=64):
    """The call every case runs on: (frames (3,w,w,3) uint8, prob1 (3,w,w) float32).  Frame 0 is a real frame (64
    wide; tiled 2 x 2 at 128), frame 1 a structured one, both under soft probabilities; frame 2 is all white with
    prob1 = 1 everywhere, so that a wrong frame offset shows in it and in its neighbours."""
    real = np.load(os.path.join(GOLDEN, "step_real_b68.npz"))["u8"][0]
    assert real.shape == (64, 64, 3) and w % 64 == 0
    real = np.tile(real, (w // 64, w // 64, 1))
    frames = np.stack([real, _structured_frames(1, w, 21)[0][0], np.full((w, w, 3), 255, np.uint8)])
    prob1 = np.stack([soft_prob(w, 10), soft_prob(w, 2), np.ones((w, w), np.float32)])
    return frames, prob1


# ---- the bar ----
def crf_bar(labels, q1, lr, qr):
    """(max |Q(1) - reference|, number of labels that differ where the reference is not within BAR of 0.5): a result
    passes when the first is < BAR and the second is 0 (test_gpu_segment._check_against_ref)."""
    err = float(np.abs(np.asarray(q1, np.float64) - qr).max())
    bad = (np.asarray(labels).astype(bool) != lr) & (np.abs(qr - 0.5) >= BAR)
    return err, int(bad.sum())


# ---- the reference with one deliberate error ----
@contextmanager
def _patched_kernel_rows(kind, W):
    """crf_ref itself, with the rows of one of its kernels masked: the error is the only difference."""
    orig = _crf_ref_module._kernel_rows
    N = W * W

    def rows(x, y, rgb, s, e, inv2, inv2c=None):
        k = orig(x, y, rgb, s, e, inv2, inv2c)
        dx, dy = (x[s:e, None] - x[None]).abs(), (y[s:e, None] - y[None]).abs()
        if kind == "gauss_far" and inv2c is None:
            k = k * ((dx <= 12) & (dy <= 12))
        elif kind == "bilateral_far_rows" and inv2c is not None:
            k = k * (dy <= 40)
        elif kind == "last_chunk" and inv2c is not None:
            k = k.clone()
            k[:, N - 1024:] = 0
        return k

    _crf_ref_module._kernel_rows = rows
    try:
        yield
    finally:
        _crf_ref_module._kernel_rows = orig


def _crf_frame_offset(imgs, prob1, params, p_floor):
    """Mean field in which frame b's messages are filtered from frame (b - 1) mod B's Q (its own kernels, normalisers
    and unary): what a kernel reading its neighbours at the wrong frame offset computes.  With B = 1 it is crf_ref."""
    w1, alpha, beta, w2, gamma, it = params
    B, W = imgs.shape[0], imgs.shape[1]
    N = W * W
    idx = torch.arange(N, dtype=torch.int64)
    x, y = (idx % W).to(torch.float64), (idx // W).to(torch.float64)
    K, n, u, Q = [], [], [], []
    for b in range(B):
        rgb = torch.from_numpy(imgs[b].reshape(N, 3).astype(np.float64))
        kg = _crf_ref_module._kernel_rows(x, y, rgb, 0, N, 0.5 / gamma ** 2)
        kb = _crf_ref_module._kernel_rows(x, y, rgb, 0, N, 0.5 / alpha ** 2, 0.5 / beta ** 2)
        K.append((kg, kb))
        n.append((kg.sum(1, keepdim=True) ** -0.5, kb.sum(1, keepdim=True) ** -0.5))
        p1 = torch.from_numpy(np.asarray(prob1[b], dtype=np.float64).reshape(N))
        u.append(-torch.log(torch.clamp(torch.stack([1.0 - p1, p1], dim=1), min=p_floor)))
        Q.append(torch.softmax(-u[b], dim=1))
    for _ in range(int(it)):
        new = []
        for b in range(B):
            (kg, kb), (ng, nb), src = K[b], n[b], Q[(b - 1) % B]
            new.append(torch.softmax(-u[b] + w2 * ng * (kg @ (ng * src)) + w1 * nb * (kb @ (nb * src)), dim=1))
        Q = new
    q1 = np.stack([q[:, 1].numpy().reshape(W, W) for q in Q])
    labels = np.stack([(q[:, 1] > q[:, 0]).numpy().reshape(W, W) for q in Q])
    return labels, q1


def crf_ref_knockout(img, prob1, params, p_floor, kind):
    """crf_ref with one deliberate error -> (labels, Q(1)) as crf_ref returns them.
        "gauss_far"            Gaussian taps with |dx| or |dy| > 12 zeroed
        "bilateral_far_rows"   bilateral pairs with |dy| > 40 zeroed
        "last_chunk"           neighbours with index >= N - 1024 left out of the bilateral sums
        "frame_offset"         img (B,W,W,3), prob1 (B,W,W): the messages of frame b come from frame b - 1's Q
    The first three take one frame (W,W,3) and drop the pairs from the normaliser as well as from the messages, as a
    kernel that skips them would."""
    img = np.asarray(img)
    if kind == "frame_offset":
        assert img.ndim == 4
        return _crf_frame_offset(img, np.asarray(prob1), params, p_floor)
    assert kind in ("gauss_far", "bilateral_far_rows", "last_chunk") and img.ndim == 3
    with _patched_kernel_rows(kind, img.shape[0]):
        return crf_ref(img, prob1, params, p_floor)


# ---- float32 restatement of the kernel's arithmetic (qualifies cases on the CPU; never the kernel's expected value) ----
def _chunk_sums(M):
    """float32 sum along axis 1 as the bilateral kernel forms it: each chunk of 1024 neighbours summed in order, the
    chunk partials then added in order."""
    f = np.float32
    acc = np.zeros(M.shape[0], f)
    for c in range(0, M.shape[1], 1024):
        acc = (acc + np.cumsum(M[:, c:c + 1024], axis=1, dtype=f)[:, -1]).astype(f)
    return acc


def crf_f32(img, prob1, params, p_floor):
    """(labels, Q(1) float32) of one frame in float32 numpy, in the kernel's form: exp2 with the prescales sa, sb and
    cg, messages from v = 2Q(1) - 1, the bilateral sum in sequential 1024-neighbour chunks, the Gaussian as a row pass
    and then a column pass, Q(1) = 1 / (1 + exp(-d))."""
    f = np.float32
    w1, alpha, beta, w2, gamma, it = params
    img = np.asarray(img)
    W = img.shape[0]
    N = W * W
    log2e = f(1.4426950408889634)
    sa = np.sqrt(log2e / (f(2) * f(alpha) * f(alpha))).astype(f)
    sb = np.sqrt(log2e / (f(2) * f(beta) * f(beta))).astype(f)
    cg = (log2e / (f(2) * f(gamma) * f(gamma))).astype(f)
    idx = np.arange(N)
    x, y = idx % W, idx // W
    xs, ys = (x.astype(f) * sa).astype(f), (y.astype(f) * sa).astype(f)
    c = (img.reshape(N, 3).astype(f) * sb).astype(f)
    a = ((ys[:, None] - ys[None]) ** 2).astype(f)
    a = (a + (xs[:, None] - xs[None]) ** 2).astype(f)
    for ch in range(3):
        a = (a + (c[:, None, ch] - c[None, :, ch]) ** 2).astype(f)
    kb = np.exp2(-a).astype(f)
    del a
    d = np.arange(W)
    tap = np.exp2(-(d * d).astype(f) * cg).astype(f)
    G = tap[np.abs(d[:, None] - d[None])]
    gx = np.cumsum(G, axis=1, dtype=f)[:, -1]
    ng = (f(1) / np.sqrt(gx[x] * gx[y])).astype(f)
    nb = (f(1) / np.sqrt(_chunk_sums(kb))).astype(f)
    p1 = np.asarray(prob1, f).reshape(N)
    d0 = (np.log(np.maximum(p1, f(p_floor))) - np.log(np.maximum(f(1) - p1, f(p_floor)))).astype(f)
    dd = d0.copy()
    for _ in range(int(it)):
        q = (f(1) / (f(1) + np.exp(-dd))).astype(f)
        v = (f(2) * q - f(1)).astype(f)
        tg = ((ng * v).reshape(W, W) @ G.T).astype(f)               # row pass
        sg = (G @ tg).astype(f).reshape(N)                          # column pass
        acc = _chunk_sums(kb * (nb * v)[None, :])
        dd = (d0 + f(w2) * (ng * sg) + f(w1) * (nb * acc)).astype(f)
    q = (f(1) / (f(1) + np.exp(-dd))).astype(f)
    return (dd > 0).reshape(W, W), q.reshape(W, W)


# ---- the pixel and integer kernels ----
def grey_ref(a, b):
    """cvae_diff_grey in float64: a, b (B,3,W,W) -> 0.2989|dR| + 0.5870|dG| + 0.1140|dB| of b - a, (B,W,W)."""
    d = np.abs(np.asarray(b, np.float64) - np.asarray(a, np.float64))
    return 0.2989 * d[:, 0] + 0.5870 * d[:, 1] + 0.1140 * d[:, 2]


def grey_bound(a, b):
    """5 * 2^-24 * (0.2989|dR| + 0.5870|dG| + 0.1140|dB|): every term passes at most five roundings of relative size
    2^-24 on its way into the sum: its subtraction, its float32 constant, its product and the two additions."""
    return 5 * 2.0 ** -24 * grey_ref(a, b)


def diff_u8_ref(diff32, mean_max, factor):
    """trunc((min(d, mean_max) * factor) * 255) as uint8, in numpy float64 and in the order of prepare_diff +
    astype(np.uint8): the operation order of test_gpu_segment._numpy_u8."""
    d = np.asarray(diff32).astype(np.float64)
    d[d > mean_max] = mean_max
    d = d * factor
    return (d * 255).astype(np.uint8)


def _u8_value(d32, mean_max, factor):
    return (min(np.float64(d32), np.float64(mean_max)) * factor) * 255


def boundary_diffs(mean_max, factor):
    """float32 inputs on the truncation boundaries of diff_u8_ref -> (values float32 (n,), names list of n str).
    For k in {1, 50, 51, 254, 255}: "k" is the smallest float32 d whose float64 value (min(d, mean_max) * factor) * 255
    reaches k (it is exactly k wherever a float32 d gives exactly k, e.g. mean_max = 255, factor = 1 / 255), and "k-"
    its float32 neighbour below, whose value lies under k.  A k that the clipped value (mean_max * factor) * 255 does
    not reach gives the largest float32 <= mean_max and its neighbour below instead.  Then d == mean_max, nextafter(mean_max, inf),
    +inf, 0, -0.0 and the smallest subnormal."""
    f = np.float32
    mean_max, factor = float(mean_max), float(factor)
    top = f(mean_max) if f(mean_max) <= mean_max else np.nextafter(f(mean_max), f(-np.inf))
    vals, names = [], []
    for k in (1, 50, 51, 254, 255):
        d = top
        if _u8_value(np.inf, mean_max, factor) >= k:
            d = f(k / (factor * 255))
            while d > 0 and _u8_value(d, mean_max, factor) >= k:
                d = np.nextafter(d, f(-np.inf))
            while _u8_value(d, mean_max, factor) < k:
                d = np.nextafter(d, f(np.inf))
        vals += [d, np.nextafter(d, f(-np.inf)) if d > 0 else f(0)]
        names += [str(k), f"{k}-"]
    vals += [f(mean_max), np.nextafter(f(mean_max), f(np.inf)), f(np.inf), f(0.0), f(-0.0), np.nextafter(f(0), f(1))]
    names += ["mean_max", "mean_max+", "inf", "0", "-0", "subnormal"]
    return np.array(vals, f), names


def counts_ref(mask, gt):
    """per-frame (tp, fn, fp) of get_iou(gt, mask), (B,3) int64; any nonzero byte is set"""
    m, g = np.asarray(mask) != 0, np.asarray(gt) != 0
    ax = tuple(range(1, m.ndim))
    return np.stack([(g & m).sum(ax), (g & ~m).sum(ax), (~g & m).sum(ax)], axis=1).astype(np.int64)
