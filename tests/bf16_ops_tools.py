"""Helpers of test_gpu_bf16_ops.py and test_host_bf16_ops_tools.py: small-integer operands for the bf16-mode conv kernels, their float64
references, the conditions under which the comparison may be EQUALITY, and mirrors of the launch geometry.  Nothing here touches a GPU.

Why integers: every value of {0, +-1, +-2} is a bf16 number, every product of two of them is exact, every fp32 partial sum of such
products below 2^24 is exact in ANY order (MFMA accumulators, split-K slabs, weight-gradient slabs), and an integer of magnitude <= 256
is a bf16 number again.  The float64 convolution of these operands, cast to the storage type, is therefore what a correct kernel must
store bit for bit, whatever its tiling; one dropped tap, pixel, image or slab changes an integer somewhere."""
import math

import torch
import torch.nn.functional as F

from critic_vae_amd import synth

SEED = 11
# (cin, cout, h_out at 64 x 64 frames, up)  -- E1..E4, D0..D4; every spatial size doubles at 128 x 128
LAYERS = [(3, 32, 64, 0), (32, 64, 32, 0), (64, 128, 16, 0), (128, 256, 8, 0),
          (256, 128, 4, 0), (128, 64, 8, 1), (64, 32, 16, 1), (32, 32, 32, 1), (32, 3, 64, 1)]
PASSES = ("fwd", "dgrad", "wgrad")
EXACT_FP32 = float(1 << 24)       # fp32 holds every integer up to here
EXACT_BF16 = 256.0                # bf16 holds every integer up to here
# D0..D3 end in a ReLU, which turns the negative half of a symmetric sum into expected zeros.  Their forward therefore runs twice: with the
# biases of [-2, 2] (the clamp itself: about half the outputs are expected zeros, "not empty" is asserted on the pre-activation), and with
# every bias lifted by this much (2 to 8 standard deviations of the sums: the expected OUTPUT is at least 90 % nonzero and at most 256)
RELU_LIFT = 64


def geom(layer, W):
    """(cin, cout, h_out, up, h_in) of conv layer `layer` at W x W frames."""
    cin, cout, h, up = LAYERS[layer]
    h = h * W // 64
    return cin, cout, h, up, (h // 2 if up else h)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def _u(name, shape):
    return torch.from_numpy(synth.uniform(SEED, f"bf16ops/{name}", shape)).double()


def sparse_act(name, shape, density=0.25, relu=False):
    """Activations: a value of {-2, -1, 1, 2} with probability `density`, else 0; relu clamps at 0 (the inputs of D1..D3 are post-ReLU)."""
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)
    t = torch.where(_u(name + "/on", shape) < density, vals[(_u(name + "/v", shape) * 4).long().clamp_(0, 3)], torch.zeros((), dtype=torch.float64))
    return t.clamp_min(0.0) if relu else t


def sparse_w(name, shape, density=0.25):
    """Weights (OIHW): -1 or +1 with probability `density`, else 0."""
    return torch.where(_u(name + "/on", shape) < density, torch.where(_u(name + "/v", shape) < 0.5, -1.0, 1.0).double(), torch.zeros((), dtype=torch.float64))


def dense_act(name, shape):
    """Both operands of the weight gradients: every element in {-2, -1, 1, 2}."""
    return torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)[(_u(name, shape) * 4).long().clamp_(0, 3)]


def int_bias(name, n, lo=-2, hi=2):
    return (torch.floor(_u(name, (n,)) * (hi - lo + 1)) + lo).clamp_(lo, hi)


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references (NCHW / OIHW on the host)
# ---------------------------------------------------------------------------------------------------------------------------------------
def up2(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def conv_fwd_ref(layer, x, w, b):
    """The layer's forward: Conv2d(5, pad 2) behind a nearest-2x upsample for D1..D3 (layers 5..7), + bias, ReLU for D0..D3."""
    y = F.conv2d(up2(x) if LAYERS[layer][3] else x, w, b, padding=2)
    return torch.relu(y) if 4 <= layer <= 7 else y


def conv_dgrad_ref(layer, dout, w, mask_src=None):
    """Input gradient of the conv; D1..D3: through the upsample (2 x 2 sums) and the ReLU of the producing layer (mask_src > 0)."""
    d = F.conv_transpose2d(dout, w, padding=2)
    if LAYERS[layer][3]:
        d = torch.where(mask_src > 0, F.avg_pool2d(d, 2) * 4.0, torch.zeros((), dtype=d.dtype))
    return d


# taps of the 5 x 5 kernel that reach source pixel offset -1 / 0 / +1 from an output pixel of phase 0 / 1 (conv_up.hip, collapse_w_kernel)
PHASE_TAPS = {0: [[0, 1], [2, 3], [4]], 1: [[0], [1, 2], [3, 4]]}


def collapse_w(w):
    """The four phase-collapsed 3 x 3 kernels of an Upsample(2) -> Conv(5) block, (4, O, I, 3, 3) with phase p = 2 py + px: sums of the 5 x 5
    taps that read the same low-resolution pixel, taken in w's dtype."""
    wc = torch.zeros((4,) + tuple(w.shape[:2]) + (3, 3), dtype=w.dtype)
    for py in (0, 1):
        for px in (0, 1):
            for ta in range(3):
                for tb in range(3):
                    for r in PHASE_TAPS[py][ta]:
                        for s in PHASE_TAPS[px][tb]:
                            wc[2 * py + px, :, :, ta, tb] += w[:, :, r, s]
    return wc


def up_conv_collapsed(x, wc, b):
    """Upsample(2) -> Conv(5) as four 3 x 3 convs at the stored resolution (differentiable)."""
    B, _, hs, _ = x.shape
    out = torch.zeros(B, wc.shape[1], 2 * hs, 2 * hs, dtype=x.dtype)
    for py in (0, 1):
        for px in (0, 1):
            out[:, :, py::2, px::2] = F.conv2d(x, wc[2 * py + px], b, padding=1)
    return out


def conv_wgrad_ref(layer, x, dout, drop_tap=None):
    """dW (OIHW) and db of the conv from its input and output gradient: 25 float64 matrix products over all pixels, a few images at a time."""
    if LAYERS[layer][3]:
        x = up2(x)
    B, cin, h, _ = x.shape
    cout = dout.shape[1]
    dw = torch.zeros(cout, cin, 5, 5, dtype=torch.float64)
    step = max(1, (1 << 22) // (cin * h * h))
    for b0 in range(0, B, step):
        xp = F.pad(x[b0:b0 + step], (2, 2, 2, 2))
        d2 = dout[b0:b0 + step].permute(1, 0, 2, 3).reshape(cout, -1)
        for ky in range(5):
            for kx in range(5):
                if drop_tap == (ky, kx):
                    continue
                dw[:, :, ky, kx] += d2 @ xp[:, :, ky:ky + h, kx:kx + h].permute(0, 2, 3, 1).reshape(-1, cin)
    return dw, dout.sum(dim=(0, 2, 3))


def max_terms(layer, W, B, what):
    """Upper bound of the sum of |terms| behind one output element, from the operands' largest magnitudes (2 for activations and
    gradients, 1 for sparse weights, 2 for a bias): the products are at most that large and there are at most this many of them."""
    cin, cout, h, up, hs = geom(layer, W)
    if what == "fwd":
        return 25 * cin * 2 + 2
    if what == "dgrad":
        return 25 * cout * 2 * (4 if up else 1)
    return B * h * h * 4            # wgrad: dense operands, one term per output pixel; the bias gradient sums B h h terms of at most 2


def assert_exact_conditions(ref, what, bound_terms, stored_bf16):
    """What a case asserts on its float64 reference BEFORE it touches the kernel: integers; within the storage type's exact integers; the
    sum of |terms| of every output below 2^24 (so every fp32 partial sum is exact in any order); and the expected tensor is not empty."""
    assert bool((ref == ref.round()).all()), f"{what}: the expected output is not integer-valued"
    assert bound_terms < EXACT_FP32, f"{what}: {bound_terms} >= 2^24: a partial sum could round"
    top = float(ref.abs().max())
    assert top <= (EXACT_BF16 if stored_bf16 else EXACT_FP32), f"{what}: largest |expected| {top} is not exact in storage"
    nz = float((ref != 0).double().mean())
    assert nz >= 0.9, f"{what}: only {100 * nz:.1f} % of the expected elements are nonzero"
    return top, nz


def case_operands(layer, W, B, what, density=0.25, bias=None, lift=0):
    """Operands and float64 reference of one (layer 1..7, pass) at batch B.  Returns a dict: fwd {x, w, b, ref}; dgrad {dout, w, mask, ref};
    wgrad {x, dout, ref_w, ref_b}.  A quarter of the elements of a sparse operand is lit unless stated."""
    cin, cout, h, up, hs = geom(layer, W)
    tag = f"L{layer}/w{W}"
    if what == "fwd":
        x = sparse_act(f"{tag}/x", (B, cin, hs, hs), density, relu=bool(up))
        w = sparse_w(f"{tag}/w", (cout, cin, 5, 5), density)
        b = (int_bias(f"{tag}/b", cout) if bias is None else torch.full((cout,), float(bias), dtype=torch.float64)) + float(lift)
        # pre: the pre-activation (see RELU_LIFT: with lift = 0 the "not empty" condition of D0..D3 is asserted on it)
        pre = F.conv2d(up2(x) if up else x, w, b, padding=2)
        return dict(x=x, w=w, b=b, pre=pre, ref=torch.relu(pre) if 4 <= layer <= 7 else pre)
    if what == "dgrad":
        dout = sparse_act(f"{tag}/do", (B, cout, h, h), density)
        w = sparse_w(f"{tag}/w", (cout, cin, 5, 5), density)
        # D1..D3: the ReLU mask source, nine tenths of it lit (a masked element is an expected zero)
        mask = torch.where(_u(f"{tag}/mask", (B, cin, hs, hs)) < 0.95, 1.0, 0.0).double() if up else None
        return dict(dout=dout, w=w, mask=mask, ref=conv_dgrad_ref(layer, dout, w, mask))
    x = dense_act(f"{tag}/wx", (B, cin, hs, hs))
    if up:
        x = x.abs()                  # post-ReLU
    dout = dense_act(f"{tag}/wdo", (B, cout, h, h))
    ref_w, ref_b = conv_wgrad_ref(layer, x, dout)
    return dict(x=x, dout=dout, ref_w=ref_w, ref_b=ref_b)


def e1_operands(W, B):
    """Layer 0 forward in bf16 storage: frames in {0, 1/4, 1/2, 3/4, 1} (NCHW), sparse integer weights, integer bias: y is a multiple of
    1/4 of magnitude at most 75 + 2, and a multiple of 1/4 is a bf16 number up to 64 (8 significant bits)."""
    x = torch.floor(_u(f"L0/w{W}/x", (B, 3, W, W)) * 5).clamp_(0, 4) / 4.0
    w = sparse_w(f"L0/w{W}/w", (32, 3, 5, 5))
    b = int_bias(f"L0/w{W}/b", 32)
    return dict(x=x, w=w, b=b, ref=F.conv2d(x, w, b, padding=2))


D4_TAPS = 6       # nonzero weights per output channel of the D4 forward case


def d4_fwd_operands(W, B):
    """D4 forward (Upsample -> Conv(32 -> 3) -> Tanh): o3 in {0, 1, 2}; per output channel D4_TAPS weights of +-1/8 on distinct
    (channel, tap) positions; bias a multiple of 1/8 in [-1/2, 1/2].  The pre-activation is a multiple of 1/8 with
    |pre| <= D4_TAPS * 2 / 8 + 1/2 = 2 by construction; the kernel's phase-collapsed weights (sums of at most four taps) are multiples of
    1/8 of magnitude <= 1/2: bf16 numbers.  Returns o3, w, b, pre (float64)."""
    o3 = sparse_act(f"L8/w{W}/o3", (B, 32, W // 2, W // 2), 1.0).abs() * (_u(f"L8/w{W}/lit", (B, 32, W // 2, W // 2)) < 0.95)
    w = torch.zeros(3, 32 * 25, dtype=torch.float64)
    for co in range(3):
        pos = torch.argsort(_u(f"L8/w{W}/pos{co}", (800,)))[:D4_TAPS]
        w[co, pos] = torch.where(_u(f"L8/w{W}/sgn{co}", (D4_TAPS,)) < 0.5, -0.125, 0.125).double()
    w = w.view(3, 32, 5, 5)
    # bias +-3/8 or +-4/8: a sum of D4_TAPS terms of +-1/8, +-2/8 is 0 in about one element of ten, -b far less often
    b = torch.tensor([-4.0, -3.0, 3.0, 4.0], dtype=torch.float64)[(_u(f"L8/w{W}/b", (3,)) * 4).long().clamp_(0, 3)] / 8.0
    return dict(o3=o3, w=w, b=b, pre=F.conv2d(up2(o3), w, b, padding=2))


def d4_bwd_operands(W, B):
    """D4 backward: recon in {0, +-1/2} (1 - r^2 is 1 or 3/4, exact), d_recon in {+-4, +-8}: dOut = d_recon (1 - r^2) is an integer of
    {+-3, +-4, +-6, +-8}; o3 in {0, 1, 2}, nine tenths lit; sparse +-1 weights.  Returns the operands and float64 dout, d_o3, dw, db."""
    recon = (torch.floor(_u(f"L8b/w{W}/r", (B, 3, W, W)) * 3).clamp_(0, 2) - 1.0) / 2.0
    d_recon = dense_act(f"L8b/w{W}/dr", (B, 3, W, W)) * 4.0
    o3 = sparse_act(f"L8b/w{W}/o3", (B, 32, W // 2, W // 2), 1.0).abs() * (_u(f"L8b/w{W}/lit", (B, 32, W // 2, W // 2)) < 0.95)
    w = sparse_w(f"L8b/w{W}/w", (3, 32, 5, 5))
    dout = d_recon * (1.0 - recon * recon)
    d_o3 = torch.where(o3 > 0, F.avg_pool2d(F.conv_transpose2d(dout, w, padding=2), 2) * 4.0, torch.zeros((), dtype=torch.float64))
    dw, db = conv_wgrad_ref(8, o3, dout)
    return dict(recon=recon, d_recon=d_recon, o3=o3, w=w, dout=dout, d_o3=d_o3, dw=dw, db=db)


# ---------------------------------------------------------------------------------------------------------------------------------------
# launch-geometry mirrors
# ---------------------------------------------------------------------------------------------------------------------------------------
def tile_geom(h):
    """Tile<h> (common.h): (TW, TH, images per tile, tiles per image) of the 128-pixel tiles of the forward / input-gradient kernels."""
    tw = min(h, 32)
    th = min(128 // tw, h)
    return tw, th, 128 // (tw * th), (h // tw) * (h // th)


# conv_route's big-tile rows (conv_mfma.hip) and run_big's instantiations (conv_bf16_big.hip): (MT, NT) per (layer, dgrad)
BIG_MT_NT = {(1, False): (8, 32), (2, False): (4, 128), (3, False): (4, 128), (1, True): (8, 32), (2, True): (8, 64), (3, True): (4, 128)}


def big_geometry(layer, W, dgrad, B, cus=256, maxwg=0):
    """run_big: (128-pixel tiles, items = tile groups of MT, tiles per item MT, channel blocks NY, grid) of E2..E4's pass at batch B.
    maxwg mirrors CVAE_PERSIST_MAXWG (persistent_grid)."""
    cin, cout, h, _, _ = geom(layer, W)
    _, _, imgs, tpi = tile_geom(h)
    mt, nt = BIG_MT_NT[layer, bool(dgrad)]
    tiles = cdiv(B, imgs) * tpi
    groups = cdiv(tiles, mt)
    ny = (cin if dgrad else cout) // nt
    items = 8 * cdiv(groups, 8) * ny
    g = cus
    if maxwg and g > maxwg:
        g = maxwg
    g -= g % 8
    g = max(g, 8)
    return tiles, groups, mt, ny, min(g, items)


def wt_tile(h, halo2=True):
    """WtTile<h, 2, 256> (5 x 5 layers) / WtTile<hs, 1, 64> (collapsed up-convs) of conv_bf16.h: (images per tile, tiles per image)."""
    np_ = 256 if halo2 else 64
    tw = min(h, 32)
    th = h if h < np_ // tw else np_ // tw
    imgs = (8 if np_ >= 128 else np_ // 16) if h == 4 else np_ // (tw * th)
    return imgs, (h // tw) * (h // th)


def wgrad_geometry(layer, W, B, cus=256):
    """(tiles, splits, tiles per split, images per tile) of the bf16 weight-gradient kernel of layer 1..7 at batch B.
    Layers 1..4: run_wgrad_bf16 / wgrad_bf16_splits (targets 256 workgroups for E2, whose two output-channel halves share a workgroup,
    512 otherwise; independent of the device).  Layers 5..7: run_up_wgrad (conv_up.hip) caps the splits at min(ceil(2 CUs / blocks), its own
    64-pixel tile count), run_up_wgrad_bf16_main then takes S = ceil(2 CUs / blocks) under that cap and its own tile count."""
    cin, cout, h, up, hs = geom(layer, W)
    if not up:
        imgs, tpi = wt_tile(h)
        tiles = cdiv(B, imgs) * tpi
        cob = 2 if (cin, cout) == (32, 64) else 1
        S = cdiv(256 if cin == 32 else 512, (cin // 32) * (cout // (32 * cob)))
    else:
        imgs, tpi = wt_tile(hs, halo2=False)
        tiles = cdiv(B, imgs) * tpi
        tw64 = min(hs, 16)
        th64 = min(64 // tw64, hs)
        tiles64 = cdiv(B, 64 // (tw64 * th64)) * (hs // tw64) * (hs // th64)          # UpTile64<hs>
        S = min(cdiv(2 * cus, (cin // 32) * (cout // 32)), tiles64)
    S = max(min(S, tiles), 1)
    tps = cdiv(tiles, S)
    return tiles, cdiv(tiles, tps), tps, imgs


def wgrad_two_tile_batch(layer, W, cus=256, limit=1 << 12):
    """The smallest batch at which a weight-gradient split walks two tiles (the prefetching tile loop runs) and the walk ends unevenly:
    the last split is shorter than the others, or the last tile's image group is only partly filled."""
    for B in range(1, limit):
        tiles, S, tps, imgs = wgrad_geometry(layer, W, B, cus)
        if tps >= 2 and (tiles % tps != 0 or B % imgs != 0):
            return B
    raise AssertionError(f"layer {layer} at {W} x {W}: no batch below {limit} walks two tiles per split")


# ---------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm partials of the forward kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def partial_rows(y, tiles_per_partial):
    """Per partial row of the conv forward (one per `tiles_per_partial` consecutive 128-pixel tiles of Tile<h>, in the kernels' tile
    order): float64 (S, M2 about the row's mean, pixel count, Q = sum of squares) of y (B, C, h, h), each (rows, C) / (rows,)."""
    B, C, h, _ = y.shape
    tw, th, imgs, tpi = tile_geom(h)
    b = torch.arange(B).view(B, 1, 1)
    yy = torch.arange(h).view(1, h, 1)
    xx = torch.arange(h).view(1, 1, h)
    row = (((b // imgs) * tpi + (yy // th) * (h // tw) + xx // tw) // tiles_per_partial).reshape(-1)
    rows = cdiv(cdiv(B, imgs) * tpi, tiles_per_partial)
    v = y.double().permute(0, 2, 3, 1).reshape(-1, C)
    S = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, row, v)
    Q = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, row, v * v)
    cnt = torch.zeros(rows, dtype=torch.float64).index_add_(0, row, torch.ones(row.numel(), dtype=torch.float64))
    m2 = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, row, (v - (S / cnt[:, None])[row]) ** 2)
    return S, m2, cnt, Q


# conv_bf16_big.hip, bn_combine: S and Q arrive as fp32 sums (exact below 2^24, which the cases assert); M2 = Q - S S rn in double, stored as
# fp32.  Roundings: S S is exact in double (48 bits), the product with rn one (a power of two for a full row: none), the subtraction one, the
# cast to fp32 one: three, each at most one fp32 ulp of Q (the double ones far less).
COMBINE_ROUNDINGS = 3


def ulp32(v):
    """The fp32 ulp of |v| (float64 tensor), 2^-149 at zero."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 23)


def combine_var_widening(Q, N):
    """What the roundings of M2 = Q - S^2 / n add to the bound of the batch variance: COMBINE_ROUNDINGS ulp(Q) per partial row, over N."""
    return COMBINE_ROUNDINGS * ulp32(Q).sum(0) / N


def far_mean_density(layer):
    """Density of both sparse operands at which the conv output's standard deviation is about 3: var = 25 cin p^2 E[x^2 | lit] with
    E[x^2 | lit] = 2.5 and unit weights."""
    return math.sqrt(9.0 / (2.5 * 25 * LAYERS[layer][0]))
