"""Helpers of test_gpu_f32_ops.py and test_host_f32_ops_tools.py: what the fp32 (precision 0) conv kernels need on top of bf16_ops_tools,
whose integer operands and float64 references do not depend on the storage type and are imported, not copied.  Nothing here touches a GPU.

Here: E1's weight-gradient operands, the mirror of the fp32 weight-gradient split arithmetic (held to cvae_op_conv_wgrad_plan_f32 on the
host), the pixels of a weight-gradient tile (for the mutated references of the host tests), mutated forms of the references, and the
grouping check of the D4 forward."""
import torch
import torch.nn.functional as F

import bf16_ops_tools as T
from bf16_ops_tools import EXACT_FP32, cdiv, geom

CU_COUNTS = (64, 104, 256, 304)       # the device sizes at which the host tests hold the mirror and the case batches


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases of test_gpu_f32_ops.py (the host tests check every one of them against its exactness conditions)
# ---------------------------------------------------------------------------------------------------------------------------------------
CAPPED_B = 37
BATCHES = {64: (1, 3, 5, 9, CAPPED_B), 128: (1, 3, 5)}
UP17 = {(64, 5): (17,), (64, 6): (17,), (64, 7): (17,)}
D0_GROUPS = {(64, 4): (33, 40)}                       # forward and input gradient only
CAPPED_128 = [(128, CAPPED_B, layer) for layer in (1, 2, 3)]


def cases(what):
    extra = {**UP17, **(D0_GROUPS if what != "wgrad" else {})}
    out = [(W, B, layer) for W in (64, 128) for layer in range(1, 8) for B in BATCHES[W] + extra.get((W, layer), ())]
    return out + (CAPPED_128 if what != "wgrad" else [])


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def e1_wgrad_operands(W, B, unit=False):
    """E1's weight gradient: frames dense in {1/4, 1/2, 3/4, 1} (NCHW), dy dense in {+-1, +-2} (+-1 with `unit`).  Every product is a
    multiple of 1/4 of magnitude at most 2, so 4 dW is an integer bounded by 8 B W^2 (4 B W^2 with `unit`): below 2^24 every fp32
    partial sum is exact in any order.  Returns x, dout, ref_w (float64, OIHW) and that bound."""
    x = (torch.floor(T._u(f"L0w/w{W}/x", (B, 3, W, W)) * 4).clamp_(0, 3) + 1.0) / 4.0
    dout = T.dense_act(f"L0w/w{W}/dy", (B, 32, W, W))
    if unit:
        dout = dout.sign()
    return dict(x=x, dout=dout, ref_w=T.conv_wgrad_ref(0, x, dout)[0], bound=(4 if unit else 8) * B * W * W)


def wgrad_bound(layer, W, B, unit=False):
    """Upper bound of the sum of |terms| of one weight-gradient element in the unit of its integer grid (1; 1/4 for E1): layers 1..7
    B h^2 products of at most 4 (1 with `unit`), E1 8 B W^2 quarters (4 B W^2), D4 16 B W^2 (|dOut| <= 8, o3 <= 2)."""
    if layer == 0:
        return (4 if unit else 8) * B * W * W
    if layer == 8:
        return 16 * B * W * W
    return B * geom(layer, W)[2] ** 2 * (1 if unit else 4)


def wgrad_case(layer, W, B):
    """Dense weight-gradient operands of layer 0..7 at batch B whose bound is below 2^24: bf16_ops_tools' {+-1, +-2} (E1: quarters against
    {+-1, +-2}), or, where that bound breaks, both operands reduced to their signs (E1: dy only).  Returns x, dout, ref_w, ref_b (None for
    E1), bound, unit."""
    unit = wgrad_bound(layer, W, B) >= EXACT_FP32
    if layer == 0:
        c = e1_wgrad_operands(W, B, unit)
        return dict(c, ref_b=None, unit=unit)
    if not unit:
        return dict(T.case_operands(layer, W, B, "wgrad"), bound=wgrad_bound(layer, W, B), unit=False)
    cin, cout, h, up, hs = geom(layer, W)
    x, dout = T.dense_act(f"L{layer}/w{W}/wx", (B, cin, hs, hs)).sign(), T.dense_act(f"L{layer}/w{W}/wdo", (B, cout, h, h)).sign()
    if up:
        x = x.abs()
    ref_w, ref_b = T.conv_wgrad_ref(layer, x, dout)
    return dict(x=x, dout=dout, ref_w=ref_w, ref_b=ref_b, bound=wgrad_bound(layer, W, B, True), unit=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fp32 weight-gradient launchers' split arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------
def up_tile64(hs):
    """UpTile64<HS> (conv_up.hip): (TW, TH, images per tile, tiles per image) of the 64-low-resolution-pixel tiles of D1..D3's weight gradient."""
    tw = min(hs, 16)
    th = min(64 // tw, hs)
    return tw, th, 64 // (tw * th), (hs // tw) * (hs // th)


def wgrad_tile_shape(layer, W):
    """(tile width, tile height, images per tile, tiles per image) of the fp32 weight-gradient kernel of layer 0..8, in the pixels the
    kernel tiles: E1 4 x 32 strips of y (B (W / 4) (W / 32) tiles), layers 1..4 Tile<h> (128 pixels), D1..D3 UpTile64<hs> (64 pixels of
    the stored low-resolution input), D4 16 x 32 blocks of recon (B (W / 16) (W / 32) tiles)."""
    cin, cout, h, up, hs = geom(layer, W)
    if layer == 0:
        return 32, 4, 1, (W // 4) * (W // 32)
    if layer == 8:
        return 32, 16, 1, (W // 16) * (W // 32)
    if up:
        return up_tile64(hs)
    return T.tile_geom(h)


def wgrad_geometry_f32(layer, W, B, cus=256):
    """(tiles, splits, tiles per split, images per tile) of the fp32 weight-gradient kernel of layer 0..8 (8: the fused D4 backward) at
    batch B on a device of `cus` compute units.  Layers 0 and 8: thin_splits with 512 wanted splits (launch_e1_wgrad, d4_splits).
    Layers 1..4: wgrad_splits<H>, ceil(512 / blocks) splits, blocks = (cin / 32) (cout / 32).  Layers 5..7: run_up_wgrad's fp32 S,
    ceil(CUs / blocks).  Each under the tile count, then evened out: tps = ceil(tiles / S), S = ceil(tiles / tps)."""
    cin, cout, h, up, hs = geom(layer, W)
    _, _, imgs, tpi = wgrad_tile_shape(layer, W)
    tiles = cdiv(B, imgs) * tpi
    if layer in (0, 8):
        S = 512
    else:
        S = cdiv(cus if up else 512, (cin // 32) * (cout // 32))
    S = max(min(S, tiles), 1)
    tps = cdiv(tiles, S)
    return tiles, cdiv(tiles, tps), tps, imgs


def walks_two_tiles_unevenly(layer, W, B, cus=256):
    tiles, S, tps, imgs = wgrad_geometry_f32(layer, W, B, cus)
    return tps >= 2 and (tiles % tps != 0 or B % imgs != 0)


def wgrad_two_tile_batch_f32(layer, W, cus=256, limit=1 << 12):
    """The smallest batch at which a split of the fp32 weight-gradient kernel walks at least two tiles and the walk ends unevenly: the
    last split is shorter than the others, or the last tile's image group is only partly filled."""
    for B in range(1, limit):
        if walks_two_tiles_unevenly(layer, W, B, cus):
            return B
    raise AssertionError(f"layer {layer} at {W} x {W}: no batch below {limit} walks two tiles per split")


def wgrad_tile_box(layer, W, t):
    """Tile t of the weight-gradient kernel as a box of the OUTPUT gradient (B, cout, h, h): (first image, images, y0, y1, x0, x1), tiles
    of an image group in row-major order.  D1..D3: the tile's low-resolution pixels doubled.  Only the mutated references of the host
    tests use it: which terms a tile holds, not the order a kernel walks them in."""
    tw, th, imgs, tpi = wgrad_tile_shape(layer, W)
    up = 5 <= layer <= 7
    side = geom(layer, W)[4] if up else geom(layer, W)[2]
    g, r = divmod(t, tpi)
    ty, tx = divmod(r, side // tw)
    k = 2 if up else 1
    return g * imgs, imgs, ty * th * k, (ty + 1) * th * k, tx * tw * k, (tx + 1) * tw * k


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutated references: what a subtly wrong kernel would compute
# ---------------------------------------------------------------------------------------------------------------------------------------
def wgrad_ref_without(layer, x, dout, box, ref):
    """The float64 weight gradient `ref` with the output-gradient pixels of `box` (first image, images, y0, y1, x0, x1) left out of the
    sums: ref minus the sum over those pixels alone (the sums are linear in their terms, and exact in float64 on integer operands)."""
    b0, n, y0, y1, x0, x1 = box
    d = torch.zeros_like(dout[b0:b0 + n])
    d[:, :, y0:y1, x0:x1] = dout[b0:b0 + n, :, y0:y1, x0:x1]
    return ref - T.conv_wgrad_ref(layer, x[b0:b0 + n], d)[0]


def collapse_w_neighbour_slot(w, py, ta):
    """bf16_ops_tools.collapse_w with one mistake: the row slot `ta` of phase row `py` sums the 5 x 5 rows that belong to the same slot of
    the other phase row (R(0, .) against R(1, .))."""
    wc = T.collapse_w(w)
    for px in (0, 1):
        for tb in range(3):
            wc[2 * py + px, :, :, ta, tb] = 0
            for r in T.PHASE_TAPS[1 - py][ta]:
                for s in T.PHASE_TAPS[px][tb]:
                    wc[2 * py + px, :, :, ta, tb] += w[:, :, r, s]
    return wc


def up_dgrad_three_of_four(dout, w, mask_src):
    """conv_dgrad_ref of D1..D3 with the 2 x 2 upsample sum taken over three of its four pixels (the odd / odd one left out)."""
    d = F.conv_transpose2d(dout, w, padding=2)
    d = F.avg_pool2d(d, 2) * 4.0 - d[:, :, 1::2, 1::2]
    return torch.where(mask_src > 0, d, torch.zeros((), dtype=d.dtype))


# ---------------------------------------------------------------------------------------------------------------------------------------
# D4 forward: one bit pattern per pre-activation value
# ---------------------------------------------------------------------------------------------------------------------------------------
def d4_value_groups(recon, pre):
    """The structural check of the D4 forward on d4_fwd_operands: the pre-activation is exact (a multiple of 1/8 in [-2, 2], every partial
    sum exact in fp32), so all elements of recon (fp32) whose expected pre-activation `pre` (float64, same shape) is the same value must
    hold one and the same bit pattern, whatever tanh the kernel uses.  Grouped by SIGNED value: the kernel's tanh, 1 - 2 / (exp(2x) + 1),
    is not an odd function in floating point.  Returns (values, patterns as int32); raises AssertionError with the first offending value."""
    assert recon.dtype == torch.float32 and recon.shape == pre.shape
    bits = recon.contiguous().view(torch.int32).flatten().long()
    vals, inv = torch.unique(pre.flatten(), return_inverse=True)
    assert len(vals) <= 33, f"{len(vals)} distinct pre-activations: not the multiples of 1/8 in [-2, 2]"
    lo = torch.full((len(vals),), 1 << 40).scatter_reduce_(0, inv, bits, "amin")
    hi = torch.full((len(vals),), -(1 << 40)).scatter_reduce_(0, inv, bits, "amax")
    bad = (lo != hi).nonzero().flatten()
    if len(bad):
        k = int(bad[0])
        members = bits[inv == k]
        n_other = int((members != members[0]).sum())
        raise AssertionError(f"D4 forward: {len(bad)} of {len(vals)} pre-activation values map to more than one bit pattern; pre = {float(vals[k])!r}: "
                             f"{n_other} of {len(members)} elements differ from the first ({int(lo[k]):#x} .. {int(hi[k]):#x})")
    return vals, lo.int()
