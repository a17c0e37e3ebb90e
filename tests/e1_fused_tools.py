"""Helpers of test_gpu_e1_fused_ops.py and test_host_e1_fused_tools.py: the fused E1 weight gradient (cvae_op_e1_wgrad_fused:
e1_wgrad_kernel<H, true> on the fp32 handles, e1_wgrad_bf16_kernel<H, XP> on bf16 handles) on operands whose float64 reference is what a
correct kernel must store bit for bit.  Nothing here touches a GPU.

Here: the float64 reference of the dy the kernels form while they stage a tile and of the weight gradient behind it; two kinds of cases
with the conditions under which the comparison may be equality ("route": which pixel of a window receives the gradient, "arith": the
- k1 - xhat k2 correction and the bf16 rounding of dy); the mutated references (what a subtly wrong kernel would compute); and the mirror
of the bf16 launch's split arithmetic.  Activations are NHWC here (B, W, W, 32), frames NCHW, weights OIHW, all float64 on the host."""
import functools

import torch
import torch.nn.functional as F

import bf16_ops_tools as T
import f32_ops_tools as F32
from bf16_ops_tools import EXACT_FP32, cdiv
from ws_tools import bn_windows

C = 32
SCALES = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)        # channel c takes SCALES[c % 6]: on a negative channel the argmax is the minimum of y
ROLES = ("mixed", "pass", "blocked", "mixed", "mixed", "mixed")     # channel c takes ROLES[c // 6]: every role meets every scale
E1W_OCC, THIN_SPLIT_CAP = 3, 1024                 # conv_thin.hip: splits per compute unit of the bf16 kernel, and the cap of both kernels


def bf(t):
    """One round-to-nearest-even to bf16 of fp32-representable float64 values (the callers assert that they are)."""
    return t.float().to(torch.bfloat16).double()


def is_f32(t):
    return bool((t.float().double() == t).all())


def is_bf16(t):
    return bool((bf(t) == t).all())


def role_channels(role):
    return [c for c in range(C) if ROLES[c // 6] == role]


def unwindow(t):
    """The inverse of ws_tools.bn_windows: (B, HO, HO, 4, C) -> (B, 2 HO, 2 HO, C)."""
    B, HO, _, _, Cc = t.shape
    return t.reshape(B, HO, HO, 2, 2, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * HO, 2 * HO, Cc)


def arg_max(nw, last=False):
    """Position of the first (last) maximum along dim 3: scan order (0,0) (0,1) (1,0) (1,1)."""
    top = nw.max(dim=3, keepdim=True).values
    rank = torch.tensor([1, 2, 3, 4] if last else [4, 3, 2, 1]).view(1, 1, 1, 4, 1)
    return ((nw == top) * rank).argmax(dim=3, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
DY_MUTATIONS = ("tie-last", "abs-scale", "gate-ge", "swap-cols", "no-k", "no-round")


def normalised(yw, coef, abs_scale=False):
    """fp32(fma(y, scale, shift)) of windows yw (B, HO, HO, 4, C), as ws_tools.check_bf16_stored_operands' `windows` rounds it: one fp32
    rounding of the exact value."""
    sc = coef[:, 0].abs() if abs_scale else coef[:, 0]
    return (yw * sc + coef[:, 1]).float().double()


def fused_dy_ref(y, a0, d_a0, coef, bcoef, bf16, mut=None):
    """dy of block 0 (B, W, W, C) as the fused kernels form it, in float64: n = fp32(fma(y, scale, shift)); the first maximum of each
    2 x 2 window in scan order; g = d_a0 [a0 > 0]; dy[p] = scale ((p == argmax ? g : 0) - k1 - xhat[p] k2), xhat = (y - mean) invstd; for
    the bf16 kernel one round-to-nearest-even of dy.  y (B, W, W, C), a0 and d_a0 (B, W/2, W/2, C), coef (C, 4) = (scale, shift, mean,
    invstd), bcoef (C, 2) = (k1, k2).
    mut: one mistake of DY_MUTATIONS: the tie routed to the last maximum; the sign of scale ignored in the argmax; the gate taken as
    a0 >= 0; the two columns of every window swapped; the - k1 - xhat k2 term dropped; the bf16 rounding of dy skipped."""
    assert mut is None or mut in DY_MUTATIONS, mut
    B, H, _, Cc = y.shape
    sc, mean, istd, k1, k2 = coef[:, 0], coef[:, 2], coef[:, 3], bcoef[:, 0], bcoef[:, 1]
    yw = bn_windows(y, B, H, Cc)
    pos = arg_max(normalised(yw, coef, mut == "abs-scale"), last=mut == "tie-last")
    g = d_a0 * ((a0 >= 0) if mut == "gate-ge" else (a0 > 0))
    sel = torch.zeros_like(yw).scatter_(3, pos, g.unsqueeze(3))
    dyw = sc * (sel if mut == "no-k" else sel - k1 - (yw - mean) * istd * k2)
    if mut == "swap-cols":
        dyw = dyw[:, :, :, [1, 0, 3, 2]]
    if bf16 and mut != "no-round":
        dyw = bf(dyw)
    return unwindow(dyw)


def recompute_y(x, w1, b1):
    """y as the bf16 kernel recomputes it: bf16(conv(bf16(x), bf16(w1)) + b1), NHWC."""
    return bf(F.conv2d(bf(x), bf(w1), b1, padding=2)).permute(0, 2, 3, 1).contiguous()


def wgrad_ref(x, dy, bf16):
    """dW (OIHW) and db of E1 from the frame x (NCHW; rounded to bf16 first for the bf16 kernel) and dy (NHWC), float64."""
    return T.conv_wgrad_ref(0, bf(x) if bf16 else x, dy.permute(0, 3, 1, 2))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launches' split arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------
def e1_geometry(W, B, bf16, cus=256):
    """(tiles, splits, tiles per split) of launch_e1_wgrad: B (W / 4) (W / 32) tiles of 4 x 32 pixels; thin_splits with 512 wanted splits
    (fp32: f32_ops_tools.wgrad_geometry_f32) or E1W_OCC per compute unit (bf16: e1_splits), under THIN_SPLIT_CAP and the tile count, then
    evened out."""
    if not bf16:
        return F32.wgrad_geometry_f32(0, W, B, cus)[:3]
    tiles = B * (W // 4) * (W // 32)
    S = min(tiles, E1W_OCC * cus, THIN_SPLIT_CAP)
    tps = cdiv(tiles, S)
    return tiles, cdiv(tiles, tps), tps


def walks_unevenly(plan):
    tiles, S, tps = plan
    return tps >= 2 and tiles % tps != 0


def uneven_batch(W, bf16, cus=256, plan=None, limit=1 << 12):
    """The smallest batch at which a split walks at least two tiles (the prefetch of the tile loop runs) and the last split is short.
    plan(B): the launcher's own plan where the caller has it (the GPU tests), else the mirror."""
    plan = plan or (lambda B: e1_geometry(W, B, bf16, cus))
    for B in range(1, limit):
        if walks_unevenly(plan(B)):
            return B
    raise AssertionError(f"{W} x {W}, {'bf16' if bf16 else 'fp32'}: no batch below {limit} walks two tiles per split unevenly")


def tile_mask(W, B, keep):
    """keep (tiles,) bool, tiles in the kernels' order (image, tile row, tile column) -> (B, W, W, 1) mask of their pixels."""
    return keep.view(B, W // 4, W // 32).repeat_interleave(4, 1).repeat_interleave(32, 2).unsqueeze(-1)


TILE_MUTATIONS = ("drop-bottom-row", "drop-last-tile", "first-tile-only")


def tile_mutation_mask(W, B, mut, plan):
    """Pixels a kernel with the mistake still sums: the bottom window row (pixel rows 2, 3) of each 4 x 32 tile dropped; the last tile of
    the last split dropped; every split's second and later tiles dropped (what a dead prefetch path leaves)."""
    tiles, S, tps = plan
    assert tiles == B * (W // 4) * (W // 32)
    if mut == "drop-bottom-row":
        return ((torch.arange(W) % 4) < 2).view(1, W, 1, 1).expand(B, W, W, 1)
    t = torch.arange(tiles)
    return tile_mask(W, B, t != tiles - 1 if mut == "drop-last-tile" else t % tps == 0)


def mutated_ref(c, mut, plan=None):
    """(dW, db) of case c under one mistake of DY_MUTATIONS or TILE_MUTATIONS (those need the launch plan)."""
    if mut in TILE_MUTATIONS:
        dy = c["dy"] * tile_mutation_mask(c["W"], c["B"], mut, plan)
    else:
        dy = fused_dy_ref(c["y"], c["a0"], c["d_a0"], c["coef"], c["bcoef"], c["bf16"], mut)
    return wgrad_ref(c["x"], dy, c["bf16"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def _frame(W, B):
    """Frames dense in {1/4, 1/2, 3/4, 1} (NCHW), as f32_ops_tools.e1_wgrad_operands: bf16 numbers."""
    return (torch.floor(T._u(f"e1f/w{W}/x", (B, 3, W, W)) * 4).clamp_(0, 3) + 1.0) / 4.0


def _int_y(W, B):
    """y of the fp32 kernel: integers of [-4, 4], NHWC."""
    return (torch.floor(T._u(f"e1f/w{W}/y", (B, W, W, C)) * 9).clamp_(0, 8) - 4.0)


def _d_a0(W, B):
    return torch.floor(T._u(f"e1f/w{W}/da", (B, W // 2, W // 2, C)) * 3).clamp_(0, 2) - 1.0


def _shifts(yw, scale):
    """Integer shifts by role (ROLES), from the window maxima m of y scale: "pass" lifts every maximum to at least 1, "blocked" keeps every
    maximum at -1 or below, "mixed" takes to 0 the integer t that splits the windows most evenly into m > t (they pass) and m <= t, among
    the integers that some maximum equals where there is one (those windows are exactly 0)."""
    m = (yw * scale).max(dim=3).values.reshape(-1, C)
    sh = torch.empty(C, dtype=torch.float64)
    for c in range(C):
        role = ROLES[c // 6]
        if role != "mixed":
            sh[c] = 1 - torch.floor(m[:, c].min()) if role == "pass" else -1 - torch.ceil(m[:, c].max())
            continue
        vals, cnt = torch.unique(m[:, c], return_counts=True)
        below = torch.cumsum(cnt, 0).double() / cnt.sum()                      # share of the windows with m <= vals[i]
        best = max((bool(v == v.round()), float(torch.minimum(b, 1 - b)), float(v.floor())) for v, b in zip(vals, below))
        sh[c] = -best[2]
    return sh


def _operands(kind, W, B, bf16):
    """x, y (bf16: recomputed from x, w1, b1), w1, b1 of a case.  bf16: w1 sparse +-1 and b1 integer (bf16_ops_tools.case_operands(0, ..);
    arith: a twelfth of the taps lit, which keeps y narrow), so y is a multiple of 1/4."""
    x = _frame(W, B)
    if not bf16:
        return x, _int_y(W, B), None, None, {}
    if kind == "route":
        f = T.case_operands(0, W, 1, "fwd")
        w1, b1 = f["w"], f["b"]
    else:
        w1, b1 = T.sparse_w(f"e1f/w{W}/w", (C, 3, 5, 5), 1.0 / 12), T.int_bias(f"e1f/w{W}/b", C)
    pre = F.conv2d(x, w1, b1, padding=2)
    cond = {"x, w1, b1 and conv(x, w1) + b1 are bf16 numbers": is_bf16(x) and is_bf16(w1) and is_bf16(b1) and is_bf16(pre),
            "the recomputed y is a multiple of 1/4 with every partial sum exact": bool((pre * 4 == (pre * 4).round()).all()) and 4 * (75 + 2) < EXACT_FP32}
    y = recompute_y(x, w1, b1)
    assert torch.equal(y, pre.permute(0, 2, 3, 1)) or not all(cond.values())
    return x, y, w1, b1, cond


def _finish(kind, W, B, bf16, x, y, w1, b1, coef, bcoef, cond):
    yw = bn_windows(y, B, W, C)
    n = yw * coef[:, 0] + coef[:, 1]
    top = n.max(dim=3).values
    a0 = top.clamp_min(0.0)
    if bf16:                      # a0 is stored as bf16; the kernels only ask whether it is positive, which the rounding keeps
        cond["the bf16 rounding of a0 keeps [a0 > 0]"] = bool(((bf(a0) > 0) == (a0 > 0)).all())
        a0 = bf(a0)
    d_a0 = _d_a0(W, B)
    cond["fma(y, scale, shift) is exact in fp32"] = is_f32(n) and torch.equal(normalised(yw, coef), n)
    lit = a0 > 0
    p, b, m = role_channels("pass"), role_channels("blocked"), role_channels("mixed")
    cond["pass channels pass everywhere, blocked channels nowhere, mixed channels both"] = (
        bool(lit[..., p].all()) and not bool(lit[..., b].any()) and all(0 < int(lit[..., c].sum()) < lit[..., c].numel() for c in m))
    zero_max = int(((top == 0) & (d_a0 != 0))[..., m].sum())
    cond["windows whose maximum is exactly 0 carry a gradient"] = zero_max > 0
    dy = fused_dy_ref(y, a0, d_a0, coef, bcoef, bf16)
    ref_w, ref_b = wgrad_ref(x, dy, bf16)
    ties = int(((n == top.unsqueeze(3)).sum(3) >= 2).sum())
    return dict(kind=kind, W=W, B=B, bf16=bf16, x=x, y=y, w1=w1, b1=b1, a0=a0, d_a0=d_a0, coef=coef, bcoef=bcoef, dy=dy, ref_w=ref_w,
                ref_b=ref_b, cond=cond, ties=ties, zero_max=zero_max)


@functools.lru_cache(maxsize=2)
def route_case(W, B, bf16):
    """Which pixel receives the gradient: scale in {+-1, +-2, +-1/2}, integer shifts by role, mean 0, invstd 1, k1 = k2 = 0, a0 = relu(max n),
    d_a0 in {0, +-1}.  Every dy is 0 or g scale, a multiple of 1/2 of magnitude at most 2, and it is nonzero at no more than one pixel of
    a window; x is a multiple of 1/4 of magnitude at most 1.  Every product is a multiple of 1/8 of magnitude at most 16 eighths, and a dW
    element sums at most B W^2 / 4 nonzero ones: 4 B W^2 eighths, below 2^24, so every fp32 partial sum is exact in any order (bf16
    kernel: dy of at most 3 significant bits and x are bf16 numbers, the products are exact in the MFMA).
    Reports `ties`, the windows whose maximum is reached at two or more positions (the first differs from the last), and `tie_changed`,
    the dW elements that change when the last maximum is taken instead."""
    x, y, w1, b1, cond = _operands("route", W, B, bf16)
    scale = torch.tensor([SCALES[c % 6] for c in range(C)], dtype=torch.float64)
    coef = torch.stack((scale, _shifts(bn_windows(y, B, W, C), scale), torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)), 1)
    c = _finish("route", W, B, bf16, x, y, w1, b1, coef, torch.zeros(C, 2, dtype=torch.float64), cond)
    dy, g = c["dy"], (c["d_a0"] * (c["a0"] > 0))
    c["unit"], c["bound"] = 0.125, 4 * B * W * W
    cond["every dy is 0 or g scale"] = bool(((dy == 0) | (dy.abs() == scale.abs())).all()) and \
        torch.equal(bn_windows(dy, B, W, C).sum(3), g * scale) and torch.equal((bn_windows(dy, B, W, C) != 0).sum(3), (g != 0).long())
    cond["x is a multiple of 1/4 in [1/4, 1]"] = bool(((x * 4 == (x * 4).round()) & (x >= 0.25) & (x <= 1)).all())
    cond["4 B W^2 eighths stay below 2^24"] = c["bound"] < EXACT_FP32
    cond["8 dW and 2 db are integers within the bound"] = bool((c["ref_w"] * 8 == (c["ref_w"] * 8).round()).all()) and \
        float((c["ref_w"] * 8).abs().max()) <= c["bound"] and bool((c["ref_b"] * 2 == (c["ref_b"] * 2).round()).all())
    blocked = role_channels("blocked")
    cond["dW is zero on the blocked channels and at least 90 % nonzero on the others"] = not bool(c["ref_w"][blocked].any()) and \
        float((c["ref_w"][role_channels("pass") + role_channels("mixed")] != 0).double().mean()) >= 0.9
    c["tie_changed"] = int((mutated_ref(c, "tie-last")[0] != c["ref_w"]).sum())
    cond["ties exist and routing them to the last maximum changes dW"] = c["ties"] > 0 and c["tie_changed"] > 0
    return c


WIDE = (4, 11)        # arith_case: the channels whose dy needs more than 8 significant bits
# the batches of F32.BATCHES at which arith_case's sums stay below 2^24 (test_host_e1_fused_tools.py holds the list to arith_case itself)
ARITH_BATCHES = {(64, False): (1, 3, 5, 9), (64, True): (1, 3, 5), (128, False): (1, 3, 5), (128, True): (1,)}


@functools.lru_cache(maxsize=2)
def arith_case(W, B, bf16):
    """The - k1 - xhat k2 correction, and on the bf16 kernel its folded form and the one bf16 rounding of dy: scale as in route_case, mean
    in {-1, 0, 1}, invstd in {1/2, 1}, k1 in {0, +-1/8}, k2 in {0, +-1/4}, y narrow (fp32: integers of [-4, 4]; bf16: quarters from a
    sparse w1).  Every fp32 intermediate of both kernels is asserted to be exactly representable, so dy before the bf16 rounding is the
    float64 value.  Channels WIDE have a mean of +-60 (scale +-1/2, invstd 1/2, k2 +-1/4): there sel - k1 - xhat k2 lies around 8 on a
    grid of 1/32, nine significant bits and more, so the bf16 rounding of dy is a real one (`needs_round` counts the elements it moves).
    dy (rounded, on the bf16 kernel) is a multiple of `dy_unit`, a product x dy one of dy_unit / 4; `bound` is the largest sum of |terms|
    of a dW element, the weight gradient of (|x|, |dy|), in those units, and must stay below 2^24.  It grows with the batch: ValueError
    where it breaks."""
    x, y, w1, b1, cond = _operands("arith", W, B, bf16)
    ch = torch.arange(C)
    scale = torch.tensor([SCALES[c % 6] for c in range(C)], dtype=torch.float64)
    mean = (ch % 3 - 1).double()
    mean[WIDE[0]], mean[WIDE[1]] = 60.0, -60.0
    istd = torch.tensor([1.0, 0.5], dtype=torch.float64)[(ch // 3) % 2]
    k1 = torch.tensor([0.0, 0.125, -0.125], dtype=torch.float64)[(ch // 2) % 3]
    k2 = torch.tensor([0.25, 0.0, -0.25], dtype=torch.float64)[(ch // 5) % 3]
    coef = torch.stack((scale, _shifts(bn_windows(y, B, W, C), scale), mean, istd), 1)
    c = _finish("arith", W, B, bf16, x, y, w1, b1, coef, torch.stack((k1, k2), 1), cond)
    yw = bn_windows(y, B, W, C)
    g = (c["d_a0"] * (c["a0"] > 0)).unsqueeze(3)
    sel = torch.zeros_like(yw).scatter_(3, arg_max(normalised(yw, coef)), g)
    xhat = (yw - mean) * istd
    exact = fused_dy_ref(y, c["a0"], c["d_a0"], coef, c["bcoef"], bf16, "no-round" if bf16 else None)
    steps = [yw - mean, xhat, xhat * k2, sel - k1, sel - k1 - xhat * k2, scale * (sel - k1 - xhat * k2)]
    cond["every intermediate of e1_wgrad_kernel is exact in fp32"] = all(is_f32(s) for s in steps) and torch.equal(unwindow(steps[-1]), exact)
    if bf16:
        bB = scale * k2 * istd
        bA = scale * k1 - bB * mean
        tv = bB * yw + bA
        folded = [scale * k2, bB, scale * k1, bB * mean, bA, bB * yw, tv, g * scale, sel * scale - tv]
        cond["every intermediate of e1_wgrad_bf16_kernel, with the folded bA and bB, is exact in fp32"] = \
            all(is_f32(s) for s in folded) and torch.equal(unwindow(folded[-1]), exact)
    c["needs_round"] = int((bf(exact) != exact).sum()) if bf16 else 0
    dy = c["dy"]
    k = next(k for k in range(16) if bool((dy * 2 ** k == (dy * 2 ** k).round()).all()))
    c["dy_unit"], c["unit"] = 2.0 ** -k, 2.0 ** -(k + 2)
    c["bound"] = float(wgrad_ref(x.abs(), dy.abs(), bf16)[0].max()) / c["unit"]
    if c["bound"] >= EXACT_FP32:
        raise ValueError(f"arith case at {W} x {W}, B = {B}, bf16 = {bf16}: sum |dy| / unit = {c['bound']:.0f} >= 2^24: a partial sum could round")
    cond["x is a multiple of 1/4 in [1/4, 1]"] = bool(((x * 4 == (x * 4).round()) & (x >= 0.25) & (x <= 1)).all())
    cond["dy is a bf16 number on the bf16 kernel"] = not bf16 or is_bf16(dy)
    cond["dW / unit is an integer within the bound"] = bool((c["ref_w"] / c["unit"] == (c["ref_w"] / c["unit"]).round()).all()) and \
        float(c["ref_w"].abs().max()) / c["unit"] <= c["bound"]
    cond["the correction is there: dy is nonzero away from the argmax"] = float((dy != 0).double().mean()) > 0.5
    return c


def assert_conditions(c):
    """What a case asserts on its reference BEFORE it touches a kernel."""
    bad = [k for k, ok in c["cond"].items() if not ok]
    assert not bad, f"{c['kind']} case at {c['W']} x {c['W']}, B = {c['B']}, bf16 = {c['bf16']}: " + "; ".join(bad)
    return c


# which cases a mutated reference is meant to differ on ("first-tile-only": where a split walks two tiles, which no arith batch does)
SEEN_BY = {"tie-last": ("route",), "abs-scale": ("route", "arith"), "gate-ge": ("route", "arith"), "swap-cols": ("route", "arith"),
           "drop-bottom-row": ("route", "arith"), "drop-last-tile": ("route", "arith"), "first-tile-only": ("route",),
           "no-k": ("arith",), "no-round": ("arith",)}
