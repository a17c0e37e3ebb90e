"""The conv kernels of the fp32-emulation modes ("bf16x9", "bf16x6"), op by op.

On a handle of these modes the per-op conv entry points run layers 1..4 (E2..E4, D0) on the kernels the training step runs there:
conv5x5_bf16_kernel with three operand splits for the forward and the input gradient (conv_bf16.hip; D0 at 64 x 64 as split-K plus a
finish launch) and conv5x5_wgrad_split_kernel for the weight gradient (conv_wgrad_split.hip).  Two kinds of test:

(a) random operands against the float64 reference, at the tolerances of test_gpu_ops (1e-4 absolute on the forward, 1e-4 of the tensor's
    max on gradients), at batches that leave tiles half full (odd B: E4's two-image tile, D0's eight- and four-image groups) and at
    which a weight-gradient split walks more than one tile and ends unevenly;
(b) exact products.  The modes promise an exact three-way bf16 split (x = hi + mid + lo, conv_bf16.h::split3) with exact partial
    products, so that only the summation order differs from fp32.  A dropped `lo` part moves a product by 2^-16 relative, far below
    (a)'s bar.  Here one operand is sparse with entries exactly 1.0 = (1, 0, 0) and the other holds full-mantissa values, placed so that
    every output element is ONE input element or zero: its three partial products (hi, mid, lo times 1) are among the six "bf16x6"
    keeps, every other addend is an exact zero, and (lo + mid) + hi, the kernels' smallest-first order, rounds back to x.  The
    reference is an index shift and the comparison is equality; the fp32 MFMA kernels are exact on these inputs for the same reason."""
import functools

import pytest
import torch
import torch.nn.functional as F

from critic_vae_amd import lib as cvlib
from oracle import cvae_oracle as orc
from test_gpu_ops import check, dev, f64, geom, handle, nhwc, rnd, to_nchw, wnat, wref
from ws_tools import ALL_ONES, poison

pytestmark = pytest.mark.gpu
MODES = ["bf16x9", "bf16x6"]
_handles = {}


def mode_handle(W, B, mode):
    """One handle per (width, batch, mode); "f32" shares test_gpu_ops' handles."""
    if mode == "f32":
        return handle(W, B)
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if (W, B, mode) not in _handles:
        _handles[W, B, mode] = cvlib.Handle(W, B, precision=mode)
    return _handles[W, B, mode]


def scratch(H, B):
    return poison(torch.empty(H.op_scratch_floats(B), device="cuda"), ALL_ONES)     # packed weights and split-K slabs land in NaNs


def run_fwd(H, B, layer, W, x, w, b):
    """-> (y as NCHW on the host, y on the device, its BatchNorm partials or None)."""
    cin, cout, h, _, _ = geom(layer, W)
    out = torch.full((B * h * h * cout,), float("nan"), device="cuda")
    part = poison(torch.empty(H.op_bn_partial_floats(layer, B), device="cuda"), ALL_ONES) if layer < 4 else None
    H.op_conv_fwd(layer, B, nhwc(x), wnat(w), dev(b), out, part, scratch(H, B))
    torch.cuda.synchronize()
    return to_nchw(out, B, h, cout), out, part


def run_dgrad(H, B, layer, W, dout, w):
    cin, cout, h, _, hs = geom(layer, W)
    din = torch.full((B * hs * hs * cin,), float("nan"), device="cuda")
    H.op_conv_dgrad(layer, B, nhwc(dout), wnat(w), None, din, scratch(H, B))
    torch.cuda.synchronize()
    return to_nchw(din, B, hs, cin)


def run_wgrad(H, B, layer, W, x, dout):
    """-> (dW as OIHW on the host, db on the host or None).  The bias gradient is taken for layer 4 (D0), as in the step."""
    cin, cout, _, _, _ = geom(layer, W)
    dw = torch.full((25 * cin * cout,), float("nan"), device="cuda")
    dbias = torch.full((cout,), float("nan"), device="cuda") if layer == 4 else None
    H.op_conv_wgrad(layer, B, nhwc(x), nhwc(dout), dw, dbias, scratch(H, B))
    torch.cuda.synchronize()
    return wref(dw, cin, cout), (dbias.cpu() if dbias is not None else None)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) random operands against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------
# (width, batch, layers).  64 x 64: odd B half-fills E4's two-image tile and D0's eight- / four-image groups; at 37 the weight-gradient
# splits of E2, E3 and E4 walk two tiles and end unevenly; 69 is 18 four-image tiles of D0, the last holding one image.  128 x 128: at 9
# the splits of E2..E4 walk more than one tile, at 35 those of D0 (18 two-image tiles).
A_SHAPES = [(64, 1, (1, 2, 3, 4)), (64, 3, (1, 2, 3, 4)), (64, 37, (1, 2, 3, 4)), (64, 69, (4,)),
            (128, 1, (1, 2, 3, 4)), (128, 3, (1, 2, 3, 4)), (128, 9, (1, 2, 3, 4)), (128, 35, (4,))]
A_CASES = [(W, B, layer) for W, B, layers in A_SHAPES for layer in layers]
# the cases named "more than one tile per split"
MULTI_TILE = {(64, 37, 1), (64, 37, 2), (64, 37, 3), (64, 69, 4), (128, 9, 1), (128, 9, 2), (128, 9, 3), (128, 35, 4)}
a_cases = pytest.mark.parametrize("W,B,layer", A_CASES, ids=[f"w{w}-b{b}-L{l}" for w, b, l in A_CASES])
modes = pytest.mark.parametrize("mode", MODES)


def wgrad_split_geometry(layer, W, B):
    """(tiles, splits, tiles per split) of conv5x5_wgrad_split_kernel for this pass on this device: SplitTile<h> (128 pixels; 64 = four
    images at 4 x 4) and the split count of run_wgrad_split, S = ceil(2 CUs / ((CIN / 32)(COUT / 32))) capped at the tile count."""
    cin, cout, h, _, _ = geom(layer, W)
    npx = 64 if h == 4 else 128
    tw = min(h, 32)
    th = min(h, npx // tw)
    imgs = npx // 16 if h == 4 else npx // (tw * th)
    tiles = -(-B // imgs) * (h // tw) * (h // th)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    S = max(min(-(-2 * cus // ((cin // 32) * (cout // 32))), tiles), 1)
    tps = -(-tiles // S)
    return tiles, -(-tiles // tps), tps


@functools.lru_cache(maxsize=2)          # the mode varies fastest: both modes share one float64 reference, then it is dropped
def reference(W, B, layer, what):
    cin, cout, h, _, hs = geom(layer, W)
    w = rnd(f"w{layer}", (cout, cin, 5, 5), -0.1, 0.1)
    if what == "fwd":
        x, b = rnd(f"x{layer}", (B, cin, hs, hs)), rnd(f"b{layer}", (cout,))
        ref = orc.conv5x5(f64(x), f64(w), f64(b), upsample_input=False)
        return x, w, b, (torch.relu(ref) if layer == 4 else ref)
    if what == "dgrad":
        dout = rnd(f"do{layer}", (B, cout, h, h))
        pre = f64(rnd(f"pre{layer}", (B, cin, hs, hs))).requires_grad_(True)
        orc.conv5x5(pre, f64(w), None, upsample_input=False).backward(f64(dout))
        return dout, w, pre.grad
    x, dout = rnd(f"x{layer}", (B, cin, hs, hs)), rnd(f"do{layer}", (B, cout, h, h))
    w64 = f64(w).requires_grad_(True)
    b64 = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    orc.conv5x5(f64(x), w64, b64, upsample_input=False).backward(f64(dout))
    return x, dout, w64.grad, b64.grad


@modes
@a_cases
def test_emulated_conv_fwd(W, B, layer, mode):
    """Forward of E2..E4 / D0 at TOL absolute (test_conv_fwd's bar).  The BatchNorm partials of E2..E4 are handed in poisoned and must
    reproduce the mean and variance of y through op_bn_pool_act_fwd, at the 1e-5 bounds of test_bn_pool_act_fwd_bwd."""
    H = mode_handle(W, B, mode)
    x, w, b, ref = reference(W, B, layer, "fwd")
    got, y, part = run_fwd(H, B, layer, W, x, w, b)
    check(got, ref, f"{mode} conv_fwd L{layer}")
    if part is None:
        return
    _, C, h, _, _ = geom(layer, W)
    gamma, beta = rnd(f"g{layer}", (C,), 0.5, 1.5), rnd(f"be{layer}", (C,), -0.5, 0.5)
    _, mean, var = orc.bn_pool_act(f64(got), f64(gamma), f64(beta), "tanh" if layer == 3 else "relu")
    rm, rv, coef = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.empty(C * 4, device="cuda")
    a = torch.empty(B * (h // 2) ** 2 * C, device="cuda")
    H.op_bn_pool_act_fwd(layer, B, y, part, dev(gamma), dev(beta), rm, rv, coef, a, scratch(H, B), True)
    torch.cuda.synchronize()
    check(coef.view(C, 4)[:, 2], mean, "bn mean from the conv's partials", 1e-5)
    check(1.0 / coef.view(C, 4)[:, 3].double() ** 2 - 1e-5, var, "bn var from the conv's partials", 1e-5, rel=True)


@modes
@a_cases
def test_emulated_conv_dgrad(W, B, layer, mode):
    """Input gradient at 1e-4 of the tensor's max (test_conv_dgrad's bar); D0 at 64 x 64 through its split-K slabs."""
    dout, w, ref = reference(W, B, layer, "dgrad")
    check(run_dgrad(mode_handle(W, B, mode), B, layer, W, dout, w), ref, f"{mode} conv_dgrad L{layer}", rel=True)


@modes
@a_cases
def test_emulated_conv_wgrad(W, B, layer, mode):
    """Weight gradient, and D0's bias gradient, at 1e-4 of the tensor's max (test_conv_wgrad's bar).  The cases that are there for the
    prefetching tile loop (tile mt + 1 fetched while tile mt computes) must walk at least two tiles per split on this device."""
    if (W, B, layer) in MULTI_TILE:
        tiles, S, tps = wgrad_split_geometry(layer, W, B)
        assert tps >= 2, f"layer {layer} at {W} x {W}, B={B}: {tiles} tiles on {S} splits: one tile per split on this device"
    x, dout, ref_w, ref_b = reference(W, B, layer, "wgrad")
    dw, db = run_wgrad(mode_handle(W, B, mode), B, layer, W, x, dout)
    check(dw, ref_w, f"{mode} conv_wgrad L{layer}", rel=True)
    if db is not None:
        check(db, ref_b, f"{mode} conv dbias L{layer}", rel=True)


@modes
def test_emulated_conv_ops_reject_a_null_scratch(mode):
    """The packed weights live in the scratch: without one the ops fail before any launch."""
    W, B, layer = 64, 1, 3
    H = mode_handle(W, B, mode)
    cin, cout, h, _, _ = geom(layer, W)
    x, w, dout = torch.zeros(B * h * h * cin, device="cuda"), torch.zeros(25 * cin * cout, device="cuda"), torch.zeros(B * h * h * cout, device="cuda")
    out, part = torch.empty_like(dout), torch.empty(H.op_bn_partial_floats(layer, B), device="cuda")
    with pytest.raises(cvlib.CvaeError, match="scratch"):
        H.op_conv_fwd(layer, B, x, w, torch.zeros(cout, device="cuda"), out, part, None)
    with pytest.raises(cvlib.CvaeError, match="scratch"):
        H.op_conv_dgrad(layer, B, dout, w, None, torch.empty_like(x), None)
    with pytest.raises(cvlib.CvaeError, match="scratch"):
        H.op_conv_wgrad(layer, B, x, dout, torch.empty_like(w), None, None)
    assert H.op_scratch_floats(B) > handle(W, B).op_scratch_floats(B)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) exact products
# ---------------------------------------------------------------------------------------------------------------------------------------
X_MODES = ["f32"] + MODES
X_CASES = [(W, 3, layer) for W in (64, 128) for layer in (1, 2, 3, 4)]
x_cases = pytest.mark.parametrize("W,B,layer", X_CASES, ids=[f"w{w}-b{b}-L{l}" for w, b, l in X_CASES])
x_modes = pytest.mark.parametrize("mode", X_MODES)


def full(name, shape):
    """Full-mantissa uniform values in (-1, 1): they equal the sum of their three bf16 parts, smallest first, and all three parts are
    non-zero in most elements (lo is zero where the remainder behind hi happens to fit mid's 8 bits: about one element in seven)."""
    v = rnd(f"exact/{name}", shape)
    hi = v.bfloat16().float()
    mid = (v - hi).bfloat16().float()
    lo = ((v - hi) - mid).bfloat16().float()
    assert torch.equal((lo + mid) + hi, v) and float((lo != 0).float().mean()) > 0.8 and float((mid != 0).float().mean()) > 0.95
    return v


def lit_pixels(h):
    """Positions of the lit pixels: corners, edges and interior (at 4 x 4 the interior is rows / columns 1..2)."""
    return [(0, 0), (h - 1, h // 2), (h // 2, h // 2 - 1), (h - 1, h - 1), (h // 2 - 1, h - 1), (1, h - 2), (0, h - 1)]


def gather_shift(src, ch, tap):
    """out[b, n, p] = src[b, ch[n], p + tap[n] - 2] with zero outside the image (tap = 5 ky + kx)."""
    B, _, h, _ = src.shape
    sp = F.pad(src, (2, 2, 2, 2))
    out = torch.empty(B, len(ch), h, h)
    for n, (c, t) in enumerate(zip(ch, tap)):
        out[:, n] = sp[:, c, t // 5:t // 5 + h, t % 5:t % 5 + h]
    return out


def one_hot_weight(cout, cin, co, ci, tap):
    w = torch.zeros(cout, cin, 25)
    w[co, ci, tap] = 1.0
    return w.view(cout, cin, 5, 5)


def one_lit_pixel_per_image(B, c, h):
    """(tensor, [(channel, y, x) per image]): image 0 a corner, image 1 an edge, image 2 interior; channels in three different 32-blocks
    where the layer has them."""
    t = torch.zeros(B, c, h, h)
    where = [((c - 1, c // 2 + 5, 3)[b % 3], *lit_pixels(h)[b % 3]) for b in range(B)]
    for b, (ch, y, x) in enumerate(where):
        t[b, ch, y, x] = 1.0
    return t, where


def one_lit_pixel_per_channel(B, c, h):
    """(tensor, [(image, y, x) per channel]): channel n lit in image n % B, positions cycling through lit_pixels."""
    t = torch.zeros(B, c, h, h)
    P = lit_pixels(h)
    where = [(n % B, *P[n % len(P)]) for n in range(c)]
    for n, (b, y, x) in enumerate(where):
        t[b, n, y, x] = 1.0
    return t, where


def assert_exact(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert int((want != 0).sum()) >= want[..., 0, 0].numel() if want.dim() == 4 else bool((want != 0).all()), f"{what}: the expected output is (nearly) empty"
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        err = (got.double() - want.double()).abs()[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} elements differ, max |diff| {float(err.max()):.3e}, "
                             f"first at {tuple(bad.nonzero()[0].tolist())}")


def oracle_fwd(x, w, layer):
    ref = orc.conv5x5(f64(x), f64(w), None, upsample_input=False)
    return torch.relu(ref) if layer == 4 else ref


def oracle_dgrad(dout, w, shape):
    pre = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    orc.conv5x5(pre, f64(w), None, upsample_input=False).backward(f64(dout))
    return pre.grad


def oracle_wgrad(x, dout, shape):
    w = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    orc.conv5x5(f64(x), w, None, upsample_input=False).backward(f64(dout))
    return w.grad


def same_as_oracle(ref, oracle, what):
    """The index-shift reference against the float64 conv on the same operands: every sum there has one non-zero term, so equal too."""
    assert torch.equal(ref.double(), oracle), f"{what}: the index-shift reference is not the convolution"
    return ref


@functools.lru_cache(maxsize=2)          # the mode varies fastest: the three modes share the operands and the reference
def exact_case(kind, W, B, layer):
    """-> [(first operand, second operand, expected)] of one exact-product construction; operands in run_fwd / run_dgrad / run_wgrad's
    order, everything NCHW / OIHW on the host."""
    cin, cout, h, _, _ = geom(layer, W)
    relu = (lambda t: torch.relu(t)) if layer == 4 else (lambda t: t)
    runs = []
    if kind == "fwd_one_hot_weight":
        # w[co, ci(co), co % 25] = 1: y[b, co, p] = x[b, ci(co), p + tap - 2] (ReLU on D0): all 25 taps and the whole halo at once
        x, co = full(f"x{layer}", (B, cin, h, h)), torch.arange(cout)
        for p in range(max(1, cin // cout)):          # cin > cout: two channel maps that between them hit every input channel
            ci, tap = (co + p * cout) % cin, co % 25
            w = one_hot_weight(cout, cin, co, ci, tap)
            runs.append((x, w, same_as_oracle(relu(gather_shift(x, ci.tolist(), tap.tolist())), oracle_fwd(x, w, layer), kind)))
    elif kind == "fwd_one_lit_pixel":
        # x[b, c_b, q_b] = 1, full-mantissa weights: y[b, co, p] = w[co, c_b, q_b - p + 2], zero where that tap does not exist
        w = full(f"w{layer}", (cout, cin, 5, 5))
        x, where = one_lit_pixel_per_image(B, cin, h)
        ref = torch.zeros(B, cout, h, h)
        for b, (c, y0, x0) in enumerate(where):
            for ky in range(5):
                for kx in range(5):
                    py, px = y0 - ky + 2, x0 - kx + 2
                    if 0 <= py < h and 0 <= px < h:
                        ref[b, :, py, px] = w[:, c, ky, kx]
        runs.append((x, w, same_as_oracle(relu(ref), oracle_fwd(x, w, layer), kind)))
    elif kind == "dgrad_one_hot_weight":
        # the transposed operation: w[co(ci), ci, ci % 25] = 1: din[b, ci, q] = dout[b, co(ci), q - tap + 2]
        dout, ci = full(f"do{layer}", (B, cout, h, h)), torch.arange(cin)
        for p in range(max(1, cout // cin)):          # cout > cin: two channel maps that between them hit every channel of dout
            co, tap = (ci + p * cin) % cout, ci % 25
            w = one_hot_weight(cout, cin, co, ci, tap)
            ref = gather_shift(dout, co.tolist(), (24 - tap).tolist())
            runs.append((dout, w, same_as_oracle(ref, oracle_dgrad(dout, w, (B, cin, h, h)), kind)))
    elif kind == "dgrad_one_lit_pixel":
        # dout[b, c_b, p_b] = 1, full-mantissa weights: din[b, ci, q] = w[c_b, ci, q - p_b + 2]
        w = full(f"w{layer}", (cout, cin, 5, 5))
        dout, where = one_lit_pixel_per_image(B, cout, h)
        ref = torch.zeros(B, cin, h, h)
        for b, (c, y0, x0) in enumerate(where):
            for ky in range(5):
                for kx in range(5):
                    qy, qx = y0 + ky - 2, x0 + kx - 2
                    if 0 <= qy < h and 0 <= qx < h:
                        ref[b, :, qy, qx] = w[c, :, ky, kx]
        runs.append((dout, w, same_as_oracle(ref, oracle_dgrad(dout, w, (B, cin, h, h)), kind)))
    elif kind == "wgrad_one_lit_dout_pixel":
        # dout[co % B, co, p_co] = 1: dW[co, ci, tap] = x[co % B, ci, p_co + tap - 2] or zero
        x = full(f"x{layer}", (B, cin, h, h))
        dout, where = one_lit_pixel_per_channel(B, cout, h)
        xp = F.pad(x, (2, 2, 2, 2))
        ref = torch.stack([xp[b, :, y0:y0 + 5, x0:x0 + 5] for b, y0, x0 in where])
        runs.append((x, dout, same_as_oracle(ref, oracle_wgrad(x, dout, (cout, cin, 5, 5)), kind)))
    else:
        # "wgrad_one_lit_input_pixel", the mirror image: x[ci % B, ci, q_ci] = 1: dW[co, ci, tap] = dout[ci % B, co, q_ci - tap + 2] or zero
        dout = full(f"do{layer}", (B, cout, h, h))
        x, where = one_lit_pixel_per_channel(B, cin, h)
        dp = F.pad(dout, (2, 2, 2, 2))
        ref = torch.stack([dp[b, :, y0:y0 + 5, x0:x0 + 5].flip(1, 2) for b, y0, x0 in where], dim=1)
        runs.append((x, dout, same_as_oracle(ref, oracle_wgrad(x, dout, (cout, cin, 5, 5)), kind)))
    return runs


@x_modes
@x_cases
@pytest.mark.parametrize("kind", ["one_hot_weight", "one_lit_pixel"])
def test_exact_fwd(W, B, layer, kind, mode):
    """Forward in both roles: a one-hot weight per output channel against a full-mantissa activation, and one lit pixel and channel per
    image (corner, edge, interior) against full-mantissa weights."""
    cout = geom(layer, W)[1]
    for i, (x, w, ref) in enumerate(exact_case(f"fwd_{kind}", W, B, layer)):
        got, _, _ = run_fwd(mode_handle(W, B, mode), B, layer, W, x, w, torch.zeros(cout))
        assert_exact(got, ref, f"{mode} fwd L{layer}, {kind}, run {i}")


@x_modes
@x_cases
@pytest.mark.parametrize("kind", ["one_hot_weight", "one_lit_pixel"])
def test_exact_dgrad(W, B, layer, kind, mode):
    """Input gradient: the same two constructions on the transposed operation."""
    for i, (dout, w, ref) in enumerate(exact_case(f"dgrad_{kind}", W, B, layer)):
        assert_exact(run_dgrad(mode_handle(W, B, mode), B, layer, W, dout, w), ref, f"{mode} dgrad L{layer}, {kind}, run {i}")


@x_modes
@x_cases
@pytest.mark.parametrize("kind", ["one_lit_dout_pixel", "one_lit_input_pixel"])
def test_exact_wgrad(W, B, layer, kind, mode):
    """Weight gradient: one lit dout pixel per output channel (in image co % B; corners, edges and interior among the positions) against a
    full-mantissa x, where D0's bias gradient is exactly 1; and the mirror image, one lit input pixel per input channel against a
    full-mantissa dout, where the bias gradient is a full sum and is held to the float64 sum at 1e-4 of its max."""
    cout = geom(layer, W)[1]
    for x, dout, ref in exact_case(f"wgrad_{kind}", W, B, layer):
        dw, db = run_wgrad(mode_handle(W, B, mode), B, layer, W, x, dout)
        assert_exact(dw, ref, f"{mode} wgrad L{layer}, {kind}")
        if db is not None and kind == "one_lit_dout_pixel":
            assert_exact(db, torch.ones(cout), f"{mode} dbias L{layer}")
        elif db is not None:
            check(db, f64(dout).sum(dim=(0, 2, 3)), f"{mode} dbias L{layer}", rel=True)
