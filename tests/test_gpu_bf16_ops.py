"""The conv kernels of bf16 mode, op by op.

On a "bf16" handle the per-op conv entry points run what the training step runs there (api.hip): conv5x5_bf16_big_kernel (E2..E4 forward and
input gradient), conv5x5_bf16_kernel<.., NS = 1, .., BF16_MT> (D0 at 128 x 128, D1..D3), conv4x4_row_bf16_kernel (D0 at 64 x 64, split-K plus
a finish launch), conv_bf16_ps.hip (D0 forward at 128 x 128), conv5x5_wgrad_tr_kernel, conv_up_wgrad_bf16_kernel, the bf16 forms of D4, and
pack_w_bf16_kernel with one split.  Activations and activation gradients are bf16 tensors, weights and their gradients fp32.

(a) EXACT.  Small-integer operands (bf16_ops_tools): every bf16 value, product and fp32 partial sum is exact in any order, every expected
    output is an integer the storage type holds, so the float64 convolution cast to the storage type is what the kernel must store and
    the comparison is equality.  Each case asserts those conditions on its reference before it touches the kernel.  Batches: 1, 3, 5, 9, 37
    at 64 x 64 (odd batches half-fill E3's two-image and E4's / D1's eight-image items; 5 and 9 open a second item with one image), D0
    also 33, 40 and 1029 (32-image groups; four against two K slices and the unsplit input gradient from 1024 on), D1..D3 also 17; 1, 3, 5
    and 37 at 128 x 128 (37 is there for the capped run of (d)).  Weight gradients also at the smallest batch at which a split walks two
    tiles and ends unevenly, from the mirror of the launchers' split arithmetic, which is held to the launchers' own plan
    (cvae_op_conv_wgrad_plan) on the device.  D0..D3's forward runs twice: with biases of [-2, 2], where the ReLU makes about half of
    the expected outputs zeros, and with every bias lifted by 64, where at least 90 % of the expected outputs are nonzero.
(b) The BatchNorm partials of E2..E4's forward (one row per 8 / 4 tiles) through op_bn_fwd_finalize with the queried tiles per row, held
    to ws_tools.bn_stats_ref's bounds on the exact integer y, widened per row by the three roundings of M2 = Q - S^2 / n in
    conv_bf16_big.hip's combine (one fp32 ulp of Q each); S and Q themselves are exact (below 2^24, asserted).  One more case per layer at
    |mean| / std of about 30 (bias 96, sparser operands): same bounds, and the variance within 1e-3 of its value.
(c) Full-mantissa plumbing: random bf16 activations and fp32 weights against float64 on the weights rounded to bf16 (D1..D3: the
    collapsed weights rounded), at the bars of check_bf16_stored_operands.  Only the packing's rounding, the bias row and the epilogue
    casts rest on this; the indexing rests on (a).
(d) A child pytest reruns the B = 37 cases of (a) and (b) with every persistent grid capped at 8 workgroups."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import bf16_ops_tools as T
from critic_vae_amd import lib as cvlib
from test_gpu_ops import rnd, wnat, wref
from ws_tools import ALL_ONES, U32, bn_stats_ref, poison, same_bits, within

pytestmark = pytest.mark.gpu
EPS = 1e-5
_handles = {}


def handle(W, B):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if (W, B) not in _handles:
        _handles[W, B] = cvlib.Handle(W, B, precision="bf16")
    return _handles[W, B]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def act_dev(t):
    """NCHW on the host -> bf16 NHWC on the device, as the fp32 tensor that holds it (two elements per float)."""
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda().view(-1).view(torch.float32)


def act_out(n):
    """n bf16 elements, every one a NaN."""
    return poison(torch.empty(n // 2, device="cuda"), ALL_ONES)


def act_host(buf, B, h, c):
    return buf.view(torch.bfloat16)[:B * h * h * c].view(B, h, h, c).permute(0, 3, 1, 2).double().cpu()


def f32_out(n):
    return torch.full((n,), float("nan"), device="cuda")


def f32_dev(t):
    return t.float().contiguous().cuda()


def scratch(H, B):
    return poison(torch.empty(H.op_scratch_floats(B), device="cuda"), ALL_ONES)


def run_fwd(H, layer, W, B, x, w, b):
    """-> (out NCHW float64 on the host, the BatchNorm partials of layers 1..3 or None)."""
    cin, cout, h, up, hs = T.geom(layer, W)
    out = act_out(B * h * h * cout)
    part = poison(torch.empty(H.op_bn_partial_floats(layer, B), device="cuda"), ALL_ONES) if layer < 4 else None
    H.op_conv_fwd(layer, B, act_dev(x), wnat(w.float()), f32_dev(b), out, part, scratch(H, B))
    torch.cuda.synchronize()
    return act_host(out, B, h, cout), part


def run_dgrad(H, layer, W, B, dout, w, mask):
    cin, cout, h, up, hs = T.geom(layer, W)
    din = act_out(B * hs * hs * cin)
    H.op_conv_dgrad(layer, B, act_dev(dout), wnat(w.float()), act_dev(mask) if mask is not None else None, din, scratch(H, B))
    torch.cuda.synchronize()
    return act_host(din, B, hs, cin)


def run_wgrad(H, layer, W, B, x, dout):
    cin, cout, h, up, hs = T.geom(layer, W)
    dw, db = f32_out(25 * cin * cout), f32_out(cout)
    H.op_conv_wgrad(layer, B, act_dev(x), act_dev(dout), dw, db, scratch(H, B))
    torch.cuda.synchronize()
    return wref(dw, cin, cout).double(), db.double().cpu()


def assert_equal(got, want, what):
    """Equality of every element (a NaN fails; the sign of a zero does not count)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = got != want
        err = (got - want).abs()[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.numel()} elements differ, largest |diff| {float(torch.nan_to_num(err, nan=float('inf')).max()):.6g}, "
                             f"first at {tuple(bad.nonzero()[0].tolist())}: got {float(got[bad][0])!r}, want {float(want[bad][0])!r}")


def stored(ref):
    """The float64 reference cast to bf16 storage (exact here: the cases assert it) and back."""
    return ref.to(torch.bfloat16).double()


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) exact
# ---------------------------------------------------------------------------------------------------------------------------------------
CAPPED_B = 37
BATCHES = {64: (1, 3, 5, 9, CAPPED_B), 128: (1, 3, 5)}
EXTRA = {(64, 4): (33, 40, 1029), (64, 5): (17,), (64, 6): (17,), (64, 7): (17,)}
# 128 x 128 at the capped batch: the passes on persistent grids (E2..E4 on the big-tile kernel, D0's forward on conv_bf16_ps.hip)
CAPPED_128 = [(128, CAPPED_B, layer, what) for layer in (1, 2, 3) for what in ("fwd", "dgrad")] + [(128, CAPPED_B, 4, "fwd")]


def a_cases(what):
    cases = [(W, B, layer) for W in (64, 128) for layer in range(1, 8) for B in BATCHES[W] + EXTRA.get((W, layer), ())]
    return cases + [(W, B, layer) for W, B, layer, p in CAPPED_128 if p == what]


def a_ids(cases):
    return [f"w{w}-b{b}-L{l}" for w, b, l in cases]


FWD_CASES, DGRAD_CASES, WGRAD_CASES = a_cases("fwd"), a_cases("dgrad"), a_cases("wgrad")


@pytest.mark.parametrize("W,B,layer", FWD_CASES, ids=a_ids(FWD_CASES))
def test_exact_fwd(W, B, layer):
    """Forward of E2..E4 (raw), D0 (ReLU) and D1..D3 (behind the upsample; bias + ReLU), bit for bit."""
    c = T.case_operands(layer, W, B, "fwd")
    T.assert_exact_conditions(c["pre"], f"fwd L{layer} pre-activation", T.max_terms(layer, W, B, "fwd"), True)
    got, _ = run_fwd(handle(W, B), layer, W, B, c["x"], c["w"], c["b"])
    assert_equal(got, stored(c["ref"]), f"fwd L{layer} at {W} x {W}, B = {B}")
    if 4 <= layer <= 7:       # the ReLU layers again with every bias lifted (bf16_ops_tools.RELU_LIFT): the expected OUTPUT is at least 90 % nonzero
        c = T.case_operands(layer, W, B, "fwd", lift=T.RELU_LIFT)
        T.assert_exact_conditions(c["ref"], f"fwd L{layer}, lifted bias", T.max_terms(layer, W, B, "fwd") + T.RELU_LIFT, True)
        got, _ = run_fwd(handle(W, B), layer, W, B, c["x"], c["w"], c["b"])
        assert_equal(got, stored(c["ref"]), f"fwd L{layer} at {W} x {W}, B = {B}, lifted bias")


@pytest.mark.parametrize("W,B,layer", DGRAD_CASES, ids=a_ids(DGRAD_CASES))
def test_exact_dgrad(W, B, layer):
    """Input gradient of E2..E4, D0 (at 64 x 64 through its split-K slabs; unsplit from B = 1024 on) and D1..D3 (2 x 2 sums and the
    ReLU mask of the producing layer), bit for bit."""
    c = T.case_operands(layer, W, B, "dgrad")
    T.assert_exact_conditions(c["ref"], f"dgrad L{layer}", T.max_terms(layer, W, B, "dgrad"), True)
    got = run_dgrad(handle(W, B), layer, W, B, c["dout"], c["w"], c["mask"])
    assert_equal(got, stored(c["ref"]), f"dgrad L{layer} at {W} x {W}, B = {B}")


def check_wgrad(W, B, layer):
    c = T.case_operands(layer, W, B, "wgrad")
    bound = T.max_terms(layer, W, B, "wgrad")
    T.assert_exact_conditions(c["ref_w"], f"wgrad L{layer}", bound, False)
    T.assert_exact_conditions(c["ref_b"], f"dbias L{layer}", bound, False)
    dw, db = run_wgrad(handle(W, B), layer, W, B, c["x"], c["dout"])
    assert_equal(dw, c["ref_w"], f"wgrad L{layer} at {W} x {W}, B = {B}")
    assert_equal(db, c["ref_b"], f"dbias L{layer} at {W} x {W}, B = {B}")


@pytest.mark.parametrize("W,B,layer", WGRAD_CASES, ids=a_ids(WGRAD_CASES))
def test_exact_wgrad(W, B, layer):
    """Weight and bias gradient of layers 1..7 on dense operands, bit for bit (fp32 outputs: integers below 2^24)."""
    check_wgrad(W, B, layer)


@pytest.mark.parametrize("layer", range(1, 8))
@pytest.mark.parametrize("W", [64, 128])
def test_exact_wgrad_two_tiles_per_split(W, layer):
    """The smallest batch at which a split of the weight-gradient kernel walks two tiles (tile mt + 1 fetched while tile mt computes) and
    the walk ends unevenly, on this device's compute-unit count."""
    B = T.wgrad_two_tile_batch(layer, W, cus())
    tiles, S, tps, imgs = T.wgrad_geometry(layer, W, B, cus())
    # the launcher's own arithmetic (cvae_op_conv_wgrad_plan), not only its mirror: at B the kernel's splits walk at least two tiles and end
    # unevenly, at B - 1 the mirror and the launcher still agree (the mirror picked the smallest such batch)
    plan = handle(W, B).op_conv_wgrad_plan(layer, B)
    assert plan == (tiles, S, tps), f"layer {layer} at {W} x {W}, B = {B}: the launcher plans {plan}, the mirror {(tiles, S, tps)}"
    assert handle(W, B).op_conv_wgrad_plan(layer, B - 1) == T.wgrad_geometry(layer, W, B - 1, cus())[:3]
    assert plan[2] >= 2 and (plan[0] % plan[2] or B % imgs), f"layer {layer} at {W} x {W}, B = {B}: {tiles} tiles on {S} splits"
    print(f"bf16ops-geometry wgrad w{W} L{layer}: B = {B}, {tiles} tiles, {S} splits, {tps} tiles per split ({cus()} CUs)")
    check_wgrad(W, B, layer)


@pytest.mark.parametrize("W", [64, 128])
def test_wgrad_geometry_mirror_is_the_launchers_arithmetic(W):
    """bf16_ops_tools.wgrad_geometry against cvae_op_conv_wgrad_plan (the split arithmetic of run_wgrad_bf16 / run_up_wgrad /
    run_up_wgrad_bf16_main themselves, no launch) at every batch up to 300 and at the large D0 batch, on this device's compute-unit count."""
    H = handle(W, 1)
    for layer in range(1, 8):
        for B in list(range(1, 301)) + [1029]:
            assert H.op_conv_wgrad_plan(layer, B) == T.wgrad_geometry(layer, W, B, cus())[:3], (layer, B)
    with pytest.raises(cvlib.CvaeError, match="bf16"):
        cvlib.Handle(W, 1).op_conv_wgrad_plan(1, 3)


@pytest.mark.parametrize("W,B", [(64, 1), (64, 3), (128, 3)])
def test_exact_e1_fwd_in_bf16_storage(W, B):
    """Layer 0 on a bf16 handle: fp32 frames in {0, 1/4, 1/2, 3/4, 1}, integer weights, y stored as bf16, bit for bit."""
    e = T.e1_operands(W, B)
    q = e["ref"] * 4
    assert bool((q == q.round()).all()) and float(q.abs().max()) <= T.EXACT_BF16 and float((q != 0).double().mean()) >= 0.9
    H = handle(W, B)
    out = act_out(B * W * W * 32)
    part = poison(torch.empty(H.op_bn_partial_floats(0, B), device="cuda"), ALL_ONES)
    H.op_conv_fwd(0, B, f32_dev(e["x"]), wnat(e["w"].float()), f32_dev(e["b"]), out, part, scratch(H, B))
    torch.cuda.synchronize()
    assert_equal(act_host(out, B, W, 32), stored(e["ref"]), f"E1 forward at {W} x {W}, B = {B}")
    assert bool(torch.isfinite(part).all()), "E1's BatchNorm partials were not all written"


@pytest.mark.parametrize("W,B", [(64, 1), (64, 5), (128, 3)])
def test_d4_fwd_on_exact_pre_activations(W, B):
    """D4's bf16 forward: the pre-activation is an exact multiple of 1/8 in [-2, 2]; recon against float64 tanh at test_d4_bwd's 1e-5."""
    f = T.d4_fwd_operands(W, B)
    p8 = f["pre"] * 8
    assert bool((p8 == p8.round()).all()) and float(f["pre"].abs().max()) <= 2.0 and float((f["pre"] != 0).double().mean()) >= 0.9
    H = handle(W, B)
    recon = f32_out(B * 3 * W * W)
    H.op_conv_fwd(8, B, act_dev(f["o3"]), wnat(f["w"].float()), f32_dev(f["b"]), recon, None, scratch(H, B))
    torch.cuda.synchronize()
    err = (recon.view(B, 3, W, W).double().cpu() - torch.tanh(f["pre"])).abs().max().item()
    print(f"bf16ops-ratio d4 fwd w{W} B{B}: max |recon - tanh| {err:.3e} of 1e-5")
    assert err <= 1e-5, f"D4 forward at {W} x {W}, B = {B}: max |recon - tanh(pre)| {err:.3e}"


@pytest.mark.parametrize("W,B", [(64, 2), (64, 5), (128, 3)])
def test_exact_d4_bwd(W, B):
    """D4's bf16 backward: dOut = d_recon (1 - recon^2) is an integer, so d_o3 (bf16), dW4 and db4 (fp32) are exact."""
    g = T.d4_bwd_operands(W, B)
    T.assert_exact_conditions(g["d_o3"], "d_o3", 3 * 25 * 8 * 4, True)
    T.assert_exact_conditions(g["dw"], "dW4", B * W * W * 16, False)
    T.assert_exact_conditions(g["db"], "db4", B * W * W * 8, False)
    H = handle(W, B)
    d_o3, dw, db = act_out(B * 32 * (W // 2) ** 2), f32_out(2400), f32_out(3)
    H.op_d4_bwd(B, act_dev(g["o3"]), f32_dev(g["d_recon"]), f32_dev(g["recon"]), wnat(g["w"].float()), None, d_o3, dw, db, scratch(H, B))
    torch.cuda.synchronize()
    assert_equal(act_host(d_o3, B, W // 2, 32), stored(g["d_o3"]), f"d_o3 at {W} x {W}, B = {B}")
    assert_equal(wref(dw, 32, 3).double(), g["dw"], f"dW4 at {W} x {W}, B = {B}")
    assert_equal(db.double().cpu(), g["db"], f"db4 at {W} x {W}, B = {B}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) the BatchNorm partials of the big-tile forward
# ---------------------------------------------------------------------------------------------------------------------------------------
BN_CASES = [(W, B, layer) for W in (64, 128) for layer in (1, 2, 3) for B in BATCHES[W]] + [(128, CAPPED_B, layer) for layer in (1, 2, 3)]
FAR_CASES = [(W, B, layer) for W, B in ((64, 9), (128, 3)) for layer in (1, 2, 3)]


def check_bn_partials(W, B, layer, c, tag, var_rel=None):
    cin, C, h, _, _ = T.geom(layer, W)
    H = handle(W, B)
    y = c["ref"]
    T.assert_exact_conditions(y, f"{tag} y", T.max_terms(layer, W, B, "fwd") + 96, True)
    tpp = H.op_conv_tiles_per_partial(layer, B)
    assert tpp == T.BIG_MT_NT[layer, False][0], f"E{layer + 1}'s forward is not on the big-tile kernel: {tpp} tiles per partial row"
    S, m2, cnt, Q = T.partial_rows(y, tpp)
    assert float(Q.max()) < T.EXACT_FP32 and float(S.abs().max()) < T.EXACT_FP32, f"{tag}: a row's S or Q is not exact in fp32"
    got, part = run_fwd(H, layer, W, B, c["x"], c["w"], c["b"])
    assert_equal(got, stored(y), f"{tag} y")
    rows = S.shape[0]
    assert_equal(part[:rows * C].view(rows, C).double().cpu(), S, f"{tag}: the partial sums")          # exact integers
    gamma, beta = rnd(f"bf16ops/g{layer}", (C,), 0.5, 1.5), rnd(f"bf16ops/be{layer}", (C,), -0.5, 0.5)
    rm0, rv0 = rnd(f"bf16ops/rm{layer}", (C,), -0.3, 0.3), rnd(f"bf16ops/rv{layer}", (C,), 0.5, 1.5)
    rm, rv, coef = rm0.clone().cuda(), rv0.clone().cuda(), f32_out(4 * C)
    H.op_bn_fwd_finalize(layer, B, part, tpp, gamma.cuda(), beta.cuda(), rm, rv, coef, scratch(H, B), True)
    torch.cuda.synchronize()
    coef = coef.view(C, 4).double().cpu()
    N = float(B * h * h)
    mu, var, mb, vb = bn_stats_ref(y.permute(0, 2, 3, 1), S, m2, cnt)
    vb = vb + T.combine_var_widening(Q, N)
    worst = {}
    within(f"{tag} mean", coef[:, 2], mu, mb, worst)
    istd = 1.0 / torch.sqrt(var + EPS)
    within(f"{tag} invstd", coef[:, 3], istd, istd * (0.5 * vb / (var + EPS) + 4 * U32), worst)
    want_rm = torch.tensor(0.9) * rm0 + torch.tensor(0.1) * coef[:, 2].float()
    assert same_bits(rm.cpu(), want_rm), f"{tag}: running_mean is not 0.9f * rm + 0.1f * mean in fp32"
    uvar = var * N / (N - 1)
    want_rv = 0.9 * rv0.double() + 0.1 * uvar
    within(f"{tag} running_var", rv.cpu(), want_rv, 0.1 * N / (N - 1) * vb + 3 * U32 * (0.9 * rv0.double().abs() + 0.1 * uvar), worst)
    if var_rel is not None:
        got_var = 1.0 / coef[:, 3] ** 2 - EPS
        within(f"{tag} variance to {var_rel:g} of its value", got_var, var, var_rel * var, worst)
        ratio = (mu.abs() / var.sqrt()).min().item()
        assert ratio > 20, f"{tag}: |mean| / std is only {ratio:.1f}"
    print(f"bf16ops-ratio (b) {tag}: " + ", ".join(f"{k.split(' ', 1)[1]} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("W,B,layer", BN_CASES, ids=a_ids(BN_CASES))
def test_bn_partials_of_the_big_tile_forward(W, B, layer):
    check_bn_partials(W, B, layer, T.case_operands(layer, W, B, "fwd"), f"w{W}-b{B}-L{layer}")


@pytest.mark.parametrize("W,B,layer", FAR_CASES, ids=a_ids(FAR_CASES))
def test_bn_partials_of_channels_far_from_zero(W, B, layer):
    """|mean| / std of about 30: bias 96 on a conv output of standard deviation about 3.  M2 = Q - S^2 / n cancels five digits there; the
    kernel takes it in double from exact S and Q, so the variance keeps the 1e-3 that test_batchnorm_statistics_of_channels_far_from_zero
    asks of the fp32 path."""
    c = T.case_operands(layer, W, B, "fwd", density=T.far_mean_density(layer), bias=96)
    check_bn_partials(W, B, layer, c, f"far w{W}-b{B}-L{layer}", var_rel=1e-3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) full-mantissa plumbing
# ---------------------------------------------------------------------------------------------------------------------------------------
C_B = 3
C_CASES = [(W, layer) for W in (64, 128) for layer in range(1, 8)]
c_ids = [f"w{w}-L{l}" for w, l in C_CASES]


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def close(got, want, what, rel):
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    print(f"bf16ops-ratio (c) {what}: err / allowed {err / (rel * scale):.3f}")
    assert err <= rel * scale, f"{what}: err {err:.3e} against {rel:.3e} of max {scale:.3e}"


def c_forward(layer, x, w, b):
    """float64 forward on the weights as the kernels hold them: rounded to bf16 (D1..D3: collapsed in fp32, then rounded)."""
    if T.LAYERS[layer][3]:
        y = T.up_conv_collapsed(x, bf(T.collapse_w(w.float())).double(), b)
    else:
        y = F.conv2d(x, bf(w.float()).double(), b, padding=2)
    return torch.relu(y) if 4 <= layer <= 7 else y


@pytest.mark.parametrize("W,layer", C_CASES, ids=c_ids)
def test_full_mantissa_fwd_and_dgrad(W, layer):
    cin, cout, h, up, hs = T.geom(layer, W)
    B, bar = C_B, 2.0 ** -6 if up else 2.0 ** -8
    H = handle(W, B)
    w, b = rnd(f"w{layer}", (cout, cin, 5, 5), -0.1, 0.1).double(), rnd(f"b{layer}", (cout,)).double()
    x = bf(rnd(f"x{layer}", (B, cin, hs, hs))).double()
    if up:
        x = torch.relu(x)
    got, _ = run_fwd(H, layer, W, B, x, w, b)
    close(got, c_forward(layer, x, w, b), f"fwd w{W} L{layer}", bar)
    dout = bf(rnd(f"do{layer}", (B, cout, h, h))).double()
    pre = bf(rnd(f"pre{layer}", (B, cin, hs, hs))).double().requires_grad_(True)
    src = torch.relu(pre) if up else pre
    (T.up_conv_collapsed(src, bf(T.collapse_w(w.float())).double(), None) if up else F.conv2d(src, bf(w.float()).double(), None, padding=2)).backward(dout)
    got = run_dgrad(H, layer, W, B, dout, w, src.detach() if up else None)
    close(got, pre.grad, f"dgrad w{W} L{layer}", bar)


@pytest.mark.parametrize("W,layer", C_CASES, ids=c_ids)
def test_full_mantissa_wgrad(W, layer):
    cin, cout, h, up, hs = T.geom(layer, W)
    B = C_B
    x, dout = bf(rnd(f"x{layer}", (B, cin, hs, hs))).double(), bf(rnd(f"do{layer}", (B, cout, h, h))).double()
    ref_w, ref_b = T.conv_wgrad_ref(layer, x, dout)
    dw, db = run_wgrad(handle(W, B), layer, W, B, x, dout)
    close(dw, ref_w, f"wgrad w{W} L{layer}", 2e-3)
    close(db, ref_b, f"dbias w{W} L{layer}", 2e-3)


@pytest.mark.parametrize("W", [64, 128])
def test_full_mantissa_d4(W):
    """D4 forward and backward on real values: recon at 2^-6 of its max against the 5 x 5 weights rounded to bf16 (the bar of "recon vs 5x5
    weights"), d_o3 at 2^-6, dW4 at 1e-2 and db4 at 1e-4 of their max (check_bf16_stored_operands)."""
    B = C_B
    H = handle(W, B)
    w, b = rnd("w8", (3, 32, 5, 5), -0.1, 0.1).double(), rnd("b8", (3,)).double()
    o3 = torch.relu(bf(rnd("pre8", (B, 32, W // 2, W // 2)))).double()
    recon = f32_out(B * 3 * W * W)
    H.op_conv_fwd(8, B, act_dev(o3), wnat(w.float()), f32_dev(b), recon, None, scratch(H, B))
    torch.cuda.synchronize()
    recon = recon.view(B, 3, W, W).cpu()
    close(recon.double(), torch.tanh(F.conv2d(T.up2(o3), bf(w.float()).double(), b, padding=2)), f"d4 fwd w{W}", 2.0 ** -6)
    d_recon = rnd("dr8", (B, 3, W, W))
    dout = (d_recon * (1.0 - recon ** 2)).double()
    d_o3, dw, db = act_out(B * 32 * (W // 2) ** 2), f32_out(2400), f32_out(3)
    H.op_d4_bwd(B, act_dev(o3), f32_dev(d_recon), f32_dev(recon), wnat(w.float()), None, d_o3, dw, db, scratch(H, B))
    torch.cuda.synchronize()
    want = torch.where(o3 > 0, F.avg_pool2d(F.conv_transpose2d(dout, bf(w.float()).double(), padding=2), 2) * 4.0, torch.zeros((), dtype=torch.float64))
    close(act_host(d_o3, B, W // 2, 32), want, f"d4 d_o3 w{W}", 2.0 ** -6)
    ref_w, ref_b = T.conv_wgrad_ref(8, o3, dout)
    close(wref(dw, 32, 3).double(), ref_w, f"d4 dW w{W}", 1e-2)
    close(db.double().cpu(), ref_b, f"d4 db w{W}", 1e-4)


def test_bf16_conv_ops_reject_a_null_scratch():
    """The packed (and collapsed) weights live in the scratch: without one the ops fail before any launch."""
    W, B = 64, 1
    H = handle(W, B)
    for layer in (3, 6):
        cin, cout, h, up, hs = T.geom(layer, W)
        x, w, dout = act_out(B * hs * hs * cin), torch.zeros(25 * cin * cout, device="cuda"), act_out(B * h * h * cout)
        with pytest.raises(cvlib.CvaeError, match="scratch"):
            H.op_conv_fwd(layer, B, x, w, torch.zeros(cout, device="cuda"), act_out(B * h * h * cout), None, None)
        with pytest.raises(cvlib.CvaeError, match="scratch"):
            H.op_conv_dgrad(layer, B, dout, w, x, act_out(B * hs * hs * cin), None)
        with pytest.raises(cvlib.CvaeError, match="scratch"):
            H.op_conv_wgrad(layer, B, x, dout, torch.empty_like(w), None, None)
    assert H.op_scratch_floats(B) > cvlib.Handle(W, B).op_scratch_floats(B)
    with pytest.raises(cvlib.CvaeError, match="tiles per partial"):
        H.op_bn_fwd_finalize(1, B, torch.zeros(128, device="cuda"), 3, *(torch.zeros(256, device="cuda") for _ in range(5)), scratch(H, B), True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (d) several items per workgroup
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_exact_cases_walk_several_items_under_a_grid_cap():
    """A child process caps every persistent grid at 8 workgroups (CVAE_PERSIST_MAXWG, read once per process) and reruns the B = 37 cases of
    (a) and (b) at both frame sizes: the big-tile kernels' next-item prefetch, their carried slab buffers and the BatchNorm rows of
    several items per workgroup then run with ragged ends (E4 forward at 64 x 64: five items of four tiles, the last with three, on two
    channel blocks; E2 forward at 128 x 128: 148 items on two channel halves)."""
    for W, layer in ((64, 3), (128, 1)):
        tiles, groups, mt, ny, grid = T.big_geometry(layer, W, False, CAPPED_B, cus(), maxwg=8)
        assert grid == 8 and groups * ny > grid, f"E{layer + 1} forward at {W} x {W}: {groups} x {ny} items on {grid} workgroups"
    want = sum(1 for cases in (FWD_CASES, DGRAD_CASES, WGRAD_CASES, BN_CASES) for _, B, _ in cases if B == CAPPED_B)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVAE_PERSIST_MAXWG="8")
    sel = f"(test_exact_fwd or test_exact_dgrad or test_exact_wgrad or test_bn_partials_of_the_big_tile_forward) and -b{CAPPED_B}- and not two_tiles"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert re.search(rf"\b{want} passed\b", p.stdout) and "failed" not in p.stdout, p.stdout[-1000:]
