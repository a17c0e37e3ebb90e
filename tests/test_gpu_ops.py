"""GPU parity: every HIP kernel, through the C-ABI, against the oracle's single-op references.

Tolerance: north_star asks 1e-4 fp32 on outputs; gradients of tensors whose magnitude is far
from 1 are additionally checked relative to the tensor's max.  The conv,
BatchNorm / pool and D4 references are evaluated in float64 on the same fp32 inputs, at both
frame sizes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth
from oracle import cvae_oracle as orc
from ws_tools import ALL_ONES, poison

pytestmark = pytest.mark.gpu
TOL = 1e-4
# (cin, cout, h_out at 64 x 64 frames, up)  — vae_nets.py:69-84, 117-133; every spatial size doubles at 128 x 128
LAYERS = [(3, 32, 64, 0), (32, 64, 32, 0), (64, 128, 16, 0), (128, 256, 8, 0),
          (256, 128, 4, 0), (128, 64, 8, 1), (64, 32, 16, 1), (32, 32, 32, 1), (32, 3, 64, 1)]
# (width, batch) of the conv tests.  3, 8: small ragged batches.  37: the capped child process below reruns these with the persistent grids
# cut to 8 workgroups.  601 / 67: LOOP_BATCHES, where the persistent conv passes walk several items per workgroup at the production grid
# (at 64 x 64: E2 forward 10 items on the busiest workgroup, E3 forward 5, E3 input gradient and E4 forward 3, E4 input gradient 2;
# odd: half-filled 2-image tiles at E4 and 8-image groups at D0;  at 128 x 128: E2 forward 5, E3 forward 3, E3 input gradient 2)
LOOP_BATCHES = {64: 601, 128: 67}
CAPPED_B = 37
SHAPES = [(64, 3), (64, 8), (64, CAPPED_B), (64, 601), (128, 3), (128, CAPPED_B), (128, 67)]


def shape_id(W, B):
    return str(B) if W == 64 and B < 10 else f"w{W}-b{B}"        # the small 64 x 64 batches keep the ids they had before the width axis


def shapes(cases=SHAPES):
    return pytest.mark.parametrize("W,B", cases, ids=[shape_id(w, b) for w, b in cases])


_handles = {}


def handle(W, B):
    """One library handle per (width, batch)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if (W, B) not in _handles:
        _handles[W, B] = cvlib.Handle(W, B)
    return _handles[W, B]


@pytest.fixture(scope="module")
def H():
    return handle(64, 64)


def geom(layer, W):
    cin, cout, h, up = LAYERS[layer]
    h = h * W // 64
    return cin, cout, h, up, (h // 2 if up else h)


def persistent_items(layer, W, dgrad, B):
    """Items of the fp32 persistent conv launcher (run_mfma_ps, conv_mfma_ps.hip) for E2..E4 pass (layer, dgrad): 128-pixel tiles of
    Tile<h> (conv_mfma.hip / common.h), rounded up to the 8 XCD lanes, times the 64-channel blocks of the output."""
    cin, cout, h, _, _ = geom(layer, W)
    tw = min(h, 32)
    th = min(128 // tw, h)
    tiles = -(-B // (128 // (tw * th))) * (h // tw) * (h // th)
    return -(-tiles // 8) * 8 * ((cin if dgrad else cout) // 64)


def assert_items_loop(layer, W, dgrad, B):
    """At LOOP_BATCHES, a pass on the two-workgroup persistent kernel must have more items than its grid (2 per CU, a multiple of 8):
    otherwise this device's CU count has turned the case back into one item per workgroup."""
    if B != LOOP_BATCHES[W] or not 1 <= layer <= 3 or cvlib.load().cvae_conv_route(0, W, layer, int(dgrad), B) != 1:
        return
    G = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    G -= G % 8
    n = persistent_items(layer, W, dgrad, B)
    assert n > G, f"layer {layer} {'dgrad' if dgrad else 'fwd'} at {W} x {W}, B={B}: {n} items on a grid of {G}: one item per workgroup"


def f64(t):
    return t.detach().double()


def dev(t):
    return t.contiguous().cuda()


def nhwc(t):       # NCHW cpu -> NHWC gpu
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def to_nchw(t, B, h, c):
    return t.view(B, h, h, c).permute(0, 3, 1, 2).cpu()


def wnat(w):       # OIHW -> [25][I][O]
    return w.permute(2, 3, 1, 0).reshape(25, w.shape[1], w.shape[0]).contiguous().cuda()


def wref(n, cin, cout):
    return n.view(5, 5, cin, cout).permute(3, 2, 0, 1).cpu()


def rnd(name, shape, lo=-1.0, hi=1.0, seed=7):
    return torch.from_numpy(synth.uniform(seed, name, shape, lo, hi))


def check(got, want, what, tol=TOL, rel=False):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs().max().item()
    scale = want.abs().max().item() if rel else 1.0
    assert np.isfinite(err) and err <= tol * max(scale, 1e-30), f"{what}: max|err|={err:.3e} scale={scale:.3e}"


@pytest.mark.parametrize("layer", range(9))
@shapes()
def test_conv_fwd(W, B, layer):
    H = handle(W, B)
    cin, cout, h, up, hs = geom(layer, W)
    assert_items_loop(layer, W, False, B)
    x = rnd(f"x{layer}", (B, cin, hs, hs))
    w = rnd(f"w{layer}", (cout, cin, 5, 5), -0.1, 0.1)
    b = rnd(f"b{layer}", (cout,))
    ref = orc.conv5x5(f64(x), f64(w), f64(b), upsample_input=bool(up))
    if 4 <= layer <= 7:
        ref = torch.relu(ref)
    if layer == 8:
        ref = torch.tanh(ref)
    xin = dev(x) if layer == 0 else nhwc(x)
    out = torch.full((B * h * h * cout,), float("nan"), device="cuda")
    # the BatchNorm partials come back fully written: uninitialised memory, filled with NaNs (ws_tools.ALL_ONES)
    part = poison(torch.empty(max(H.op_bn_partial_floats(min(layer, 3), B), 1), device="cuda"), ALL_ONES) if layer < 4 else None
    H.op_conv_fwd(layer, B, xin, wnat(w), dev(b), out, part, torch.empty(H.op_scratch_floats(B), device="cuda"))
    torch.cuda.synchronize()
    got = out.view(B, cout, h, h).cpu() if layer == 8 else to_nchw(out, B, h, cout)
    check(got, ref, f"conv_fwd L{layer}")


@pytest.mark.parametrize("B", [37, 64])
def test_conv_fwd_d0_image_major_tiles(H, B):
    """D0 (4x4 images) runs on conv4x4_row_kernel: M tiles of 32 IMAGES x two image rows that skip the zero padding, split-K
    over channel chunks.  Batches that end inside a 32-image group (the cases above stay inside the first one)."""
    cin, cout, h, _ = LAYERS[4]
    x = rnd("x4r", (B, cin, h, h))
    w = rnd("w4r", (cout, cin, 5, 5), -0.1, 0.1)
    b = rnd("b4r", (cout,))
    ref = torch.relu(orc.conv5x5(f64(x), f64(w), f64(b), upsample_input=False))
    out = torch.full((B * h * h * cout,), float("nan"), device="cuda")
    H.op_conv_fwd(4, B, nhwc(x), wnat(w), dev(b), out, None, torch.empty(H.op_scratch_floats(B), device="cuda"))
    torch.cuda.synchronize()
    check(to_nchw(out, B, h, cout), ref, "conv_fwd L4 (ragged image groups)")


# (64, 33), (128, 9): conv-emitted partials past the 32 chunks of bn_fwd_reduce and partial rows past the 64 of launch_col_reduce_partial
BN_CASES = [(W, B, ties) for W in (64, 128) for B, ties in [(3, False), (8, True), (5, "tiny_gamma")]] + [(64, 33, False), (128, 9, False)]


@pytest.mark.parametrize("layer", range(4))
@pytest.mark.parametrize("W,B,ties", BN_CASES, ids=[f"{shape_id(W, B)}-{t}" for W, B, t in BN_CASES])
def test_bn_pool_act_fwd_bwd(W, layer, B, ties):
    """ties=True: exact max-pool ties + negative gamma.  "tiny_gamma": channels with gamma = 0 / 3e-3 / -5e-3 —
    the ReLU blocks' pooled-tensor shortcut xhat = (a - beta)/gamma is ill-conditioned there and the kernel
    must fall back to y (dgamma of a zero-gamma channel is sum(g*xhat), not 0)."""
    H = handle(W, B)
    tiny = ties == "tiny_gamma"
    ties = ties is True
    cin, C, h, _, _ = geom(layer, W)
    act = "tanh" if layer == 3 else "relu"
    x = rnd(f"bx{layer}", (B, cin, h, h))
    w = rnd(f"bw{layer}", (C, cin, 5, 5), -0.1, 0.1)
    b = rnd(f"bb{layer}", (C,))
    if ties:       # y = x[co % cin] exactly, x on a coarse grid -> many EXACT ties inside pooling windows
        x = torch.round(x * 2) / 2
        w = torch.zeros_like(w)
        w[torch.arange(C), torch.arange(C) % cin, 2, 2] = 1.0
        b = torch.zeros_like(b)
    gamma = rnd(f"g{layer}", (C,), 0.5, 1.5)
    beta = rnd(f"be{layer}", (C,), -0.5, 0.5)
    if ties:
        gamma[::3] *= -1            # negative scale flips which element is the maximum
    if tiny:
        gamma[0], gamma[5], gamma[9] = 0.0, 3e-3, -5e-3
        beta[0], beta[5], beta[9] = 0.3, 0.5, 0.2          # ReLU lets these channels through
    # conv on the GPU provides y and the BatchNorm partials; the reference starts from that same fp32 y
    y = torch.empty(B * h * h * C, device="cuda")
    part = poison(torch.empty(H.op_bn_partial_floats(layer, B), device="cuda"), ALL_ONES)
    H.op_conv_fwd(layer, B, dev(x) if layer == 0 else nhwc(x), wnat(w), dev(b), y, part)
    y_ref = f64(to_nchw(y, B, h, C)).requires_grad_(True)
    g_ref, b_ref = f64(gamma).requires_grad_(True), f64(beta).requires_grad_(True)
    a_ref, mean, var = orc.bn_pool_act(y_ref, g_ref, b_ref, act)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    coef = torch.empty(C * 4, device="cuda")
    a = torch.empty(B * (h // 2) ** 2 * C, device="cuda")
    sc = torch.empty(H.op_scratch_floats(B), device="cuda")
    H.op_bn_pool_act_fwd(layer, B, y, part, dev(gamma), dev(beta), rm, rv, coef, a, sc, True)
    torch.cuda.synchronize()
    check(coef.view(C, 4)[:, 2], mean, "bn mean", 1e-5)
    check(1.0 / coef.view(C, 4)[:, 3].double() ** 2 - 1e-5, var, "bn var", 1e-5, rel=True)
    check(to_nchw(a, B, h // 2, C), a_ref, f"bn_pool_act fwd L{layer}")
    n = B * h * h
    check(rm, 0.1 * mean, "running_mean", 1e-5)
    check(rv, 0.9 + 0.1 * var * n / (n - 1), "running_var", 1e-5)
    # backward
    da = rnd(f"da{layer}", (B, C, h // 2, h // 2))
    a_ref.backward(f64(da))
    dy = torch.empty_like(y)
    dg, db, dbias = (torch.empty(C, device="cuda") for _ in range(3))
    sc = torch.empty(H.op_scratch_floats(B), device="cuda")
    H.op_bn_pool_act_bwd(layer, B, y, a, nhwc(da), coef, dev(gamma), dy, dg, db, dbias, sc)
    torch.cuda.synchronize()
    check(to_nchw(dy, B, h, C), y_ref.grad, f"bn_pool_act bwd dy L{layer}", rel=True)
    check(dg, g_ref.grad, "dgamma", rel=True)
    check(db, b_ref.grad, "dbeta", rel=True)
    # the conv bias feeds a train-mode BatchNorm: its true gradient is 0 and both sides hold pure
    # summation round-off, so compare against the size of the summed terms
    noise = 2e-6 * y_ref.grad.abs().sum(dim=(0, 2, 3)).max().item()
    check(dbias, y_ref.grad.sum(dim=(0, 2, 3)), "dbias (round-off level)", max(noise, 1e-9))


@pytest.mark.parametrize("layer", range(1, 8))
@shapes()
def test_conv_dgrad(W, B, layer):
    """Layer 4 (D0) at 64 x 64 runs the training step's split-K kernel (the scratch holds its partial slabs)."""
    H = handle(W, B)
    cin, cout, h, up, hs = geom(layer, W)
    assert_items_loop(layer, W, True, B)
    w = rnd(f"w{layer}", (cout, cin, 5, 5), -0.1, 0.1)
    dout = rnd(f"do{layer}", (B, cout, h, h))
    pre = f64(rnd(f"pre{layer}", (B, cin, hs, hs))).requires_grad_(True)
    src = torch.relu(pre) if up else pre
    orc.conv5x5(src, f64(w), None, upsample_input=bool(up)).backward(f64(dout))
    din = torch.full((B * hs * hs * cin,), float("nan"), device="cuda")
    sc = torch.empty(H.op_scratch_floats(B), device="cuda")
    H.op_conv_dgrad(layer, B, nhwc(dout), wnat(w), nhwc(src.detach().float()) if up else None, din, sc)
    torch.cuda.synchronize()
    check(to_nchw(din, B, hs, cin), pre.grad, f"conv_dgrad L{layer}", rel=True)


@pytest.mark.parametrize("layer", range(8))
@shapes()
def test_conv_wgrad(W, B, layer):
    H = handle(W, B)
    cin, cout, h, up, hs = geom(layer, W)
    x = rnd(f"x{layer}", (B, cin, hs, hs))
    w = f64(rnd(f"w{layer}", (cout, cin, 5, 5), -0.1, 0.1)).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    dout = rnd(f"do{layer}", (B, cout, h, h))
    orc.conv5x5(f64(x), w, b, upsample_input=bool(up)).backward(f64(dout))
    dw = torch.full((25 * cin * cout,), float("nan"), device="cuda")
    dbias = torch.empty(cout, device="cuda") if layer >= 4 else None
    sc = torch.empty(H.op_scratch_floats(B), device="cuda")
    H.op_conv_wgrad(layer, B, dev(x) if layer == 0 else nhwc(x), nhwc(dout), dw, dbias, sc)
    torch.cuda.synchronize()
    check(wref(dw, cin, cout), w.grad, f"conv_wgrad L{layer}", rel=True)
    if dbias is not None:
        check(dbias, b.grad, f"conv dbias L{layer}", rel=True)


@shapes([(64, 2), (64, 5), (64, 601), (128, 2), (128, 5), (128, 67)])
def test_d4_bwd(W, B):
    H = handle(W, B)
    w = f64(rnd("w8", (3, 32, 5, 5), -0.1, 0.1)).requires_grad_(True)
    b = f64(rnd("b8", (3,))).requires_grad_(True)
    pre = f64(rnd("pre8", (B, 32, W // 2, W // 2))).requires_grad_(True)
    o3 = torch.relu(pre)
    recon = torch.tanh(orc.conv5x5(o3, w, b, upsample_input=True))
    d_recon = rnd("dr8", (B, 3, W, W))
    recon.backward(f64(d_recon))
    recon32 = recon.detach().float()
    dout = torch.empty(B * 3 * W * W, device="cuda")
    d_o3 = torch.full((B * 32 * (W // 2) ** 2,), float("nan"), device="cuda")
    dw = torch.empty(2400, device="cuda")
    db = torch.empty(3, device="cuda")
    sc = torch.empty(H.op_scratch_floats(B), device="cuda")
    H.op_d4_bwd(B, nhwc(o3.detach().float()), dev(d_recon), dev(recon32), wnat(w.detach().float()), dout, d_o3, dw, db, sc)
    torch.cuda.synchronize()
    check(dout.view(B, 3, W, W), f64(d_recon) * (1 - f64(recon32) ** 2), "d4 tanh bwd", 1e-5)
    check(to_nchw(d_o3, B, W // 2, 32), pre.grad, "d4 dgrad", rel=True)
    check(wref(dw, 32, 3), w.grad, "d4 wgrad", rel=True)
    check(db, b.grad, "d4 dbias", rel=True)


def test_persistent_conv_kernels_walk_several_items_under_a_grid_cap():
    """The persistent conv launchers (conv_mfma_ps.hip, conv_bf16_ps.hip, conv_bf16_big.hip) size their grid by the CU count: at the test
    batches above (but LOOP_BATCHES) every item gets its own workgroup, and at the production grid (2 per CU: 512 = 64 per XCD lane) a
    workgroup keeps its channel block from item to item.  A child process caps every persistent grid at 8 workgroups (CVAE_PERSIST_MAXWG,
    read once per process) and reruns the conv tests of this file at B = 37: each XCD lane then walks several tiles AND channel blocks
    (at 64 x 64: E4 forward 19 tiles x 4 blocks, E3 forward 74 x 2; at 128 x 128: E3 forward 296 x 2, E3 input gradient 296, E2 forward 1184),
    so the next item's operand loads run with a new tile origin and a new n0, ending unevenly."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVAE_PERSIST_MAXWG="8")
    sel = f"(test_conv_fwd or test_conv_dgrad or test_conv_wgrad) and (w64-b{CAPPED_B} or w128-b{CAPPED_B})"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert re.search(r"\b48 passed\b", r.stdout) and "failed" not in r.stdout, r.stdout[-1000:]


def _ms_inputs(tag):
    b = torch.from_numpy(synth.uniform(5, f"ms/{tag}/b", (4, 3, 64, 64)))
    if tag == "nan":
        a = 0.5 - b + 0.01 * torch.from_numpy(synth.uniform(5, f"ms/{tag}/a", (4, 3, 64, 64)))
    else:
        a = torch.from_numpy(synth.uniform(5, f"ms/{tag}/a", (4, 3, 64, 64), -1.0 if tag == "neg" else 0.0, 1.0))
    return a.clone(), b


@pytest.mark.parametrize("tag", ["pos", "neg", "nan"])
def test_msssim(H, golden_dir, tag):
    import os
    fx = np.load(os.path.join(golden_dir, "msssim_ops.npz"))
    a, b = _ms_inputs(tag)
    a_ref = a.clone().requires_grad_(True)
    loss, sims, css = orc.msssim(a_ref, b)
    ws = torch.empty(H.op_msssim_ws_floats(4), device="cuda")
    scal = torch.empty(16, device="cuda")
    d_a = torch.empty(4 * 3 * 64 * 64, device="cuda")
    H.op_msssim(4, dev(a), dev(b), ws, scal, d_a)
    torch.cuda.synchronize()
    s = scal.cpu()
    check(s[3:8], sims, "ssim levels", 2e-5)
    check(s[8:13], css, "cs levels", 2e-5)
    check(s[3:8], torch.from_numpy(fx[f"{tag}/ssim"]), "ssim levels vs reference fixture", 2e-5)
    check(s[8:13], torch.from_numpy(fx[f"{tag}/cs"]), "cs levels vs reference fixture", 2e-5)
    if tag == "nan":
        assert torch.isnan(s[1]) and torch.isnan(loss) and np.isnan(fx["nan/loss"])    # NaN propagates, no clamp
        return
    check(s[1], loss, "msssim loss", 2e-5)
    assert abs(s[1].item() - float(fx[f"{tag}/loss"])) < 2e-5
    assert s[2].item() == 0.0 and abs(s[0].item() - s[1].item()) < 1e-7
    loss.backward()
    check(d_a.view(4, 3, 64, 64), a_ref.grad, "msssim grad", rel=True)


@pytest.mark.parametrize("B", [3, 90])          # 90: 270 planes on 256 persistent workgroups (some walk two planes)
def test_msssim_128_wide_streamed_level_against_oracle(B):
    """Round 4: level 0 of 128x128 frames runs on msssim_stream_kernel (the plane streamed through LDS in 16-row bands,
    msssim.hip).  Loss, the five ssim / cs levels and every element of the gradient against the oracle's MSSIM
    (vae_nets.py:181-247 restated) on frames with structure (a smooth image against a noisy copy: all levels positive)."""
    h = cvlib.Handle(128, B)
    g = torch.Generator().manual_seed(100 + B)
    b = torch.rand(B, 3, 128, 128, generator=g)
    a = (0.7 * b + 0.3 * torch.rand(B, 3, 128, 128, generator=g)).clone()
    a_ref = a.clone().requires_grad_(True)
    loss, sims, css = orc.msssim(a_ref, b)
    assert torch.isfinite(loss)
    ws = torch.empty(h.op_msssim_ws_floats(B), device="cuda")
    scal = torch.empty(16, device="cuda")
    d_a = torch.empty(B * 3 * 128 * 128, device="cuda")
    h.op_msssim(B, dev(a), dev(b), ws, scal, d_a)
    torch.cuda.synchronize()
    s = scal.cpu()
    check(s[3:8], sims, "ssim levels", 2e-5)
    check(s[8:13], css, "cs levels", 2e-5)
    check(s[1], loss, "msssim loss", 2e-5)
    loss.backward()
    check(d_a.view(B, 3, 128, 128), a_ref.grad, "msssim grad", rel=True)


def test_adam_matches_torch(H):
    n = 4096
    p0, g = rnd("ap", (n,)), rnd("ag", (n,), -1e-2, 1e-2)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=5e-5)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 6):
        gs = g * step
        p_ref.grad = gs.clone()
        opt.step()
        H.adam_step(p, dev(gs * 2.0), m, v, step, 5e-5, grad_scale=0.5)
    torch.cuda.synchronize()
    check(p, p_ref, "adam params", 1e-7)


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_critic_forward_and_preprocess(H, golden_dir, scale):
    """cvae_critic_forward / cvae_preprocess_u8 vs the oracle (and the reference-generated fixture)."""
    import os
    from critic_vae_amd.critic import Critic
    fx = np.load(os.path.join(golden_dir, "critic_b8.npz"))
    cp = {k: torch.from_numpy(v) * scale for k, v in synth.make_critic_params(int(fx["wseed"])).items()}
    x, _, _ = synth.make_batch(int(fx["dseed"]), int(fx["step"]), int(fx["batch"]))
    x = torch.from_numpy(x)
    want = orc.critic_forward(cp, x)
    crit = Critic(handle=H).cuda()
    crit.load_state_dict(cp)
    got = crit.evaluate(x.cuda())
    torch.cuda.synchronize()
    check(got, want, "critic pred", 2e-6)
    if scale == 1.0:
        check(got, torch.from_numpy(fx["pred"]), "critic pred vs reference fixture", 2e-6)
    else:
        assert want.std().item() > 1e-3          # the scaled weights really exercise the network
    sd = crit.state_dict()
    assert all(torch.equal(sd[k].cpu(), cp[k]) for k in cp)
    u8 = torch.from_numpy(fx["u8"])
    pre = crit.preprocess(u8.cuda())
    torch.cuda.synchronize()
    assert torch.equal(pre.cpu(), orc.preprocess_frames(u8))
    if scale == 1.0:        # the reference's REAL checkpoint: weights + predictions of its own Critic.evaluate
        fr = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
        crit.load_state_dict({k[2:]: torch.from_numpy(fr[k]) for k in fr.files if k.startswith("w/")})
        got = crit.evaluate(x.cuda())
        torch.cuda.synchronize()
        check(got, torch.from_numpy(fr["pred"]), "critic pred, real checkpoint vs reference fixture", 2e-6)
