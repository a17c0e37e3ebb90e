"""The fp32 (precision 0) conv kernels, op by op, on exact operands: the fp32 counterpart of parts (a) and (d) of test_gpu_bf16_ops.py.

On an "f32" handle the per-op entry points run e1_fwd_kernel / e1_wgrad_kernel and the D4 forward / fused backward (conv_thin.hip), the
per-tile and persistent 5 x 5 kernels of E2..E4 and D0 (conv_mfma.hip, conv_mfma_ps.hip; D0 at 64 x 64 on conv4x4_row_kernel with split-K
slabs in both directions), conv5x5_wgrad_kernel (conv_wgrad.hip) and the phase-collapsed D1..D3 (conv_up.hip: collapse_w_kernel, the
split-K slabs of D1 / D2, conv_up_wgrad_kernel's split walk over UpTile64 tiles, expand_dw_kernel).  All tensors are fp32; activations NHWC,
x and recon NCHW.  Outputs, scratch and BatchNorm partials are handed in poisoned (ws_tools.ALL_ONES: NaNs).

Operands are bf16_ops_tools' small integers (E1: quarters; D4 forward: eighths): every product and every fp32 partial sum below 2^24 is
exact in ANY order, so the float64 reference is what a correct kernel must store bit for bit and every comparison is torch.equal, except
the D4 forward's tanh (see test_d4_fwd).  Each case asserts the exactness conditions on its reference before it touches the kernel.
test_gpu_ops.py's random operands keep holding the rounding behaviour at 1e-4; the indexing rests on this file.

Batches, each the smallest at which a kernel's geometry changes (Tile<h>: two images per tile at h = 8, eight at h = 4; UpTile64<4>: four):
  every layer     1, 3, 5, 9, 37 at 64 x 64 and 1, 3, 5 at 128 x 128: image groups half full, a second / fifth group holding one image
  D1..D3          also 17 at 64 x 64: a third UpTile<4> tile holding one image
  D0, 64 x 64     forward and input gradient also 33 and 40: the 32-image groups of conv4x4_row_kernel, ragged.  D0's fp32 input gradient
                  has NO batch at which it leaves split-K: launch_conv_dgrad (conv_mfma.hip) takes the four-slab form at 64 x 64 whenever it
                  is given scratch, which the per-op entry and the training step always do (the bf16 launcher leaves it at 1024)
  E2..E4          forward and input gradient also (128, 37), for the capped run below
  weight gradients, every (width, layer 0..8): the smallest batch at which a split walks at least two tiles and the walk ends unevenly,
                  from f32_ops_tools' mirror at this device's compute-unit count, held to the launchers' own arithmetic
                  (cvae_op_conv_wgrad_plan_f32); one "f32ops-geometry" line each
A child pytest reruns the B = 37 forward / input-gradient cases of E2..E4 at both sizes and the D4 forward at (64, 37) with every
persistent grid capped at 8 workgroups (CVAE_PERSIST_MAXWG): several tiles and channel blocks per workgroup in conv_mfma_ps.hip, 37 tiles
per workgroup in d4_fwd_pc_f32_kernel."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch

import bf16_ops_tools as T
import f32_ops_tools as F32
from critic_vae_amd import lib as cvlib
from test_gpu_bf16_ops import assert_equal
from test_gpu_ops import TOL, dev, nhwc, rnd, to_nchw, wnat, wref
from ws_tools import ALL_ONES, U32, bn_stats_ref, poison, synth_bn_partials, within

pytestmark = pytest.mark.gpu
EPS = 1e-5
_handles = {}


def handle(W, B):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if (W, B) not in _handles:
        _handles[W, B] = cvlib.Handle(W, B)          # precision 0
    return _handles[W, B]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def nan_out(n):
    return poison(torch.empty(n, device="cuda"), ALL_ONES)


def scratch(H, B):
    return nan_out(H.op_scratch_floats(B))


@functools.lru_cache(maxsize=2)
def operands(layer, W, B, what, lift=0):
    """bf16_ops_tools' case (float64, on the host), shared by the tests of one case; nobody writes to it."""
    return T.case_operands(layer, W, B, what, lift=lift)


def f32(t):
    return t.float()


def run_fwd(H, layer, W, B, x, w, b):
    """-> (out NCHW float64 on the host, y on the device, its BatchNorm partials or None)."""
    cin, cout, h, up, hs = T.geom(layer, W)
    out = nan_out(B * h * h * cout)
    part = nan_out(H.op_bn_partial_floats(layer, B)) if layer < 4 else None
    H.op_conv_fwd(layer, B, dev(f32(x)) if layer == 0 else nhwc(f32(x)), wnat(f32(w)), dev(f32(b)), out, part, scratch(H, B))
    torch.cuda.synchronize()
    return to_nchw(out, B, h, cout).double(), out, part


def run_dgrad(H, layer, W, B, dout, w, mask):
    cin, cout, h, up, hs = T.geom(layer, W)
    din = nan_out(B * hs * hs * cin)
    H.op_conv_dgrad(layer, B, nhwc(f32(dout)), wnat(f32(w)), nhwc(f32(mask)) if mask is not None else None, din, scratch(H, B))
    torch.cuda.synchronize()
    return to_nchw(din, B, hs, cin).double()


def run_wgrad(H, layer, W, B, x, dout):
    """-> (dW OIHW float64, db float64 or None: the per-op entry takes the bias gradient from layer 4 on)."""
    cin, cout, h, up, hs = T.geom(layer, W)
    dw, db = nan_out(25 * cin * cout), nan_out(cout) if layer >= 4 else None
    H.op_conv_wgrad(layer, B, dev(f32(x)) if layer == 0 else nhwc(f32(x)), nhwc(f32(dout)), dw, db, scratch(H, B))
    torch.cuda.synchronize()
    return wref(dw, cin, cout).double(), None if db is None else db.double().cpu()


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
CAPPED_B, BATCHES, cases = F32.CAPPED_B, F32.BATCHES, F32.cases


def ids(cs):
    return [f"w{w}-b{b}-L{l}" for w, b, l in cs]


FWD_CASES, DGRAD_CASES, WGRAD_CASES = cases("fwd"), cases("dgrad"), cases("wgrad")
THIN_CASES = [(W, B) for W in (64, 128) for B in BATCHES[W]]           # E1 and D4: every batch of "every layer"
thin_ids = [f"w{w}-b{b}" for w, b in THIN_CASES]


# ---------------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_bn_partials(H, layer, W, B, y_ref, y_dev, part, tag):
    """The partials of E1..E4's forward: fully written, and through op_bn_pool_act_fwd they give the mean and the variance of the exact y
    within ws_tools.bn_stats_ref's bounds.  The per-row (sum, M2, count) behind the bounds: bf16_ops_tools.partial_rows on the 128-pixel
    tiles of Tile<h>; E1's 512-pixel rows from ws_tools.synth_bn_partials."""
    cin, C, h, _, _ = T.geom(layer, W)
    assert part.numel() == 2 * (B * 8 * (W // 64) ** 2 if layer == 0 else T.cdiv(B, T.tile_geom(h)[2]) * T.tile_geom(h)[3]) * C
    assert bool(torch.isfinite(part).all()), f"{tag}: {int((~torch.isfinite(part)).sum())} of {part.numel()} BatchNorm partials were not written"
    y_nhwc = y_ref.permute(0, 2, 3, 1).contiguous()
    if layer == 0:
        _, S, m2, cnt = synth_bn_partials(y_nhwc, 0, B)
    else:
        S, m2, cnt, _ = T.partial_rows(y_ref, 1)
    gamma, beta = rnd(f"f32ops/g{layer}", (C,), 0.5, 1.5), rnd(f"f32ops/be{layer}", (C,), -0.5, 0.5)
    rm, rv, coef = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), nan_out(4 * C)
    a = nan_out(B * (h // 2) ** 2 * C)
    H.op_bn_pool_act_fwd(layer, B, y_dev, part, dev(gamma), dev(beta), rm, rv, coef, a, scratch(H, B), True)
    torch.cuda.synchronize()
    coef = coef.view(C, 4).double().cpu()
    mu, var, mb, vb = bn_stats_ref(y_nhwc, S, m2, cnt)
    worst = {}
    try:
        within(f"{tag} mean", coef[:, 2], mu, mb, worst)
        istd = 1.0 / torch.sqrt(var + EPS)
        within(f"{tag} invstd", coef[:, 3], istd, istd * (0.5 * vb / (var + EPS) + 4 * U32), worst)
    finally:
        print(f"f32ops-ratio bn {tag}: " + ", ".join(f"{k.rsplit(' ', 1)[1]} err / allowed {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("W,B,layer", FWD_CASES, ids=ids(FWD_CASES))
def test_exact_fwd(W, B, layer):
    """Forward of E2..E4 (raw, with their BatchNorm partials), D0 (ReLU; at 64 x 64 through eight split-K slabs) and D1..D3 (collapsed
    weights behind the upsample; bias + ReLU), bit for bit.  D0..D3 twice: biases of [-2, 2] (the clamp itself: about half of the expected
    outputs are zeros, "not empty" is asserted on the pre-activation) and every bias lifted by RELU_LIFT (at least 90 % nonzero)."""
    H = handle(W, B)
    c = operands(layer, W, B, "fwd")
    T.assert_exact_conditions(c["pre"], f"fwd L{layer} pre-activation", T.max_terms(layer, W, B, "fwd"), False)
    got, y_dev, part = run_fwd(H, layer, W, B, c["x"], c["w"], c["b"])
    assert_equal(got, c["ref"], f"fwd L{layer} at {W} x {W}, B = {B}")
    if layer < 4:
        check_bn_partials(H, layer, W, B, c["ref"], y_dev, part, f"w{W}-b{B}-L{layer}")
    else:
        c = operands(layer, W, B, "fwd", T.RELU_LIFT)
        T.assert_exact_conditions(c["ref"], f"fwd L{layer}, lifted bias", T.max_terms(layer, W, B, "fwd") + T.RELU_LIFT, False)
        got, _, _ = run_fwd(H, layer, W, B, c["x"], c["w"], c["b"])
        assert_equal(got, c["ref"], f"fwd L{layer} at {W} x {W}, B = {B}, lifted bias")


@pytest.mark.parametrize("W,B", THIN_CASES, ids=thin_ids)
def test_exact_e1_fwd(W, B):
    """E1 (e1_fwd_kernel): frames that are multiples of 1/4, integer weights and bias: y is a multiple of 1/4, bit for bit; its partials
    (one row per 512-pixel strip) as for E2..E4."""
    e = T.e1_operands(W, B)
    T.assert_exact_conditions(e["ref"] * 4, "E1 forward, in quarters", 4 * (75 + 2), False)
    H = handle(W, B)
    got, y_dev, part = run_fwd(H, 0, W, B, e["x"], e["w"], e["b"])
    assert_equal(got, e["ref"], f"E1 forward at {W} x {W}, B = {B}")
    check_bn_partials(H, 0, W, B, e["ref"], y_dev, part, f"w{W}-b{B}-L0")


@pytest.mark.parametrize("W,B", THIN_CASES, ids=thin_ids)
def test_d4_fwd(W, B):
    """D4's forward (d4_fwd_pc_f32_kernel) on pre-activations that are exact multiples of 1/8 in [-2, 2]: at most 33 distinct values.
    Structure, by equality: all outputs of one expected pre-activation hold one bit pattern (f32_ops_tools.d4_value_groups; by signed value:
    the kernel's tanh, 1 - 2 / (exp(2x) + 1), is not odd in floating point).  One tap, source pixel or phase slot wrong anywhere moves an
    element into another group.  Value: max |recon - tanh(pre)| against float64 tanh within test_gpu_ops.TOL, the project's forward bar
    (measured on the MI355X: LABNOTES)."""
    f = T.d4_fwd_operands(W, B)
    p8 = f["pre"] * 8
    assert bool((p8 == p8.round()).all()) and float(f["pre"].abs().max()) <= 2.0 and float((f["pre"] != 0).double().mean()) >= 0.9
    H = handle(W, B)
    recon = nan_out(B * 3 * W * W)
    H.op_conv_fwd(8, B, nhwc(f32(f["o3"])), wnat(f32(f["w"])), dev(f32(f["b"])), recon, None, scratch(H, B))
    torch.cuda.synchronize()
    recon = recon.view(B, 3, W, W).cpu()
    vals, _ = F32.d4_value_groups(recon, f["pre"])
    gap = (recon.double() - torch.tanh(f["pre"])).abs().max().item()
    print(f"f32ops-ratio d4 fwd w{W} B{B}: {len(vals)} pre-activation values, one bit pattern each; max |recon - tanh(pre)| {gap:.3e} of {TOL:g}")
    assert gap <= TOL, f"D4 forward at {W} x {W}, B = {B}: max |recon - tanh(pre)| {gap:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,B,layer", DGRAD_CASES, ids=ids(DGRAD_CASES))
def test_exact_dgrad(W, B, layer):
    """Input gradient of E2..E4, D0 (at 64 x 64 through its four split-K slabs, at every batch: see the module docstring) and D1..D3 (2 x 2
    sums and the ReLU mask of the producing layer, 95 % lit), bit for bit."""
    c = operands(layer, W, B, "dgrad")
    T.assert_exact_conditions(c["ref"], f"dgrad L{layer}", T.max_terms(layer, W, B, "dgrad"), False)
    got = run_dgrad(handle(W, B), layer, W, B, c["dout"], c["w"], c["mask"])
    assert_equal(got, c["ref"], f"dgrad L{layer} at {W} x {W}, B = {B}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# weight and bias gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_wgrad(W, B, layer):
    """Layers 0..7 on dense operands (f32_ops_tools.wgrad_case: reduced to +-1 where the batch would break the 2^24 bound)."""
    c = F32.wgrad_case(layer, W, B)
    unit = 4 if layer == 0 else 1            # E1: dW is a multiple of 1/4
    assert c["bound"] == F32.wgrad_bound(layer, W, B, c["unit"]) < T.EXACT_FP32
    T.assert_exact_conditions(c["ref_w"] * unit, f"wgrad L{layer}", c["bound"], False)
    dw, db = run_wgrad(handle(W, B), layer, W, B, c["x"], c["dout"])
    assert_equal(dw, c["ref_w"], f"wgrad L{layer} at {W} x {W}, B = {B}")
    if layer >= 4:
        T.assert_exact_conditions(c["ref_b"], f"dbias L{layer}", c["bound"], False)
        assert_equal(db, c["ref_b"], f"dbias L{layer} at {W} x {W}, B = {B}")


def check_d4_bwd(W, B):
    """op_d4_bwd: dOut = d_recon (1 - recon^2) with recon in {0, +-1/2} is an integer (d4_actbwd_kernel forms 1 - r r and multiplies: exact),
    so dout, d_o3 (ReLU-masked), dW4 and db4 are all equalities."""
    g = T.d4_bwd_operands(W, B)
    assert F32.wgrad_bound(8, W, B) == 16 * B * W * W < T.EXACT_FP32
    T.assert_exact_conditions(g["dout"], "dOut", 8, False)
    T.assert_exact_conditions(g["d_o3"], "d_o3", 3 * 25 * 8 * 4, False)
    T.assert_exact_conditions(g["dw"], "dW4", 16 * B * W * W, False)
    T.assert_exact_conditions(g["db"], "db4", 8 * B * W * W, False)
    H = handle(W, B)
    dout, d_o3, dw, db = nan_out(B * 3 * W * W), nan_out(B * 32 * (W // 2) ** 2), nan_out(2400), nan_out(3)
    H.op_d4_bwd(B, nhwc(f32(g["o3"])), dev(f32(g["d_recon"])), dev(f32(g["recon"])), wnat(f32(g["w"])), dout, d_o3, dw, db, scratch(H, B))
    torch.cuda.synchronize()
    assert_equal(dout.view(B, 3, W, W).double().cpu(), g["dout"], f"dOut at {W} x {W}, B = {B}")
    assert_equal(to_nchw(d_o3, B, W // 2, 32).double(), g["d_o3"], f"d_o3 at {W} x {W}, B = {B}")
    assert_equal(wref(dw, 32, 3).double(), g["dw"], f"dW4 at {W} x {W}, B = {B}")
    assert_equal(db.double().cpu(), g["db"], f"db4 at {W} x {W}, B = {B}")


@pytest.mark.parametrize("W,B,layer", WGRAD_CASES, ids=ids(WGRAD_CASES))
def test_exact_wgrad(W, B, layer):
    """Weight gradient of layers 1..7 (bias gradient from D0 on), bit for bit."""
    check_wgrad(W, B, layer)


@pytest.mark.parametrize("W,B", THIN_CASES, ids=thin_ids)
def test_exact_e1_wgrad(W, B):
    """E1's weight gradient (e1_wgrad_kernel, unfused form): 4 dW is an integer bounded by 8 B W^2."""
    assert 8 * B * W * W < T.EXACT_FP32
    check_wgrad(W, B, 0)


@pytest.mark.parametrize("W,B", THIN_CASES, ids=thin_ids)
def test_exact_d4_bwd(W, B):
    check_d4_bwd(W, B)


@pytest.mark.parametrize("layer", range(9))
@pytest.mark.parametrize("W", [64, 128])
def test_exact_wgrad_two_tiles_per_split(W, layer):
    """Every fp32 weight-gradient kernel (layer 8: the fused D4 backward) at the smallest batch at which a split walks at least two tiles
    and the walk ends unevenly, on this device's compute-unit count.  The batch comes from the mirror, and the mirror is held to the
    launchers' own split functions (cvae_op_conv_wgrad_plan_f32) at that batch and the one below."""
    n = cus()
    B = F32.wgrad_two_tile_batch_f32(layer, W, n)
    tiles, S, tps, imgs = F32.wgrad_geometry_f32(layer, W, B, n)
    plan = cvlib.conv_wgrad_plan_f32(W, layer, B, n)
    assert plan == (tiles, S, tps), f"layer {layer} at {W} x {W}, B = {B}: the launcher plans {plan}, the mirror {(tiles, S, tps)}"
    assert cvlib.conv_wgrad_plan_f32(W, layer, B - 1, n) == F32.wgrad_geometry_f32(layer, W, B - 1, n)[:3]
    assert plan[2] >= 2 and (plan[0] % plan[2] or B % imgs), f"layer {layer} at {W} x {W}, B = {B}: {tiles} tiles on {S} splits"
    assert not F32.walks_two_tiles_unevenly(layer, W, B - 1, n)
    assert F32.wgrad_bound(layer, W, B, F32.wgrad_bound(layer, W, B) >= T.EXACT_FP32) < T.EXACT_FP32
    print(f"f32ops-geometry wgrad w{W} L{layer}: B = {B}, {tiles} tiles, {S} splits, {tps} tiles per split ({n} CUs)")
    if layer == 8:
        check_d4_bwd(W, B)
    else:
        check_wgrad(W, B, layer)


# ---------------------------------------------------------------------------------------------------------------------------------------
# several items per workgroup
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_exact_cases_walk_several_items_under_a_grid_cap():
    """A child process caps every persistent grid at 8 workgroups (CVAE_PERSIST_MAXWG, read once per process) and reruns the B = 37 forward
    and input-gradient cases of E2..E4 at both frame sizes and the D4 forward at (64, 37): conv_mfma_ps.hip then walks several tiles and
    channel blocks per workgroup with ragged ends (E4 forward at 64 x 64: 19 tiles, rounded up to 24, x 4 blocks on 8 workgroups), and
    d4_fwd_pc_f32_kernel 37 tiles per workgroup (296 tiles of 16 x 32 outputs), all on exact operands."""
    routes = [(W, layer, dg) for W in (64, 128) for layer in (1, 2, 3) for dg in (0, 1) if cvlib.load().cvae_conv_route(0, W, layer, dg, CAPPED_B) == 1]
    assert (64, 3, 0) in routes and (128, 1, 0) in routes, f"the persistent fp32 passes at B = {CAPPED_B}: {routes}"
    assert CAPPED_B * (64 // 16) * (64 // 32) > 8
    sel = (f"((test_exact_fwd or test_exact_dgrad) and -b{CAPPED_B}-L and (L1 or L2 or L3)) or (test_d4_fwd and w64-b{CAPPED_B})")
    want = sum(1 for cs in (FWD_CASES, DGRAD_CASES) for _, B, layer in cs if B == CAPPED_B and layer in (1, 2, 3)) + 1
    assert want == 13
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVAE_PERSIST_MAXWG="8")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    m = re.search(r"\b(\d+) passed\b", p.stdout)
    print(f"f32ops-capped: the child run with CVAE_PERSIST_MAXWG=8: {m.group(1) if m else 'no'} passed (of {want})")
    assert m and int(m.group(1)) == want and "failed" not in p.stdout, p.stdout[-1000:]
