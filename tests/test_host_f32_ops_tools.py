"""f32_ops_tools on the host: the mirror of the fp32 weight-gradient split arithmetic is the launchers' own (cvae_op_conv_wgrad_plan_f32, host
logic only), the batches it picks walk two tiles and end unevenly, every case batch of test_gpu_f32_ops.py meets the conditions under which
the comparison may be equality at every device size, the float64 references bite (each mutation a subtly wrong kernel could compute
differs from the true reference somewhere; the count is printed), and the D4 grouping check rejects what it must."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import bf16_ops_tools as T
import f32_ops_tools as F32
from critic_vae_amd import lib as cvlib

CUS = F32.CU_COUNTS


@pytest.mark.parametrize("cus", CUS)
def test_mirror_is_the_launchers_split_arithmetic(cus):
    """wgrad_geometry_f32 against cvae_op_conv_wgrad_plan_f32 (thin_splits, wgrad_splits<H>, run_up_wgrad's arithmetic, d4_splits: the
    functions the launchers call) for every layer, both widths and every batch up to 300."""
    for W in (64, 128):
        for layer in range(9):
            for B in range(1, 301):
                assert cvlib.conv_wgrad_plan_f32(W, layer, B, cus) == F32.wgrad_geometry_f32(layer, W, B, cus)[:3], (W, layer, B, cus)


def test_plan_entry_answers_without_a_device_and_checks_its_arguments():
    lib = cvlib.load()
    out = (ctypes.c_int32 * 3)()
    assert lib.cvae_op_conv_wgrad_plan_f32(64, 1, 65, 256, out) == 0 and tuple(out) == (520, 174, 3)
    assert cvlib.conv_wgrad_plan_f32(64, 0, 34, 256) == (1088, 363, 3)            # E1: 32 strips of 4 x 32 per image on 512 splits
    assert cvlib.conv_wgrad_plan_f32(64, 8, 130, 256) == (1040, 347, 3)           # D4: 8 blocks of 16 x 32 per image
    assert cvlib.conv_wgrad_plan_f32(64, 7, 130, 256) == (520, 174, 3)            # D3: one workgroup per CU
    assert cvlib.conv_wgrad_plan_f32(64, 7, 130, 64) != cvlib.conv_wgrad_plan_f32(64, 7, 130, 256)
    assert cvlib.conv_wgrad_plan_f32(64, 3, 130, 64) == cvlib.conv_wgrad_plan_f32(64, 3, 130, 256)      # only D1..D3 ask the device
    for W, layer, B, cus in ((96, 1, 8, 256), (0, 1, 8, 256), (64, -1, 8, 256), (64, 9, 8, 256), (64, 1, 0, 256), (128, 1, -3, 256), (64, 1, 8, 0)):
        assert lib.cvae_op_conv_wgrad_plan_f32(W, layer, B, cus, out) != 0, (W, layer, B, cus)
    assert lib.cvae_op_conv_wgrad_plan_f32(64, 1, 8, 256, None) != 0
    with pytest.raises(cvlib.CvaeError, match="width 96"):
        cvlib.conv_wgrad_plan_f32(96, 1, 8, 256)


@pytest.mark.parametrize("cus", CUS)
def test_two_tile_batches_walk_two_tiles_and_end_unevenly(cus):
    for W in (64, 128):
        for layer in range(9):
            B = F32.wgrad_two_tile_batch_f32(layer, W, cus)
            tiles, S, tps, imgs = F32.wgrad_geometry_f32(layer, W, B, cus)
            assert tps >= 2 and (S - 1) * tps < tiles <= S * tps and (tiles % tps != 0 or B % imgs != 0), (W, layer, B)
            assert all(not F32.walks_two_tiles_unevenly(layer, W, b, cus) for b in range(1, B)), (W, layer, B)
            assert cvlib.conv_wgrad_plan_f32(W, layer, B, cus) == (tiles, S, tps)
            print(f"f32ops-geometry (host) wgrad w{W} L{layer} on {cus} CUs: B = {B}, {tiles} tiles, {S} splits, {tps} tiles per split")
    if cus == 256:
        assert [F32.wgrad_two_tile_batch_f32(l, 64) for l in range(9)] == [34, 65, 65, 33, 129, 129, 129, 130, 130]
        assert [F32.wgrad_two_tile_batch_f32(l, 128) for l in range(9)] == [10, 17, 17, 17, 33, 33, 65, 34, 34]


def test_every_case_batch_keeps_its_sums_below_2_to_24():
    """The bound arithmetic of every case of test_gpu_f32_ops.py: forward and input gradient do not depend on the batch; the weight
    gradients' bounds grow with it, at the listed batches and at the two-tile batches of every device size."""
    for what in ("fwd", "dgrad"):
        for W, B, layer in F32.cases(what):
            assert T.max_terms(layer, W, B, what) + T.RELU_LIFT < T.EXACT_FP32
    for W, B, layer in F32.cases("wgrad"):
        assert F32.wgrad_bound(layer, W, B) < T.EXACT_FP32, (W, B, layer)
    for W in (64, 128):
        for B in F32.BATCHES[W]:
            assert F32.wgrad_bound(0, W, B) < T.EXACT_FP32 and F32.wgrad_bound(8, W, B) < T.EXACT_FP32
        for cus in CUS:
            for layer in range(9):
                B = F32.wgrad_two_tile_batch_f32(layer, W, cus)
                unit = F32.wgrad_bound(layer, W, B) >= T.EXACT_FP32
                assert F32.wgrad_bound(layer, W, B, unit) < T.EXACT_FP32, (W, layer, B, cus)
                assert not (unit and layer == 8), "D4's backward operands have no reduced form"


B0 = 3          # the smallest odd batch: half-filled image groups, a last image that is not the first


@pytest.mark.parametrize("W,layer", [(64, 0), (128, 0), (64, 2), (64, 4), (64, 5), (128, 7)])
def test_weight_gradient_operands_meet_the_exactness_conditions(W, layer):
    """On a cheap subset of layers (the others share the construction): integer-valued (E1: in quarters), at least 90 % nonzero, dense
    operands; and the reduced +-1 form that wgrad_case falls back to is exact too."""
    c = F32.wgrad_case(layer, W, B0)
    assert not c["unit"] and c["bound"] == F32.wgrad_bound(layer, W, B0)
    T.assert_exact_conditions(c["ref_w"] * (4 if layer == 0 else 1), f"wgrad L{layer}", c["bound"], False)
    assert bool((c["x"] != 0).all()) and bool((c["dout"] != 0).all())
    if layer == 0:
        assert set(c["x"].unique().tolist()) == {0.25, 0.5, 0.75, 1.0} and set(c["dout"].unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
        assert float((c["ref_w"] * 4).abs().max()) <= 8 * B0 * W * W
        u = F32.e1_wgrad_operands(W, B0, unit=True)
        assert set(u["dout"].unique().tolist()) == {-1.0, 1.0} and u["bound"] == 4 * B0 * W * W
        T.assert_exact_conditions(u["ref_w"] * 4, "wgrad L0, unit", u["bound"], False)
        wz = torch.zeros(32, 3, 5, 5, dtype=torch.float64, requires_grad=True)
        F.conv2d(c["x"], wz, padding=2).backward(c["dout"])
        assert torch.equal(wz.grad, c["ref_w"]), "e1_wgrad_operands' reference is not the gradient of conv2d"


def differs(mut, ref, what):
    n = int((mut != ref).sum())
    print(f"f32ops-mutation {what}: {n} of {ref.numel()} expected elements differ")
    assert n > 0, f"{what}: the mutated reference equals the true one"
    return n


@pytest.mark.parametrize("W,layer", [(64, 0), (64, 3), (64, 6), (64, 8)])
def test_weight_gradient_reference_bites(W, layer):
    """At the layer's two-tile batch on 256 compute units (E1, E4, D2 and D4's dW at 64 x 64): one tap, one image of the last group, one
    pixel row at a tile edge, or the last tile of the last split less changes the expected weight gradient."""
    B = F32.wgrad_two_tile_batch_f32(layer, W)
    tiles, S, tps, imgs = F32.wgrad_geometry_f32(layer, W, B)
    tag = f"wgrad w{W} L{layer} B{B}"
    if layer == 8:
        g = T.d4_bwd_operands(W, B)
        x, dout, ref = g["o3"], g["dout"], g["dw"]
    else:
        c = F32.wgrad_case(layer, W, B)
        x, dout, ref = c["x"], c["dout"], c["ref_w"]
    # the sums are linear in the terms: a reference with some terms left out is the full one minus the sum over those terms alone (exact
    # in float64 on these operands), which keeps D4's 130 images of 64 x 64 out of four more full passes
    few = T.conv_wgrad_ref(layer, x[:4], dout[:4])[0]
    r = T.conv_wgrad_ref(layer, x[:4], dout[:4], drop_tap=(1, 3))[0]
    assert bool((r[:, :, 1, 3] == 0).all()) and differs(r, few, f"{tag}, tap (1, 3) dropped (first four images)") == int((few[:, :, 1, 3] != 0).sum())
    differs(ref - T.conv_wgrad_ref(layer, x[-1:], dout[-1:])[0], ref, f"{tag}, last image of the last group dropped")
    assert torch.equal(ref - T.conv_wgrad_ref(layer, x[-1:], dout[-1:])[0], T.conv_wgrad_ref(layer, x[:-1], dout[:-1])[0]) or layer == 8
    b0, n, y0, y1, x0, x1 = F32.wgrad_tile_box(layer, W, tiles - 1)
    assert b0 + n >= B > b0 and y1 <= dout.shape[2] and x1 <= dout.shape[3], "the last tile holds the last image"
    differs(F32.wgrad_ref_without(layer, x, dout, (B - 1, 1, y1 - 1, y1, x0, x1), ref), ref, f"{tag}, one pixel row at a tile edge dropped")
    differs(F32.wgrad_ref_without(layer, x, dout, (b0, n, y0, y1, x0, x1), ref), ref, f"{tag}, last tile of the last split dropped")


@pytest.mark.parametrize("W,layer", [(64, 5), (64, 7)])
def test_up_conv_references_bite(W, layer):
    """D1 and D3: a collapsed phase tap taken from the neighbouring slot, the ReLU mask ignored, the 2 x 2 upsample sum over three pixels."""
    c = T.case_operands(layer, W, B0, "fwd", lift=T.RELU_LIFT)
    assert torch.equal(T.up_conv_collapsed(c["x"], T.collapse_w(c["w"]), c["b"]).relu(), c["ref"]), "the collapsed form is not the 5 x 5 form"
    for py, ta in ((0, 0), (1, 2), (0, 1)):
        mut = T.up_conv_collapsed(c["x"], F32.collapse_w_neighbour_slot(c["w"], py, ta), c["b"]).relu()
        differs(mut, c["ref"], f"fwd w{W} L{layer}: slot {ta} of phase row {py} taken from R({1 - py}, {ta})")
    d = T.case_operands(layer, W, B0, "dgrad")
    differs(T.conv_dgrad_ref(layer, d["dout"], d["w"], torch.ones_like(d["mask"])), d["ref"], f"dgrad w{W} L{layer}: ReLU mask ignored")
    differs(F32.up_dgrad_three_of_four(d["dout"], d["w"], d["mask"]), d["ref"], f"dgrad w{W} L{layer}: upsample sum over three of four pixels")


def test_d4_grouping_check_rejects_one_ulp_and_a_missing_tap():
    W, B = 64, 2
    f = T.d4_fwd_operands(W, B)
    recon = torch.tanh(f["pre"]).float()
    vals, pats = F32.d4_value_groups(recon, f["pre"])
    assert 8 <= len(vals) <= 33 and len(set(pats.tolist())) == len(vals)
    # one ulp in one pixel, at a value that other pixels share
    k = int((f["pre"].flatten() == vals[len(vals) // 2]).nonzero()[1])
    bad = recon.clone()
    bad.view(torch.int32).view(-1)[k] += 1
    with pytest.raises(AssertionError, match="more than one bit pattern"):
        F32.d4_value_groups(bad, f["pre"])
    # a kernel that loses one tap: exact in itself, but its groups are not the expected ones
    w1 = f["w"].clone()
    co, ci, r, s = (int(v) for v in (w1 != 0).nonzero()[0])
    w1[co, ci, r, s] = 0
    pre1 = F.conv2d(T.up2(f["o3"]), w1, f["b"], padding=2)
    print(f"f32ops-mutation d4 fwd: tap ({co}, {ci}, {r}, {s}) dropped: {int((pre1 != f['pre']).sum())} of {pre1.numel()} pre-activations differ")
    with pytest.raises(AssertionError, match="more than one bit pattern"):
        F32.d4_value_groups(torch.tanh(pre1).float(), f["pre"])
    with pytest.raises(AssertionError, match="distinct pre-activations"):
        F32.d4_value_groups(recon, f["pre"] + 0.01 * T._u("L8/jitter", tuple(f["pre"].shape)))
