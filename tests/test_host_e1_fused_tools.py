"""e1_fused_tools on the host: the reference is the gradient of BatchNorm -> MaxPool -> ReLU, the split mirrors are the launchers' own
arithmetic (cvae_op_conv_wgrad_plan_f32 at every device size, cvae_op_conv_wgrad_plan(layer 0) on a bf16 handle at the size it reports), the
uneven-walk batches walk two tiles and end short, every case of test_gpu_e1_fused_ops.py meets its exactness conditions, and every mutated
reference (what a subtly wrong kernel would compute) differs from the true one on the cases that are meant to see it."""
import pytest
import torch
import torch.nn.functional as F

import e1_fused_tools as E
import f32_ops_tools as F32
from bf16_ops_tools import EXACT_FP32
from critic_vae_amd import lib as cvlib

CUS = F32.CU_COUNTS
MODES = [False, True]
mode_ids = ["f32", "bf16"]


def this_device_cus():
    """What cvae_num_cus answers here: the device's count, or 256 without a device."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def test_reference_is_the_gradient_of_batchnorm_pool_relu():
    """fused_dy_ref with (k1, k2) = (sum g, sum g xhat) / N against autograd through the float64 forward."""
    g0 = torch.Generator().manual_seed(5)
    B, H, C = 3, 8, 32
    y = torch.randn(B, H, H, C, generator=g0, dtype=torch.float64, requires_grad=True)
    gamma = torch.rand(C, generator=g0, dtype=torch.float64) + 0.5
    gamma[::3] *= -1
    beta = torch.rand(C, generator=g0, dtype=torch.float64) - 0.5
    d_a = torch.randn(B, H // 2, H // 2, C, generator=g0, dtype=torch.float64)
    mean, var = y.mean(dim=(0, 1, 2)), y.var(dim=(0, 1, 2), unbiased=False)
    istd = 1.0 / torch.sqrt(var + 1e-5)
    n = (y - mean) * istd * gamma + beta
    a = F.max_pool2d(n.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).relu()
    (a * d_a).sum().backward()
    with torch.no_grad():
        coef = torch.stack((gamma * istd, beta - mean * gamma * istd, mean, istd), 1)
        g = d_a * (a > 0)
        yw = E.bn_windows(y, B, H, C)
        xm = ((yw - mean) * istd).gather(3, E.arg_max(E.normalised(yw, coef)))[:, :, :, 0]
        N = B * H * H
        bcoef = torch.stack((g.sum(dim=(0, 1, 2)) / N, (g * xm).sum(dim=(0, 1, 2)) / N), 1)
        dy = E.fused_dy_ref(y.detach(), a, d_a, coef, bcoef, False)
    assert float((dy - y.grad).abs().max()) < 1e-12
    assert torch.equal(E.unwindow(E.bn_windows(y.detach(), B, H, C)), y.detach())


@pytest.mark.parametrize("cus", CUS)
def test_fp32_mirror_is_the_launchers_split_arithmetic(cus):
    for W in (64, 128):
        for B in range(1, 301):
            assert cvlib.conv_wgrad_plan_f32(W, 0, B, cus) == E.e1_geometry(W, B, False, cus), (W, B, cus)


def test_bf16_mirror_is_the_launchers_split_arithmetic():
    """cvae_op_conv_wgrad_plan(layer 0) of a bf16 handle asks the device for its compute units (256 without one); the mirror is held to it
    at that count, and to hand-checked plans at the others."""
    cus = this_device_cus()
    for W in (64, 128):
        h = cvlib.Handle(W, 8, precision="bf16")
        for B in range(1, 301):
            assert h.op_conv_wgrad_plan(0, B) == E.e1_geometry(W, B, True, cus), (W, B, cus)
        with pytest.raises(cvlib.CvaeError, match="layer 0"):
            cvlib.Handle(W, 8).op_conv_wgrad_plan(0, 8)
    assert E.e1_geometry(64, 49, True, 256) == (1568, 523, 3) and E.e1_geometry(128, 13, True, 256) == (1664, 555, 3)
    assert E.e1_geometry(64, 48, True, 256) == (1536, 768, 2) and E.e1_geometry(64, 24, True, 256) == (768, 768, 1)
    assert E.e1_geometry(64, 13, True, 64) == (416, 139, 3) and E.e1_geometry(64, 100, True, 304) == (3200, 800, 4)
    assert E.e1_geometry(64, 200, True, 512) == (6400, 915, 7), "THIN_SPLIT_CAP: never more than 1024 splits"


@pytest.mark.parametrize("cus", CUS)
def test_uneven_batches_walk_two_tiles_and_end_short(cus):
    for W in (64, 128):
        for bf16 in MODES:
            B = E.uneven_batch(W, bf16, cus)
            tiles, S, tps = E.e1_geometry(W, B, bf16, cus)
            assert tps >= 2 and tiles % tps != 0 and (S - 1) * tps < tiles < S * tps, (W, bf16, B)
            assert all(not E.walks_unevenly(E.e1_geometry(W, b, bf16, cus)) for b in range(1, B))
            assert 4 * B * W * W < EXACT_FP32, "the route case of this batch keeps its sums below 2^24"
            print(f"e1fused-geometry (host) w{W} {'bf16' if bf16 else 'f32'} on {cus} CUs: B = {B}, {tiles} tiles, {S} splits, {tps} tiles per split")
    if cus == 256:
        assert [E.uneven_batch(W, bf16) for bf16 in MODES for W in (64, 128)] == [34, 10, 49, 13]


ROUTE_SMALL = [(W, B) for W in (64, 128) for B in F32.BATCHES[W]]
ROUTE_UNEVEN = [(W, bf16, E.uneven_batch(W, bf16)) for W in (64, 128) for bf16 in MODES]


def report(c):
    print(f"e1fused-case {c['kind']} w{c['W']} B{c['B']} {'bf16' if c['bf16'] else 'f32'}: bound {c['bound']:.0f} of {EXACT_FP32:.0f} units of {c['unit']}, "
          f"{c['ties']} tied windows, {c['zero_max']} gradient-carrying windows with maximum 0"
          + (f", {c['tie_changed']} dW elements move with the last maximum" if c["kind"] == "route" else f", {c['needs_round']} dy elements need rounding"))


@pytest.mark.parametrize("bf16", MODES, ids=mode_ids)
def test_route_cases_meet_their_conditions(bf16):
    for W, B in ROUTE_SMALL + [(W, B) for W, m, B in ROUTE_UNEVEN if m == bf16]:
        c = E.assert_conditions(E.route_case(W, B, bf16))
        assert c["ties"] > 0 and c["tie_changed"] > 0 and c["bound"] == 4 * B * W * W < EXACT_FP32
        report(c)


@pytest.mark.parametrize("bf16", MODES, ids=mode_ids)
def test_arith_cases_meet_their_conditions_and_larger_batches_are_refused(bf16):
    rounded = 0
    for W in (64, 128):
        allowed = E.ARITH_BATCHES[W, bf16]
        assert set(allowed) <= set(F32.BATCHES[W])
        for B in allowed:
            c = E.assert_conditions(E.arith_case(W, B, bf16))
            assert c["bound"] < EXACT_FP32
            rounded += c["needs_round"] > 0
            report(c)
        nxt = min(b for b in F32.BATCHES[64] if b > max(allowed))              # the next batch of the per-op tests' list
        with pytest.raises(ValueError, match="2\\^24"):
            E.arith_case(W, nxt, bf16)
    assert rounded > 0 or not bf16, "no bf16 arith case has a dy of more than 8 significant bits"


def differs(mut, ref, what):
    n = int((mut != ref).sum())
    print(f"e1fused-mutation {what}: {n} of {ref.numel()} expected dW elements differ")
    assert n > 0, f"{what}: the mutated reference equals the true one"


@pytest.mark.parametrize("bf16", MODES, ids=mode_ids)
@pytest.mark.parametrize("kind", ["route", "arith"])
def test_mutated_references_differ(kind, bf16):
    """At (64, 3) and (128, 1), where every split holds one tile: every mistake but the dead prefetch path."""
    for W, B in ((64, 3), (128, 1)):
        c = E.assert_conditions((E.route_case if kind == "route" else E.arith_case)(W, B, bf16))
        plan = E.e1_geometry(W, B, bf16)
        for mut, kinds in E.SEEN_BY.items():
            if kind not in kinds or mut == "first-tile-only" or (mut == "no-round" and not bf16):
                continue
            dw, db = E.mutated_ref(c, mut, plan)
            differs(dw, c["ref_w"], f"{kind} w{W} B{B} {'bf16' if bf16 else 'f32'}, {mut}")
        if kind == "arith" and bf16:
            assert c["needs_round"] > 0
        same, _ = E.mutated_ref(c, "first-tile-only", plan)
        assert plan[2] == 1 and torch.equal(same, c["ref_w"]), "one tile per split: nothing to drop"


@pytest.mark.parametrize("W,bf16,B", ROUTE_UNEVEN, ids=[f"w{w}-{'bf16' if m else 'f32'}-b{b}" for w, m, b in ROUTE_UNEVEN])
def test_tile_mutations_differ_at_the_uneven_batches(W, bf16, B):
    """At the uneven-walk batch on 256 compute units: the last (short) split's last tile, the second and later tiles of every split, the
    bottom window row of every tile, and the tie rule."""
    c = E.assert_conditions(E.route_case(W, B, bf16))
    plan = E.e1_geometry(W, B, bf16)
    assert E.walks_unevenly(plan)
    for mut in E.TILE_MUTATIONS + ("tie-last",):
        dw, db = E.mutated_ref(c, mut, plan)
        differs(dw, c["ref_w"], f"route w{W} B{B} {'bf16' if bf16 else 'f32'}, {mut}")
        assert mut == "tie-last" or not torch.equal(db, c["ref_b"])
    keep = E.tile_mutation_mask(W, B, "first-tile-only", plan)
    assert int(keep.sum()) == plan[1] * 128 and int(E.tile_mutation_mask(W, B, "drop-last-tile", plan).sum()) == (plan[0] - 1) * 128
