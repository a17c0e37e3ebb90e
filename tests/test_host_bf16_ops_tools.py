"""bf16_ops_tools on the host: the integer operands meet the conditions under which test_gpu_bf16_ops.py may compare by equality, the
float64 references bite (one tap, one border pixel or one image less changes an expected element), and the launch-geometry mirrors give
the numbers the kernels' launchers give at known batches."""
import pytest
import torch

import bf16_ops_tools as T

B0 = 2          # the smallest batch with a last image that is not the first
CASES = [(W, layer, what) for W in (64, 128) for layer in range(1, 8) for what in T.PASSES]
ids = [f"w{w}-L{l}-{p}" for w, l, p in CASES]


@pytest.mark.parametrize("W,layer,what", CASES, ids=ids)
def test_integer_operands_meet_the_exactness_conditions_and_the_reference_bites(W, layer, what):
    cin, cout, h, up, hs = T.geom(layer, W)
    c = T.case_operands(layer, W, B0, what)
    bound = T.max_terms(layer, W, B0, what)
    if what == "fwd":
        T.assert_exact_conditions(c["pre"], "pre-activation", bound, True)
        assert float(c["ref"].abs().max()) <= T.EXACT_BF16 and bool((c["ref"] == c["ref"].round()).all())
        assert bool((c["x"] >= 0).all()) == bool(up), "the inputs of D1..D3, and only they, are post-ReLU"
        ref, x, w, b = c["ref"], c["x"], c["w"], c["b"]
        w1 = w.clone()
        w1[:, :, 0, 0] = 0
        assert not torch.equal(T.conv_fwd_ref(layer, x, w1, b), ref), "tap (0, 0) zeroed: nothing changes"
        x1 = x.clone()
        x1[:, :, 0, 0] = 0
        assert bool((x[:, :, 0, 0] != 0).any()) and not torch.equal(T.conv_fwd_ref(layer, x1, w, b), ref), "corner pixel zeroed: nothing changes"
        x2 = x.clone()
        x2[-1] = 0
        assert not torch.equal(T.conv_fwd_ref(layer, x2, w, b)[-1], ref[-1]), "last image dropped: nothing changes"
    elif what == "dgrad":
        T.assert_exact_conditions(c["ref"], "input gradient", bound, True)
        ref, d, w, m = c["ref"], c["dout"], c["w"], c["mask"]
        w1 = w.clone()
        w1[:, :, 0, 0] = 0
        assert not torch.equal(T.conv_dgrad_ref(layer, d, w1, m), ref), "tap (0, 0) zeroed: nothing changes"
        d1 = d.clone()
        d1[:, :, -1, -1] = 0
        assert not torch.equal(T.conv_dgrad_ref(layer, d1, w, m), ref), "corner pixel zeroed: nothing changes"
        d2 = d.clone()
        d2[-1] = 0
        assert not torch.equal(T.conv_dgrad_ref(layer, d2, w, m)[-1], ref[-1]), "last image dropped: nothing changes"
        if up:
            assert bool((ref[m == 0] == 0).all()) and bool((m == 0).any()), "the ReLU mask is not in the reference"
    else:
        T.assert_exact_conditions(c["ref_w"], "weight gradient", bound, False)
        T.assert_exact_conditions(c["ref_b"], "bias gradient", bound, False)
        ref, x, d = c["ref_w"], c["x"], c["dout"]
        assert bool((x != 0).all()) and bool((d != 0).all()), "both operands of the weight gradient are dense"
        # one pixel less moves every element it reaches by one product: at most 4 of a sum of B h h terms
        x1 = x.clone()
        x1[:, :, 0, 0] = 0
        r1 = T.conv_wgrad_ref(layer, x1, d)[0]
        assert not torch.equal(r1, ref) and float((r1 - ref).abs().max()) <= 4 * B0 * (4 if up else 1), "corner pixel zeroed"
        assert not torch.equal(T.conv_wgrad_ref(layer, x[:-1], d[:-1])[0], ref), "last image dropped: nothing changes"
        r3 = T.conv_wgrad_ref(layer, x, d, drop_tap=(0, 0))[0]
        assert bool((r3[:, :, 0, 0] == 0).all()) and bool((ref[:, :, 0, 0] != 0).any()) and torch.equal(r3[:, :, 1:, :], ref[:, :, 1:, :])
        # the 25 matrix products are the convolution's weight gradient
        xin = (T.up2(x) if up else x).requires_grad_(False)
        wz = torch.zeros(cout, cin, 5, 5, dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(xin, wz, padding=2).backward(d)
        assert torch.equal(wz.grad, ref), "conv_wgrad_ref is not the gradient of conv2d"


@pytest.mark.parametrize("W", [64, 128])
def test_e1_and_d4_operands(W):
    e = T.e1_operands(W, B0)
    q = e["ref"] * 4
    assert bool((q == q.round()).all()) and float(q.abs().max()) <= T.EXACT_BF16 and float((q != 0).double().mean()) >= 0.9
    assert torch.equal(e["ref"].bfloat16().double(), e["ref"]), "E1's expected output is not exact in bf16"
    f = T.d4_fwd_operands(W, B0)
    p8 = f["pre"] * 8
    assert bool((p8 == p8.round()).all()) and float(f["pre"].abs().max()) <= 2.0
    assert float((f["pre"] != 0).double().mean()) >= 0.9 and int((f["w"] != 0).sum()) == 3 * T.D4_TAPS
    g = T.d4_bwd_operands(W, B0)
    assert set(g["dout"].abs().unique().tolist()) <= {3.0, 4.0, 6.0, 8.0}
    T.assert_exact_conditions(g["d_o3"], "d_o3", 3 * 25 * 8 * 4, True)
    T.assert_exact_conditions(g["dw"], "dW4", B0 * W * W * 16, False)
    T.assert_exact_conditions(g["db"], "db4", B0 * W * W * 8, False)
    assert bool((g["d_o3"][g["o3"] == 0] == 0).all()) and bool((g["o3"] == 0).any())


def test_geometry_mirrors_at_known_batches():
    # wgrad_bf16_splits: E2 at 64 x 64 has four 256-pixel tiles per image and 256 splits; E3 one tile per image and 64 splits; E4 four images
    # per tile and 16 splits; D0 eight images per tile and 16 splits
    assert T.wgrad_geometry(1, 64, 37)[:3] == (148, 148, 1)
    assert T.wgrad_geometry(1, 64, 130)[:3] == (520, 174, 3)
    assert T.wgrad_geometry(2, 64, 65)[:3] == (65, 33, 2)
    assert T.wgrad_geometry(3, 64, 65) == (17, 9, 2, 4)
    assert T.wgrad_geometry(4, 64, 129) == (17, 9, 2, 8)
    assert [T.wgrad_two_tile_batch(l, 64) for l in (1, 2, 3, 4)] == [130, 65, 65, 129]
    # the up-conv splits follow the device: 256 compute units give 64 / 256 / 512 splits for D1 / D2 / D3
    assert [T.wgrad_two_tile_batch(l, 64, 256) for l in (5, 6, 7)] == [257, 257, 257]
    assert T.wgrad_geometry(5, 64, 257, 256) == (65, 33, 2, 4)
    assert T.wgrad_two_tile_batch(5, 64, 128) < 257
    for W in (64, 128):
        for layer in range(1, 8):
            B = T.wgrad_two_tile_batch(layer, W)
            tiles, S, tps, imgs = T.wgrad_geometry(layer, W, B)
            assert tps >= 2 and (S - 1) * tps < tiles <= S * tps
    # run_big: E2 forward, eight tiles (one image at 64 x 64) per item, two channel halves; E4 forward, four tiles of two images
    assert T.big_geometry(1, 64, False, 5) == (40, 5, 8, 2, 16)
    assert T.big_geometry(3, 64, False, 9) == (5, 2, 4, 2, 16)
    assert T.big_geometry(3, 64, False, 37, maxwg=8) == (19, 5, 4, 2, 8)
    assert T.big_geometry(2, 128, True, 3)[:3] == (24, 3, 8)


def test_weight_gradient_reference_is_sensitive_to_one_tile_and_to_one_pixel():
    """A property of the REFERENCE only (no kernel runs here, and this says nothing about which tiles a kernel walks): on the dense
    operands of E3's two-tiles-per-split batch at 64 x 64 (a tile is one image), the float64 weight gradient without the last tile of
    every two-tile split differs from the full one in nearly every element, and with a single pixel of one tile left out it still
    differs in nearly every element, by at most one product (4).  So no tile and no pixel can go missing behind the equality of the GPU
    case; that the GPU case's splits do walk two tiles is held to the launcher's own plan there (cvae_op_conv_wgrad_plan)."""
    layer, W = 2, 64
    B = T.wgrad_two_tile_batch(layer, W)
    tiles, S, tps, imgs = T.wgrad_geometry(layer, W, B)
    assert (tiles, tps, imgs) == (B, 2, 1)
    c = T.case_operands(layer, W, B, "wgrad")
    keep = [t for t in range(tiles) if not (t % tps == tps - 1 and t // tps < S and min((t // tps + 1) * tps, tiles) - (t // tps) * tps > 1)]
    assert len(keep) == tiles - (S - 1)
    mut = T.conv_wgrad_ref(layer, c["x"][keep], c["dout"][keep])[0]
    diff = (mut - c["ref_w"]).abs()
    assert float((diff != 0).double().mean()) > 0.95
    x1 = c["x"].clone()
    x1[1, :, 7, 9] = 0
    d1 = (T.conv_wgrad_ref(layer, x1, c["dout"])[0] - c["ref_w"]).abs()
    assert 0 < float(d1.max()) <= 4 and float((d1 != 0).double().mean()) > 0.95


def test_partial_rows_add_up_to_the_batch_statistics():
    y = T.case_operands(3, 64, 5, "fwd")["ref"]          # E4 at 64 x 64: two images per tile, four tiles per row: the last row holds one image
    S, m2, cnt, Q = T.partial_rows(y, 4)
    assert S.shape == (1, 256)
    assert cnt.tolist() == [5 * 64.0]
    S, m2, cnt, Q = T.partial_rows(T.case_operands(3, 64, 9, "fwd")["ref"], 4)
    assert cnt.tolist() == [512.0, 64.0]
    y = T.case_operands(3, 64, 9, "fwd")["ref"]
    v = y.permute(1, 0, 2, 3).reshape(256, -1)
    assert torch.equal(S.sum(0), v.sum(1)) and torch.equal(Q.sum(0), (v * v).sum(1))
    assert torch.allclose(m2[0], ((y[:8] - y[:8].mean(dim=(0, 2, 3), keepdim=True)) ** 2).sum(dim=(0, 2, 3)), rtol=1e-12)
    assert float(T.ulp32(torch.tensor([1.0, 3.0, 2.0 ** 23, 2.0 ** 24 - 1], dtype=torch.float64))[2]) == 1.0
    assert T.ulp32(torch.tensor([1.0], dtype=torch.float64)).item() == 2.0 ** -23
