"""Host checks of the BatchNorm / pool helpers of ws_tools that tests/test_gpu_bn_ops.py stands on: the launch geometry against the
numbers worked out by hand from bn.hip / reduce.hip, the synthesised partials against a plain variance, and the generated inputs
against the properties the float64 reference relies on."""
import pytest
import torch

from ws_tools import (BN_CASES, U32, bn_assert_edge, bn_bwd_blocks, bn_bwd_chain, bn_bwd_ppb, bn_case_batch, bn_facts, bn_fwd_chunks,
                      bn_fwd_ref, bn_gen_params, bn_gen_y, bn_layer, bn_num_tiles, bn_part_geom, bn_stats_ref, bn_sweep_items, bn_windows,
                      synth_bn_partials)


def test_partial_geometry_restates_part_geom():
    assert bn_part_geom(0, 64) == (1, 512, 8) and bn_part_geom(0, 128) == (1, 512, 32)
    assert bn_part_geom(1, 32) == (1, 128, 8)            # TW 32, TH 4
    assert bn_part_geom(2, 16) == (1, 128, 2)            # TW 16, TH 8
    assert bn_part_geom(3, 8) == (2, 64, 1)              # two whole images per tile
    assert bn_part_geom(3, 16) == (1, 128, 2) and bn_part_geom(1, 64) == (1, 128, 32)
    for layer, per_image in ((0, 8), (1, 8), (2, 2)):
        assert bn_num_tiles(layer, bn_layer(layer, 64)[1], 5) == 5 * per_image
    assert [bn_num_tiles(3, 8, B) for B in (1, 2, 3, 63, 65, 513)] == [1, 1, 2, 32, 33, 257]
    assert bn_fwd_chunks(32) == (1, 32) and bn_fwd_chunks(33) == (2, 17) and bn_fwd_chunks(257) == (9, 29)


def test_backward_blocks_restate_the_launcher():
    assert bn_bwd_blocks(16 * 32, 256) == 64 and bn_bwd_blocks(16 * 33, 256) == 66          # block 3 at 64 x 64: B = 32 / 33
    assert bn_bwd_blocks(1024 * 4, 32) == 64 and bn_bwd_blocks(1024 * 5, 32) == 80          # block 0: B = 4 / 5
    assert bn_bwd_blocks(16 * 513, 256) == 1024 and bn_bwd_ppb(16 * 513, 256) == 9 and 912 * 9 == 16 * 513
    assert bn_bwd_blocks(16, 256) == 2 and bn_bwd_blocks(3, 256) == 1
    assert bn_sweep_items(256) == 1048576
    f = bn_facts(64, 3, 513, False)
    assert (f["nblk"], f["ppb"], f["live"], f["tpb"], f["last_ni"]) == (1024, 9, 912, 9, 1)
    # chains: block 3, B = 33, fp32 Tanh statistics: 8 pixels on one thread, one LDS row, 66 rows -> rows_sum_kernel with 3 rows per chunk
    # (1 per row group + 8 LDS rows), then 22 rows over 16 lanes (2) and 4 shuffle levels
    assert bn_bwd_chain(66, 8, 256, 1, True) == 8 + 1 + (1 + 8) + (2 + 4)
    assert bn_bwd_chain(64, 8, 256, 1, True) == 8 + 1 + (4 + 4)
    assert bn_bwd_chain(66, 8, 256, 1, False, per_px=4) == 32 + 1 + (3 + 32)                # rows_sum_1024_kernel
    assert bn_bwd_chain(64, 64, 32, 4, True) == 2 + 32 + (4 + 4)                            # block 0 ReLU statistics: NSUB = 32


def test_derived_batches_at_256_compute_units():
    want = {(64, 3): {"n64": 1, "one-tile": 2, "rows64": 32, "rows65": 33, "tiles32": 63, "tiles33": 65, "wrap": 513},
            (64, 0): {"rows64": 4, "rows65": 5, "wrap": 33}, (64, 2): {"tiles32": 16, "tiles33": 17, "wrap": 129}, (64, 1): {"tiles33": 5}}
    sweep = {(0, "f32"): (32, 33), (0, "bf16"): (64, 65), (3, "f32"): (256, 257), (3, "bf16"): (512, 513)}
    seen = 0
    for W, layer, edge, modes in BN_CASES:
        for m in modes:
            B = bn_case_batch(W, layer, edge, m == "bf16", 256)
            bn_assert_edge(W, layer, edge, B, m == "bf16", 256)
            if W == 64:
                assert B == want[W, layer][edge], (W, layer, edge, m, B)
            else:
                assert B == sweep[layer, m][edge == "sweep"], (W, layer, edge, m, B)
            C, H = bn_layer(layer, W)
            assert B * H * H * C * (2 if m == "bf16" else 4) < 150e6, "a tensor of the case passes 150 MB"
            seen += 1
    assert seen == 2 * 14 + 2 * 4 + 1
    with pytest.raises(AssertionError):                  # a device with more compute units moves the sweep edge: the case must notice
        bn_assert_edge(128, 0, "sweep", 33, False, 304)


@pytest.mark.parametrize("layer,W,B", [(0, 64, 2), (1, 64, 3), (2, 64, 3), (3, 64, 5), (3, 64, 1), (3, 128, 2)])
def test_synthesised_partials_merge_to_the_variance(layer, W, B):
    g = torch.Generator().manual_seed(layer * 100 + B)
    y = bn_gen_y(g, layer, W, B, False)
    C, H = bn_layer(layer, W)
    part, s, m2, cnt = synth_bn_partials(y, layer, B, 2 * bn_num_tiles(layer, H, B) * C + 64)
    nt = bn_num_tiles(layer, H, B)
    assert s.shape == (nt, C) and float(cnt.sum()) == B * H * H
    assert torch.isnan(part[2 * nt * C:]).all() and torch.isfinite(part[:2 * nt * C]).all()
    assert torch.equal(part[:nt * C].double().view(nt, C), s) and torch.equal(part[nt * C:2 * nt * C].double().view(nt, C), m2)
    imgs, ppi, tpi = bn_part_geom(layer, H)
    img0 = (torch.arange(nt) // tpi) * imgs
    assert torch.equal(cnt, (torch.clamp(B - img0, max=imgs) * ppi).double()), "the counts are not the ones the kernel derives"
    N = cnt.sum()
    S = s.sum(0)
    var = (m2.sum(0) + (s * s / cnt[:, None]).sum(0) - S * S / N) / N                          # the Chan merge of bn_fwd_coef
    mu, v64, mb, vb = bn_stats_ref(y, s, m2, cnt)
    y64 = y.double().reshape(-1, C)
    assert torch.allclose(v64, y64.var(0, unbiased=False), rtol=1e-12) and torch.allclose(mu, y64.mean(0), rtol=1e-12, atol=1e-15)
    assert bool(((S / N - mu).abs() <= mb).all()) and bool(((var - v64).abs() <= vb).all())
    assert bool((vb <= 1e-6 * v64).all()), "the variance bound is no round-off bound"


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("layer", range(4))
def test_generated_inputs_keep_the_window_separation_and_the_gate_cap(layer, bf):
    W, B = 64, 3
    g = torch.Generator().manual_seed(layer)
    y = bn_gen_y(g, layer, W, B, bf)
    C, H = bn_layer(layer, W)
    gamma, beta, rm, rv = bn_gen_params(g, C)
    assert y.shape == (B, H, H, C) and float(y.abs().max()) < 2
    assert (0.5 <= gamma.abs()).all() and (gamma.abs() <= 1.5).all() and (gamma[::3] < 0).all() and (gamma[1::3] > 0).all()
    assert (beta.abs() <= 0.5).all() and (rm.abs() <= 0.3).all() and (rv >= 0.5).all() and (rv <= 1.5).all() and rm.abs().min() > 0
    if bf:
        assert torch.equal(y, y.to(torch.bfloat16).float()), "bf16 storage: y must be bf16-representable"
    yw = bn_windows(y.double(), B, H, C)
    srt = yw.sort(dim=3).values
    assert float((srt[:, :, :, 1:] - srt[:, :, :, :-1]).min()) >= 2.0 ** -6, "two values of a window are closer than 2^-6"
    # the float64 reference alone: the share of ReLU gates that a's own bound could flip stays under 1e-3, and the argmax is decided
    y64 = y.double().reshape(-1, C)
    istd = 1.0 / torch.sqrt(y64.var(0, unbiased=False) + 1e-5)
    sc = gamma.double() * istd
    coef = torch.stack((sc, beta.double() - y64.mean(0) * sc, y64.mean(0), istd), 1)
    want, bound, nw, pos = bn_fwd_ref(yw, coef, layer == 3, bf)
    top = nw.gather(3, pos)[:, :, :, 0]
    assert float((top.abs() <= bound).double().mean()) <= 1e-3
    n_srt = nw.sort(dim=3).values
    assert bool(((n_srt[:, :, :, 3] - n_srt[:, :, :, 2]) > 64 * U32 * nw.abs().max(dim=3).values).all())
