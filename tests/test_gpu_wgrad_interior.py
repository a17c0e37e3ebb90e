"""fp32 conv weight gradients where the kernels leave the padding tests out (conv_wgrad.hip: wgrad_interior_row).

An interior image row (2 <= gy <= H-3) runs as one untested straight line that skips, by construction, the MFMAs the tested
form skips on the row's first and last pixel pair.  With `in` and `dout` all ones every weight gradient is the NUMBER of
(image, pixel) pairs its tap reaches inside the image, an integer below 2^24 and therefore exact in fp32 whatever the order of
summation: one MFMA wrongly skipped or added changes it.  The cases take every path of the split:

* 64 x 64, B = 3, layers 1..7: H = 32, 16 (interior rows on the untested line), H = 8, 4 (tested loop only); three images
  leave a ragged image group in the 2-image tiles of H = 8 and the 8-image tiles of H = 4 (whose tile staging works its
  addresses out per tile); layers 5..7 are the phase-collapsed up-sampling kernels;
* 128 x 128, B = 2, layer 1: H = 64 has two x-tiles per row, so the first pixel pair of a row is in one tile and the last
  in the other;
* 64 x 64, layer 1, B = 17 and B = 33: layer 1 has 2 workgroups per split and hence at most 256 splits of its B * 8
  128-pixel tiles (wgrad_splits), so B = 33 is the smallest batch at which a workgroup walks two tiles (asserted below);
  B = 17 is kept beside it as the largest case of one tile per split that the 8-tile images leave ragged against the grid.

All through cvae_op_conv_wgrad, against the oracle's conv weight gradient in float64 with the tolerance of
tests/test_gpu_ops.py::test_conv_wgrad."""
import functools

import pytest
import torch

from oracle import cvae_oracle as orc
from test_gpu_ops import check, f64, geom, handle, nhwc, rnd, wref

pytestmark = pytest.mark.gpu

CASES = [(64, 3, layer) for layer in range(1, 8)] + [(128, 2, 1), (64, 17, 1), (64, 33, 1)]
cases = pytest.mark.parametrize("W,B,layer", CASES, ids=[f"w{w}-b{b}-L{l}" for w, b, l in CASES])


def inputs(W, B, layer, ones):
    cin, cout, h, up, hs = geom(layer, W)
    if ones:
        return torch.ones(B, cin, hs, hs), torch.ones(B, cout, h, h)
    return rnd(f"x{layer}", (B, cin, hs, hs)), rnd(f"do{layer}", (B, cout, h, h))


@functools.lru_cache(maxsize=None)
def reference(W, B, layer, ones):
    """(dW as OIHW, dbias) of the oracle's convolution in float64; computed once per case, never modified."""
    cin, cout, h, up, hs = geom(layer, W)
    x, dout = inputs(W, B, layer, ones)
    w = torch.zeros(cout, cin, 5, 5, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    orc.conv5x5(f64(x), w, b, upsample_input=bool(up)).backward(f64(dout))
    return w.grad.detach(), b.grad.detach()


def run(W, B, layer, ones):
    """(dW as OIHW, dbias) of the library, on the CPU."""
    H = handle(W, B)
    cin, cout, h, up, hs = geom(layer, W)
    x, dout = inputs(W, B, layer, ones)
    dw = torch.full((25 * cin * cout,), float("nan"), device="cuda")
    dbias = torch.full((cout,), float("nan"), device="cuda")
    sc = torch.empty(H.op_scratch_floats(B), device="cuda")
    H.op_conv_wgrad(layer, B, nhwc(x), nhwc(dout), dw, dbias, sc)
    torch.cuda.synchronize()
    return wref(dw, cin, cout), dbias.cpu()


@functools.lru_cache(maxsize=None)
def result(W, B, layer, ones):
    return run(W, B, layer, ones)


def test_b33_walks_two_tiles_per_split():
    """The arithmetic of wgrad_splits (conv_wgrad.hip) for layer 1 at 64 x 64: 8 tiles per 32 x 32 image, 512 / 2 = 256 splits."""
    def tiles_per_split(B):
        tiles, S = B * 8, min(512 // 2, B * 8)
        return -(-tiles // S)
    assert tiles_per_split(17) == 1 and tiles_per_split(32) == 1 and tiles_per_split(33) == 2


@cases
def test_tap_counts_exact(W, B, layer):
    cin, cout, h, up, hs = geom(layer, W)
    dw, dbias = result(W, B, layer, True)
    want_w, want_b = reference(W, B, layer, True)
    assert want_w.max().item() <= 2 ** 24 and torch.equal(want_w, want_w.round())
    if not up:          # closed form: tap (r, s) reaches (H - |r-2|) x (H - |s-2|) pixels of every image
        n = torch.tensor([h - abs(r - 2) for r in range(5)], dtype=torch.float64)
        assert torch.equal(want_w, (B * n[:, None] * n[None, :]).expand(cout, cin, 5, 5))
    bad = (dw.double() != want_w).nonzero()
    assert bad.numel() == 0, (f"L{layer} {W}x{W} B={B}: {bad.shape[0]} weight gradients differ from their tap count, first (co, ci, r, s) = "
                              f"{bad[0].tolist()}: got {dw[tuple(bad[0])].item()}, want {want_w[tuple(bad[0])].item()}")
    assert torch.equal(dbias.double(), torch.full((cout,), float(B * h * h), dtype=torch.float64)), dbias
    assert torch.equal(want_b, torch.full((cout,), float(B * h * h), dtype=torch.float64))


@cases
def test_random_against_oracle(W, B, layer):
    dw, dbias = result(W, B, layer, False)
    want_w, want_b = reference(W, B, layer, False)
    check(dw, want_w, f"conv_wgrad L{layer}", rel=True)
    check(dbias, want_b, f"conv dbias L{layer}", rel=True)


@cases
def test_two_runs_bitwise_equal(W, B, layer):
    dw, dbias = result(W, B, layer, False)
    dw2, dbias2 = run(W, B, layer, False)
    assert torch.equal(dw, dw2) and torch.equal(dbias, dbias2)
