"""Every per-op conv entry point replays the step's link to the bit.

include/cvae.h promises that cvae_op_conv_fwd / dgrad / wgrad of layers 1..7 "run the kernels the step runs there".  The step and the
per-op entries choose their launcher in the same three dispatch functions over one table (api.hip), so a per-op call on the operands
the step left in its workspace must store the very words the step stored: the conv kernels contain no atomics and reduce their split-K
slabs in a fixed order, and carve gives every saved tensor its own range, so what is read back is what the kernels read.  Compared as
raw 32-bit words, so bf16 storage is compared as stored and a NaN would compare as the bits it is.

The odd batches leave a ragged last 128-pixel tile in E4 and D0 at 64 x 64 (5 images of 64 and 16 pixels); the table does not depend on
the batch."""
import pytest
import torch

from critic_vae_amd import synth
from bf16_ops_tools import geom
from ws_tools import ALL_ONES, StepRig, poison

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "bf16", "bf16x9", "bf16x6"]


def step_of(precision, W, B):
    """One forward + loss + backward through the Handle (no optimizer step: the replay needs the parameters the step used)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    rig = StepRig(W, B, precision)
    x, pred, eps = (torch.from_numpy(a).cuda() for a in synth.make_batch(11, 0, B, W))
    rig.step(B, x, pred, eps)
    return rig


def links(rig, layer, B):
    """The step's link of conv layer 1..7: (input, output, output gradient, input gradient, weights, bias, weight gradient, bias
    gradient), the activations as the workspace floats that hold them (bf16 storage: two elements per float)."""
    h, W = rig.h, rig.width
    cin, cout, ho, _, hi = geom(layer, W)
    per = 2 if rig.h.precision == "bf16" else 1
    n_in, n_out = B * hi * hi * cin // per, B * ho * ho * cout // per
    i = layer - 4
    src, dst = (f"a{layer - 1}", f"y{layer}") if layer < 4 else ("h" if i == 0 else f"o{i - 1}", f"o{i}")
    d_dst, d_src = (f"d_y{layer}", f"d_a{layer - 1}") if layer < 4 else (f"d_o{i}", "d_h" if i == 0 else f"d_o{i - 1}")
    name = f"enc{layer}" if layer < 4 else f"dec{i}"
    (ow, nw), (ob, nb) = h.layout[name + ".w"], h.layout[name + ".b"]
    view = lambda nm, n: h.ws_view(rig.ws, B, nm, n)
    return (view(src, n_in), view(dst, n_out), view(d_dst, n_out), view(d_src, n_in), rig.theta[ow:ow + nw], rig.theta[ob:ob + nb],
            rig.grads[ow:ow + nw], rig.grads[ob:ob + nb])


def fresh(like):
    return poison(torch.empty_like(like), ALL_ONES)          # a NaN in fp32 and in each bf16 half


def same_words(got, want, what):
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        f"{what}: {(got.view(torch.int32) != want.view(torch.int32)).sum().item()} of {got.numel()} words differ from the step's"


@pytest.mark.parametrize("W,B", [(64, 5), (128, 3)], ids=["w64-b5", "w128-b3"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_op_conv_entries_replay_the_steps_links_to_the_bit(precision, W, B):
    rig = step_of(precision, W, B)
    h = rig.h
    scratch = lambda: fresh(torch.empty(h.op_scratch_floats(B), device="cuda"))
    for layer in range(1, 8):
        x, y, dy, dx, w, b, dw, db = links(rig, layer, B)
        part = fresh(torch.empty(h.op_bn_partial_floats(layer, B), device="cuda")) if layer < 4 else None
        out = fresh(y)
        h.op_conv_fwd(layer, B, x, w, b, out, part, scratch())
        din = fresh(dx)
        h.op_conv_dgrad(layer, B, dy, w, x if layer >= 5 else None, din, scratch())      # D1..D3: the ReLU mask of their input
        gw, gb = fresh(dw), fresh(db)
        h.op_conv_wgrad(layer, B, x, dy, gw, gb, scratch())
        torch.cuda.synchronize()
        same_words(out, y, f"{precision} {W} x {W} B={B}: forward of layer {layer}")
        same_words(din, dx, f"{precision} {W} x {W} B={B}: input gradient of layer {layer}")
        same_words(gw, dw, f"{precision} {W} x {W} B={B}: weight gradient of layer {layer}")
        same_words(gb, db, f"{precision} {W} x {W} B={B}: bias gradient of layer {layer}")
