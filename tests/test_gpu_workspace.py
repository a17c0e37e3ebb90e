"""No kernel may read workspace, scratch or output memory that was not written earlier in the same call sequence.

Every buffer the library works in is the caller's and comes from torch.empty (include/cvae.h: their contents on entry do not matter), and
the workspace holds many slots whose extent moves with the batch: split-K slabs, BatchNorm partials, reduction partials, the MS-SSIM
per-plane partials and its arrival ticket.  A consumer that reads one slab, tile or partial more than its producer wrote goes unnoticed
when the memory still holds the right values of the previous run at the same shape, which is what the caching allocator hands back to a
test that builds a fresh model per batch size.  Here every buffer is filled with a pattern first (ws_tools.poison): zeros, the largest
finite value (3.39e38 as fp32 and as each bf16 half: ReLU and max-pool written with fmaxf or compares swallow a NaN, not this), and all
ones (a NaN in every float format, the largest unsigned for the ticket).  Results are compared bit for bit through integer views, NaNs
included; one fill of each case is also held to the oracle or to the stored-operand check, so the runs are right and not merely equal.
An element that comes back the same under all three fills was written: that is the "fully written" check of the outputs."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from critic_vae_amd import lib as cvlib
from critic_vae_amd import segment as seg
from critic_vae_amd import synth
from oracle import cvae_oracle as orc
from decisions import check_step_against_oracle
from test_gpu_ops import LAYERS, dev, geom, handle, nhwc, rnd, wnat
from ws_tools import ALL_ONES, FILLS, HUGE, ZERO, StepRig, assert_same_outputs, check_bf16_stored_operands, holds, poison, same_bits

pytestmark = pytest.mark.gpu
TOL = 1e-4
CAP_ENV = "CVAE_PERSIST_MAXWG"


def _inputs(dseed, step, B, width=64):
    return tuple(torch.from_numpy(a).cuda() for a in synth.make_batch(dseed, step, B, width))


def _cpu(*ts):
    return tuple(t.cpu() for t in ts)


_rigs = {}


def rig(width, max_batch, precision):
    """One model, handle and set of buffers per (width, max_batch, precision), shared by the tests of this file: what the buffers hold
    from an earlier test is one more thing the results must not depend on."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    key = (width, max_batch, precision)
    if key not in _rigs:
        _rigs[key] = StepRig(width, max_batch, precision)
    return _rigs[key]


def _check_f32_against_oracle(r, B, x, pred, eps, out):
    """The bars of test_gpu_step.test_step_b256_fp32_against_oracle, on the step whose saved tensors the workspace holds."""
    xc, pc, ec = _cpu(x, pred, eps)
    rep, o = check_step_against_oracle(r.vae, xc, pc, ec, B, verbose=True)
    assert rep is not None, "seed must give a finite loss"
    assert (out["mu"].cpu() - o["mu"]).abs().max() < TOL and (out["logvar"].cpu() - o["logvar"]).abs().max() < TOL
    assert (out["recon"].cpu() - o["recon"]).abs().max() < TOL
    s = out["scalars"].cpu()
    assert abs(float(s[0]) - float(o["total_loss"].detach())) < TOL and abs(float(s[1]) - float(o["recon_loss"])) < TOL
    assert abs(float(s[2]) - float(o["KLD"])) < TOL
    assert (s[3:8] - o["ssim_levels"]).abs().max() < TOL and (s[8:13] - o["cs_levels"]).abs().max() < TOL
    assert rep["rel_forced"] <= 1e-4


# ---- 2. the whole step, every precision and width ----
# 64 x 64, B = 37 and 128 x 128, B = 5: ragged tiles in every kernel.  B = 133: ragged 128-row latent_gemm tiles and a second 64-image
# bgemm_f32 tile.  The oracle runs at B <= 37 (64 x 64) and B <= 5 (128 x 128) only.
STEP_CASES = [(p, 64, 37) for p in ("f32", "bf16", "bf16x9", "bf16x6")] + [(p, 128, 5) for p in ("f32", "bf16", "bf16x9", "bf16x6")] \
    + [("f32", 64, 133), ("bf16", 64, 133)]
step_cases = pytest.mark.parametrize("precision,W,B", STEP_CASES, ids=[f"{p}-w{w}-b{b}" for p, w, b in STEP_CASES])


@step_cases
def test_step_does_not_depend_on_buffer_contents(precision, W, B):
    """forward(train) + loss + backward(zero_padding) with the whole workspace and every output filled with each pattern first, nothing
    touched between the three calls (the workspace carries the saved activations): mu, logvar, recon, the 13 documented scalars, d_recon,
    d_mu, d_logvar, the running statistics and the WHOLE gradient buffer, padding included (it comes back 0), bit-identical across the
    fills.  The last (all-ones) run is then checked: f32 against the oracle at the bars of test_gpu_step, bf16 link by link against its
    stored operands."""
    r = rig(W, B, precision)
    x, pred, eps = _inputs(1234, 0, B, W)
    outs = {}
    for name, pat in FILLS:
        r.poison(pat)
        outs[name] = r.step(B, x, pred, eps, zero_padding=True)
        assert torch.isfinite(outs[name]["scalars"]).all(), (name, outs[name]["scalars"])
        assert not bool(outs[name]["grads"][~r.used].any()), f"{name}: the gradient padding is not zero"
        if pat == HUGE:                       # said directly, for the two outputs with layout of their own
            assert not bool(holds(outs[name]["scalars"], HUGE).any()), "a documented scalar was not written"
            assert not bool(holds(outs[name]["grads"], HUGE).any()), "a gradient element was not written"
    for name, _ in FILLS[1:]:
        assert_same_outputs(outs[name], outs["zero"], f"{name} fill vs zero fill")
    assert torch.isfinite(outs["zero"]["grads"]).all()
    if precision == "f32" and B <= 37:
        _check_f32_against_oracle(r, B, x, pred, eps, outs["ones"])
    if precision == "bf16":
        t0 = time.perf_counter()
        worst = check_bf16_stored_operands(r.h, r, B, x, pred, eps, r.theta, r.bn0, r.vae.bn_state)
        print(f"{precision} W={W} B={B}: stored-operand check {time.perf_counter() - t0:.1f} s, worst err / allowed {max(worst.values()):.2e}")


@step_cases
def test_step_without_padding_zeroing_leaves_the_padding_alone(precision, W, B):
    """backward(zero_padding=False) (cvae_backward): the gradient values are those of the zeroing form, under every fill, and the
    alignment padding between the tensors still holds what the caller put there (include/cvae.h: never touched)."""
    r = rig(W, B, precision)
    x, pred, eps = _inputs(1234, 0, B, W)
    r.poison(ZERO)
    want = r.step(B, x, pred, eps, zero_padding=True)
    for name, pat in FILLS:
        r.poison(pat)
        got = r.step(B, x, pred, eps, zero_padding=False)
        assert_same_outputs(got, want, f"{name} fill, no padding zeroing", skip=("grads",))
        assert same_bits(got["grads"][r.used], want["grads"][r.used]), f"{name}: gradient values differ"
        assert not r.padding_written(got["grads"], pat), f"{name}: the gradient padding was written behind {r.padding_written(got['grads'], pat)}"
        assert bool(holds(got["grads"][~r.used], pat).all()), f"{name}: the gradient padding was written"


EVAL_CASES = [(p, w) for p in ("f32", "bf16") for w in (64, 128)]


@pytest.mark.parametrize("precision,W", EVAL_CASES, ids=[f"{p}-w{w}" for p, w in EVAL_CASES])
def test_eval_forward_and_decode_do_not_depend_on_buffer_contents(precision, W):
    """forward(train=False) and the stand-alone decode at B = 5 under the three fills: mu, logvar and recon bit-identical, the running
    statistics untouched.  The eval-mode encoder is held to the oracle's (running statistics of one training step on both sides) and, in
    f32, the decode to the oracle's decoder; bf16 mode at its documented output bound (3e-2, test_gpu_bf16)."""
    B = 5
    r = rig(W, B, precision)
    r.poison(HUGE)
    r.step(B, *_inputs(1234, 0, B, W))                       # one training step: running statistics away from (0, 1)
    bn = r.vae.bn_state.clone()
    p = orc.to_torch(synth.make_params(0, W), requires_grad=True)
    bn_o = orc.new_bn_state(p)
    orc.train_step(p, *_cpu(*_inputs(1234, 0, B, W)), bn_state=bn_o)
    x, pred, eps = _inputs(1234, 1, B, W)
    zcat = torch.cat((torch.from_numpy(synth.normal(3, "ws/z", (B, 32))), torch.from_numpy(synth.uniform(3, "ws/p", (B, 1)))), 1).cuda()
    fwd, dec = {}, {}
    for name, pat in FILLS:
        r.poison(pat)
        r.h.forward(B, x, pred, eps, r.theta, r.vae.bn_state, r.mu, r.logvar, r.recon, r.ws, train=False)
        torch.cuda.synchronize()
        fwd[name] = {k: getattr(r, k)[:B].clone() for k in ("mu", "logvar", "recon")}
        assert torch.equal(r.vae.bn_state, bn), "eval mode changed the running statistics"
        r.poison(pat)
        r.h.decode(B, zcat, r.theta, r.recon, r.ws)
        torch.cuda.synchronize()
        dec[name] = {"recon": r.recon[:B].clone()}
    for name, _ in FILLS[1:]:
        assert_same_outputs(fwd[name], fwd["zero"], f"eval forward, {name} fill vs zero fill")
        assert_same_outputs(dec[name], dec["zero"], f"decode, {name} fill vs zero fill")
    tol = TOL if precision == "f32" else 3e-2
    with torch.no_grad():
        mu_o, lv_o = orc.encoder(p, x.cpu(), bn_o, train=False)
        assert (fwd["zero"]["mu"].cpu() - mu_o).abs().max() < tol and (fwd["zero"]["logvar"].cpu() - lv_o).abs().max() < tol
        z_o = orc.reparametrize(mu_o, lv_o, eps.cpu())
        assert (fwd["zero"]["recon"].cpu() - orc.decoder(p, z_o, pred.cpu())).abs().max() < tol
        assert (dec["zero"]["recon"].cpu() - orc.decoder(p, zcat[:, :32].cpu(), zcat[:, 32:].cpu())).abs().max() < tol


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_staged_step_does_not_depend_on_buffer_contents(precision):
    """One rank's staged step (forward stages 0..4, loss 0..1, backward 0..4, no exchange; test_gpu_sync_stats) with workspace, outputs
    and the fp64 sync record under the three fills: bit-identical, and the single-call step as that file requires.  The stages leave
    the gradient padding alone, as cvae_backward does."""
    W, B = 64, 37
    r = rig(W, B, precision)
    x, pred, eps = _inputs(1234, 0, B, W)
    r.poison(ZERO)
    want = r.step(B, x, pred, eps, zero_padding=False)
    for name, pat in FILLS:
        r.poison(pat)
        got = r.staged(B, x, pred, eps)
        assert_same_outputs(got, want, f"staged step, {name} fill, vs the single-call step", skip=("grads",))
        assert same_bits(got["grads"][r.used], want["grads"][r.used]), f"{name}: gradient values differ"
        assert not r.padding_written(got["grads"], pat), f"{name}: the gradient padding was written behind {r.padding_written(got['grads'], pat)}"
        assert bool(holds(got["grads"][~r.used], pat).all()), f"{name}: the gradient padding was written"


# ---- 3. batch sequences on one handle and one workspace ----
# the training loop keeps the ragged tail batch: full batch, tail, full batch on one handle, and every workspace offset moves with B
SEQ_CASES = [("f32", 64, 133, (133, 5, 133, 37, 1, 133)), ("bf16", 64, 133, (133, 5, 133, 37, 1, 133)), ("f32", 128, 37, (37, 3, 37))]
ORACLE_MAX_B = {64: 37, 128: 5}


@pytest.mark.parametrize("precision,W,max_batch,seq", SEQ_CASES, ids=[f"{p}-w{w}" for p, w, _, _ in SEQ_CASES])
def test_batch_sequence_on_one_workspace(precision, W, max_batch, seq):
    """Steps of different batch sizes, one after the other, nothing cleared in between (the running statistics move on, as in training):
    each step's outputs are bit for bit those of the same handle running that batch alone, from the same running statistics, on a
    zero-filled and on an all-ones workspace; the small f32 steps also meet the oracle.  At 64 x 64 the last step repeats the first
    one's inputs and must repeat its results."""
    r = rig(W, max_batch, precision)
    base = 10 if W == 64 else 20
    batches = [_inputs(1234, base + i, B, W) for i, B in enumerate(seq)]
    if W == 64:
        batches[-1] = batches[0]
    r.poison(HUGE)                                           # once, before the first step
    bn, bns, outs = r.bn0.clone(), [], []
    for B, (x, pred, eps) in zip(seq, batches):
        bns.append(bn)
        outs.append(r.step(B, x, pred, eps, bn=bn))
        bn = outs[-1]["bn_state"]
    for i, (B, (x, pred, eps)) in enumerate(zip(seq, batches)):
        assert torch.isfinite(outs[i]["scalars"]).all() and torch.isfinite(outs[i]["grads"]).all(), i
        for name, pat in (("zero", ZERO), ("ones", ALL_ONES)):
            r.poison(pat)
            alone = r.step(B, x, pred, eps, bn=bns[i])
            assert_same_outputs(outs[i], alone, f"step {i} (B = {B}) of the sequence vs alone on a {name}-filled workspace")
        if precision == "f32" and B <= ORACLE_MAX_B[W]:
            _check_f32_against_oracle(r, B, x, pred, eps, alone)
    if W == 64:
        assert_same_outputs(outs[-1], outs[0], "the third 133 step on the first one's inputs", skip=("bn_state",))


def test_under_a_grid_cap_the_persistent_kernels_walk_poisoned_slabs():
    """A child process caps every persistent grid at 8 workgroups (CVAE_PERSIST_MAXWG, read once per process) and reruns the f32 step at
    64 x 64, B = 37 and the 128 x 128 sequence 37, 3, 37: every persistent kernel then walks several items with its slabs poisoned."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{CAP_ENV: "8"})
    sel = "(test_step_does_not_depend_on_buffer_contents and f32-w64-b37) or (test_batch_sequence_on_one_workspace and f32-w128)"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", sel],
                       env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-1000:]
    assert re.search(r"\b2 passed\b", p.stdout) and "failed" not in p.stdout, p.stdout[-1000:]


# ---- 4. per-op entry points ----
OP_SHAPES = [(64, 3), (64, 37), (128, 3)]
op_shapes = pytest.mark.parametrize("W,B", OP_SHAPES, ids=[f"w{w}-b{b}" for w, b in OP_SHAPES])


def _under_fills(run, bufs, part=None):
    """run() under each fill of the tensors in `bufs` (scratch and outputs; a dict by name): every one of them bit-identical afterwards,
    except the working memory (names that start with "scratch": only what it leads to counts).  part: {name: the slice that counts}."""
    res = {}
    for name, pat in FILLS:
        for t in bufs.values():
            poison(t, pat)
        run()
        torch.cuda.synchronize()
        res[name] = {k: (part or {}).get(k, slice(None)) for k in bufs if not k.startswith("scratch")}
        res[name] = {k: bufs[k][sl].clone() for k, sl in res[name].items()}
    for name, _ in FILLS[1:]:
        assert_same_outputs(res[name], res["zero"], f"{name} fill vs zero fill")
    return res["zero"]


def _empty(n, dtype=torch.float32):
    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda")


@op_shapes
def test_conv_ops_do_not_depend_on_scratch_partials_or_outputs(W, B):
    """op_conv_fwd (all nine layers, with the BatchNorm partials of the encoder layers), op_conv_dgrad (1..7), op_conv_wgrad (0..7) and
    op_d4_bwd with the scratch, the partials and every output under the three fills.  At B = 3 also layers 1..4 on handles of the two
    fp32-emulation modes, whose ops run the step's split-operand kernels: the packed weights and D0's split-K slabs sit in the scratch;
    and layers 1..8 and op_d4_bwd on a bf16 handle, whose ops run the step's bf16 kernels on bf16 activations."""
    _conv_ops_under_fills(handle(W, B), W, B, range(9))
    if B == 3:
        for mode in ("bf16x9", "bf16x6"):
            _conv_ops_under_fills(cvlib.Handle(W, B, precision=mode), W, B, range(1, 5))
        # a bf16 handle: layers 1..8 on the step's bf16 kernels, activations and their gradients as bf16 (layer 0's weight gradient is the
        # fp32 kernel there too and is covered above); the packed and collapsed weights, D0's slabs and the weight-gradient slabs sit in the scratch
        Hb = cvlib.Handle(W, B, precision="bf16")
        _conv_ops_under_fills(Hb, W, B, range(1, 9), bf16=True)
        _d4_bwd_under_fills(Hb, W, B, bf16=True)
    _d4_bwd_under_fills(handle(W, B), W, B)


def _as_bf16(t):
    """A device fp32 tensor -> its bf16 rounding, as the fp32 tensor that holds it (two elements per float)."""
    return t.to(torch.bfloat16).reshape(-1).view(torch.float32)


def _conv_ops_under_fills(H, W, B, layers, bf16=False):
    for layer in layers:
        cin, cout, h, up, hs = geom(layer, W)
        x, w, b = rnd(f"x{layer}", (B, cin, hs, hs)), rnd(f"w{layer}", (cout, cin, 5, 5), -0.1, 0.1), rnd(f"b{layer}", (cout,))
        dout = rnd(f"do{layer}", (B, cout, h, h))
        xin, wn, bd, dn = (dev(x) if layer == 0 else nhwc(x)), wnat(w), dev(b), (dev(dout) if layer == 8 else nhwc(dout))
        mask = torch.relu(xin) if up else None
        per = 1           # elements per float of the activation tensors
        if bf16:          # activations and activation gradients (the ReLU mask source among them) in bf16 storage; recon and d_recon stay fp32
            per = 2
            xin, dn, mask = _as_bf16(xin), (dn if layer == 8 else _as_bf16(dn)), (_as_bf16(mask) if up else None)
        bufs = {"out": _empty(B * h * h * cout // (1 if layer == 8 else per)), "scratch": _empty(H.op_scratch_floats(B))}
        part = None
        if layer < 4:
            bufs["partials"] = _empty(H.op_bn_partial_floats(layer, B))
            # a partial row of the big-tile bf16 kernels covers several tiles: [S | M2] of ceil(tiles / that) rows at the front of the buffer
            tiles, tpp = bufs["partials"].numel() // (2 * cout), H.op_conv_tiles_per_partial(layer, B)
            part = {"partials": slice(0, 2 * -(-tiles // tpp) * cout)}
        _under_fills(lambda: H.op_conv_fwd(layer, B, xin, wn, bd, bufs["out"], bufs.get("partials"), bufs["scratch"]), bufs, part)
        if 1 <= layer <= 7:
            bufs = {"din": _empty(B * hs * hs * cin // per), "scratch": _empty(H.op_scratch_floats(B))}
            _under_fills(lambda: H.op_conv_dgrad(layer, B, dn, wn, mask, bufs["din"], bufs["scratch"]), bufs)
        if layer <= 7:
            bufs = {"dw": _empty(25 * cin * cout), "scratch": _empty(H.op_scratch_floats(B))}
            if layer >= 4:
                bufs["dbias"] = _empty(cout)
            _under_fills(lambda: H.op_conv_wgrad(layer, B, xin, dn, bufs["dw"], bufs.get("dbias"), bufs["scratch"]), bufs)


def _d4_bwd_under_fills(H, W, B, bf16=False):
    o3 = torch.relu(nhwc(rnd("pre8", (B, 32, W // 2, W // 2))))
    d_recon, recon, w8 = dev(rnd("dr8", (B, 3, W, W))), dev(rnd("rc8", (B, 3, W, W), -0.9, 0.9)), wnat(rnd("w8", (3, 32, 5, 5), -0.1, 0.1))
    bufs = {"dout": _empty(B * 3 * W * W), "d_o3": _empty(B * 32 * (W // 2) ** 2 // (2 if bf16 else 1)), "dw": _empty(2400), "db": _empty(3),
            "scratch": _empty(H.op_scratch_floats(B))}
    if bf16:        # o3 / d_o3 in bf16; the Tanh backward runs inside the kernel and no dOut tensor is written
        o3 = _as_bf16(o3)
        del bufs["dout"]
    _under_fills(lambda: H.op_d4_bwd(B, o3, d_recon, recon, w8, bufs.get("dout"), bufs["d_o3"], bufs["dw"], bufs["db"], bufs["scratch"]), bufs)


@op_shapes
def test_bn_pool_act_ops_do_not_depend_on_scratch_partials_or_outputs(W, B):
    """op_bn_pool_act_fwd and op_bn_pool_act_bwd of the four encoder blocks: scratch, coef and every output under the three fills (the
    partials are op_conv_fwd's, written into a poisoned buffer each time; the running statistics are state and start from (0, 1))."""
    H = handle(W, B)
    for layer in range(4):
        cin, C, h, _, _ = geom(layer, W)
        x, w, b = rnd(f"bx{layer}", (B, cin, h, h)), rnd(f"bw{layer}", (C, cin, 5, 5), -0.1, 0.1), rnd(f"bb{layer}", (C,))
        gamma, beta, da = dev(rnd(f"g{layer}", (C,), 0.5, 1.5)), dev(rnd(f"be{layer}", (C,), -0.5, 0.5)), nhwc(rnd(f"da{layer}", (B, C, h // 2, h // 2)))
        xin, wn, bd = (dev(x) if layer == 0 else nhwc(x)), wnat(w), dev(b)
        f = {"y": _empty(B * h * h * C), "partials": _empty(H.op_bn_partial_floats(layer, B)), "coef": _empty(C * 4),
             "a": _empty(B * (h // 2) ** 2 * C), "run_mean": _empty(C), "run_var": _empty(C), "scratch": _empty(H.op_scratch_floats(B))}

        def fwd():
            H.op_conv_fwd(layer, B, xin, wn, bd, f["y"], f["partials"], f["scratch"])
            f["run_mean"].zero_()
            f["run_var"].fill_(1.0)
            H.op_bn_pool_act_fwd(layer, B, f["y"], f["partials"], gamma, beta, f["run_mean"], f["run_var"], f["coef"], f["a"], f["scratch"], True)

        _under_fills(fwd, f)
        g = {"dy": _empty(B * h * h * C), "dgamma": _empty(C), "dbeta": _empty(C), "dbias": _empty(C), "scratch": _empty(H.op_scratch_floats(B))}
        _under_fills(lambda: H.op_bn_pool_act_bwd(layer, B, f["y"], f["a"], da, f["coef"], gamma, g["dy"], g["dgamma"], g["dbeta"], g["dbias"],
                                                  g["scratch"]), g)


@op_shapes
def test_msssim_op_does_not_depend_on_workspace_scalars_or_gradient(W, B):
    """op_msssim: its workspace (per-plane partials, the arrival ticket the level-0 kernel zeroes a launch ahead), the scalars and the
    gradient under the three fills; the 13 documented scalars and every gradient element bit-identical."""
    H = handle(W, B)
    b = torch.from_numpy(synth.uniform(5, f"ws/ms/{W}/b", (B, 3, W, W)))
    a = 0.7 * b + 0.3 * torch.from_numpy(synth.uniform(5, f"ws/ms/{W}/a", (B, 3, W, W)))
    a, b = dev(a), dev(b)
    bufs = {"scratch": _empty(H.op_msssim_ws_floats(B)), "scalars": _empty(16), "d_img1": _empty(B * 3 * W * W)}
    out = _under_fills(lambda: H.op_msssim(B, a, b, bufs["scratch"], bufs["scalars"], bufs["d_img1"]), bufs, part={"scalars": slice(0, 13)})
    assert torch.isfinite(out["scalars"]).all() and torch.isfinite(out["d_img1"]).all()


def test_dense_crf_does_not_depend_on_its_scratch(golden_dir):
    """cvae_dense_crf at B = 3 on the real fixture frames of test_gpu_segment, scratch and outputs under the three fills: labels and q1
    bit-identical."""
    B = 3
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"][:B]
    g = u8.astype(np.int32)
    masks = ((g[..., 0] > g[..., 1]) & (g[..., 0] > 40)).astype(np.float32)
    h = cvlib.Handle(64, 1)
    frames, prob1 = torch.from_numpy(u8).cuda(), torch.from_numpy(masks).cuda()
    bufs = {"labels": _empty(B * 64 * 64, torch.uint8), "q1": _empty(B * 64 * 64), "scratch": _empty(h.crf_scratch_bytes(B), torch.uint8)}
    out = _under_fills(lambda: h.dense_crf(B, frames, prob1, seg.crf_params(), bufs["labels"], bufs["q1"], bufs["scratch"]), bufs)
    assert torch.isfinite(out["q1"]).all() and bool((out["labels"] <= 1).all()) and 0 < int(out["labels"].sum()) < B * 64 * 64


def test_poison_fills_every_byte_of_any_dtype():
    """The helper itself: every dtype the buffers have, sizes that are no multiple of four bytes, and what each pattern reads as."""
    for dtype, n in ((torch.float32, 7), (torch.float64, 3), (torch.bfloat16, 6), (torch.uint8, 13), (torch.int64, 2)):
        t = torch.zeros(n, dtype=dtype, device="cuda")
        poison(t, 0x7F7F7F7F)
        assert bool((t.view(torch.uint8) == 0x7F).all()), dtype
        poison(t, 0x04030201)
        assert t.view(torch.uint8).cpu().tolist() == [1 + k % 4 for k in range(n * t.element_size())], dtype
    f, d, b = torch.empty(4, device="cuda"), torch.empty(4, dtype=torch.float64, device="cuda"), torch.empty(4, dtype=torch.bfloat16, device="cuda")
    for t in (f, d, b):
        assert torch.isnan(poison(t, ALL_ONES)).all()
        assert torch.isfinite(poison(t, HUGE)).all() and bool((t.double() > 3e38).all())
        assert bool((poison(t, ZERO) == 0).all())
    assert bool(holds(poison(f, HUGE), HUGE).all()) and same_bits(poison(f, ALL_ONES), poison(f.clone(), ALL_ONES))
