"""precision="bf16" (BASELINE.json configs 3-5): forward / input-gradient convs of E2..E4 and D0 on
the bf16 MFMA, everything else fp32.  bf16 operands carry 8 significant bits, so this mode is NOT
held to the 1e-4 fp32 bar; the tolerances below are what bf16 rounding of the conv operands gives
on the oracle's own fp32 result (measured margins ~3x)."""
import numpy as np
import pytest
import torch

from critic_vae_amd import synth

pytestmark = pytest.mark.gpu


def _oracle_step(B, seed=0, width=64):
    from oracle import cvae_oracle as orc
    params = synth.make_params(seed, width)
    x, pred, eps = synth.make_batch(1234, 0, B, width)
    p = orc.to_torch(params, requires_grad=True)
    out = orc.train_step(p, torch.from_numpy(x), torch.from_numpy(pred), torch.from_numpy(eps), bn_state=orc.new_bn_state(p))
    return params, (x, pred, eps), p, out


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize("B,width", [(4, 64), (32, 64), (3, 128)])
def test_bf16_step_close_to_fp32_oracle(B, width):
    """width 128 = BASELINE.json config 5's frame size."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    from critic_vae_amd import layout as L
    dev = torch.device("cuda:0")
    params, (x, pred, eps), p, out = _oracle_step(B, width=width)
    vae = VariationalAutoencoder(width=width, max_batch=B, seed=0, precision="bf16").to(dev)
    assert vae.handle.precision == "bf16"
    tr = FusedTrainer(vae)
    xs, ps, es = (torch.from_numpy(v).to(dev) for v in (x, pred, eps))
    theta0 = vae.theta.data.clone()
    scal = tr.step(xs, ps, es).cpu()
    # forward outputs and the loss: bf16 conv operands, fp32 accumulation
    mu, logvar, recon = out["mu"].detach(), out["logvar"].detach(), out["recon"].detach()
    assert (tr.mu[:B].cpu() - mu).abs().max() < 3e-2
    assert (tr.logvar[:B].cpu() - logvar).abs().max() < 3e-2
    assert (tr.recon[:B].cpu() - recon).abs().max() < 3e-2
    assert abs(float(scal[0]) - float(out["total_loss"].detach())) < 5e-3
    assert torch.isfinite(scal[:13]).all()
    # gradients: same direction as the fp32 gradient, per tensor and overall
    ref = {k: v.grad.detach() for k, v in p.items() if v.grad is not None}
    got = L.native_to_ref(vae.handle.layout, tr.grads.cpu())
    worst = 1.0
    for k, g in ref.items():
        if g.abs().max() < 1e-7:
            continue
        c = _cos(got[k], g)
        worst = min(worst, c)
        assert c > 0.95, (k, c)       # worst: BatchNorm-1 gamma, 0.97 — the end of the backward chain
    flat_ref = torch.cat([ref[k].flatten() for k in sorted(ref)])
    flat_got = torch.cat([got[k].flatten() for k in sorted(ref)])
    assert _cos(flat_got, flat_ref) > 0.995
    # and the optimiser moved the parameters
    assert (vae.theta.data - theta0).abs().max() > 0


def _rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


# Relative L2 error of the bf16-mode gradient (bf16 MFMA operands AND bf16 activation storage) against the fp32
# oracle gradient at full size, per tensor, as MEASURED on the MI355X (the step is bit-reproducible, so these are exact
# until a kernel changes); the test allows 1.5x each.  The error grows backwards through the encoder; the worst tensor
# is the first conv's weight at the very end of the chain.  profiles/experiments/bf16_e1_ablation.py explains it
# (profiles/r03_bf16_e1_ablation_*.txt): the element-wise error of d_a0 that the bf16 chain hands to block 0 is 0.23 rel
# L2 (max-pool argmax flips + bf16 storage upstream) and averages down to 0.096 in dW1 at B = 2048 (0.18 at B = 256:
# it is noise, ~1/sqrt(B)); block 0's own roundings (x, W1, dy0 to bf16; pooling of bf16-rounded y) add 0.033; both are
# amplified by the cancellation BatchNorm's backward builds into the sum (|sum x dy| / sum |x dy| = 1.3e-3).
MEASURED_REL_L2 = {
    (2048, 64): {"e.model.0.weight": 0.1012, "e.model.1.weight": 0.0459, "e.model.1.bias": 0.0311, "e.model.4.weight": 0.0559,
                 "e.model.5.weight": 0.0186, "e.model.5.bias": 0.0118, "e.model.8.weight": 0.0203, "e.model.9.weight": 0.0084,
                 "e.model.9.bias": 0.0071, "e.model.12.weight": 0.0083, "e.model.13.weight": 0.0026, "e.model.13.bias": 0.0024,
                 "e.fc_mu.weight": 0.0026, "e.fc_mu.bias": 0.0022, "e.fc_var.weight": 0.0022, "e.fc_var.bias": 0.0017,
                 "d.model.0.weight": 0.0077, "d.model.0.bias": 0.0017, "d.model.3.weight": 0.0018, "d.model.3.bias": 0.0015,
                 "d.model.6.weight": 0.0016, "d.model.6.bias": 0.0015, "d.model.9.weight": 0.0015, "d.model.9.bias": 0.0013,
                 "d.model.12.weight": 0.0006, "d.model.12.bias": 0.0001, "d.decoder_input.weight": 0.0083, "d.decoder_input.bias": 0.0037},
    (1024, 128): {"e.model.0.weight": 0.1621, "e.model.1.weight": 0.0897, "e.model.1.bias": 0.0482, "e.model.4.weight": 0.0804,
                  "e.model.5.weight": 0.0385, "e.model.5.bias": 0.0251, "e.model.8.weight": 0.0339, "e.model.9.weight": 0.0141,
                  "e.model.9.bias": 0.0101, "e.model.12.weight": 0.0117, "e.model.13.weight": 0.0016, "e.model.13.bias": 0.0013,
                  "e.fc_mu.weight": 0.0014, "e.fc_mu.bias": 0.0009, "e.fc_var.weight": 0.0016, "e.fc_var.bias": 0.0012,
                  "d.model.0.weight": 0.0128, "d.model.0.bias": 0.0017, "d.model.3.weight": 0.0019, "d.model.3.bias": 0.0017,
                  "d.model.6.weight": 0.0016, "d.model.6.bias": 0.0014, "d.model.9.weight": 0.0017, "d.model.9.bias": 0.0015,
                  "d.model.12.weight": 0.0008, "d.model.12.bias": 0.0003, "d.decoder_input.weight": 0.0138, "d.decoder_input.bias": 0.0061},
}
FULL_SIZE_MARGIN = 1.5            # x measured, + 2e-4 absolute for the tensors measured at ~1e-4
FULL_SIZE_REL_L2_ALL = 0.02       # the whole flat gradient


@pytest.mark.parametrize("B,width", [(2048, 64), (1024, 128)])
def test_bf16_full_size_configs(B, width):
    """BASELINE.json configs[2]/[3] (bf16, 2048 frames of 64x64 per GPU) and configs[4] (1024 frames of 128x128 per
    GPU) at FULL per-GPU size: finite, bit-reproducible across two runs, forward outputs and loss against the fp32
    oracle run at the same size on the host, and every gradient tensor within 1.5x its own measured relative L2 error
    against the oracle's (MEASURED_REL_L2: 1e-4 .. 0.014 on decoder / fc tensors, 0.10 / 0.16 on the worst one)."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    from critic_vae_amd import layout as L
    dev = torch.device("cuda:0")
    params, (x, pred, eps), p, out = _oracle_step(B, width=width)
    assert torch.isfinite(out["total_loss"]).item(), "pick a finite seed"
    xs, ps, es = (torch.from_numpy(v).to(dev) for v in (x, pred, eps))
    runs = []
    for _ in range(2):
        vae = VariationalAutoencoder(width=width, max_batch=B, seed=0, precision="bf16").to(dev)
        tr = FusedTrainer(vae)
        scal = tr.step(xs, ps, es)
        torch.cuda.synchronize()
        runs.append((tr.grads.clone(), scal.clone(), tr.mu.clone(), tr.recon.clone(), vae.theta.data.clone()))
        del tr, vae
    g, scal, mu, recon, theta = runs[0]
    assert torch.isfinite(g).all() and torch.isfinite(scal[:13]).all() and torch.isfinite(theta).all()
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b), "two runs of the bf16 step differ bitwise"
    assert (mu.cpu() - out["mu"].detach()).abs().max() < 3e-2
    assert (recon.cpu() - out["recon"].detach()).abs().max() < 3e-2
    assert abs(float(scal[0]) - float(out["total_loss"].detach())) < 2e-3
    assert abs(float(scal[2]) - float(out["KLD"])) < 1e-4
    from critic_vae_amd.lib import Handle
    got = L.native_to_ref(Handle(width, 1).layout, g.cpu())
    worst, errs = ("", 0.0), {}
    for k, v in p.items():
        ref = v.grad.detach()
        if ref.abs().max() < 1e-7:            # pre-BatchNorm conv biases: true gradient 0
            continue
        e = _rel_l2(got[k], ref)
        if e > worst[1]:
            worst = (k, e)
        errs[k] = e
    print(f"bf16 B={B} W={width}: loss {float(scal[0]):.6f} (oracle {float(out['total_loss'].detach()):.6f}); worst gradient rel L2 {worst}")
    print("   per tensor:", {k.replace("encoder.", "e.").replace("decoder.", "d."): round(e, 4) for k, e in errs.items()})
    meas = MEASURED_REL_L2[(B, width)]
    for k, e in errs.items():
        short = k.replace("encoder.", "e.").replace("decoder.", "d.")
        assert e < FULL_SIZE_MARGIN * meas[short] + 2e-4, (k, e, meas[short])
    keys = sorted(errs)
    flat_got = torch.cat([got[k].flatten() for k in keys])
    flat_ref = torch.cat([p[k].grad.detach().flatten() for k in keys])
    assert _rel_l2(flat_got, flat_ref) < FULL_SIZE_REL_L2_ALL


def test_bf16_training_trajectory_tracks_fp32():
    """32 Adam steps at B=32 (BASELINE config 1 shape): the bf16-mode loss curve stays within 2e-2 of
    the fp32-mode one and both fall."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    dev = torch.device("cuda:0")
    B, curves = 32, {}
    for prec in ("f32", "bf16"):
        vae = VariationalAutoencoder(max_batch=B, seed=0, precision=prec).to(dev)
        tr = FusedTrainer(vae)
        losses = []
        for step in range(32):
            x, pred, eps = (torch.from_numpy(v).to(dev) for v in synth.make_batch(1234, step, B))
            losses.append(float(tr.step(x, pred, eps)[0]))
        curves[prec] = np.array(losses)
    assert np.isfinite(curves["bf16"]).all()
    assert np.abs(curves["bf16"] - curves["f32"]).max() < 2e-2
    assert curves["bf16"][-1] < 0.6 * curves["bf16"][0]


def test_bf16_config2_trains_like_fp32_at_full_batch():
    """BASELINE.json configs[2] must TRAIN, not just step: 200 Adam steps (lr 5e-5, the reference's) at batch 2048 in
    bf16 mode and in fp32 mode from the same weights on the same device-generated frames.  The loss curves must
    stay together (max gap over the run) and end together (final-loss ratio); both must have gone down.
    Measured on the MI355X: printed below.
    Frames are U[0,1) noise on purpose.  Round 3 first tried smooth frames (U[0,1) on an 8x8 grid, bilinear to 64x64) and every
    loss of the run came out NaN: that is the REFERENCE's own behaviour on those frames, not a bf16 problem — the CPU oracle
    (== the reference, tests/golden) gives loss = NaN on them at step 0 with the seed-0 weights at B = 64 and B = 256
    (cs level 2 = -0.0045 / -0.0043 < 0 -> fractional power -> NaN; checked in round 4).  Parity on frames
    that look like frames is test_gpu_step.py::test_step_on_the_references_real_frames (finite in the reference)."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    dev = torch.device("cuda:0")
    B, STEPS = 2048, 200
    curves = {}
    for prec in ("bf16", "f32"):
        vae = VariationalAutoencoder(max_batch=B, seed=0, precision=prec).to(dev)
        tr = FusedTrainer(vae)
        gen = torch.Generator(device=dev).manual_seed(77)
        # the benchmark's synthetic frames, U[0,1) (BASELINE.json; finite MS-SSIM from the first step on): 8 batches, cycled
        frames = torch.rand(8, B, 3, 64, 64, device=dev, generator=gen)
        losses = torch.empty(STEPS, 3, device=dev)
        for i in range(STEPS):
            x = frames[i % 8]
            pr = torch.rand(B, 1, device=dev, generator=gen)
            ep = torch.randn(B, 32, device=dev, generator=gen)
            losses[i] = tr.step(x, pr, ep)[:3]
        torch.cuda.synchronize()
        curves[prec] = losses.cpu()
        del tr, vae
    a, b = curves["bf16"][:, 0], curves["f32"][:, 0]
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    gap, ratio = float((a - b).abs().max()), float(a[-8:].mean() / b[-8:].mean())
    print(f"bf16 vs f32, {STEPS} steps at B={B}: loss {float(b[0]):.4f} -> f32 {float(b[-1]):.4f} / bf16 {float(a[-1]):.4f}; "
          f"max |gap| {gap:.2e}, final ratio {ratio:.5f}")
    assert float(b[-8:].mean()) < 0.9 * float(b[0]) and float(a[-8:].mean()) < 0.9 * float(a[0]), "the loss must go down"
    assert gap < 1.5e-3 and abs(ratio - 1.0) < 5e-4          # measured: max gap 4.7e-4, ratio 0.99999


def test_packed_frame_is_the_bf16_rounded_frame_and_survives_an_eval_forward():
    """Round 5: E1's statistics pass leaves the frame in the workspace as packed bf16 pixels (r, g, b, 0), and the pool pass and E1's weight-gradient
    kernel stage their strips from that copy.  (1) The copy is exactly the RNE-rounded frame, every pixel once.  (2) A backward that follows an
    EVAL-mode forward on the same workspace (no statistics pass: the copy is stale) must not read it: the gradients of a train forward + backward are
    bit-identical whether or not an eval-mode encoder call on OTHER frames ran in between and overwrote nothing... and, the hard case, when the copy
    is poisoned by hand between forward and backward the backward still uses it only if the handle says it is current — so poisoning after a train
    forward changes dW1 (the copy IS what the kernel reads), while an eval forward in between makes the kernel fall back to the fp32 frame."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    dev = torch.device("cuda:0")
    B = 6
    x, pred, eps = (torch.from_numpy(v).to(dev) for v in synth.make_batch(1234, 0, B))
    vae = VariationalAutoencoder(max_batch=B, seed=0, precision="bf16").to(dev)
    tr = FusedTrainer(vae)
    h, theta = vae.handle, vae.theta.data

    def fwd(train):
        h.forward(B, x, pred, eps, theta, vae.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=train)
        h.loss(B, x, tr.mu, tr.logvar, tr.recon, tr.ws, tr.scalars, tr.d_recon, tr.d_mu, tr.d_logvar)

    def bwd():
        h.backward(B, x, pred, eps, theta, tr.logvar, tr.recon, tr.d_recon, tr.d_mu, tr.d_logvar, tr.ws, tr.grads)
        torch.cuda.synchronize()
        return tr.grads.clone()

    off = h.lib.cvae_ws_offset(h.h, B, b"xp")
    assert off >= 0
    fwd(True)
    xp = tr.ws.view(torch.bfloat16)[2 * off:2 * off + B * 64 * 64 * 4].view(B, 64, 64, 4)
    want = torch.cat([x.permute(0, 2, 3, 1).to(torch.bfloat16), torch.zeros(B, 64, 64, 1, device=dev, dtype=torch.bfloat16)], dim=-1)
    assert torch.equal(xp, want)
    g_ref = bwd()
    # the copy is what the kernel stages: poisoning it after a train-mode forward changes E1's weight gradient
    fwd(True)
    xp.zero_()
    g_poison = bwd()
    assert not torch.equal(g_poison, g_ref)
    # an eval-mode forward makes the copy stale: the backward converts the fp32 frame itself (poison ignored).  The saved activations of an
    # eval-mode forward differ from a train-mode one's, so compare against the same sequence without the poison
    bn0 = vae.bn_state.clone()                     # the eval-mode forward reads the running statistics every train-mode forward moves
    fwd(True); fwd(False)
    g_a = bwd()
    vae.bn_state.copy_(bn0)
    fwd(True); fwd(False); xp.fill_(3.0)
    g_b = bwd()
    assert torch.equal(g_a, g_b)


def test_unknown_precisions_are_rejected():
    import ctypes as C
    from critic_vae_amd import lib as cvlib
    with pytest.raises(ValueError):
        cvlib.Handle(64, 4, precision="fp8")
    h = cvlib._p()
    cfg = cvlib._Config(64, 4, 0, 7)
    assert cvlib.load().cvae_create(C.byref(cfg), C.byref(h)) != 0


def test_bf16_inference_path_matches_fp32_mode():
    """evaluate / decode (cvae_forward(recon=NULL) + stand-alone cvae_decode, which re-packs the bf16
    weights itself) in bf16 mode vs the fp32 mode of the same library."""
    from critic_vae_amd.nets import VariationalAutoencoder
    dev = torch.device("cuda:0")
    B = 6
    x, pred, _ = (torch.from_numpy(v).to(dev) for v in synth.make_batch(7, 0, B))
    outs = {}
    for prec in ("f32", "bf16"):
        vae = VariationalAutoencoder(max_batch=B, seed=3, precision=prec).to(dev).eval()
        with torch.no_grad():
            mu, logvar = vae.encoder(x)
            outs[prec] = (mu.cpu(), vae.decoder(mu, pred).cpu())
    assert (outs["bf16"][0] - outs["f32"][0]).abs().max() < 3e-2
    assert (outs["bf16"][1] - outs["f32"][1]).abs().max() < 3e-2


@pytest.mark.parametrize("mode", ["bf16x9", "bf16x6"])
@pytest.mark.parametrize("B", [4, 32])
def test_bf16x9_emulation_meets_the_fp32_parity_bar(B, mode):
    """precision="bf16x9": operands split exactly into three bf16 parts, nine exact partial products per
    fp32 product -> only the summation order differs from fp32 ("bf16x6" keeps the six leading products and
    drops three terms of relative size <= 2^-24 each — the size of one fp32 rounding).  Held to the SAME bar as the
    fp32 mode (tests/decisions.py, as tests/test_gpu_step.py uses it): 1e-4 absolute on outputs, loss and every
    gradient element; the max-pool / ReLU decisions that differ from the oracle's are counted and shown to be ties;
    every gradient element within 1e-4 of its tensor's max against the oracle run with those decisions imposed.
    (Round 2 allowed 5e-3 relative here instead; test_gpu_step.py::test_step_b256_fp32_against_oracle runs the same
    check at the bench size.)"""
    import sys, os
    sys.path.insert(0, os.path.dirname(__file__))
    from decisions import check_step_against_oracle
    from critic_vae_amd.nets import VariationalAutoencoder
    dev = torch.device("cuda:0")
    x, pred, eps = (torch.from_numpy(v) for v in synth.make_batch(1234, 0, B))
    res = {}
    for prec in (mode, "f32"):
        vae = VariationalAutoencoder(max_batch=B, seed=0, precision=prec).to(dev)
        vae.load_reference_params(synth.make_params(0))
        out = vae(x.to(dev), pred.to(dev), eps=eps.to(dev))
        losses = vae.vae_loss(*out)
        losses["total_loss"].backward()
        torch.cuda.synchronize()
        res[prec] = (out[1].detach().cpu(), out[3].detach().cpu(), float(losses["total_loss"].item()))
        if prec == mode:
            rep, o = check_step_against_oracle(vae, x, pred, eps, B)
            assert rep is not None and rep["rel_forced"] <= 1e-4
    mu, recon, loss = res[mode]
    assert (mu - o["mu"].detach()).abs().max() < 1e-4
    assert (recon - o["recon"].detach()).abs().max() < 1e-4
    assert abs(loss - float(o["total_loss"].detach())) < 1e-4
    # and it sits as close to the fp32-MFMA mode as that mode sits to the oracle
    assert (mu - res["f32"][0]).abs().max() < 2e-5 and (recon - res["f32"][1]).abs().max() < 2e-5


DSEED_128 = {"bf16x9": 1234, "bf16x6": 1234}        # data seed per mode (the tie study's seeds: 1234, 7, 11, 21, 33)


@pytest.mark.parametrize("mode", ["bf16x9", "bf16x6"])
def test_bf16x6_step_at_128x128_frames_meets_the_fp32_parity_bar(mode):
    """Round 4: in the fp32-emulation modes the weight gradients of E2..E4 / D0 run on the bf16 MFMA too
    (conv_wgrad_split.hip: both fp32 operands split exactly into three bf16 parts while staged, the nine / six leading partial
    products per 16-pixel block).  The 64x64 instantiations are covered by the B = 4 / 32 / 256 parity tests; this is the
    128x128 set (64 / 32 / 16 / 8-pixel layers, other tile geometries) at a ragged batch: same bar as the fp32 mode —
    1e-4 absolute on outputs and loss, every gradient element within 1e-4 of its tensor's max with the decisions imposed.
    "bf16x9" has instantiations of its own here (the DMAX = 4 weight-gradient bodies, the nine-product forward / input-gradient
    geometries); both modes run data seed 1234, whose oracle loss is finite (0.99367)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(__file__))
    from decisions import check_step_against_oracle
    from critic_vae_amd.nets import VariationalAutoencoder
    dev = torch.device("cuda:0")
    W, B, DSEED = 128, 3, DSEED_128[mode]   # bf16x6: data seed 1234 has one block-3 pool window 1.007e-5 from a tie in this mode: inside the mode's bound (decisions.TIE_TOL_BY_MODE,
                                            # derived from profiles/r05_tie_gap_study.txt) and inside twice the two sides' value deviation, which check_step_against_oracle asserts
    x, pred, eps = (torch.from_numpy(v) for v in synth.make_batch(DSEED, 0, B, W))
    vae = VariationalAutoencoder(width=W, max_batch=B, seed=0, precision=mode).to(dev)
    vae.load_reference_params(synth.make_params(0, W))
    out = vae(x.to(dev), pred.to(dev), eps=eps.to(dev))
    losses = vae.vae_loss(*out)
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    rep, o = check_step_against_oracle(vae, x, pred, eps, B, verbose=True)
    assert rep is not None and rep["rel_forced"] <= 1e-4, rep
    assert torch.isfinite(o["total_loss"])
    assert (out[1].detach().cpu() - o["mu"].detach()).abs().max() < 1e-4
    assert (out[3].detach().cpu() - o["recon"].detach()).abs().max() < 1e-4
    assert abs(float(losses["total_loss"].item()) - float(o["total_loss"].detach())) < 1e-4


def test_big_tile_conv_kernels_every_instantiation_exact_on_their_stored_operands():
    """conv_bf16_big.hip (rounds 4-5: PERSISTENT workgroups on a 16-accumulator-tile wave tile, everything inside the MFMA stream) runs
    E2 / E3 / E4 forward and input gradient (E2 on image-high items / 16-row strips).  At test batch sizes every item would get its own workgroup, so the item loop — next
    item's tiles and slabs requested across the epilogue, fragment sets and slab buffers carried over — would never run: a child process
    caps the grid at 8 workgroups (CVAE_PERSIST_MAXWG, read once per process) and runs the stored-operand test of this file — every conv
    output recomputed on the CPU from the bf16 operands the kernels consumed; B = 8, the ragged B = 5, and B = 37 (74 / 19 tiles: several
    items per workgroup, uneven ends, partial groups, the forward kernels' four-tile BatchNorm partials).  The cap holds for every persistent
    conv launcher: at (128, 37) D0's forward on conv_bf16_ps.hip walks 10 tile pairs x 2 channel blocks on 8 workgroups, so the workgroups
    move on to the next pair as well as to the next channel block."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CVAE_PERSIST_MAXWG="8")
    sel = "kernels_exact_on_their_stored_operands or two_pass_e1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_bf16.py"), "-m", "gpu", "-q", "-x",
                        "-k", sel], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("W,B", [(128, 5), (64, 5), (128, 2)])
def test_big_tile_bn_partials_match_the_per_tile_kernels(W, B, tmp_path):
    """The persistent big-tile forward kernels emit ONE BatchNorm partial per item of four 128-pixel tiles, and launch_bn_fwd_finalize derives the
    pixel count of every partial from the tile geometry: a quarter of an image (tiles per image >= 4: E3 at 128 x 128), two whole images (two tiles
    per image: E4 at 128 x 128, E3 at 64 x 64), four half-filled... (8 x 8 images: E4 at 64 x 64), with ragged ends at odd batch sizes.  Two child
    processes (the switch is read once per process) run the same bf16 forward with the big-tile kernels (the default: all six) and with
    the per-tile kernels (CVAE_CONV_PER_TILE=1): the running statistics — sums over ALL pixels, merged from differently grouped partials — must agree
    to fp32 summation noise, the outputs to bf16 noise.  A wrong count or a wrong partial row would be off by whole percents."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for per_tile in ("0", "1"):
        out = str(tmp_path / f"bn_{per_tile}.npz")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "bn_geom_worker.py"), str(W), str(B), out],
                           env=dict(os.environ, CVAE_CONV_PER_TILE=per_tile), capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res[per_tile] = np.load(out)
    a, b = res["0"], res["1"]
    for bi in (1, 5, 9, 13):
        for k in (f"rm{bi}", f"rv{bi}"):
            scale = max(float(np.abs(b[k]).max()), 1e-6)
            assert np.abs(a[k] - b[k]).max() <= 2e-4 * scale, (k, float(np.abs(a[k] - b[k]).max()), scale)
    assert np.abs(a["mu"] - b["mu"]).max() < 2e-2 and np.abs(a["logvar"] - b["logvar"]).max() < 2e-2


def test_bn_pool_ops_follow_the_handle_storage_type():
    """The stand-alone BatchNorm/pool ops of a bf16-storage handle read and write bf16 tensors (as the step does):
    eval-mode forward (coefficients from the running statistics) and the backward apply pass against a torch
    evaluation of the same formulas on the same bf16 operands."""
    from critic_vae_amd import lib as cvlib
    dev = torch.device("cuda:0")
    B, layer, C, H = 4, 1, 64, 32
    h = cvlib.Handle(64, B, precision="bf16")
    g = torch.Generator(device="cpu").manual_seed(5)
    y = (torch.randn(B, H, H, C, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.3).to(dev)
    rm, rv = (torch.randn(C, generator=g) * 0.2).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    coef = torch.empty(4 * C, device=dev)
    a = torch.empty(B, H // 2, H // 2, C, dtype=torch.bfloat16, device=dev)
    sc = torch.empty(h.op_scratch_floats(B), device=dev)
    f32v = lambda t: t.view(torch.float32)      # noqa: E731  (opaque pointer: two bf16 elements per float)
    h.op_bn_pool_act_fwd(layer, B, f32v(y), None, gamma, beta, rm, rv, coef, f32v(a), sc, train=False)
    torch.cuda.synchronize()
    invstd = 1.0 / torch.sqrt(rv + 1e-5)
    scale, shift = gamma * invstd, beta - rm * gamma * invstd
    n = torch.addcmul(shift, y.float(), scale)                        # fma(y, scale, shift) per element
    want = torch.relu(n.view(B, H // 2, 2, H // 2, 2, C).amax(dim=(2, 4))).to(torch.bfloat16)
    assert (a.float() - want.float()).abs().max() <= 2.0 ** -7 * want.float().abs().max()
    # backward: dy = scale * ((p == argmax ? g : 0) - k1 - xhat * k2), k1 = sum(g)/N, k2 = sum(g*xhat)/N, g = da*[a > 0]
    da = torch.randn(B, H // 2, H // 2, C, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.empty_like(y)
    dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
    h.op_bn_pool_act_bwd(layer, B, f32v(y), f32v(a), f32v(da), coef, gamma, f32v(dy), dgamma, dbeta, None, sc)
    torch.cuda.synchronize()
    win = n.view(B, H // 2, 2, H // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, H // 2, C, 4)
    pos = win.argmax(dim=-1)                                           # first maximum in scan order (ties: measure zero here)
    gq = da.float() * (a.float() > 0)
    xhat = (y.float() - rm) * invstd
    xw = xhat.view(B, H // 2, 2, H // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, H // 2, C, 4)
    N = B * H * H
    k1, k2 = gq.sum(dim=(0, 1, 2)) / N, (gq * xw.gather(-1, pos[..., None])[..., 0]).sum(dim=(0, 1, 2)) / N
    sel = torch.zeros_like(xw).scatter_(-1, pos[..., None], gq[..., None])
    dw = scale[:, None] * (sel - k1[:, None] - xw * k2[:, None])
    dy_ref = dw.view(B, H // 2, H // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, H, H, C)
    assert (dy.float() - dy_ref).abs().max() <= 2.0 ** -7 * dy_ref.abs().max() + 1e-6
    assert (dbeta - gq.sum(dim=(0, 1, 2))).abs().max() <= 1e-3 * gq.abs().sum(dim=(0, 1, 2)).max()


def _e1_per_op(h, B, W, x, theta, bn_state, train):
    """Block 0's forward in the per-op form: op_conv_fwd(0) stores y0 (bf16) and the BatchNorm partials, op_bn_pool_act_fwd(0)
    merges them and reads y0 back.  Returns (a0, coef0, running mean, running var); bn_state itself is not modified."""
    from critic_vae_amd import layout as L
    prm = {k: theta[o:o + n] for k, (o, n) in h.layout.items() if k.startswith("enc0.")}
    y0 = torch.empty(B * W * W * 32 // 2, device=x.device)
    part = torch.empty(h.op_bn_partial_floats(0, B), device=x.device)
    h.op_conv_fwd(0, B, x, prm["enc0.w"], prm["enc0.b"], y0, part)
    rm, rv = bn_state[:32].clone(), bn_state[L.BN_TOTAL:L.BN_TOTAL + 32].clone()
    coef = torch.empty(128, device=x.device)
    a0 = torch.empty(B * (W // 2) * (W // 2) * 32 // 2, device=x.device)
    h.op_bn_pool_act_fwd(0, B, y0, part, prm["enc0.gamma"], prm["enc0.beta"], rm, rv, coef, a0,
                         torch.empty(h.op_scratch_floats(B), device=x.device), train=train)
    torch.cuda.synchronize()
    return a0, coef, rm, rv


def test_two_pass_e1_forward_is_bit_identical():
    """bf16 mode runs E1's forward twice (statistics pass, then conv + BatchNorm / pool / ReLU epilogue) instead of
    conv -> bn_pool_act_fwd reading y1 back (the per-op form: op_conv_fwd(0), then op_bn_pool_act_fwd(0)).  The epilogue
    pools the bf16-rounded values exactly as the separate kernel pools the stored tensor, so the step's a0, coef0 and
    block-0 running statistics must equal the per-op form's on the same theta, x and pre-step running statistics to the
    bit — at both frame sizes; and the eval-mode encoder's a0 must equal the same ops at train=False."""
    from critic_vae_amd import layout as L
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    dev = torch.device("cuda:0")
    for W, B in ((64, 8), (128, 3)):
        x, pred, eps = (torch.from_numpy(v).to(dev) for v in synth.make_batch(1234, 0, B, W))
        vae = VariationalAutoencoder(width=W, max_batch=B, seed=0, precision="bf16").to(dev)
        h = vae.handle
        tr = FusedTrainer(vae)
        theta0, bn0 = vae.theta.data.clone(), vae.bn_state.clone()
        tr.step(x, pred, eps)
        torch.cuda.synchronize()
        step_a0 = h.ws_view(tr.ws, B, "a0", B * (W // 2) * (W // 2) * 32 // 2).clone()
        step_coef0 = h.ws_view(tr.ws, B, "coef0", 128).clone()
        a0, coef, rm, rv = _e1_per_op(h, B, W, x, theta0, bn0, train=True)
        assert torch.equal(step_a0.view(torch.int32), a0.view(torch.int32)), (W, "a0")
        assert torch.equal(step_coef0, coef), (W, "coef0")
        assert torch.equal(vae.bn_state[:32], rm), (W, "running mean 0")
        assert torch.equal(vae.bn_state[L.BN_TOTAL:L.BN_TOTAL + 32], rv), (W, "running var 0")
        with torch.no_grad():
            vae.eval().encoder(x)
        torch.cuda.synchronize()
        eval_a0 = h.ws_view(tr.ws, B, "a0", a0.numel()).clone()
        a0e, _, _, _ = _e1_per_op(h, B, W, x, vae.theta.data, vae.bn_state, train=False)
        assert torch.equal(eval_a0.view(torch.int32), a0e.view(torch.int32)), (W, "eval a0")


@pytest.mark.parametrize("B,vec_bound,tiny_bound", [(8, 0.35, 0.25), (512, 0.20, 0.10)])
def test_bf16_step_never_stores_y0_unless_a_block0_gamma_is_tiny(B, vec_bound, tiny_bound):
    """Round 3: in bf16 mode the forward's second E1 pass writes only a0; E1's weight-gradient kernel recomputes the
    75-tap conv on its tiles.  (1) With ordinary gammas the y0 slot of the workspace is never touched (NaN-prefilled
    here) and the step is finite.  (2) With |gamma| < 1e-2 channels in block 0 (0, 1e-3, -5e-3) the forward keeps y0 —
    decided on the device — because the backward's statistics take xhat of such channels from it (a0 cannot be
    inverted through a vanishing gamma): dgamma / dbeta / dW1 then still track the fp32 oracle.

    The bounds on the three tiny channels are read against max|dgamma| of the layer, not against the channel's own
    value: profiles/r04_c_tiny_gamma_sweep.txt (bf16 mode against fp32 mode, same inputs, B = 8 ... 2048) shows their
    error to be the bf16 noise every channel of the layer carries — at B = 8 0.11 / 0.08 of the scale beside 0.24 max /
    0.07 median over the 29 ordinary channels, falling with the batch like theirs (B = 512: 0.03 / 0.06 beside 0.08 /
    0.02; B = 2048: 0.005 / 0.02 beside 0.04 / 0.01).  A tiny-gamma channel's own dgamma can be a small fraction of the
    scale (B = 8, gamma = 1e-3: -5.5e-5 of 3.9e-4), which is all the "87 % of its own value" of round 3's red run was."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    from critic_vae_amd import layout as L
    from oracle import cvae_oracle as orc
    dev = torch.device("cuda:0")
    W = 64
    x, pred, eps = synth.make_batch(1234, 0, B, W)
    xs, ps, es = (torch.from_numpy(v).to(dev) for v in (x, pred, eps))
    for tiny in (False, True):
        params = synth.make_params(0, W)
        if tiny:
            gam = params["encoder.model.1.weight"].copy()
            gam[3], gam[7], gam[20] = 0.0, 1e-3, -5e-3
            params["encoder.model.1.weight"] = gam
        vae = VariationalAutoencoder(width=W, max_batch=B, seed=0, precision="bf16").to(dev)
        vae.load_reference_params(params)
        tr = FusedTrainer(vae, lr=0.0)
        h = vae.handle
        off = h.lib.cvae_ws_offset(h.h, B, b"y0")
        y0 = tr.ws[off:off + B * W * W * 32 // 2]
        y0.fill_(float("nan"))
        scal = tr.step(xs, ps, es)
        torch.cuda.synchronize()
        assert torch.isfinite(scal[:13]).all() and torch.isfinite(tr.grads).all()
        written = bool(torch.isfinite(y0.view(torch.bfloat16).float()).all())
        untouched = bool(torch.isnan(y0).all())
        assert (written and not untouched) if tiny else (untouched and not written), (tiny, written, untouched)
        p = orc.to_torch(params, requires_grad=True)
        orc.train_step(p, torch.from_numpy(x), torch.from_numpy(pred), torch.from_numpy(eps), bn_state=orc.new_bn_state(p))
        got = L.native_to_ref(h.layout, tr.grads.cpu())
        for k in ("encoder.model.0.weight", "encoder.model.1.weight", "encoder.model.1.bias"):
            assert _rel_l2(got[k], p[k].grad) < vec_bound, (tiny, k, _rel_l2(got[k], p[k].grad))     # bf16 noise: dW1 0.23 / dgamma 0.25 / dbeta 0.18 at B = 8, 0.17 / 0.09 / 0.07 at B = 512
        if tiny:          # the tiny channels themselves: dgamma = sum(g * xhat[argmax]) must come out, not 0 / inf
            gk, rk = got["encoder.model.1.weight"][[3, 7, 20]], p["encoder.model.1.weight"].grad[[3, 7, 20]]
            scale = p["encoder.model.1.weight"].grad.abs().max()
            assert torch.isfinite(gk).all() and (gk - rk).abs().max() < tiny_bound * scale, (gk, rk, scale)
            assert gk[0] == 0 and rk[0] == 0          # gamma = 0, beta = 0: the channel's output is 0 everywhere and ReLU'(0) = 0 blocks its gradient


def _bf16_step(W, B):
    """One bf16-mode forward + loss + backward of B images; returns (vae, trainer, x, pred, eps, running statistics before it)."""
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    dev = torch.device("cuda:0")
    vae = VariationalAutoencoder(width=W, max_batch=B, seed=0, precision="bf16").to(dev)
    tr = FusedTrainer(vae)
    x, pred, eps = (torch.from_numpy(v).to(dev) for v in synth.make_batch(1234, 0, B, W))
    h, theta = vae.handle, vae.theta.data
    bn0 = vae.bn_state.clone()
    h.forward(B, x, pred, eps, theta, vae.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=True)
    h.loss(B, x, tr.mu, tr.logvar, tr.recon, tr.ws, tr.scalars, tr.d_recon, tr.d_mu, tr.d_logvar)
    h.backward(B, x, pred, eps, theta, tr.logvar, tr.recon, tr.d_recon, tr.d_mu, tr.d_logvar, tr.ws, tr.grads)
    torch.cuda.synchronize()
    return vae, tr, x, pred, eps, bn0


# 5, 37: ragged tile counts (the persistent D4 / MS-SSIM / E1 / conv loops end unevenly); 128 x 128: the other set of instantiations (every
# spatial size doubles); 133: every fc kernel runs past its first block and ends partway through its last one (latent_gemm 128 + 5 images,
# fc_bwd_dflat 4 x 32 + 5, decin_fwd 8 x 16 + 5)
@pytest.mark.parametrize("W,B", [(64, 8), (64, 5), (64, 37), (128, 5), (128, 37), (64, 133), (128, 133)])
def test_bf16_kernels_exact_on_their_stored_operands(W, B):
    """Layout / indexing check of every link of the bf16-mode step, independent of the bf16 rounding noise: after one bf16 step the
    workspace holds the bf16 activations and activation gradients the kernels actually consumed.  Recomputing each link on the CPU from
    THOSE operands (ws_tools.check_bf16_stored_operands: the convs, BatchNorm statistics and running statistics, BatchNorm / pool / act
    forward and backward with dgamma / dbeta, fc_mu | fc_var, reparameterize, decoder_input forward and input gradient, the fc backward,
    the loss) must reproduce the kernel outputs up to fp32 summation order or up to one bf16 rounding of the stored result.  Catches
    what the statistical bounds above cannot: a wrong tap, channel or pixel permutation, a skipped tail image, a wrong flatten order or
    pixel count, a tie routed to the wrong pool position."""
    import time
    from ws_tools import check_bf16_stored_operands
    vae, tr, x, pred, eps, bn0 = _bf16_step(W, B)
    ties, t0 = {}, time.perf_counter()
    worst = check_bf16_stored_operands(vae.handle, tr, B, x, pred, eps, vae.theta.data, bn0, vae.bn_state, ties=ties)
    print(f"W={W} B={B}: check {time.perf_counter() - t0:.1f} s; near-tie windows {ties}; err / allowed: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_stored_operand_check_names_each_corrupted_link():
    """The links of check_bf16_stored_operands bite: after one bf16 step at (64, 133), a COPY of one link's stored result is corrupted in
    the ragged tail (the last image, past the fc kernels' first blocks), and the check must fail naming that link.  Only copies change;
    every kernel ran once, on the real data."""
    import types
    from ws_tools import check_bf16_stored_operands
    W, B = 64, 133
    vae, tr, x, pred, eps, bn0 = _bf16_step(W, B)
    h, theta = vae.handle, vae.theta.data
    names = ("ws", "grads", "mu", "logvar", "recon", "d_recon", "d_mu", "d_logvar", "scalars")
    clean = {k: getattr(tr, k).clone() for k in names}
    clean_bn = vae.bn_state.clone()
    work = types.SimpleNamespace(**{k: v.clone() for k, v in clean.items()})
    bn1 = clean_bn.clone()
    K, last = 4096, B - 1

    def off(name):
        o = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert o >= 0, name
        return o

    def bf16_last(name, per):       # the last image's elements of a stored bf16 tensor (a view into the copy)
        return work.ws.view(torch.bfloat16)[2 * off(name) + last * per:2 * off(name) + B * per]

    def windows(name, s, c):        # the last image of a stored bf16 NHWC tensor as (s/2, s/2, c, 4) windows, scan order
        return bf16_last(name, s * s * c).view(s // 2, 2, s // 2, 2, c).permute(0, 2, 4, 1, 3).reshape(s // 2, s // 2, c, 4)

    def c_mu():
        work.mu[last, 31] += 1e-3 * clean["mu"].abs().max()

    def c_zcat():
        work.ws[off("zcat") + last * 33 + 32] += 0.5

    def c_h():
        v = bf16_last("h", K).view(-1, 256)
        t = v[:, 3].clone()
        v[:, 3] = v[:, 7]
        v[:, 7] = t

    def c_d_zcat():
        row = work.ws[off("d_zcat") + last * 33:off("d_zcat") + B * 33]
        row[int(row.abs().argmax())] = 0.0

    def c_d_a3():
        v = bf16_last("d_a3", K)
        j = int(v.float().abs().argmax())
        v[j] = (v[j].float() * 1.02).to(torch.bfloat16)

    def c_dw_fc():                  # the last image's outer product a3 (x) bf16(dml) taken out of the fc weight gradient
        dz = work.ws[off("d_zcat") + last * 33:off("d_zcat") + last * 33 + 32]
        ex = 0.5 * eps[last] * torch.exp(0.5 * work.logvar[last])
        dml = torch.cat((dz + work.d_mu[last], dz * ex + work.d_logvar[last])).to(torch.bfloat16).float()
        o, n_ = h.layout["fc.w"]
        work.grads[o:o + n_].view(K, 64).sub_(torch.outer(bf16_last("a3", K).float(), dml))

    def c_d_logvar():
        j = int(work.d_logvar[last].abs().argmax())
        work.d_logvar[last, j] *= 1.01

    def c_coef1():
        cf = work.ws[off("coef1"):off("coef1") + 4 * 64].view(64, 4)
        cf[int(cf[:, 2].abs().argmax()), 2] *= 1.005

    def c_running_var2():
        bn1[480 + 96 + 5] *= 1.001

    def c_a2():                     # one pooled value of the last image taken from another window position
        cf = work.ws[off("coef2"):off("coef2") + 4 * 128].view(128, 4)
        nw = torch.relu(windows("y2", 16, 128).float() * cf[:, 0, None] + cf[:, 1, None])
        srt = nw.sort(dim=-1, descending=True).values
        j = int((srt[..., 0] - srt[..., 1]).flatten().argmax())
        bf16_last("a2", 8 * 8 * 128)[j] = srt[..., 1].flatten()[j].to(torch.bfloat16)

    def c_d_y2():                   # the last image's gradient moved between two positions of one window
        w = windows("d_y2", 16, 128)
        j = int((w[..., 0].float() - w[..., 1].float()).abs().flatten().argmax())
        v = w.reshape(-1, 4)[j].clone()
        wv = bf16_last("d_y2", 16 * 16 * 128).view(8, 2, 8, 2, 128)
        py, px, c = j // (8 * 128), (j // 128) % 8, j % 128
        wv[py, 0, px, 0, c], wv[py, 0, px, 1, c] = v[1], v[0]

    def c_dgamma1():
        o, _ = h.layout["enc1.gamma"]
        g = work.grads[o:o + 64]
        g[int(g.abs().argmax())] *= 1.1

    cases = [("mu", c_mu), ("zcat", c_zcat), ("h", c_h), ("d_zcat", c_d_zcat), ("d_a3", c_d_a3), ("dW fc", c_dw_fc),
             ("loss d_logvar", c_d_logvar), ("coef1 mean", c_coef1), ("running_var2", c_running_var2), ("a2", c_a2), ("d_y2", c_d_y2),
             ("dgamma1", c_dgamma1)]
    for link, corrupt in cases:
        for k, v in clean.items():
            getattr(work, k).copy_(v)
        bn1.copy_(clean_bn)
        corrupt()
        torch.cuda.synchronize()
        with pytest.raises(AssertionError) as ei:
            check_bf16_stored_operands(h, work, B, x, pred, eps, theta, bn0, bn1)
        assert str(ei.value).startswith(link), (link, str(ei.value)[:300])
        print(f"{link}: {str(ei.value)[:160]}")


@pytest.mark.parametrize("B", [40, 1029])      # 40: two ragged 32-image groups, four / two K slices;  1029: the large-batch paths
def test_bf16_d0_padding_skip_kernels_exact_on_their_stored_operands(B):
    """D0 (4x4 images) runs on conv4x4_row_bf16_kernel in bf16 mode: image-major M tiles that skip the zero padding, two K
    slices for the forward and NO split (bf16 result written directly) for the input gradient at B >= 1024.  Both passes
    recomputed on the CPU from the bf16 operands the kernels consumed (same bar as the test above: one bf16 rounding of the
    stored result); the input gradient d_h is not covered there."""
    import torch.nn.functional as F
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    from critic_vae_amd import layout as L
    dev = torch.device("cuda:0")
    vae = VariationalAutoencoder(width=64, max_batch=B, seed=0, precision="bf16").to(dev)
    tr = FusedTrainer(vae)
    x, pred, eps = (torch.from_numpy(v).to(dev) for v in synth.make_batch(77, 0, B, 64))
    h, theta = vae.handle, vae.theta.data
    h.forward(B, x, pred, eps, theta, vae.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=True)
    h.loss(B, x, tr.mu, tr.logvar, tr.recon, tr.ws, tr.scalars, tr.d_recon, tr.d_mu, tr.d_logvar)
    h.backward(B, x, pred, eps, theta, tr.logvar, tr.recon, tr.d_recon, tr.d_mu, tr.d_logvar, tr.ws, tr.grads)
    torch.cuda.synchronize()
    ws16 = tr.ws.view(torch.bfloat16)

    def act(name, c, s):
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        return ws16[2 * off:2 * off + B * s * s * c].float().view(B, s, s, c).permute(0, 3, 1, 2).contiguous().cpu()

    ref = L.native_to_ref(h.layout, theta.cpu())
    w0 = ref["decoder.model.0.weight"].to(torch.bfloat16).float()
    o0 = torch.relu(F.conv2d(act("h", 256, 4), w0, ref["decoder.model.0.bias"], padding=2))
    got = act("o0", 128, 4)
    assert torch.isfinite(got).all() and (got - o0).abs().max().item() <= 2.0 ** -8 * o0.abs().max().item(), "o0"
    d_h = F.conv_transpose2d(act("d_o0", 128, 4), w0, padding=2)
    got = act("d_h", 256, 4)
    assert torch.isfinite(got).all() and (got - d_h).abs().max().item() <= 2.0 ** -8 * d_h.abs().max().item(), "d_h"
