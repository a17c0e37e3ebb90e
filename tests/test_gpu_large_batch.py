"""GPU: the whole training step at batches whose tensors pass 2^31 bytes ("Tensors of 2 GiB and more").

A step on K = 8 distinct images, each repeated R times (x, pred and eps together; replica r = images [rK, rK + K)), has exactly the
loss, BatchNorm batch statistics and parameter gradients of a step on the K images: the loss and the KL term are batch means, and the
biased variance of a repeated set is the variance of the set.  So a step at a huge B is checked against references that cost no more
than a step at B = 8:

  (a) cvae_conv_route of every conv pass of the case (and E1's packed-frame row in bf16 mode) is asserted: the test states which kernel
      family ran;
  (b) replica consistency: replicas 0, 1, R - 1 and the ones whose bytes straddle 2^31, 2^32 and 2^33 bytes of each stored tensor (and the
      top of the packed frame xp) hold mu, logvar, recon and workspace slices (y*, a*, d_y*, d_a*, o*, d_o*, h) bitwise equal to replica
      0's: every forward and input-gradient kernel computes an image's outputs from that image and per-channel values shared by the
      batch, so any difference is an addressing error;
  (c) replica 0 against a reference: fp32 and bf16x6 against the CPU oracle on the K images (the bar of
      test_step_fp32_against_oracle_past_one_item_per_workgroup, decisions read from replica 0's slices), BatchNorm running statistics
      after the unbiased-variance factor n/(n-1) is converted; bf16 against the recomputation from its stored operands
      (ws_tools.check_bf16_stored_operands, weight-gradient references R times the K-image recomputation).

Each case runs in a child process (its memory is released before the next one starts) under a timeout; after a child that ends by a
signal or its timeout no further child starts."""
import os
import subprocess
import sys

import pytest

K = 8
GIB = 1 << 30
# (precision, width, B, routes): routes = cvae_conv_route of (E2, E3, E4) x (forward, input gradient), then E1's packed-frame row in bf16
# mode.  B: the smallest multiple of 8 past an edge (a tensor of exactly 2^31 bytes still has every offset below 2^31), or the last one below.
CASES = [
    ("f32", 64, 8184, "101111"),           # E2 forward on conv_mfma_ps.hip at the top of its range
    ("f32", 64, 8200, "001111"),           # ... on the per-tile kernel; y0 past 2^32 bytes
    ("f32", 64, 16392, "000011"),          # E3 forward and input gradient rerouted; y0 past 2^31 elements
    ("f32", 128, 2040, "101100"),
    ("f32", 128, 2056, "001100"),
    ("bf16", 64, 16376, "222222" "1"),     # E2 forward / input gradient on the big-tile kernel at the top of its range
    ("bf16", 64, 16392, "002222" "1"),     # ... on the per-tile bf16 kernels
    ("bf16", 128, 4088, "222222" "1"),
    ("bf16", 128, 4104, "002222" "1"),
    ("bf16x6", 64, 8200, "000000"),        # the emulation modes' per-tile and split weight-gradient kernels past 2^31 bytes
    ("bf16", 64, 65528, "000022" "1"),     # the packed bf16 frame at its last batch
    ("bf16", 64, 65544, "000000" "0"),     # E1 on the fp32 frame; activation gradients past 2^31 elements
]
PREC = {"f32": 0, "bf16": 1, "bf16x9": 2, "bf16x6": 3}
CASE_TIMEOUT_S = 900
_stop = []          # set once a child ended by a signal or its timeout: no further child starts


def _stored_tensors(prec, W):
    """(name, elements per image) of every stored per-image workspace tensor the step writes."""
    m = W // 64
    out = []
    for l, c in enumerate((32, 64, 128, 256)):
        s = 64 * m >> l
        if not (prec == "bf16" and l == 0):             # bf16 mode: the y0 slot is stale (E1's weight gradient recomputes y0)
            out.append((f"y{l}", s * s * c))
        out.append((f"a{l}", (s // 2) ** 2 * c))
        if l > 0:                                       # d_y0 is never stored (block 0's BatchNorm backward runs inside E1's weight gradient)
            out.append((f"d_y{l}", s * s * c))
        out.append((f"d_a{l}", (s // 2) ** 2 * c))
    for i, (c, s) in enumerate(((128, 4), (64, 8), (32, 16), (32, 32))):
        out += [(f"o{i}", (s * m) ** 2 * c), (f"d_o{i}", (s * m) ** 2 * c)]
    out.append(("h", 4096 * m * m))
    return out


def _replicas(prec, W, B):
    """Replicas to check: 0, 1, R - 1, and per stored tensor past 2^31 bytes the ones on both sides of 2^31, 2^32 and 2^33 bytes."""
    R, esz = B // K, 2 if prec == "bf16" else 4
    reps = {0: ["first"], 1: ["second"], R - 1: ["last"]}
    for name, per in _stored_tensors(prec, W):
        rb = per * K * esz                              # bytes of one replica
        for p in (31, 32, 33):
            if B * per * esz > 1 << p:
                for r in sorted({((1 << p) - 1) // rb, (1 << p) // rb}):
                    reps.setdefault(r, []).append(f"{name}@2^{p}")
    if prec == "bf16" and W * W * 8 * B + (2 * W + 2) * 8 < 1 << 31:
        reps.setdefault(R - 1, []).append("xp top")     # the packed frame's last bytes (its descriptor ends just below 2^31)
    return reps


def _case(prec, W, B, routes):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from critic_vae_amd import synth
    from critic_vae_amd.nets import VariationalAutoencoder
    from critic_vae_amd.train import FusedTrainer
    from oracle import cvae_oracle as orc

    dev = torch.device("cuda:0")
    R = B // K
    vae = VariationalAutoencoder(width=W, max_batch=B, seed=0, precision=prec).to(dev)
    vae.load_reference_params(synth.make_params(0, W))
    h, theta = vae.handle, vae.theta.data
    lib = h.lib
    # (a) routes
    got = "".join(str(lib.cvae_conv_route(PREC[prec], W, l, d, B)) for l in (1, 2, 3) for d in (0, 1))
    if prec == "bf16":
        got += str(lib.cvae_conv_route(1, W, 0, 0, B))
    print(f"case {prec} W={W} B={B} R={R}: routes {got}")
    assert got == routes, (got, routes)

    tr = FusedTrainer(vae)
    xk, pk, ek = (torch.from_numpy(v) for v in synth.make_batch(1234, 0, K, W))
    x = xk.to(dev).repeat(R, 1, 1, 1)
    pred, eps = pk.to(dev).repeat(R, 1), ek.to(dev).repeat(R, 1)
    bn0 = vae.bn_state.clone()
    h.forward(B, x, pred, eps, theta, vae.bn_state, tr.mu, tr.logvar, tr.recon, tr.ws, train=True)
    h.loss(B, x, tr.mu, tr.logvar, tr.recon, tr.ws, tr.scalars, tr.d_recon, tr.d_mu, tr.d_logvar)
    h.backward(B, x, pred, eps, theta, tr.logvar, tr.recon, tr.d_recon, tr.d_mu, tr.d_logvar, tr.ws, tr.grads)
    torch.cuda.synchronize()
    esz = 2 if prec == "bf16" else 4
    big = sorted(((B * per * esz, B * per, name) for name, per in _stored_tensors(prec, W)), reverse=True)[:3]
    print("  largest stored tensors: " + ", ".join(f"{n} {b / GIB:.2f} GiB = {e} elements" for b, e, n in big)
          + f"; frame x {B * 3 * W * W * 4 / GIB:.2f} GiB; workspace {h.workspace_bytes(B) / GIB:.1f} GiB")

    # (b) replica consistency, bitwise, on device slices
    reps = _replicas(prec, W, B)
    print("  replicas checked: " + ", ".join(f"{r} ({'/'.join(w)})" for r, w in sorted(reps.items())))
    bits = tr.ws.view(torch.int16) if esz == 2 else tr.ws.view(torch.int32)
    bad = []
    for name, per in _stored_tensors(prec, W):
        off = lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        base = off * (4 // esz)
        n = K * per
        ref0 = bits[base:base + n]
        for r in reps:
            if r and not torch.equal(bits[base + r * n:base + (r + 1) * n], ref0):
                bad.append(f"{name} replica {r}: {int((bits[base + r * n:base + (r + 1) * n] != ref0).sum())} of {n} elements differ")
    for name, t in (("mu", tr.mu), ("logvar", tr.logvar), ("recon", tr.recon)):
        for r in reps:
            if r and not torch.equal(t[r * K:(r + 1) * K].view(torch.int32), t[:K].view(torch.int32)):
                bad.append(f"{name} replica {r} differs")
    assert not bad, bad
    print(f"  replica consistency: {len(_stored_tensors(prec, W)) + 3} tensors x {len(reps) - 1} replicas bitwise equal to replica 0")

    # (c) replica 0 against a reference
    if prec == "bf16":
        from ws_tools import check_bf16_stored_operands
        ties = {}
        worst = check_bf16_stored_operands(h, tr, B, x, pred, eps, theta, bn0, vae.bn_state, images=(0, K), mult=R, ties=ties)
        top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
        print("  stored-operand recomputation, worst err / allowed: " + ", ".join(f"{k} {v:.2e}" for k, v in top)
              + f"; near-tie windows {ties}")
    else:
        from decisions import check_step_against_oracle
        tol = 1e-4
        vae.theta.grad = tr.grads
        rep, o = check_step_against_oracle(vae, xk, pk, ek, B, images=(0, K))
        assert rep is not None, "seed must give a finite loss"
        dm = float((tr.mu[:K].cpu() - o["mu"]).abs().max())
        dl = float((tr.logvar[:K].cpu() - o["logvar"]).abs().max())
        dr = float((tr.recon[:K].cpu() - o["recon"]).abs().max())
        s = tr.scalars.cpu()
        want = torch.cat([torch.stack([o["total_loss"], o["recon_loss"], o["KLD"]]).detach().float(),
                          torch.as_tensor(o["ssim_levels"]).float(), torch.as_tensor(o["cs_levels"]).float()])
        ds = float((s[:13] - want).abs().max())
        assert max(dm, dl, dr, ds) < tol, (dm, dl, dr, ds)
        assert rep["rel_forced"] <= 1e-4, rep
        # BatchNorm running statistics: the mean is the K images'; the running variance takes the unbiased batch variance, whose factor
        # n / (n - 1) differs between n = B * s * s and n = K * s * s pixels
        p = orc.to_torch(synth.make_params(0, W), requires_grad=True)
        bn = orc.new_bn_state(p)
        orc.train_step(p, xk, pk, ek, bn_state=bn)
        got_bn, b0 = vae.bn_state.cpu().double(), bn0.cpu().double()
        dbn, off = 0.0, 0
        for l, (c, (_, bi, _)) in enumerate(zip((32, 64, 128, 256), orc.ENC_BLOCKS)):
            s2 = (W >> l) ** 2                                                 # pixels per image of the conv output
            nK, nB = K * s2, B * s2
            rm = bn[f"encoder.model.{bi}.running_mean"].double()
            rv = bn[f"encoder.model.{bi}.running_var"].double()
            var_b = (rv - 0.9) / 0.1 * (nK - 1) / nK                       # the oracle started from running_var = 1
            want_rv = 0.9 * b0[480 + off:480 + off + c] + 0.1 * var_b * nB / (nB - 1)
            dbn = max(dbn, float((got_bn[off:off + c] - (0.9 * b0[off:off + c] + rm)).abs().max()),
                      float((got_bn[480 + off:480 + off + c] - want_rv).abs().max()))
            off += c
        assert dbn < tol, dbn
        print(f"  oracle on replica 0: mu {dm:.2e} logvar {dl:.2e} recon {dr:.2e} scalars {ds:.2e} BatchNorm running {dbn:.2e}; "
              f"gradients abs {rep['abs']:.2e}, rel (decisions imposed) {rep['rel_forced']:.2e}, flips {rep['flips']}")
    print(f"  peak device memory {torch.cuda.max_memory_allocated() / GIB:.1f} GiB")
    print("CASE_OK")


def _need_bytes(prec, W, B):
    """Device memory of a case: the workspace, the frame x, recon, d_recon, plus 1 GiB for everything of K images or smaller."""
    from critic_vae_amd import lib as cvlib
    return cvlib.Handle(W, B, precision=prec).workspace_bytes(B) + 3 * B * 3 * W * W * 4 + GIB


@pytest.mark.gpu
@pytest.mark.parametrize("prec,W,B,routes", CASES, ids=[f"{p}-w{w}-b{b}" for p, w, b, _ in CASES])
def test_training_step_past_two_gib(prec, W, B, routes):
    import torch
    if _stop:
        pytest.skip(_stop[0])
    need = _need_bytes(prec, W, B)
    free, total = torch.cuda.mem_get_info()
    if free < need + 8 * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free of {total / GIB:.1f} GiB; the case needs {need / GIB:.1f} GiB + 8 GiB")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("CVAE_")}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), prec, str(W), str(B), routes], env=env, cwd=root,
                           capture_output=True, text=True, timeout=CASE_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        _stop.append(f"an earlier case ({prec} W={W} B={B}) hit its {CASE_TIMEOUT_S} s timeout")
        pytest.fail(f"timeout after {CASE_TIMEOUT_S} s: {(e.stdout or '')[-3000:]}")
    print(r.stdout)
    if r.returncode < 0:
        _stop.append(f"an earlier case ({prec} W={W} B={B}) ended by signal {-r.returncode}")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("CASE_OK"), r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _case(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
