"""Helpers for tests that look at tensors inside a handle's workspace."""
import torch


def recompute_y0(h, ws, B, x, theta, width=64):
    """bf16 mode does not store y0 either (round 3): the forward's second E1 pass writes only the pooled a0, and E1's
    weight-gradient kernel runs the 75-tap conv again on the tiles it stages.  Write y0 into its workspace slot with the
    stand-alone conv op (layer 0 follows the handle's storage type: bf16 here) from the frames and the E1 parameters."""
    off = h.lib.cvae_ws_offset(h.h, B, b"y0")
    assert off >= 0
    ow, nw = h.layout["enc0.w"]
    ob, nb = h.layout["enc0.b"]
    part = torch.empty(h.op_bn_partial_floats(0, B), device=ws.device)
    h.op_conv_fwd(0, B, x, theta[ow:ow + nw], theta[ob:ob + nb], ws[off:off + B * width * width * 32 // 2], part)
    torch.cuda.synchronize()


def recompute_d_y0(h, ws, B, width=64, bf16_storage=False, x=None, theta=None):
    """d_y0 is never materialised by the step: E1's weight-gradient kernel applies block 0's BatchNorm / pool / ReLU
    backward while it stages its tiles (conv_thin.hip, E1Fuse).  Write it into its workspace slot with the stand-alone
    BatchNorm-backward op from the y0 / a0 / d_a0 / coef0 the step left there, so that tests can compare it.  The
    workspace has no d_y0 slot in the default (fused) configuration: the result is RETURNED as a flat buffer in the handle's
    storage type (fp32 elements, or bf16 elements packed two per float).
    bf16_storage: the handle keeps activations as bf16 (two elements per workspace float); y0 is then recomputed first
    (needs x and theta)."""
    per = 2 if bf16_storage else 1
    if bf16_storage:
        recompute_y0(h, ws, B, x, theta, width)

    def sl(name, n_elems, per_float=per):
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        return ws[off:off + n_elems // per_float]

    n_full, n_pool = B * width * width * 32, B * (width // 2) * (width // 2) * 32
    junk = torch.empty(3 * 32, device=ws.device)
    d_y0 = torch.empty(n_full // per, device=ws.device)
    h.op_bn_pool_act_bwd(0, B, sl("y0", n_full), sl("a0", n_pool), sl("d_a0", n_pool), sl("coef0", 128, 1),
                         junk[:32], d_y0, junk[32:64], junk[64:], None,
                         torch.empty(h.op_scratch_floats(B), device=ws.device))
    torch.cuda.synchronize()
    return d_y0


def check_bf16_stored_operands(h, ws, B, x, theta, grads, recon, d_recon, images=None, mult=1):
    """After one bf16-mode step of B images on handle h (workspace ws, frames x, parameters theta, gradient buffer grads, recon and
    d_recon as cvae_forward / cvae_loss wrote them): recompute every layer's result on the CPU in fp32 from the bf16 operands the
    kernels stored (weights rounded to bf16 as the packed copies are) and compare.  Activations and activation gradients: up to the
    bf16 rounding of the stored result (2^-8 of the tensor max); weight / bias gradients: up to fp32 summation order (2e-3).
    images = (i0, i1): only images [i0, i1) are read and recomputed (default: all B).  mult: every image of the step occurs `mult`
    times in it (a batch of replicas of those images, each bitwise equal to the one checked): the weight-gradient reference is mult
    times the recomputation on the images checked."""
    import torch.nn.functional as F
    from critic_vae_amd import layout as L
    i0, i1 = images if images is not None else (0, B)
    n, W = i1 - i0, h.width
    m = W // 64
    dev = ws.device
    ws16 = ws.view(torch.bfloat16)

    def slot(name, per):            # images [i0, i1) of a stored bf16 tensor with `per` elements per image, as a flat fp32 view
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        return ws[off + i0 * per // 2:off + i1 * per // 2]

    # neither y0 nor block 0's dy is stored: both exist only inside the fused E1 weight-gradient kernel.  Recompute y0 of the images
    # with the stand-alone conv op, then their d_y0 with the stand-alone BatchNorm-backward op from the a0 / d_a0 / coef0 the step left
    # (its batch sums over these images are the step's: every image occurs mult times in it)
    n_full, n_pool = W * W * 32, (W // 2) * (W // 2) * 32
    ow, nw = h.layout["enc0.w"]
    ob, nb = h.layout["enc0.b"]
    y0 = torch.empty(n * n_full // 2, device=dev)
    h.op_conv_fwd(0, n, x[i0:i1], theta[ow:ow + nw], theta[ob:ob + nb], y0, torch.empty(h.op_bn_partial_floats(0, n), device=dev))
    junk = torch.empty(3 * 32, device=dev)
    d_y0f = torch.empty(n * n_full // 2, device=dev)
    coef0 = h.ws_view(ws, B, "coef0", 128)
    h.op_bn_pool_act_bwd(0, n, y0, slot("a0", n_pool), slot("d_a0", n_pool), coef0, junk[:32], d_y0f, junk[32:64], junk[64:], None,
                         torch.empty(h.op_scratch_floats(n), device=dev))
    torch.cuda.synchronize()
    d_y0 = d_y0f.view(torch.bfloat16)

    def act(name, c, s):            # stored bf16 NHWC tensor -> fp32 NCHW on the CPU
        if name == "d_y0":
            return d_y0[:n * s * s * c].float().view(n, s, s, c).permute(0, 3, 1, 2).contiguous().cpu()
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        per = s * s * c
        return ws16[2 * off + i0 * per:2 * off + i1 * per].float().view(n, s, s, c).permute(0, 3, 1, 2).contiguous().cpu()

    ref = L.native_to_ref(h.layout, theta.cpu())
    grd = L.native_to_ref(h.layout, grads.cpu())
    bf = lambda t: t.to(torch.bfloat16).float()      # noqa: E731
    enc = [(3, 32, 64 * m), (32, 64, 32 * m), (64, 128, 16 * m), (128, 256, 8 * m)]
    dec = [(256, 128, 4 * m), (128, 64, 8 * m), (64, 32, 16 * m), (32, 32, 32 * m), (32, 3, 64 * m)]
    worst = {}

    def close(got, want, what, rel):
        scale = want.abs().max().item()
        err = (got - want).abs().max().item()
        worst[what] = err / max(scale, 1e-30)
        assert err <= rel * scale + 1e-12, f"{what}: err {err:.3e} vs max {scale:.3e}"

    def wgrad(inp, dout):           # dW (O,I,5,5), db of a 5x5 / pad 2 conv from its input and output gradient, times mult
        return (mult * torch.nn.grad.conv2d_weight(inp, (dout.shape[1], inp.shape[1], 5, 5), dout, padding=2),
                mult * dout.sum(dim=(0, 2, 3)))

    # ---- encoder: forward conv, weight / bias gradient, input gradient ----
    for l, (ci, co, s) in enumerate(enc):
        inp = bf(x[i0:i1].cpu()) if l == 0 else act(f"a{l - 1}", ci, s)
        wk, bk = f"encoder.model.{4 * l}.weight", f"encoder.model.{4 * l}.bias"
        y = F.conv2d(inp, bf(ref[wk]), ref[bk], padding=2)
        if l == 0:
            close(y0.view(torch.bfloat16)[:n * s * s * co].float().view(n, s, s, co).permute(0, 3, 1, 2).cpu(), y, "y0", 2.0 ** -8)
        else:
            close(act(f"y{l}", co, s), y, f"y{l}", 2.0 ** -8)
        dy = act(f"d_y{l}", co, s)
        dw, db = wgrad(inp, dy)
        close(grd[wk], dw, f"dW enc{l}", 2e-3)
        # pre-BatchNorm bias: the true gradient cancels to ~0, so compare against the size of the summed terms
        assert (grd[bk] - db).abs().max().item() <= 1e-5 * mult * dy.abs().sum(dim=(0, 2, 3)).max().item() + 1e-7, f"db enc{l}"
        if l > 0:
            da = F.conv_transpose2d(dy, bf(ref[wk]), padding=2)
            close(act(f"d_a{l - 1}", ci, s), da, f"d_a{l - 1}", 2.0 ** -8)
    # ---- decoder: D0 plain, D1..D3 behind a nearest-2x upsample (phase-collapsed in the kernels) ----
    for i, (ci, co, s) in enumerate(dec[:4]):
        src = act("h", 256, 4 * m) if i == 0 else act(f"o{i - 1}", ci, s // 2)
        inp = src if i == 0 else F.interpolate(src, scale_factor=2, mode="nearest")
        wk, bk = f"decoder.model.{3 * i}.weight", f"decoder.model.{3 * i}.bias"
        o = torch.relu(F.conv2d(inp, bf(ref[wk]), ref[bk], padding=2))
        # D1..D3 round the PRE-SUMMED collapsed weights to bf16, not the 5x5 ones: allow one more bf16 rounding
        close(act(f"o{i}", co, s), o, f"o{i}", 2.0 ** -8 if i == 0 else 2.0 ** -6)
        do = act(f"d_o{i}", co, s)
        dw, db = wgrad(inp, do)
        close(grd[wk], dw, f"dW dec{i}", 2e-3)
        close(grd[bk], db, f"db dec{i}", 2e-3)
    # ---- decoder_input: [zcat | 1]^T . d_h ----
    off = h.lib.cvae_ws_offset(h.h, B, b"zcat")
    zcat = ws[off + i0 * 33:off + i1 * 33].view(n, 33).cpu()
    dh = act("d_h", 256, 4 * m)                                        # (n,256,4,4) = the reference's view(-1,256,4,4)
    dwd = mult * (bf(zcat).t() @ dh.reshape(n, -1))                    # (33, 4096) in (C,H,W) column order
    close(grd["decoder.decoder_input.weight"], dwd.t().contiguous(), "dW decoder_input", 2e-3)
    close(grd["decoder.decoder_input.bias"], mult * dh.reshape(n, -1).sum(0), "db decoder_input", 2e-3)
    # ---- D4 (Upsample -> Conv(32->3) -> Tanh): forward on exact bf16 products; backward through G rounded to bf16 ----
    o3 = act("o3", 32, 32 * m)
    up3 = F.interpolate(o3, scale_factor=2, mode="nearest")
    w4, b4 = ref["decoder.model.12.weight"], ref["decoder.model.12.bias"]
    # the forward kernel contracts the PHASE-COLLAPSED 3x3 weights (sums of the 5x5 taps that reach one source pixel from
    # one output phase), summed in fp32 and rounded to bf16 once: reproduce exactly that
    taps = {0: [[0, 1], [2, 3], [4]], 1: [[0], [1, 2], [3, 4]]}
    pre = torch.empty(n, 3, W, W)
    for py in (0, 1):
        for px in (0, 1):
            wc = torch.zeros(3, 32, 3, 3)
            for ta in range(3):
                for tb in range(3):
                    for r in taps[py][ta]:
                        for s5 in taps[px][tb]:
                            wc[:, :, ta, tb] += w4[:, :, r, s5]
            pre[:, :, py::2, px::2] = F.conv2d(o3, bf(wc), b4, padding=1)
    rec = recon[i0:i1].cpu()
    close(rec, torch.tanh(pre), "recon", 1e-4)
    close(rec, torch.tanh(F.conv2d(up3, bf(w4), b4, padding=2)), "recon vs 5x5 weights", 2.0 ** -6)
    dout = (d_recon[i0:i1] * (1.0 - recon[i0:i1] ** 2)).cpu()
    dw4, db4 = wgrad(up3, dout)
    close(grd["decoder.model.12.weight"], dw4, "dW dec4", 1e-2)         # the 2x2-block sums G are rounded to bf16
    close(grd["decoder.model.12.bias"], db4, "db dec4", 1e-4)            # summed in fp32 from dOut itself
    d_up = F.conv_transpose2d(dout, bf(w4), padding=2)
    d_o3 = F.avg_pool2d(d_up, 2) * 4.0 * (o3 > 0).float()                # Upsample backward = 2x2 sum, then the ReLU mask
    close(act("d_o3", 32, 32 * m), d_o3, "d_o3", 2.0 ** -6)
    return worst
