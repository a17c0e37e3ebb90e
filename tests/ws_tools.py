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


# ---- poisoned buffers: results must not depend on what the caller's workspace, scratch and outputs held on entry ----
ZERO = 0x00000000         # the baseline
ALL_ONES = 0xFFFFFFFF     # a NaN as fp32, as each bf16 half and as fp64; the largest unsigned (the MS-SSIM arrival ticket)
HUGE = 0x7F7F7F7F         # 3.39e38 as fp32 and as each bf16 half, a huge finite fp64: survives the fmaxf / compares that swallow a NaN
FILLS = (("zero", ZERO), ("huge", HUGE), ("ones", ALL_ONES))       # HUGE runs before ALL_ONES


def poison(t, pattern):
    """Fill every byte of the contiguous device tensor t (any dtype) with the 32-bit pattern, repeated from t's first byte on
    (little endian), through an int32 view, or a uint8 view where t's size or address is no multiple of 4 bytes."""
    assert t.is_contiguous(), "poison: need a contiguous tensor"
    pattern &= 0xFFFFFFFF
    flat = t.reshape(-1)
    if flat.numel() == 0:
        return t
    if (flat.numel() * flat.element_size()) % 4 == 0 and flat.data_ptr() % 4 == 0:
        flat.view(torch.int32).fill_(pattern - (1 << 32) if pattern >= 1 << 31 else pattern)
    else:
        b = flat.view(torch.uint8)
        for k in range(4):
            b[k::4] = (pattern >> (8 * k)) & 0xFF
    return t


def bits(t):
    """t as a flat integer view, so that NaNs compare as the bits they are."""
    flat = t.contiguous().reshape(-1)
    return flat if not flat.dtype.is_floating_point else flat.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[flat.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def holds(t, pattern):
    """True where the 32-bit words of t (fp32 / int32) still hold the pattern."""
    return bits(t) == (pattern - (1 << 32) if pattern >= 1 << 31 else pattern)


class StepRig:
    """One model and handle with every buffer of the step owned here, as the training loop owns them: workspace, outputs, gradient
    buffer and sync record from torch.empty, none of them ever cleared.  The calls are the Handle-level ones (forward, loss, backward or
    the stages); the BatchNorm running statistics, the step's one piece of state, are set by the caller of step()."""
    OUT = ("mu", "logvar", "recon", "scalars", "d_recon", "d_mu", "d_logvar", "grads")

    def __init__(self, width, max_batch, precision, wseed=0):
        from critic_vae_amd import synth
        from critic_vae_amd.lib import SYNC_DOUBLES
        from critic_vae_amd.nets import VariationalAutoencoder
        vae = VariationalAutoencoder(max_batch=max_batch, seed=wseed, width=width, precision=precision).cuda()
        vae.load_reference_params(synth.make_params(wseed, width))
        self.vae, self.h, self.width, self.max_batch = vae, vae.handle, width, max_batch
        self.theta = vae.theta.data
        self.bn0 = vae.bn_state.clone()
        dev = self.theta.device
        self.ws = vae._workspace(max_batch)             # torch.empty; decisions.hip_decisions reads the same tensor through the model
        self.mu = torch.empty(max_batch, 32, device=dev)
        self.logvar, self.d_mu, self.d_logvar = (torch.empty_like(self.mu) for _ in range(3))
        self.recon = torch.empty(max_batch, 3, width, width, device=dev)
        self.d_recon = torch.empty_like(self.recon)
        self.scalars = torch.empty(16, device=dev)
        self.grads = torch.empty_like(self.theta)
        self.sync = torch.empty(SYNC_DOUBLES, dtype=torch.float64, device=dev)
        self.used = torch.zeros(self.grads.numel(), dtype=torch.bool, device=dev)       # gradient elements that belong to a tensor
        for off, n in self.h.layout.values():
            self.used[off:off + n] = True

    def poison(self, pattern, workspace=True):
        """The whole workspace, every output and the sync record."""
        for t in ([self.ws] if workspace else []) + [getattr(self, k) for k in self.OUT] + [self.sync]:
            poison(t, pattern)

    def step(self, B, x, pred, eps, bn=None, zero_padding=True):
        """forward(train) + loss + backward on the running statistics `bn` (default: the initial ones); nothing touched in between."""
        h, v = self.h, self.vae
        v.bn_state.copy_(self.bn0 if bn is None else bn)
        h.forward(B, x, pred, eps, self.theta, v.bn_state, self.mu, self.logvar, self.recon, self.ws, train=True)
        h.loss(B, x, self.mu, self.logvar, self.recon, self.ws, self.scalars, self.d_recon, self.d_mu, self.d_logvar)
        h.backward(B, x, pred, eps, self.theta, self.logvar, self.recon, self.d_recon, self.d_mu, self.d_logvar, self.ws, self.grads,
                   zero_padding=zero_padding)
        torch.cuda.synchronize()
        v.theta.grad = self.grads                       # decisions.check_step_against_oracle reads the model's .grad
        return self.outputs(B)

    def staged(self, B, x, pred, eps, bn=None):
        """The same step through the stages of one rank (no exchange): forward 0..4, loss 0..1, backward 0..4."""
        h, v = self.h, self.vae
        v.bn_state.copy_(self.bn0 if bn is None else bn)
        for k in range(5):
            h.forward_stage(k, B, x, pred, eps, self.theta, v.bn_state, self.mu, self.logvar, self.recon, self.ws, self.sync)
        for k in range(2):
            h.loss_stage(k, B, x, self.mu, self.logvar, self.recon, self.ws, self.scalars, self.d_recon, self.d_mu, self.d_logvar, self.sync)
        for k in range(5):
            h.backward_stage(k, B, x, pred, eps, self.theta, self.logvar, self.recon, self.d_recon, self.d_mu, self.d_logvar, self.ws,
                             self.grads, self.sync)
        torch.cuda.synchronize()
        return self.outputs(B)

    def padding_written(self, grads, pattern):
        """Names of the parameter tensors behind which the alignment padding of `grads` no longer holds the pattern."""
        kept = holds(grads, pattern)
        return [name for name, (off, n) in self.h.layout.items() if not bool(kept[off + n:(off + n + 63) // 64 * 64].all())]

    def outputs(self, B):
        """Copies of everything the step returns: the B rows of the per-image outputs, the 13 documented scalars (include/cvae.h: 13..15
        are reserved), the whole gradient buffer with its padding, the running statistics."""
        out = {k: getattr(self, k)[:B].clone() for k in ("mu", "logvar", "recon", "d_recon", "d_mu", "d_logvar")}
        out.update(scalars=self.scalars[:13].clone(), grads=self.grads.clone(), bn_state=self.vae.bn_state.clone())
        return out


def assert_same_outputs(got, want, what, skip=()):
    """Every tensor of two StepRig.outputs() dicts, bit for bit (NaNs included)."""
    for k in want:
        if k in skip:
            continue
        if not same_bits(got[k], want[k]):
            d = bits(got[k]) != bits(want[k])
            i = int(d.flatten().nonzero()[0])
            raise AssertionError(f"{what}: {k} differs in {int(d.sum())} of {d.numel()} elements, first at flat index {i}: "
                                 f"{got[k].flatten()[i].item()!r} vs {want[k].flatten()[i].item()!r}")


U32 = 2.0 ** -24          # fp32 unit roundoff
BF16 = 2.0 ** -8          # one round-to-nearest bf16 rounding (8 significant bits): |bf16(v) - v| <= 2^-8 |v|
FC_KS = 32                # fc.hip: K slices of latent_gemm, summed by fc_finish / decin_dz_finish
BN_OFF = (0, 32, 96, 224)  # per-block channel offsets of the running means (bn_state[0:480]) and variances (bn_state[480:960])
# BatchNorm forward statistics: every partial is an fp32 sum of at most 512 conv outputs, taken before the bf16 rounding (conv_epilogue.h:
# per-tile sum / M2 of the accumulators; conv_thin.hip: the strip's raw S0 / Q0; conv_bf16_big.hip: M2 in double), with chains of at most
# 128 additions plus a tree of 16: <= 144 u = 8.6e-6 of the sum of |terms|, merged in fp64 (bn_fwd_reduce / finalize).
BN_STAT_REL = 1e-5


def within(what, got, want, bound, worst=None):
    """Elementwise |got - want| <= bound, every element, a NaN fails.  Returns the largest err / allowed (<= 1 passes) and, when
    `worst` is a dict, records it there under `what` before it asserts."""
    got, want, bound = got.double(), want.double(), bound.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    r = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    if worst is not None:
        worst[what] = r
    if not r <= 1.0:
        k = int(torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf")).flatten().argmax())
        raise AssertionError(f"{what}: err / allowed {r:.3e} (at flat index {k}: got {got.flatten()[k].item():.6e}, "
                             f"want {want.flatten()[k].item():.6e}, allowed {bound.flatten()[k].item():.3e})")
    return r


# ---- term counts of the latent-layer links (fc.hip): the worst-case fp32 error of a sum is (terms) * U32 * sum |addends| ----
def fc_split_terms(K, bias):
    """latent_gemm + fc_finish / decin_dz_finish: each of the FC_KS slices sums K / FC_KS products in series (a product is rounded: +1),
    then the FC_KS slabs are added in series, after the bias where there is one (+1)."""
    return K // FC_KS + 1 + FC_KS + (1 if bias else 0)


DECIN_TERMS = 33 + 1      # decin_fwd: fmaf from the bias over i = 0..32
DML_TERMS = 8             # fc_bwd_prep: expf (a few ulps), three products and the sum, per element of dml
DFLAT_TERMS = 64 + DML_TERMS      # fc_bwd_dflat: 64 fmaf in series per output, on a dml that carries DML_TERMS roundings of its terms
ZCAT_TERMS = 8            # fc_finish: expf (a few ulps), the product and the sum: 8 ulps of the two terms


def batch_terms(B):
    """The batch-contracted sums (bgemm_*: dW fc, dW / db decoder_input; colsum: db fc): at most B additions in any order, the
    three partial-tile additions of the last stage, one product rounding."""
    return B + 4


_within = within          # check_bf16_stored_operands binds the name to its own record of worst ratios


def check_bf16_stored_operands(h, tr, B, x, pred, eps, theta, bn_before, bn_after, images=None, mult=1, ties=None):
    """After one bf16-mode step of B images on handle h: recompute every link of the step on the CPU from the operands the kernels
    stored and compare.  tr holds the step's buffers (ws, grads, mu, logvar, recon, d_recon, d_mu, d_logvar, scalars: a FusedTrainer
    or anything with those attributes); x, pred, eps are the step's inputs, theta its parameters, bn_before / bn_after the BatchNorm
    running statistics before and after the forward.  Operands are what each kernel reads: bf16 activations as stored, fp32 weights
    where the kernel takes fp32 (latent_gemm, decin_fwd, fc_bwd_dflat), weights rounded to bf16 where the packed copies are.

    Links, in the order the step computes them, so that a wrong stored result fails at the link that produced it before any link
    that reads it (each assertion message starts with the link's name):
      y{l}, coef{l} mean / var, running_mean{l} / running_var{l}, a{l}   per encoder block: the conv; the batch statistics of its fp32
                  output (recomputed), the running statistics (unbiased over the WHOLE batch); act(maxpool(fma(y, scale, shift))) of
                  the stored bf16 y and coef, one bf16 rounding
      mu, logvar, zcat   a3 (NCHW flatten) . [fc_mu | fc_var]^T + b, fp32 summation order;  [mu + eps exp(logvar / 2) | pred]
      h, o{i}, recon     zcat . Wd^T + bd, one bf16 rounding;  the decoder convs and D4
      loss scalars, loss d_recon / d_mu / d_logvar   the oracle's MS-SSIM + KL on the stored recon / mu / logvar: scalars to 2e-5,
                  gradients to 1e-4 of their max (the test_msssim bars)
      dW / db dec4, d_o3, dW / db dec{i}, dW / db decoder_input, d_zcat (d_h . Wd), d_a3 (dml . Wfc, one bf16 rounding), dW / db fc
      dgamma{l}, dbeta{l}, d_y{l} (l = 1..3), dW / db enc{l}, d_a{l-1}   per encoder block, last first: the bn.hip backward
                  (gradient at the first window maximum), one bf16 rounding; the conv gradients
    Activations and activation gradients: elementwise, one bf16 rounding of the stored result plus the bound of the fp32 arithmetic
    that produced it; sums: the worst-case fp32 error depth * 2^-24 of the sum of |terms|, depth = the longest chain of additions
    the kernel's fixed order takes.  Weight / bias gradients of the convs and fc layers: 2e-3 of the tensor max.
    images = (i0, i1): only images [i0, i1) are read and recomputed (default: all B).  mult: every image of the step occurs `mult`
    times in it (a batch of replicas of those images, each bitwise equal to the one checked): batch statistics are the images' own,
    sums over the batch are mult times theirs, per-image loss gradients (i1 - i0) / B times the checked images' loss gradients.
    Returns {link: largest err / allowed err} (<= 1 passes).  ties: a dict that receives, per d_y{l}, the number of windows whose two
    largest normalised values are within 4 fp32 ulps (not equal): there only the window sum is compared, and the routed gradient must
    sit at one of the near-tied positions."""
    import torch.nn.functional as F
    from critic_vae_amd import layout as L
    from oracle import cvae_oracle as orc
    ws, grads, recon, d_recon = tr.ws, tr.grads, tr.recon, tr.d_recon
    i0, i1 = images if images is not None else (0, B)
    n, W = i1 - i0, h.width
    m = W // 64
    K = 4096 * m * m
    dev = ws.device
    ws16 = ws.view(torch.bfloat16)
    worst = {}
    ties = ties if ties is not None else {}

    def slot(name, per):            # images [i0, i1) of a stored bf16 tensor with `per` elements per image, as a flat fp32 view
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        return ws[off + i0 * per // 2:off + i1 * per // 2]

    def f32slot(name, per):         # images [i0, i1) of a stored fp32 tensor, (n, per) float64 on the CPU
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        return ws[off + i0 * per:off + i1 * per].view(n, per).double().cpu()

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
        if name == "y0":
            return y0.view(torch.bfloat16)[:n * s * s * c].float().view(n, s, s, c).permute(0, 3, 1, 2).contiguous().cpu()
        off = h.lib.cvae_ws_offset(h.h, B, name.encode())
        assert off >= 0, name
        per = s * s * c
        return ws16[2 * off + i0 * per:2 * off + i1 * per].float().view(n, s, s, c).permute(0, 3, 1, 2).contiguous().cpu()

    ref = L.native_to_ref(h.layout, theta.cpu())
    grd = L.native_to_ref(h.layout, grads.cpu())
    bf = lambda t: t.to(torch.bfloat16).to(t.dtype)      # noqa: E731
    enc = [(3, 32, 64 * m), (32, 64, 32 * m), (64, 128, 16 * m), (128, 256, 8 * m)]
    dec = [(256, 128, 4 * m), (128, 64, 8 * m), (64, 32, 16 * m), (32, 32, 32 * m), (32, 3, 64 * m)]

    def close(got, want, what, rel):
        scale = want.abs().max().item()
        err = (got - want).abs().max().item()
        worst[what] = err / max(rel * scale, 1e-30)
        assert err <= rel * scale + 1e-12, f"{what}: err {err:.3e} vs max {scale:.3e}"

    def within(what, got, want, bound):     # elementwise |got - want| <= bound (NaN fails), recorded in `worst`
        return _within(what, got, want, bound, worst)

    def wgrad(inp, dout):           # dW (O,I,5,5), db of a 5x5 / pad 2 conv from its input and output gradient, times mult
        return (mult * torch.nn.grad.conv2d_weight(inp, (dout.shape[1], inp.shape[1], 5, 5), dout, padding=2),
                mult * dout.sum(dim=(0, 2, 3)))

    # ---- encoder forward: per block the conv, its BatchNorm statistics and running statistics, BatchNorm / pool / act ----
    bn0, bn1 = bn_before.double().cpu(), bn_after.double().cpu()

    def windows(l, co, s):          # stored bf16 y of block l as 2x2 windows (scan order (0,0) (0,1) (1,0) (1,1)), coef, fmaf(y, sc, sh)
        cf = h.ws_view(ws, B, f"coef{l}", 4 * co).double().cpu().view(co, 4)
        c4 = [cf[:, k].view(1, co, 1, 1, 1) for k in range(4)]
        yw = act(f"y{l}", co, s).double().view(n, co, s // 2, 2, s // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, co, s // 2, s // 2, 4)
        return cf, c4, yw, (yw * c4[0] + c4[1]).float().double()      # fmaf: one fp32 rounding of the exact value

    for l, (ci, co, s) in enumerate(enc):
        inp = bf(x[i0:i1].cpu()) if l == 0 else act(f"a{l - 1}", ci, s)
        wk, bk = f"encoder.model.{4 * l}.weight", f"encoder.model.{4 * l}.bias"
        y = F.conv2d(inp, bf(ref[wk]), ref[bk], padding=2)
        close(act(f"y{l}", co, s), y, f"y{l}", 2.0 ** -8)               # block 0: the y0 recomputed above
        # -- statistics: the kernels sum the fp32 conv output before rounding it, so compare with the batch statistics of y --
        cf, (sc, sh, mn, istd), yw, nwin = windows(l, co, s)
        yd = y.double()
        mean, var = yd.mean(dim=(0, 2, 3)), yd.var(dim=(0, 2, 3), unbiased=False)
        sq = (yd ** 2).mean(dim=(0, 2, 3)) + ((yd - ref[bk].double().view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        within(f"coef{l} mean", cf[:, 2], mean, BN_STAT_REL * sq.sqrt())
        # invstd = 1 / sqrtf(var + 1e-5) in fp32 (a few ulps: 16 u of var + eps); the E1 strips' M2 = Q0 - S0^2 / n is about the
        # bias, the others' about the tile mean: bound against both second moments
        var_b = 2 * BN_STAT_REL * sq + 16 * U32 * (var + 1e-5)
        within(f"coef{l} var", 1.0 / cf[:, 3] ** 2 - 1e-5, var, var_b)
        o = BN_OFF[l]
        rm0, rv0 = bn0[o:o + co], bn0[480 + o:480 + o + co]
        N = B * s * s                                                   # the WHOLE batch's pixel count
        within(f"running_mean{l}", bn1[o:o + co], 0.9 * rm0 + 0.1 * cf[:, 2], 4 * U32 * (0.9 * rm0.abs() + 0.1 * cf[:, 2].abs()))
        rv = 0.9 * rv0 + 0.1 * var * N / (N - 1)
        within(f"running_var{l}", bn1[480 + o:480 + o + co], rv, 0.1 * var_b * N / (N - 1) + 4 * U32 * rv.abs())
        # -- a = act(max over the 2x2 window of fmaf(y, scale, shift)) on the stored bf16 y, one bf16 rounding --
        top = nwin.max(dim=-1).values
        a_ref = torch.tanh(top) if l == 3 else top.clamp_min(0.0)
        within(f"a{l}", act(f"a{l}", co, s // 2), a_ref, (BF16 + 4 * U32) * a_ref.abs())
    # ---- fc_mu | fc_var (latent_gemm<false, bf16>: bf16 a3 x fp32 weights on the fp32 MFMA, FC_KS K slices) + fc_finish ----
    mu_g, lv_g = tr.mu[i0:i1].cpu(), tr.logvar[i0:i1].cpu()
    a3 = act("a3", 256, 4 * m).double().reshape(n, K)                   # NCHW flatten = the reference's view(-1, 256 * s * s)
    wfc = torch.cat((ref["encoder.fc_mu.weight"], ref["encoder.fc_var.weight"]), 0).double()           # (64, K)
    bfc = torch.cat((ref["encoder.fc_mu.bias"], ref["encoder.fc_var.bias"]), 0).double()
    ml = a3 @ wfc.t() + bfc
    ml_abs = (a3.abs() @ wfc.abs().t() + bfc.abs()) * (fc_split_terms(K, bias=True) * U32)
    within("mu", mu_g, ml[:, :32], ml_abs[:, :32])
    within("logvar", lv_g, ml[:, 32:], ml_abs[:, 32:])
    zc = f32slot("zcat", 33)
    e_, p_ = eps[i0:i1].double().cpu(), pred[i0:i1].double().cpu()
    se = e_ * torch.exp(0.5 * lv_g.double())
    within("zcat", zc[:, :32], mu_g.double() + se, ZCAT_TERMS * U32 * (mu_g.double().abs() + se.abs()))
    assert torch.equal(zc[:, 32:], p_), "zcat: the pred column is not the step's pred"

    # ---- decoder_input forward (decin_fwd<bf16>: fp32 zcat, fp32 Wd, fmaf from the bias over i = 0..32, bf16 store) ----
    wd = ref["decoder.decoder_input.weight"].double()                   # (K, 33), rows in (C, H, W) order
    bd = ref["decoder.decoder_input.bias"].double()
    hr = (zc @ wd.t() + bd).view(n, 256, 4 * m, 4 * m)
    hb = (zc.abs() @ wd.abs().t() + bd.abs()).view(n, 256, 4 * m, 4 * m) * (DECIN_TERMS * U32)
    within("h", act("h", 256, 4 * m), hr, BF16 * hr.abs() + (1 + BF16) * hb)
    # ---- decoder forward: D0 plain, D1..D3 behind a nearest-2x upsample (phase-collapsed in the kernels) ----
    for i, (ci, co, s) in enumerate(dec[:4]):
        src = act("h", 256, 4 * m) if i == 0 else act(f"o{i - 1}", ci, s // 2)
        inp = src if i == 0 else F.interpolate(src, scale_factor=2, mode="nearest")
        wk, bk = f"decoder.model.{3 * i}.weight", f"decoder.model.{3 * i}.bias"
        o = torch.relu(F.conv2d(inp, bf(ref[wk]), ref[bk], padding=2))
        # D1..D3 round the PRE-SUMMED collapsed weights to bf16, not the 5x5 ones: allow one more bf16 rounding
        close(act(f"o{i}", co, s), o, f"o{i}", 2.0 ** -8 if i == 0 else 2.0 ** -6)
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
    # ---- loss (msssim.hip, shared with fp32 mode): the oracle on the stored recon, x, mu, logvar ----
    rec = recon[i0:i1].cpu().clone().requires_grad_(True)
    mu_r, lv_r = mu_g.clone().requires_grad_(True), lv_g.clone().requires_grad_(True)
    lo = orc.vae_loss(x[i0:i1].cpu(), mu_r, lv_r, rec)
    lo["total_loss"].backward()
    want = torch.cat([torch.stack([lo["total_loss"], lo["recon_loss"], lo["KLD"]]).detach().float(), lo["ssim_levels"].float(),
                      lo["cs_levels"].float()])
    within("loss scalars", tr.scalars[:13].cpu(), want, torch.full((13,), 2e-5))
    per = n / B                         # a batch-mean loss: the full batch's per-image gradient is n / B times the n images'
    for what, got, g in (("loss d_recon", d_recon[i0:i1].cpu(), rec.grad), ("loss d_mu", tr.d_mu[i0:i1].cpu(), mu_r.grad),
                         ("loss d_logvar", tr.d_logvar[i0:i1].cpu(), lv_r.grad)):
        want = per * g.double()
        within(what, got, want, torch.full_like(want, 1e-4 * want.abs().max().item()))

    # ---- D4 backward ----
    dout = (d_recon[i0:i1] * (1.0 - recon[i0:i1] ** 2)).cpu()
    dw4, db4 = wgrad(up3, dout)
    close(grd["decoder.model.12.weight"], dw4, "dW dec4", 1e-2)         # the 2x2-block sums G are rounded to bf16
    close(grd["decoder.model.12.bias"], db4, "db dec4", 1e-4)            # summed in fp32 from dOut itself
    d_up = F.conv_transpose2d(dout, bf(w4), padding=2)
    d_o3 = F.avg_pool2d(d_up, 2) * 4.0 * (o3 > 0).float()                # Upsample backward = 2x2 sum, then the ReLU mask
    close(act("d_o3", 32, 32 * m), d_o3, "d_o3", 2.0 ** -6)
    # ---- decoder backward: D3..D0 weight / bias gradients ----
    for i in (3, 2, 1, 0):
        ci, co, s = dec[i]
        src = act("h", 256, 4 * m) if i == 0 else act(f"o{i - 1}", ci, s // 2)
        inp = src if i == 0 else F.interpolate(src, scale_factor=2, mode="nearest")
        wk, bk = f"decoder.model.{3 * i}.weight", f"decoder.model.{3 * i}.bias"
        dw, db = wgrad(inp, act(f"d_o{i}", co, s))
        close(grd[wk], dw, f"dW dec{i}", 2e-3)
        close(grd[bk], db, f"db dec{i}", 2e-3)
    # ---- decoder_input: [zcat | 1]^T . d_h ----
    dh = act("d_h", 256, 4 * m)                                        # (n,256,4,4) = the reference's view(-1,256,4,4)
    dwd = mult * (bf(zc.float()).t() @ dh.reshape(n, -1))                    # (33, 4096) in (C,H,W) column order
    close(grd["decoder.decoder_input.weight"], dwd.t().contiguous(), "dW decoder_input", 2e-3)
    close(grd["decoder.decoder_input.bias"], mult * dh.reshape(n, -1).sum(0), "db decoder_input", 2e-3)
    # ---- decoder_input input gradient (latent_gemm<true, bf16> + decin_dz_finish): d_h . Wd ----
    dh_flat = act("d_h", 256, 4 * m).double().reshape(n, K)
    dz = f32slot("d_zcat", 33)
    within("d_zcat", dz, dh_flat @ wd, (dh_flat.abs() @ wd.abs()) * (fc_split_terms(K, bias=False) * U32))
    # ---- fc backward: dml (fc_bwd_prep), d_a3 = dml . Wfc (fc_bwd_dflat<bf16>), dWfc = a3^T . bf16(dml), dbfc = colsum(dml) ----
    lvd = lv_g.double()
    ex = 0.5 * e_ * torch.exp(0.5 * lvd)
    dml = torch.cat((dz[:, :32] + tr.d_mu[i0:i1].double().cpu(), dz[:, :32] * ex + tr.d_logvar[i0:i1].double().cpu()), 1)
    dml_abs = torch.cat((dz[:, :32].abs() + tr.d_mu[i0:i1].double().cpu().abs(),
                         (dz[:, :32] * ex).abs() + tr.d_logvar[i0:i1].double().cpu().abs()), 1)
    da3 = (dml @ wfc).view(n, 256, 4 * m, 4 * m)
    da3_b = (dml_abs @ wfc.abs()).view(n, 256, 4 * m, 4 * m) * (DFLAT_TERMS * U32)
    within("d_a3", act("d_a3", 256, 4 * m), da3, BF16 * da3.abs() + (1 + BF16) * da3_b)
    dwfc = mult * (bf(dml).t() @ a3)                                    # the bf16 MFMA takes dml rounded to bf16
    close(grd["encoder.fc_mu.weight"], dwfc[:32], "dW fc_mu", 2e-3)
    close(grd["encoder.fc_var.weight"], dwfc[32:], "dW fc_var", 2e-3)
    dbfc = mult * dml.sum(0)
    close(grd["encoder.fc_mu.bias"], dbfc[:32], "db fc_mu", 2e-3)
    close(grd["encoder.fc_var.bias"], dbfc[32:], "db fc_var", 2e-3)

    # ---- encoder backward, last block first ----
    for l in (3, 2, 1, 0):
        ci, co, s = enc[l]
        inp = bf(x[i0:i1].cpu()) if l == 0 else act(f"a{l - 1}", ci, s)
        wk, bk = f"encoder.model.{4 * l}.weight", f"encoder.model.{4 * l}.bias"
        cf, (sc, sh, mn, istd), yw, nw_ = windows(l, co, s)
        a_st = act(f"a{l}", co, s // 2).double()
        # -- backward statistics (bn_bwd_stats_relu_kernel<__bf16> / bn_bwd_kernel<__bf16, 1, 0>) -> dgamma = s2, dbeta = s1, k = s / N --
        da = act(f"d_a{l}", co, s // 2).double()
        g = da * (1.0 - a_st ** 2) if l == 3 else da * (a_st > 0)
        pos = nw_.argmax(dim=-1, keepdim=True)                         # first maximum in scan order, as the kernels take it
        xw = (yw - mn) * istd
        xm = xw.gather(-1, pos)[..., 0]
        xw_abs = (yw.abs() + mn.abs()) * istd                          # the size of xhat's fp32 terms
        xm_abs = xw_abs.gather(-1, pos)[..., 0]
        gam = (sc / istd)[..., 0]
        bet = (sh + mn * sc)[..., 0]
        if l == 3:                                                      # tanh block: xhat from y at the argmax
            xs, xs_abs = xm, xm_abs
        else:                                                           # ReLU blocks: xhat = (a - beta) / gamma, unless |gamma| < 1e-2
            tiny = gam.abs() < 1e-2
            safe = torch.where(tiny, torch.ones_like(gam), gam)
            xs = torch.where(tiny, xm, (a_st - bet) / safe)
            xs_abs = torch.where(tiny, xm_abs, (a_st.abs() + bet.abs()) / safe.abs())
        s1, s2 = g.sum(dim=(0, 2, 3)), (g * xs).sum(dim=(0, 2, 3))
        t1, t2 = g.abs().sum(dim=(0, 2, 3)), (g.abs() * xs_abs).sum(dim=(0, 2, 3))     # + a few roundings per term: depth + 4
        # depth of the fixed-order sums: pixels per thread, the workgroup's NSUB rows in series, then at most nblk partials
        tot = B * (s // 2) ** 2
        nblk = max(1, min(1024, tot // ((256 // co) * 8)))
        nsub = 256 // (co // 8)
        ppb = -(-tot // nblk)
        depth = -(-ppb // nsub) + nsub + nblk + 4
        gk, bek = f"encoder.model.{4 * l + 1}.weight", f"encoder.model.{4 * l + 1}.bias"
        within(f"dgamma{l}", grd[gk], mult * s2, mult * depth * U32 * t2)
        within(f"dbeta{l}", grd[bek], mult * s1, mult * depth * U32 * t1)
        if l > 0:                   # -- the apply pass: dy = scale * ([p == argmax] g - k1 - xhat k2), bf16 --
            Nk = n * s * s
            k1, k2 = (s1 / Nk).view(1, co, 1, 1, 1), (s2 / Nk).view(1, co, 1, 1, 1)
            dk1, dk2 = (depth * U32 * t1 / Nk).view(1, co, 1, 1, 1), (depth * U32 * t2 / Nk).view(1, co, 1, 1, 1)
            sel = torch.zeros_like(xw).scatter_(-1, pos, g[..., None])
            base = -k1 - xw * k2
            d_ref = sc * (sel + base)
            bnd = BF16 * d_ref.abs() + (1 + BF16) * sc.abs() * (dk1 + xw.abs() * dk2 + 4 * U32 * (sel.abs() + k1.abs() + xw_abs * k2.abs()))
            d_st = act(f"d_y{l}", co, s).double().view(n, co, s // 2, 2, s // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, co, s // 2, s // 2, 4)
            srt = nw_.sort(dim=-1, descending=True).values
            gap = srt[..., 0] - srt[..., 1]
            near = (gap > 0) & (gap <= 4 * 2.0 ** -23 * srt[..., 0].abs()) & (g != 0)
            far = ~near
            within(f"d_y{l}", d_st[far], d_ref[far], bnd[far])
            ties[f"d_y{l}"] = int(near.sum())
            if near.any():          # which near-tied position wins is not fixed by the operands: the window sum is, and the routed
                within(f"d_y{l} near-tie window sums", d_st.sum(-1)[near], d_ref.sum(-1)[near], bnd.sum(-1)[near])
                routed = (d_st - sc * base).abs().argmax(dim=-1, keepdim=True)      # gradient must sit at a near-tied position
                nr = nw_.gather(-1, routed)[..., 0]
                assert bool((nr[near] >= srt[..., 0][near] - 4 * 2.0 ** -23 * srt[..., 0][near].abs()).all()), \
                    f"d_y{l}: a near-tie window routes its gradient to a position that is not near the maximum"
        dy = act(f"d_y{l}", co, s)
        dw, db = wgrad(inp, dy)
        close(grd[wk], dw, f"dW enc{l}", 2e-3)
        # pre-BatchNorm bias: the true gradient cancels to ~0, so compare against the size of the summed terms
        assert (grd[bk] - db).abs().max().item() <= 1e-5 * mult * dy.abs().sum(dim=(0, 2, 3)).max().item() + 1e-7, f"db enc{l}"
        if l > 0:
            da_ = F.conv_transpose2d(dy, bf(ref[wk]), padding=2)
            close(act(f"d_a{l - 1}", ci, s), da_, f"d_a{l - 1}", 2.0 ** -8)
    return worst


# ---- BatchNorm / pool / activation (bn.hip, reduce.hip): launch geometry, term counts, inputs and float64 references ----
BN_CH = (32, 64, 128, 256)        # channels of the four encoder blocks; their conv output is 64, 32, 16, 8 pixels wide at 64 x 64 frames
TANH_ULPS = 5                     # tanhf of the device library: the OpenCL bound it is built to; an fp32 ulp is at most 2 U32 |v|
DY_ULPS = 6                       # bn_bwd_kernel<.., 1>: the longest chain of roundings a term of dy passes through (test_gpu_bn_ops.py)
XS_ULPS = 8                       # bn_bwd_stats_relu_kernel: roundings behind the numerator and 1 / gamma of xhat = (a - beta) (1 / gamma)


def _cdiv(a, b):
    return -(-a // b)


def bn_layer(layer, W):
    """(C, H) of encoder block `layer` at W x W frames: bn_geom."""
    return BN_CH[layer], (64 >> layer) * (W // 64)


def bn_part_geom(layer, H):
    """(images per tile, pixels per image, tiles per image) of the partials a block's conv emits: part_geom / tile_geom."""
    if layer == 0:
        return 1, 512, (H // 16) * (H // 32)
    tw = min(H, 32)
    th = min(128 // tw, H)
    return 128 // (tw * th), tw * th, (H // tw) * (H // th)


def bn_num_tiles(layer, H, B):
    imgs, _, tpi = bn_part_geom(layer, H)
    return _cdiv(B, imgs) * tpi


def bn_fwd_chunks(num_tiles):
    """(tiles per chunk, chunks) of bn_fwd_reduce: tpb = cdiv(numTiles, 32), RA = cdiv(numTiles, tpb)."""
    tpb = _cdiv(num_tiles, 32)
    return tpb, _cdiv(num_tiles, tpb)


def bn_bwd_blocks(total_px, C):
    """Workgroups of the backward passes: at least 8 pooled pixels per thread, between 1 and 1024."""
    return max(1, min(1024, total_px // ((256 // C) * 8)))


def bn_bwd_ppb(total_px, C):
    """Pooled pixels per workgroup of the backward passes."""
    return _cdiv(total_px, bn_bwd_blocks(total_px, C))


def bn_sweep_items(cus):
    """Items one sweep of bn_pool_act_fwd's grid covers: 16 workgroups of 256 threads per compute unit."""
    return 16 * cus * 256


def bn_width(bf16, apply=False):
    """Channels per thread (BnWidth): W of the forward and the ReLU statistics, WB of bn_bwd_kernel (apply = True)."""
    return 8 if bf16 else (1 if apply else 4)


def bn_facts(W, layer, B, bf16, cus=256):
    """Every batch-dependent launch decision of one (frame size, block, batch, storage type)."""
    C, H = bn_layer(layer, W)
    imgs, ppi, tpi = bn_part_geom(layer, H)
    nt = bn_num_tiles(layer, H, B)
    tpb, RA = bn_fwd_chunks(nt)
    px = B * (H // 2) ** 2
    nblk, ppb = bn_bwd_blocks(px, C), bn_bwd_ppb(px, C)
    total = px * C // bn_width(bf16)
    return dict(C=C, H=H, N=B * H * H, imgs=imgs, ppi=ppi, tpi=tpi, tiles=nt, tpb=tpb, RA=RA, last_chunk=nt - (RA - 1) * tpb,
                last_ni=B - (_cdiv(B, imgs) - 1) * imgs, px=px, nblk=nblk, ppb=ppb, live=_cdiv(px, ppb), total=total,
                sweeps=_cdiv(total, bn_sweep_items(cus)))


# the edges of ISSUE / LABNOTES, each as a predicate on bn_facts; a case runs at the smallest batch that meets it ("below": the largest
# batch that does not) and asserts it again on the device it runs on
BN_EDGES = {
    "n64": lambda f: f["N"] == 64,                                              # the smallest count: N / (N - 1) at its largest
    "one-tile": lambda f: f["tiles"] == 1 and f["last_ni"] == f["imgs"],
    "rows64": lambda f: f["nblk"] == 64,                                        # 64 partial rows: straight into the finalize
    "rows65": lambda f: f["nblk"] > 64,                                         # rows_sum_kernel first, ragged last chunk; rows_sum_1024
    "tiles32": lambda f: f["tiles"] == 32 and f["tpb"] == 1,                    # the last batch inside 32 one-tile chunks
    "tiles33": lambda f: f["tiles"] > 32,                                       # two tiles per chunk, RA < 32
    "wrap": lambda f: f["tpb"] >= 9,                                            # the eight row groups take a second tile
    "sweep": lambda f: f["sweeps"] > 1,                                         # the forward's grid-stride loop runs
}
BN_BELOW = {"below-sweep": "sweep"}
# (W, layer, edge, storage types)
BN_CASES = ([(64, 3, e, ("f32", "bf16")) for e in ("n64", "one-tile", "rows64", "rows65", "tiles32", "tiles33", "wrap")]
            + [(64, 0, e, ("f32", "bf16")) for e in ("rows64", "rows65", "wrap")]
            + [(64, 2, e, ("f32", "bf16")) for e in ("tiles32", "tiles33", "wrap")]
            + [(64, 1, "tiles33", ("f32", "bf16"))]
            + [(128, l, e, ("f32", "bf16")) for l in (0, 3) for e in ("below-sweep", "sweep")]
            + [(64, 2, "tiles33", ("bf16x6",))])


def bn_case_batch(W, layer, edge, bf16, cus=256):
    """The batch of a case: the smallest that meets the edge's predicate, or the largest below it."""
    pred = BN_EDGES[BN_BELOW.get(edge, edge)]
    B = next(b for b in range(1, 1 << 14) if pred(bn_facts(W, layer, b, bf16, cus)))
    return B - 1 if edge in BN_BELOW else B


def bn_assert_edge(W, layer, edge, B, bf16, cus):
    """The case still sits on the edge it is named for, on this device's compute-unit count."""
    f = bn_facts(W, layer, B, bf16, cus)
    if edge in BN_BELOW:
        ok = not BN_EDGES[BN_BELOW[edge]](f) and BN_EDGES[BN_BELOW[edge]](bn_facts(W, layer, B + 1, bf16, cus))
    else:
        ok = BN_EDGES[edge](f)
    assert ok, f"{W} x {W}, block {layer}, B = {B}: not on the edge '{edge}' with {cus} compute units: {f}"
    return f


def _rows_chain(R, finalize):
    """Additions a workgroup's partial row passes through on its way to the channel sum.  finalize: launch_col_reduce_partial
    (rows_sum_kernel above 64 rows: cdiv(rpb, 8) rows per row group, then the 8 LDS rows) and bn_bwd_finalize_kernel (cdiv(R, 16) rows
    per lane, 4 shuffle levels); else launch_col_reduce (rows_sum_1024_kernel for 64 < R <= 2048: cdiv(R, 32) rows per lane, then the 32
    LDS rows; one rows_sum_kernel workgroup up to 64 rows)."""
    if finalize:
        n = 0
        if R > 64:
            rpb = _cdiv(R, 32)
            n, R = _cdiv(rpb, 8) + 8, _cdiv(R, rpb)
        return n + _cdiv(R, 16) + 4
    assert R <= 2048
    return _cdiv(R, 32) + 32 if R > 64 else _cdiv(R, 8) + 8


def bn_bwd_chain(nblk, ppb, C, V, finalize, per_px=1):
    """n of the (n + c) 2^-24 sum |terms| bounds: the longest chain of additions a term of a backward sum passes through in this
    launch.  A thread owns V channels and every NSUB-th pixel of its workgroup's ppb (NSUB = 256 / (C / V)), per_px additions each;
    then the NSUB LDS rows in series; then the rows of reduce.hip (_rows_chain)."""
    nsub = 256 // (C // V)
    return _cdiv(ppb, nsub) * per_px + nsub + _rows_chain(nblk, finalize)


def bn_windows(t, B, H, C):
    """(B, H, H, C) -> (B, H/2, H/2, 4, C): the 2x2 windows in the kernels' scan order (0,0) (0,1) (1,0) (1,1)."""
    return t.reshape(B, H // 2, 2, H // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, H // 2, 4, C)


def bn_gen_y(gen, layer, W, B, bf16, device="cpu"):
    """y (B, H, H, C) fp32 whose four values in every pooling window differ by at least 2^-6, per channel: 2^-6 times (a per-window
    integer offset + a random permutation of {0, 2, 4, 6} + a per-channel shift), |y| < 2, so every value has at most 8 significant
    bits (bf16-representable); fp32 storage adds a jitter in [0, 2^-6) below that, which keeps neighbours 2^-6 apart."""
    C, H = bn_layer(layer, W)
    HO = H // 2
    off = torch.randint(-90, 85, (B, HO, HO, 1, C), generator=gen, device=device)
    perm = torch.rand((B, HO, HO, 4, C), generator=gen, device=device).argsort(dim=3) * 2
    shift = torch.randint(-20, 21, (C,), generator=gen, device=device)
    k = (off + perm + shift).float()
    if not bf16:
        k = k + torch.rand(k.shape, generator=gen, device=device)
    k = k / 64.0
    return k.reshape(B, HO, HO, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, H, C).contiguous()


def bn_gen_params(gen, C, device="cpu"):
    """gamma with |gamma| in [0.5, 1.5], every third channel negative; beta in [-0.5, 0.5]; running_mean in [-0.3, 0.3], running_var
    in [0.5, 1.5]."""
    u = lambda lo, hi: torch.rand(C, generator=gen, device=device) * (hi - lo) + lo      # noqa: E731
    gamma = u(0.5, 1.5)
    gamma[::3] *= -1
    return gamma, u(-0.5, 0.5), u(-0.3, 0.3), u(0.5, 1.5)


def synth_bn_partials(y, layer, B, n_floats=None):
    """The conv epilogue's BatchNorm partials, built from the stored y (B, H, H, C) widened to float64: row t holds the sum of
    ni * pxPerImg pixels of images img0 .. img0 + ni - 1, img0 = (t // tilesPerImg) * imgsPerTile (the images' pixels in storage
    order, cut into tilesPerImg equal runs: any partition with those counts is valid, the Chan merge only needs the counts), row
    numTiles + t their M2 about that row's own mean; each rounded once to fp32.  Returns the fp32 buffer (n_floats long, default
    2 numTiles C; whatever lies behind the rows holds ALL_ONES) and the float64 (sum, M2, count) per row."""
    C, H = y.shape[3], y.shape[1]
    imgs, ppi, tpi = bn_part_geom(layer, H)
    nt = bn_num_tiles(layer, H, B)
    y64 = y.double().reshape(B, H * H, C)
    sums, m2s, cnt = [], [], []
    full = B // imgs
    for i0, groups, ni in ((0, full, imgs), (full * imgs, 1 if B % imgs else 0, B % imgs)):
        if groups == 0:
            continue
        v = y64[i0:i0 + groups * ni].reshape(groups, ni, tpi, ppi, C).permute(0, 2, 1, 3, 4).reshape(groups * tpi, ni * ppi, C)
        s = v.sum(1)
        sums.append(s)
        m2s.append(((v - (s / (ni * ppi))[:, None]) ** 2).sum(1))
        cnt.append(torch.full((groups * tpi,), float(ni * ppi), dtype=torch.float64, device=y.device))
    s, m2, cnt = torch.cat(sums).float(), torch.cat(m2s).float(), torch.cat(cnt)
    assert s.shape == (nt, C)
    n_floats = 2 * nt * C if n_floats is None else n_floats
    part = torch.empty(n_floats, device=y.device)
    if y.is_cuda:
        poison(part, ALL_ONES)
    else:
        part.view(torch.int32).fill_(-1)
    part[:nt * C] = s.reshape(-1)
    part[nt * C:2 * nt * C] = m2.reshape(-1)
    return part, s.double(), m2.double(), cnt


def bn_stats_ref(y, s, m2, cnt):
    """float64 batch statistics of the stored y and the bounds the fp32 roundings of the partials allow (the merge itself runs in fp64:
    2^-45 of the summed terms covers it).  mean: each s_t carries U32 |s_t|, the cast U32 |mu|.  var = (sum m_t + sum s_t^2 / n_t - S^2 / N)
    / N: d var / d s_t = 2 (s_t / n_t - mu) / N, m_t carries U32 m_t, the cast U32 var.  Returns mean, var, mean bound, var bound."""
    N = cnt.sum()
    y64 = y.double().reshape(-1, y.shape[-1])
    mu, var = y64.mean(0), y64.var(0, unbiased=False)
    sa, n_t = s.abs().sum(0), cnt[:, None]
    mb = U32 * (sa / N + mu.abs()) + 2.0 ** -45 * sa / N
    vb = (U32 * (m2.sum(0) + (2 * (s / n_t - mu).abs() * s.abs()).sum(0)) / N + U32 * var
          + 2.0 ** -45 * (m2.sum(0) + (s * s / n_t).sum(0)) / N)
    return mu, var, mb, vb


def bn_first_max(nw):
    """Position of the first maximum along dim 3 (the kernels' and ATen's tie rule), whatever torch.argmax does with ties."""
    top = nw.max(dim=3, keepdim=True).values
    rank = torch.tensor([4, 3, 2, 1], device=nw.device).view(1, 1, 1, 4, 1)
    return ((nw == top) * rank).argmax(dim=3, keepdim=True)


def bn_fwd_ref(yw, coef, tanh, bf16):
    """float64 a = act(max over the window of y scale + shift) from the coefficients the kernel returned, and its bound: one fma
    rounding of |n| (the largest of the window), TANH_ULPS ulps of tanhf (Tanh block), one bf16 rounding of the result (bf16 storage),
    and the rounding of this float64 evaluation itself (the fma can sit on its bound exactly).
    yw (B, HO, HO, 4, C) float64, coef (C, 4) float64.  Returns a, bound, n (the window's normalised values), first-max position."""
    nw = yw * coef[:, 0] + coef[:, 1]
    pos = bn_first_max(nw)
    top = nw.gather(3, pos)[:, :, :, 0]
    want = torch.tanh(top) if tanh else top.clamp_min(0.0)
    b = U32 * nw.abs().max(dim=3).values + (2 * TANH_ULPS * U32 * want.abs() if tanh else 0.0)
    b = b + 2.0 ** -50 * ((yw * coef[:, 0]).abs() + coef[:, 1].abs()).max(dim=3).values      # the float64 reference's own rounding
    if bf16:
        b = BF16 * want.abs() + (1 + BF16) * b
    return want, b, nw, pos


# ---- MS-SSIM / KLD / scores (msssim.hip, msssim_finish.h, score.hip): launch geometry, replica inputs and float64 references ----
MS_LDS = 160 * 1024               # LDS of a compute unit (msssim.hip: byLds = 160 KiB / (SMEM + 256))
MS_BASES = 5                      # base pairs of a replica batch: image i is base[i % MS_BASES]
# recon = a x + (1 - a) u per base pair, u uniform on [0, MS_NOISE_TOP).  With u on [0, 1) every pair has the brightness of its x, and the
# levels of 8 and 4 pixels, where the zero padding and C2 outweigh the image, are 1 - 1e-5 for EVERY a: a plane taken from the neighbouring
# image moves no level mean by even one fp32 ulp at the large batches (tests/test_host_msssim_tools.py, condition (c)).  A dim u makes the
# brightness ratio a + MS_NOISE_TOP (1 - a) differ per pair; a spread over [0.1, 0.9] in steps of 0.2, ordered so that neighbours in the
# batch (k, k + 1 mod 5) are two steps apart, then moves some mean of every level by 11 ulps or more at B = 5462.
MS_ALPHAS = (0.9, 0.5, 0.1, 0.7, 0.3)
MS_NOISE_TOP = 0.1
MS_CONFIG_BATCH = {64: 2048, 128: 1024}    # the bf16 configs' batches
EXPF_ULPS = 3                     # expf of the device library: the OpenCL bound it is built to; an fp32 ulp is at most 2 U32 |v|


def ms_plane_geom(S):
    """MsP<S> of msssim.hip: the whole-plane kernel's threads per plane, planes per workgroup and LDS bytes."""
    NTP = S * S // 4
    PPW = 1 if NTP >= 256 else 256 // NTP
    DAS, DCS, TAS, TR = S + 14, S + 12, S + 2, S + 10
    LIN = S * (2 * DAS + DCS)
    TA = 2 * TR * TAS
    TMP = 2 * TA + TR * S
    return dict(NTP=NTP, PPW=PPW, NT=NTP * PPW, LIN=LIN, TA=TA, TMP=TMP, SMEM=PPW * (LIN + TMP) * 4)


def ms_resident_groups(S, cus):
    """Workgroups of msssim_plane_kernel<S> in one residency of the chip: ms_fwd's grid cap."""
    g = ms_plane_geom(S)
    return cus * min(MS_LDS // (g["SMEM"] + 256), 2048 // g["NT"])


def ms_level_facts(W, B, cus=256):
    """Per pyramid level of a batch of B frames W wide: the kernel, plane groups, grid and the trips of the busiest (and idlest)
    workgroup.  128-wide level 0 is msssim_stream_kernel: one plane per group, one workgroup per compute unit."""
    P, out = 3 * B, []
    for l in range(5):
        S = W >> l
        if S == 128:
            ppw, resident, kernel = 1, cus, "stream"
        else:
            ppw, resident, kernel = ms_plane_geom(S)["PPW"], ms_resident_groups(S, cus), "plane"
        groups = _cdiv(P, ppw)
        grid = min(groups, resident)
        out.append(dict(level=l, S=S, kernel=kernel, PPW=ppw, P=P, groups=groups, resident=resident, grid=grid,
                        trips=_cdiv(groups, grid), min_trips=groups // grid, last_group=P - (groups - 1) * ppw))
    return out


# edges: "below" = the largest batch whose level still runs one group per workgroup, "loops" = the first batch at which a workgroup
# walks a second group; "config" = the bf16 configs' batch (MS_CONFIG_BATCH), level = the deepest level that loops there
MS_EDGES = ("below", "loops", "config")
MS_CASES = ([(64, l, e) for l in range(5) for e in ("below", "loops")] + [(64, 3, "config")]
            + [(128, l, e) for l in range(1, 5) for e in ("below", "loops")] + [(128, 3, "config")])
MS_RAGGED = (1, 21, 22, 43, 64)   # P = 3, 63, 66, 129, 192: one short of a 64-group, two over, one plane in the last group at 4 / 16 / 64, all full


def ms_case_batch(W, level, edge, cus=256):
    """The batch of a case, from this device's compute-unit count."""
    assert edge in MS_EDGES, edge
    if edge == "config":
        return MS_CONFIG_BATCH[W]
    B = next(b for b in range(1, 1 << 15) if ms_level_facts(W, b, cus)[level]["trips"] > 1)
    return B - 1 if edge == "below" else B


def ms_assert_edge(W, level, edge, B, cus):
    """The case still sits on the edge it is named for, on this device's compute-unit count.  Returns ms_level_facts."""
    f = ms_level_facts(W, B, cus)
    if edge == "below":
        ok = f[level]["trips"] == 1 and ms_level_facts(W, B + 1, cus)[level]["trips"] == 2
    elif edge == "loops":
        ok = f[level]["trips"] == 2 and ms_level_facts(W, B - 1, cus)[level]["trips"] == 1
    else:               # four levels loop, `level` is the deepest of them and its workgroups end unevenly
        looping = [x["level"] for x in f if x["trips"] > 1]
        ok = looping == [0, 1, 2, 3] and level == 3 and f[level]["groups"] % f[level]["grid"] != 0 and f[level]["min_trips"] < f[level]["trips"]
    if W == 128 and level == 1 and edge != "config":      # the stream kernel's edge is the 64-wide plane kernel's
        ok = ok and f[0]["trips"] == f[1]["trips"] and f[0]["kernel"] == "stream"
    assert ok, f"{W} wide, level {level}, B = {B}: not on the edge '{edge}' with {cus} compute units: {f}"
    return f


def ms_counts(B, n=MS_BASES):
    """Occurrences of each base image in a replica batch of B (image i is base i % n), float64."""
    return torch.tensor([(B - k + n - 1) // n for k in range(n)], dtype=torch.float64)


def ms_base_pairs(W, seed=0):
    """MS_BASES base pairs built the way test_gpu_objective.smooth_case builds a batch, recon = a x + (1 - a) u with a = MS_ALPHAS[k]
    (u dimmer than x, see MS_ALPHAS), and a latent per base image: x, mu, logvar, recon as CPU fp32 tensors."""
    g = torch.Generator().manual_seed(77000 + 10 * W + seed)
    x = torch.rand(MS_BASES, 3, W, W, generator=g)
    u = torch.rand(MS_BASES, 3, W, W, generator=g) * MS_NOISE_TOP
    a = torch.tensor(MS_ALPHAS).view(-1, 1, 1, 1)
    recon = (a * x + (1 - a) * u).contiguous()
    mu = torch.randn(MS_BASES, 32, generator=g) * 0.5
    logvar = torch.randn(MS_BASES, 32, generator=g) * 0.3
    return x, mu, logvar, recon


def ms_inputs(tag, W, B):
    """The "pos" / "neg" / "nan" pairs of test_gpu_ops._ms_inputs at any shape (img1, img2), and "unused": a pair whose ssim means of the
    fine levels are negative while every cs mean and ssim_4 stay positive (only levels the product never uses are negative)."""
    from critic_vae_amd import synth
    b = torch.from_numpy(synth.uniform(5, f"ms/{tag}/b", (B, 3, W, W)))
    if tag == "unused":               # left half flipped (bright, anti-correlated: cs < 0 where lum = 1), right half centred (cs = 1 where lum = 0)
        a = torch.cat((1 - b[..., :W // 2], b[..., W // 2:] - 0.5), dim=-1)
        return a.clone(), b
    if tag == "nan":
        a = 0.5 - b + 0.01 * torch.from_numpy(synth.uniform(5, f"ms/{tag}/a", (B, 3, W, W)))
    else:
        a = torch.from_numpy(synth.uniform(5, f"ms/{tag}/a", (B, 3, W, W), -1.0 if tag == "neg" else 0.0, 1.0))
    return a.clone(), b


def ms_oracle64(img1, img2):
    """oracle.cvae_oracle.msssim in float64: its level function and window on double tensors.  Returns (loss, ssim[5], cs[5])."""
    import torch.nn.functional as F
    from oracle import cvae_oracle as orc
    window = orc.ms_window_2d(img1.shape[1]).double()
    w = torch.tensor(orc.MS_WEIGHTS, dtype=torch.float32).double()
    a, b, sims, css = img1.double(), img2.double(), [], []
    for _ in range(5):
        s, c = orc.ssim_level(a, b, window)
        sims.append(s)
        css.append(c)
        a, b = F.avg_pool2d(a, (2, 2)), F.avg_pool2d(b, (2, 2))
    sims, css = torch.stack(sims), torch.stack(css)
    return 1 - torch.prod((css ** w)[:-1] * (sims ** w)[-1]), sims, css


def ms_plane_means64(img1, img2):
    """The oracle's five levels restated per plane, float64: (ssim, cs), each (N, 3, 5) = the mean of the level's map over one plane."""
    import torch.nn.functional as F
    from oracle import cvae_oracle as orc
    a, b = img1.double(), img2.double()
    c = a.shape[1]
    window = orc.ms_window_2d(c).double()
    conv = lambda t: F.conv2d(t, window, padding=orc.MS_WINDOW // 2, groups=c)      # noqa: E731
    ps, pc = [], []
    for _ in range(5):
        mu1, mu2 = conv(a), conv(b)
        s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
        v1, v2 = 2.0 * s12 + orc.C2, s1 + s2 + orc.C2
        pc.append((v1 / v2).mean(dim=(2, 3)))
        ps.append((((2 * mu1 * mu2 + orc.C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + orc.C1) * v2)).mean(dim=(2, 3)))
        a, b = F.avg_pool2d(a, (2, 2)), F.avg_pool2d(b, (2, 2))
    return torch.stack(ps, 2), torch.stack(pc, 2)


def ms_loss_from_means(sims, css):
    """1 - prod_{l<4}(cs_l^w_l * ssim_4^w_4): the oracle's product, on float64 batch means."""
    from oracle import cvae_oracle as orc
    w = torch.tensor(orc.MS_WEIGHTS, dtype=torch.float32).double()
    return 1 - torch.prod((css ** w)[:-1] * (sims ** w)[-1])


def ms_replica_ref(recon, x, counts=None):
    """float64 MS-SSIM loss of the batch in which pair k = (recon[k], x[k]) occurs counts[k] times (default: once each): the batch mean
    of level l is sum_k n_k m[k, l] / B with m the per-image level means.  Returns loss, ssim[5], cs[5] (batch means), grad (the gradient
    of ONE occurrence of each pair w.r.t. its recon: autograd's gradient of the base image divided by n_k; zero rows where n_k = 0),
    plane_ssim / plane_cs (N, 3, 5)."""
    n = torch.ones(recon.shape[0], dtype=torch.float64) if counts is None else counts.double()
    r = recon.double().clone().requires_grad_(True)
    ps, pc = ms_plane_means64(r, x)
    B = n.sum()
    sims = (n[:, None] * ps.mean(1)).sum(0) / B
    css = (n[:, None] * pc.mean(1)).sum(0) / B
    loss = ms_loss_from_means(sims, css)
    loss.backward()
    grad = r.grad / n.clamp_min(1.0).view(-1, 1, 1, 1)
    return dict(loss=loss.detach(), ssim=sims.detach(), cs=css.detach(), grad=grad, plane_ssim=ps.detach(), plane_cs=pc.detach())


def f32_ulp(v):
    """The spacing of fp32 at |v| (float64 tensor), at least the smallest normal's."""
    v = torch.as_tensor(v, dtype=torch.float64).abs().clamp_min(2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(v)) - 23)


def ms_swap_shift(ref, counts):
    """Condition (c) of the replica inputs: at the batch with these counts, compute ONE plane of an occurrence of base image k from the
    same plane of image k + 1 (its neighbour in the batch) at level l.  Returns (MS_BASES, 3, 5): the larger of the two shifts of that
    level's batch means (ssim, cs) in fp32 ulps of the mean."""
    B3 = 3.0 * counts.sum()
    out = []
    for p, m in ((ref["plane_ssim"], ref["ssim"]), (ref["plane_cs"], ref["cs"])):
        out.append(((torch.roll(p, -1, 0) - p).abs() / B3) / f32_ulp(m))
    return torch.maximum(out[0], out[1])


# ---- KLD (msssim_finalize_kernel): inputs, float64 reference and the bounds of the kernel's fp32 arithmetic ----
KW32 = 0.0010000000474974513      # MS_REF_KW = 0.001f as the kernel holds it


def kld_case(B, seed=0):
    """mu ~ 0.5 N(0, 1), logvar ~ U(-1, 1), every image distinct: CPU fp32 (B, 32)."""
    g = torch.Generator().manual_seed(88000 + 7 * B + seed)
    return torch.randn(B, 32, generator=g) * 0.5, torch.rand(B, 32, generator=g) * 2 - 1


def kld_ref(mu, logvar, kw=KW32):
    """float64 weighted KLD, d_mu, d_logvar and what the kernel's arithmetic may be off by (tests/test_gpu_msssim_ops.py, (f)).
      term   t = 1.0f + lv - m * m - e, e = expf(lv): the sum 1 + lv, the product (none if contracted), the difference, expf's
             EXPF_ULPS ulps (<= 2 U32 e each), the last difference: U32 (|1 + lv| + m^2 + |1 + lv - m^2| + |t|) + 2 EXPF_ULPS U32 e
      KLD    (float)(-0.5 k / B) * kw on the fp64 sum k of the fp32 terms: the terms' errors, 2^-45 of sum |t| for the fp64
             additions in any order, then the cast and the product: 2 U32 |KLD|
      d_mu   kw * m * (1.0f / (float)B): the reciprocal, two products: 3 U32 |d_mu|
      d_lv   kw * 0.5f * (e - 1.0f) * (1.0f / (float)B): expf's error enters e - 1 in full (the cancellation near lv = 0), then the
             difference, the reciprocal and two products (kw * 0.5f is exact): kw / (2 B) 2 EXPF_ULPS U32 e + 4 U32 |d_lv|
    Returns a dict; `terms` (B,) is each image's float64 sum of its 32 terms."""
    m, lv = mu.double(), logvar.double()
    B = m.shape[0]
    e = lv.exp()
    t = 1 + lv - m * m - e
    kld = kw * -0.5 * t.sum() / B
    t_err = U32 * ((1 + lv).abs() + m * m + (1 + lv - m * m).abs() + t.abs()) + 2 * EXPF_ULPS * U32 * e
    kld_b = 0.5 * kw / B * (t_err.sum() + 2.0 ** -45 * t.abs().sum()) + 2 * U32 * kld.abs()
    d_mu, d_lv = kw * m / B, kw * 0.5 * (e - 1) / B
    slack = 1 + 2.0 ** -20            # second-order terms of the products of roundings
    return dict(kld=kld, kld_bound=kld_b * slack, d_mu=d_mu, d_mu_bound=3 * U32 * d_mu.abs() * slack + 2.0 ** -149,
                d_logvar=d_lv, d_logvar_bound=(0.5 * kw / B * 2 * EXPF_ULPS * U32 * e + 4 * U32 * d_lv.abs()) * slack + 2.0 ** -149,
                terms=t.sum(1))
