"""BatchNorm / pool / activation (bn.hip) and the column sums it ends in (reduce.hip), op by op, at every chunk, block and sweep edge.

cvae_op_bn_pool_act_fwd runs bn_fwd_reduce (numTiles partials in at most 32 chunks, eight row groups per chunk), bn_fwd_finalize and
bn_pool_act_fwd (a grid-stride sweep of 16 workgroups per compute unit); cvae_op_bn_pool_act_bwd runs the statistics pass
(bn_bwd_stats_relu_kernel or bn_bwd_kernel<.., 1, 0>, nblk <= 1024 workgroups of ppb pooled pixels), launch_col_reduce_partial (through
rows_sum_kernel above 64 rows), bn_bwd_finalize, the apply pass and launch_col_reduce (rows_sum_1024_kernel above 64 rows).  The cases
(ws_tools.BN_CASES) sit on both sides of each of those edges; their batches are derived from the launchers' rules and this device's
compute-unit count (ws_tools.bn_case_batch), and every test asserts first that its batch is on the edge it is named for.

The partials are built by the test (ws_tools.synth_bn_partials) from the stored y in float64, rounded once: the statistics are then
checked independently of the conv kernels, and a bf16-storage handle's train-mode forward of blocks 1..3 can be driven at all.

(a) parity against float64, U = 2^-24.  y: the four values of every window at least 2^-6 apart, so that the float64 argmax is the
    kernel's; |gamma| in [0.5, 1.5], every third negative; bf16 storage: y, da and the stored a are bf16 values.
      mean           U (sum_t |s_t| / N + |mu|): one rounding per partial sum (the test's own), the final cast; the merge is fp64
      invstd         (var_bound / (2 (var + eps)) + 4 U) invstd: var = (sum m_t + sum s_t^2 / n_t - S^2 / N) / N carries
                     U (sum m_t + sum 2 |s_t / n_t - mu| |s_t|) / N + U var; then the sum var + eps, sqrtf, the quotient
      scale, shift   scale = gamma * invstd bit for bit; shift = beta - mean * scale to 2 U (|beta| + |mean scale|)
      running_mean   0.9f * rm + 0.1f * mean in fp32 on the host, bit for bit (two roundings, no fma), from rm in [-0.3, 0.3]
      running_var    0.1 N / (N - 1) var_bound + 3 U (0.9 |rv| + 0.1 uvar): the constants, the two products, the sum; N = 64 included
      a              against act(max(y scale + shift)) from the RETURNED coef: U max |n| over the window (one fma rounding), tanhf
                     TANH_ULPS = 5 ulps (the OpenCL bound the device library is built to; the worst case over the fp32 cases is printed
                     as "tanhf ulps", against float64 tanh of the fp32 argument: 1.38 on an MI355X), bf16 storage 2^-8 |want| more
      ReLU gate      the backward reference takes a > 0 from the kernel's a; it may differ from float64 only where |n| is within a's bound
      dbeta, dgamma  (n + c) U sum |terms| against float64 sum g, sum g xhat (g from the kernel's a, xhat = (y_argmax - mean) invstd from the
                     returned coef): n = ws_tools.bn_bwd_chain (pixels per thread, NSUB LDS rows, rows per lane and the trees of reduce.hip),
                     c = 3 for the product g xhat with xhat's two roundings.  Tanh: g = da (1 - a a) carries 3 U |da| per term.  ReLU channels
                     on the pooled-tensor shortcut xhat = (a - beta)(1 / gamma): per term XS_ULPS = 8 U (|a| + |beta| + |mean scale|) / |gamma|
                     (a's fma rounding, beta rebuilt from shift + mean scale, the difference, gamma rebuilt as scale / invstd and inverted, the
                     product), and on bf16 storage 2^-8 |a| / |gamma| from the stored a
      dy             against scale (g [p = argmax] - k1 - xhat k2), k1 / k2 = fp32 dbeta / dgamma (as returned) * (1.0f / (float)N):
                     DY_ULPS = 6 U |scale| (|da| [p = argmax] + |k1| + |xhat k2|), bf16 storage 2^-8 |want| more
      dbias          against the float64 sum of the reference dy (0 up to the roundings of k1, k2): n U sum |dy| + sum of dy's own bounds,
                     n = bn_bwd_chain of the apply pass (four additions per pixel) through launch_col_reduce
(b) exact counts: all-ones da with every gate open (ReLU: beta = 8, gamma = 1; Tanh: constant y, beta = 0: xhat = n = a = 0) gives
    dbeta = totalPx exactly in any summation order; one lit pooled pixel (first / last of block 0, first of block 1, first / last of the
    last live block, a pixel of block 911 at B = 513) gives dbeta = 1 exactly, and on the Tanh setup dy = scale * ([first element of that
    window] - k1) bit for bit.
(c) the tiny-gamma switch: gamma in {0, +-1e-2 (1 +- 2^-10), 3e-3, -5e-3}: dgamma inside the bound of the path the kernel takes (the
    larger of the two within 2^-9 of the threshold).
(d) eval mode: coef from the running statistics (invstd 4 U, shift 2 U (|beta| + |mean scale|)), which stay bit for bit; a as in (a).
(e) hygiene on every call: PAD images of NaN behind every input, 128 NaN rows behind the partials, a sentinel behind every output and
    the scratch, the scratch itself NaN on entry; no NaN comes out, no sentinel is touched, and the same call twice gives the same bits.

The measured head-room of every bound is in LABNOTES.md."""
import zlib

import pytest
import torch

from critic_vae_amd import lib as cvlib
from ws_tools import (ALL_ONES, BF16, BN_CASES, DY_ULPS, U32, XS_ULPS, bn_assert_edge, bn_bwd_chain, bn_case_batch, bn_fwd_ref,
                      bn_gen_params, bn_gen_y, bn_layer, bn_num_tiles, bn_stats_ref, bn_width, bn_windows, poison, same_bits,
                      synth_bn_partials, within)

pytestmark = pytest.mark.gpu

PAD = 2                      # images past B in every batch-indexed buffer: the largest image count of a partial tile
TAIL = 256                   # floats behind the per-channel outputs and the scratch
SENTINEL = 0xDEADBEEF        # finite as fp32 and as each bf16 half
EPS = 1e-5
DEV = "cuda"              # where the inputs are generated and the float64 references run
CASES = [(W, layer, edge, m) for W, layer, edge, modes in BN_CASES for m in modes]
cases = pytest.mark.parametrize("W,layer,edge,mode", CASES, ids=[f"w{w}-l{l}-{e}-{m}" for w, l, e, m in CASES])
WORST = {}                   # (output, mode) -> largest err / bound seen, printed per module (pytest -s) for LABNOTES
TINY = {}                    # (c): per (layer, mode, gamma) the measured dgamma error, its bound, the path and dgamma itself


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def handles():
    """One handle per (width, precision) for the whole module, max_batch = the largest batch the module runs on it."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(W, mode):
        if (W, mode) not in made:
            top = max(bn_case_batch(w, l, e, m == "bf16", cus()) for w, l, e, m in CASES if (w, m) == (W, mode))
            made[W, mode] = cvlib.Handle(W, top, precision=mode)
        return made[W, mode]
    yield get
    made.clear()
    for (tag, mode), r in sorted(WORST.items()):
        print(f"worst err / bound  {tag:14s} {mode:7s} {r:.3f}")
    for (layer, mode, gam), (err, bound, path, want) in sorted(TINY.items()):
        print(f"tiny gamma  block {layer} {mode:5s} gamma {gam:+.7e} ({path}): dgamma {want:+.3e} err {err:.3e} bound {bound:.3e}")


def gen(*key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def bounded(tag, mode, got, want, bound):
    r = within(tag, got, want, bound)
    WORST[tag, mode] = max(WORST.get((tag, mode), 0.0), r)
    print(f"{tag} [{mode}]: err / bound {r:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# buffers (e): padding inside the same allocation, always
# ---------------------------------------------------------------------------------------------------------------------------------------
def _i32(pattern):
    return pattern - (1 << 32) if pattern >= 1 << 31 else pattern


def imgs_in(t, bf):
    """(B, ...) device fp32 values -> buffer of B + PAD images, the padding NaN, in bf16 storage if asked (the values are bf16 already)."""
    full = torch.full((t.shape[0] + PAD,) + tuple(t.shape[1:]), float("nan"), dtype=torch.bfloat16 if bf else torch.float32, device=DEV)
    full[:t.shape[0]] = t
    return full


def imgs_out(B, shape, bf):
    return poison(torch.empty((B + PAD,) + tuple(shape), dtype=torch.bfloat16 if bf else torch.float32, device=DEV), SENTINEL)


def flat_out(n):
    return poison(torch.empty(n + TAIL, device=DEV), SENTINEL)


def flat_io(t):
    """A per-channel in / out tensor (running statistics) with the sentinel tail."""
    b = flat_out(t.numel())
    b[:t.numel()] = t
    return b


def scratch_for(H, B):
    n = H.op_scratch_floats(B)
    s = torch.empty(n + TAIL, device=DEV)
    poison(s[:n], ALL_ONES)
    poison(s[n:], SENTINEL)
    return s, n


def arg(t):
    return t if t.dtype == torch.float32 else t.reshape(-1).view(torch.float32)


def take(name, buf, n):
    """The first n images (floats) of an output, still on the device, after the checks of (e)."""
    tail = buf[n:].reshape(-1)
    words = tail.view(torch.int32) if tail.dtype == torch.float32 else tail.view(torch.int16).view(torch.int32)
    bad = int((words != _i32(SENTINEL)).sum())
    assert bad == 0, f"{name}: {bad} words of the padding behind the output were overwritten"
    got = buf[:n]
    nan = int(torch.isnan(got).sum())
    assert nan == 0, f"{name}: {nan} NaN in the output: NaN padding or scratch that was never written has been read"
    return got


def twice(call):
    """(e): run the call twice on fresh buffers; the outputs must agree bit for bit.  Returns the first."""
    first, second = call(), call()
    for k in first:
        assert same_bits(first[k], second[k]), f"{k} differs between two identical calls"
    return first


def run_fwd(H, layer, B, y, part, gamma, beta, rm, rv, train=True):
    """y (B, H, H, C) fp32 values on the device.  Returns coef (C, 4), a (B, HO, HO, C) as stored, running statistics after."""
    bf = H.precision == "bf16"
    C, h = y.shape[3], y.shape[1]
    ybuf = imgs_in(y, bf)

    def call():
        coef, a = flat_out(4 * C), imgs_out(B, (h // 2, h // 2, C), bf)
        rmb, rvb = flat_io(rm), flat_io(rv)
        s, n = scratch_for(H, B)
        H.op_bn_pool_act_fwd(layer, B, arg(ybuf), part, gamma, beta, rmb, rvb, coef, arg(a), s, train)
        torch.cuda.synchronize()
        assert int((s[n:].view(torch.int32) != _i32(SENTINEL)).sum()) == 0, "bn forward: words behind the scratch were overwritten"
        return {"coef": take("coef", coef, 4 * C).view(C, 4), "a": take("a", a, B), "rm": take("running_mean", rmb, C),
                "rv": take("running_var", rvb, C)}
    return twice(call)


def run_bwd(H, layer, B, y, a, da, coef, gamma):
    """y, a (as stored by the forward), da: (B, ., ., C) on the device.  Returns dy as stored, dgamma, dbeta, dbias."""
    bf = H.precision == "bf16"
    C, h = y.shape[3], y.shape[1]
    ybuf, abuf, dabuf = imgs_in(y, bf), imgs_in(a, bf), imgs_in(da, bf)
    cbuf = coef.contiguous().reshape(-1)

    def call():
        dy = imgs_out(B, (h, h, C), bf)
        dg, db, dbias = flat_out(C), flat_out(C), flat_out(C)
        s, n = scratch_for(H, B)
        H.op_bn_pool_act_bwd(layer, B, arg(ybuf), arg(abuf), arg(dabuf), cbuf, gamma, arg(dy), dg, db, dbias, s)
        torch.cuda.synchronize()
        assert int((s[n:].view(torch.int32) != _i32(SENTINEL)).sum()) == 0, "bn backward: words behind the scratch were overwritten"
        return {"dy": take("dy", dy, B), "dgamma": take("dgamma", dg, C), "dbeta": take("dbeta", db, C), "dbias": take("dbias", dbias, C)}
    return twice(call)


def case_setup(handles, W, layer, edge, mode):
    bf = mode == "bf16"
    B = bn_case_batch(W, layer, edge, bf, cus())
    f = bn_assert_edge(W, layer, edge, B, bf, cus())
    if edge == "wrap" and layer == 3:      # past the cap of 1024 workgroups: ppb no longer divides, the last workgroups are empty
        assert f["nblk"] == 1024 and f["live"] < f["nblk"] and f["live"] * f["ppb"] == f["px"], f
    if edge == "tiles33":
        assert f["tpb"] == 2 and f["RA"] < 32, f
    if edge == "n64":
        assert f["last_ni"] < f["imgs"], f
    return handles(W, mode), bf, B, f


def partials_for(H, y, layer, B):
    """The op's partials, op_bn_partial_floats long, with a NaN tail of 128 rows behind them in the same allocation (a chunk that runs
    past numTiles reads it)."""
    C, h = y.shape[3], y.shape[1]
    n = H.op_bn_partial_floats(layer, B)
    assert n == 2 * bn_num_tiles(layer, h, B) * C, "op_bn_partial_floats is not two rows per tile"
    return synth_bn_partials(y, layer, B, n + 128 * C)


def to_bf16(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# float64 references and bounds
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_forward(mode, layer, B, y, part_rows, gamma, beta, rm0, rv0, got, train=True):
    """The statistics (train) or the coefficients from the running statistics (eval), then a.  Returns the forward reference."""
    bf = mode == "bf16"
    C, h = y.shape[3], y.shape[1]
    coef = got["coef"].double()
    g64, b64 = gamma.double(), beta.double()
    if train:
        s, m2, cnt = part_rows
        N = float(B * h * h)
        mu, var, mb, vb = bn_stats_ref(y, s, m2, cnt)
        bounded("mean", mode, coef[:, 2], mu, mb)
        istd = 1.0 / torch.sqrt(var + EPS)
        bounded("invstd", mode, coef[:, 3], istd, istd * (0.5 * vb / (var + EPS) + 4 * U32))
        want_rm = torch.tensor(0.9) * rm0.cpu() + torch.tensor(0.1) * got["coef"][:, 2].cpu()          # fp32: two products, one sum
        assert same_bits(got["rm"].cpu(), want_rm), "running_mean is not 0.9f * rm + 0.1f * mean in fp32, bit for bit"
        uvar = var * N / (N - 1)
        rv = 0.9 * rv0.double() + 0.1 * uvar
        bounded("running_var", mode, got["rv"], rv, 0.1 * N / (N - 1) * vb + 3 * U32 * (0.9 * rv0.double().abs() + 0.1 * uvar))
    else:
        assert same_bits(got["rm"], rm0) and same_bits(got["rv"], rv0), "eval mode changed the running statistics"
        assert same_bits(got["coef"][:, 2].contiguous(), rm0), "eval mode: coef mean is not the running mean"
        istd = 1.0 / torch.sqrt(rv0.double() + EPS)
        bounded("eval invstd", mode, coef[:, 3], istd, 4 * U32 * istd)
    assert same_bits(got["coef"][:, 0].contiguous(), gamma * got["coef"][:, 3]), "scale is not gamma * invstd in fp32"
    ms = coef[:, 2] * coef[:, 0]
    bounded("shift", mode, coef[:, 1], b64 - ms, 2 * U32 * (b64.abs() + ms.abs()))
    yw = bn_windows(y.double(), B, h, C)
    want, bound, nw, pos = bn_fwd_ref(yw, coef, layer == 3, bf)
    a = got["a"].double()
    bounded("a", mode, a, want, bound)
    if layer == 3:               # tanhf alone, in fp32 ulps of the result, against float64 tanh of the correctly rounded argument
        top = nw.gather(3, pos)[:, :, :, 0]
        if not bf:
            t = torch.tanh(top.float().double())
            ulp = 2.0 ** (torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126))) - 23)
            r = ((a - t).abs() / ulp).max().item()
            WORST["tanhf ulps", mode] = max(WORST.get(("tanhf ulps", mode), 0.0), r)
    else:                        # the ReLU gate of the kernel's own a against float64
        top = nw.gather(3, pos)[:, :, :, 0]
        differ = (a > 0) != (top > 0)
        assert not bool((differ & (top.abs() > bound)).any()), "a ReLU gate differs from float64 where |n| is outside a's bound"
        assert int(differ.sum()) <= 1e-3 * differ.numel(), f"{int(differ.sum())} of {differ.numel()} ReLU gates differ from float64"
    return yw, nw, pos


def check_backward(mode, layer, B, f, yw, pos, a, da, coef, gamma, beta, got, tiny_report=None):
    """dbeta, dgamma, dy, dbias against float64 from the kernel's a and coef."""
    bf = mode == "bf16"
    C = yw.shape[4]
    tanh = layer == 3
    coef = coef.double()
    sc, mean, istd = coef[:, 0], coef[:, 2], coef[:, 3]
    a, da = a.double(), da.double()
    g = da * (1 - a * a) if tanh else da * (a > 0)
    ge = 3 * U32 * da.abs() if tanh else torch.zeros_like(g)             # what the fp32 g may be off by
    xw = (yw - mean) * istd
    xm = xw.gather(3, pos)[:, :, :, 0]
    red = (0, 1, 2)
    s1, s2 = g.sum(red), (g * xm).sum(red)
    vs = bn_width(bf, apply=tanh)        # the Tanh statistics run on bn_bwd_kernel<.., 1, 0> (WB); ReLU on bn_bwd_stats_relu_kernel (W)
    n1 = bn_bwd_chain(f["nblk"], f["ppb"], C, vs, True)
    n2 = bn_bwd_chain(f["nblk"], f["ppb"], C, vs, True, per_px=1 if tanh else 2)
    b1 = n1 * U32 * g.abs().sum(red) + ge.sum(red)
    by = (n2 + 3) * U32 * (g * xm).abs().sum(red) + (ge * xm.abs()).sum(red)            # xhat from y at the argmax
    if tanh:
        b2 = by
    else:                                # ReLU: the shortcut unless |gamma| < 1e-2; within 2^-9 of the threshold either
        ga = gamma.double().abs()
        e = (XS_ULPS * U32 * (a.abs() + beta.double().abs() + (mean * sc).abs()) + (BF16 * a.abs() if bf else 0.0)) / ga.clamp_min(1e-30)
        bs = (n1 + 1) * U32 * (g.abs() * (xm.abs() + e)).sum(red) + (g.abs() * e).sum(red)
        near = (ga / 1e-2 - 1).abs() <= 2.0 ** -9
        b2 = torch.where(near, torch.maximum(bs, by), torch.where(ga < 1e-2, by, bs))
        if tiny_report is not None:
            err = (got["dgamma"].double() - s2).abs()
            for c in tiny_report:
                path = "either" if bool(near[c]) else ("y" if float(ga[c]) < 1e-2 else "shortcut")
                TINY[layer, mode, float(gamma[c])] = (float(err[c]), float(b2[c]), path, float(s2[c]))
    bounded("dbeta", mode, got["dbeta"], s1, b1)
    bounded("dgamma", mode, got["dgamma"], s2, b2)
    # dy from the k1, k2 the launcher derives from the sums it returned
    invN = torch.tensor(1.0) / torch.tensor(float(f["N"]))                                # fp32
    k1, k2 = (got["dbeta"].cpu() * invN).to(DEV).double(), (got["dgamma"].cpu() * invN).to(DEV).double()
    sel = torch.zeros_like(xw).scatter_(3, pos, g[:, :, :, None])
    sel_abs = torch.zeros_like(xw).scatter_(3, pos, da.abs()[:, :, :, None])
    want = sc * (sel - k1 - xw * k2)
    b32 = DY_ULPS * U32 * sc.abs() * (sel_abs + k1.abs() + (xw * k2).abs())
    bound = BF16 * want.abs() + (1 + BF16) * b32 if bf else b32
    H = f["H"]
    dyw = bn_windows(got["dy"].double(), B, H, C)
    bounded("dy", mode, dyw, want, bound)
    na = bn_bwd_chain(f["nblk"], f["ppb"], C, bn_width(bf, apply=True), False, per_px=4)
    red4 = (0, 1, 2, 3)
    bounded("dbias", mode, got["dbias"], want.sum(red4), na * U32 * (want.abs() + b32).sum(red4) + b32.sum(red4))


def parity_inputs(W, layer, B, bf, tag="parity"):
    g = gen(tag, W, layer, B, bf)
    C, h = bn_layer(layer, W)
    y = bn_gen_y(g, layer, W, B, bf, DEV)
    gamma, beta, rm, rv = bn_gen_params(g, C, DEV)
    da = torch.rand((B, h // 2, h // 2, C), generator=g, device=DEV) * 2 - 1
    return y, gamma, beta, rm, rv, to_bf16(da) if bf else da


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) parity
# ---------------------------------------------------------------------------------------------------------------------------------------
@cases
def test_parity_against_fp64(handles, W, layer, edge, mode):
    """(a) and (e): train-mode forward from synthesised partials, then the backward from the kernel's own a and coef."""
    H, bf, B, f = case_setup(handles, W, layer, edge, mode)
    y, gamma, beta, rm, rv, da = parity_inputs(W, layer, B, bf)
    part, s, m2, cnt = partials_for(H, y, layer, B)
    fw = run_fwd(H, layer, B, y, part, gamma, beta, rm, rv)
    yw, nw, pos = check_forward(mode, layer, B, y, (s, m2, cnt), gamma, beta, rm, rv, fw)
    del nw
    bw = run_bwd(H, layer, B, y, fw["a"].float(), da, fw["coef"], gamma)
    check_backward(mode, layer, B, f, yw, pos, fw["a"].float(), da, fw["coef"], gamma, beta, bw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) exact counts
# ---------------------------------------------------------------------------------------------------------------------------------------
@cases
def test_exact_counts(handles, W, layer, edge, mode):
    """(b): every pooled pixel counted exactly once: all-ones da, then one lit pixel at the block edges."""
    H, bf, B, f = case_setup(handles, W, layer, edge, mode)
    C, h, px, ppb = f["C"], f["H"], f["px"], f["ppb"]
    tanh = layer == 3
    y, _, _, rm, rv, _ = parity_inputs(W, layer, B, bf)
    if tanh:
        y = torch.full_like(y, 0.5)
    gamma = torch.ones(C, device=DEV)
    beta = torch.full((C,), 0.0 if tanh else 8.0, device=DEV)
    part, _, _, _ = partials_for(H, y, layer, B)
    fw = run_fwd(H, layer, B, y, part, gamma, beta, rm, rv)
    a, coef = fw["a"].float(), fw["coef"]
    if tanh:
        assert not bool(a.any()) and not bool(coef[:, 1].add(0.5 * coef[:, 0]).any()), "constant y: n and a must be exactly 0"
    else:
        assert bool((a > 0).all()), "beta = 8: every ReLU gate must be open"
    ho = h // 2
    da = torch.ones((B, ho, ho, C), device=DEV)
    bw = run_bwd(H, layer, B, y, a, da, coef, gamma)
    assert bool((bw["dbeta"] == float(px)).all()), f"all-ones da: dbeta is not totalPx = {px}: {bw['dbeta'][:8].tolist()}"
    lit = {0, ppb - 1, min(ppb, px - 1), (f["live"] - 1) * ppb, px - 1}
    if f["live"] < f["nblk"]:
        lit.add((f["live"] - 1) * ppb + ppb // 2)
    invN = torch.tensor(1.0) / torch.tensor(float(f["N"]))
    for pp in sorted(lit):
        da = torch.zeros((B, ho, ho, C), device=DEV)
        da.view(px, C)[pp] = 1.0
        bw = run_bwd(H, layer, B, y, a, da, coef, gamma)
        assert bool((bw["dbeta"] == 1.0).all()), f"pooled pixel {pp} lit: dbeta is not 1: {bw['dbeta'][:8].tolist()}"
        if tanh:                 # xhat = 0: dy = scale * ([first element of the lit window] - k1), one rounding each
            assert not bool(bw["dgamma"].any()), f"pooled pixel {pp} lit: dgamma is not 0"
            k1 = (bw["dbeta"].cpu() * invN).to(DEV)
            sel = torch.zeros((B, ho, ho, 4, C), device=DEV)
            sel.view(px, 4, C)[pp, 0] = 1.0
            want = coef[:, 0] * (sel - k1)
            want = want.to(torch.bfloat16) if bf else want
            got = bn_windows(bw["dy"], B, h, C)
            assert same_bits(got.contiguous(), want.contiguous()), f"pooled pixel {pp} lit: dy is not scale * ([window's first element] - k1)"


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) the tiny-gamma switch
# ---------------------------------------------------------------------------------------------------------------------------------------
TINY_GAMMA = {0: 0.0, 1: 1e-2 * (1 + 2.0 ** -10), 2: 1e-2 * (1 - 2.0 ** -10), 3: -1e-2 * (1 + 2.0 ** -10), 4: -1e-2 * (1 - 2.0 ** -10),
              5: 3e-3, 9: -5e-3}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("layer", [0, 1])
def test_tiny_gamma_switch(handles, layer, mode):
    """(c): channels on both sides of |gamma| = 1e-2, beta >= 0.3 there so that ReLU passes them."""
    W, B, bf = 64, 5, mode == "bf16"
    H = handles(W, mode)
    f = bn_assert_edge(W, layer, "tiles33", B, bf, cus())
    y, gamma, beta, rm, rv, da = parity_inputs(W, layer, B, bf, "tiny")
    for c, v in TINY_GAMMA.items():
        gamma[c], beta[c] = v, 0.3 + 0.02 * c
    part, s, m2, cnt = partials_for(H, y, layer, B)
    fw = run_fwd(H, layer, B, y, part, gamma, beta, rm, rv)
    yw, nw, pos = check_forward(mode, layer, B, y, (s, m2, cnt), gamma, beta, rm, rv, fw)
    a = fw["a"].float()
    assert bool((a[..., list(TINY_GAMMA)] > 0).all()), "the tiny-gamma channels must pass ReLU"
    bw = run_bwd(H, layer, B, y, a, da, fw["coef"], gamma)
    check_backward(mode, layer, B, f, yw, pos, a, da, fw["coef"], gamma, beta, bw, tiny_report=list(TINY_GAMMA))


# ---------------------------------------------------------------------------------------------------------------------------------------
# (d) eval mode
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("layer", range(4))
def test_eval_mode_forward(handles, layer, mode):
    """(d): train = False, no partials: coef from the running statistics, which stay as they were."""
    W, B, bf = 64, 3, mode == "bf16"
    H = handles(W, mode)
    y, gamma, beta, rm, rv, _ = parity_inputs(W, layer, B, bf, "eval")
    fw = run_fwd(H, layer, B, y, None, gamma, beta, rm, rv, train=False)
    check_forward(mode, layer, B, y, None, gamma, beta, rm, rv, fw, train=False)
