"""E1's weight gradient in the form the training step launches (cvae_op_e1_wgrad_fused), on exact operands.

The step never runs the plain E1 weight-gradient kernel that cvae_op_conv_wgrad(layer 0) and test_gpu_f32_ops.py::test_exact_e1_wgrad
reach: BwdCtx::block_grads(0) launches e1_wgrad_kernel<H, true> (precision 0, 2, 3) or e1_wgrad_bf16_kernel<H, XP> (precision 1), which
apply block 0's BatchNorm / MaxPool / ReLU backward while they stage a tile: first maximum in scan order, the a0 > 0 gate, the (k1, k2)
correction; the bf16 kernel also recomputes y from x, w1 and b1, rounds y and dy to bf16 and never reads y0.  Here they run through their
own entry point, on an "f32" and on a "bf16" handle, the latter from the fp32 frame (XP = false) and from the packed bf16 frame that the
entry's statistics pass writes into scratch (flag bit 0, XP = true).

Operands are e1_fused_tools' cases: every product and every fp32 partial sum is exact in any order, so the float64 reference is what a
correct kernel stores bit for bit, and every comparison on them is torch.equal.  Each case asserts its exactness conditions first.
  route cases   which pixel of a window gets the gradient: ties, negative scales, windows whose maximum is exactly 0; k1 = k2 = 0
  arith cases   the - k1 - xhat k2 correction and, on the bf16 handle, the folded constants and the one bf16 rounding of dy
Batches: f32_ops_tools.BATCHES (64: 1, 3, 5, 9, 37; 128: 1, 3, 5), and per (width, precision) the smallest batch at which a split walks
at least two tiles (the prefetch of the tile loop runs) and the last split is short, from the launchers' own plans at this device's
compute-unit count (one "e1fused-geometry" line each).  Outputs and scratch arrive poisoned (ws_tools.ALL_ONES: NaNs).

test_fused_against_float64_and_the_separate_passes compares the fp32 kernel on real-valued operands with the float64 reference under
the summation bound and with cvae_op_bn_pool_act_bwd(0) + cvae_op_conv_wgrad(0); it prints whether the two forms agree bit for bit and
asserts the bound and, since it was observed on an MI355X, the bit equality (README.md)."""
import functools
import zlib

import pytest
import torch

import e1_fused_tools as E
import f32_ops_tools as F32
from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth
from test_gpu_bf16_ops import assert_equal
from test_gpu_ops import dev, wnat, wref
from ws_tools import (ALL_ONES, U32, _rows_chain, bn_bwd_blocks, bn_gen_params, bn_gen_y, holds, poison, same_bits, synth_bn_partials,
                      within)

pytestmark = pytest.mark.gpu
MAX_B = 256
MODES = ("f32", "bf16")
_handles = {}


def handle(W, mode, max_batch=MAX_B):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    if (W, mode, max_batch) not in _handles:
        _handles[W, mode, max_batch] = cvlib.Handle(W, max_batch, precision=mode)
    return _handles[W, mode, max_batch]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def nan_out(n):
    return poison(torch.empty(n, device="cuda"), ALL_ONES)


def scratch(H, B):
    return nan_out(H.op_scratch_floats(B))


def plan(W, mode, B):
    """(tiles, splits, tiles per split) from the launchers: cvae_op_conv_wgrad_plan(layer 0) on a bf16 handle, _plan_f32 otherwise."""
    return handle(W, "bf16").op_conv_wgrad_plan(0, B) if mode == "bf16" else cvlib.conv_wgrad_plan_f32(W, 0, B, cus())


@functools.lru_cache(maxsize=None)
def uneven(W, mode):
    B = E.uneven_batch(W, mode == "bf16", plan=lambda b: plan(W, mode, b))
    assert B <= MAX_B
    return B


def batch_of(W, mode, b):
    return uneven(W, mode) if b == "uneven" else b


def stored(t, bf):
    """float64 host tensor -> the device buffer of the handle's storage type (bf16 elements packed two per float)."""
    t = t.contiguous().cuda()
    return t.to(torch.bfloat16).reshape(-1).view(torch.float32) if bf else t.float().reshape(-1)


def run(H, c, flags=0, y0="real", layout="separate", x=None):
    """One call on case c.  y0: "real", "nan" (a NaN-filled buffer) or None; layout: "separate" (dw, db), "adjacent" (db = dw + 2432 inside
    one 2496-float buffer) or "no-bias".  Returns (dw [2400], db [32] or None, the whole output buffer), on the device."""
    bf = H.precision == "bf16"
    B, W = c["B"], c["W"]
    per = 2 if bf else 1
    yb = None if y0 is None else stored(c["y"], bf) if y0 == "real" else nan_out(B * W * W * 32 // per)
    w1 = None if c["w1"] is None else wnat(c["w1"].float())
    b1 = None if c["b1"] is None else dev(c["b1"].float())
    buf = nan_out(2496 if layout == "adjacent" else 2432)
    dw = buf[:2400]
    db = buf[2432:2464] if layout == "adjacent" else nan_out(32) if layout == "separate" else None
    H.op_e1_wgrad_fused(B, dev(c["x"].float()) if x is None else x, yb, stored(c["a0"], bf), stored(c["d_a0"], bf), dev(c["coef"].float()),
                        dev(c["bcoef"].float()), w1, b1, dw, db, scratch(H, B), flags)
    torch.cuda.synchronize()
    return dw, db, buf


def check_exact(c, dw, db, tag):
    assert_equal(wref(dw, 3, 32).double(), c["ref_w"], f"dW1, {tag}")
    assert_equal(db.double().cpu(), c["ref_b"], f"db1, {tag}")


def check_case(c, mode, tag):
    """The case on one handle, against its float64 reference; bf16: y0 null and NaN-filled, frame fp32 and packed, all the same bits."""
    E.assert_conditions(c)
    H = handle(c["W"], mode)
    if mode == "f32":
        dw, db, _ = run(H, c)
        return check_exact(c, dw, db, tag)
    dw, db, _ = run(H, c, y0=None)
    check_exact(c, dw, db, f"{tag}, fp32 frame, null y0")
    for flags, y0, what in ((0, "nan", "fp32 frame, NaN y0"), (1, None, "packed frame, null y0"), (1, "nan", "packed frame, NaN y0")):
        dw2, db2, _ = run(H, c, flags, y0)
        check_exact(c, dw2, db2, f"{tag}, {what}")
        assert same_bits(dw2, dw) and same_bits(db2, db), f"{tag}: {what} differs in bits from the fp32 frame with a null y0"


# ---------------------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [64, 128])
def test_uneven_batch_walks_two_tiles_and_ends_short(W, mode):
    """The batch of the "uneven" cases, from the launchers' plans on this device, and the mirror of e1_fused_tools against them."""
    B = uneven(W, mode)
    tiles, S, tps = plan(W, mode, B)
    assert tps >= 2 and tiles % tps != 0, f"{W} x {W}, {mode}, B = {B}: {tiles} tiles on {S} splits of {tps}"
    assert (S - 1) * tps < tiles < S * tps and tiles == B * (W // 4) * (W // 32)
    for b in range(1, B + 1):
        assert plan(W, mode, b) == E.e1_geometry(W, b, mode == "bf16", cus()), (W, mode, b)
        assert b == B or not E.walks_unevenly(plan(W, mode, b))
    assert 4 * B * W * W < E.EXACT_FP32
    print(f"e1fused-geometry w{W} {mode}: B = {B}, {tiles} tiles, {S} splits, {tps} tiles per split, last split {tiles - (S - 1) * tps} ({cus()} CUs)")


# ---------------------------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------------------------
ROUTE = [(W, b, m) for W in (64, 128) for b in F32.BATCHES[W] + ("uneven",) for m in MODES]
ARITH = [(W, b, m) for W in (64, 128) for m in MODES for b in E.ARITH_BATCHES[W, m == "bf16"]]


@pytest.mark.parametrize("W,b,mode", ROUTE, ids=[f"w{w}-b{b}-{m}" for w, b, m in ROUTE])
def test_exact_route(W, b, mode):
    """Ties, negative scales, blocked windows: dW1 and db1 bit for bit."""
    B = batch_of(W, mode, b)
    c = E.route_case(W, B, mode == "bf16")
    assert c["ties"] > 0 and c["tie_changed"] > 0 and c["bound"] < E.EXACT_FP32
    if b == "uneven":
        tiles, S, tps = plan(W, mode, B)
        assert tps >= 2 and tiles % tps != 0
        print(f"e1fused-geometry w{W} {mode} route case: B = {B}, {tiles} tiles, {S} splits, {tps} tiles per split")
    check_case(c, mode, f"route case at {W} x {W}, B = {B}, {mode}")


@pytest.mark.parametrize("W,B,mode", ARITH, ids=[f"w{w}-b{b}-{m}" for w, b, m in ARITH])
def test_exact_arith(W, B, mode):
    """The (k1, k2) correction with every intermediate exact; bf16: dy rounded once to bf16, as the reference rounds it."""
    c = E.arith_case(W, B, mode == "bf16")
    assert mode != "bf16" or c["needs_round"] > 0
    check_case(c, mode, f"arith case at {W} x {W}, B = {B}, {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W", [64, 128])
def test_adjacent_separate_and_null_dbias(W, mode):
    """dbias = dw + 2432 (the flat gradient buffer's layout: one column reduction on the fp32 kernel) leaves the 32 floats between the
    weights and the bias, and the 32 behind the bias, as they were; it gives the bits of the separate buffers; a null dbias leaves dw's."""
    c = E.assert_conditions(E.route_case(W, 3, mode == "bf16"))
    H = handle(W, mode)
    y0 = "real" if mode == "f32" else None
    for flags in ((0,) if mode == "f32" else (0, 1)):
        dw, db, _ = run(H, c, flags, y0)
        check_exact(c, dw, db, f"{mode}, flags {flags}, separate")
        dwa, dba, buf = run(H, c, flags, y0, "adjacent")
        assert bool(holds(buf[2400:2432], ALL_ONES).all()) and bool(holds(buf[2464:], ALL_ONES).all()), "the padding around db1 was written"
        assert same_bits(dwa, dw) and same_bits(dba, db), f"{mode}, flags {flags}: adjacent dbias differs from the separate form"
        dwn, _, buf = run(H, c, flags, y0, "no-bias")
        assert same_bits(dwn, dw) and bool(holds(buf[2400:], ALL_ONES).all()), f"{mode}, flags {flags}: a null dbias changes dw or writes behind it"


def test_packed_and_fp32_frame_agree_on_a_real_frame():
    """bf16 handle, a real-valued frame (synth.make_batch): both forms round the same x to bf16 once, so the bits agree."""
    W, B = 64, 5
    c = E.assert_conditions(E.route_case(W, B, True))
    x = torch.from_numpy(synth.make_batch(21, 0, B, W)[0]).cuda()
    assert int((x.to(torch.bfloat16).float() != x).sum()) > x.numel() // 2, "the frame is not real-valued"
    H = handle(W, "bf16")
    dw0, db0, _ = run(H, c, 0, None, x=x)
    dw1, db1, _ = run(H, c, 1, None, x=x)
    assert bool(torch.isfinite(dw0).all()) and bool(torch.isfinite(db0).all()) and float(dw0.abs().max()) > 0
    assert same_bits(dw0, dw1) and same_bits(db0, db1), "packed and fp32 frame differ"


def test_emulation_handle_runs_the_fp32_kernel():
    c = E.assert_conditions(E.route_case(64, 3, False))
    dw, db, _ = run(handle(64, "f32"), c)
    dw6, db6, _ = run(handle(64, "bf16x6"), c)
    check_exact(c, dw6, db6, "bf16x6 handle")
    assert same_bits(dw, dw6) and same_bits(db, db6)


# ---------------------------------------------------------------------------------------------------------------------------------------
# real-valued operands: float64 under the summation bound, and the separate passes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 128])
def test_fused_against_float64_and_the_separate_passes(W):
    """fp32 handle, the uneven-walk batch, inputs as test_gpu_bn_ops.py generates them (window values 2^-6 apart, every third gamma
    negative); coef, a0 and (k1, k2) are the BatchNorm entry points' own.
    Bound per element: depth 2^-24 sum |x dy|, with sum |x dy| the float64 weight gradient of (|x|, |dy|) and depth the longest chain of
    additions of e1_wgrad_kernel's fixed order: dW1 two products per MFMA and 16 MFMAs per tile (32 tps), one product rounding, three
    additions over the waves; db1 16 tps in the lane, two lane-half exchanges and the three over the waves; each then the rows of
    launch_col_reduce (ws_tools._rows_chain over the splits).
    Measured on an MI355X (256 CUs; depth 144 / 97 at 64 x 64, 146 / 99 at 128 x 128): err / bound 0.0041 (dW1) and 0.0051 (db1) at 64 x 64, B = 34; 0.0041 and 0.0052 at
    128 x 128, B = 10, the same for both forms: the fused form and cvae_op_bn_pool_act_bwd(0) + cvae_op_conv_wgrad(0) were bit-equal in
    dW1 and db1 at both sizes (conv_thin.hip's header comment of the fused staging claims a dy "the same to the bit", and the two kernels
    share one summation order), so the equality is asserted too."""
    H, B, C, HO = handle(W, "f32"), uneven(W, "f32"), 32, W // 2
    tiles, S, tps = plan(W, "f32", B)
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(("e1fused", W, B)).encode()))
    y = bn_gen_y(g, 0, W, B, False, "cuda")
    gamma, beta, rm, rv = bn_gen_params(g, C, "cuda")
    da = torch.rand((B, HO, HO, C), generator=g, device="cuda") * 2 - 1
    x = torch.rand((B, 3, W, W), generator=g, device="cuda")
    coef, a = nan_out(4 * C), nan_out(B * HO * HO * C)
    H.op_bn_pool_act_fwd(0, B, y.reshape(-1), synth_bn_partials(y, 0, B)[0], gamma, beta, rm, rv, coef, a, scratch(H, B), True)
    # the separate passes: (k1, k2) stay in the scratch of the BatchNorm backward, behind its nblk partial rows
    s, dy, junk = scratch(H, B), nan_out(B * W * W * C), nan_out(2 * C)
    H.op_bn_pool_act_bwd(0, B, y.reshape(-1), a, da.reshape(-1), coef, gamma, dy, junk[:C], junk[C:], None, s)
    torch.cuda.synchronize()
    nblk = bn_bwd_blocks(B * HO * HO, C)
    bcoef = s[nblk * 2 * C:nblk * 2 * C + 2 * C].clone()
    assert bool(torch.isfinite(bcoef).all()) and bool(torch.isfinite(dy).all())
    dws, dbs, dwf, dbf = nan_out(2400), nan_out(C), nan_out(2400), nan_out(C)
    H.op_conv_wgrad(0, B, x, dy, dws, dbs, scratch(H, B))
    H.op_e1_wgrad_fused(B, x, y.reshape(-1), a, da.reshape(-1), coef, bcoef, None, None, dwf, dbf, scratch(H, B), 0)
    torch.cuda.synchronize()
    cpu64 = lambda t, *shape: t.double().cpu().view(*shape)      # noqa: E731
    dyr = E.fused_dy_ref(cpu64(y, B, W, W, C), cpu64(a, B, HO, HO, C), cpu64(da, B, HO, HO, C), cpu64(coef, C, 4), cpu64(bcoef, C, 2), False)
    x64 = x.double().cpu()
    ref_w, ref_b = E.wgrad_ref(x64, dyr, False)
    abs_w, abs_b = E.wgrad_ref(x64.abs(), dyr.abs(), False)
    rows = _rows_chain(S, False)
    worst = {}
    try:
        for name, got in (("fused", (dwf, dbf)), ("separate", (dws, dbs))):
            within(f"dW1 {name}", wref(got[0], 3, C).double(), ref_w, (32 * tps + 1 + 3 + rows) * U32 * abs_w, worst)
            within(f"db1 {name}", got[1].double().cpu(), ref_b, (16 * tps + 2 + 3 + rows) * U32 * abs_b, worst)
    finally:
        print(f"e1fused-ratio w{W} B{B} ({tiles} tiles, {S} splits of {tps}): " + ", ".join(f"{k} err / bound {v:.4f}" for k, v in worst.items())
              + f"; fused and separate bit-equal: dW1 {same_bits(dwf, dws)}, db1 {same_bits(dbf, dbs)}"
              + f" ({int((dwf != dws).sum())} of 2400 dW1 elements differ, largest |diff| {float((dwf - dws).abs().max()):.3e} of max |dW1| {float(dwf.abs().max()):.3e})")
    assert same_bits(dwf, dws) and same_bits(dbf, dbs), "the fused form and the separate passes differ in bits"


# ---------------------------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_leave_the_outputs_untouched():
    """Every CVAE_EINVAL of the entry returns before any launch: dw and dbias keep their poison, cvae_last_error names the argument."""
    W, B = 64, 3
    lib = cvlib.load()
    assert lib.cvae_conv_route(1, W, 0, 0, 65535) == 1 and lib.cvae_conv_route(1, W, 0, 0, 65536) == 0
    seen = 0
    for mode in MODES:
        H = handle(W, mode)
        bf = mode == "bf16"
        n_act = B * W * W * 32 // (2 if bf else 1)
        ok = dict(x=torch.zeros(B * 3 * W * W, device="cuda"), y0=torch.zeros(n_act, device="cuda"), a0=torch.zeros(n_act // 4, device="cuda"),
                  d_a0=torch.zeros(n_act // 4, device="cuda"), coef0=torch.ones(128, device="cuda"), bcoef0=torch.zeros(64, device="cuda"),
                  w1=torch.zeros(2400, device="cuda"), b1=torch.zeros(32, device="cuda"), dw=nan_out(2400), dbias=nan_out(32),
                  scratch=scratch(H, B))
        order = ("x", "y0", "a0", "d_a0", "coef0", "bcoef0", "w1", "b1", "dw", "dbias", "scratch")

        def call(h=H.h, batch=B, flags=0, **repl):
            a = dict(ok, **repl)
            rc = lib.cvae_op_e1_wgrad_fused(h, batch, *[None if a[k] is None else a[k].data_ptr() for k in order], flags, None)
            torch.cuda.synchronize()
            assert bool(holds(ok["dw"], ALL_ONES).all()) and bool(holds(ok["dbias"], ALL_ONES).all()), f"{mode}: a refused call wrote its outputs"
            return rc, lib.cvae_last_error().decode()

        bad = [(dict(h=None), "null handle"), (dict(batch=0), "batch 0"), (dict(batch=MAX_B + 1), f"batch {MAX_B + 1}"),
               (dict(flags=2), "flag"), (dict(flags=3), "flag"), (dict(flags=-1), "flag")]
        bad += [({k: None}, f"null {k}") for k in ("x", "a0", "d_a0", "coef0", "bcoef0", "dw", "scratch") + (("w1", "b1") if bf else ("y0",))]
        if not bf:
            bad.append((dict(flags=1), "not bf16"))
        for kw, msg in bad:
            rc, err = call(**kw)
            assert rc == -1 and msg in err and "cvae_op_e1_wgrad_fused" in err, (mode, kw.keys(), rc, err)
            seen += 1
        # a valid call on the same buffers writes them: the calls above kept the poison because they were refused, not because nothing runs
        rc = lib.cvae_op_e1_wgrad_fused(H.h, B, *[ok[k].data_ptr() for k in order], 0, None)
        torch.cuda.synchronize()
        assert rc == 0 and bool(torch.isfinite(ok["dw"]).all()) and bool(torch.isfinite(ok["dbias"]).all())
    # flag bit 0 at a batch whose packed frame would pass 2 GiB: refused before any launch (the buffers here are far too small for it)
    big = handle(W, "bf16", 65536)
    dw, db = nan_out(2400), nan_out(32)
    t = torch.zeros(4096, device="cuda")
    rc = lib.cvae_op_e1_wgrad_fused(big.h, 65536, *[t.data_ptr()] * 8, dw.data_ptr(), db.data_ptr(), t.data_ptr(), 1, None)
    torch.cuda.synchronize()
    assert rc == -1 and "cvae_conv_route" in lib.cvae_last_error().decode()
    assert bool(holds(dw, ALL_ONES).all()) and bool(holds(db, ALL_ONES).all())
    assert seen == 30
