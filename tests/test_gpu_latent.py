"""The latent audit on the GPU: cvae_latent_stats' pooled record against latent.record_host — by EQUALITY where every product and
partial sum is exact in fp64 (integer mu and logvar, pred in eighths), within derived bounds otherwise —, rows left out,
memory / determinism / stream hygiene, FusedTrainer.latent_report end to end on the 68 real fixture frames, and
cvae_recon_response (latent.decoder_response) against float64 and against diff_images.

Bounds (u = 2^-53, so 2^-52 = 2 u allows the device's and the host's own roundings).  n = rows used.
  Gram and first-moment sums: the products of widened fp32 values are exact in fp64; a sum of n terms in ANY order errs by at
    most (n - 1) u sum |terms| on each side:  |dev - ref| <= n 2^-52 sum |a_i a_j|.
  KL and exp sums: per term an exp within 1 ulp on each side and four roundings (mu^2 + e, - lv, - 1, * 0.5 is exact), then n
    additions:  |dev - ref| <= (n + 16) 2^-52 sum_rows 0.5 (mu^2 + e^lv + |lv| + 1).
Largest measured ratio to the bound on an MI355X (check() prints every one): README.md, "Latent audit"."""
import functools
import os

import numpy as np
import pytest
import torch

from critic_vae_amd import episodes as E
from critic_vae_amd import latent as LT
from critic_vae_amd import lib as cvlib
from critic_vae_amd.train import FusedTrainer
from ws_tools import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = np.r_[0:596, 660:692]           # slots whose sums are exact on integer data
U52 = 2.0 ** -52
WORST = {}


@functools.lru_cache(maxsize=None)
def handle(width=64, max_batch=8, precision="f32"):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return cvlib.Handle(width, max_batch, precision=precision)


@functools.lru_cache(maxsize=None)
def plan():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = cvlib.latent_stats_plan(1 << 24, cus)             # the largest batch: the grid the launcher itself stops at
    assert p["chunks"] > p["grid"] >= 1
    return p["rows"], p["grid"]


@functools.lru_cache(maxsize=None)
def exact_inputs(B, seed=0):
    rng = np.random.default_rng(1000 * seed + B % 997)
    mu = rng.integers(-8, 9, (B, 32)).astype(np.float32)
    lv = rng.integers(-3, 4, (B, 32)).astype(np.float32)
    pred = (rng.integers(0, 9, B) / 8.0).astype(np.float32)
    return mu, lv, pred


@functools.lru_cache(maxsize=None)
def gauss_inputs(B, seed=0):
    rng = np.random.default_rng(77 + seed)
    mu = (rng.standard_normal((B, 32)) * rng.uniform(0.1, 3.0, 32)).astype(np.float32)
    lv = (rng.standard_normal((B, 32)) * 1.5 - 1.0).astype(np.float32)
    return mu, lv, rng.uniform(0, 1, B).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_record(kind, B, seed=0):
    return LT.record_host(*(exact_inputs if kind == "exact" else gauss_inputs)(B, seed))


def bounds(mu, lv, pred):
    """The allowed |dev - ref| of every slot of the record of these (used) rows."""
    m, l, p = mu.astype(np.float64), lv.astype(np.float64), np.asarray(pred, np.float64).reshape(-1)
    n = m.shape[0]
    a = np.abs(np.concatenate([m, p[:, None]], 1))
    b = np.zeros(LT.RECORD)
    b[LT.SUM:LT.GRAM] = n * U52 * a.sum(0)
    b[LT.GRAM:LT.KL] = n * U52 * (a.T @ a)[np.triu_indices(33)]
    b[LT.KL:LT.EXP] = b[LT.EXP:LT.LV] = (n + 16) * U52 * (0.5 * (m * m + np.exp(l) + np.abs(l) + 1.0)).sum(0)
    b[LT.LV:] = n * U52 * np.abs(l).sum(0)
    return b


def check(what, got, want, bound):
    err = np.abs(got - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"{what}: largest |dev - ref| / bound = {ratio:.4f}")
    assert np.isfinite(got).all() and ratio <= 1.0, (what, ratio, int(np.argmax(err - bound)))


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def run(B, mu, lv, pred, state=None, scratch=None, kl_rows=None, H=None):
    H = H or handle()
    state = H.latent_stats_state("cuda") if state is None else state
    scratch = H.latent_stats_scratch(B, "cuda") if scratch is None else scratch
    H.latent_stats(B, mu, lv, pred, state, scratch, kl_rows)
    return state


def batches():
    R, G = plan()
    return sorted({1, 2, R - 1, R, R + 1, 2 * R + 1, G * R - 1, G * R, G * R + 1, 2 * G * R + 1})


def test_exact_record_at_every_chunk_and_grid_edge():
    """Integer data: slots [0..595] and [660..691] by equality, the KL and exp sums within their bound, at batches below, at and
    above one chunk, one chunk per workgroup and two; batch is not capped by the handle's max_batch (8)."""
    for B in batches():
        mu, lv, pred = exact_inputs(B)
        got = run(B, *dev(mu, lv, pred)).cpu().numpy()
        want = host_record("exact", B)
        assert np.array_equal(got[EXACT], want[EXACT]), (B, np.flatnonzero(got[:LT.RECORD] != want)[:8])
        assert got[0] == B and got[1] == B and not got[LT.RECORD:].any()       # the arrival counter is back at 0
        check("exact batches, KL and exp sums", got[:LT.RECORD], want, bounds(mu, lv, pred))


def test_second_call_adds_to_the_record():
    R, _ = plan()
    (m1, l1, p1), (m2, l2, p2) = exact_inputs(R + 1), exact_inputs(2 * R + 1, seed=1)
    state = run(R + 1, *dev(m1, l1, p1))
    got = run(2 * R + 1, *dev(m2, l2, p2), state=state).cpu().numpy()
    mu, lv, pred = np.concatenate([m1, m2]), np.concatenate([l1, l2]), np.concatenate([p1, p2])
    want = LT.record_host(mu, lv, pred)
    assert np.array_equal(got[EXACT], want[EXACT])
    check("two calls, KL and exp sums", got[:LT.RECORD], want, bounds(mu, lv, pred))


def test_gaussian_inputs_within_the_derived_bounds():
    R, G = plan()
    for B in (R + 1, 2 * G * R + 1):
        mu, lv, pred = gauss_inputs(B)
        got = run(B, *dev(mu, lv, pred)).cpu().numpy()
        assert got[0] == B and got[1] == B
        check("gaussian batches, every sum", got[:LT.RECORD], host_record("gauss", B), bounds(mu, lv, pred))


def test_rows_left_out_are_counted_not_hidden():
    R, _ = plan()
    B = 2 * R + 1
    mu, lv, pred = (a.copy() for a in exact_inputs(B, seed=2))
    mu[3, 5] = np.nan
    lv[R, 0] = np.inf
    lv[R + 5, 31] = -np.inf
    lv[7, 2] = 800.0                 # finite input, exp overflows in fp64
    pred[2 * R] = np.nan
    lv[11, 4] = 100.0                # stays in: e^100 is finite in fp64
    out = [3, R, R + 5, 7, 2 * R]
    keep = np.setdiff1d(np.arange(B), out)
    kl = torch.full((B, 32), 7.0, device="cuda")
    got = run(B, *dev(mu, lv, pred), kl_rows=kl).cpu().numpy()
    want = LT.record_host(mu[keep], lv[keep], pred[keep])
    assert got[0] == B and got[1] == B - len(out) == want[1]
    assert np.array_equal(got[EXACT][1:], want[EXACT][1:])
    check("rows left out, KL and exp sums", got[:LT.RECORD], np.r_[B, want[1:]], bounds(mu[keep], lv[keep], pred[keep]))
    assert got[LT.EXP + 4] > 1e43
    # kl_rows: every row, used or not, whatever the arithmetic gives
    k64 = LT.kl_rows_host(mu, lv)
    with np.errstate(over="ignore"):
        kf = k64.astype(np.float32)
    kd = kl.cpu().numpy()
    fin = np.isfinite(kf)
    assert np.array_equal(np.isnan(kd), np.isnan(kf)) and np.array_equal(kd[~fin & ~np.isnan(kf)], kf[~fin & ~np.isnan(kf)])
    assert (np.abs(kd[fin].astype(np.float64) - kf[fin]) <= np.spacing(np.abs(kf[fin]))).all()
    assert np.isnan(kd[3, 5]) and np.isinf(kd[7, 2]) and np.isnan(kd[R, 0]) and np.isinf(kd[R + 5, 31])      # inf - inf; 0 + inf


# ---- the side-stream case of the two entry points that end in (stream, flags): tests/stream_tools.py does not see them ----
@functools.lru_cache(maxsize=None)
def blocker():
    """(matrix, products for about 0.25 s of torch.mm on the device), measured once."""
    a = torch.randn(4096, 4096, device="cuda") * 0.01
    b = torch.empty_like(a)
    for _ in range(4):
        torch.mm(a, a, out=b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(16):
        torch.mm(a, a, out=b)
    e1.record(); e1.synchronize()
    return a, b, max(16, int(0.25 / max(e0.elapsed_time(e1) / 1000.0 / 16, 1e-6)))


def block_null_stream():
    """About 0.25 s of work on the null (current) stream; returns the event behind it."""
    a, b, n = blocker()
    for _ in range(n):
        torch.mm(a, a, out=b)
    ev = torch.cuda.Event()
    ev.record()
    return ev


@functools.lru_cache(maxsize=None)
def independent_stream():
    """A torch side stream on which a tiny kernel completes while the null stream is busy (streams can share a hardware queue)."""
    probe = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(8):
        s = torch.cuda.Stream()
        end = block_null_stream()
        with torch.cuda.stream(s):
            probe.add_(1.0)
        s.synchronize()
        free = not end.query()
        torch.cuda.synchronize()
        if free:
            return s
    pytest.fail("no side stream runs while the null stream is busy: the side-stream case cannot be decided here")


def on_side_stream_with_null_busy(call, result):
    """Run `call` under a side stream while the null stream is busy and copy `result` to the host ON THE SIDE STREAM; the null
    stream's work must still be running when the copy has arrived: a launcher that ignored its stream argument would have queued
    its kernel behind that work, and the copy would hold the old bytes."""
    side = independent_stream()
    host = torch.empty(result.shape, dtype=result.dtype, pin_memory=True)
    torch.cuda.synchronize()
    end = block_null_stream()
    with torch.cuda.stream(side):
        call()
        host.copy_(result, non_blocking=True)
    side.synchronize()
    still_busy = not end.query()
    torch.cuda.synchronize()
    assert still_busy, "inconclusive: the null stream's work had ended when the side stream's result arrived"
    return host.clone()


def test_hygiene_scratch_repeat_stream_kl_rows():
    R, G = plan()
    B = G * R + 1
    mu, lv, pred = dev(*gauss_inputs(B, seed=3))
    H = handle()
    first = run(B, mu, lv, pred)
    assert same_bits(run(B, mu, lv, pred), first), "the same call twice"
    dirty = torch.full((H.latent_stats_scratch_bytes(B),), 0xFF, dtype=torch.uint8, device="cuda")
    assert same_bits(run(B, mu, lv, pred, scratch=dirty.view(torch.float64)), first), "scratch full of 0xFF bytes"
    # a side stream while the null stream is busy: the result is read back on the side stream alone
    kl = torch.empty(B, 32, device="cuda")
    pred1 = pred.reshape(B, 1)
    state, scratch = H.latent_stats_state("cuda"), H.latent_stats_scratch(B, "cuda")
    on_side = on_side_stream_with_null_busy(lambda: H.latent_stats(B, mu, lv, pred1, state, scratch, kl), state)
    assert same_bits(on_side, first.cpu()), "a call on a side stream"
    kf = LT.kl_rows_host(*gauss_inputs(B, seed=3)[:2]).astype(np.float32)
    assert (np.abs(kl.cpu().numpy().astype(np.float64) - kf) <= np.spacing(np.abs(kf))).all(), "kl_rows within 1 fp32 ulp"


def test_einval_leaves_the_state_untouched():
    H = handle()
    mu, lv, pred = dev(*exact_inputs(5))
    state = run(5, mu, lv, pred)
    before = state.clone()
    scratch = H.latent_stats_scratch(5, "cuda")
    ok = dict(B=5, mu=mu, logvar=lv, pred=pred, state=state, scratch=scratch, kl_rows=None, flags=0)
    for bad in (dict(flags=1), dict(B=0), dict(B=(1 << 24) + 1), dict(mu=None), dict(logvar=None), dict(pred=None), dict(scratch=None),
                dict(state=state.data_ptr() + 4), dict(scratch=scratch.data_ptr() + 4), dict(mu=mu.data_ptr() + 2),
                dict(kl_rows=mu.data_ptr() + 1)):
        with pytest.raises(cvlib.CvaeError):
            H.latent_stats(**dict(ok, **bad))
    torch.cuda.synchronize()
    assert same_bits(state, before)
    assert np.array_equal(run(5, mu, lv, pred, state=state).cpu().numpy()[EXACT], 2 * before.cpu().numpy()[EXACT])


# ---- end to end on the 68 real fixture frames, the weights test_gpu_score.py trains from the fixtures ----
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_latent_report_end_to_end(precision):
    from test_gpu_score import real_fixture, score_fixture, scoring_vae
    vae, _, pred = scoring_vae(68, precision)
    fx, sf = real_fixture(), score_fixture()
    ds = E.DeviceDataset(torch.from_numpy(fx["u8"][sf["index"]].copy()).cuda(), pred.clone(),
                         np.stack([np.zeros(68, np.int64), np.arange(68)], 1))
    tr = FusedTrainer(vae)
    kept = lambda: [t.clone() for t in (vae.theta.data, tr.m, tr.v, vae.bn_state)]      # noqa: E731
    before, steps, nbt = kept(), tr.step_count, vae.num_batches_tracked
    r68 = tr.latent_report(ds, 68)
    r17 = tr.latent_report(ds, 17)
    ev = tr.evaluate(ds, 68)
    assert all(same_bits(a, b) for a, b in zip(before, kept())) and tr.step_count == steps and vae.num_batches_tracked == nbt
    # a direct eval forward of the same gathered frames
    h = vae.handle
    x, pg = torch.empty(68, 3, 64, 64, device="cuda"), torch.empty(68, 1, device="cuda")
    ds.gather(h, 68, torch.arange(68, device="cuda"), x, pg)
    mu, lv, zero = torch.empty(68, 32, device="cuda"), torch.empty(68, 32, device="cuda"), torch.zeros(68, 32, device="cuda")
    h.forward(68, x, pg, zero, vae.theta.data, vae.bn_state, mu, lv, None, vae._workspace(68), train=False)
    m, l, p = mu.cpu().numpy(), lv.cpu().numpy(), pg.cpu().numpy()
    want, bnd = LT.record_host(m, l, p), bounds(m, l, p)
    assert r68["rows"] == r68["used"] == r17["rows"] == r17["used"] == 68 and want[1] == 68
    check(f"latent_report(68) {precision}", r68["record"], want, bnd)
    check(f"latent_report(17) against batch 68 {precision}", r17["record"], r68["record"], bnd)
    # the pooled KLD of evaluate(): score.hip evaluates each term in fp32
    kld = 0.001 * r68["record"][LT.KL:LT.EXP].sum() / 68
    m64, l64 = m.astype(np.float64), l.astype(np.float64)
    allowed = 8 * 2.0 ** -24 * 0.001 * (0.5 * (1 + np.abs(l64) + m64 * m64 + np.exp(l64))).sum(1).mean() + 2.0 ** -23 * abs(ev["KLD"])
    print(f"KLD: record {kld!r} evaluate {ev['KLD']!r} allowed {allowed:.3e} active units {r68['n_active']} probe R^2 {r68['probe_r2']:.4f}")
    assert abs(kld - ev["KLD"]) <= allowed
    assert abs(r68["kl_total"] * 0.001 - kld) <= 1e-12 and len(LT.report_lines(r68)) == 36
    # frames in hand give the same record
    s = vae.latent_stats(x, pg)
    check(f"vae.latent_stats {precision}", s["record"], want, bnd)


# ---- cvae_recon_response ----
@functools.lru_cache(maxsize=None)
def quarter_recons(W, n, K):
    rng = np.random.default_rng(W + 10 * n + K)
    base = (rng.integers(0, 5, (n, 3, W, W)) / 4.0).astype(np.float32)
    var = (rng.integers(0, 5, (n, K, 3, W, W)) / 4.0).astype(np.float32)
    return base, var


def response_ref(base, var):
    d = var.astype(np.float64) - base.astype(np.float64)[:, None]
    grey = 0.2989 * np.abs(d[:, :, 0]) + 0.5870 * np.abs(d[:, :, 1]) + 0.1140 * np.abs(d[:, :, 2])
    return (d * d).mean(axis=(2, 3, 4)), grey.max(axis=(2, 3))


@pytest.mark.parametrize("W,n,K", [(64, 1, 1), (64, 3, 34), (128, 2, 3)])
def test_recon_response_exact_and_nan(W, n, K):
    H = handle(W, 4)
    base, var = quarter_recons(W, n, K)
    b, v = dev(base, var)
    out = torch.full((n, K, 2), -1.0, device="cuda")
    H.recon_response(n, K, b, v, out)
    got = out.cpu().numpy()
    mse, grey = response_ref(base, var)
    # squares are multiples of 1/16 up to 1 and their sum is exact in fp64: the one rounding left is (float)(sum / 3 W^2)
    assert np.array_equal(got[..., 0], mse.astype(np.float32))
    # values up to 1: three products and two additions in fp32 (one fused) and three fp32 coefficients, each within 2^-24
    assert np.abs(got[..., 1] - grey).max() <= 8 * 2.0 ** -24
    # a planted NaN: both columns of its (image, variant), nothing else
    i, k = n - 1, K // 2
    v2 = v.clone()
    v2[i, k, 1, W // 2, 3] = float("nan")
    out2 = torch.empty_like(out)
    H.recon_response(n, K, b, v2, out2)
    got2 = out2.cpu().numpy()
    assert np.isnan(got2[i, k]).all()
    mask = np.ones((n, K), bool); mask[i, k] = False
    assert np.array_equal(got2[mask], got[mask])
    out3 = torch.full((n, K, 2), -1.0, device="cuda")
    on_side = on_side_stream_with_null_busy(lambda: H.recon_response(n, K, b, v, out3), out3)
    assert same_bits(on_side, out.cpu()), "a call on a side stream"
    with pytest.raises(cvlib.CvaeError):
        H.recon_response(n, K, b, v, out, flags=1)
    with pytest.raises(cvlib.CvaeError):
        H.recon_response(n, K, b.data_ptr() + 4, v, out)


def test_decoder_response_on_real_frames():
    from test_gpu_score import scoring_vae
    vae, x, pred = scoring_vae(5 * LT.RESPONSE_VARIANTS)
    x, pred = x[:5].contiguous(), pred[:5].contiguous()
    resp = LT.decoder_response(vae, x, pred)
    assert tuple(resp.shape) == (5, 34, 2)
    one, zero_, _, max_values = vae.diff_images(x, pred)
    assert same_bits(resp[:, 32, 1].contiguous(), max_values.contiguous()), (resp[:, 32, 1], max_values)
    d = zero_.double() - one.double()
    mse = (d * d).flatten(1).mean(1).cpu().numpy()
    got = resp[:, 32, 0].cpu().numpy().astype(np.float64)
    print("pred -> 0: mse", got, "float64", mse)
    assert (np.abs(got - mse) <= (3 * 64 * 64 + 4) * 2.0 ** -24 * mse).all()
    s = LT.summarize_response(resp)
    assert s["frames"] == 5 and np.isfinite(s["latent_response"]).all() and s["pred_response"] > 0
