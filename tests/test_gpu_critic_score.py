"""cvae_critic_score (csrc/critic_score.hip) and the validation loop of CriticTrainer on the device.

Frames: the 68 real frames of step_real_b68.npz["u8"], repeated / permuted; weights: the reference checkpoint's
(critic_real_b8.npz w/*), so that — through cvae_critic_forward's own fixture test — the new kernel is pinned to the reference
critic.  Targets: exact 0 and 1, every fp32 bin edge with its nextafter neighbours on both sides, and two values in the gaps
between the bins.  Batches 1, 2, 68, 257 (one past the pooling loop's 256-thread stride; with 256 compute units also the first
batch at which a workgroup of the persistent grid walks two frames) and 300 with a permuted index that repeats frames."""
import os

import numpy as np
import pytest
import torch

from critic_vae_amd import critic_train as CT
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import train as T
from critic_vae_amd.critic import CRITIC_KEYS, Critic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLS, DOUBLES = cvlib.CRITIC_SCORE_COLS, cvlib.CRITIC_SCORE_STATE_DOUBLES
EINVAL, EUNSUPPORTED = -1, -2
ONE, ZERO = np.float32(1), np.float32(0)


def _targets():
    vals = [ZERO, ONE]
    for e in (np.float32(0.4), np.float32(0.6), np.float32(0.7), np.float32(0.25)):
        vals += [e, np.nextafter(e, ZERO), np.nextafter(e, ONE)]
    vals += [np.float32(0.3), np.float32(0.65)]
    return np.resize(np.array(vals, np.float32), 68)             # the 16 values, repeated over the 68 frames


def _selection(B):
    if B == 300:
        return np.random.default_rng(300).integers(0, 68, B).astype(np.int64)      # permuted, frames repeat
    return (np.arange(B) % 68).astype(np.int64)


@pytest.fixture(scope="module")
def fx(golden_dir):
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    ck = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    w = {k: ck["w/" + k] for k, _ in CRITIC_KEYS}
    flat = np.concatenate([w[k].reshape(-1) for k, _ in CRITIC_KEYS]).astype(np.float32)
    h = cvlib.Handle(64, 320)
    t = _targets()
    return dict(h=h, w=w, u8=u8, t=t, frames=torch.from_numpy(u8).to(DEV), targets=torch.from_numpy(t).to(DEV),
                flat=torch.from_numpy(flat).to(DEV), cache={})


def _score(fx, B, frames, targets, idx=None, per_frame=True, state=None, flat=None):
    """One call on fresh buffers -> (rows (B, 8) numpy or None, state)."""
    h = fx["h"]
    rows = torch.full((B, COLS), -7.0, device=DEV) if per_frame else None
    scratch = None if per_frame else torch.empty(h.critic_score_scratch_bytes(B), dtype=torch.uint8, device=DEV)
    h.critic_score(B, frames, targets, fx["flat"] if flat is None else flat, idx=idx, per_frame=rows, state=state, scratch=scratch)
    torch.cuda.synchronize()
    return (None if rows is None else rows.cpu().numpy()), state


def _case(fx, B):
    """Rows and record of batch B through the general path (the 68 frames, idx = the selection), computed once."""
    if B not in fx["cache"]:
        sel = _selection(B)
        state = fx["h"].critic_score_state(DEV)
        rows, _ = _score(fx, B, fx["frames"], fx["targets"], idx=torch.from_numpy(sel).to(DEV), state=state)
        fx["cache"][B] = dict(sel=sel, rows=rows, rec=state.cpu().numpy())
    return fx["cache"][B]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _host_record(rows, rec=None):
    """The documented record from rows, summed in float64 on the host (added to `rec` when given)."""
    rows = np.asarray(rows, np.float32)
    out = np.zeros(27) if rec is None else rec.copy()
    if rec is None:
        out[10] = -np.inf
    fin = np.isfinite(rows[:, :5]).all(1)
    r = rows[fin].astype(np.float64)
    out[0] += rows.shape[0]
    out[1] += fin.sum()
    out[2:10] += [r[:, 2].sum(), r[:, 3].sum(), r[:, 4].sum(), r[:, 0].sum(), r[:, 1].sum(), (r[:, 0] ** 2).sum(), (r[:, 1] ** 2).sum(),
                  (r[:, 0] * r[:, 1]).sum()]
    if fin.any():
        out[10] = max(out[10], r[:, 4].max())
    for bp, bt in zip(r[:, 5].astype(int), r[:, 6].astype(int)):
        out[11 + 4 * bt + bp] += 1
    return out


def _assert_record(rec, want, what):
    assert rec.shape == (DOUBLES,) and not rec[27:].any(), f"{what}: reserved doubles / the arrival counter are not zero"
    assert np.array_equal(rec[:2], want[:2]) and rec[10] == want[10] and np.array_equal(rec[11:27], want[11:27]), what
    gap = np.abs(rec[2:10] - want[2:10])
    print(f"{what}: worst relative gap of a sum {np.max(gap / np.maximum(np.abs(want[2:10]), 1e-300)):.2e}")
    assert (gap <= 1e-12 * np.abs(want[2:10])).all(), f"{what}: sums {rec[2:10]} vs the host's {want[2:10]}"


@pytest.mark.parametrize("B", [1, 2, 68, 257, 300])
def test_p_is_bit_equal_to_gather_plus_forward(fx, B):
    """rows[:, 0] == cvae_preprocess_u8_gather + cvae_critic_forward on the same indices, rows[:, 1] == the gathered targets, bit
    for bit; the same batch laid out as frames of its own gives the same rows with idx null and with idx = arange."""
    h, c = fx["h"], _case(fx, B)
    sel, rows = c["sel"], c["rows"]
    d_sel = torch.from_numpy(sel).to(DEV)
    x, tg, pred = torch.empty(B, 3, 64, 64, device=DEV), torch.empty(B, 1, device=DEV), torch.empty(B, 1, device=DEV)
    h.preprocess_u8_gather(B, fx["frames"], fx["targets"].view(-1, 1), d_sel, x, tg)
    h.critic_forward(B, x, fx["flat"], pred)
    p_ref, t_ref = pred.cpu().numpy()[:, 0], tg.cpu().numpy()[:, 0]
    assert np.array_equal(_bits(rows[:, 0]), _bits(p_ref)), f"B={B}: p differs from the two-kernel route by {np.abs(rows[:, 0] - p_ref).max():.3e}"
    assert np.array_equal(_bits(rows[:, 1]), _bits(t_ref)) and np.array_equal(_bits(t_ref), _bits(fx["t"][sel]))
    assert (rows[:, 7] == 0).all() and np.isfinite(rows).all() and (rows[:, 0] > 0).all() and (rows[:, 0] < 1).all()
    own_f, own_t = fx["frames"][d_sel].contiguous(), fx["targets"][d_sel].contiguous()
    null, _ = _score(fx, B, own_f, own_t)
    ar, _ = _score(fx, B, own_f, own_t, idx=torch.arange(B, dtype=torch.int64, device=DEV))
    assert np.array_equal(_bits(null), _bits(ar)) and np.array_equal(_bits(null), _bits(rows))


def test_row_columns(fx):
    """[3] = (p - t)^2 and [4] = |p - t| are the fp32 results exactly; [5], [6] are episodes.value_bins of the row's own p, t.

    [2] against float64 from the row's own p and t, L = -(t max(ln p, -100) + (1 - t) max(ln(1 - p), -100)).  With e = 2^-24 (half
    an fp32 ulp, relative) the device computes -(rn(t A) + rn(u Bq)) where
      A = max(logf(p), -100): logf is documented to 1 ulp, i.e. 2 e relative; the clamp is 1-Lipschitz;
      u = rn(1 - t): e relative (exact for t >= 1/2);
      q = rn(1 - p): exact for p >= 1/2, else q in (1/2, 1] with an absolute error of at most e / 2, which moves ln q by at most
        e / (2 q) <= e;   Bq = max(logf(q), -100): 2 e relative;
      each product and the final sum: e relative.
    To first order, with T1 = t |A| and T2 = (1 - t) |B|:  |row[2] - L| <= e (4 T1 + 5 T2 + (1 - t)) — T1: 2 (logf) + 1 (product)
    + 1 (sum); T2: 1 (u) + 2 (logf) + 1 (product) + 1 (sum); (1 - t) e: the shift of ln q.  1 % is added for the second-order
    terms and 1.5e-45 (the smallest subnormal) for a result that underflows."""
    rows = _case(fx, 300)["rows"]
    p, t = rows[:, 0], rows[:, 1]
    d = p - t                                                    # numpy float32 arithmetic: each operation rounded once
    assert np.array_equal(_bits(rows[:, 3]), _bits(d * d)) and np.array_equal(_bits(rows[:, 4]), _bits(np.abs(d)))
    assert np.array_equal(rows[:, 5].astype(np.int64), E.value_bins(p)) and np.array_equal(rows[:, 6].astype(np.int64), E.value_bins(t))
    assert set(np.unique(rows[:, 6]).tolist()) == {0.0, 1.0, 2.0, 3.0} and len(np.unique(rows[:, 5])) >= 3
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    A, Bq = np.maximum(np.log(p64), -100.0), np.maximum(np.log1p(-p64), -100.0)
    want = -(t64 * A + (1 - t64) * Bq)
    T1, T2 = t64 * np.abs(A), (1 - t64) * np.abs(Bq)
    bound = 2.0 ** -24 * (4 * T1 + 5 * T2 + (1 - t64)) * 1.01 + 1.5e-45
    gap = np.abs(rows[:, 2].astype(np.float64) - want)
    print(f"BCE column: worst gap {gap.max():.3e}, worst gap / bound {np.max(gap / bound):.3f}")
    assert (gap <= bound).all(), f"worst gap / bound {np.max(gap / bound):.3f}"


@pytest.mark.parametrize("bias,p_want", [(200.0, 1.0), (-200.0, 0.0)])
def test_saturated_sigmoid(fx, bias, p_want):
    """All parameters zero but crit.4.bias = +-200: p is exactly 1 or 0; against t = 0 and 1 the BCE term is exactly 100 or 0 and
    finite — torch.nn.functional.binary_cross_entropy's value on the CPU for the same p and t."""
    flat = torch.zeros_like(fx["flat"])
    flat[-1] = bias
    t = torch.tensor([0.0, 1.0], device=DEV)
    state = fx["h"].critic_score_state(DEV)
    rows, _ = _score(fx, 2, fx["frames"][:2], t, state=state, flat=flat)
    assert (rows[:, 0] == p_want).all() and np.isfinite(rows).all()
    want = torch.nn.functional.binary_cross_entropy(torch.from_numpy(rows[:, 0].copy()), t.cpu(), reduction="none").numpy()
    assert np.array_equal(rows[:, 2], want) and sorted(rows[:, 2].tolist()) == [0.0, 100.0]
    assert np.array_equal(rows[:, 3], (rows[:, 0] - rows[:, 1]) ** 2) and np.array_equal(rows[:, 4], np.abs(rows[:, 0] - rows[:, 1]))
    rec = state.cpu().numpy()
    assert rec[0] == 2 and rec[1] == 2 and rec[2] == 100.0 and rec[10] == 1.0


@pytest.mark.parametrize("B", [1, 257])
def test_pooled_record(fx, B):
    """Counts, confusion matrix and maximum exactly, every sum within 1e-12 relative of the float64 host sum of the call's own
    rows (fp64 reordering is the only difference); without per_frame (rows in scratch) the record is the same, bit for bit."""
    c = _case(fx, B)
    _assert_record(c["rec"], _host_record(c["rows"]), f"B={B}")
    assert c["rec"][0] == B == c["rec"][1] and c["rec"][11:27].sum() == B
    state = fx["h"].critic_score_state(DEV)
    _score(fx, B, fx["frames"], fx["targets"], idx=torch.from_numpy(c["sel"]).to(DEV), per_frame=False, state=state)
    assert np.array_equal(_bits(state.cpu().numpy()), _bits(c["rec"]))


def test_two_calls_add_into_one_record(fx):
    """68 frames, then 5: the record equals one host sum over the 73 rows — the second call found the arrival counter at 0."""
    state = fx["h"].critic_score_state(DEV)
    r1, _ = _score(fx, 68, fx["frames"], fx["targets"], state=state)
    mid = state.cpu().numpy()
    assert not mid[27:].any()
    r2, _ = _score(fx, 5, fx["frames"][30:35], fx["targets"][30:35], state=state)
    rec = state.cpu().numpy()
    _assert_record(rec, _host_record(np.concatenate([r1, r2])), "68 + 5")
    assert rec[0] == 73 and rec[1] == 73
    assert np.array_equal(_bits(r2), _bits(r1[30:35]))


def test_nan_target_is_counted_not_summed(fx):
    t = fx["targets"].clone()
    t[11] = float("nan")
    state = fx["h"].critic_score_state(DEV)
    rows, _ = _score(fx, 68, fx["frames"], t, state=state)
    rec = state.cpu().numpy()
    assert rec[0] == 68 and rec[1] == 67 and np.isfinite(rec[2:11]).all() and rec[11:27].sum() == 67
    assert np.isnan(rows[11, 1]) and np.isnan(rows[11, 2:5]).all() and rows[11, 6] == 3 and np.isfinite(rows[11, 0])
    _assert_record(rec, _host_record(rows), "NaN target")
    clean = _case(fx, 68)["rows"]
    keep = np.arange(68) != 11
    assert np.array_equal(_bits(rows[keep]), _bits(clean[keep]))


def test_determinism(fx):
    """The same calls twice: byte-identical rows and record (two batches into one record, the second with several frames per
    workgroup on any device of fewer than 300 compute units)."""
    def run():
        state = fx["h"].critic_score_state(DEV)
        a, _ = _score(fx, 68, fx["frames"], fx["targets"], state=state)
        b, _ = _score(fx, 300, fx["frames"], fx["targets"], idx=torch.from_numpy(_selection(300)).to(DEV), state=state)
        return a, b, state.cpu().numpy()
    x, y = run(), run()
    for u, v, name in zip(x, y, ("rows of call 1", "rows of call 2", "record")):
        assert np.array_equal(_bits(u), _bits(v)), f"{name}: two runs differ"


def _dataset(fx, lo, hi, traj):
    n = hi - lo
    source = np.stack([np.full(n, traj, np.int64), np.arange(n, dtype=np.int64)], 1)
    return E.DeviceDataset(fx["frames"][lo:hi].contiguous(), fx["targets"][lo:hi].reshape(n, 1).contiguous(), source)


def _critic(fx):
    critic = Critic(handle=fx["h"]).to(DEV)
    critic.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx["w"].items()})
    return critic


def test_evaluate_agrees_with_score_frames(fx):
    """CriticTrainer.evaluate == the host summary of a loop over score_frames; the same at batch sizes 7 and 68 (counts, maximum
    and confusion exactly, sums to fp64 reordering); it leaves the training state and the generators alone."""
    critic = _critic(fx)
    tr = CT.CriticTrainer(critic)
    ds = _dataset(fx, 0, 68, 0)
    before = [t.clone() for t in (tr.theta, tr.m, tr.v)]
    rng_state, np_state = torch.cuda.get_rng_state(), np.random.get_state()[1].copy()
    r7, r68 = tr.evaluate(ds, 7, per_frame=True), tr.evaluate(ds, 68)
    rows = torch.cat([CT.score_frames(critic, ds.frames[b:b + 7], ds.preds[b:b + 7].view(-1)) for b in range(0, 68, 7)]).cpu().numpy()
    assert torch.equal(torch.cuda.get_rng_state(), rng_state) and np.array_equal(np.random.get_state()[1], np_state)
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.theta, tr.m, tr.v))) and tr.step_count == 0 and tr.val_history == []
    assert np.array_equal(_bits(r7["per_frame"].cpu().numpy()), _bits(rows)) and "per_frame" not in r68
    assert np.array_equal(_bits(rows), _bits(_case(fx, 68)["rows"]))
    idx_rows = CT.score_frames(critic, ds.frames, ds.preds.view(-1), idx=torch.arange(67, -1, -1, device=DEV)).cpu().numpy()
    assert np.array_equal(_bits(idx_rows[::-1]), _bits(rows))
    want = CT.summarize_record(_host_record(rows), "bce")
    for r in (r7, r68):
        assert r["frames"] == 68 == r["finite_frames"] and np.array_equal(r["confusion"], want["confusion"])
        assert r["worst"] == want["worst"] and r["bin_agreement"] == want["bin_agreement"] and r["loss"] == r["bce"]
        for k in ("bce", "mse", "mae", "pearson", "mean_pred", "mean_target"):
            assert abs(r[k] - want[k]) <= 1e-12 * abs(want[k]), (k, r[k], want[k])
    assert CT.CriticTrainer(_critic(fx), loss="mse").evaluate(ds, 68)["loss"] == r68["mse"]


def _fit(fx, **kw):
    critic = _critic(fx)
    tr = CT.CriticTrainer(critic)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    np.random.seed(3)
    log = tr.fit_device(_dataset(fx, 0, 60, 0), 32, epochs=2, generator=gen, **kw)
    return tr, log.cpu().numpy()


def test_validation_does_not_touch_the_training_run(fx):
    """2 epochs over 60 frames with and without val= (8 frames of a second trajectory): bit-identical log and parameters;
    val_history holds 2 entries; a patience of 1 stops the fit after the first evaluation that is no improvement."""
    val = _dataset(fx, 60, 68, 1)
    plain, log0 = _fit(fx)
    seen = []
    tr, log1 = _fit(fx, val=val, on_val=lambda t, r: seen.append((t.step_count, r["loss"])) and False)
    assert log0.shape == (4, 4) and np.array_equal(_bits(log0), _bits(log1))
    for a, b in zip((plain.theta, plain.m, plain.v), (tr.theta, tr.m, tr.v)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert [s for s, _ in tr.val_history] == [2, 4] and seen == [(s, r["loss"]) for s, r in tr.val_history] and plain.val_history == []
    for _, r in tr.val_history:
        assert r["frames"] == 8 == r["finite_frames"] and np.isfinite(r["loss"]) and r["confusion"].sum() == 8
    assert tr.val_history[0][1]["loss"] != tr.val_history[1][1]["loss"]          # the parameters moved in between
    st = tr.state_dict()
    assert len(st["val_history"]) == 2 and isinstance(st["val_history"][0][1]["confusion"], list) and st["val_stale"] == 0
    # after every optimizer step instead of every epoch
    tr2, log2 = _fit(fx, val=val, val_every=1)
    assert [s for s, _ in tr2.val_history] == [1, 2, 3, 4] and np.array_equal(_bits(log2), _bits(log0))
    # the command line's callback with --patience 1 against a best value nothing can beat
    args = T.build_parser().parse_args(["-critic", "--episodes", "e", "--rewards", "r", "--save", "d", "--val-fraction", "0.2", "--patience", "1"])
    critic = _critic(fx)
    tr3 = CT.CriticTrainer(critic)
    tr3.best_val = -1.0
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    np.random.seed(3)
    log3 = tr3.fit_device(_dataset(fx, 0, 60, 0), 32, epochs=2, generator=gen, val=val, on_val=T._CriticValidationLog(args)).cpu().numpy()
    assert log3.shape == (2, 4) and np.array_equal(_bits(log3), _bits(log0[:2])) and tr3.step_count == 2
    assert len(tr3.val_history) == 1 and tr3.val_stale == 1
    with pytest.raises(ValueError):
        plain.fit_device(_dataset(fx, 0, 60, 0), 32, on_val=lambda t, r: False)


def test_argument_checks_launch_nothing(fx):
    h, lib = fx["h"], fx["h"].lib
    rows = torch.full((8, COLS), -7.0, device=DEV)
    state = h.critic_score_state(DEV)
    rec0 = state.cpu().numpy()
    f, t, p, st = fx["frames"].data_ptr(), fx["targets"].data_ptr(), fx["flat"].data_ptr(), torch.cuda.current_stream().cuda_stream

    def call(hh=h.h, B=4, frames=f, rows_ptr=rows.data_ptr(), state_ptr=state.data_ptr()):
        return lib.cvae_critic_score(hh, B, frames, t, 68, None, p, rows_ptr, state_ptr, None, st)

    wide = cvlib.Handle(128, 2)
    assert call(B=0) == EINVAL and call(B=65537) == EINVAL and call(frames=None) == EINVAL
    assert call(rows_ptr=None, state_ptr=None) == EINVAL and call(hh=wide.h) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (rows == -7.0).all() and np.array_equal(_bits(state.cpu().numpy()), _bits(rec0))
    assert call() == 0                                            # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rows[:4].cpu().numpy()), _bits(_case(fx, 68)["rows"][:4])) and (rows[4:] == -7.0).all()


def test_out_of_range_index_gives_a_nan_row(fx):
    """A checked argument path: the index is never dereferenced, its row is NaN, counted as seen and not as finite; the
    neighbouring rows are what they are without it."""
    idx = torch.tensor([0, 68, 1, -1, 2, 2 ** 40], dtype=torch.int64, device=DEV)
    state = fx["h"].critic_score_state(DEV)
    rows, _ = _score(fx, 6, fx["frames"], fx["targets"], idx=idx, state=state)
    clean = _case(fx, 68)["rows"]
    assert np.array_equal(_bits(rows[[0, 2, 4]]), _bits(clean[:3]))
    for i in (1, 3, 5):
        assert np.isnan(rows[i, :5]).all() and rows[i, 5] == 3 and rows[i, 6] == 3 and rows[i, 7] == 0
    rec = state.cpu().numpy()
    assert rec[0] == 6 and rec[1] == 3
    _assert_record(rec, _host_record(rows), "out-of-range indices")
