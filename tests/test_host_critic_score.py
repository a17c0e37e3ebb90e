"""Held-out validation of the critic without a GPU: the host statement of the bin rule (episodes.value_bins) against the
selection walk, the record -> dict arithmetic (critic_train.summarize_record) on hand-built records, the split of a critic
dataset's source array, the command line of `-critic`, and the size queries / argument checks of cvae_critic_score that
precede any device access."""
import os
import re

import numpy as np
import pytest
import torch

from critic_vae_amd import critic_train as CT
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = (np.float32(0.4), np.float32(0.6), np.float32(0.7), np.float32(0.25))
ONE, ZERO = np.float32(1), np.float32(0)


def test_value_bins_at_every_edge_and_its_neighbours():
    lo, hi, high, low = EDGES
    below = lambda v: np.nextafter(v, ZERO)                      # noqa: E731
    above = lambda v: np.nextafter(v, ONE)                       # noqa: E731
    cases = [(lo, 0), (below(lo), 3), (above(lo), 0),            # mid is closed on both sides
             (hi, 0), (below(hi), 0), (above(hi), 3),
             (high, 1), (below(high), 3), (above(high), 1),      # high: v >= 0.7
             (low, 2), (below(low), 2), (above(low), 3),         # low: v <= 0.25
             (ZERO, 2), (ONE, 1), (np.float32(0.5), 0), (np.float32(0.3), 3), (np.float32(0.65), 3),
             (np.float32("nan"), 3), (np.float32("inf"), 1), (np.float32("-inf"), 2)]
    got = E.value_bins(np.array([v for v, _ in cases], np.float32))
    assert got.dtype == np.int64 and got.tolist() == [b for _, b in cases]
    # the edges are the float32 ones: the double 0.7 lies below fp32(0.7) and above fp32(0.6)'s neighbour, and is taken to float32 first
    assert E.value_bins(0.7) == 1 and E.value_bins(np.float64(0.6)) == 0 and E.value_bins([[0.25, 0.26]]).tolist() == [[2, 3]]
    assert (E.MID_LO, E.MID_HI, E.HIGH, E.LOW) == EDGES


def test_value_bins_agree_with_the_selection_walk(golden_dir):
    """_select_walk with no cap and no cut bins every frame it keeps: its choice on the reference critic's values of the 68 real
    frames is value_bins', and what it skips is bin 3."""
    preds = np.load(os.path.join(golden_dir, "episodes_real.npz"))["pool_preds"]
    _, rows, counts = E._select_walk([preds], 10 ** 9, 10 ** 9, lambda t, i: [(i, 0)], lambda t, i: [(i, 1)], lambda t, i: [(i, 2)])
    walk = np.full(preds.shape[0], 3, np.int64)
    for i, b in rows:
        walk[i] = b
    bins = E.value_bins(preds)
    assert np.array_equal(bins, walk)
    assert counts[0].tolist() == [int((bins == k).sum()) for k in range(3)] and min(counts[0]) > 0 and (bins == 3).any()


def record(p, t):
    """The pooled record cvae_critic_score documents, built on the host from values p and targets t (float32)."""
    p, t = np.asarray(p, np.float32), np.asarray(t, np.float32)
    rec = np.zeros(cvlib.CRITIC_SCORE_STATE_DOUBLES)
    rec[10] = -np.inf
    rec[0] = p.size
    with np.errstate(divide="ignore", invalid="ignore"):
        bce = -(t * np.maximum(np.log(p), np.float32(-100)) + (ONE - t) * np.maximum(np.log(ONE - p), np.float32(-100)))
    d = p - t
    fin = np.isfinite(p) & np.isfinite(t) & np.isfinite(bce) & np.isfinite(d * d)
    p64, t64 = p[fin].astype(np.float64), t[fin].astype(np.float64)
    rec[1] = fin.sum()
    rec[2:10] = [bce[fin].astype(np.float64).sum(), (d * d)[fin].astype(np.float64).sum(), np.abs(d)[fin].astype(np.float64).sum(),
                 p64.sum(), t64.sum(), (p64 * p64).sum(), (t64 * t64).sum(), (p64 * t64).sum()]
    if fin.any():
        rec[10] = np.abs(d)[fin].max()
    for bp, bt in zip(E.value_bins(p[fin]), E.value_bins(t[fin])):
        rec[11 + 4 * bt + bp] += 1
    return rec


def test_summarize_record_on_a_hand_built_record():
    p = np.array([0.5, 0.9, 0.1, 0.3, 0.65, 0.75], np.float32)
    t = np.array([0.45, 1.0, 0.0, 0.8, 0.65, 0.2], np.float32)
    r = CT.summarize_record(record(p, t), "bce")
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    assert r["frames"] == 6 and r["finite_frames"] == 6
    assert abs(r["mse"] - np.mean((p - t).astype(np.float64) ** 2)) < 1e-7 and abs(r["mae"] - np.mean(np.abs(p - t))) < 1e-7
    want_bce = -np.mean(t64 * np.log(p64) + (1 - t64) * np.log(1 - p64))
    assert abs(r["bce"] - want_bce) < 1e-6 and r["loss"] == r["bce"]
    assert CT.summarize_record(record(p, t), "mse")["loss"] == r["mse"]
    assert abs(r["pearson"] - np.corrcoef(p64, t64)[0, 1]) < 1e-12
    assert abs(r["mean_pred"] - p64.mean()) < 1e-15 and abs(r["mean_target"] - t64.mean()) < 1e-15
    assert r["worst"] == float(np.abs(p - t).max())
    # bins of p: mid high low none none high; of t: mid high low high none low
    want = np.zeros((4, 4), np.int64)
    for bt, bp in ((0, 0), (1, 1), (2, 2), (1, 3), (3, 3), (2, 1)):
        want[bt, bp] += 1
    assert r["confusion"].dtype == np.int64 and np.array_equal(r["confusion"], want)
    assert r["bin_agreement"] == 4 / 6
    with pytest.raises(ValueError):
        CT.summarize_record(np.zeros(10))
    with pytest.raises(ValueError):
        CT.summarize_record(record(p, t), "l1")


def test_summarize_record_counts_nonfinite_frames_apart():
    p = np.array([0.5, 0.9, 0.2], np.float32)
    t = np.array([0.5, np.nan, 0.1], np.float32)
    r = CT.summarize_record(record(p, t))
    assert r["frames"] == 3 and r["finite_frames"] == 2 and all(np.isfinite(r[k]) for k in ("bce", "mse", "mae", "pearson", "worst"))
    assert r["confusion"].sum() == 2 and r["bin_agreement"] == 1.0


def test_summarize_record_zero_variance_and_empty():
    # every value the same: no correlation is defined, whatever the rounding of the sums left
    for n in (1, 3, 1000):
        r = CT.summarize_record(record(np.full(n, 0.3, np.float32), np.linspace(0.1, 0.9, n).astype(np.float32)))
        assert np.isnan(r["pearson"]) and np.isfinite(r["bce"]) and r["finite_frames"] == n
        r = CT.summarize_record(record(np.linspace(0.1, 0.9, n).astype(np.float32), np.full(n, 0.7, np.float32)))
        assert np.isnan(r["pearson"])
    empty = np.zeros(cvlib.CRITIC_SCORE_STATE_DOUBLES)
    empty[10] = -np.inf                                          # what cvae_critic_score_init writes
    r = CT.summarize_record(empty)
    assert r["frames"] == 0 and r["finite_frames"] == 0 and not r["confusion"].any()
    for k in ("bce", "mse", "mae", "loss", "pearson", "bin_agreement", "mean_pred", "mean_target", "worst"):
        assert np.isnan(r[k]), k
    # frames seen, none finite
    empty[0] = 4
    r = CT.summarize_record(empty)
    assert r["frames"] == 4 and r["finite_frames"] == 0 and np.isnan(r["loss"])


def test_split_of_a_critic_dataset_source():
    """critic_dataset's source: (trajectory, frame) in DRAWN order, trajectories interleaved; the split holds whole ones out."""
    src = E.critic_dataset_indices([30, 12, 50, 8, 21], None, seed=4)
    tr, va, taken = E.split_indices(src, 0.2, seed=0)
    assert np.array_equal(np.sort(np.concatenate([tr, va])), np.arange(len(src)))
    assert set(src[va, 0].tolist()) == set(taken) and not set(src[tr, 0].tolist()) & set(taken)
    assert len(va) >= 0.2 * len(src) and len(tr) > 0
    assert len(va) == sum([30, 12, 50, 8, 21][k] for k in taken)          # every frame of a held-out trajectory


def test_critic_command_line(capsys):
    for argv, msg in ((["-critic", "--val-fraction", "0.2"], "-critic needs --episodes, --rewards and --save"),
                      (["-critic", "--eval-only", "--episodes", "e", "--rewards", "r"], "--eval-only needs --critic"),
                      (["-critic", "--eval-only", "--critic", "c.pt"], "--eval-only needs --episodes and --rewards"),
                      (["-train", "--eval-only"], "--eval-only belongs to -critic"),
                      (["-critic", "--episodes", "e", "--rewards", "r", "--save", "d", "--keep-best"], "need --val-fraction"),
                      (["-train", "--val-fraction", "0.2"], "belongs to the fused trainer")):
        with pytest.raises(SystemExit):
            T.main(argv)
        assert msg in capsys.readouterr().err, argv
    a = T.build_parser().parse_args(["-critic", "--episodes", "e", "--rewards", "r", "--save", "d", "--val-fraction", "0.2", "--keep-best",
                                     "--patience", "3", "--critic", "c.pt"])
    assert a.critic_mode and a.val_fraction == 0.2 and a.keep_best and a.patience == 3 and a.critic == "c.pt" and not a.eval_only


def test_val_fraction_reaches_the_critic_mode(capsys):
    with pytest.raises(SystemExit):
        T.main(["-critic", "--val-fraction", "0.2"])
    err = capsys.readouterr().err
    assert "-critic needs --episodes, --rewards and --save" in err and "fused trainer" not in err


class _StubCritic:
    def state_dict(self):
        return {"crit.4.bias": torch.zeros(1)}


class _StubTrainer:
    def __init__(self):
        self.best_val, self.val_stale, self.step_count, self.loss, self.critic = None, 0, 0, "bce", _StubCritic()


def _result(loss):
    return dict(loss=loss, bce=loss, mse=0.01, mae=0.05, pearson=0.5, bin_agreement=0.75, worst=0.9, frames=10, finite_frames=10)


def test_critic_validation_log(tmp_path, capsys):
    args = T.build_parser().parse_args(["-critic", "--episodes", "e", "--rewards", "r", "--save", str(tmp_path), "--val-fraction", "0.2",
                                        "--keep-best", "--patience", "2"])
    log, tr = T._CriticValidationLog(args), _StubTrainer()
    stops = []
    for loss in (0.5, float("nan"), 0.4, 0.45, float("inf")):
        tr.step_count += 1
        stops.append(log(tr, _result(loss)))
    assert stops == [False, False, False, False, True] and tr.best_val == 0.4 and tr.val_stale == 2
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("val @ step")]
    assert len(lines) == 5 and [ln.endswith("*") for ln in lines] == [True, False, True, False, False]
    for word in ("bce", "mse", "mae", "pearson", "bin agreement", "10 frames"):
        assert word in lines[0]
    best = os.path.join(str(tmp_path), "best", "critic.pt")
    assert os.path.isfile(best) and list(torch.load(best)) == ["crit.4.bias"]


def test_load_state_dict_accepts_a_state_without_the_validation_keys():
    tr = CT.CriticTrainer.__new__(CT.CriticTrainer)              # no device: only what load_state_dict touches
    n = cvlib.CRITIC_TRAIN_FLOATS
    tr.critic = type("C", (), {"flat": torch.zeros(n - 3)})()
    tr.theta, tr.m, tr.v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
    tr.guarded, tr.guard = False, None
    tr.val_history, tr.best_val, tr.val_stale = [(1, {})], 0.1, 5
    old = {"flat": torch.ones(n - 3), "m": torch.ones(n), "v": torch.ones(n), "step_count": 7, "applied": 7, "skipped": 0}
    tr.load_state_dict(old)
    assert tr.step_count == 7 and tr.val_history == [] and tr.best_val is None and tr.val_stale == 0 and tr.theta[0] == 1
    new = dict(old, val_history=[(3, {"loss": 0.5, "confusion": [[1, 0], [0, 1]]})], best_val=0.5, val_stale=2)
    tr.load_state_dict(new)
    assert tr.val_history == [(3, {"loss": 0.5, "confusion": [[1, 0], [0, 1]]})] and tr.best_val == 0.5 and tr.val_stale == 2


def test_size_queries_and_host_argument_checks():
    """What include/cvae.h documents, and everything cvae_critic_score rejects before it touches a device."""
    lib = cvlib.load()
    header = open(os.path.join(ROOT, "include", "cvae.h")).read()
    cols = int(re.search(r"#define CVAE_CRITIC_SCORE_COLS (\d+)", header).group(1))
    doubles = int(re.search(r"#define CVAE_CRITIC_SCORE_STATE_DOUBLES (\d+)", header).group(1))
    assert cols == cvlib.CRITIC_SCORE_COLS == 8 and doubles == cvlib.CRITIC_SCORE_STATE_DOUBLES == 40
    assert lib.cvae_critic_score_state_bytes() == 8 * doubles and CT.RECORD_DOUBLES == 27 <= doubles
    for name in ("cvae_critic_score_state_bytes", "cvae_critic_score_scratch_bytes", "cvae_critic_score_init", "cvae_critic_score"):
        assert name in cvlib.EXPORTS
    h = cvlib.Handle(64, 4)
    sb = lib.cvae_critic_score_scratch_bytes
    assert sb(h.h, 1) == 32 and sb(h.h, 65536) == 65536 * 32            # independent of the handle's max_batch
    assert sb(h.h, 0) == -1 and sb(h.h, 65537) == -1 and sb(None, 4) == -1
    ok = 4096                                                            # non-null, 16-byte aligned, never dereferenced

    def call(hh=h.h, B=4, frames=ok, targets=ok, n=8, idx=None, params=ok, rows=ok, state=ok, scratch=ok):
        return lib.cvae_critic_score(hh, B, frames, targets, n, idx, params, rows, state, scratch, None)

    EINVAL, EUNSUPPORTED = -1, -2
    assert call(hh=None) == EINVAL
    assert call(B=0) == EINVAL and call(B=65537) == EINVAL and call(B=65537, n=10 ** 6) == EINVAL
    assert call(frames=None) == EINVAL and call(targets=None) == EINVAL and call(params=None) == EINVAL
    assert call(rows=None, state=None) == EINVAL
    assert b"both null" in lib.cvae_last_error()
    assert call(rows=None, scratch=None) == EINVAL                       # the rows would have nowhere to go
    assert call(n=0) == EINVAL and call(B=4, n=3) == EINVAL              # without idx the batch is the first B frames
    assert call(frames=ok + 8) == EINVAL and call(state=ok + 4) == EINVAL and call(rows=ok + 2) == EINVAL
    wide = cvlib.Handle(128, 2)
    assert call(hh=wide.h) == EUNSUPPORTED
    assert b"64x64" in lib.cvae_last_error()
    assert lib.cvae_critic_score_init(h.h, None, None) == EINVAL and lib.cvae_critic_score_init(None, ok, None) == EINVAL
