"""Held-out validation without a GPU: the index logic of episodes.split_by_trajectory on hand-built source arrays, the size
queries of the score entry points against what include/cvae.h documents, and the command-line options."""
import os
import re

import numpy as np
import pytest

from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(lengths, ids=None, cols=2):
    """Rows (trajectory, frame[, kind]) of trajectories `ids` with `lengths` entries each, in dataset order."""
    ids = list(range(len(lengths))) if ids is None else ids
    traj = np.repeat(np.asarray(ids, np.int64), lengths)
    frame = np.concatenate([np.arange(n, dtype=np.int64) for n in lengths])
    return np.stack([traj, frame] + [np.zeros_like(traj)] * (cols - 2), 1)


def split(src, fraction, seed=0):
    if not hasattr(E, "split_indices"):
        pytest.fail("episodes has no split_indices / split_by_trajectory: no held-out set can be made")
    return E.split_indices(src, fraction, seed)


@pytest.mark.parametrize("cols", [2, 3])
@pytest.mark.parametrize("fraction", [0.1, 0.25, 0.5])
def test_split_holds_out_whole_trajectories(fraction, cols):
    lengths = [10, 20, 5, 15, 1, 30, 7]
    src = source(lengths, ids=[3, 0, 9, 4, 7, 1, 12], cols=cols)
    for seed in range(5):
        tr, va, taken = split(src, fraction, seed)
        assert np.array_equal(np.sort(np.concatenate([tr, va])), np.arange(len(src)))      # a partition, ...
        assert np.all(np.diff(tr) > 0) and np.all(np.diff(va) > 0)                           # ... each half in dataset order
        t_tr, t_va = set(src[tr, 0].tolist()), set(src[va, 0].tolist())
        assert not (t_tr & t_va) and t_va == set(taken)
        assert len(va) >= fraction * len(src) and len(tr) > 0                               # honoured from above
        # ... and minimal: without the last trajectory taken in the seeded order, val would fall short
        order = np.random.default_rng(seed).permutation(len(lengths))
        ids_sorted, per = np.unique(src[:, 0], return_counts=True)
        n, k = 0, 0
        while n < fraction * len(src):
            n += per[order[k]]
            k += 1
        assert sorted(ids_sorted[order[:k]].tolist()) == taken and n == len(va)


def test_split_is_deterministic_in_the_seed():
    src = source([4, 9, 3, 8, 6, 5, 7, 2])
    a, b = split(src, 0.3, seed=5), split(src, 0.3, seed=5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert len({tuple(split(src, 0.3, seed=s)[2]) for s in range(12)}) > 1          # and the seed matters


def test_split_rejects_the_degenerate_cases():
    with pytest.raises(ValueError):
        split(source([12]), 0.5)                      # one trajectory
    with pytest.raises(ValueError):
        split(source([12], ids=[4]), 0.2)
    with pytest.raises(ValueError):
        split(source([5, 5]), 0.9)                    # both trajectories would go: no training entry
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            split(source([5, 5, 5]), bad)


def test_size_queries_return_what_the_header_documents():
    lib = cvlib.load()
    header = open(os.path.join(ROOT, "include", "cvae.h")).read()
    cols = int(re.search(r"#define CVAE_SCORE_COLS (\d+)", header).group(1))
    doubles = int(re.search(r"#define CVAE_SCORE_STATE_DOUBLES (\d+)", header).group(1))
    assert cols == 8 and lib.cvae_score_cols() == cols == cvlib.SCORE_COLS
    assert lib.cvae_score_state_bytes() == 8 * doubles == 8 * cvlib.SCORE_STATE_DOUBLES
    assert doubles >= 18                               # 11 sums, 2 counts, 4 sums, 1 maximum


def test_command_line_options_parse():
    ap = T.build_parser()
    a = ap.parse_args(["-train", "--episodes", "e", "--critic", "synth", "--val-fraction", "0.2", "--val-every", "50", "--keep-best",
                       "--patience", "3", "--save", "out"])
    assert a.val_fraction == 0.2 and a.val_every == 50 and a.keep_best and a.patience == 3
    d = ap.parse_args(["-second", "--dataset", "d.npz", "--critic", "synth"])
    assert d.val_fraction is None and d.val_every is None and not d.keep_best and d.patience is None
    for argv in (["-train", "--episodes", "e", "--critic", "synth", "--val-every", "5"],                      # needs --val-fraction
                 ["-train", "--episodes", "e", "--critic", "synth", "--val-fraction", "1.5"],
                 ["-train", "--episodes", "e", "--critic", "synth", "--val-fraction", "0.2", "--keep-best"],   # needs --save
                 ["-train", "--val-fraction", "0.2"]):                                                       # the synthetic loop has no trainer
        with pytest.raises(SystemExit):
            T.main(argv)


def test_subset_bookkeeping_stays_consistent():
    """names / sizes / counts of both halves: visited trajectories in order, sizes = entries before each in the half; a visited
    trajectory that contributed no entry (index 1 here) is in neither; a ReconDataset's 3-column source goes through."""
    if not hasattr(E, "subset_meta"):
        pytest.fail("episodes has no subset_meta: the halves of a split carry no names / sizes / counts")
    lengths = [4, 0, 3, 5]                                     # walk order; trajectory ids below
    ids, names = [7, 2, 9, 4], ["a", "empty", "c", "d"]
    src = source([n for n in lengths if n], ids=[i for i, n in zip(ids, lengths) if n], cols=3)
    src[:, 2] = np.arange(len(src)) % 2
    sizes = [0, 4, 4, 7]
    counts = np.array([[1, 2, 1], [0, 0, 0], [3, 0, 0], [2, 2, 1]], np.int64)
    tr, va, taken = split(src, 0.3, seed=1)
    halves = [E.subset_meta(src, names, sizes, counts, rows) for rows in (tr, va)]
    seen = []
    for rows, (s, n, z, c) in zip((tr, va), halves):
        assert np.array_equal(s, src[rows]) and s.shape[1] == 3
        assert len(n) == len(z) == len(c) and "empty" not in n
        for j, name in enumerate(n):
            t = ids[names.index(name)]
            end = z[j + 1] if j + 1 < len(z) else len(s)
            assert end > z[j] and np.all(s[z[j]:end, 0] == t)                      # its entries, and only they, start at sizes[j]
            assert end - z[j] == lengths[names.index(name)] and np.array_equal(c[j], counts[names.index(name)])
        assert [names.index(k) for k in n] == sorted(names.index(k) for k in n)   # walk order kept
        seen += n
    assert sorted(seen) == ["a", "c", "d"]
    assert {ids[names.index(k)] for k in halves[1][1]} == set(taken)


class _StubTrainer:
    def __init__(self):
        self.best_val, self.val_stale, self.step_count, self.vae = None, 0, 0, object()


def _result(loss):
    return dict(total_loss=loss, recon_loss=loss, KLD=0.0, images=10, finite_images=10, mean_total=loss, worst=loss, psnr=20.0)


def test_validation_log_keeps_the_best_and_stops_on_patience(monkeypatch, capsys):
    if not hasattr(T, "_ValidationLog"):
        pytest.fail("train has no _ValidationLog: --keep-best / --patience do nothing")
    saved = []
    monkeypatch.setattr(T, "save_networks", lambda vae, directory, second=False: saved.append((directory, second)))
    args = T.build_parser().parse_args(["-second", "--dataset", "d", "--critic", "synth", "--val-fraction", "0.2", "--keep-best",
                                        "--patience", "2", "--save", "out"])
    log, tr = T._ValidationLog(args, second=True), _StubTrainer()
    stops = []
    for loss in (0.5, float("nan"), 0.4, 0.45, float("inf"), 0.3):
        tr.step_count += 1
        stops.append(log(tr, _result(loss)))
    # 0.5 best; NaN no improvement (stale 1); 0.4 best; 0.45 stale 1; inf stale 2 -> stop; (a caller that went on) 0.3 best again
    assert stops == [False, False, False, False, True, False]
    assert saved == [(os.path.join("out", "best"), True)] * 3 and tr.best_val == 0.3 and tr.val_stale == 0
    assert capsys.readouterr().out.count("val @ step") == 6
    # a non-finite first value is no best value
    tr2 = _StubTrainer()
    assert log(tr2, _result(float("nan"))) is False and tr2.best_val is None and tr2.val_stale == 1
    # without --keep-best nothing is written
    saved.clear()
    args.keep_best = False
    T._ValidationLog(args, False)(_StubTrainer(), _result(0.1))
    assert saved == []
