"""The loop that FusedTrainer.fit_device and CriticTrainer.fit_device share (critic_vae_amd/fit.py), driven on the CPU with a
stub trainer and a stub dataset that record what happens: the slices, the one shuffle per epoch, when validation runs, the
early stop, the argument checks and the shared part of the trainer state."""
import numpy as np
import pytest
import torch

from critic_vae_amd.fit import DeviceTrainer

N, B, EPOCHS = 5, 2, 2                                      # slices of 2, 2 and 1 per epoch
RESULT = {"loss": 0.5}


class _Dataset:
    def __init__(self, events):
        self.events = events

    def __len__(self):
        return N

    def gather(self, h, nb, idx, x, pred):
        assert nb == idx.numel() == x.shape[0] == pred.shape[0]
        self.events.append(("gather", idx.tolist()))


class _Trainer(DeviceTrainer):
    def __init__(self, guarded=False):
        self._init_shared(guarded, None)
        self.h, self.m, self.events = None, torch.zeros(4), []

    def evaluate(self, val, batch_size):
        self.events.append(("validate", self.step_count, val, batch_size))
        return RESULT

    def batch(self, x, pred):
        self.step_count += 1
        self.events.append(("step", self.step_count, x.shape[0]))
        return self.step_count

    def fit(self, **kw):
        return self._fit(_Dataset(self.events), B, EPOCHS, kw.pop("shuffle", False), torch.empty(B, 3), torch.empty(B, 1), self.batch, **kw)

    def of(self, kind):
        return [e[1] for e in self.events if e[0] == kind]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_unshuffled_slices_and_no_draw():
    np.random.seed(11)
    before = np.random.get_state()
    tr = _Trainer()
    assert tr.fit(shuffle=False) == 6
    assert tr.of("gather") == [[0, 1], [2, 3], [4]] * 2
    assert [e[1:] for e in tr.events if e[0] == "step"] == [(1, 2), (2, 2), (3, 1), (4, 2), (5, 2), (6, 1)]
    assert [e[0] for e in tr.events] == ["gather", "step"] * 6              # the gather comes before its step
    assert _same_state(before, np.random.get_state())
    assert tr.val_history == [] and tr.of("validate") == []


def test_one_shuffle_per_epoch():
    rs = np.random.RandomState(3)
    want = []
    for _ in range(EPOCHS):
        idx = np.arange(N)
        rs.shuffle(idx)
        want += [idx[b:b + B].tolist() for b in range(0, N, B)]
    np.random.seed(3)
    tr = _Trainer()
    tr.fit(shuffle=True)
    assert tr.of("gather") == want
    assert _same_state(rs.get_state(), np.random.get_state())              # exactly one draw per epoch


@pytest.mark.parametrize("val_every, at", [(2, [2, 4, 6]), (None, [3, 6])])
def test_validation_schedule(val_every, at):
    tr, val, seen = _Trainer(), object(), []
    tr.fit(val=val, val_every=val_every, val_batch=7, on_val=lambda trainer, r: seen.append((trainer, r)))
    assert [e[1:] for e in tr.events if e[0] == "validate"] == [(t, val, 7) for t in at]
    assert tr.val_history == [(t, RESULT) for t in at]
    assert seen == [(tr, RESULT)] * len(at) and len(tr.of("gather")) == 6
    for t in at:                                                            # right after step t, before the next gather
        k = tr.events.index(("validate", t, val, 7))
        assert tr.events[k - 1][:2] == ("step", t) and (k + 1 == len(tr.events) or tr.events[k + 1][0] == "gather")


@pytest.mark.parametrize("val_every, last", [(2, 2), (None, 3)])
def test_on_val_ends_the_fit(val_every, last):
    tr = _Trainer()
    assert tr.fit(val=object(), val_every=val_every, val_batch=B, on_val=lambda trainer, r: True) == last
    assert tr.step_count == last and len(tr.of("gather")) == last and tr.events[-1][:2] == ("validate", last)
    assert tr.val_history == [(last, RESULT)]


def test_bad_arguments():
    with pytest.raises(ValueError, match="val_every 0"):
        _Trainer().fit(val=object(), val_every=0)
    with pytest.raises(ValueError, match="need val"):
        _Trainer().fit(val_every=2)
    with pytest.raises(ValueError, match="need val"):
        _Trainer().fit(on_val=lambda trainer, r: False)


def test_shared_state_round_trip():
    tr = _Trainer()
    tr.step_count, tr.best_val, tr.val_stale = 4, 0.25, 1
    tr.val_history = [(4, {"loss": 0.25, "confusion": np.eye(2, dtype=np.int64), "per_frame": torch.zeros(3, 8)})]
    sd = tr._shared_state()
    assert sd == {"step_count": 4, "applied": 4, "skipped": 0, "best_val": 0.25, "val_stale": 1,
                  "val_history": [(4, {"loss": 0.25, "confusion": [[1, 0], [0, 1]]})]}
    assert "per_frame" in tr.val_history[0][1]                              # the trainer's own history keeps its rows
    back = _Trainer()
    back._load_shared_state(sd)
    assert (back.step_count, back.best_val, back.val_stale, back.val_history) == (4, 0.25, 1, sd["val_history"])
    back._load_shared_state({"step_count": 7, "applied": 7, "skipped": 0})  # a state from before validation existed
    assert (back.step_count, back.val_history, back.best_val, back.val_stale) == (7, [], None, 0)


def test_unguarded_trainer_refuses_a_state_that_skipped():
    skipped = {"step_count": 7, "applied": 5, "skipped": 2}
    tr = _Trainer()
    with pytest.raises(ValueError, match="cannot continue it"):
        tr._load_shared_state(skipped)
    assert tr.step_count == 0                                               # refused before anything changed
    guarded = _Trainer(guarded=True)
    guarded._load_shared_state(skipped)
    assert guarded.step_count == 7 and guarded.guard_stats() == dict(applied=5, skipped=2, norm=0.0, coef=1.0)
    assert (guarded._shared_state()["applied"], guarded._shared_state()["skipped"]) == (5, 2)
