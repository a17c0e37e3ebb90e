"""The optimizer options without a GPU: optim.Optim's host arithmetic against its closed forms in float64, decay_ranges on a
hand-written layout, the command line's flags, the trainers' checkpoint of the options, and the argument checks of
cvae_adam_step_opt / cvae_adam_step_guarded_opt (every call here fails them, so nothing is launched)."""
import ctypes as C
import math

import pytest
import torch

from critic_vae_amd import lib as cvlib
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.optim import Optim, critic_layout, decay_ranges
from critic_vae_amd.train import FusedTrainer, build_parser, load_trainer, optim_from_kwargs, optim_kwargs_from_args, save_trainer

FAKE = 4096                                  # a non-null "device address": never dereferenced, every call below fails its checks first
LR, WARMUP, TOTAL, LR_MIN = 3e-4, 5, 23, 2e-5
EDGES = (0, WARMUP - 1, WARMUP, TOTAL - 1, TOTAL, TOTAL + 1)


def closed_form(schedule, step, lr=LR, warmup=WARMUP, total=TOTAL, lr_min=LR_MIN):
    if step < warmup:
        return lr * (step + 1) / warmup
    if schedule == "constant":
        return lr
    if step >= total:
        return lr_min
    if schedule == "linear":
        return lr + (lr_min - lr) * ((step - warmup) / (total - warmup))
    return lr_min + (lr - lr_min) * 0.5 * (1 + math.cos(math.pi * (step - warmup) / (total - warmup)))


@pytest.mark.parametrize("schedule", ["constant", "linear", "cosine"])
def test_lr_at_is_the_closed_form(schedule):
    o = Optim(schedule=schedule, warmup=WARMUP, total=TOTAL, lr_min=LR_MIN)
    for step in list(EDGES) + list(range(TOTAL + 3)):
        assert o.lr_at(step, LR) == closed_form(schedule, step), (schedule, step)
    after = [o.lr_at(s, LR) for s in range(WARMUP, TOTAL + 3)]
    assert all(a >= b for a, b in zip(after, after[1:])), "the rate rises after the warm-up"
    assert o.lr_at(WARMUP, LR) == LR and o.lr_at(0, LR) == LR / WARMUP
    if schedule != "constant":
        assert o.lr_at(TOTAL, LR) == LR_MIN == o.lr_at(TOTAL + 1, LR) and o.lr_at(TOTAL - 1, LR) > LR_MIN


def test_constant_without_warmup_returns_lr_itself():
    lr = 1.2345e-4
    o = Optim()
    assert all(o.lr_at(s, lr) is lr for s in (0, 1, 10 ** 9))
    a = o.args_at(7, lr, [(0, 4)])
    assert a == {"lr": lr, "decay_mul": 1.0, "ema_omd": 0.0, "ranges": []}      # nothing decays: no range travels


def test_ema_decay_at():
    assert Optim().ema_decay_at(3) is None
    o = Optim(ema=0.999)
    assert [o.ema_decay_at(s) for s in (0, 1, 10 ** 6)] == [0.999] * 3
    w = Optim(ema=0.999, ema_warmup=True)
    for s in (0, 1, 8, 8990, 8991, 8992, 10 ** 6):
        assert w.ema_decay_at(s) == min(0.999, (1 + s) / (10 + s)), s
    assert w.ema_decay_at(0) == 0.1 and w.ema_decay_at(10 ** 6) == 0.999


def test_args_at_rounds_as_the_header_says():
    o = Optim(schedule="cosine", warmup=2, total=9, lr_min=1e-6, weight_decay=0.05, ema=0.99, ema_warmup=True)
    for s in (0, 1, 2, 5, 8, 9):
        a = o.args_at(s, LR, [(1, 2), (8, 40)])
        lr_s = o.lr_at(s, LR)
        assert a["lr"] == lr_s and a["ranges"] == [(1, 2), (8, 40)]
        assert a["decay_mul"] == C.c_float(1.0 - lr_s * 0.05).value and 0.0 < a["decay_mul"] < 1.0
        assert a["ema_omd"] == C.c_float(1.0 - o.ema_decay_at(s)).value
    packed = cvlib.Handle._opt(o.args_at(3, LR, [(1, 2), (8, 40)]))
    assert isinstance(packed, cvlib.OptArgs) and packed.n_ranges == 2 and packed.reserved == 0
    assert (packed.begin[0], packed.end[0], packed.begin[1], packed.end[1]) == (1, 2, 8, 40)
    assert C.sizeof(cvlib.OptArgs) == 16 + 2 * 8 * cvlib.OPT_MAX_RANGES
    with pytest.raises(ValueError, match="17"):
        o.args_at(0, LR, [(k, k + 1) for k in range(17)])
    with pytest.raises(ValueError, match="weight_decay"):
        Optim(weight_decay=1e5).args_at(0, LR)               # 1 - lr * wd <= 0


@pytest.mark.parametrize("kw, word", [(dict(schedule="step"), "'step'"), (dict(warmup=-1), "-1"), (dict(warmup=1.5), "1.5"),
                                      (dict(schedule="cosine"), "None"), (dict(schedule="linear", warmup=4, total=4), "4"),
                                      (dict(schedule="cosine", warmup=4, total=3), "3"), (dict(total=2, warmup=3), "2"),
                                      (dict(lr_min=-1e-6), "-1e-06"), (dict(lr_min=float("nan")), "nan"),
                                      (dict(weight_decay=-0.1), "-0.1"), (dict(weight_decay=float("inf")), "inf"),
                                      (dict(ema=1.0), "1.0"), (dict(ema=-0.1), "-0.1"), (dict(ema=float("nan")), "nan"),
                                      (dict(ema_warmup=True), "ema_warmup"), (dict(ema=0.9, ema_warmup="yes"), "'yes'")])
def test_bad_arguments_raise_with_the_value(kw, word):
    with pytest.raises(ValueError) as e:
        Optim(**kw)
    assert word in str(e.value), str(e.value)


def test_bad_steps_and_a_floor_above_the_peak():
    o = Optim(schedule="linear", total=4, lr_min=1e-3)
    with pytest.raises(ValueError, match="-1"):
        o.lr_at(-1, LR)
    with pytest.raises(ValueError, match="lr_min"):
        o.lr_at(1, 1e-4)
    with pytest.raises(ValueError):
        o.ema_decay_at(-2)


def test_state_dict_round_trip_and_equality():
    o = Optim(schedule="cosine", warmup=3, total=50, lr_min=1e-6, weight_decay=0.01, ema=0.995, ema_warmup=True)
    back = Optim().load_state_dict(o.state_dict())
    assert back == o and back is not o and repr(back) == repr(o) and back != Optim() and o != "cosine"
    assert Optim.from_state_dict(o.state_dict()) == o
    assert all(back.lr_at(s, LR) == o.lr_at(s, LR) and back.ema_decay_at(s) == o.ema_decay_at(s) for s in range(60))
    line = o.describe()
    assert "\n" not in line and "cosine" in line and "0.995" in line and "0.01" in line
    assert "no EMA" in Optim().describe()
    with pytest.raises(ValueError):
        Optim().load_state_dict(dict(o.state_dict(), schedule="step"))


def test_decay_ranges_on_an_unaligned_layout():
    layout = {"enc0.w": (0, 7), "enc0.b": (7, 3), "enc0.gamma": (10, 3), "enc0.beta": (13, 3), "fc.w": (21, 9), "fc.b": (30, 2),
              "dec0.w": (33, 5), "dec0.b": (38, 1), "decin.w": (16, 5), "decin.b": (39, 2),
              "features.0.weight": (41, 6), "features.0.bias": (47, 2), "crit.4.weight": (50, 1), "empty.w": (60, 0)}
    got = decay_ranges(layout)
    assert got == [(0, 7), (16, 21), (21, 30), (33, 38), (41, 47), (50, 51)]
    assert got == sorted(got) and all(a[1] <= b[0] for a, b in zip(got, got[1:])) and all(b < e for b, e in got)
    names = {n for n, (off, k) in layout.items() if (off, off + k) in got}
    assert names == {"enc0.w", "decin.w", "fc.w", "dec0.w", "features.0.weight", "crit.4.weight"}
    with pytest.raises(ValueError, match="overlap"):
        decay_ranges({"a.w": (0, 8), "b.w": (4, 8)})


def test_decay_ranges_of_the_two_trainers():
    h = cvlib.Handle(64, 8)
    vae = decay_ranges(h.layout)
    weights = sorted(n for n in h.layout if n.endswith(".w"))
    assert weights == sorted([f"enc{l}.w" for l in range(4)] + ["fc.w"] + [f"dec{i}.w" for i in range(5)] + ["decin.w"])
    assert vae == sorted((h.layout[n][0], sum(h.layout[n])) for n in weights) and len(vae) == 11 <= cvlib.OPT_MAX_RANGES
    assert all(e <= h.param_total for _, e in vae)
    lay = critic_layout()
    crit = decay_ranges(lay)
    assert len(crit) == 7 and sum(n for _, n in lay.values()) == 11873 == h.lib.cvae_critic_param_count()
    assert crit[0] == (0, 216) and crit[1] == (224, 224 + 576) and crit[-1] == (11840, 11872)      # biases lie between them
    assert any(e % 256 for _, e in crit)                   # boundaries inside a wave's 256-element span: the per-element test decides there


def test_parser_has_the_flags(tmp_path, monkeypatch):
    from critic_vae_amd import train
    ap = build_parser()
    a = ap.parse_args(["-train", "--lr-schedule", "cosine", "--lr-warmup", "100", "--lr-min", "1e-6", "--lr-total", "5000",
                       "--weight-decay", "0.01", "--ema", "0.999", "--ema-warmup"])
    kw = optim_kwargs_from_args(a)
    assert kw == {"schedule": "cosine", "warmup": 100, "lr_min": 1e-6, "total": 5000, "weight_decay": 0.01, "ema": 0.999,
                  "ema_warmup": True}
    assert optim_from_kwargs(kw, 77) == Optim(schedule="cosine", warmup=100, total=5000, lr_min=1e-6, weight_decay=0.01, ema=0.999,
                                              ema_warmup=True)
    assert optim_kwargs_from_args(ap.parse_args(["-train"])) is None and optim_from_kwargs(None, 5) is None
    assert optim_from_kwargs({"schedule": "linear"}, 640).total == 640          # --lr-total's default: the length of the run
    seen = {}
    monkeypatch.setattr(train, "_train_episodes", lambda args: seen.setdefault("args", args))
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth", "--ema", "0.99"])
    assert seen["args"].optim_kw == {"ema": 0.99}
    seen.clear()
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth"])
    assert seen["args"].optim_kw is None
    for argv in (["-train", "--weight-decay", "0.1"],                            # the torch-Adam loop takes none of them
                 ["-train", "--episodes", str(tmp_path), "--critic", "synth", "--ema", "1.5"],
                 ["-train", "--episodes", str(tmp_path), "--critic", "synth", "--ema-warmup"],
                 ["-train", "--episodes", str(tmp_path), "--critic", "synth", "--lr-schedule", "cosine", "--lr-warmup", "9", "--lr-total", "9"]):
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2, argv


def test_a_floor_above_the_peak_is_refused_at_the_start(capsys):
    """lr_min above the run's lr: a ValueError at construction and an argument error of the command line before the first
    step, not a ValueError after the warm-up."""
    from critic_vae_amd import train
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    bad = Optim(schedule="cosine", warmup=50, total=100, lr_min=1e-2)
    with pytest.raises(ValueError, match="lr_min"):
        FusedTrainer(vae, lr=1e-4, optim=bad)
    FusedTrainer(vae, lr=1e-1, optim=bad)
    FusedTrainer(vae, lr=1e-4, optim=Optim(lr_min=1e-2))                      # a constant schedule never reads lr_min
    assert Optim(schedule="linear", total=4, lr_min=1e-4).check_lr(1e-4).lr_at(0, 1e-4) == 1e-4
    args = build_parser().parse_args(["-train", "--lr-schedule", "cosine", "--lr-min", "0.5", "--lr-warmup", "50", "--batch", "8"])
    args.optim_kw, args.epochs = optim_kwargs_from_args(args), 1

    class Stand:
        lr, optim = 1e-4, None

    with pytest.raises(SystemExit, match="lr_min"):
        train._settle_optim(args, Stand(), None, 4000, None)


def test_trainer_takes_and_checkpoints_the_options(tmp_path):
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    with pytest.raises(ValueError, match="optim"):
        FusedTrainer(vae, optim="cosine")
    plain = FusedTrainer(vae)
    assert plain.optim is None and not plain.has_ema() and "optim" not in plain.state_dict()
    o = Optim(schedule="linear", warmup=2, total=9, weight_decay=0.02, ema=0.9)
    tr = FusedTrainer(vae, optim=o)
    assert tr.has_ema() and tr.ema is None and tr.aux_ema is None            # created by the first update, not at construction
    assert tr.decay_ranges == decay_ranges(vae.handle.layout)
    sd = tr.state_dict()
    assert sd["optim"] == o.state_dict() and "ema" not in sd and "aux_ema" not in sd
    g = torch.Generator().manual_seed(3)
    tr.ema = torch.randn(tr.m.numel(), generator=g)
    tr.aux_ema = torch.randn(vae.bn_state.numel(), generator=g)
    tr.step_count = 5
    path = save_trainer(tr, str(tmp_path / "trainer.pt"))
    other = load_trainer(FusedTrainer(VariationalAutoencoder(max_batch=2, seed=1)), path)      # built without: the state's options win
    assert other.optim == o and other.optim is not o and other.step_count == 5
    assert torch.equal(other.ema, tr.ema) and torch.equal(other.aux_ema, tr.aux_ema) and other.ema is not tr.ema
    kept = FusedTrainer(vae, optim=Optim(ema=0.5))
    kept.load_state_dict(plain.state_dict())                                  # a state without options keeps the trainer's own
    assert kept.optim == Optim(ema=0.5)
    with pytest.raises(ValueError, match="averaged"):
        FusedTrainer(vae).load_state_dict(dict(sd, ema=torch.zeros(8)))
    fresh = FusedTrainer(vae)
    with pytest.raises(ValueError, match="2.0"):                              # raises before it changes anything
        fresh.load_state_dict(dict(sd, step_count=3, applied=3, optim=dict(sd["optim"], ema=2.0)))
    assert fresh.optim is None and fresh.step_count == 0


# ---- every CVAE_EINVAL case of the two entries: refused, message set, nothing touched ----
def _refused(rc, *words):
    msg = cvlib.load().cvae_last_error().decode()
    assert rc == -1, rc                      # CVAE_EINVAL
    assert all(w in msg for w in words), msg


def _calls(h, n=64, opt="default", ema=FAKE, aux=FAKE, aux_ema=FAKE, n_aux=8, ptrs=None, step=1, hh="default"):
    """Both entries with the same arguments: (name, call) each; call() returns the code (cvae_last_error is the last call's)."""
    if opt == "default":
        opt = cvlib.opt_args(0.999, 0.01, [(1, 2), (3, 9)])
    ref = None if opt is None else C.byref(opt)
    p = ptrs or [FAKE] * 5                   # params, grads, exp_avg, exp_avg_sq, guard state
    hh = h.h if hh == "default" else hh
    lib = h.lib
    return [("cvae_adam_step_opt", lambda: lib.cvae_adam_step_opt(hh, p[0], p[1], p[2], p[3], n, step, 1e-4, 0.9, 0.999, 1e-8, 1.0, ref,
                                                          ema, aux, aux_ema, n_aux, None)),
            ("cvae_adam_step_guarded_opt", lambda: lib.cvae_adam_step_guarded_opt(hh, p[0], p[1], p[2], p[3], n, 1e-8, p[4], ref, ema, aux,
                                                                          aux_ema, n_aux, None))]


def _all_refused(results, *words):
    for name, call in results:
        _refused(call(), name, *words)


@pytest.fixture(scope="module")
def h():
    return cvlib.Handle(64, 8)


@pytest.mark.parametrize("n", [1, 6, 4095, -4])
def test_opt_calls_refuse_a_length_that_is_no_multiple_of_4(h, n):
    _all_refused(_calls(h, n=n, opt=cvlib.opt_args()), str(n))


def test_opt_calls_refuse_a_null_opt_and_null_buffers(h):
    _all_refused(_calls(h, opt=None), "opt")
    for k in range(4):
        ptrs = [FAKE] * 5
        ptrs[k] = None
        _all_refused(_calls(h, ptrs=ptrs))
    _all_refused(_calls(h, hh=None))
    _all_refused(_calls(h, ptrs=[FAKE] * 4 + [None])[1:])
    _all_refused(_calls(h, step=0)[:1], "step")


@pytest.mark.parametrize("n_ranges", [-1, 17, 1 << 20])
def test_opt_calls_refuse_a_bad_range_count(h, n_ranges):
    opt = cvlib.opt_args()
    opt.n_ranges = n_ranges
    _all_refused(_calls(h, opt=opt), "n_ranges", str(n_ranges))


@pytest.mark.parametrize("ranges", [[(5, 5)], [(9, 3)], [(8, 12), (0, 4)], [(0, 8), (7, 12)], [(0, 4), (60, 65)], [(64, 68)],
                                    [(-1, 3)], [(0, 4), (4, 8), (6, 9)]])
def test_opt_calls_refuse_bad_ranges(h, ranges):
    _all_refused(_calls(h, opt=cvlib.opt_args(0.99, 0.0, ranges)), "range")


def test_opt_calls_take_touching_ranges_up_to_n_as_valid_arguments(h):
    """[(0, 4), (4, 64)] is ascending and disjoint: the range check passes and the NEXT check (a bad decay_mul here) answers."""
    _all_refused(_calls(h, opt=cvlib.opt_args(2.0, 0.0, [(0, 4), (4, 64)])), "decay_mul")


@pytest.mark.parametrize("decay_mul", [0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")])
def test_opt_calls_refuse_a_bad_decay_mul(h, decay_mul):
    _all_refused(_calls(h, opt=cvlib.opt_args(decay_mul, 0.0)), "decay_mul")


@pytest.mark.parametrize("omd", [-1e-3, 1.0000001, float("nan"), float("inf")])
def test_opt_calls_refuse_a_bad_ema_omd_only_when_ema_is_given(h, omd):
    _all_refused(_calls(h, opt=cvlib.opt_args(1.0, omd)), "ema_omd")
    _all_refused(_calls(h, opt=cvlib.opt_args(1.0, omd), ema=None, aux=None, aux_ema=None, n_aux=-1), "n_aux")      # not read: the next check answers


@pytest.mark.parametrize("n_aux", [-1, 4097, 1 << 30])
def test_opt_calls_refuse_a_bad_n_aux(h, n_aux):
    _all_refused(_calls(h, n_aux=n_aux), "n_aux", str(n_aux))


def test_opt_calls_refuse_inconsistent_aux_pointers(h):
    _all_refused(_calls(h, aux=None), "aux")
    _all_refused(_calls(h, aux_ema=None), "aux")
    _all_refused(_calls(h, ema=None), "aux_ema without ema")
    _all_refused(_calls(h, ema=None, aux=None, n_aux=0), "aux_ema without ema")


def test_binding_refuses_more_ranges_than_the_table_holds():
    with pytest.raises(ValueError, match="17"):
        cvlib.opt_args(0.9, 0.0, [(k, k + 1) for k in range(17)])
    for name in ("cvae_adam_step_opt", "cvae_adam_step_guarded_opt"):
        assert name in cvlib.EXPORTS and hasattr(cvlib.load(), name)
