"""CPU: the augmentation as data (critic_vae_amd/augment.py) — validation and quantisation, the hashed draws and their
coverage, the numpy statement of the pixel rule against hand-checked pixels and against the torch statement the GPU tests
use, the trainer state, the refusals of the trainers and of the command line, and the two new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import augment_tools as AT
from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth
from critic_vae_amd import train as T
from critic_vae_amd.augment import Augment, key
from critic_vae_amd.critic_train import CriticTrainer
from critic_vae_amd.fit import DeviceTrainer
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer, load_trainer, save_trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_validation_and_quantisation():
    a = Augment()
    assert (a.flip, a.shift, a.brightness, a.seed) == (0.0, 0, 0.0, 0) and a.at(0)[1:] == (0, 0, 0)
    assert Augment(flip=0.5).flip_below == 2 ** 23 and Augment(flip=1.0).flip_below == 2 ** 24
    assert Augment(brightness=0.5).gain_q16 == 32768 and Augment(brightness=0.99999999).gain_q16 == 65535
    assert Augment(flip=0.5, shift=2, brightness=0.5, seed=3).at(9) == (key(3, 9), 2 ** 23, 2, 32768)
    for bad in (dict(flip=-0.1), dict(flip=1.1), dict(flip=float("nan")), dict(shift=-1), dict(shift=1.5), dict(shift=True),
                dict(brightness=-0.1), dict(brightness=1.0), dict(brightness=float("nan")), dict(seed=0.5)):
        with pytest.raises(ValueError):
            Augment(**bad)
    with pytest.raises(ValueError):
        Augment().at(-1)
    assert Augment(shift=16).check_width(64).shift == 16 and Augment(shift=32).check_width(128).shift == 32
    with pytest.raises(ValueError, match="width / 4"):
        Augment(shift=17).check_width(64)
    assert "flip" in Augment(flip=0.5).describe() and "stored" in Augment().describe()


def test_key_and_draws_follow_the_definition():
    mix = lambda z: int(synth._mix64(np.uint64(z & (2 ** 64 - 1))))      # noqa: E731
    assert key(0, 0) == mix(0) and key(3, 5) == mix(3 * 0x100000001B3 + 5)
    assert key(-1, 0) == mix((-0x100000001B3) % 2 ** 64)                   # seed * prime reduced mod 2^64
    a = Augment(flip=0.25, shift=3, brightness=0.125, seed=11)
    k, below, S, gain = a.at(4)
    idx = [0, 1, 5, 2 ** 31 + 7, 174762]
    d = a.draws(4, idx)
    assert d.dtype == np.int64 and d.shape == (5, 4)
    for row, s in zip(d, idx):
        r = mix(k ^ mix(s))
        want = [int((r >> 40) < below), ((r >> 12) & 0xFFF) % (2 * S + 1) - S, (r & 0xFFF) % (2 * S + 1) - S,
                gain * (((r >> 24) & 0xFFFF) - 32768)]
        assert row.tolist() == want


def test_draws_are_deterministic_and_depend_on_draw_and_seed():
    idx = np.arange(256)
    a = Augment(flip=0.5, shift=2, brightness=0.5, seed=0)
    d0 = a.draws(0, idx)
    assert np.array_equal(d0, a.draws(0, idx)) and np.array_equal(d0, Augment(flip=0.5, shift=2, brightness=0.5).draws(0, idx))
    assert not np.array_equal(d0, a.draws(1, idx))
    assert not np.array_equal(d0, Augment(flip=0.5, shift=2, brightness=0.5, seed=1).draws(0, idx))
    assert np.array_equal(d0[[3, 3, 200]], a.draws(0, [3, 3, 200]))         # a function of the dataset index, not of the row
    z = Augment().draws(5, idx)
    assert not z.any()                                                      # the all-zero configuration draws nothing


@pytest.mark.parametrize("seed,draw", [(0, 0), (0, 1), (0, 7), (1, 0)])
def test_all_fifty_combinations_in_256_samples(seed, draw):
    d = Augment(flip=0.5, shift=2, seed=seed).draws(draw, np.arange(256))
    assert AT.combinations(d) == AT.all_combinations(2) and len(AT.all_combinations(2)) == 50
    assert abs(d[:, 0].mean() - 0.5) <= 0.1


def test_every_shift_value_occurs_at_sixteen():
    d = Augment(shift=16).draws(0, np.arange(4096))
    for col in (1, 2):
        assert sorted(set(d[:, col].tolist())) == list(range(-16, 17))
    assert np.bincount(d[:, 1] + 16).min() >= 60                            # 4096 / 33 = 124 expected per value


def test_gain_numerator_stays_in_range():
    a = Augment(brightness=0.99999999)
    d = a.draws(0, np.arange(1 << 16))
    num = d[:, 3] + 2 ** 31
    assert a.gain_q16 == 65535 and num.min() >= 1 and num.max() < 2 ** 32
    assert d[:, 3].min() >= -2 ** 31 and d[:, 3].max() < 2 ** 31
    for k in (-32768, 32767):                                               # the extremes of k, whether drawn or not
        assert 1 <= 2 ** 31 + 65535 * k < 2 ** 32 and -2 ** 31 <= 65535 * k < 2 ** 31
    g = Augment.gains(d)
    assert g.dtype == np.float32 and g.min() > 0.0 and g.max() < 2.0
    assert Augment.gains(np.zeros((1, 4), np.int64))[0] == np.float32(1.0)


def _coded(W):
    """uint8 HWC frame whose pixel (row, col) is (row, col, row ^ col)."""
    r, c = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
    return np.stack([r, c, r ^ c], axis=-1).astype(np.uint8)[None]


def test_apply_host_on_a_frame_that_encodes_its_coordinates():
    W, S = 64, 5
    f = _coded(W)
    px = lambda out, i, j: tuple(int(round(float(v) * 255)) for v in out[0, :, i, j])       # noqa: E731
    src = lambda i, j: (i, j, i ^ j)                                                         # noqa: E731
    # flip, dx = +S, dy = -S: out(i, j) = src(clamp(i + S), clamp(W-1-j - S))
    out = Augment.apply_host(f, [[1, S, -S, 0]])
    assert out.shape == (1, 3, W, W) and out.dtype == np.float32
    assert px(out, 0, 0) == src(S, W - 1 - S)
    assert px(out, 0, W - 1) == src(S, 0)                                   # W-1-(W-1) - S = -S, clamped to column 0
    assert px(out, W - 1, 0) == src(W - 1, W - 1 - S)                       # row W-1+S clamped
    assert px(out, W - 1, W - 1) == src(W - 1, 0)
    assert px(out, W - 1 - S, W - 1 - S) == src(W - 1, 0)                   # the last unclamped row / column
    # no flip, dx = -S, dy = +S: out(i, j) = src(clamp(i - S), clamp(j + S))
    out = Augment.apply_host(f, [[0, -S, S, 0]])
    assert px(out, 0, 0) == src(0, S)
    assert px(out, 0, W - 1) == src(0, W - 1)
    assert px(out, W - 1, 0) == src(W - 1 - S, S)
    assert px(out, W - 1, W - 1) == src(W - 1 - S, W - 1)
    assert px(out, S, W - 1 - S) == src(0, W - 1)
    # identity, and the gain with its clamp: g = 1.5 -> 200/255 * 1.5 > 1
    plain = (f.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)
    assert np.array_equal(Augment.apply_host(f, [[0, 0, 0, 0]]), plain)
    g15 = Augment.apply_host(np.full((1, W, W, 3), 200, np.uint8), [[0, 0, 0, 2 ** 30]])
    assert np.all(g15 == np.float32(1.0))
    g05 = Augment.apply_host(np.full((1, W, W, 3), 200, np.uint8), [[0, 0, 0, -2 ** 30]])
    assert np.all(g05 == np.float32(200) / np.float32(255) * np.float32(0.5))


def test_apply_host_on_fp32_entries_copies_bits():
    rng = np.random.default_rng(0)
    f = rng.uniform(-1, 1, size=(3, 3, 64, 64)).astype(np.float32)
    f[0, 0, 0, 0], f[1, 2, 63, 63], f[2, 1, 5, 0] = -0.0, np.nan, -0.0
    d = np.array([[1, 16, -16, 0], [0, -3, 7, 0], [1, 0, 0, 0]])
    out = Augment.apply_host(f, d)
    want = AT.permute(torch.from_numpy(f).view(torch.int32), torch.from_numpy(d)).numpy()
    assert np.array_equal(out.view(np.int32), want)
    assert np.array_equal(out[2].view(np.int32), f[2][:, :, ::-1].view(np.int32))
    with pytest.raises(ValueError, match="gain"):
        Augment.apply_host(f, [[0, 0, 0, 5]] * 3)
    with pytest.raises(ValueError):
        Augment.apply_host(f.astype(np.float64), d)
    with pytest.raises(ValueError):
        Augment.apply_host(f, d[:2])


@pytest.mark.parametrize("W", [64, 128])
def test_numpy_and_torch_statements_agree(W):
    """apply_host (numpy, per frame) against augment_tools.transform (torch, batched indexing): two independent statements of
    the rule, compared bit for bit on every combination of a shift of 2 plus the extreme shifts."""
    rng = np.random.default_rng(W)
    a = Augment(flip=0.5, shift=2, brightness=0.5, seed=0)
    d = a.draws(0, np.arange(64))
    S = W // 4
    d = np.concatenate([d, [[1, S, -S, 123456789], [0, -S, S, -2 ** 31 + 1], [1, -S, -S, 2 ** 31 - 1], [0, S, S, 0]]])
    frames = rng.integers(0, 256, size=(len(d), W, W, 3), dtype=np.uint8)
    plain = (torch.from_numpy(frames).to(torch.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
    got = torch.from_numpy(Augment.apply_host(frames, d))
    assert torch.equal(got.view(torch.int32), AT.transform(plain, torch.from_numpy(d)).view(torch.int32))
    assert np.array_equal(Augment.gains(d), AT.gains(torch.from_numpy(d)).numpy())


def test_state_round_trip_and_equality():
    a = Augment(flip=0.25, shift=3, brightness=0.125, seed=11)
    sd = a.state_dict()
    assert sd == dict(flip=0.25, shift=3, brightness=0.125, seed=11)
    b = Augment.from_state_dict(sd)
    assert b == a and b is not a and b.at(5) == a.at(5) and repr(b) == repr(a)
    assert a != Augment(flip=0.25, shift=3, brightness=0.125, seed=12) and a != Augment() and a != sd
    with pytest.raises(ValueError):
        Augment.from_state_dict(dict(sd, flip=2.0))
    with pytest.raises(KeyError):
        Augment.from_state_dict({"flip": 0.5})


def test_trainers_carry_the_augmentation_and_refuse_what_they_cannot_do(tmp_path):
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    assert FusedTrainer(vae).augment is None and "augment" not in FusedTrainer(vae).state_dict()
    a = Augment(flip=0.5, shift=2, brightness=0.1, seed=4)
    tr = FusedTrainer(vae, augment=a)
    tr.step_count = 3
    path = save_trainer(tr, str(tmp_path / "trainer.pt"))
    tr2 = load_trainer(FusedTrainer(VariationalAutoencoder(max_batch=2, seed=1)), path)
    assert tr2.augment == a and tr2.augment is not a and tr2.augment.at(tr2.step_count) == a.at(3)
    plain = save_trainer(FusedTrainer(vae), str(tmp_path / "plain.pt"))          # a state without one keeps the trainer's own
    assert load_trainer(FusedTrainer(vae, augment=a), plain).augment == a
    with pytest.raises(ValueError, match="fit_u8"):
        tr.fit_u8(np.zeros((2, 64, 64, 3), np.uint8), None, 2)
    with pytest.raises(ValueError, match="width / 4"):
        FusedTrainer(vae, augment=Augment(shift=17))
    with pytest.raises(ValueError, match="Augment"):
        FusedTrainer(vae, augment=(0, 0, 0, 0))
    bad = dict(tr.state_dict(), augment=dict(a.state_dict(), shift=17))
    fresh = FusedTrainer(vae)
    with pytest.raises(ValueError, match="width / 4"):
        fresh.load_state_dict(bad)
    assert fresh.step_count == 0 and fresh.augment is None                       # raised before anything changed
    stub = type("C", (), {"handle": None, "flat": torch.zeros(3)})()
    with pytest.raises(ValueError, match="width / 4"):
        CriticTrainer(stub, augment=Augment(shift=17))
    with pytest.raises(ValueError, match="on the device"):                       # a valid one gets as far as the device check
        CriticTrainer(stub, augment=Augment(shift=16))


class _Recorder(DeviceTrainer):
    """The shared loop on the CPU: a dataset that records how gather was called."""

    def __init__(self, augment, dtype=torch.uint8):
        self._init_shared(False, None)
        self.h, self.m, self.calls = None, torch.zeros(4), []
        self.augment = augment
        self.frames = torch.zeros(1, dtype=dtype)

    def __len__(self):
        return 5

    def gather(self, h, nb, idx, x, pred, **kw):
        self.calls.append((self.step_count, kw))

    def batch(self, x, pred):
        self.step_count += 1

    def fit(self):
        self._fit(self, 2, 2, False, torch.empty(2, 3), torch.empty(2, 1), self.batch)
        return self.calls


def test_fit_loop_passes_the_key_of_the_step_and_nothing_without_an_augmentation():
    assert _Recorder(None).fit() == [(s, {}) for s in range(6)]                  # today's five positional arguments only
    a = Augment(flip=0.5, shift=1, seed=2)
    r = _Recorder(a)
    r.step_count = 10                                                            # a resumed run continues at its step
    assert r.fit() == [(s, {"aug": a.at(s)}) for s in range(10, 16)]
    with pytest.raises(ValueError, match="fp32 entries"):
        _Recorder(Augment(brightness=0.1), dtype=torch.float32).fit()
    assert _Recorder(Augment(flip=0.5, shift=2), dtype=torch.float32).fit()      # flip and shift are fine there
    st = r._shared_state()
    assert st["augment"] == a.state_dict() and "augment" not in _Recorder(None)._shared_state()


def test_command_line(tmp_path, monkeypatch, capsys):
    ap = T.build_parser()
    assert T.augment_from_args(ap.parse_args(["-train"])) is None
    got = T.augment_from_args(ap.parse_args(["-second", "--augment-flip", "0.5", "--augment-shift", "2", "--augment-brightness", "0.1",
                                             "--augment-seed", "7"]))
    assert got == Augment(0.5, 2, 0.1, 7)
    assert T.augment_from_args(ap.parse_args(["-train", "--augment-seed", "3"])) == Augment(seed=3)
    seen = {}
    for fn in ("_train_episodes", "_train_second", "_train_critic"):
        monkeypatch.setattr(T, fn, lambda args, fn=fn: seen.setdefault(fn, args))
    d = str(tmp_path)
    T.main(["-train", "--episodes", d, "--critic", "synth"])
    assert seen.pop("_train_episodes").augment is None
    T.main(["-train", "--episodes", d, "--critic", "synth", "--augment-flip", "0.5", "--augment-brightness", "0.2"])
    assert seen.pop("_train_episodes").augment == Augment(flip=0.5, brightness=0.2)
    T.main(["-second", "--dataset", d, "--critic", "synth", "--augment-shift", "4"])
    assert seen.pop("_train_second").augment == Augment(shift=4)
    T.main(["-critic", "--episodes", d, "--rewards", d, "--save", d, "--augment-flip", "1", "--augment-brightness", "0.3"])
    assert seen.pop("_train_critic").augment == Augment(flip=1.0, brightness=0.3)
    refused = [
        (["-train", "--augment-flip", "0.5"], "gather their batches on the device"),                        # synthetic -train
        (["-dataset", "--episodes", d, "--critic", "synth", "--out", d, "--augment-shift", "1"], "gather their batches"),
        (["-critic", "--eval-only", "--critic", "synth", "--episodes", d, "--rewards", d, "--augment-flip", "0.5"], "gather their"),
        (["-second", "--dataset", d, "--critic", "synth", "--augment-brightness", "0.1"], "-second takes no --augment-brightness"),
        (["-train", "--episodes", d, "--critic", "synth", "--augment-shift", "17"], "width / 4"),
        (["-train", "--episodes", d, "--critic", "synth", "--augment-flip", "1.5"], "probability"),
        (["-train", "--episodes", d, "--critic", "synth", "--augment-brightness", "1"], "brightness"),
    ]
    for argv, word in refused:
        with pytest.raises(SystemExit):
            T.main(argv)
        assert word in capsys.readouterr().err, argv
    assert not seen


def test_resume_keeps_the_checkpoints_augmentation_and_refuses_another(tmp_path, capsys):
    vae = VariationalAutoencoder(max_batch=2, seed=0)
    a = Augment(flip=0.5, shift=2, seed=1)
    with_aug = save_trainer(FusedTrainer(vae, augment=a), str(tmp_path / "a.pt"))
    plain = save_trainer(FusedTrainer(vae), str(tmp_path / "b.pt"))

    def resume(given, path):
        tr = load_trainer(FusedTrainer(vae, augment=given), path)
        T._check_resumed_augment(given, tr, "DIR")
        return tr

    assert resume(None, plain).augment is None and capsys.readouterr().out == ""
    assert resume(None, with_aug).augment == a and "continuing with the augmentation saved in DIR" in capsys.readouterr().out
    assert resume(Augment(flip=0.5, shift=2, seed=1), with_aug).augment == a     # the run's own flags repeated
    other = Augment(flip=0.5, shift=2, seed=2)
    with pytest.raises(SystemExit) as e:
        resume(other, with_aug)
    assert repr(a) in str(e.value) and repr(other) in str(e.value)               # the message names both
    with pytest.raises(SystemExit, match="plain batch gathers"):
        resume(a, plain)


def test_exports_and_declared_signatures():
    lib = cvlib.load()
    header = open(os.path.join(ROOT, "include", "cvae.h")).read()
    m = re.search(r"typedef struct cvae_augment \{(.*?)\} cvae_augment;", header, re.S)
    fields = re.findall(r"(uint64_t|uint32_t|int32_t)\s+(\w+);", m.group(1))
    ctype = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(cvlib.AugmentParams._fields_)
    assert C.sizeof(cvlib.AugmentParams) == 24
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = [p, i32, i32, p, p, i64, p, C.POINTER(cvlib.AugmentParams), p, p, p, p]
    for name in ("cvae_preprocess_u8_gather_aug", "cvae_gather_f32_aug"):
        assert name in cvlib.EXPORTS and hasattr(lib, name)
        decl = re.search(r"int " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(want) and "const cvae_augment* aug" in decl and "int32_t* applied_or_null" in decl
        fn = getattr(lib, name)
        assert fn.restype == C.c_int and list(fn.argtypes) == want
    # a null handle is refused on the host, before any device access
    zero = cvlib.AugmentParams(0, 0, 0, 0, 0)
    assert lib.cvae_preprocess_u8_gather_aug(None, 1, 64, None, None, 1, None, C.byref(zero), None, None, None, None) == -1
    assert lib.cvae_gather_f32_aug(None, 1, 64, None, None, 1, None, C.byref(zero), None, None, None, None) == -1
