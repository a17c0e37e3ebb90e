"""The augmented batch gathers on the MI355X (cvae_preprocess_u8_gather_aug / cvae_gather_f32_aug, dataset.hip): bits
against the plain kernel's own output moved and scaled by torch (augment_tools), `applied` against the host statement
(Augment.draws), single transforms against torch alone, the all-zero configuration, bounds and guard bands, addressing past
2^31 bytes, and the trainers: fit_device with an augmentation against a hand loop, an interrupted run, and evaluate()."""
import numpy as np
import pytest
import torch

import augment_tools as AT
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import params as P
from critic_vae_amd.augment import Augment
from critic_vae_amd.critic import Critic
from critic_vae_amd.critic_train import CriticTrainer, initial_state_dict
from critic_vae_amd.lib import Handle
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 256
FULL = Augment(flip=0.5, shift=2, brightness=0.5, seed=0)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module", params=[64, 128])
def u8set(request):
    """256 random uint8 frames of one width on the device with their plain gather (computed once, never changed)."""
    w = request.param
    rng = np.random.default_rng(w)
    frames = rng.integers(0, 256, size=(N, w, w, 3), dtype=np.uint8)
    preds = rng.random(N).astype(np.float32)
    ds = E.DeviceDataset.from_host(frames, preds)
    h = Handle(w, 64)
    plain = torch.empty(N, 3, w, w, device=DEV)
    ppred = torch.empty(N, 1, device=DEV)
    every = torch.arange(N, dtype=torch.int64, device=DEV)
    for b in range(0, N, 64):
        h.preprocess_u8_gather(64, ds.frames, ds.preds, every[b:b + 64], plain[b:b + 64], ppred[b:b + 64])
    return dict(w=w, ds=ds, h=h, plain=plain, pred=ppred, rng=rng)


def run_u8(s, aug, idx, draw=0):
    """One augmented gather of dataset rows idx -> (x, pred, applied) on the device."""
    B, w = len(idx), s["w"]
    x = torch.full((B, 3, w, w), -3.0, device=DEV)
    pred = torch.full((B, 1), -3.0, device=DEV)
    applied = torch.full((B, 4), -77, dtype=torch.int32, device=DEV)
    s["ds"].gather(s["h"], B, torch.as_tensor(np.asarray(idx, np.int64)).to(DEV), x, pred, aug=aug.at(draw), applied=applied)
    return x, pred, applied


# ---- 1. bits against the host statement ----

def test_bits_against_the_host_statement(u8set):
    s, rng = u8set, np.random.default_rng(1)
    batches = [rng.integers(0, N, size=1), np.array([7, 7, 200, 7, 0]), np.concatenate([rng.integers(0, N, size=30), [5] * 7])]
    batches += [np.arange(b, b + 64) for b in range(0, N, 64)]
    seen = set()
    for idx in batches:
        x, pred, applied = run_u8(s, FULL, idx)
        want = FULL.draws(0, idx)
        assert np.array_equal(applied.cpu().numpy(), want), len(idx)
        d_idx = torch.from_numpy(np.asarray(idx, np.int64)).to(DEV)
        ref = AT.transform(s["plain"][d_idx], applied)            # the plain kernel's output, moved and scaled by torch
        assert torch.equal(bits(x), bits(ref)), len(idx)
        assert torch.equal(bits(pred), bits(s["pred"][d_idx]))
        x2, pred2, applied2 = run_u8(s, FULL, idx)                 # the same call again: the same bits
        assert torch.equal(bits(x), bits(x2)) and torch.equal(bits(pred), bits(pred2)) and torch.equal(applied, applied2)
        if len(idx) == 64:
            seen |= AT.combinations(applied.cpu().numpy())
    assert seen == AT.all_combinations(2)                           # both flip states at all four corner clamps
    # another draw is another key: other transforms for the same rows
    assert not torch.equal(run_u8(s, FULL, np.arange(64), draw=1)[2], run_u8(s, FULL, np.arange(64), draw=0)[2])


# ---- 2. single transforms against torch alone ----

def test_flip_alone(u8set):
    s = u8set
    for b in range(0, N, 64):
        x, _, applied = run_u8(s, Augment(flip=1.0), np.arange(b, b + 64))
        assert torch.equal(bits(x), bits(s["plain"][b:b + 64].flip(3)))
        assert applied.cpu().tolist() == [[1, 0, 0, 0]] * 64


def test_largest_shift_alone(u8set):
    s = u8set
    S = s["w"] // 4
    rows = []
    for b in range(0, N, 64):
        x, _, applied = run_u8(s, Augment(shift=S), np.arange(b, b + 64))
        a = applied.cpu().numpy()
        assert not a[:, 0].any() and not a[:, 3].any()
        assert torch.equal(bits(x), bits(AT.permute(s["plain"][b:b + 64], applied)))
        rows.append(a)
    a = np.concatenate(rows)
    for col in (1, 2):
        assert a[:, col].min() == -S and a[:, col].max() == S


def test_brightness_alone(u8set):
    s = u8set
    clamped = unclamped = 0
    for b in range(0, N, 64):
        x, _, applied = run_u8(s, Augment(brightness=0.9), np.arange(b, b + 64))
        assert not applied[:, :3].any()
        prod = s["plain"][b:b + 64] * AT.gains(applied)[:, None, None, None]
        assert torch.equal(bits(x), bits(torch.minimum(prod, torch.ones((), device=DEV))))
        clamped += int((prod > 1).sum())
        unclamped += int((prod < 1).sum())
    assert clamped > 0 and unclamped > 0


# ---- 3. the all-zero configuration ----

def test_zero_augment_is_the_plain_gather(u8set):
    s = u8set
    for draw in (0, 3):
        x, pred, applied = run_u8(s, Augment(seed=draw), np.arange(64, 128), draw=draw)
        assert torch.equal(bits(x), bits(s["plain"][64:128])) and torch.equal(bits(pred), bits(s["pred"][64:128]))
        assert not applied.any()


# ---- 4. the fp32 variant ----

@pytest.fixture(scope="module", params=[64, 128])
def f32set(request):
    w = request.param
    n = 64 if w == 64 else 24
    rng = np.random.default_rng(w + 1)
    frames = rng.uniform(-1, 1, size=(n, 3, w, w)).astype(np.float32)
    frames[0, 0, 0, 0], frames[1, 2, w - 1, w - 1], frames[2, 1, w // 2, 0] = -0.0, np.nan, -0.0
    frames[3, :, 0, :], frames[3, :, :, w - 1] = np.nan, -0.0              # whole edges: what the clamps replicate
    preds = rng.random((n, 1)).astype(np.float32)
    ds = E.ReconDataset(torch.from_numpy(frames).to(DEV), torch.from_numpy(preds).to(DEV), np.zeros((n, 3), np.int64))
    return dict(w=w, n=n, ds=ds, h=Handle(w, 64))


def test_f32_flip_and_shift_are_bit_copies(f32set):
    s = f32set
    n, w, ds, h = s["n"], s["w"], s["ds"], s["h"]
    every = torch.arange(n, dtype=torch.int64, device=DEV)
    plain, ppred = torch.empty(n, 3, w, w, device=DEV), torch.empty(n, 1, device=DEV)
    ds.gather(h, n, every, plain, ppred)
    assert torch.equal(bits(plain), bits(ds.frames))
    for aug, draw in ((Augment(flip=0.5, shift=2), 0), (Augment(flip=0.5, shift=w // 4, seed=3), 5), (Augment(flip=1.0), 1), (Augment(), 2)):
        x, pred = torch.full((n, 3, w, w), -3.0, device=DEV), torch.full((n, 1), -3.0, device=DEV)
        applied = torch.full((n, 4), -77, dtype=torch.int32, device=DEV)
        ds.gather(h, n, every, x, pred, aug=aug.at(draw), applied=applied)
        assert np.array_equal(applied.cpu().numpy(), aug.draws(draw, np.arange(n)))
        assert torch.equal(bits(x), AT.permute(bits(ds.frames), applied))
        assert torch.equal(bits(pred), bits(ds.preds))
    assert torch.equal(bits(x), bits(plain))                               # the last one, Augment(): the plain gather's bits
    # repeated and permuted indices
    idx = torch.tensor([2, 2, 3, 1, 3, 0], dtype=torch.int64, device=DEV)
    x, pred, applied = torch.empty(6, 3, w, w, device=DEV), torch.empty(6, 1, device=DEV), torch.empty(6, 4, dtype=torch.int32, device=DEV)
    ds.gather(h, 6, idx, x, pred, aug=Augment(flip=0.5, shift=2).at(9), applied=applied)
    assert torch.equal(bits(x), AT.permute(bits(ds.frames[idx]), applied))
    assert np.array_equal(applied.cpu().numpy(), Augment(flip=0.5, shift=2).draws(9, idx.cpu().numpy()))


def test_f32_refuses_a_gain_and_writes_nothing(f32set):
    s = f32set
    w, ds, h = s["w"], s["ds"], s["h"]
    x, pred = torch.full((4, 3, w, w), -3.0, device=DEV), torch.full((4, 1), -3.0, device=DEV)
    applied = torch.full((4, 4), -77, dtype=torch.int32, device=DEV)
    with pytest.raises(cvlib.CvaeError, match="error -1.*gain_q16"):
        ds.gather(h, 4, torch.arange(4, dtype=torch.int64, device=DEV), x, pred, aug=Augment(brightness=0.1).at(0), applied=applied)
    torch.cuda.synchronize()
    assert bool((x == -3.0).all()) and bool((pred == -3.0).all()) and bool((applied == -77).all())


# ---- 5. bounds ----

GUARD = 16384                   # elements of 4 bytes: 64 KB on either side


def _banded(numel, fill, dtype):
    buf = torch.full((GUARD + numel + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _bands_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_bad_indices_and_guard_bands(u8set, f32set, kind):
    if kind == "u8":
        w, ds, h, n = u8set["w"], u8set["ds"], u8set["h"], N
        aug = FULL
    else:
        w, ds, h, n = f32set["w"], f32set["ds"], f32set["h"], f32set["n"]
        aug = Augment(flip=0.5, shift=2)
    idx = np.array([3, -1, 4, n, n - 1, 0, -2 ** 40, 2 ** 40, 1], np.int64)
    B = len(idx)
    bad = (idx < 0) | (idx >= n)
    good = torch.from_numpy(np.flatnonzero(~bad)).to(DEV)
    SENT = -123.0
    xb, x = _banded(B * 3 * w * w, SENT, torch.float32)
    pb, pred = _banded(B, SENT, torch.float32)
    ab, applied = _banded(B * 4, -77, torch.int32)
    x, pred, applied = x.view(B, 3, w, w), pred.view(B, 1), applied.view(B, 4)
    d_idx = torch.from_numpy(idx).to(DEV)
    ds.gather(h, B, d_idx, x, pred, aug=aug.at(0), applied=applied)
    torch.cuda.synchronize()
    assert _bands_intact(xb, SENT) and _bands_intact(pb, SENT) and _bands_intact(ab, -77)
    assert not bool((x == SENT).any()) and not bool((pred == SENT).any()) and not bool((applied == -77).any())     # all written
    d_bad = torch.from_numpy(bad).to(DEV)
    assert bool(torch.isnan(x[d_bad]).all()) and bool(torch.isnan(pred[d_bad]).all()) and not applied[d_bad].any()
    # the rows next to them are what the same rows give in a batch of valid indices only
    gx, gp, ga = torch.empty(len(good), 3, w, w, device=DEV), torch.empty(len(good), 1, device=DEV), torch.empty(len(good), 4, dtype=torch.int32, device=DEV)
    ds.gather(h, len(good), d_idx[good], gx, gp, aug=aug.at(0), applied=ga)
    assert torch.equal(bits(x[good]), bits(gx)) and torch.equal(bits(pred[good]), bits(gp)) and torch.equal(applied[good], ga)
    assert np.array_equal(ga.cpu().numpy(), aug.draws(0, idx[~bad]))
    if kind == "u8":
        plain = u8set["plain"][d_idx[good]]
        assert torch.equal(bits(gx), bits(AT.transform(plain, ga)))
    else:
        assert torch.equal(bits(gx), AT.permute(bits(ds.frames[d_idx[good]]), ga))


def test_invalid_arguments_leave_the_outputs_untouched(u8set):
    s = u8set
    w, ds, h = s["w"], s["ds"], s["h"]
    x, pred = torch.full((4, 3, w, w), -3.0, device=DEV), torch.full((4, 1), -3.0, device=DEV)
    applied = torch.full((4, 4), -77, dtype=torch.int32, device=DEV)
    idx = torch.arange(4, dtype=torch.int64, device=DEV)
    A = cvlib.AugmentParams
    cases = [(None, "null aug"), (A(1, 2 ** 24 + 1, 0, 0, 0), "flip_below"), (A(1, 0, w // 4 + 1, 0, 0), "max_shift"),
             (A(1, 0, -1, 0, 0), "max_shift"), (A(1, 0, 0, 65536, 0), "gain_q16"), (A(1, 0, 0, -1, 0), "gain_q16"),
             (A(1, 0, 0, 0, 1), "reserved")]
    for aug, word in cases:
        with pytest.raises(cvlib.CvaeError, match="error -1.*" + word):
            h.preprocess_u8_gather_aug(4, ds.frames, ds.preds, idx, aug, x, pred, applied)
    with pytest.raises(cvlib.CvaeError, match="error -1.*batch"):           # what the plain gather refuses
        h.preprocess_u8_gather_aug(65, ds.frames, ds.preds, torch.zeros(65, dtype=torch.int64, device=DEV), FULL.at(0),
                                   torch.empty(65, 3, w, w, device=DEV), torch.empty(65, 1, device=DEV))
    torch.cuda.synchronize()
    assert bool((x == -3.0).all()) and bool((pred == -3.0).all()) and bool((applied == -77).all())
    # the extremes of every range are accepted
    h.preprocess_u8_gather_aug(4, ds.frames, ds.preds, idx, A(2 ** 64 - 1, 2 ** 24, w // 4, 65535, 0), x, pred, applied)
    assert bool((applied[:, 0] == 1).all()) and bool(torch.isfinite(x).all())


# ---- 6. past 2^31 bytes ----

def _pattern(first, n):
    i = torch.arange(first, first + n, device=DEV, dtype=torch.int64)[:, None]
    j = torch.arange(64 * 64 * 3, device=DEV, dtype=torch.int64)[None, :]
    return ((i * 7 + j * 13 + (i * j) % 5) % 251).to(torch.uint8).view(n, 64, 64, 3)


def test_augmented_gather_past_2_31_bytes():
    fb = 64 * 64 * 3
    n = 174763 + 40                                       # 2^31 / 12288 = 174762.67 frames
    assert n * fb > 2 ** 31
    try:
        frames = torch.empty(n, 64, 64, 3, dtype=torch.uint8, device=DEV)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"no room for a {n * fb / 2 ** 30:.1f} GiB dataset buffer: {e}")
    straddle = 2 ** 31 // fb                              # the frame that holds byte 2^31
    assert straddle * fb < 2 ** 31 < (straddle + 1) * fb
    idx = np.array([n - 1, straddle, straddle - 1, straddle + 1, n - 2, 0, n - 40], np.int64)
    for i in idx:                                         # only the gathered frames need their pattern
        frames[int(i)] = _pattern(int(i), 1)[0]
    preds = torch.arange(n, dtype=torch.float32, device=DEV).view(n, 1)
    B = len(idx)
    h = Handle(64, 16)
    aug = Augment(flip=1.0, shift=1)
    x, p = torch.empty(B, 3, 64, 64, device=DEV), torch.empty(B, 1, device=DEV)
    applied = torch.empty(B, 4, dtype=torch.int32, device=DEV)
    h.preprocess_u8_gather_aug(B, frames, preds, torch.from_numpy(idx).to(DEV), aug.at(0), x, p, applied)
    src = torch.cat([_pattern(int(i), 1) for i in idx])
    ref = torch.empty(B, 3, 64, 64, device=DEV)
    h.preprocess_u8(B, src, ref)
    want = aug.draws(0, idx)
    assert np.array_equal(applied.cpu().numpy(), want) and want[:, 0].all() and np.abs(want[:, 1:3]).max() == 1
    assert torch.equal(bits(x), bits(AT.transform(ref, applied)))
    assert p[:, 0].cpu().tolist() == idx.astype(np.float32).tolist()


# ---- 7. the trainers ----

TRAIN_AUG = Augment(flip=0.5, shift=2, brightness=0.2, seed=3)


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(23)
    frames = rng.integers(0, 256, size=(23, 64, 64, 3), dtype=np.uint8)
    vals = rng.random(23).astype(np.float32)
    return E.DeviceDataset.from_host(frames, vals)


def _vae_state(vae, tr):
    return [vae.theta.detach().clone(), tr.m.clone(), tr.v.clone(), vae.bn_state.clone()]


def _same(a, b):
    return all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))


def _same_result(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(bits(a[k]), bits(b[k])), k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _seed(gen, np_seed=123, gen_seed=9):
    np.random.seed(np_seed)
    gen.manual_seed(gen_seed)


def _hand_loop_vae(tr, ds, aug, B, epochs, gen):
    n, w = len(ds), ds.width
    x, pred = torch.empty(B, 3, w, w, device=DEV), torch.empty(B, 1, device=DEV)
    for _ in range(epochs):
        idx = np.arange(n)
        np.random.shuffle(idx)
        d_idx = torch.from_numpy(idx).to(DEV)
        for b in range(0, n, B):
            nb = min(B, n - b)
            ds.gather(tr.h, nb, d_idx[b:b + nb], x[:nb], pred[:nb], aug=aug.at(tr.step_count))
            tr.step(x[:nb], pred[:nb], torch.randn(nb, P.latent_dim, device=DEV, generator=gen))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fused_trainer_with_an_augmentation(small, precision):
    B, gen = 8, torch.Generator(device=DEV)
    make = lambda: VariationalAutoencoder(max_batch=B, seed=5, precision=precision).to(DEV)      # noqa: E731
    vae = make()
    tr = FusedTrainer(vae, augment=TRAIN_AUG)
    _seed(gen)
    tr.fit_device(small, B, epochs=2, generator=gen)
    assert tr.step_count == 6
    # a hand loop of gather(aug=at(step_count)) + step on a trainer that has no augmentation
    vae2 = make()
    tr2 = FusedTrainer(vae2)
    _seed(gen)
    _hand_loop_vae(tr2, small, TRAIN_AUG, B, 2, gen)
    torch.cuda.synchronize()
    assert _same(_vae_state(vae, tr), _vae_state(vae2, tr2)) and vae.num_batches_tracked == vae2.num_batches_tracked
    # ... and it is not the plain run
    vae0 = make()
    tr0 = FusedTrainer(vae0)
    _seed(gen)
    tr0.fit_device(small, B, epochs=2, generator=gen)
    assert not torch.equal(vae0.theta, vae.theta)
    # interrupted after 3 steps (one epoch), continued by a new trainer from the state
    vae3 = make()
    tr3 = FusedTrainer(vae3, augment=TRAIN_AUG)
    _seed(gen)
    tr3.fit_device(small, B, epochs=1, generator=gen)
    state = tr3.state_dict()
    assert tr3.step_count == 3 and state["augment"] == TRAIN_AUG.state_dict()
    vae4 = make()
    vae4.theta.data.copy_(vae3.theta.data)
    vae4.bn_state.copy_(vae3.bn_state)
    tr4 = FusedTrainer(vae4)
    tr4.load_state_dict(state)
    assert tr4.augment == TRAIN_AUG and tr4.step_count == 3
    tr4.fit_device(small, B, epochs=1, generator=gen)
    torch.cuda.synchronize()
    assert tr4.step_count == 6 and _same(_vae_state(vae, tr), _vae_state(vae4, tr4))
    # evaluate() never augments: the trainer with an augmentation against the identical one without
    _same_result(tr.evaluate(small, B, per_image=True), tr2.evaluate(small, B, per_image=True))


def test_recon_dataset_with_an_augmentation():
    rng = np.random.default_rng(4)
    n, B, gen = 23, 8, torch.Generator(device=DEV)
    frames = torch.from_numpy(np.tanh(rng.normal(size=(n, 3, 64, 64))).astype(np.float32)).to(DEV)
    ds = E.ReconDataset(frames, torch.from_numpy(rng.random((n, 1)).astype(np.float32)).to(DEV), np.zeros((n, 3), np.int64))
    aug = Augment(flip=0.5, shift=2)
    vae = VariationalAutoencoder(max_batch=B, seed=6).to(DEV)
    tr = FusedTrainer(vae, augment=aug)
    _seed(gen)
    tr.fit_device(ds, B, epochs=2, generator=gen)
    vae2 = VariationalAutoencoder(max_batch=B, seed=6).to(DEV)
    tr2 = FusedTrainer(vae2)
    _seed(gen)
    _hand_loop_vae(tr2, ds, aug, B, 2, gen)
    torch.cuda.synchronize()
    assert tr.step_count == 6 and _same(_vae_state(vae, tr), _vae_state(vae2, tr2))
    # a brightness gain on fp32 entries: refused before the first launch
    tr3 = FusedTrainer(vae2, augment=Augment(flip=0.5, brightness=0.1))
    before = _vae_state(vae2, tr3)
    with pytest.raises(ValueError, match="fp32 entries"):
        tr3.fit_device(ds, B, epochs=1, generator=gen)
    torch.cuda.synchronize()
    assert tr3.step_count == 0 and _same(before, _vae_state(vae2, tr3))


def test_critic_trainer_with_an_augmentation(small):
    B, gen = 8, torch.Generator(device=DEV)
    handle = Handle(64, 32)

    def make(**kw):
        critic = Critic(handle=handle).to(DEV)
        critic.load_state_dict(initial_state_dict(3))
        return critic, CriticTrainer(critic, **kw)

    state_of = lambda t: [t.theta.clone(), t.m.clone(), t.v.clone()]      # noqa: E731
    c1, tr = make(augment=TRAIN_AUG)
    _seed(gen)
    log = tr.fit_device(small, B, epochs=2, generator=gen).clone()
    assert tr.step_count == 6 and log.shape == (6, 4)
    c2, tr2 = make()
    _seed(gen)
    x, target, hand = torch.empty(B, 3, 64, 64, device=DEV), torch.empty(B, 1, device=DEV), []
    for _ in range(2):
        idx = np.arange(len(small))
        np.random.shuffle(idx)
        d_idx = torch.from_numpy(idx).to(DEV)
        for b in range(0, len(small), B):
            nb = min(B, len(small) - b)
            small.gather(handle, nb, d_idx[b:b + nb], x[:nb], target[:nb], aug=TRAIN_AUG.at(tr2.step_count))
            keep = tr2.draw_keep(nb, gen)
            hand.append(tr2.step(x[:nb], target[:nb], keep=keep).clone())
    torch.cuda.synchronize()
    assert torch.equal(bits(log), bits(torch.stack(hand))) and _same(state_of(tr), state_of(tr2))
    c0, tr0 = make()
    _seed(gen)
    tr0.fit_device(small, B, epochs=2, generator=gen)
    assert not torch.equal(tr0.theta, tr.theta)
    # interrupted after 3 steps
    c3, tr3 = make(augment=TRAIN_AUG)
    _seed(gen)
    tr3.fit_device(small, B, epochs=1, generator=gen)
    state = tr3.state_dict()
    assert tr3.step_count == 3 and state["augment"] == TRAIN_AUG.state_dict()
    c4, tr4 = make()
    tr4.load_state_dict(state)
    assert tr4.augment == TRAIN_AUG
    tr4.fit_device(small, B, epochs=1, generator=gen)
    torch.cuda.synchronize()
    assert tr4.step_count == 6 and _same(state_of(tr), state_of(tr4))
    _same_result(tr.evaluate(small, B, per_frame=True), tr2.evaluate(small, B, per_frame=True))
