"""Host-side checks of critic training (no GPU): the torch-CPU restatement against the reference-pinned fixture, the
target helper, the reward loader, the dataset draw, and the argument checks of cvae_critic_grad that precede any device access."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_train_ref as ref                                  # noqa: E402
from critic_vae_amd import episodes as E                        # noqa: E402
from critic_vae_amd import lib as cvlib                         # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "critic_train_real.npz"))
    ck = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    return dict(z=z, w={k: ck["w/" + k] for k, _ in ref.KEYS}, x=ref.frames_to_x(u8[:37]))


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("loss", ["bce", "mse"])
def test_restatement_matches_reference_fixture(fx, B, loss):
    """critic_train_ref.step (fp32) == the reference class's train-mode step stored by make_critic_train_golden.py."""
    z = fx["z"]
    r = ref.step(fx["w"], fx["x"][:B], z["target"][:B], z["keep"][:B], float(z["dropout_p"]), loss)
    # the generator asserts 1e-6 in its own process; another host's thread count and BLAS branch reorder the fp32 sums:
    # 1e-5 on pred / loss and 1e-5 of the largest gradient, an order below the device tests' bounds
    g = z[f"b{B}/{loss}/grads"]
    gap = np.abs(r["flat_grads"] - g).max() / np.abs(g).max()
    print(f"B={B} {loss}: pred gap {np.abs(r['pred'] - z[f'b{B}/{loss}/pred']).max():.2e}, gradient gap {gap:.2e} of max")
    assert np.abs(r["pred"] - z[f"b{B}/{loss}/pred"]).max() <= 1e-5
    assert abs(r["bce"] - z[f"b{B}/{loss}/scalars"][0]) <= 1e-5 and abs(r["mse"] - z[f"b{B}/{loss}/scalars"][1]) <= 1e-5
    assert gap <= 1e-5
    assert np.array_equal(r["decisions"], z["decisions"][:B])
    # imposing a run's own decisions changes nothing
    r2 = ref.step(fx["w"], fx["x"][:B], z["target"][:B], z["keep"][:B], float(z["dropout_p"]), loss, decisions=r["decisions"])
    assert np.array_equal(r2["flat_grads"], r["flat_grads"]) and np.array_equal(r2["pred"], r["pred"])


def test_fixture_layout(fx):
    z = fx["z"]
    assert z["keep"].shape == (37, cvlib.CRITIC_KEEP) and z["decisions"].shape == (37, cvlib.CRITIC_DECISIONS)
    assert z["decisions"][:, :11008].max() <= 4 and z["decisions"][:, 11008:].max() <= 1
    assert z["traj/loss64"].shape == (40,) and z["traj/params64"].shape == (ref.N_PARAMS,)
    assert np.unpackbits(z["traj/keep_bits"], axis=1).shape == (40, 37 * cvlib.CRITIC_KEEP)
    assert 0 < float(z["traj/gap32"]) < 1e-5


def test_discounted_targets_hand_worked():
    # shift 1, gamma 1/2: r' = (0,1,0,0,0,2,0,0); v backwards = 0, 0, 2, 1, 1/2, 1/4, 1 + 1/8, 9/16; clipped at 1
    got = E.discounted_targets([0, 0, 1, 0, 0, 0, 2, 0], gamma=0.5, shift=1, clip=1.0)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([0.5625, 1.0, 0.25, 0.5, 1.0, 1.0, 0.0, 0.0], np.float32))
    unclipped = E.discounted_targets([0, 0, 1, 0, 0, 0, 2, 0], gamma=0.5, shift=1, clip=np.inf)
    assert np.array_equal(unclipped, np.array([0.5625, 1.125, 0.25, 0.5, 1.0, 2.0, 0.0, 0.0], np.float32))


@pytest.mark.parametrize("T,k,shift,gamma", [(50, 30, 12, 0.98), (50, 5, 12, 0.98), (20, 19, 0, 0.9), (8, 3, 20, 0.5)])
def test_discounted_targets_single_reward_closed_form(T, k, shift, gamma):
    """One reward R at frame k: v_t = R * gamma^(k - shift - t) for t <= k - shift, 0 after (and all 0 if k < shift)."""
    R = 0.75
    r = np.zeros(T)
    r[k] = R
    want = np.zeros(T)
    if k - shift >= 0:
        t = np.arange(k - shift + 1)
        want[:k - shift + 1] = R * gamma ** (k - shift - t)
    got = E.discounted_targets(r, gamma=gamma, shift=shift, clip=1.0)
    assert np.abs(got - want.astype(np.float32)).max() <= 1e-7


def _write(dirpath, name, arr):
    os.makedirs(dirpath, exist_ok=True)
    np.save(os.path.join(dirpath, name + ".npy"), arr)


def test_load_rewards_matches_and_errors(tmp_path):
    fr, rw = str(tmp_path / "frames"), str(tmp_path / "rewards")
    for name, T in (("b", 4), ("a", 3)):
        _write(fr, name, np.zeros((T, 64, 64, 3), np.uint8))
        _write(rw, name, np.arange(T, dtype=np.float32))
    eps = E.load_episodes([fr])
    assert [n for n, _ in eps] == ["a", "b"]                               # the frame directory still yields every .npy
    got = E.load_rewards([rw], eps)
    assert [n for n, _ in got] == ["a", "b"] and got[0][1].dtype == np.float64 and got[1][1].shape == (4,)
    assert [n for n, _ in E.load_rewards(rw)] == ["a", "b"]
    _write(fr, "c", np.zeros((2, 64, 64, 3), np.uint8))
    with pytest.raises(ValueError, match="no reward file"):
        E.load_rewards([rw], E.load_episodes([fr]))
    _write(rw, "c", np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="2 frames"):
        E.load_rewards([rw], E.load_episodes([fr]))
    _write(rw, "c", np.zeros((2, 1), np.float32))
    with pytest.raises(ValueError, match="numeric"):
        E.load_rewards([rw])
    with pytest.raises(FileNotFoundError):
        E.load_rewards([str(tmp_path / "nowhere")])


def test_critic_dataset_index_draw():
    lengths = [7, 0, 12, 5]
    full = E.critic_dataset_indices(lengths, None, seed=3)
    assert full.shape == (24, 2) and full.dtype == np.int64
    assert sorted(map(tuple, full)) == [(t, f) for t, L in enumerate(lengths) for f in range(L)]      # every frame once
    part = E.critic_dataset_indices(lengths, 10, seed=3)
    assert np.array_equal(part, full[:10]) and len(set(map(tuple, part))) == 10                        # without replacement
    assert np.array_equal(part, E.critic_dataset_indices(lengths, 10, seed=3))
    assert not np.array_equal(part, E.critic_dataset_indices(lengths, 10, seed=4))
    pick = np.random.default_rng(3).permutation(24)[:10]                                               # the documented draw
    offs = np.array([0, 7, 7, 19])
    assert np.array_equal(part[:, 1] + offs[part[:, 0]], pick)
    with pytest.raises(ValueError):
        E.critic_dataset_indices(lengths, 25)


def test_critic_grad_host_argument_checks():
    """Everything cvae_critic_grad rejects before it touches a device; the pointers are never dereferenced."""
    lib = cvlib.load()
    assert lib.cvae_critic_train_floats() == cvlib.CRITIC_TRAIN_FLOATS == 11876
    assert cvlib.CRITIC_TRAIN_FLOATS % 4 == 0 and cvlib.CRITIC_TRAIN_FLOATS - lib.cvae_critic_param_count() == 3
    h = cvlib.Handle(64, 4)
    sb = lib.cvae_critic_grad_scratch_bytes
    # at most 256 gradient partials + two loss terms per image, independent of the handle's max_batch
    assert sb(h.h, 1) >= (11876 + 2) * 4 and sb(h.h, 37) >= (37 * 11876 + 74) * 4
    assert sb(h.h, 65536) >= (256 * 11876 + 2 * 65536) * 4 and sb(h.h, 65536) < (257 * 11876 + 2 * 65536) * 4 + 256
    assert sb(h.h, 4096) - sb(h.h, 2048) <= 2 * 2048 * 4 + 256
    assert sb(h.h, 0) == -1 and sb(h.h, 65537) == -1 and sb(None, 4) == -1
    ok = 4096                                    # a non-null, 16-byte aligned address that no check dereferences

    def call(hh=h.h, B=4, x=ok, target=ok, keep=None, p=0.3, kind=0, params=ok, grads=ok, pred=ok, scal=ok, dec=None, scratch=ok):
        return lib.cvae_critic_grad(hh, B, x, target, keep, C.c_float(p), kind, params, grads, pred, scal, dec, scratch, None)

    EINVAL, EUNSUPPORTED = -1, -2
    assert call(hh=None) == EINVAL
    assert call(B=0) == EINVAL and call(B=65537) == EINVAL
    assert call(p=1.0) == EINVAL and call(p=-0.1) == EINVAL and call(p=float("nan")) == EINVAL
    assert call(kind=2) == EINVAL and call(kind=-1) == EINVAL
    assert b"loss_kind" in lib.cvae_last_error()
    for name in ("x", "target", "params", "grads", "pred", "scal", "scratch"):
        assert call(**{name: None}) == EINVAL, name
    assert call(x=ok + 4) == EINVAL and call(scratch=ok + 8) == EINVAL and call(dec=ok + 1) == EINVAL
    wide = cvlib.Handle(128, 2)
    assert call(hh=wide.h) == EUNSUPPORTED
    assert b"64x64" in lib.cvae_last_error()
