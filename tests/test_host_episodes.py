"""Dataset curation from recorded trajectories, host side (critic_vae_amd.episodes): the plain restatement of
load_minerl_data (vae_utility.py:406-459) against what the reference's own code selected (episodes_real.npz, written by
tests/golden/make_episode_golden.py), the reference's trajectory order, episode loading and the -train CLI flags."""
import os

import numpy as np
import pytest

from critic_vae_amd import episodes as E
from critic_vae_amd import params as P
from critic_vae_amd import train


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "episodes_real.npz"))


def fixture_trajectories(fx):
    """Per trajectory in sorted-name order: its pool index sequence."""
    offs = np.concatenate([[0], np.cumsum(fx["traj_len"])])
    return [fx["traj_idx"][offs[t]:offs[t + 1]] for t in range(len(fx["traj_len"]))]


def test_params_cite_the_reference():
    assert P.collect == 150 and P.total_images == 50000
    assert np.float32(P.bin_mid[0]) == np.float32(0.4) and float(np.float32(P.bin_mid[1])) == 0.6000000238418579
    assert float(np.float32(P.bin_high)) == 0.699999988079071 and P.bin_low == 0.25


def test_restatement_reproduces_the_reference(fx):
    trajs = fixture_trajectories(fx)
    walk = [trajs[t] for t in fx["order"]]
    preds = fx["pool_preds"]
    sizes, selected, counts = E.select_host([preds[s] for s in walk], collect=int(fx["collect"]),
                                            total_images=int(fx["total_images"]))
    assert sizes == fx["sizes"].tolist()
    content = np.array([walk[t][i] for t, i in selected], np.int64)
    np.testing.assert_array_equal(content, fx["dset_pool"])
    assert counts.sum() == len(fx["dset_pool"])
    assert (counts == int(fx["collect"])).any(axis=0).all(), "every bin reaches its cap in some visited trajectory"
    assert len(sizes) < len(walk), "the cut falls inside the trajectory list"


def test_restatement_edges_are_float32():
    f = np.float32
    vals = [f(0.4), np.nextafter(f(0.4), f(0)), f(0.6), np.nextafter(f(0.6), f(1)), f(0.7), np.nextafter(f(0.7), f(0)),
            f(0.25), np.nextafter(f(0.25), f(1)), f("nan"), f(-0.0), f(1.0), f(0.65)]
    _, selected, counts = E.select_host([vals], collect=100, total_images=100)
    assert [i for _, i in selected] == [0, 2, 4, 6, 9, 10]
    assert counts[0].tolist() == [2, 2, 2]


def test_restatement_caps_and_cut():
    mid = np.full(400, 0.5, np.float32)
    _, sel, counts = E.select_host([mid, mid], collect=150, total_images=151)
    assert counts.tolist() == [[150, 0, 0], [150, 0, 0]] and len(sel) == 300
    sizes, sel, counts = E.select_host([mid, mid], collect=150, total_images=150)
    assert sizes == [0] and counts.tolist() == [[150, 0, 0], [0, 0, 0]]
    assert E.select_host([mid], total_images=0)[0] == []


def test_reference_order_matches_the_fixture(fx):
    names = fx["traj_names"].tolist()
    assert names == sorted(names)
    assert E.reference_order(names) == [names[i] for i in fx["order"]]
    rng_names = list(names)
    np.random.default_rng(seed=0).shuffle(rng_names)
    assert E.reference_order(names) == rng_names


def test_load_episodes_sorted_and_memory_mapped(tmp_path):
    for name, n in (("b", 3), ("a", 0), ("c", 2)):
        np.save(tmp_path / f"{name}.npy", np.full((n, 64, 64, 3), n, np.uint8))
    sub = tmp_path / "more"
    sub.mkdir()
    np.save(sub / "0.npy", np.zeros((1, 64, 64, 3), np.uint8))
    eps = E.load_episodes([str(tmp_path), str(sub / "0.npy")])
    assert [n for n, _ in eps] == ["0", "a", "b", "c"]
    assert [a.shape[0] for _, a in eps] == [1, 0, 3, 2]
    assert isinstance(eps[2][1], np.memmap) and int(eps[2][1][0, 0, 0, 0]) == 3
    assert [n for n, _ in E.load_episodes(str(tmp_path))] == ["a", "b", "c"]


@pytest.mark.parametrize("bad", [np.zeros((2, 64, 64, 3), np.float32), np.zeros((64, 64, 3), np.uint8),
                                 np.zeros((2, 64, 64, 4), np.uint8), np.zeros((2, 32, 32, 3), np.uint8),
                                 np.zeros((2, 64, 32, 3), np.uint8)])
def test_load_episodes_rejects_bad_arrays(tmp_path, bad):
    np.save(tmp_path / "bad.npy", bad)
    with pytest.raises(ValueError):
        E.load_episodes([str(tmp_path / "bad.npy")])


def test_load_episodes_rejects_duplicate_names(tmp_path):
    for d in ("x", "y"):
        (tmp_path / d).mkdir()
        np.save(tmp_path / d / "t.npy", np.zeros((1, 64, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        E.load_episodes([str(tmp_path / "x"), str(tmp_path / "y")])


def test_cli_accepts_episodes(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(train, "_train_episodes", lambda args: seen.setdefault("args", args))
    train.main(["-train", "--episodes", str(tmp_path), "x.npy", "--critic", "synth", "--total-images", "77",
                "--collect", "5", "--epochs", "2", "--batch", "16", "--save", str(tmp_path / "out")])
    a = seen["args"]
    assert a.episodes == [str(tmp_path), "x.npy"] and a.critic == "synth" and a.total_images == 77
    assert a.collect == 5 and a.epochs == 2 and a.batch == 16 and a.save == str(tmp_path / "out")
    seen.clear()
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "c.pt"])
    assert seen["args"].total_images == P.total_images and seen["args"].collect == P.collect


@pytest.mark.parametrize("critic", [[], ["--critic", "random"]])
def test_cli_refuses_episodes_without_critic(tmp_path, monkeypatch, critic):
    monkeypatch.setattr(train, "_train_episodes", lambda args: pytest.fail("must not train"))
    with pytest.raises(SystemExit) as e:
        train.main(["-train", "--episodes", str(tmp_path)] + critic)
    assert e.value.code == 2


def test_dataset_entry_points_reject_bad_arguments():
    """Host-side argument checks of the three C-ABI entry points (no device access before them)."""
    import ctypes as C
    from critic_vae_amd import lib as cvlib
    lib = cvlib.load()
    h = cvlib.Handle(64, 8)
    fake = C.c_void_p(4096)                 # never dereferenced: every call below fails its checks first

    def err(rc):
        return rc == -1 and lib.cvae_last_error().decode()

    assert "collect" in err(lib.cvae_curate_select(h.h, 1, fake, 4, fake, 0, 10, fake, fake, fake, fake, fake, None))
    assert ">= 0" in err(lib.cvae_curate_select(h.h, -1, fake, 4, fake, 1, 10, fake, fake, fake, fake, fake, None))
    assert ">= 0" in err(lib.cvae_curate_select(h.h, 1, fake, 4, fake, 1, -5, fake, fake, fake, fake, fake, None))
    assert "null" in err(lib.cvae_curate_select(h.h, 1, None, 4, fake, 1, 10, fake, fake, fake, fake, fake, None))
    assert "null" in err(lib.cvae_curate_select(None, 1, fake, 4, fake, 1, 10, fake, fake, fake, fake, fake, None))
    assert "width" in err(lib.cvae_gather_frames_u8(h.h, 128, fake, None, 4, fake, 4, fake, fake, None, 4, None))
    assert "null" in err(lib.cvae_gather_frames_u8(h.h, 64, None, None, 4, fake, 4, fake, fake, None, 4, None))
    assert "null" in err(lib.cvae_gather_frames_u8(h.h, 64, fake, fake, 4, fake, 4, fake, fake, None, 4, None))
    assert "range" in err(lib.cvae_gather_frames_u8(h.h, 64, fake, None, -1, fake, 4, fake, fake, None, 4, None))
    assert "aligned" in err(lib.cvae_gather_frames_u8(h.h, 64, C.c_void_p(4100), None, 4, fake, 4, fake, fake, None, 4, None))
    assert "width" in err(lib.cvae_preprocess_u8_gather(h.h, 2, 128, fake, fake, 4, fake, fake, fake, None))
    assert "batch" in err(lib.cvae_preprocess_u8_gather(h.h, 9, 64, fake, fake, 4, fake, fake, fake, None))
    assert "batch" in err(lib.cvae_preprocess_u8_gather(h.h, 0, 64, fake, fake, 4, fake, fake, fake, None))
    assert "n_frames" in err(lib.cvae_preprocess_u8_gather(h.h, 2, 64, fake, fake, 0, fake, fake, fake, None))
    assert "null" in err(lib.cvae_preprocess_u8_gather(h.h, 2, 64, fake, fake, 4, None, fake, fake, None))
