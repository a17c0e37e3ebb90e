"""The second VAE's dataset, host side (critic_vae_amd.episodes / train / segment): the plain restatement of the recon
branch of load_minerl_data (vae_utility.py:406-443) against what the reference's own code built (recon_real.npz, written by
tests/golden/make_recon_golden.py), the CLI flags of -dataset / -second / --second, and the argument checks of the new C-ABI
entry points."""
import os

import numpy as np
import pytest

from critic_vae_amd import episodes as E
from critic_vae_amd import segment
from critic_vae_amd import train


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "recon_real.npz"))


@pytest.fixture(scope="module")
def ep(golden_dir):
    return np.load(os.path.join(golden_dir, "episodes_real.npz"))


def walk_of(ep):
    offs = np.concatenate([[0], np.cumsum(ep["traj_len"])])
    trajs = [ep["traj_idx"][offs[t]:offs[t + 1]] for t in range(len(ep["traj_len"]))]
    return [trajs[t] for t in ep["order"]]


def test_restatement_reproduces_the_reference(fx, ep):
    walk = walk_of(ep)
    preds = ep["pool_preds"]
    collect, total = int(fx["collect"]), int(fx["total_images"])
    sizes, entries, counts = E.select_recon_host([preds[s] for s in walk], collect=collect, total_images=total)
    assert sizes == fx["sizes"].tolist()
    assert [int(walk[t][i]) for t, i, _ in entries] == fx["dset_pool"].tolist()
    assert [k for _, _, k in entries] == fx["dset_kind"].tolist()
    assert 2 * counts[:, 0].sum() + counts[:, 1].sum() + counts[:, 2].sum() == len(fx["dset_pool"])
    assert len(sizes) < len(walk), "the cut falls inside the trajectory list"
    plain = E.select_host([preds[s] for s in walk], collect=collect, total_images=total)[0]
    assert len(plain) != len(sizes), "counting mid frames twice changes which trajectory is last"


def test_restatement_kinds_edges_and_nan():
    f = np.float32
    vals = [f(0.4), np.nextafter(f(0.4), f(0)), f(0.6), np.nextafter(f(0.6), f(1)), f(0.7), np.nextafter(f(0.7), f(0)),
            f(0.25), np.nextafter(f(0.25), f(1)), f("nan"), f(-0.0), f(1.0), f(0.65)]
    _, entries, counts = E.select_recon_host([vals], collect=100, total_images=100)
    assert entries == [(0, 0, 0), (0, 0, 1), (0, 2, 0), (0, 2, 1), (0, 4, 0), (0, 6, 1), (0, 9, 1), (0, 10, 0)]
    assert counts[0].tolist() == [2, 2, 2]


def test_restatement_caps_and_doubled_cut():
    mid = np.full(400, 0.5, np.float32)
    sizes, entries, counts = E.select_recon_host([mid, mid], collect=150, total_images=301)
    assert sizes == [0, 300] and counts.tolist() == [[150, 0, 0], [150, 0, 0]] and len(entries) == 600
    sizes, entries, counts = E.select_recon_host([mid, mid], collect=150, total_images=300)      # 150 mid frames = 300 entries
    assert sizes == [0] and counts.tolist() == [[150, 0, 0], [0, 0, 0]] and len(entries) == 300
    assert E.select_host([mid, mid], collect=150, total_images=300)[0] == [0, 150]
    assert E.select_recon_host([mid], total_images=0)[0] == []
    mixed = np.tile(np.array([0.5, 0.9, 0.1], np.float32), 200)
    _, entries, counts = E.select_recon_host([mixed], collect=150, total_images=10 ** 6)
    assert counts.tolist() == [[150, 150, 150]] and len(entries) == 600          # the overshoot bound 4 * collect
    assert [k for _, _, k in entries[:4]] == [0, 1, 0, 1]


def test_cli_dataset_and_second_modes(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(train, "_build_recon_dataset", lambda args: seen.setdefault("dataset", args))
    monkeypatch.setattr(train, "_train_second", lambda args: seen.setdefault("second", args))
    monkeypatch.setattr(train, "_train_episodes", lambda args: seen.setdefault("train", args))
    train.main(["-dataset", "--episodes", str(tmp_path), "--critic", "synth", "--networks", "nets", "--out", "r.npz",
                "--total-images", "77", "--collect", "5", "--pickle", "r.pickle"])
    a = seen["dataset"]
    assert a.episodes == [str(tmp_path)] and a.networks == "nets" and a.out == "r.npz" and a.pickle == "r.pickle"
    assert a.total_images == 77 and a.collect == 5 and not a.train and not a.second
    train.main(["-second", "--dataset", "r.npz", "--critic", "c.pt", "--batch", "16", "--epochs", "3", "--save", "out"])
    a = seen["second"]
    assert a.dataset == "r.npz" and a.batch == 16 and a.epochs == 3 and a.save == "out" and not a.dataset_mode
    train.main(["-train", "--episodes", str(tmp_path), "--critic", "synth"])
    assert seen["train"].episodes == [str(tmp_path)]
    assert set(seen) == {"dataset", "second", "train"}


@pytest.mark.parametrize("argv", [[], ["-dataset", "--critic", "synth", "--out", "r.npz"],
                                  ["-dataset", "--episodes", "e", "--out", "r.npz"],
                                  ["-dataset", "--episodes", "e", "--critic", "synth"],
                                  ["-second", "--critic", "synth"], ["-second", "--dataset", "r.npz"],
                                  ["-train", "-second", "--dataset", "r.npz", "--critic", "synth"]])
def test_cli_refuses_incomplete_modes(monkeypatch, argv):
    for name in ("_build_recon_dataset", "_train_second", "_train_episodes"):
        monkeypatch.setattr(train, name, lambda args: pytest.fail("must not run"))
    with pytest.raises(SystemExit) as e:
        train.main(argv)
    assert e.value.code == 2


def test_network_file_names_of_the_second_vae():
    assert (train.SECOND_ENCODER_FILE, train.SECOND_DECODER_FILE) == ("vae2_encoder.pt", "vae2_decoder.pt")
    assert train._network_files("d", False) == (os.path.join("d", "vae_encoder.pt"), os.path.join("d", "vae_decoder.pt"))
    assert train._network_files("d", True) == (os.path.join("d", "vae2_encoder.pt"), os.path.join("d", "vae2_decoder.pt"))


def test_segment_cli_second_flag():
    a = segment.parse_args(["-video", "--second", "--networks", "nets"])
    assert a.second and a.networks == "nets"
    assert not segment.parse_args(["-video"]).second
    with pytest.raises(SystemExit):
        segment.parse_args([])
    with pytest.raises(SystemExit):
        segment.parse_args(["--second"])


def test_recon_entry_points_reject_bad_arguments():
    """Host-side argument checks of the new C-ABI entry points (no device access before them)."""
    import ctypes as C
    from critic_vae_amd import lib as cvlib
    lib = cvlib.load()
    h = cvlib.Handle(64, 8)
    fake = C.c_void_p(4096)                 # never dereferenced: every call below fails its checks first

    def err(rc):
        return rc == -1 and lib.cvae_last_error().decode()

    def select(hh=h.h, n_traj=1, off=fake, n_frames=4, collect=1, total=10, running=fake, sel=fake):
        return lib.cvae_curate_select_recon(hh, n_traj, off, n_frames, fake, collect, total, running, fake, fake, fake, fake,
                                            fake, fake, fake, sel, None)

    assert "collect" in err(select(collect=0))
    assert ">= 0" in err(select(n_traj=-1))
    assert ">= 0" in err(select(n_frames=-4))
    assert ">= 0" in err(select(total=-5))
    assert "null" in err(select(off=None))
    assert "null" in err(select(running=None))
    assert "null" in err(select(sel=None))
    assert "null" in err(select(hh=None))
    assert "width" in err(lib.cvae_gather_f32(h.h, 2, 128, fake, fake, 4, fake, fake, fake, None))
    assert "batch" in err(lib.cvae_gather_f32(h.h, 9, 64, fake, fake, 4, fake, fake, fake, None))
    assert "batch" in err(lib.cvae_gather_f32(h.h, 0, 64, fake, fake, 4, fake, fake, fake, None))
    assert "n_frames" in err(lib.cvae_gather_f32(h.h, 2, 64, fake, fake, 0, fake, fake, fake, None))
    assert "n_frames" in err(lib.cvae_gather_f32(h.h, 2, 64, fake, fake, -3, fake, fake, fake, None))
    assert "null" in err(lib.cvae_gather_f32(h.h, 2, 64, fake, fake, 4, None, fake, fake, None))
    assert "null" in err(lib.cvae_gather_f32(h.h, 2, 64, None, fake, 4, fake, fake, fake, None))
    assert "null" in err(lib.cvae_gather_f32(None, 2, 64, fake, fake, 4, fake, fake, fake, None))
    assert "aligned" in err(lib.cvae_gather_f32(h.h, 2, 64, C.c_void_p(4100), fake, 4, fake, fake, fake, None))
    assert "n_entries" in err(lib.cvae_recon_zcat(h.h, 0, fake, fake, fake, fake, 4, fake, None))
    assert "n_entries" in err(lib.cvae_recon_zcat(h.h, 9, fake, fake, fake, fake, 4, fake, None))
    assert "n_sel" in err(lib.cvae_recon_zcat(h.h, 2, fake, fake, fake, fake, 0, fake, None))
    assert "null" in err(lib.cvae_recon_zcat(h.h, 2, fake, None, fake, fake, 4, fake, None))
