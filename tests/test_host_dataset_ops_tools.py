"""Host checks of tests/dataset_ops_tools.py, which tests/test_gpu_dataset_ops.py stands on: every named cut of every
trajectory family lands where its name says, shown with the plain restatement (episodes.select_host / select_recon_host)
alone; the list of cases that exist per family; the value set; the per-call expectation against the whole-walk restatement."""
import numpy as np
import pytest

import dataset_ops_tools as D
from critic_vae_amd import episodes as E

FORMS = [False, True]                 # cvae_curate_select, cvae_curate_select_recon


def test_value_set_holds_every_bin_edge_and_its_neighbours():
    f = np.float32
    vals = D.adversarial_values()
    assert vals.dtype == np.float32
    bits = set(vals.view(np.uint32).tolist())
    for e in (E.MID_LO, E.MID_HI, E.HIGH, E.LOW):
        e = f(e)
        for v in (np.nextafter(e, f(-1)), e, np.nextafter(e, f(2))):
            assert int(v.view(np.uint32)) in bits, v
    assert np.isnan(vals).any() and int(f(0.0).view(np.uint32)) in bits and int(f(-0.0).view(np.uint32)) in bits


@pytest.mark.parametrize("n_traj", D.N_TRAJ)
def test_families(n_traj):
    trajs = D.family(n_traj)
    assert len(trajs) == n_traj and D.family(n_traj) is trajs
    lens = np.array([len(a) for a in trajs])
    assert lens.min() == 0 and lens.max() <= D.MAX_LEN and set(lens.tolist()) == set(range(D.MAX_LEN + 1))
    assert all(a.dtype == np.float32 for a in trajs)
    vals = set(D.adversarial_values().view(np.uint32).tolist())
    assert all(set(a.view(np.uint32).tolist()) <= vals for a in trajs)
    assert np.isnan(np.concatenate(trajs)).any()
    runs = D.empty_runs(n_traj)
    assert len(runs) == {63: 1, 64: 1, 65: 1, 255: 2, 256: 2, 257: 2, 513: 3, 700: 4}[n_traj]
    for start, m in runs:                # several consecutive empty trajectories after a non-empty one, not the walk's last
        assert m >= 4 and all(lens[t] == 0 for t in range(start, start + m)) and lens[start - 1] > 0 and start + m < n_traj
    # single empty trajectories besides the runs
    in_runs = {t for s, m in runs for t in range(s, s + m)}
    assert any(lens[t] == 0 for t in range(n_traj) if t not in in_runs)


def test_the_cases_that_exist():
    assert sorted(D.CASES) == sorted(D.N_TRAJ)
    total = 0
    for n_traj in D.N_TRAJ:
        for collect in D.COLLECTS:
            for recon in FORMS:
                assert list(D.named_cuts(n_traj, collect, recon)) == D.CASES[n_traj], (n_traj, collect, recon)
                total += len(D.CASES[n_traj])
    assert [len(D.CASES[n]) for n in D.N_TRAJ] == [4, 4, 5, 7, 7, 9, 11, 11]
    assert total == 58 * 3 * 2


@pytest.mark.parametrize("recon", FORMS, ids=["plain", "recon"])
@pytest.mark.parametrize("n_traj", D.N_TRAJ)
def test_every_named_cut_lands_where_its_name_says(n_traj, recon):
    trajs = D.family(n_traj)
    for collect in D.COLLECTS:
        sizes_all, rows_all, counts_all = D.host_select(trajs, collect, 10 ** 9, recon)
        s_all = D.entry_weights(counts_all, recon)
        for name, total in D.named_cuts(n_traj, collect, recon).items():
            case = (n_traj, collect, recon, name, total)
            sizes, rows, counts = D.host_select(trajs, collect, total, recon)
            u = len(sizes)                                   # the first unvisited trajectory (n_traj: none)
            s = D.entry_weights(counts, recon)
            assert np.array_equal(s[:u], s_all[:u]) and not s[u:].any(), case
            if name == "never":
                assert u == n_traj and total == len(rows_all) + 1 and len(rows) == len(rows_all), case
            elif name == "at_empty_run":
                start, m = D.empty_runs(n_traj)[-1]
                assert u == start and len(rows) == total and s[u - 1] > 0, case       # reached exactly, by the one before the run
                assert m >= 4 and all(len(trajs[t]) == 0 for t in range(u, u + m)) and u + m < n_traj, case
                assert sizes_all[u] == sizes_all[u + m] == total, case                # every empty one sees len(dset) == total
            else:
                lo, hi = D.WHERE[name]
                assert lo <= u < hi, case
            if name == "zero":
                assert total == 0 and rows == [], case
                continue
            if name == "first":
                assert total == 1 and u == 1, case
            if name == "round_edge_exact":
                assert total == sizes_all[D.ROUND] and len(rows) == total and s[D.ROUND - 1] > 0, case
            if name == "round_edge_plus1":
                assert total == sizes_all[D.ROUND] + 1 and s[D.ROUND] > 0 and sizes[-1] == total - 1, case
            if name.startswith("wave") or name in ("round1", "round2"):
                assert u < n_traj and sizes[u - 1] == total - 1 and s[u - 1] >= 1, case      # one entry into trajectory u - 1
            # every wave of 64 trajectories that starts before the cut has a visited trajectory that selects something
            for w0 in range(0, u, D.WAVE):
                assert s[w0:min(w0 + D.WAVE, u)].sum() > 0, (case, w0)
            # entries of every weight before the cut (recon: a mid frame is two entries)
            if recon:
                kinds = {}
                for t, i, k in rows:
                    kinds.setdefault((t, i), []).append(k)
                assert any(v == [0, 1] for v in kinds.values()) and any(len(v) == 1 for v in kinds.values()), case
                assert counts[:, 0].sum() > 0 and counts[:, 1:].sum() > 0, case


def test_some_cut_overshoots_total_images():
    """The reference adds a visited trajectory's whole selection: some wave / round cut ends with more entries than asked."""
    over = 0
    for n_traj in D.N_TRAJ:
        for recon in FORMS:
            for name, total in D.named_cuts(n_traj, 2, recon).items():
                over += len(D.host_select(D.family(n_traj), 2, total, recon)[1]) > total
    assert over >= 20


def test_chunk_bounds():
    for n_traj in D.N_TRAJ:
        b = D.chunk_bounds(n_traj)
        sizes = np.diff(b)
        assert b[0] == 0 and b[-1] == n_traj and len(b) == 4 and (sizes > 0).all()
        assert sizes.min() < D.WAVE
        if n_traj >= 513:
            assert sizes.max() > D.ROUND
        elif n_traj >= 255:
            assert sizes.max() > D.WAVE


@pytest.mark.parametrize("recon", FORMS, ids=["plain", "recon"])
def test_expected_chunks_restate_the_whole_walk(recon):
    """The per-call arrays put together are the restatement's walk; a walk entered at running0 is the same walk shifted."""
    n_traj, collect = 513, 2
    trajs = D.family(n_traj)
    for name, total in D.named_cuts(n_traj, collect, recon).items():
        sizes, rows, counts = D.host_select(trajs, collect, total, recon)
        for bounds in ([0, n_traj], D.chunk_bounds(n_traj)):
            for r0 in (0, 2 ** 33 + 3):
                ch = D.expected_chunks(trajs, collect, total + r0, bounds, recon, running0=r0)
                assert len(ch) == len(bounds) - 1
                first = np.concatenate([c["first"] for c in ch])
                assert first.tolist() == [r0 + v for v in sizes] + [-1] * (n_traj - len(sizes)), (name, bounds)
                assert np.array_equal(np.concatenate([c["counts"] for c in ch]), counts)
                assert ch[-1]["running"] == r0 + len(rows)
                got, run = [], r0
                lens = [len(a) for a in trajs]
                for c, b0, b1 in zip(ch, bounds[:-1], bounds[1:]):
                    offs = np.concatenate([[0], np.cumsum(lens[b0:b1])])
                    assert c["span"][0] == run and c["span"][1] == len(c["ent_frame"])
                    run += int(c["span"][1])
                    assert c["running"] == run
                    tr = np.searchsorted(offs, c["ent_frame"], side="right") - 1
                    rel = [(int(b0 + a), int(p - offs[a])) for a, p in zip(tr, c["ent_frame"])]
                    if recon:
                        assert c["span"][2] == len(c["sel"]) == c["counts"].sum()
                        assert np.array_equal(c["sel"][c["ent_sel"]], c["ent_frame"]) and (np.diff(c["sel"]) > 0).all()
                        rel = [(t, i, int(k)) for (t, i), k in zip(rel, c["ent_kind"])]
                    got += rel
                assert got == rows, (name, bounds)


def test_entered_past_the_cut_nothing_is_visited():
    trajs = D.family(257)
    for recon in FORMS:
        for r0, total in ((50, 50), (51, 50)):
            for c in D.expected_chunks(trajs, 2, total, D.chunk_bounds(257), recon, running0=r0):
                assert (c["first"] == -1).all() and not c["counts"].any() and c["running"] == r0
                assert c["span"].tolist() == [r0, 0] + ([0] if recon else []) and len(c["ent_frame"]) == 0
