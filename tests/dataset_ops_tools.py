"""What tests/test_gpu_dataset_ops.py stands on, and what tests/test_host_dataset_ops_tools.py proves about it on the CPU.

curate_cut_kernel (dataset.hip) scans the trajectories of a chunk through ONE workgroup of 256 threads: a shuffle scan per wave
of 64, the wave totals through LDS, a carry between rounds of 256 trajectories, then a backward search for the last visited one.
The families here are walks with many short trajectories, so that the cut lands in a chosen wave or round:

  family(n_traj)                       n_traj trajectories of 0 .. 6 critic values out of the adversarial value set (bin edges
                                       +- 1 ulp, NaN, +-0), with runs of consecutive empty trajectories
  named_cuts(n_traj, collect, recon)   {name: total_images}: where the name says the first unvisited trajectory lies
  chunk_bounds(n_traj)                 the walk in three calls
  expected_chunks(...)                 per call, every output array of cvae_curate_select / cvae_curate_select_recon as the plain
                                       restatement (episodes.select_host / select_recon_host) gives it
  device_select / device_select_recon  the walk on the device (also used by test_gpu_episodes.py and test_gpu_recon.py)

Only the two device_* functions touch the GPU."""
import functools

import numpy as np
import torch

from critic_vae_amd import episodes as E

DEV = torch.device("cuda:0")
FILL = -7                                    # what every output holds before a call

N_TRAJ = (63, 64, 65, 255, 256, 257, 513, 700)
COLLECTS = (1, 2, 100)
MAX_LEN = 6
WAVE, ROUND = 64, 256                        # trajectories per wave and per round of curate_cut_kernel (TPB = 256)
# (first trajectory, length) of the runs of empty trajectories: inside wave 0, across the wave 1 / 2 edge, inside round 1,
# across the round 1 / 2 edge.  A family holds those that end before its last trajectory.
EMPTY_RUNS = ((30, 4), (126, 4), (300, 5), (510, 5))
# the cases each family must have (the builder leaves out what cannot exist: no wave 1 below 65 trajectories, ...)
CASES = {
    63: ["never", "zero", "first", "at_empty_run"],
    64: ["never", "zero", "first", "at_empty_run"],
    65: ["never", "zero", "first", "wave1", "at_empty_run"],
    255: ["never", "zero", "first", "wave1", "wave2", "wave3", "at_empty_run"],
    256: ["never", "zero", "first", "wave1", "wave2", "wave3", "at_empty_run"],
    257: ["never", "zero", "first", "wave1", "wave2", "wave3", "round_edge_exact", "round_edge_plus1", "at_empty_run"],
    513: ["never", "zero", "first", "wave1", "wave2", "wave3", "round_edge_exact", "round_edge_plus1", "round1", "round2", "at_empty_run"],
    700: ["never", "zero", "first", "wave1", "wave2", "wave3", "round_edge_exact", "round_edge_plus1", "round1", "round2", "at_empty_run"],
}
# where the first unvisited trajectory of a named cut lies: [lo, hi) (None: given by the family, see the host test)
WHERE = {"zero": (0, 1), "first": (1, 2), "wave1": (64, 128), "wave2": (128, 192), "wave3": (192, 256),
         "round_edge_exact": (256, 257), "round_edge_plus1": (257, 258), "round1": (257, 512), "round2": (512, 10 ** 9)}


def adversarial_values():
    """The value set of _adversarial_trajectories (test_gpu_episodes.py, test_gpu_recon.py)."""
    f = np.float32
    edges = [f(0.4), f(0.6), f(0.7), f(0.25)]
    vals = [v for e in edges for v in (np.nextafter(e, f(-1)), e, np.nextafter(e, f(2)))]
    vals += [f("nan"), f(0.0), f(-0.0), f(1.0), f(0.5), f(0.9), f(0.1), f(0.65)]
    return np.array(vals, np.float32)


def empty_runs(n_traj):
    return [(s, m) for s, m in EMPTY_RUNS if s + m < n_traj]


@functools.lru_cache(maxsize=None)
def family(n_traj):
    """n_traj trajectories (a tuple of float32 arrays; treat as read-only).  Trajectory 0 holds a mid, a high and a low value;
    the trajectory before every empty run and trajectories 63, 255, 256 and 511 (where no empty run covers them) select at
    least one frame."""
    rng = np.random.default_rng(1000 + n_traj)
    vals = adversarial_values()
    binned = np.array([0.5, 0.9, 0.1], np.float32)

    def selecting():
        return np.concatenate([rng.choice(binned, size=1), rng.choice(vals, size=int(rng.integers(0, MAX_LEN)))]).astype(np.float32)

    trajs = [rng.choice(vals, size=int(n)).astype(np.float32) for n in rng.integers(0, MAX_LEN + 1, size=n_traj)]
    trajs[0] = np.concatenate([binned, rng.choice(vals, size=2)]).astype(np.float32)
    for t in (WAVE - 1, ROUND - 1, ROUND, 2 * ROUND - 1):     # so that a cut can land on trajectory 64, 256, 257, 512
        if t < n_traj:
            trajs[t] = selecting()
    for start, m in empty_runs(n_traj):
        trajs[start - 1] = selecting()
        for t in range(start, start + m):
            trajs[t] = np.zeros(0, np.float32)
    return tuple(trajs)


def host_select(trajs, collect, total_images, recon):
    fn = E.select_recon_host if recon else E.select_host
    return fn(list(trajs), collect=collect, total_images=total_images)


def entry_weights(counts, recon):
    """Dataset entries per trajectory out of its (mid, high, low) frame counts."""
    counts = np.asarray(counts, np.int64).reshape(-1, 3)
    return (2 if recon else 1) * counts[:, 0] + counts[:, 1] + counts[:, 2]


@functools.lru_cache(maxsize=None)
def named_cuts(n_traj, collect, recon):
    """{name: total_images} in the order of CASES[n_traj]; a case that cannot exist for this family is left out."""
    trajs = family(n_traj)
    sizes, rows, counts = host_select(trajs, collect, 10 ** 9, recon)
    s = entry_weights(counts, recon)
    before = list(sizes) + [len(rows)]                    # len(dset) before trajectory t; [n_traj] = the whole walk
    assert len(sizes) == n_traj

    def inside(lo, hi):
        """A cut after which the first unvisited trajectory u lies in [lo, hi): one entry into trajectory u - 1's selection,
        preferably of one that selects more than that (the reference then overshoots total_images)."""
        hi = min(hi, n_traj)
        order = list(range((lo + hi) // 2, hi)) + list(range(lo, (lo + hi) // 2))
        for need in (2, 1):
            for u in order:
                if u >= 1 and s[u - 1] >= need:
                    return before[u - 1] + 1
        return None

    cuts = {"never": len(rows) + 1, "zero": 0, "first": 1}
    for name in ("wave1", "wave2", "wave3"):
        cuts[name] = inside(*WHERE[name])
    if n_traj > ROUND:                                    # trajectories 255 and 256 select something (family)
        cuts["round_edge_exact"] = before[ROUND]
        cuts["round_edge_plus1"] = before[ROUND] + 1
    cuts["round1"] = inside(*WHERE["round1"])
    cuts["round2"] = inside(*WHERE["round2"])
    runs = empty_runs(n_traj)
    if runs:
        cuts["at_empty_run"] = before[runs[-1][0]]        # reached by the trajectory before the run
    return {k: int(v) for k, v in cuts.items() if v is not None}


def chunk_bounds(n_traj):
    """The walk in three calls: from 513 trajectories on one call has fewer than 64 and one more than 256 trajectories;
    below that (no three calls can have both) a short, a long and a middle one."""
    if n_traj >= 2 * ROUND + 1:
        return [0, 40, 340, n_traj]
    return [0, n_traj // 5, n_traj // 5 + n_traj // 2, n_traj]


def expected_chunks(trajs, collect, total_images, bounds, recon, running0=0):
    """Per call c over trajectories bounds[c] .. bounds[c + 1]: dict(first, counts, span, running, ent_frame, and for the recon
    form ent_kind, ent_sel, sel, sel_first) as the restatement gives them.  ent_frame is `sel` of the plain form.  A walk that
    starts at running0 entries is the restatement's walk towards total_images - running0, shifted."""
    sizes, rows, counts = host_select(trajs, collect, total_images - running0, recon)
    lens = [len(a) for a in trajs]
    out, r = [], 0
    for c in range(len(bounds) - 1):
        b0, b1 = int(bounds[c]), int(bounds[c + 1])
        offs = np.concatenate([[0], np.cumsum(lens[b0:b1])]).astype(np.int64)
        r1 = r
        while r1 < len(rows) and rows[r1][0] < b1:
            r1 += 1
        mine = rows[r:r1]
        ent_frame = np.array([offs[row[0] - b0] + row[1] for row in mine], np.int64)
        cn = counts[b0:b1]
        exp = dict(first=np.array([running0 + sizes[t] if t < len(sizes) else -1 for t in range(b0, b1)], np.int64),
                   counts=cn, ent_frame=ent_frame, running=running0 + r1)
        if recon:
            sel = []
            ent_sel = np.zeros(len(mine), np.int64)
            for e, p in enumerate(ent_frame):
                if not sel or sel[-1] != p:                 # the two entries of a mid frame are neighbours
                    sel.append(int(p))
                ent_sel[e] = len(sel) - 1
            visited = exp["first"] >= 0
            prefix = np.concatenate([[0], np.cumsum(cn.sum(1))[:-1]]) if b1 > b0 else np.zeros(0, np.int64)
            exp.update(ent_kind=np.array([row[2] for row in mine], np.int32), ent_sel=ent_sel, sel=np.array(sel, np.int64),
                       sel_first=np.where(visited, prefix, -1).astype(np.int64),
                       span=np.array([running0 + r, len(mine), len(sel)], np.int64))
        else:
            exp["span"] = np.array([running0 + r, len(mine)], np.int64)
        out.append(exp)
        r = r1
    return out


# ---- the walk on the device ----

def _bounds(n_traj, n_chunks, bounds):
    return np.linspace(0, n_traj, n_chunks + 1).round().astype(int) if bounds is None else np.asarray(bounds, int)


def device_select(h, trajs, collect, total_images, n_chunks, bounds=None, running0=0, raw=None):
    """The walk in n_chunks calls of cvae_curate_select, the running count carried on the device; returns the
    selected (t, i), first and counts of every trajectory.  bounds: the calls' trajectory bounds instead of n_chunks even
    ones; running0: the count on entry; raw: a list that receives per call every output array whole (numpy)."""
    bounds = _bounds(len(trajs), n_chunks, bounds)
    running = torch.full((1,), running0, dtype=torch.int64, device=DEV)
    span = torch.zeros(2, dtype=torch.int64, device=DEV)
    selected, first, counts = [], [], []
    for c in range(len(bounds) - 1):
        ts = list(range(bounds[c], bounds[c + 1]))
        lens = [len(trajs[t]) for t in ts]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        preds = torch.from_numpy(np.concatenate([trajs[t] for t in ts]) if ts else np.zeros(0, np.float32)).to(DEV)
        n = preds.numel()
        sel = torch.full((max(n, 1),), FILL, dtype=torch.int64, device=DEV)
        d_counts = torch.full((len(ts), 3), FILL, dtype=torch.int64, device=DEV)
        d_first = torch.full((len(ts),), FILL, dtype=torch.int64, device=DEV)
        h.curate_select(torch.from_numpy(offs).to(DEV), preds, collect, total_images, running, d_counts, d_first, span, sel)
        sp = span.cpu().numpy()
        picked = sel[:int(sp[1])].cpu().numpy()
        tr = np.searchsorted(offs, picked, side="right") - 1
        selected += [(ts[a], int(p - offs[a])) for a, p in zip(tr, picked)]
        first += d_first.cpu().tolist()
        counts += d_counts.cpu().tolist()
        assert sp[0] + sp[1] == int(running.item())
        if raw is not None:
            raw.append(dict(first=d_first.cpu().numpy(), counts=d_counts.cpu().numpy(), span=sp.copy(), running=int(running.item()),
                            ent_frame=sel.cpu().numpy()))
    return selected, first, np.array(counts, np.int64).reshape(-1, 3), int(running.item())


def device_select_recon(h, trajs, collect, total_images, n_chunks, bounds=None, running0=0, raw=None):
    """device_select for cvae_curate_select_recon: returns the entries (t, i, kind), first and counts; checks per call that
    the selected frames are in walk order, each once, that every entry points at its own frame, and sel_first."""
    bounds = _bounds(len(trajs), n_chunks, bounds)
    running = torch.full((1,), running0, dtype=torch.int64, device=DEV)
    span = torch.zeros(3, dtype=torch.int64, device=DEV)
    entries, first, counts = [], [], []
    for c in range(len(bounds) - 1):
        ts = list(range(bounds[c], bounds[c + 1]))
        lens = [len(trajs[t]) for t in ts]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        preds = torch.from_numpy(np.concatenate([trajs[t] for t in ts]) if ts else np.zeros(0, np.float32)).to(DEV)
        n = preds.numel()
        full = lambda m, dt=torch.int64: torch.full((max(m, 1),), FILL, dtype=dt, device=DEV)          # noqa: E731
        sel, ent_frame, ent_sel, ent_kind = full(n), full(2 * n), full(2 * n), full(2 * n, torch.int32)
        d_counts = torch.full((len(ts), 3), FILL, dtype=torch.int64, device=DEV)
        d_first, d_sfirst = full(len(ts))[:len(ts)], full(len(ts))[:len(ts)]
        h.curate_select_recon(torch.from_numpy(offs).to(DEV), preds, collect, total_images, running, d_counts, d_first,
                              d_sfirst, span, ent_frame, ent_kind, ent_sel, sel)
        e0, ne, ns = span.cpu().tolist()
        ef, ek, es = ent_frame[:ne].cpu().numpy(), ent_kind[:ne].cpu().numpy(), ent_sel[:ne].cpu().numpy()
        fs = sel[:ns].cpu().numpy()
        tr = np.searchsorted(offs, ef, side="right") - 1
        entries += [(ts[a], int(p - offs[a]), int(k)) for a, p, k in zip(tr, ef, ek)]
        # the per-selected-frame index: frames in walk order, each once, and every entry points at its own frame
        assert np.all(np.diff(fs) > 0) and np.array_equal(fs[es], ef) and len(set(ef.tolist())) == ns
        sf, cn = d_sfirst.cpu().numpy(), d_counts.cpu().numpy()
        want_sf = np.where(d_first.cpu().numpy() >= 0, np.concatenate([[0], np.cumsum(cn.sum(1))[:-1]]) if len(ts) else [], -1)
        assert np.array_equal(sf, want_sf)
        first += d_first.cpu().tolist()
        counts += cn.tolist()
        assert e0 + ne == int(running.item())
        if raw is not None:
            raw.append(dict(first=d_first.cpu().numpy(), counts=cn, span=np.array([e0, ne, ns], np.int64), running=int(running.item()),
                            ent_frame=ent_frame.cpu().numpy(), ent_kind=ent_kind.cpu().numpy(), ent_sel=ent_sel.cpu().numpy(),
                            sel=sel.cpu().numpy(), sel_first=sf))
    return entries, first, np.array(counts, np.int64).reshape(-1, 3), int(running.item())
