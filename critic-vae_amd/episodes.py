"""The reference's training set from recorded trajectories (load_minerl_data(critic), vae_utility.py:393-461, non-recon
branch), curated on the device and kept there for the training loop.

A trajectory is one `.npy` file of uint8 frames (T, w, w, 3) — MineRL's `pov` observations, and the reference's own
`minerl-episode/X.npy` format (segment.load_episode).  The selection rule (include/cvae.h, "The training set on the
device"): trajectories in the reference's order (np.random.default_rng(seed=0).shuffle of the name list; here the sorted
file names), frames in order, p = the critic value of preprocess_observation(frame); bins mid 0.4 <= p <= 0.6, then high
p >= 0.7, then low p <= 0.25, compared in float32; at most `collect` frames per bin and trajectory; the walk stops before a
trajectory once len(dset) >= total_images.

    eps = load_episodes(["episodes/"])                       # (name, memory-mapped array) pairs, sorted by name
    ds = curate(eps, critic)                                 # DeviceDataset: frames (N,w,w,3) uint8 + preds (N,1) on the GPU
    FusedTrainer(vae).fit_device(ds, batch_size=128, epochs=7)

The recon branch of the same function (load_minerl_data(critic, recon_dset=True, vae=vae), vae_utility.py:422-443) builds
the dataset of the SECOND VAE: instead of the frame, the first VAE's eval-mode reconstructions vae.evaluate(obs, p) and / or
vae.evaluate(obs, 0) — two entries for a mid frame, one for a high (at p) or low (at 0) frame:

    rd = curate_recon(eps, critic, vae)                      # ReconDataset: frames (N,3,w,w) fp32 + preds (N,1) on the GPU
    FusedTrainer(vae2).fit_device(rd, batch_size=128, epochs=7)
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import params as P
from .critic import Critic
from .feeder import StagingSet
from .lib import Handle

# bin edges as the reference compares them: a float32 tensor against a Python float, in float32
MID_LO, MID_HI = np.float32(P.bin_mid[0]), np.float32(P.bin_mid[1])
HIGH, LOW = np.float32(P.bin_high), np.float32(P.bin_low)
CURATE_PIECE = 1024          # frames per critic launch during curation (the curation handle's max_batch)


def value_bins(values):
    """The bin of every critic value (or target), as the selection walk and cvae_critic_score assign it: 0 = mid
    (MID_LO <= v <= MID_HI), 1 = high (v >= HIGH), 2 = low (v <= LOW), 3 = none; tested in that order, the value taken to
    float32 and compared against the float32 edges; NaN falls in no bin.  Returns int64 of the input's shape."""
    v = np.asarray(values, np.float32)
    mid = (v >= MID_LO) & (v <= MID_HI)
    return np.where(mid, 0, np.where(v >= HIGH, 1, np.where(v <= LOW, 2, 3))).astype(np.int64)


def load_episodes(paths, width=P.w):
    """`.npy` files, or directories of them (not recursive): one trajectory (T, width, width, 3) uint8 per file.
    Returns [(name, array)] sorted by name (the file name without `.npy`); arrays are memory-mapped.
    ValueError for a wrong dtype, rank, channel count or width, or for two files of the same name."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    files = []
    for p in paths:
        p = os.fspath(p)
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in os.listdir(p) if f.endswith(".npy")]
        elif os.path.isfile(p):
            files.append(p)
        else:
            raise FileNotFoundError(p)
    out = {}
    for f in files:
        name = os.path.basename(f)[:-4] if f.endswith(".npy") else os.path.basename(f)
        if name in out:
            raise ValueError(f"two trajectories named {name!r}")
        a = np.load(f, mmap_mode="r")
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3 or a.shape[1] != width or a.shape[2] != width:
            raise ValueError(f"{f}: a trajectory must be uint8 (T, {width}, {width}, 3), got {a.dtype} {a.shape}")
        out[name] = a
    return sorted(out.items())


def reference_order(names, seed=0):
    """The reference's visiting order: np.random.default_rng(seed=0).shuffle of the name list (vae_utility.py:400-402)."""
    names = list(names)
    np.random.default_rng(seed=seed).shuffle(names)
    return names


def _select_walk(traj_preds, collect, total_images, mid, high, low):
    """vae_utility.py:406-459 in plain Python over critic values (float32 comparisons, as torch makes them).  mid / high /
    low (t, i) -> the dataset rows a kept frame of that bin appends; len(dset) — the cut and the sizes — counts rows."""
    sizes, rows = [], []
    counts = np.zeros((len(traj_preds), 3), np.int64)
    for t, preds in enumerate(traj_preds):
        if len(rows) >= total_images:
            break
        sizes.append(len(rows))
        c_high = c_mid = c_low = 0
        for i, pred in enumerate(np.asarray(preds, np.float32).reshape(-1)):
            if c_high >= collect and c_low >= collect and c_mid >= collect:
                break
            elif MID_LO <= pred <= MID_HI and c_mid < collect:
                rows += mid(t, i)
                c_mid += 1
            elif pred >= HIGH and c_high < collect:
                rows += high(t, i)
                c_high += 1
            elif pred <= LOW and c_low < collect:
                rows += low(t, i)
                c_low += 1
        counts[t] = (c_mid, c_high, c_low)
    return sizes, rows, counts


def select_host(traj_preds, collect=P.collect, total_images=P.total_images):
    """vae_utility.py:406-459 restated in plain Python over critic values (float32 comparisons, as torch makes them).
    traj_preds: per visited-order trajectory, its frames' critic values.  Returns (sizes, selected, counts):
    sizes = len(dset) before each visited trajectory (the reference's `total images = ...` prints), selected = [(t, i)]
    in dataset order, counts (T, 3) int64 = frames taken per bin (mid, high, low), 0 for trajectories never visited."""
    def frame(t, i):
        return [(t, i)]
    return _select_walk(traj_preds, collect, total_images, frame, frame, frame)


def select_recon_host(traj_preds, collect=P.collect, total_images=P.total_images):
    """The recon branch, vae_utility.py:406-443, restated like select_host: a mid frame appends two entries (kind 0 = decoded
    at its critic value, then kind 1 = decoded at 0) and counts once against the mid cap, a high frame one entry of kind 0, a
    low frame one of kind 1; len(dset) — the cut and the sizes — counts entries.  Returns (sizes, entries, counts): entries =
    [(t, i, kind)] in dataset order, counts (T, 3) = FRAMES taken per bin."""
    return _select_walk(traj_preds, collect, total_images, lambda t, i: [(t, i, 0), (t, i, 1)],
                        lambda t, i: [(t, i, 0)], lambda t, i: [(t, i, 1)])


class _CuratedDataset:
    """What DeviceDataset and ReconDataset share: preds beside the frames, source (N, SOURCE_COLS), names / sizes / counts."""

    def __init__(self, frames, preds, source, names, sizes, counts):
        if not (preds.is_cuda and preds.dtype == torch.float32 and tuple(preds.shape) == (frames.shape[0], 1)
                and preds.is_contiguous()):
            raise ValueError("preds must be a contiguous fp32 device tensor (N, 1)")
        self.frames, self.preds = frames, preds
        self.source = np.asarray(source, np.int64).reshape(-1, self.SOURCE_COLS)
        self.names, self.sizes = list(names), list(sizes)
        self.counts = np.zeros((0, 3), np.int64) if counts is None else np.asarray(counts, np.int64)

    def __len__(self):
        return self.frames.shape[0]


class DeviceDataset(_CuratedDataset):
    """A training set on the device: frames (N, w, w, 3) uint8, preds (N, 1) fp32 (the critic's value of every frame),
    source (N, 2) int64 host array (trajectory, frame).  curate() also fills `names` (visited trajectories, in order),
    `sizes` (len(dset) before each) and `counts` (per visited trajectory, frames per bin mid / high / low)."""
    SOURCE_COLS = 2

    def __init__(self, frames, preds, source, names=(), sizes=(), counts=None):
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3
                and frames.shape[1] == frames.shape[2] and frames.is_contiguous()):
            raise ValueError("frames must be a contiguous uint8 device tensor (N, w, w, 3)")
        super().__init__(frames, preds, source, names, sizes, counts)

    @property
    def width(self):
        return self.frames.shape[1]

    def gather(self, handle, nb, idx, x, pred, aug=None, applied=None):
        """One training batch: x = frames[idx] / 255 as CHW fp32, pred = preds[idx] (cvae_preprocess_u8_gather).  aug: the
        values of augment.Augment.at(draw) — the batch then comes from cvae_preprocess_u8_gather_aug (still one launch), and
        applied (nb, 4) int32 receives what was drawn per row."""
        if aug is None:
            if applied is not None:
                raise ValueError("applied needs aug: the plain gather draws nothing")
            handle.preprocess_u8_gather(nb, self.frames, self.preds, idx, x, pred)
        else:
            handle.preprocess_u8_gather_aug(nb, self.frames, self.preds, idx, aug, x, pred, applied)

    @classmethod
    def from_host(cls, frames_u8, critic=None, device="cuda:0"):
        """From host uint8 frames (N, w, w, 3), w = 64 or 128.  critic: None (preds = 0), a Critic (its values, computed
        on the device; 64x64 only), or the preds themselves (N or (N, 1) values)."""
        frames_u8 = np.ascontiguousarray(frames_u8)
        if frames_u8.dtype != np.uint8 or frames_u8.ndim != 4 or frames_u8.shape[3] != 3 or frames_u8.shape[1] != frames_u8.shape[2]:
            raise ValueError(f"frames must be uint8 (N, w, w, 3), got {frames_u8.dtype} {frames_u8.shape}")
        n = frames_u8.shape[0]
        frames = torch.from_numpy(frames_u8).to(device)
        if critic is None:
            preds = torch.zeros(n, 1, device=device)
        elif isinstance(critic, Critic):
            preds = torch.empty(n, 1, device=device)
            _critic_values(critic, frames, preds)
        else:
            preds = torch.as_tensor(np.asarray(critic, np.float32).reshape(n, 1)).to(device)
        source = np.stack([np.zeros(n, np.int64), np.arange(n, dtype=np.int64)], 1)
        return cls(frames, preds, source)


def split_indices(source, fraction, seed=0):
    """The index logic of split_by_trajectory on a host `source` array (N, >= 2) whose column 0 is the trajectory:
    (train rows, val rows, val trajectories), rows in dataset order.  Trajectories are taken in the order of
    np.random.default_rng(seed).permutation over the sorted trajectory indices until val holds at least fraction * N rows."""
    source = np.asarray(source, np.int64)
    if source.ndim != 2 or source.shape[1] < 2:
        raise ValueError("source must be (N, >= 2): trajectory, frame, ...")
    if not 0.0 < float(fraction) < 1.0:
        raise ValueError(f"fraction {fraction!r} must lie in (0, 1)")
    traj = source[:, 0]
    ids, per = np.unique(traj, return_counts=True)
    if ids.size < 2:
        raise ValueError(f"a split by trajectory needs at least two trajectories, the dataset has {ids.size}")
    order = np.random.default_rng(seed).permutation(ids.size)
    need, have, taken = float(fraction) * traj.size, 0, []
    for k in order:
        if have >= need:
            break
        taken.append(int(ids[k]))
        have += int(per[k])
    if have == traj.size:
        raise ValueError(f"holding out {fraction} of {traj.size} entries by whole trajectories leaves no training entry")
    in_val = np.isin(traj, np.asarray(taken, np.int64))
    return np.flatnonzero(~in_val), np.flatnonzero(in_val), sorted(taken)


def subset_meta(source, names, sizes, counts, rows):
    """Host bookkeeping of a subset of whole trajectories: (source, names, sizes, counts) of the entries `rows` (ascending
    host indices).  names / sizes / counts keep the visited trajectories whose entries stayed, in their order, with sizes =
    entries of the subset before each; a visited trajectory that contributed no entry belongs to neither half and is dropped."""
    rows = np.asarray(rows, np.int64)
    source = np.asarray(source, np.int64)
    out_names, out_sizes, out_counts = [], [], []
    for j, start in enumerate(sizes):
        end = sizes[j + 1] if j + 1 < len(sizes) else len(source)
        k = int(np.searchsorted(rows, start))
        if end <= start or k >= rows.size or rows[k] != start:
            continue
        out_names.append(names[j])
        out_sizes.append(k)
        if len(counts) > j:
            out_counts.append(counts[j])
    return source[rows], out_names, out_sizes, np.asarray(out_counts, np.int64).reshape(-1, 3)


def _subset(dataset, rows):
    """`dataset` restricted to `rows`: the same class, frames / preds copied on the device, bookkeeping by subset_meta."""
    rows = np.asarray(rows, np.int64)
    idx = torch.from_numpy(rows).to(dataset.frames.device)
    source, names, sizes, counts = subset_meta(dataset.source, dataset.names, dataset.sizes, dataset.counts, rows)
    kw = dict(names=names, sizes=sizes, counts=counts if len(counts) else None)
    if isinstance(dataset, ReconDataset):
        kw["stats"] = dataset.stats
    return type(dataset)(dataset.frames[idx].contiguous(), dataset.preds[idx].contiguous(), source, **kw)


def split_by_trajectory(dataset, fraction, seed=0):
    """(train, val) of a DeviceDataset or ReconDataset, each of the dataset's own class.  WHOLE trajectories are held out:
    consecutive frames of a trajectory are near-duplicates, so a split by frame would put a validation frame's neighbours in
    the training set and the held-out loss would measure memorisation.  Trajectories are taken in a seeded order
    (split_indices) until val holds at least `fraction` of the entries; no trajectory index appears in both halves.
    ValueError for fewer than two trajectories, a fraction outside (0, 1) or an empty half."""
    tr, va, _ = split_indices(dataset.source, fraction, seed)
    return _subset(dataset, tr), _subset(dataset, va)


def _critic_values(critic, frames_u8, out, handle=None, x=None):
    """out[i] = critic.evaluate(preprocess_observation(frames_u8[i])) on the device, in pieces of the handle's max_batch."""
    if frames_u8.shape[1] != 64:
        raise ValueError("the critic is 64x64 only (critic_net.py)")
    h = handle or Handle(64, CURATE_PIECE)
    if x is None:
        x = torch.empty(h.max_batch, 3, 64, 64, device=frames_u8.device)
    for p in range(0, frames_u8.shape[0], h.max_batch):
        nb = min(h.max_batch, frames_u8.shape[0] - p)
        h.preprocess_u8(nb, frames_u8[p:p + nb], x[:nb])
        h.critic_forward(nb, x[:nb], critic.flat, out[p:p + nb])


def _chunks(lengths, chunk_frames):
    """Consecutive runs of trajectories of at most chunk_frames frames (a longer trajectory is a chunk of its own)."""
    out, cur, n = [], [], 0
    for t, L in enumerate(lengths):
        if cur and n + L > chunk_frames:
            out.append(cur)
            cur, n = [], 0
        cur.append(t)
        n += L
    if cur:
        out.append(cur)
    return out


class _PlainPlan:
    """What curate() adds to the walk: one uint8 entry per kept frame, gathered out of the chunk on the device."""
    who, per_frame, per_traj, x_rows = "curate", 1, 3, 0        # a trajectory adds at most per_traj * collect entries

    def validate(self, device):
        pass

    def allocate(self, cap, biggest, device):
        self.frames = torch.empty(max(cap, 1), 64, 64, 3, dtype=torch.uint8, device=device)
        self.preds = torch.empty(max(cap, 1), 1, device=device)
        self.sel = torch.empty(biggest, dtype=torch.int64, device=device)
        self.span = torch.zeros(2, dtype=torch.int64, device=device)

    def enqueue(self, w, ch):
        w.h.curate_select(ch.d_offs, w.cpred[:ch.n], w.collect, w.total_images, w.running, ch.d_counts, ch.d_first, self.span,
                          self.sel)
        if ch.n:
            w.h.gather_frames_u8(ch.set.dev, w.cpred, self.sel, ch.n, self.span, self.frames, self.preds)
        ch.set.release(w.stream)

    def collect(self, w, ch):
        sp = self.span.cpu().numpy()
        return int(sp[0] + sp[1]), self.sel[:int(sp[1])].cpu().numpy(), []

    def summary(self, n, n_traj, tot):
        return f"dataset: {n} frames from {n_traj} trajectories (mid {tot[0]}, high {tot[1]}, low {tot[2]})"

    def dataset(self, n, source, names, sizes, counts):
        return DeviceDataset(self.frames[:n], self.preds[:n], source, names, sizes, counts)


def _walk(plan, episodes, critic, collect, total_images, chunk_frames, order, device, log):
    """The walk of curate() and curate_recon().  Per chunk: the critic pass, plan.enqueue (the selection and what needs no host
    read), the staging of the next chunk, plan.collect (the host reads and what they size) -> (len(dset) after the chunk, the
    chunk frame index of every new entry, further source columns), the per-trajectory records and the cut."""
    if not isinstance(critic, Critic):
        raise TypeError(f"{plan.who} needs a critic_vae_amd.critic.Critic (the HIP critic)")
    if collect < 1 or total_images < 0:
        raise ValueError(f"collect {collect} must be >= 1 and total_images {total_images} >= 0")
    device = torch.device(device)
    plan.validate(device)
    episodes = list(episodes)
    by_name = {}
    for pos, (name, a) in enumerate(episodes):
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 4 and a.shape[1:] == (64, 64, 3)):
            raise ValueError(f"trajectory {name!r}: curation needs uint8 (T, 64, 64, 3) frames (the critic is 64x64 only)")
        by_name[name] = pos
    names = reference_order([n for n, _ in episodes]) if order is None else list(order)
    walk = [by_name[n] for n in names]
    lengths = [episodes[p][1].shape[0] for p in walk]
    # the cut overshoots by at most per_traj * collect - 1 entries, and no walk selects more than the trajectories can yield
    cap = min(total_images - 1 + plan.per_traj * collect, plan.per_frame * sum(lengths)) if total_images > 0 else 0
    log("loading episodes...")
    if total_images == 0 or not walk:
        plan.allocate(0, 1, device)
        return plan.dataset(0, [], [], [], None)

    chunks = _chunks(lengths, chunk_frames)
    biggest = max(max(sum(lengths[t] for t in c) for c in chunks), 1)
    plan.allocate(cap, biggest, device)
    w = SimpleNamespace(h=Handle(64, CURATE_PIECE), critic=critic, collect=collect, total_images=total_images, cap=cap,
                        x=torch.empty(max(CURATE_PIECE, plan.x_rows), 3, 64, 64, device=device),
                        cpred=torch.empty(biggest, device=device),
                        running=torch.zeros(1, dtype=torch.int64, device=device),
                        stream=torch.cuda.current_stream(device))
    copy_stream = torch.cuda.Stream(device=device)
    sets = [StagingSet(biggest, 64, device, copy_stream) for _ in range(2)]

    def rows_of(c):
        def fill(pin):
            n = 0
            for t in c:
                a = episodes[walk[t]][1]
                pin[n:n + a.shape[0]] = a
                n += a.shape[0]
            return n
        return fill

    source, sizes, visited, counts = [], [], [], []
    sets[0].stage(rows_of(chunks[0]))
    for ci, c in enumerate(chunks):
        s = sets[ci % 2]
        s.wait_copied(w.stream)
        offs = np.concatenate([[0], np.cumsum([lengths[t] for t in c])]).astype(np.int64)
        ch = SimpleNamespace(index=ci, set=s, n=s.n, d_offs=torch.from_numpy(offs).to(device),
                             d_counts=torch.empty(len(c), 3, dtype=torch.int64, device=device),
                             d_first=torch.empty(len(c), dtype=torch.int64, device=device))
        if s.n:
            _critic_values(critic, s.dev[:s.n], w.cpred[:s.n], handle=w.h, x=w.x)
        plan.enqueue(w, ch)
        if ci + 1 < len(chunks):
            sets[(ci + 1) % 2].stage(rows_of(chunks[ci + 1]))  # host fill + H2D of the next chunk under this one's kernels
        end, picked, extra = plan.collect(w, ch)
        first, cnt = ch.d_first.cpu().numpy(), ch.d_counts.cpu().numpy()
        tr = np.searchsorted(offs, picked, side="right") - 1
        source.append(np.stack([np.asarray(walk)[np.asarray(c)[tr]] if len(picked) else np.zeros(0, np.int64),
                                picked - offs[tr]] + extra, 1))
        for j, t in enumerate(c):
            if first[j] >= 0:
                log(f"total images = {first[j]}")
                sizes.append(int(first[j]))
                visited.append(names[t])
                counts.append(cnt[j])
        if end >= total_images:
            break
    torch.cuda.synchronize(device)
    n = int(w.running.item())
    counts = np.array(counts, np.int64).reshape(-1, 3)
    log(plan.summary(n, len(visited), counts.sum(0)))
    return plan.dataset(n, np.concatenate(source).astype(np.int64), visited, sizes, counts)


def curate(episodes, critic, collect=P.collect, total_images=P.total_images, chunk_frames=8192, order=None,
           device="cuda:0", log=print):
    """load_minerl_data(critic) (vae_utility.py:393-461, non-recon branch) on the device.

    episodes: [(name, array (T, 64, 64, 3) uint8)] (load_episodes).  order: None = reference_order of the names, or an
    explicit list of names.  Chunks of whole trajectories (at most chunk_frames frames, unless one trajectory is longer)
    stream through two pinned staging buffers, the copy of chunk i+1 on a side stream under chunk i's kernels; per chunk:
    cvae_preprocess_u8 + cvae_critic_forward in pieces of CURATE_PIECE, cvae_curate_select (the running count stays on
    the device) and cvae_gather_frames_u8 into the dataset buffer.  The running count is read once per chunk, to stop
    streaming at the cut.  log gets the reference's progress lines (`total images = N` before each visited trajectory)
    and the per-bin totals.  Returns a DeviceDataset."""
    return _walk(_PlainPlan(), episodes, critic, collect, total_images, chunk_frames, order, device, log)


class ReconDataset(_CuratedDataset):
    """The second VAE's training set on the device: frames (N, 3, w, w) fp32 = the first VAE's eval-mode reconstructions
    (Tanh range), preds (N, 1) fp32 = the critic's value OF THE RECONSTRUCTION (train() evaluates the critic on what it
    trains on, vae.py:50; the critic is frozen, so the value is computed once), source (N, 3) int64 host array (trajectory,
    frame, kind: 0 = decoded at the frame's critic value, 1 = decoded at 0).  names / sizes / counts as DeviceDataset has
    them (sizes count entries, counts frames per bin); stats = what curate_recon ran (walked / encoded / decoded)."""
    SOURCE_COLS = 3

    def __init__(self, frames, preds, source, names=(), sizes=(), counts=None, stats=None):
        if not (frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 4 and frames.shape[1] == 3
                and frames.shape[2] == frames.shape[3] and frames.is_contiguous()):
            raise ValueError("frames must be a contiguous fp32 device tensor (N, 3, w, w)")
        super().__init__(frames, preds, source, names, sizes, counts)
        self.stats = dict(stats or {})

    @property
    def width(self):
        return self.frames.shape[2]

    def gather(self, handle, nb, idx, x, pred, aug=None, applied=None):
        """One training batch: x = frames[idx] (a bit copy), pred = preds[idx] (cvae_gather_f32).  aug / applied as
        DeviceDataset.gather, through cvae_gather_f32_aug: flip and shift only (a brightness gain is refused)."""
        if aug is None:
            if applied is not None:
                raise ValueError("applied needs aug: the plain gather draws nothing")
            handle.gather_f32(nb, self.frames, self.preds, idx, x, pred)
        else:
            handle.gather_f32_aug(nb, self.frames, self.preds, idx, aug, x, pred, applied)

    def save(self, path):
        """Plain arrays (numpy .npz, uncompressed): frames, preds, source, names, sizes, counts."""
        with open(path, "wb") as f:
            np.savez(f, frames=self.frames.cpu().numpy(), preds=self.preds.cpu().numpy(), source=self.source,
                     names=np.array(self.names, dtype=str), sizes=np.array(self.sizes, np.int64), counts=self.counts)

    @classmethod
    def load(cls, path, device="cuda:0"):
        with np.load(path, allow_pickle=False) as z:
            frames = torch.from_numpy(np.ascontiguousarray(z["frames"], np.float32)).to(device)
            preds = torch.from_numpy(np.ascontiguousarray(z["preds"], np.float32).reshape(-1, 1)).to(device)
            return cls(frames, preds, z["source"], z["names"].tolist(), z["sizes"].tolist(), z["counts"])

    def to_reference_list(self):
        """The reference's recon dset: [(1, 3, w, w) float32 ndarray, ...] (pickle.dump of it is recon-dataset.pickle)."""
        a = self.frames.cpu().numpy()
        return [a[i:i + 1].copy() for i in range(a.shape[0])]


class _ReconPlan:
    """What curate_recon() adds to the walk: the first VAE's reconstructions of the kept frames, two entries for a mid frame."""
    who, per_frame, per_traj = "curate_recon", 2, 4               # a trajectory adds at most per_traj * collect entries

    def __init__(self, vae):
        self.vae, self.x_rows = vae, vae.max_batch
        self.stats = {"walked": 0, "encoded": 0, "decoded": 0}

    def validate(self, device):
        if self.vae.width != 64:
            raise ValueError("curate_recon needs a 64x64 VAE (the critic is 64x64 only)")
        self.vae.eval()
        if self.vae.theta.device != device:
            raise ValueError(f"the VAE is on {self.vae.theta.device}, the dataset goes to {device}")

    def allocate(self, cap, biggest, device):
        VB = self.vae.max_batch
        self.frames = torch.empty(max(cap, 1), 3, 64, 64, device=device)
        self.preds = torch.empty(max(cap, 1), 1, device=device)
        self.ws = self.vae._workspace(VB)
        self.sel = torch.empty(biggest, dtype=torch.int64, device=device)
        self.ent_frame = torch.empty(2 * biggest, dtype=torch.int64, device=device)
        self.ent_sel = torch.empty(2 * biggest, dtype=torch.int64, device=device)
        self.ent_kind = torch.empty(2 * biggest, dtype=torch.int32, device=device)
        self.mu = torch.empty(biggest, P.latent_dim, device=device)
        self.spred = torch.empty(biggest, 1, device=device)
        self.logvar = torch.empty(VB, P.latent_dim, device=device)
        self.zeros = torch.zeros(VB, P.latent_dim, device=device)
        self.zcat = torch.empty(VB, P.latent_dim + 1, device=device)
        self.span = torch.zeros(3, dtype=torch.int64, device=device)

    def enqueue(self, w, ch):
        d_sfirst = torch.empty(ch.d_first.shape[0], dtype=torch.int64, device=ch.d_first.device)
        w.h.curate_select_recon(ch.d_offs, w.cpred[:ch.n], w.collect, w.total_images, w.running, ch.d_counts, ch.d_first,
                                d_sfirst, self.span, self.ent_frame, self.ent_kind, self.ent_sel, self.sel)

    def collect(self, w, ch):
        vae, vh, VB, theta = self.vae, self.vae.handle, self.vae.max_batch, self.vae.theta.data
        sp = self.span.cpu().numpy()                           # the one host read of the chunk: sizes the launches below
        e0, ne, ns = int(sp[0]), int(sp[1]), int(sp[2])
        if e0 + ne > w.cap or ns > ch.n:
            raise RuntimeError(f"curate_recon: chunk {ch.index} claims entries [{e0}, {e0 + ne}) of {w.cap} and {ns} of {ch.n} frames")
        for p in range(0, ns, VB):                             # the encoder, once per selected frame
            nb = min(VB, ns - p)
            vh.preprocess_u8_gather(nb, ch.set.dev, w.cpred, self.sel[p:p + nb], w.x[:nb], self.spred[p:p + nb])
            vh.forward(nb, w.x[:nb], self.spred[p:p + nb], self.zeros[:nb], theta, vae.bn_state, self.mu[p:p + nb],
                       self.logvar[:nb], None, self.ws, train=False)
        ch.set.release(w.stream)
        for p in range(0, ne, VB):                             # the decoder, once per entry, into the dataset slots
            nb = min(VB, ne - p)
            vh.recon_zcat(nb, self.ent_sel[p:p + nb], self.ent_kind[p:p + nb], self.mu[:ns], self.spred[:ns], self.zcat[:nb])
            vh.decode(nb, self.zcat[:nb], theta, self.frames[e0 + p:e0 + p + nb], self.ws)
        for p in range(0, ne, CURATE_PIECE):                   # train() evaluates the critic on the reconstructions
            nb = min(CURATE_PIECE, ne - p)
            w.h.critic_forward(nb, self.frames[e0 + p:e0 + p + nb], w.critic.flat, self.preds[e0 + p:e0 + p + nb])
        vae._stamp_workspace()
        self.stats["walked"] += ch.n
        self.stats["encoded"] += ns
        self.stats["decoded"] += ne
        return e0 + ne, self.ent_frame[:ne].cpu().numpy(), [self.ent_kind[:ne].cpu().numpy().astype(np.int64)]

    def summary(self, n, n_traj, tot):
        return (f"recon dataset: {n} entries from {self.stats['encoded']} frames of {n_traj} trajectories "
                f"(mid {tot[0]}, high {tot[1]}, low {tot[2]})")

    def dataset(self, n, source, names, sizes, counts):
        return ReconDataset(self.frames[:n], self.preds[:n], source, names, sizes, counts, self.stats)


def curate_recon(episodes, critic, vae, collect=P.collect, total_images=P.total_images, chunk_frames=8192, order=None,
                 device="cuda:0", log=print):
    """load_minerl_data(critic, recon_dset=True, vae=vae) (vae_utility.py:393-443) on the device.

    The streaming structure of curate().  Per chunk: the critic values of all frames, cvae_curate_select_recon (running
    ENTRY count on the device), one host read of span; then for the selected frames only, in pieces of the VAE handle's
    max_batch: cvae_preprocess_u8_gather (x and the frames' critic values) and the eval-mode encoder
    (cvae_forward(recon=NULL, train=0): running BatchNorm statistics, mu) — once per selected frame, also when the frame owns
    two entries; for the entries, in pieces: cvae_recon_zcat and cvae_decode straight into the dataset slots (no staging
    copy), then cvae_critic_forward on the finished entries for preds.  Unselected frames cost the critic launch only.
    The VAE is put in eval mode and must be 64 x 64.  Returns a ReconDataset."""
    return _walk(_ReconPlan(vae), episodes, critic, collect, total_images, chunk_frames, order, device, log)


# ---- the critic's own training set: frames + discounted reward targets (critic_train.CriticTrainer) ----
CRITIC_CHUNK = 4096          # frames per staged host -> device copy of critic_dataset


def discounted_targets(rewards, gamma=0.98, shift=12, clip=1.0):
    """Value targets of one trajectory from its (T,) reward array — THIS PROJECT's definition: the reference ships only a
    trained checkpoint (its file name carries `shift=12`) and no critic training code, so nothing pins it.
        r'_t = r_{t+shift}  (0 past the end),   v_t = r'_t + gamma * v_{t+1}  (v_T = 0, computed backwards),   target = min(v, clip)
    in float64, returned as float32 (T,).  With rewards >= 0 and clip = 1 the targets lie in [0, 1], what the BCE loss needs."""
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    if shift < 0:
        raise ValueError(f"shift {shift} must be >= 0")
    T = r.shape[0]
    rs = np.zeros(T, np.float64)
    if shift < T:
        rs[:T - shift] = r[shift:]
    v = np.zeros(T, np.float64)
    nxt = 0.0
    for t in range(T - 1, -1, -1):
        nxt = rs[t] + gamma * nxt
        v[t] = nxt
    return np.minimum(v, clip).astype(np.float32)


def load_rewards(paths, episodes=None):
    """`.npy` files, or directories of them: one (T,) reward array per trajectory, named as the trajectory's frame file and
    kept in a directory of its own (load_episodes takes every `.npy` of a directory).  Returns [(name, float64 array)] sorted
    by name.  With `episodes` (load_episodes' result): ValueError for a trajectory without rewards or of another length;
    the result then holds exactly the episodes' names, in their order."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    files = []
    for p in paths:
        p = os.fspath(p)
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in os.listdir(p) if f.endswith(".npy")]
        elif os.path.isfile(p):
            files.append(p)
        else:
            raise FileNotFoundError(p)
    out = {}
    for f in files:
        name = os.path.basename(f)[:-4] if f.endswith(".npy") else os.path.basename(f)
        if name in out:
            raise ValueError(f"two reward files named {name!r}")
        a = np.load(f)
        if a.ndim != 1 or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{f}: rewards must be a numeric (T,) array, got {a.dtype} {a.shape}")
        out[name] = a.astype(np.float64)
    if episodes is None:
        return sorted(out.items())
    return _match_rewards(episodes, out)


def _match_rewards(episodes, rewards):
    rewards = dict(rewards)
    matched = []
    for name, frames in episodes:
        if name not in rewards:
            raise ValueError(f"trajectory {name!r} has no reward file")
        r = np.asarray(rewards[name])
        if r.ndim != 1 or r.shape[0] != frames.shape[0]:
            raise ValueError(f"trajectory {name!r}: {frames.shape[0]} frames but rewards of shape {r.shape}")
        matched.append((name, r))
    return matched


def critic_dataset_indices(lengths, size=None, seed=0):
    """The draw of critic_dataset: `size` (default: all) of the sum(lengths) frames without replacement, in drawn order
    (np.random.default_rng(seed).permutation) -> (trajectory, frame) int64 (size, 2)."""
    lengths = np.asarray(lengths, np.int64)
    total = int(lengths.sum())
    size = total if size is None else int(size)
    if not 0 <= size <= total:
        raise ValueError(f"size {size} outside [0, {total}] (the trajectories' frames)")
    pick = np.random.default_rng(seed).permutation(total)[:size]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    traj = np.searchsorted(offs, pick, side="right") - 1
    return np.stack([traj, pick - offs[traj]], 1).astype(np.int64)


def critic_dataset(episodes, rewards, size=None, seed=0, gamma=0.98, shift=12, clip=1.0, device="cuda:0"):
    """The critic's training set on the device: `size` frames drawn over all trajectories (critic_dataset_indices) with
    discounted_targets(rewards of their trajectory) in the `preds` slot of a DeviceDataset, so CriticTrainer.fit_device
    gathers (frame, target) batches with cvae_preprocess_u8_gather.  episodes: load_episodes' pairs; rewards: load_rewards'
    pairs or a dict.  Frames travel in chunks of CRITIC_CHUNK through two StagingSets (pinned, side stream)."""
    episodes = list(episodes)
    matched = _match_rewards(episodes, rewards)
    for name, a in episodes:
        if not (a.dtype == np.uint8 and a.ndim == 4 and a.shape[1:] == (64, 64, 3)):
            raise ValueError(f"trajectory {name!r}: the critic needs uint8 (T, 64, 64, 3) frames")
    device = torch.device(device)
    source = critic_dataset_indices([a.shape[0] for _, a in episodes], size, seed)
    n = source.shape[0]
    targets = [discounted_targets(r, gamma, shift, clip) for _, r in matched]
    offs = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
    tg = np.concatenate(targets + [np.zeros(0, np.float32)])[offs[source[:, 0]] + source[:, 1]].astype(np.float32).reshape(n, 1)
    frames = torch.empty(max(n, 1), 64, 64, 3, dtype=torch.uint8, device=device)[:n]
    preds = torch.from_numpy(tg).to(device)
    if n:
        stream = torch.cuda.current_stream(device)
        copy_stream = torch.cuda.Stream(device=device)
        sets = [StagingSet(min(CRITIC_CHUNK, n), 64, device, copy_stream) for _ in range(2)]

        def rows_of(lo):
            def fill(pin):
                part = source[lo:lo + CRITIC_CHUNK]
                for t in np.unique(part[:, 0]):
                    pos = np.nonzero(part[:, 0] == t)[0]
                    pin[pos] = episodes[t][1][part[pos, 1]]
                return part.shape[0]
            return fill

        starts = list(range(0, n, CRITIC_CHUNK))
        sets[0].stage(rows_of(0))
        for ci, lo in enumerate(starts):
            s = sets[ci % 2]
            s.wait_copied(stream)
            frames[lo:lo + s.n].copy_(s.dev[:s.n])
            s.release(stream)
            if ci + 1 < len(starts):
                sets[(ci + 1) % 2].stage(rows_of(starts[ci + 1]))
        torch.cuda.synchronize(device)
    return DeviceDataset(frames, preds, source, names=[name for name, _ in episodes])
