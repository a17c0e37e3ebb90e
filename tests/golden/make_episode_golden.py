"""Generate tests/golden/episodes_real.npz from the REFERENCE's own dataset builder (run only where the reference
checkout exists, like make_segment_golden.py).

    python tests/golden/make_episode_golden.py            # needs /root/reference (read-only)

Runs the reference's load_minerl_data(critic) (vae_utility.py:393-461, non-recon branch) on CPU with the stand-ins of
make_segment_golden.py (`minerl`, `denseCRF`, PIL.ImageFont.truetype) plus one more: `minerl.data.make(...)` returns a
stub whose get_trajectory_names() lists TRAJ names in sorted order and whose load_data(name, ...) yields
({"pov": frame}, None, None, None, None) tuples, frame = POOL[i] for i in the trajectory's index sequence.

POOL is the 68 real frames of step_real_b68.npz["u8"] (asserted distinct).  With the reference critic
(critic_real_b8.npz weights) they fall 13 mid / 32 high / 2 low, the rest in no bin.  The trajectories are index
sequences over the pool, drawn with per-bin weights so that every bin reaches its cap of 150 in some trajectory, and
vae_utility.total_images is patched so that the global cut falls inside the list.

The fixture holds index arrays and results only (no frames, no reference code):
  pool_preds   (68,) float32   the reference critic's value of every pool frame
  traj_names   (T,)  str       sorted names; traj_len (T,) and traj_idx (concatenated pool indices) in that order
  order        (T,)  int64     the reference's shuffled visiting order (positions in traj_names)
  total_images, collect        the cut and the per-bin cap the reference ran with
  sizes        (V,)  int64     len(dset) printed before each visited trajectory ("total images = ..." lines)
  dset_pool    (N,)  int64     the content of the returned dset, each frame mapped back to its pool index
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

TOTAL_IMAGES = 1000
EDGES = (np.float32(0.4), np.float32(0.6), np.float32(0.7), np.float32(0.25))
MARGIN = 1e-4
# (name, length, bin weights (mid, high, low, none)) — names are listed in sorted order by the stub
TRAJ = (("traj_a", 1200, (1, 1, 1, 1)), ("traj_b", 151, (1, 0, 0, 0)), ("traj_c", 400, (4, 1, 0, 1)),
        ("traj_d", 1, (0, 1, 0, 0)), ("traj_e", 700, (0, 0, 1, 0)), ("traj_f", 0, None),
        ("traj_g", 900, (1, 2, 1, 0)), ("traj_h", 320, (0, 1, 1, 1)))


def _stub_modules(pool, traj_seqs):
    minerl = types.ModuleType("minerl")

    class _Data:
        def get_trajectory_names(self):
            return sorted(traj_seqs)

        def load_data(self, name, skip_interval=0, include_metadata=False):
            for i in traj_seqs[name]:
                yield {"pov": pool[i]}, None, None, None, None

    minerl.data = types.SimpleNamespace(make=lambda *a, **k: _Data())
    sys.modules["minerl"] = minerl
    dcrf = types.ModuleType("denseCRF")
    dcrf.densecrf = lambda img, prob, param: None
    sys.modules["denseCRF"] = dcrf
    from PIL import ImageFont
    ImageFont.truetype = lambda *a, **k: None


def bins_of(preds):
    """0 mid, 1 high, 2 low, -1 none — vae_utility.py:450-459 in float32."""
    p = np.asarray(preds, np.float32)
    return np.where((p >= EDGES[0]) & (p <= EDGES[1]), 0,
                    np.where(p >= EDGES[2], 1, np.where(p <= EDGES[3], 2, -1)))


def main():
    fx = np.load(os.path.join(HERE, "step_real_b68.npz"))
    pool = fx["u8"]
    assert len({f.tobytes() for f in pool}) == len(pool), "pool frames must be distinct"

    import critic_net                                  # noqa: E402  (the reference)
    cw = np.load(os.path.join(HERE, "critic_real_b8.npz"))
    critic = critic_net.Critic()
    critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
    critic.eval()

    # the pool's critic values through the reference's own preprocess_observation + evaluate
    rng = np.random.default_rng(11)
    traj_seqs = {}
    _stub_modules(pool, traj_seqs)
    import vae_utility as vu                           # noqa: E402
    with torch.no_grad():
        preds = np.array([critic.evaluate(vu.preprocess_observation(f))[0].item() for f in pool], np.float32)
    dist = np.min(np.abs(preds[:, None].astype(np.float64) - np.array(EDGES, np.float64)[None, :]))
    assert dist > MARGIN, f"a pool frame lies {dist:.2e} from a bin edge"
    b = bins_of(preds)
    members = [np.flatnonzero(b == k) for k in (0, 1, 2, -1)]
    print(f"[episodes] pool bins mid {len(members[0])} high {len(members[1])} low {len(members[2])} none {len(members[3])}")
    for name, n, wts in TRAJ:
        if n == 0:
            traj_seqs[name] = np.zeros(0, np.int64)
            continue
        wts = np.array(wts, np.float64) * np.array([len(m) > 0 for m in members])
        which = rng.choice(4, size=n, p=wts / wts.sum())
        traj_seqs[name] = np.array([rng.choice(members[k]) for k in which], np.int64)

    vu.total_images = TOTAL_IMAGES
    out = io.StringIO()
    with contextlib.redirect_stdout(out), torch.no_grad():
        dset = vu.load_minerl_data(critic)
    sizes = [int(line.split("=")[1]) for line in out.getvalue().splitlines() if line.startswith("total images =")]

    # map every dset frame back to its pool index through the reference's own preprocessing
    key = {vu.preprocess_observation(f).numpy().tobytes(): i for i, f in enumerate(pool)}
    dset_pool = np.array([key[np.asarray(d).tobytes()] for d in dset], np.int64)

    names = sorted(traj_seqs)
    shuffled = list(names)
    np.random.default_rng(seed=0).shuffle(shuffled)
    order = np.array([names.index(n) for n in shuffled], np.int64)
    assert len(sizes) < len(names), "the cut must fall inside the trajectory list"
    caps = {k: False for k in range(3)}
    for n in shuffled[:len(sizes)]:                    # the visited trajectories
        s = traj_seqs[n]
        for k in range(3):
            caps[k] |= int(np.sum(b[s] == k)) > 150
    assert all(caps.values()), f"every bin must reach its cap in some trajectory: {caps}"
    np.savez_compressed(os.path.join(HERE, "episodes_real.npz"),
                        pool_source="step_real_b68.npz/u8", pool_preds=preds,
                        traj_names=np.array(names), traj_len=np.array([len(traj_seqs[n]) for n in names], np.int64),
                        traj_idx=np.concatenate([traj_seqs[n] for n in names]).astype(np.int64),
                        order=order, total_images=TOTAL_IMAGES, collect=150,
                        sizes=np.array(sizes, np.int64), dset_pool=dset_pool)
    print(f"[episodes] order {[names[i] for i in order]} sizes {sizes} -> {len(dset_pool)} frames")


if __name__ == "__main__":
    main()
