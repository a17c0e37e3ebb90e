"""The training trace: a loss curve and per-tensor statistics of a fit_device run, kept ON THE DEVICE until somebody asks.

A trainer built with trace=Trace(...) ends every step in Trace._after_update: one cvae_trace_push launch (the step's loss
scalars bit for bit, its lr and the guard's decision into a ring of 128-byte rows) every `every` steps, and one
cvae_tensor_stats launch (gradient / weight / update sums of squares, maxima and non-finite counts of every parameter tensor,
include/cvae.h) every `tensors_every` steps into a second ring.  Neither touches the host; read() copies each ring once.
Host Python only: the module imports (and decodes, merges and prints files) without a GPU.

    python -m critic_vae_amd.trace FILE.npz      the last tensor row as a table, and the number of steps held
"""
import os
import sys

import numpy as np

ROW_BYTES, STAT_BYTES, MAX_SCALARS, MAX_TENSORS = 128, 48, 16, 32
# cvae_trace_row and cvae_tensor_stat (include/cvae.h) as NumPy records
ROW_DTYPE = np.dtype([("step", "<i8"), ("lr", "<f4"), ("applied", "<i4"), ("nonfinite", "<u4"), ("grad_norm", "<f4"),
                      ("coef", "<f4"), ("n_scalars", "<i4"), ("reserved", "u1", (32,)), ("scalars", "<f4", (MAX_SCALARS,))])
STAT_DTYPE = np.dtype([("g2", "<f8"), ("p2", "<f8"), ("u2", "<f8"), ("gmax", "<f4"), ("pmax", "<f4"),
                       ("g_nonfinite", "<u4"), ("p_nonfinite", "<u4"), ("step", "<i8")])
assert ROW_DTYPE.itemsize == ROW_BYTES and STAT_DTYPE.itemsize == STAT_BYTES
STEP_KEYS = ("step", "lr", "applied", "nonfinite", "grad_norm", "coef", "scalars")
TENSOR_KEYS = ("tensor_step", "grad_norm_t", "weight_norm", "update_norm", "update_ratio", "grad_max", "weight_max",
               "grad_nonfinite", "weight_nonfinite")
# read() returns the per-tensor gradient norms under "grad_norm" of its "tensors" part; a flat .npz needs another name
VAE_SCALARS = {"total_loss": 0, "recon_loss": 1, "kld": 2}          # slots of the VAE's 16 loss scalars (cvae_loss)


def tensor_table(handle_or_layout):
    """[(name, begin, end), ...] of every parameter tensor in the flat buffers, ascending, alignment padding excluded: from a
    lib.Handle (its cvae_param_name / offset / numel: the VAE's 30 tensors) or from a layout {name: (offset, numel)} such as
    optim.critic_layout() (the critic's 14)."""
    layout = getattr(handle_or_layout, "layout", handle_or_layout)
    table = sorted((int(off), int(off) + int(n), name) for name, (off, n) in layout.items() if int(n) > 0)
    for (_, e, a), (b, _, c) in zip(table, table[1:]):
        if b < e:
            raise ValueError(f"the layout's tensors {a} and {c} overlap at element {b}")
    return [(name, b, e) for b, e, name in table]


class Trace:
    """capacity: rows of the step ring (the last `capacity` pushed steps survive).  every: push a step row when step_count % every
    == 0 (0: never).  tensors_every: per-tensor statistics when step_count % tensors_every == 0 (0: never); tensor_capacity:
    rows of their ring (default: as many as cover the span of the step ring, at least 1).  A Trace belongs to ONE trainer:
    the first step binds it (tensor table, rings on the trainer's device)."""

    def __init__(self, capacity=4096, every=1, tensors_every=0, tensor_capacity=None):
        capacity, every, tensors_every = int(capacity), int(every), int(tensors_every)
        if capacity < 1:
            raise ValueError(f"capacity {capacity}: at least one row")
        if every < 0 or tensors_every < 0:
            raise ValueError(f"every {every} / tensors_every {tensors_every}: a positive step interval, or 0 for never")
        if tensor_capacity is None:
            tensor_capacity = max(1, -(-capacity * max(every, 1) // tensors_every)) if tensors_every else 0
        tensor_capacity = int(tensor_capacity)
        if tensors_every and tensor_capacity < 1:
            raise ValueError(f"tensors_every {tensors_every} with tensor_capacity {tensor_capacity}: the tensor ring has no room")
        self.capacity, self.every, self.tensors_every, self.tensor_capacity = capacity, every, tensors_every, tensor_capacity
        self.table = None                  # [(name, begin, end)] once bound
        self.n_scalars = None
        self._owner = None
        self._ring, self._pushed = None, 0            # uint8 (capacity * 128) on the device, zero = an empty row; launches so far
        self._tring, self._tpushed = None, 0          # uint8 (tensor_capacity * tensors * 48)
        self._scratch = None

    # ---- the hook ----
    def _bind(self, trainer):
        layout = trainer._trace_layout()
        self.table = tensor_table(layout)
        if len(self.table) > MAX_TENSORS:
            raise ValueError(f"{len(self.table)} parameter tensors: cvae_tensor_stats takes at most {MAX_TENSORS}")
        self.n_scalars = int(trainer.scalars.numel())
        self._owner = trainer

    def _after_update(self, trainer, theta, grad_scale, lr):
        """The end of trainer.step(): launches only, nothing is read."""
        import torch
        from .lib import tensor_stats_scratch_bytes
        if self._owner is None:
            self._bind(trainer)
        elif self._owner is not trainer:
            raise RuntimeError("this Trace already follows another trainer: one Trace per trainer")
        step, dev = int(trainer.step_count), theta.device
        guard = trainer.guard if trainer.guarded else None
        if self.every and step % self.every == 0:
            if self._ring is None:
                self._ring = torch.zeros(self.capacity * ROW_BYTES, dtype=torch.uint8, device=dev)
            row = (step // self.every - 1) % self.capacity
            # the entry writes row (step - 1) % capacity of the ring it is given: a ring of one row, placed where this push belongs
            trainer.h.trace_push(self._ring[row * ROW_BYTES:(row + 1) * ROW_BYTES], 1, step, lr, trainer.scalars, self.n_scalars, guard=guard)
            self._pushed += 1
        if self.tensors_every and step % self.tensors_every == 0:
            nt = len(self.table)
            ranges = [(b, e) for _, b, e in self.table]
            if self._tring is None:
                self._tring = torch.zeros(self.tensor_capacity * nt * STAT_BYTES, dtype=torch.uint8, device=dev)
                self._scratch = torch.empty(tensor_stats_scratch_bytes(ranges), dtype=torch.uint8, device=dev)
            row = (step // self.tensors_every - 1) % self.tensor_capacity
            trainer.h.tensor_stats(theta, trainer.grads, trainer.m, trainer.v, ranges, step,
                                   self._tring[row * nt * STAT_BYTES:(row + 1) * nt * STAT_BYTES], self._scratch, lr=lr,
                                   b1=trainer.betas[0], b2=trainer.betas[1], eps=trainer.eps, grad_scale=grad_scale, guard=guard)
            self._tpushed += 1

    # ---- the one place that copies ----
    def read(self):
        """One device -> host copy of each ring (the only synchronisation a trace ever causes) -> dict of NumPy arrays ordered
        by step: step, lr, applied, nonfinite, grad_norm (the guard's global norm), coef, scalars (rows, n_scalars), dropped;
        "tensors": dict(tensor_step, names, grad_norm, weight_norm, update_norm, update_ratio, grad_max, weight_max,
        grad_nonfinite, weight_nonfinite — each (rows, tensors) — and dropped)."""
        names = [name for name, _, _ in (self.table or [])]
        ring = np.zeros(0, np.uint8) if self._ring is None else self._ring.cpu().numpy()
        tring = np.zeros(0, np.uint8) if self._tring is None else self._tring.cpu().numpy()
        return decode(ring, self._pushed, tring, self._tpushed, names, self.n_scalars)

    def save(self, path):
        """read() -> `path` (.npz).  An existing file of the same layout (tensor names, scalar count) is continued: its rows
        BEFORE the first new step are kept, its rows at or after it are dropped, so a resumed run extends the curve it left."""
        new = flatten(self.read())
        if os.path.exists(path):
            with np.load(path, allow_pickle=False) as f:
                old = {k: f[k] for k in f.files}
            new = merge(old, new)
        with open(path, "wb") as f:
            np.savez(f, **new)
        return path

    def to_tensorboard(self, directory, batch_size, num_samples=None, data=None):
        """The reference's three scalar tags (recon_loss, kld, total_loss: log_info, vae_utility.py:372-380) from the VAE's
        step rows, at the reference's x axis: images seen before the batch, batch_i + num_samples * ep."""
        try:
            from torch.utils.tensorboard import SummaryWriter
        except ImportError as e:
            raise RuntimeError(f"to_tensorboard needs torch.utils.tensorboard ({e})")
        data = self.read() if data is None else data
        writer = SummaryWriter(directory)
        for step, row in zip(data["step"], data["scalars"]):
            x = reference_x(int(step), batch_size, num_samples)
            for tag, slot in VAE_SCALARS.items():
                writer.add_scalar(tag, float(row[slot]), x)
        writer.close()
        return directory


def reference_x(step, batch_size, num_samples=None):
    """The x of the reference's Logger for 1-based optimizer step `step`: batch_i + num_samples * ep (vae.py:60-64)."""
    if num_samples is None:
        return (step - 1) * batch_size
    per_epoch = -(-num_samples // batch_size)
    ep, i = divmod(step - 1, per_epoch)
    return i * batch_size + num_samples * ep


def decode(ring, pushed, tring, tpushed, names, n_scalars=None):
    """The two rings as bytes (uint8 arrays; a row whose step is 0 was never written) -> what Trace.read() returns."""
    rows = np.frombuffer(np.ascontiguousarray(ring).tobytes(), dtype=ROW_DTYPE)
    rows = rows[rows["step"] > 0]
    rows = rows[np.argsort(rows["step"], kind="stable")]
    if n_scalars is None:
        n_scalars = int(rows["n_scalars"][0]) if len(rows) else 0
    out = {k: rows[k].copy() for k in STEP_KEYS if k != "scalars"}
    out["scalars"] = rows["scalars"][:, :n_scalars].copy()
    out["dropped"] = int(pushed) - len(rows)
    nt = len(names)
    stats = np.frombuffer(np.ascontiguousarray(tring).tobytes(), dtype=STAT_DTYPE).reshape(-1, nt) if nt else np.zeros((0, 0), STAT_DTYPE)
    stats = stats[stats["step"][:, 0] > 0] if nt else stats
    stats = stats[np.argsort(stats["step"][:, 0], kind="stable")] if nt else stats
    gn, wn, un = np.sqrt(stats["g2"]), np.sqrt(stats["p2"]), np.sqrt(stats["u2"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = un / wn
    out["tensors"] = {"tensor_step": stats["step"][:, 0].copy() if nt else np.zeros(0, np.int64), "names": list(names),
                      "grad_norm": gn, "weight_norm": wn, "update_norm": un, "update_ratio": ratio,
                      "grad_max": stats["gmax"].copy(), "weight_max": stats["pmax"].copy(),
                      "grad_nonfinite": stats["g_nonfinite"].copy(), "weight_nonfinite": stats["p_nonfinite"].copy(),
                      "dropped": int(tpushed) - len(stats)}
    return out


def flatten(data):
    """read()'s dict as the flat arrays of the .npz: the per-tensor gradient norms become "grad_norm_t"."""
    t = data["tensors"]
    flat = {k: np.asarray(data[k]) for k in STEP_KEYS}
    flat["dropped"] = np.asarray(data["dropped"], np.int64)
    flat["names"] = np.asarray(t["names"], dtype=np.str_)
    for k in TENSOR_KEYS:
        flat[k] = np.asarray(t["grad_norm" if k == "grad_norm_t" else k])
    flat["tensor_dropped"] = np.asarray(t["dropped"], np.int64)
    return flat


def same_layout(old, new):
    return (set(old) == set(new) and list(old["names"]) == list(new["names"]) and old["scalars"].ndim == 2
            and old["scalars"].shape[1] == new["scalars"].shape[1])


def merge(old, new):
    """Flat arrays of an existing file + new ones: old rows with step below the first new step, then the new rows; the same for
    the tensor rows.  Another layout: the new arrays alone (the file is replaced)."""
    if not same_layout(old, new):
        return new
    out = dict(new)
    keep = old["step"] < new["step"][0] if len(new["step"]) else np.ones(len(old["step"]), bool)
    for k in STEP_KEYS:
        out[k] = np.concatenate([old[k][keep], new[k]])
    keep = old["tensor_step"] < new["tensor_step"][0] if len(new["tensor_step"]) else np.ones(len(old["tensor_step"]), bool)
    for k in TENSOR_KEYS:
        out[k] = np.concatenate([old[k][keep], new[k]]) if old[k].size or new[k].size else new[k]
    out["dropped"] = old["dropped"] + new["dropped"]
    out["tensor_dropped"] = old["tensor_dropped"] + new["tensor_dropped"]
    return out


def nonfinite_tensors(data):
    """Names of the tensors whose gradient held an Inf or a NaN in the LAST tensor row of a skipped step, with that step:
    (step, [names]) or None when no tensor row belongs to a skipped step.  data: what read() returns."""
    t = data["tensors"]
    skipped = set(data["step"][data["applied"] == 0].tolist())
    for k in range(len(t["tensor_step"]) - 1, -1, -1):
        if int(t["tensor_step"][k]) in skipped:
            return int(t["tensor_step"][k]), [n for n, c in zip(t["names"], t["grad_nonfinite"][k]) if c > 0]
    return None


def table_lines(flat):
    """The last tensor row of a file's arrays as text lines, then the count of steps held."""
    lines = []
    if len(flat["tensor_step"]):
        lines.append(f"tensor statistics at step {int(flat['tensor_step'][-1])}:")
        lines.append(f"{'tensor':<16}{'grad norm':>14}{'weight norm':>14}{'update ratio':>14}{'non-finite':>12}")
        for j, name in enumerate(flat["names"]):
            lines.append(f"{str(name):<16}{flat['grad_norm_t'][-1, j]:>14.6e}{flat['weight_norm'][-1, j]:>14.6e}"
                         f"{flat['update_ratio'][-1, j]:>14.6e}{int(flat['grad_nonfinite'][-1, j]) + int(flat['weight_nonfinite'][-1, j]):>12d}")
    else:
        lines.append("no tensor statistics in this file")
    steps = flat["step"]
    span = f" ({int(steps[0])}..{int(steps[-1])})" if len(steps) else ""
    lines.append(f"{len(steps)} steps held{span}, {len(flat['tensor_step'])} tensor rows")
    return lines


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        raise SystemExit("usage: python -m critic_vae_amd.trace FILE.npz")
    with np.load(argv[0], allow_pickle=False) as f:
        flat = {k: f[k] for k in f.files}
    print("\n".join(table_lines(flat)))


if __name__ == "__main__":
    main()
