"""What the augmentation tests share: the torch statement of the pixel rule on an already gathered batch (the yardstick
of the GPU tests: the plain kernel's output, torch indexing and torch fp32 arithmetic — no code of the kernels under test,
no use of Augment.draws), and the enumeration of the (flip, dx, dy) combinations a set of rows holds.  Works on any device."""
import torch


def index_maps(applied, W):
    """(rows, cols), each (B, W) int64: output row i reads source row rows[b, i], output column j source column cols[b, j]."""
    a = applied.to(torch.int64)
    ar = torch.arange(W, device=a.device, dtype=torch.int64)[None, :]
    flip, dx, dy = a[:, 0:1], a[:, 1:2], a[:, 2:3]
    rows = (ar - dy).clamp(0, W - 1)
    cols = (torch.where(flip != 0, W - 1 - ar, ar) - dx).clamp(0, W - 1)
    return rows, cols


def permute(plain, applied):
    """plain (B, 3, W, W), any dtype -> the flipped / shifted copy (pure indexing: bits move, nothing is computed)."""
    B, C, W = plain.shape[0], plain.shape[1], plain.shape[3]
    rows, cols = index_maps(applied, W)
    b = torch.arange(B, device=plain.device)[:, None, None, None]
    c = torch.arange(C, device=plain.device)[None, :, None, None]
    return plain[b, c, rows[:, None, :, None], cols[:, None, None, :]]


def gains(applied):
    """float32(num) * 2^-31 per row, num = applied[:, 3] + 2^31: torch's int64 -> fp32 conversion rounds to nearest."""
    num = applied[:, 3].to(torch.int64) + (1 << 31)
    return num.to(torch.float32) * torch.tensor(2.0 ** -31, dtype=torch.float32, device=applied.device)


def transform(plain, applied):
    """The uint8 value rule on the plain gather's fp32 output: min(permuted * g, 1) in torch fp32."""
    g = gains(applied)[:, None, None, None]
    return torch.minimum(permute(plain, applied) * g, torch.ones((), dtype=torch.float32, device=plain.device))


def combinations(rows):
    """The set of (flip, dx, dy) in (n, >= 3) integer rows."""
    return {tuple(int(v) for v in r[:3]) for r in rows}


def all_combinations(shift):
    return {(f, dx, dy) for f in (0, 1) for dx in range(-shift, shift + 1) for dy in range(-shift, shift + 1)}
