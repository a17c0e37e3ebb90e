"""Float64 reference of the dense CRF that cvae_dense_crf computes (include/cvae.h), restated from its equations:

    features    Gaussian (x/gamma, y/gamma); bilateral (x/alpha, y/alpha, r/beta, g/beta, b/beta) on raw uint8 RGB
    kernels     k(i,j) = exp(-|f_i - f_j|^2 / 2), the sum over j includes j = i
    normalise   n_i = (sum_j k(i,j))^-1/2, filtered(v)_i = n_i sum_j k(i,j) n_j v_j   (per kernel)
    unary       u(l) = -log(max(prob(l), p_floor)), prob = (1 - prob1, prob1)
    inference   Q = softmax(-u); `it` times Q = softmax(-u + w2 filtered_g(Q) + w1 filtered_b(Q)) (Potts, per label)
    label       1 iff Q(1) > Q(0)

Brute force over all pixel pairs in torch float64, on the CPU or (device="cuda", the 128 x 128 case of the GPU tests)
on the GPU; on the CPU, frames larger than 64 x 64 build the kernel rows in chunks instead of holding the (W*W)^2
matrices.  Any square size works (host tests use small frames).
"""
import numpy as np
import torch

CRF_REF = (22, 12, 3.1, 8, 1.8, 10)


def _kernel_rows(x, y, rgb, s, e, inv2, inv2c=None):
    """k(i, :) for rows i in [s, e): exp(-(dx^2 + dy^2) * inv2 [- |dc|^2 * inv2c])"""
    d = (x[s:e, None] - x[None]) ** 2 + (y[s:e, None] - y[None]) ** 2
    a = d * inv2
    if inv2c is not None:
        c = torch.zeros_like(a)
        for ch in range(3):
            c += (rgb[s:e, None, ch] - rgb[None, :, ch]) ** 2
        a = a + c * inv2c
    return torch.exp(-a)


def crf_ref(img, prob1, params=CRF_REF, p_floor=1e-5, rows=1024, device="cpu"):
    """img (W,W,3) uint8, prob1 (W,W) -> (labels (W,W) bool, Q(1) (W,W) float64)"""
    w1, alpha, beta, w2, gamma, it = params
    img = np.asarray(img)
    W = img.shape[0]
    assert img.shape == (W, W, 3)
    N = W * W
    idx = torch.arange(N, dtype=torch.int64, device=device)
    x, y = (idx % W).to(torch.float64), (idx // W).to(torch.float64)
    rgb = torch.from_numpy(img.reshape(N, 3).astype(np.float64)).to(device)
    spec = {"g": (0.5 / gamma ** 2, None), "b": (0.5 / alpha ** 2, 0.5 / beta ** 2)}
    cache = {}
    if N <= (4096 if device == "cpu" else 16384):
        for kname, (a, c) in spec.items():
            cache[kname] = _kernel_rows(x, y, rgb, 0, N, a, c)

    def apply(kname, v):                       # sum_j k(i,j) v_j, v (N, m)
        if kname in cache:
            return cache[kname] @ v
        out = torch.empty(N, v.shape[1], dtype=torch.float64, device=device)
        for s in range(0, N, rows):
            e = min(N, s + rows)
            out[s:e] = _kernel_rows(x, y, rgb, s, e, *spec[kname]) @ v
        return out

    ones = torch.ones(N, 1, dtype=torch.float64, device=device)
    n = {k: apply(k, ones) ** -0.5 for k in spec}
    p1 = torch.from_numpy(np.asarray(prob1, dtype=np.float64).reshape(N)).to(device)
    prob = torch.stack([1.0 - p1, p1], dim=1)
    u = -torch.log(torch.clamp(prob, min=p_floor))
    Q = torch.softmax(-u, dim=1)
    for _ in range(int(it)):
        logits = -u + w2 * n["g"] * apply("g", n["g"] * Q) + w1 * n["b"] * apply("b", n["b"] * Q)
        Q = torch.softmax(logits, dim=1)
    Q = Q.cpu()
    labels = (Q[:, 1] > Q[:, 0]).numpy().reshape(W, W)
    return labels, Q[:, 1].numpy().reshape(W, W)
