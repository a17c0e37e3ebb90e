"""Generate tests/golden/critic_saliency_real.npz: the embeddings, the logit's input gradient, integrated gradients and
occlusion drops of the REFERENCE's Critic class with its real checkpoint on three of the 68 real frames (run only where
the reference checkout exists, on the CPU).

    python tests/golden/make_critic_saliency_golden.py            # needs /root/reference (read-only)

The reference's Critic (critic_net.py:5-69) runs in eval mode in fp64: forward(X, collect=True) for the embeddings,
autograd through the class down to its last Linear for the gradient of the logit, forward on host-occluded frames for the
drops.  tests/critic_saliency_ref.py (the restatement the GPU tests compare against) is asserted equal to it in fp64 within
1e-12 on every stored result: the reference is the authority, the restatement is what travels.

Inputs by reference, not stored again: the frames are step_real_b68.npz["u8"][FRAMES], the weights critic_real_b8.npz["w/*"]
(asserted equal to the checkpoint that file names).  Stored:
  frames (3,) int64                    indices into the 68 real frames
  pred (3,1) fp64, logit (3,) fp64
  e1..e5                               fp64 results rounded to fp32: (3,8,32,32) (3,8,16,16) (3,8,8,8) (3,16,4,4) (3,32,1,1)
  grad (3,3,64,64) fp64                d logit / d x
  decisions (3,11072) uint8            the fp64 run's own (free) pool / ReLU choices, cvae_critic_grad's layout
  ig_steps, ig (3,3,64,64) fp64        integrated gradients from black, N = 4, the kernel's scaling and order
  occ_patch, occ_fill (3,) fp32, occ_drop (3,4,4) fp64     occlusion with 16 x 16 patches of the stored colour
  gap32/grad, gap32/flips              the fp32 restatement's own distance to fp64: worst |g32 - g64| / max |g64| over the
                                       frames, and how many of its decisions differ
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import critic_saliency_ref as sref      # noqa: E402
import critic_train_ref as ref          # noqa: E402

FRAMES, IG_STEPS, PATCH = (3, 29, 61), 4, 16
TOL = 1e-12


def reference_net(weights):
    from critic_net import Critic
    net = Critic(dropout=0.3).double()
    net.load_state_dict({k: torch.from_numpy(weights[k]).double() for k, _ in ref.KEYS})
    net.eval()
    return net


def reference_logit(net, x):
    """The class's own layers down to crit.4: (embeds, logit (B,))."""
    a = x
    embeds = []
    for layer in net.features:
        a = layer(a)
        if isinstance(layer, type(net.pool)):
            embeds.append(a)
    embeds.append(a)
    for layer in list(net.crit)[:-1]:
        a = layer(a)
    return embeds, a.reshape(-1)


def reference_grad(net, x):
    xt = torch.from_numpy(np.asarray(x)).double().requires_grad_()
    _, z = reference_logit(net, xt)
    z.sum().backward()
    return xt.grad.numpy(), z.detach().numpy()


def gap(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    real = np.load(os.path.join(HERE, "step_real_b68.npz"))
    ck = np.load(os.path.join(HERE, "critic_real_b8.npz"))
    weights = {k: ck["w/" + k] for k, _ in ref.KEYS}
    sd = torch.load(os.path.join(REF, "saved-networks", str(ck["checkpoint"])), map_location="cpu")
    assert all(np.array_equal(sd[k].numpy(), weights[k]) for k, _ in ref.KEYS), "critic_real_b8.npz does not hold that checkpoint"
    x = ref.frames_to_x(real["u8"][list(FRAMES)])
    x64 = torch.from_numpy(x).double()
    net = reference_net(weights)

    # embeddings and pred: forward(X, collect=True) itself
    with torch.no_grad():
        pred, embeds = net(x64, collect=True)
    my_pred, my_embeds = sref.embeddings(weights, x)
    worst = max([gap(pred, my_pred)] + [gap(a, b) for a, b in zip(embeds, my_embeds)])
    print(f"embeddings: reference vs restatement (fp64) max diff {worst:.3e}")
    assert worst <= TOL and [tuple(e.shape[1:]) for e in embeds] == list(sref.EMBED_SHAPES)

    # gradient of the logit
    g, z = reference_grad(net, x)
    mine = sref.logit_grad(weights, x)
    worst = max(gap(g, mine["grad"]), gap(z, mine["logit"]), gap(pred, mine["pred"]))
    print(f"logit gradient: max diff {worst:.3e}; per-frame max |g| {np.abs(g).reshape(3, -1).max(1)}")
    assert worst <= TOL
    m32 = sref.logit_grad(weights, x, torch.float32)
    gmax = np.abs(g).reshape(3, -1).max(1)
    gap32 = float((np.abs(m32["grad"].astype(np.float64) - g).reshape(3, -1).max(1) / gmax).max())
    flips32 = int((m32["decisions"] != mine["decisions"]).sum())
    print(f"fp32 restatement: gradient within {gap32:.2e} of each frame's max, {flips32} decisions differ")

    # integrated gradients: the reference class on the scaled frames, the kernel's order
    acc = np.zeros_like(g)
    for k in range(1, IG_STEPS + 1):
        acc = acc + reference_grad(net, sref.scaled_frames(x, k, IG_STEPS))[0]
    ig = (acc * x.astype(np.float64)) * np.float64(np.float32(1.0) / np.float32(IG_STEPS))
    my_ig = sref.integrated_gradients(weights, x, IG_STEPS)
    worst = gap(ig, my_ig["grad"])
    print(f"integrated gradients (N = {IG_STEPS}): max diff {worst:.3e}")
    assert worst <= TOL and np.array_equal(my_ig["decisions"], mine["decisions"])

    # occlusion
    fill = (real["u8"].reshape(-1, 3).mean(0) / 255.0).astype(np.float32)
    gdim = 64 // PATCH
    drop = np.empty((3, gdim, gdim))
    with torch.no_grad():
        for b in range(3):
            occ = torch.from_numpy(sref.occluded_frames(x[b], PATCH, fill)).double()
            drop[b] = (pred[b, 0] - net(occ).reshape(-1)).numpy().reshape(gdim, gdim)
    my_occ = sref.occlusion(weights, x, PATCH, fill)
    worst = max(gap(drop, my_occ["drop"]), gap(pred.reshape(-1), my_occ["pred"]))
    print(f"occlusion (P = {PATCH}, fill {fill}): max diff {worst:.3e}; largest drop per frame {drop.reshape(3, -1).max(1)}")
    assert worst <= TOL

    out = dict(frames=np.asarray(FRAMES, np.int64), pred=pred.numpy(), logit=z, grad=g, decisions=mine["decisions"],
               ig_steps=np.int64(IG_STEPS), ig=ig, occ_patch=np.int64(PATCH), occ_fill=fill, occ_drop=drop)
    for i, e in enumerate(embeds):
        out[f"e{i + 1}"] = e.numpy().astype(np.float32)
    out["gap32/grad"], out["gap32/flips"] = np.float64(gap32), np.int64(flips32)
    path = os.path.join(HERE, "critic_saliency_real.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
