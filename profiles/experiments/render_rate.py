"""cvae_compose_frames against the same composition written with torch indexing ops on the device, same inputs, same
process, alternating: 2 450 video pictures (an episode's X[100:5000:2]) at 64 x 64, and `segment -video` end to end with
and without --out.

    python profiles/experiments/render_rate.py [OUT.txt]
"""
import os, sys, time, statistics, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from critic_vae_amd import render, segment, synth, train
from critic_vae_amd.lib import PANEL_F32_CHW, PANEL_MASK, PANEL_U8_GREY, PANEL_U8_HWC
from critic_vae_amd.nets import VariationalAutoencoder
dev = torch.device("cuda:0")
B, w = 2450, 64
g = torch.Generator(device=dev); g.manual_seed(0)
frames = torch.randint(0, 256, (B, w, w, 3), dtype=torch.uint8, device=dev, generator=g)
ro = torch.rand(B, 3, w, w, device=dev, generator=g) * 2 - 1
rz = torch.rand(B, 3, w, w, device=dev, generator=g) * 2 - 1
du8 = torch.randint(0, 256, (B, w, w), dtype=torch.uint8, device=dev, generator=g)
thr, crf, gt = ((torch.rand(B, w, w, device=dev, generator=g) < 0.3).to(torch.uint8) for _ in range(3))
preds = torch.rand(B, device=dev, generator=g)
overlay = torch.from_numpy(render.title_overlay(w, 0.123, 0.456)).to(dev)
atlas, idx = render._labels(preds, dev)
h = segment._handle(w)
panels = [(PANEL_U8_HWC, frames, 3 * w * w), (PANEL_F32_CHW, ro, 3 * w * w), (PANEL_F32_CHW, rz, 3 * w * w), (PANEL_U8_GREY, du8, w * w),
          (PANEL_MASK, thr, w * w), (PANEL_MASK, crf, w * w), (PANEL_MASK, gt, w * w)]
out = torch.empty(B, 2 * w, 7 * w, 3, dtype=torch.uint8, device=dev)
out_t = torch.empty_like(out)
bytes_moved = out.numel() + frames.numel() + 4 * (ro.numel() + rz.numel()) + du8.numel() * 4      # HBM side: the overlay and the atlas stay in cache


def hip():
    h.compose_frames(B, panels, w, out, overlay, atlas, idx, (2, w + 2))


def torch_ops():
    """the same picture with torch indexing on the device"""
    out_t[:, :w] = 0
    out_t[:, w:, :w] = frames
    for p, r in ((1, ro), (2, rz)):
        out_t[:, w:, p * w:(p + 1) * w] = (r * 255).to(torch.int32).to(torch.uint8).permute(0, 2, 3, 1)
    out_t[:, w:, 3 * w:4 * w] = du8[..., None]
    for p, m in ((4, thr), (5, crf), (6, gt)):
        out_t[:, w:, p * w:(p + 1) * w] = (m * 255)[..., None]
    out_t[:, overlay != 0] = 255
    lab = atlas[idx.long()] != 0
    box = out_t[:, w + 2:w + 2 + lab.shape[1], 2:2 + lab.shape[2]]
    box[lab] = 255


def timed_launches(f, n=20, reps=7):
    """median over reps of (events around n launches) / n, in ms"""
    f(); f(); torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record(); e1.synchronize()
        t.append(e0.elapsed_time(e1) / n)
    return statistics.median(t), t


lines = []
th, ah = timed_launches(hip)
tt, at = timed_launches(torch_ops, n=20, reps=3)
th2, ah2 = timed_launches(hip)
same = torch.equal(out, out_t)
for name, t, a in (("cvae_compose_frames", th, ah), ("torch indexing ops", tt, at), ("cvae_compose_frames again", th2, ah2)):
    lines.append(f"{name}: {B} video pictures 64x64, per launch {' '.join(f'{x:.3f}' for x in a)} ms; median {t:.3f} ms = {B / t * 1e3:.3e} pictures/s, "
                 f"{bytes_moved / t / 1e9:.2f} TB/s of {bytes_moved / 1e6:.0f} MB (written {out.numel() / 1e6:.0f} MB)")
lines.append(f"torch composition bytewise equal: {same}")

# segment -video end to end (load, VAE + critic, normalise, CRF, IoU [, compose, copy to the host, write]) on a synthetic episode
with tempfile.TemporaryDirectory() as tmp:
    rng = np.random.default_rng(0)
    X = np.kron(rng.integers(0, 256, size=(5000, 8, 8, 3), dtype=np.uint8), np.ones((1, 8, 8, 1), np.uint8))
    Y = np.zeros((5000, 64, 64, 3), np.uint8); Y[:, 16:48, 24:40] = 255
    np.save(os.path.join(tmp, "X.npy"), X); np.save(os.path.join(tmp, "Y.npy"), Y)
    train.save_networks(VariationalAutoencoder(max_batch=8, seed=0).to(dev), os.path.join(tmp, "nets"))
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_critic_params(0).items()}, os.path.join(tmp, "critic.pt"))
    argv = ["-video", "--frames", os.path.join(tmp, "X.npy"), "--gt", os.path.join(tmp, "Y.npy"), "--networks", os.path.join(tmp, "nets"),
            "--critic", os.path.join(tmp, "critic.pt")]
    import contextlib, io
    def run(extra):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            segment.main(argv + extra)
        torch.cuda.synchronize(); return time.perf_counter() - t0
    run([])                                                    # warm-up
    cases = {"without --out": [], "--out (PNG files)" if render._pil_image() else "--out (one .npy, no PIL)": [os.path.join(tmp, "o")]}
    T = {k: [] for k in cases}
    for _ in range(3):
        for k, extra in cases.items():
            T[k].append(run(["--out", extra[0]] if extra else []))
    ep_frames, ep_gt = segment.load_episode(X, Y)
    r = segment.eval_frames(ep_frames, VariationalAutoencoder(max_batch=256, seed=0).to(dev), ep_gt, preds=np.full(2450, 0.5, np.float32),
                            keep_device=True)
    def pictures_only():
        return render.video_frames(r).cpu()
    pictures_only(); torch.cuda.synchronize()
    t0 = time.perf_counter(); pictures_only(); tp = time.perf_counter() - t0
    for k, v in T.items():
        lines.append(f"segment -video {k}: runs {' '.join(f'{x:.2f}' for x in v)} s; median {statistics.median(v):.2f} s")
    lines.append(f"video_frames + copy of {out.numel() / 1e6:.0f} MB to the host alone: {tp * 1e3:.1f} ms")
with open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w") as f:
    for line in lines:
        print(line, flush=True); f.write(line + "\n")
