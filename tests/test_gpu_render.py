"""The reference's pictures on the MI355X (cvae_compose_frames, cvae_inject_zcat, critic_vae_amd.render), all through the
C-ABI: the compose kernel byte for byte against the numpy restatement of tests/golden/make_render_golden.py (which the
generator proves equal to the reference's PIL pictures), the three layouts against the reference's own pictures
(render_real.npz), the batched injection against the reference's, and the CLIs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_render_golden import compose_ref, panel_f32  # noqa: E402

from critic_vae_amd import render  # noqa: E402
from critic_vae_amd import segment as seg  # noqa: E402
from critic_vae_amd import synth, train  # noqa: E402
from critic_vae_amd.critic import Critic  # noqa: E402
from critic_vae_amd.lib import CvaeError, Handle, Panel, PANEL_F32_CHW, PANEL_MASK, PANEL_U8_GREY, PANEL_U8_HWC  # noqa: E402
from critic_vae_amd.nets import VariationalAutoencoder  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                      # the project's fp32 parity bound
W = 64


def _salt():
    """every k / 255 in [-1.3, 1.3] and its two float32 neighbours, +-0, +-1, NaN"""
    k = (np.arange(-332, 333, dtype=np.float32) / np.float32(255)).astype(np.float32)
    return np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)),
                           np.array([0.0, -0.0, 1.0, -1.0, np.nan], np.float32)])


def _panel_data(kind, B, w, rng):
    if kind == PANEL_F32_CHW:
        a = rng.uniform(-1.3, 1.3, size=(B, 3, w, w)).astype(np.float32)
        s = _salt()
        flat = a.reshape(B, -1)
        for b in range(B):                                         # the salt at another place in every picture
            o = (b * 977) % (flat.shape[1] - s.size)
            flat[b, o:o + s.size] = s
        return a
    if kind == PANEL_U8_HWC:
        return rng.integers(0, 256, size=(B, w, w, 3), dtype=np.uint8)
    if kind == PANEL_U8_GREY:
        return rng.integers(0, 256, size=(B, w, w), dtype=np.uint8)
    return (rng.random((B, w, w)) < 0.4).astype(np.uint8) * rng.integers(1, 256, size=(B, w, w), dtype=np.uint8)   # nonzero = set


@pytest.mark.parametrize("text", [False, True])
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("ih_is_w", [False, True])
@pytest.mark.parametrize("w", [64, 128])
def test_compose_kernel_is_byte_exact(w, ih_is_w, B, text):
    rng = np.random.default_rng(w + 2 * B + ih_is_w + 7 * text)
    ih = w if ih_is_w else 0
    kinds = [PANEL_F32_CHW, PANEL_U8_HWC, PANEL_U8_GREY, PANEL_MASK] + ([PANEL_MASK, PANEL_F32_CHW, PANEL_U8_GREY, PANEL_U8_HWC] if B < 257 else [])
    data = [_panel_data(k, B, w, rng) for k in kinds]
    h = Handle(w, 1)
    dev = [torch.from_numpy(a).cuda() for a in data]
    panels = [(k, t, t[0].numel()) for k, t in zip(kinds, dev)]
    H, Wout = ih + w, len(kinds) * w
    out = torch.full((B, H, Wout, 3), 77, dtype=torch.uint8, device="cuda")
    overlay = atlas = idx = None
    xy = (2, ih + 2) if B != 3 else (-3, H - 4)                    # B = 3: a label clipped at two edges of the picture
    if text:
        overlay = (rng.random((H, Wout)) < 0.05).astype(np.uint8) * rng.integers(1, 256, size=(H, Wout), dtype=np.uint8)
        atlas = render.label_atlas(render.label_strings())
        idx = rng.integers(-1, 12, size=B).astype(np.int32)        # -1 and 11: no label
    for clamp in (False, True):
        h.compose_frames(B, panels, ih, out, None if overlay is None else torch.from_numpy(overlay).cuda(),
                         None if atlas is None else torch.from_numpy(atlas).cuda(), None if idx is None else torch.from_numpy(idx).cuda(),
                         xy, clamp)
        got = out.cpu().numpy()
        for b in range(B):
            want = compose_ref([(k, a[b]) for k, a in zip(kinds, data)], ih, overlay, atlas, None if idx is None else int(idx[b]), xy, clamp)
            assert np.array_equal(got[b], want), (clamp, b, int((got[b] != want).sum()))
    assert (panel_f32(data[0][0]) != panel_f32(data[0][0], clamp=True)).any()            # the wrap is exercised


def test_compose_rejects_bad_arguments_before_any_launch():
    h = Handle(64, 1)
    f = torch.zeros(2, 3, 64, 64, device="cuda")
    out = torch.empty(2, 64, 64, 3, dtype=torch.uint8, device="cuda")

    def raw(B, n_panels, arr, row_offset=0, flags=0):
        h._check(h.lib.cvae_compose_frames(h.h, B, n_panels, arr, row_offset, flags, None, None, 0, 0, 0, None, 0, 0, out.data_ptr(), None))

    one = (Panel * 1)(Panel(PANEL_F32_CHW, 0, f.data_ptr(), 3 * 64 * 64))
    raw(2, 1, one)                                                                       # the valid call
    for bad in ((0, 1, one), (2, 0, one), (2, 9, one), (2, 1, None), (2, 1, one, -1), (2, 1, one, 129), (2, 1, one, 0, 2),
                (2, 1, (Panel * 1)(Panel(4, 0, f.data_ptr(), 0))), (2, 1, (Panel * 1)(Panel(0, 0, None, 0))),
                (2, 1, (Panel * 1)(Panel(0, 0, f.data_ptr() + 4, 0))), (2, 1, (Panel * 1)(Panel(0, 0, f.data_ptr(), 6))),
                (2, 1, (Panel * 1)(Panel(PANEL_U8_HWC, 0, f.data_ptr(), 8))), (2, 1, (Panel * 1)(Panel(0, 0, f.data_ptr(), -4)))):
        with pytest.raises(CvaeError):
            raw(*bad)
    with pytest.raises(CvaeError):                                                       # a workgroup count past 2^31: refused, not wrapped
        raw(2 ** 31 - 1, 1, (Panel * 1)(Panel(PANEL_F32_CHW, 0, f.data_ptr(), 0)))
    assert "workgroups" in h.lib.cvae_last_error().decode()
    torch.cuda.synchronize()


def _vae_and_critic(golden_dir, max_batch):
    vae = VariationalAutoencoder(max_batch=max_batch, seed=0).to("cuda")
    vae.load_reference_params(synth.make_params(0))
    cw = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    sd = {k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")}
    critic = Critic(64, handle=Handle(64, max_batch)).to("cuda")
    critic.load_state_dict(sd)
    return vae, critic, sd


def test_layouts_from_the_reference_floats_equal_its_pictures(golden_dir):
    fx = np.load(os.path.join(golden_dir, "render_real.npz"))
    sfx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    fr = fx["frames"]
    video = render.video_frames({"frames": u8[fr], "recon_one": fx["recon_one"], "recon_zero": fx["recon_zero"],
                                 "diff_u8": np.ascontiguousarray(fx["video"][:, W:, 3 * W:4 * W, 0]),      # the reference's diff_u8 of these frames
                                 "thr_masks": sfx["thr_masks/50"][fr], "crf_masks": sfx["thr_masks/50"][fr], "gt": sfx["gt"][fr],
                                 "preds": fx["preds"][fr]}, text=False)
    assert np.array_equal(video.cpu().numpy(), fx["video"])
    frames = torch.from_numpy(u8[fr]).cuda()
    ro, rz = torch.from_numpy(fx["recon_one"]).cuda(), torch.from_numpy(fx["recon_zero"]).cuda()
    du8 = torch.from_numpy(np.ascontiguousarray(fx["strip"][:, :, 3 * W:, 0])).cuda()
    strip = render.compose(W, [(PANEL_U8_HWC, frames), (PANEL_F32_CHW, ro), (PANEL_F32_CHW, rz), (PANEL_U8_GREY, du8)])
    assert np.array_equal(strip.cpu().numpy(), fx["strip"])
    inj = torch.from_numpy(fx["injected"]).cuda()
    strip = render.compose(W, [(PANEL_U8_HWC, frames)] + [(PANEL_F32_CHW, inj[:, r]) for r in range(6)])
    assert np.array_equal(strip.cpu().numpy(), fx["inject"])
    # with text: exactly the textless picture plus the overlay and the label, white
    with_text = render.video_frames({"frames": u8[fr], "recon_one": fx["recon_one"], "recon_zero": fx["recon_zero"],
                                     "diff_u8": np.ascontiguousarray(fx["video"][:, W:, 3 * W:4 * W, 0]), "thr_masks": sfx["thr_masks/50"][fr],
                                     "crf_masks": sfx["thr_masks/50"][fr], "gt": sfx["gt"][fr], "preds": fx["preds"][fr],
                                     "thr_iou": float(fx["thr_iou"]), "crf_iou": float(fx["crf_iou"])}).cpu().numpy()
    ov = render.title_overlay(W, float(fx["thr_iou"]), float(fx["crf_iou"]))
    atlas = render.label_atlas(render.label_strings())
    for j, f in enumerate(fr):
        want = fx["video"][j].copy()
        want[ov != 0] = 255
        lab = atlas[render.label_index(fx["preds"][f:f + 1])[0]] != 0
        want[W + 2:W + 2 + lab.shape[0], 2:2 + lab.shape[1]][lab] = 255
        assert np.array_equal(with_text[j], want)
        assert (with_text[j] != fx["video"][j]).any()


def _check_recon_panel(name, ours, ref, ref_chw, E, totals):
    """A truncation may fall on the other side of an integer only where the reference's v * 255 is within 255 E of one."""
    v = np.transpose(ref_chw, (1, 2, 0)) * np.float32(255)                              # the value the reference truncates
    dist = np.abs(v.astype(np.float64) - np.rint(v.astype(np.float64)))
    differs = ours != ref
    step = (ours.astype(np.int64) - ref.astype(np.int64)) % 256
    assert np.isin(step[differs], (1, 255)).all(), (name, np.unique(step[differs]))
    assert (dist[differs] <= 255 * E).all(), (name, float(dist[differs].max()), 255 * E)
    totals[0] += int(differs.sum())
    totals[1] += int((dist <= 255 * TOL).sum())


@pytest.fixture(scope="module")
def e2e(golden_dir):
    """eval_frames -> video_frames, evaluate_strips, inject_strips on the 68 real frames, text=False"""
    sfx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    vae, critic, critic_sd = _vae_and_critic(golden_dir, 32)                             # 68 frames in chunks of 32
    r = seg.eval_frames(u8, vae, sfx["gt"], critic=critic, t=50, keep_device=True)
    video = render.video_frames(r, text=False)
    strips, sparts = render.evaluate_strips(u8, vae, critic=critic, text=False, return_parts=True)
    inject, iparts = render.inject_strips(u8, vae, return_parts=True)
    host = lambda t: t.cpu().numpy()                                                     # noqa: E731
    return {"u8": u8, "gt": sfx["gt"], "r": r, "video": host(video), "strips": host(strips), "inject": host(inject),
            "recon_one": host(r["device"]["recon_one"]), "recon_zero": host(r["device"]["recon_zero"]),
            "s_recon_one": host(sparts["recon_one"]), "s_recon_zero": host(sparts["recon_zero"]), "s_diff_u8": host(sparts["diff_u8"]),
            "injected": host(iparts["injected"]), "vae": vae, "critic_sd": critic_sd}


def test_end_to_end_against_the_reference_pictures(e2e, golden_dir):
    fx = np.load(os.path.join(golden_dir, "render_real.npz"))
    fr, r = fx["frames"], e2e["r"]
    assert set(r) >= {"preds", "diff", "max_values", "diff_u8", "thr_masks", "crf_masks", "thr_iou", "crf_iou", "bins", "mean_max", "hist", "device"}
    assert e2e["video"].shape == (68, 2 * W, 7 * W, 3) and e2e["strips"].shape == (68, W, 4 * W, 3) and e2e["inject"].shape == (68, W, 7 * W, 3)
    E = max(np.abs(e2e["recon_one"][fr] - fx["recon_one"]).max(), np.abs(e2e["recon_zero"][fr] - fx["recon_zero"]).max(),
            np.abs(e2e["s_recon_one"][fr] - fx["recon_one"]).max(), np.abs(e2e["s_recon_zero"][fr] - fx["recon_zero"]).max(),
            np.abs(e2e["injected"][fr] - fx["injected"]).max())
    print(f"E = max |recon_hip - recon_ref| over frames {fr.tolist()}: {E:.3e}")
    assert E <= TOL, E
    totals = [0, 0]
    panel = lambda pic, p, ih=0: pic[ih:, p * W:(p + 1) * W]                             # noqa: E731
    for j, f in enumerate(fr):
        v, s, i = e2e["video"][f], e2e["strips"][f], e2e["inject"][f]
        rv, rs, ri = fx["video"][j], fx["strip"][j], fx["inject"][j]
        assert not v[:W].any() and not rv[:W].any()                                      # the title band, textless
        # frame and ground truth: exact
        for ours, ref in ((panel(v, 0, W), panel(rv, 0, W)), (panel(s, 0), panel(rs, 0)), (panel(i, 0), panel(ri, 0)), (panel(v, 6, W), panel(rv, 6, W))):
            assert np.array_equal(ours, ref)
        assert np.array_equal(panel(v, 0, W), e2e["u8"][f])
        # reconstructions: within the measured error of a truncation boundary
        _check_recon_panel("video recon(pred)", panel(v, 1, W), panel(rv, 1, W), fx["recon_one"][j], E, totals)
        _check_recon_panel("video recon(0)", panel(v, 2, W), panel(rv, 2, W), fx["recon_zero"][j], E, totals)
        _check_recon_panel("strip recon(pred)", panel(s, 1), panel(rs, 1), fx["recon_one"][j], E, totals)
        _check_recon_panel("strip recon(0)", panel(s, 2), panel(rs, 2), fx["recon_zero"][j], E, totals)
        for k in range(6):
            _check_recon_panel(f"inject {k}", panel(i, 1 + k), panel(ri, 1 + k), fx["injected"][j][k], E, totals)
        # difference, thr-mask, crf: the paste of the arrays this run returned, and the fixture's panel wherever they agree
        for p, arr, is_mask in ((3, r["diff_u8"][f], False), (4, r["thr_masks"][f], True), (5, r["crf_masks"][f], True)):
            ours = panel(v, p, W)
            want = np.repeat((arr.astype(np.uint8) * (255 if is_mask else 1))[..., None], 3, -1).astype(np.uint8)
            assert np.array_equal(ours, want), p
            if p != 5:                                             # the fixture's crf panel is its thr-mask panel (identity stand-in)
                same = want[..., 0] == panel(rv, p, W)[..., 0]
                assert np.array_equal(ours[same], panel(rv, p, W)[same])
        assert np.array_equal(panel(rv, 4, W), panel(rv, 5, W))
        want = np.repeat(e2e["s_diff_u8"][f][..., None], 3, -1)
        assert np.array_equal(panel(s, 3), want)
        same = want[..., 0] == panel(rs, 3)[..., 0]
        assert np.array_equal(panel(s, 3)[same], panel(rs, 3)[same])
    print(f"differing reconstruction bytes {totals[0]}, reference values within 255 * {TOL} of an integer {totals[1]}")
    assert totals[0] <= totals[1], totals
    # every other frame: the pictures are the restatement of what the run returned
    for f in (0, 33, 67):
        want = compose_ref([(1, e2e["u8"][f]), (0, e2e["recon_one"][f]), (0, e2e["recon_zero"][f]), (2, r["diff_u8"][f]),
                            (3, r["thr_masks"][f]), (3, r["crf_masks"][f]), (3, e2e["gt"][f])], ih=W)
        assert np.array_equal(e2e["video"][f], want)
        assert np.array_equal(e2e["inject"][f], compose_ref([(1, e2e["u8"][f])] + [(0, e2e["injected"][f][k]) for k in range(6)]))


def test_inject_images_against_the_reference_and_per_frame_inject(golden_dir):
    """inference_b5.npz as test_inference_path_eval_mode reads it: three training steps, then eval mode."""
    fx = np.load(os.path.join(golden_dir, "inference_b5.npz"))
    B = int(fx["batch"])
    assert B == 5 and list(fx["train_steps"]) == [20, 21, 22] and int(fx["step"]) == 9
    vae = VariationalAutoencoder(max_batch=6 * B, seed=0).to("cuda")
    vae.load_reference_params(synth.make_params(0))
    for s in fx["train_steps"]:
        xs, ps, es = (torch.from_numpy(a).cuda() for a in synth.make_batch(1234, int(s), B, 64, first_index=0))
        vae.theta.grad = None
        vae.vae_loss(*vae(xs, ps, eps=es))["total_loss"].backward()
    vae.eval()
    x = torch.from_numpy(synth.make_batch(1234, 9, B, 64, first_index=0)[0]).cuda()
    got = vae.inject_images(x)
    assert got.shape == (B, 6, 3, 64, 64)
    assert np.abs(got[0].cpu().numpy().reshape(6, -1)[:, ::4] - fx["inject_first_frame_sample"]).max() < TOL
    for b in range(B):
        one = torch.stack([t[0] for t in vae.inject(x[b:b + 1])])
        assert (got[b] - one).abs().max().item() < TOL, b
    # train mode changes nothing: the encoder runs in eval mode whatever the module's flag, and leaves the statistics alone
    bn = vae.bn_state.clone()
    vae.train()
    assert torch.equal(vae.inject_images(x), got) and torch.equal(vae.bn_state, bn)
    # more rows than max_batch: several decoder calls, the same bits
    small = VariationalAutoencoder(max_batch=8, seed=0).to("cuda")
    small.theta.data.copy_(vae.theta.data)
    small.bn_state.copy_(vae.bn_state)
    assert torch.equal(small.inject_images(x), got)
    with pytest.raises(ValueError):
        small.inject_images(x, rewards=tuple(range(9)))


def test_compose_is_independent_of_the_batch():
    rng = np.random.default_rng(3)
    B, w = 257, 64
    kinds = [PANEL_U8_HWC, PANEL_F32_CHW, PANEL_F32_CHW, PANEL_U8_GREY, PANEL_MASK, PANEL_MASK, PANEL_MASK]
    dev = [torch.from_numpy(_panel_data(k, B, w, rng)).cuda() for k in kinds]
    preds = torch.from_numpy(rng.random(B).astype(np.float32)).cuda()
    ov = render.title_overlay(w, 0.123, 0.456)
    big = render.compose(w, list(zip(kinds, dev)), w, ov, preds)
    again = render.compose(w, list(zip(kinds, dev)), w, ov, preds)
    assert torch.equal(big, again)
    for b in range(B):
        one = render.compose(w, [(k, t[b:b + 1]) for k, t in zip(kinds, dev)], w, ov, preds[b:b + 1])
        assert torch.equal(one[0], big[b]), b


def test_cli_writes_the_pictures(e2e, tmp_path):
    nets = tmp_path / "nets"
    train.save_networks(e2e["vae"], str(nets))
    torch.save(e2e["critic_sd"], tmp_path / "critic.pt")
    np.save(tmp_path / "u8.npy", e2e["u8"])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(module, *args):
        r = subprocess.run([sys.executable, "-m", module, *args], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout

    def reload(d, n):
        if (d / "pictures.npy").exists():
            return np.load(d / "pictures.npy")
        from PIL import Image
        files = sorted(os.listdir(d))
        assert files[:n] == [f"image-{i:03d}.png" for i in range(n)]
        return np.stack([np.array(Image.open(d / f)) for f in files[:n]])

    common = ["--networks", str(nets), "--critic", str(tmp_path / "critic.pt")]
    out = run("critic_vae_amd.render", "--images", str(tmp_path / "u8.npy"), "--out", str(tmp_path / "strips"), "--no-text", "--chunk", "32", *common)
    assert "wrote 68 pictures" in out
    assert np.array_equal(reload(tmp_path / "strips", 68), e2e["strips"])
    run("critic_vae_amd.render", "-inject", "--images", str(tmp_path / "u8.npy"), "--out", str(tmp_path / "inject"), "--npy", "--chunk", "32", *common)
    assert np.array_equal(reload(tmp_path / "inject", 68), e2e["inject"])
    # segment -video --out: the episode slice X[100:5000:2] is the 68 frames
    X = np.zeros((100 + 2 * 68, 64, 64, 3), np.uint8)
    Y = np.zeros((100 + 2 * 68, 64, 64, 3), np.uint8)
    X[100::2] = e2e["u8"]
    Y[100::2] = (e2e["gt"][..., None] * 255).astype(np.uint8)
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "Y.npy", Y)
    out = run("critic_vae_amd.segment", "-video", "--frames", str(tmp_path / "X.npy"), "--gt", str(tmp_path / "Y.npy"), "--out", str(tmp_path / "video"),
              "--no-text", "--chunk", "32", *common)
    assert f"thr_iou={e2e['r']['thr_iou']}" in out and f"crf_iou={e2e['r']['crf_iou']}" in out
    assert np.array_equal(reload(tmp_path / "video", 68), e2e["video"])
