"""critic_vae_amd.render without a GPU: the text layout against the text calls recorded from the reference's own
get_final_frame (render_real.npz), the label index against Python's formatting, both CLIs' arguments, the writers'
fallback without PIL, and the generator's numpy restatement against the fixture's pictures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_render_golden import compose_ref, panel_f32  # noqa: E402

from critic_vae_amd import render  # noqa: E402
from critic_vae_amd import segment  # noqa: E402

W = 64


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "render_real.npz"))


def _inside(boxes, x0, y0, x1, y1):
    return all(x0 <= b[1] and y0 <= b[2] and b[3] <= x1 and b[4] <= y1 for b in boxes)


def test_text_layout_matches_the_reference_text_calls(fx):
    thr_iou, crf_iou = float(fx["thr_iou"]), float(fx["crf_iou"])
    titles = render.title_calls(W, thr_iou, crf_iou, int(fx["threshold"]))
    strings = render.label_strings()
    assert len(strings) == 11 and strings[0] == "0.0" and strings[10] == "1.0"
    idx = render.label_index(fx["preds"])
    seen = set()
    for i in range(fx["preds"].shape[0]):
        got = titles + [(render.LABEL_XY[0], W + render.LABEL_XY[1], strings[idx[i]])]
        want = [(int(x), int(y), str(s)) for (x, y), s in zip(fx["text_video_xy"][i], fx["text_video"][i])]
        assert got == want, i
        # the strip of image_evaluate: the critic value alone, at (2, 2)
        assert (render.LABEL_XY[0], render.LABEL_XY[1], strings[idx[i]]) == \
            (int(fx["text_strip_xy"][i][0]), int(fx["text_strip_xy"][i][1]), str(fx["text_strip"][i]))
        seen.add(strings[idx[i]])
    assert "1.0" in seen or "0.0" in seen
    # every glyph box inside the picture, the titles inside the black band above their own panel, the label inside the frame panel
    for p, (x, y, s) in enumerate(titles):
        boxes = render.glyph_boxes(x, y, s)
        assert len(boxes) == len(s.replace("\n", "")) and _inside(boxes, p * W, 0, (p + 1) * W, W), (p, s)
    for s in strings:
        assert _inside(render.glyph_boxes(2, W + 2, s), 0, W, W, 2 * W) and _inside(render.glyph_boxes(2, 2, s), 0, 0, W, W)
    # the rasters: white only inside those boxes, something in every box but a space
    ov = render.title_overlay(W, thr_iou, crf_iou, int(fx["threshold"]))
    assert ov.shape == (2 * W, 7 * W) and ov.dtype == np.uint8 and not ov[W:].any()
    cover = np.zeros_like(ov, bool)
    for x, y, s in titles:
        for ch, x0, y0, x1, y1 in render.glyph_boxes(x, y, s):
            cover[y0:y1, x0:x1] = True
            assert ch == " " or ov[y0:y1, x0:x1].any(), (s, ch)
    assert not ov[~cover].any()
    atlas = render.label_atlas(strings)
    assert atlas.shape == (11, render.GLYPH_H, 3 * render.ADVANCE - 1) and all(a.any() for a in atlas)
    assert len({a.tobytes() for a in atlas}) == 11
    # 128-pixel frames: same strings, positions scale with w
    assert [c[0] for c in render.title_calls(128)] == [128 * i + 2 for i in range(7)]
    assert render.title_calls(W)[4][2] == f"thr-mask\nthr={segment.THRESHOLD}"             # no IoU given: none drawn
    with pytest.raises(ValueError):
        render.glyph_boxes(0, 0, "IoU")


def test_label_index_is_pythons_one_decimal_formatting():
    rng = np.random.default_rng(5)
    ties = np.arange(-5, 16, dtype=np.float64) / 10 + 0.05                                 # x.x5
    v = np.concatenate([rng.random(900), ties, np.nextafter(ties.astype(np.float32), np.float32(2)),
                        np.nextafter(ties.astype(np.float32), np.float32(-2)), [0.0, 1.0, 0.25, 0.75, 0.5, 0.95, 0.05],
                        rng.random(30) * 0.1 + 0.9]).astype(np.float32)
    assert v.size >= 1000
    k = render.label_index(v)
    for val, kk in zip(v, k):
        assert f"{float(val):.1f}".replace("-0.0", "0.0") == f"{kk / 10:.1f}".replace("-0.0", "0.0"), (val, kk)
    import torch
    assert np.array_equal(render.label_index(torch.from_numpy(v)).numpy(), k)
    inside = (k >= 0) & (k <= 10)
    strings = render.label_strings()
    assert all(strings[kk] == f"{float(val):.1f}" for val, kk in zip(v[inside & (v >= 0)], k[inside & (v >= 0)]))


def test_restatement_reproduces_the_fixture_pictures(fx, golden_dir):
    """compose_ref on the reference's floats = the reference's PIL pictures (the generator asserts it on all 68 frames)."""
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    sfx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    assert fx["frames"].size >= 2 and fx["video"].shape[1:] == (2 * W, 7 * W, 3)
    wrapped = 0
    for j, f in enumerate(fx["frames"]):
        ro, rz, inj = fx["recon_one"][j], fx["recon_zero"][j], fx["injected"][j]
        assert min(ro.min(), rz.min(), inj.min()) < 0
        wrapped += int((panel_f32(ro) != panel_f32(ro, clamp=True)).sum())
        video = fx["video"][j]
        du8 = video[W:, 3 * W:4 * W, 0]
        v = compose_ref([(1, u8[f]), (0, ro), (0, rz), (2, du8), (3, sfx["thr_masks/50"][f]), (3, sfx["thr_masks/50"][f]),
                         (3, sfx["gt"][f])], ih=W)
        assert np.array_equal(v, video)
        assert np.array_equal(video[W:, 4 * W:5 * W], video[W:, 5 * W:6 * W])              # the generator's CRF is the identity
        assert np.array_equal(compose_ref([(1, u8[f]), (0, ro), (0, rz), (2, du8)]), fx["strip"][j])
        assert np.array_equal(compose_ref([(1, u8[f])] + [(0, inj[r]) for r in range(6)]), fx["inject"][j])
    assert wrapped > 0                                                                     # negative pixels wrap, and it shows
    assert panel_f32(np.full((3, 1, 1), -1.2, np.float32)).ravel().tolist() == [206] * 3
    assert [int(panel_f32(np.full((3, 1, 1), v, np.float32))[0, 0, 0]) for v in (-0.99, -0.3, 1.0, np.nan)] == [4, 180, 255, 0]


def test_cli_arguments():
    a = render.parse_args(["--images", "x.npy", "--networks", "nets", "--out", "o"])
    assert not a.inject and not a.second and a.text and not a.npy and a.chunk == 256
    assert a.critic == os.path.join("nets", segment.CRITIC_FILE)
    a = render.parse_args(["-inject", "--second", "--images", "dir", "--out", "o", "--critic", "c.pt", "--no-text", "--npy", "--chunk", "12"])
    assert a.inject and a.second and not a.text and a.npy and a.critic == "c.pt" and a.chunk == 12
    for bad in ([], ["--images", "x.npy"], ["--out", "o"], ["--images", "x.npy", "--out", "o", "--chunk", "5"]):
        with pytest.raises(SystemExit):
            render.parse_args(bad)
    # segment -video: the new options default to off and need --out
    a = segment.parse_args(["-video"])
    assert a.out is None and not a.gif and a.text
    a = segment.parse_args(["-video", "--out", "d", "--gif", "--no-text", "--second"])
    assert a.out == "d" and a.gif and not a.text and a.second
    for bad in (["-video", "--gif"], ["-video", "--no-text"], ["-video", "-thresh", "--out", "d"], ["--out", "d"]):
        with pytest.raises(SystemExit):
            segment.parse_args(bad)


def test_writers_fall_back_to_npy_without_pil(tmp_path, monkeypatch):
    pics = np.random.default_rng(0).integers(0, 256, size=(3, 8, 16, 3), dtype=np.uint8)
    for name in [m for m in sys.modules if m == "PIL" or m.startswith("PIL.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "PIL", None)                  # `import PIL` now raises ImportError
    assert render._pil_image() is None
    paths = render.save_pngs(str(tmp_path / "a"), pics)
    assert paths == [str(tmp_path / "a" / "pictures.npy")] and np.array_equal(np.load(paths[0]), pics)
    g = render.save_gif(str(tmp_path / "v.gif"), pics)
    assert g == str(tmp_path / "v.gif.npy") and np.array_equal(np.load(g), pics) and not (tmp_path / "v.gif").exists()
    with pytest.raises(RuntimeError):
        render.load_images(str(tmp_path))
    monkeypatch.undo()
    # on request, also where PIL is installed; and with PIL the PNGs hold the same bytes
    paths = render.save_pngs(str(tmp_path / "b"), pics, npy=True)
    assert np.array_equal(np.load(paths[0]), pics)
    Image = render._pil_image()
    if Image is not None:
        paths = render.save_pngs(str(tmp_path / "c"), pics)
        assert [os.path.basename(p) for p in paths] == ["image-000.png", "image-001.png", "image-002.png"]
        assert all(np.array_equal(np.array(Image.open(p)), pics[i]) for i, p in enumerate(paths))
        g = render.save_gif(str(tmp_path / "w.gif"), pics)
        with Image.open(g) as im:
            assert im.n_frames == 3 and im.size == (16, 8)
    np.save(tmp_path / "f.npy", pics[:, :8, :8])
    assert render.load_images(str(tmp_path / "f.npy")).shape == (3, 8, 8, 3)
    with pytest.raises(ValueError):
        np.save(tmp_path / "g.npy", pics.astype(np.float32))
        render.load_images(str(tmp_path / "g.npy"))
