"""Critic-side masks without a GPU: the restatement tests/critic_saliency_ref.py against the fixture the reference's own
class wrote (critic_saliency_real.npz), what cvae_critic_collect / cvae_critic_saliency / cvae_critic_occlusion reject before
they touch a device, the bindings, and the command line of `segment -video --mask-source`."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_saliency_ref as sref                                # noqa: E402
import critic_train_ref as ref                                    # noqa: E402
from critic_vae_amd import lib as cvlib                           # noqa: E402
from critic_vae_amd import segment as seg                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cvae_critic_collect", "cvae_critic_saliency", "cvae_critic_occlusion")
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "critic_saliency_real.npz"))
    ck = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"][z["frames"]]
    return dict(z=z, w={k: ck["w/" + k] for k, _ in ref.KEYS}, x=ref.frames_to_x(u8))


def gap(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_fixture_is_small_and_holds_data_only(golden_dir):
    path = os.path.join(golden_dir, "critic_saliency_real.npz")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(golden_dir, "step_real_b68.npz")) < 1 << 20
    z = np.load(path)                                             # allow_pickle=False: arrays only
    assert all(z[k].dtype.kind in "fiu" for k in z.files)


def test_ref_reproduces_the_embeddings(fx):
    z = fx["z"]
    pred, embeds = sref.embeddings(fx["w"], fx["x"])
    assert gap(pred, z["pred"]) <= 1e-12
    for i, (e, shape) in enumerate(zip(embeds, sref.EMBED_SHAPES)):
        assert e.shape == (3,) + shape
        assert np.array_equal(e.astype(np.float32), z[f"e{i + 1}"]), f"e{i + 1}"      # stored rounded to fp32
    # the reference's list: a pooled map is >= 0, and the bottleneck is what crit reads
    assert all((e >= 0).all() for e in embeds) and embeds[0].max() > 0


def test_ref_reproduces_the_logit_gradient(fx):
    z = fx["z"]
    r = sref.logit_grad(fx["w"], fx["x"])
    assert gap(r["grad"], z["grad"]) <= 1e-12 and gap(r["logit"], z["logit"]) <= 1e-12
    assert np.array_equal(r["decisions"], z["decisions"])
    assert np.allclose(1 / (1 + np.exp(-z["logit"])), z["pred"].reshape(-1), atol=1e-12)
    assert np.abs(z["grad"]).reshape(3, -1).max(1).min() > 0.1
    # imposing a run's own decisions changes nothing; fp32 follows within the gap the generator measured
    again = sref.logit_grad(fx["w"], fx["x"], decisions=z["decisions"])
    assert np.array_equal(again["grad"], r["grad"])
    r32 = sref.logit_grad(fx["w"], fx["x"], torch.float32)
    rel = (np.abs(r32["grad"].astype(np.float64) - z["grad"]).reshape(3, -1).max(1) / np.abs(z["grad"]).reshape(3, -1).max(1)).max()
    assert rel <= 1e-5 and int((r32["decisions"] != z["decisions"]).sum()) == int(z["gap32/flips"]) == 0


def test_ref_reproduces_integrated_gradients(fx):
    z = fx["z"]
    n = int(z["ig_steps"])
    r = sref.integrated_gradients(fx["w"], fx["x"], n)
    assert n == 4 and gap(r["grad"], z["ig"]) <= 1e-12 and np.array_equal(r["decisions"], z["decisions"])
    # the last pass runs on x itself: k / n == 1 leaves the bits
    assert np.array_equal(sref.scaled_frames(fx["x"], n, n), fx["x"])
    # completeness: the attributions sum to logit(x) - logit(black) as the Riemann sum converges (the scaling by x and 1 / N
    # is right): the miss at N = 64 is below that at N = 4 on every frame, and below 0.15 (measured 0.08 .. 0.11 of 0.7 .. 4.0)
    z0 = sref.logit_grad(fx["w"], np.zeros_like(fx["x"]))["logit"]
    miss4 = np.abs(z["ig"].reshape(3, -1).sum(1) - (z["logit"] - z0))
    miss64 = np.abs(sref.integrated_gradients(fx["w"], fx["x"], 64)["grad"].reshape(3, -1).sum(1) - (z["logit"] - z0))
    assert (miss64 < miss4).all() and (miss64 < 0.15).all(), (miss4, miss64)


def test_ref_reproduces_occlusion(fx):
    z = fx["z"]
    r = sref.occlusion(fx["w"], fx["x"], int(z["occ_patch"]), z["occ_fill"])
    assert gap(r["drop"], z["occ_drop"]) <= 1e-12 and r["drop"].shape == (3, 4, 4)
    assert (r["map"][:, :16, 16:32] == np.maximum(r["drop"][:, 0, 1], 0)[:, None, None]).all()
    assert np.array_equal(r["max_values"], np.maximum(r["drop"], 0).reshape(3, -1).max(1)) and (r["max_values"] > 0).all()
    occ = sref.occluded_frames(fx["x"][0], 16, z["occ_fill"])
    assert occ.shape == (16, 3, 64, 64) and (occ[5, :, 16:32, 16:32] == z["occ_fill"].reshape(3, 1, 1)).all()
    changed = (occ[5] != fx["x"][0]).any(0)
    assert not changed[:16].any() and not changed[32:].any() and not changed[:, :16].any() and not changed[:, 32:].any()


def test_grey_map_weights_are_diff_greys():
    src = open(os.path.join(ROOT, "critic-vae_amd", "csrc", "critic.hip")).read()
    assert "r * 0.2989f + g * 0.5870f + bl * 0.1140f" in src
    g = np.zeros((1, 3, 64, 64))
    g[0, 0, 1, 2], g[0, 1, 1, 2], g[0, 2, 1, 2] = -1.0, 2.0, -4.0
    want = float(np.float32(0.2989)) + 2 * float(np.float32(0.5870)) + 4 * float(np.float32(0.1140))
    assert sref.grey_map(g)[0, 1, 2] == want and sref.grey_map(g).sum() == want


def test_lib_binds_every_new_symbol():
    lib = cvlib.load()
    header = open(os.path.join(ROOT, "include", "cvae.h")).read()
    for name in NEW:
        assert name in cvlib.EXPORTS and hasattr(lib, name) and re.search(rf"\bint {name}\(cvae_handle h, int32_t batch,", header), name
    assert int(re.search(r"#define CVAE_CRITIC_IG_MAX_STEPS (\d+)", header).group(1)) == cvlib.CRITIC_IG_MAX_STEPS == 256
    assert cvlib.CRITIC_EMBED_SHAPES == sref.EMBED_SHAPES and cvlib.CRITIC_OCCLUSION_PATCHES == (4, 8, 16)
    for m in ("critic_collect", "critic_saliency", "critic_occlusion"):
        assert callable(getattr(cvlib.Handle, m))


OK = 4096                                                         # non-null, 16-byte aligned, never dereferenced


def _err(lib):
    return lib.cvae_last_error().decode()


def test_collect_rejects_bad_arguments_before_any_device_access():
    lib, h = cvlib.load(), cvlib.Handle(64, 4)

    def call(hh=h.h, B=4, x=OK, params=OK, pred=OK, e=(OK, OK, OK, OK, OK)):
        return lib.cvae_critic_collect(hh, B, x, params, pred, *e, None)

    assert call(hh=None) == EINVAL and "null handle" in _err(lib)
    for B in (0, 65537, -1):
        assert call(B=B) == EINVAL and f"batch {B} outside [1, 65536]" in _err(lib)
    assert call(hh=cvlib.Handle(128, 2).h) == EUNSUPPORTED and "width 128" in _err(lib) and "64x64" in _err(lib)
    assert call(x=None) == EINVAL and "x is null" in _err(lib)
    assert call(x=OK + 8) == EINVAL and "x must be 16-byte aligned" in _err(lib)
    assert call(params=None) == EINVAL and "critic_params" in _err(lib)
    assert call(pred=None) == EINVAL and "pred is null" in _err(lib)
    assert call(e=(OK, OK, OK + 2, OK, OK)) == EINVAL and "e3 must be 4-byte aligned" in _err(lib)
    assert all(m.startswith("cvae_critic_collect:") for m in (_err(lib),))


def test_saliency_rejects_bad_arguments_before_any_device_access():
    lib, h = cvlib.load(), cvlib.Handle(64, 4)

    def call(hh=h.h, B=4, x=OK, params=OK, steps=1, pred=OK, grad=OK, map_=OK, maxv=OK, dec=OK):
        return lib.cvae_critic_saliency(hh, B, x, params, steps, pred, grad, map_, maxv, dec, None)

    assert call(hh=None) == EINVAL and "null handle" in _err(lib)
    for B in (0, 65537):
        assert call(B=B) == EINVAL and f"batch {B} outside" in _err(lib)
    assert call(hh=cvlib.Handle(128, 2).h) == EUNSUPPORTED and "width 128" in _err(lib)
    for steps in (0, 257, -3):
        assert call(steps=steps) == EINVAL and f"steps {steps} outside [1, 256]" in _err(lib)
    assert call(x=OK + 4) == EINVAL and "x must be 16-byte aligned" in _err(lib)
    assert call(x=None) == EINVAL and "x is null" in _err(lib)
    assert call(map_=None) == EINVAL and "map is null" in _err(lib)
    assert call(maxv=None) == EINVAL and "max_values is null" in _err(lib)
    assert call(pred=None) == EINVAL and "pred is null" in _err(lib)
    assert call(dec=OK + 1) == EINVAL and "decisions must be 4-byte aligned" in _err(lib)
    assert call(grad=OK + 2) == EINVAL and "grad must be 4-byte aligned" in _err(lib)
    assert _err(lib).startswith("cvae_critic_saliency:")


def test_occlusion_rejects_bad_arguments_before_any_device_access():
    lib, h = cvlib.load(), cvlib.Handle(64, 4)

    def call(hh=h.h, B=4, x=OK, params=OK, patch=8, pred=OK, drop=OK, map_=OK, maxv=OK):
        return lib.cvae_critic_occlusion(hh, B, x, params, patch, 0.5, 0.5, 0.5, pred, drop, map_, maxv, None)

    assert call(hh=None) == EINVAL and "null handle" in _err(lib)
    for B in (0, 65537):
        assert call(B=B) == EINVAL and f"batch {B} outside" in _err(lib)
    assert call(hh=cvlib.Handle(128, 2).h) == EUNSUPPORTED and "width 128" in _err(lib)
    for patch in (5, 0, 32, 2):
        assert call(patch=patch) == EINVAL and f"patch {patch} (4, 8 or 16)" in _err(lib)
    assert call(x=OK + 8) == EINVAL and "x must be 16-byte aligned" in _err(lib)
    assert call(map_=None) == EINVAL and "map is null" in _err(lib)
    assert call(drop=None) == EINVAL and "drop is null" in _err(lib)
    assert call(maxv=OK + 2) == EINVAL and "max_values must be 4-byte aligned" in _err(lib)
    assert _err(lib).startswith("cvae_critic_occlusion:")


def test_cli_parses_the_mask_source_flags():
    a = seg.parse_args(["-video"])
    assert a.mask_source == "vae" and a.ig_steps == seg.IG_STEPS == 32 and a.occlusion_patch == seg.OCCLUSION_PATCH == 8
    a = seg.parse_args(["-video", "-thresh", "--mask-source", "critic-ig", "--ig-steps", "16", "--critic", "c.pt"])
    assert a.mask_source == "critic-ig" and a.ig_steps == 16 and a.thresh and a.critic == "c.pt"
    a = seg.parse_args(["-video", "--mask-source", "critic-occlusion", "--occlusion-patch", "16"])
    assert a.occlusion_patch == 16 and seg.MASK_SOURCES[a.mask_source] == "occlusion"
    assert seg.MASK_SOURCES == {"vae": None, "critic-grad": "grad", "critic-ig": "ig", "critic-occlusion": "occlusion"}


def test_cli_refuses_pictures_and_bad_values_with_a_critic_source(capsys):
    for argv, msg in ((["-video", "--mask-source", "critic-grad", "--out", "d"], "reconstruction panels"),
                      (["-video", "--mask-source", "critic-occlusion", "--out", "d", "--gif"], "reconstruction panels"),
                      (["-video", "--mask-source", "critic-ig", "--second"], "--second selects a VAE"),
                      (["-video", "--mask-source", "critic-ig", "--ig-steps", "1"], "--ig-steps must be in 2..256"),
                      (["-video", "--mask-source", "critic-ig", "--ig-steps", "257"], "--ig-steps must be in 2..256"),
                      (["-video", "--mask-source", "critic-occlusion", "--occlusion-patch", "5"], "invalid choice"),
                      (["-video", "--mask-source", "critic"], "invalid choice")):
        with pytest.raises(SystemExit):
            seg.parse_args(argv)
        assert msg in capsys.readouterr().err, argv
    assert seg.parse_args(["-video", "--out", "d"]).out == "d"      # the VAE source still writes pictures
