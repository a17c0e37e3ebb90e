"""cvae_mask_objects / cvae_object_overlap on the MI355X against objects_host (critic_vae_amd.objects) by equality over the
whole arrays: every pattern of tests/objects_tools.py at both widths and connectivities, filter off and on; the table sizes;
every optional argument null; batches and slots; the overlap matrix; eval_frames(..., objects=...) on the 68 real frames against
the host route; every CVAE_EINVAL case with pointers that would fault if read; a side stream with the null stream busy; the
command line.  info[..., 3] (passes) is a diagnostic: only 1 <= passes <= W*W + 1 is required, and the largest is printed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_tools as OT  # noqa: E402
import stream_tools  # noqa: E402
from test_gpu_latent import on_side_stream_with_null_busy  # noqa: E402

from critic_vae_amd import lib as cvlib  # noqa: E402
from critic_vae_amd import objects as ob  # noqa: E402
from critic_vae_amd import segment as seg  # noqa: E402
from critic_vae_amd import synth  # noqa: E402
from critic_vae_amd.critic import Critic  # noqa: E402
from critic_vae_amd.nets import VariationalAutoencoder  # noqa: E402
from critic_vae_amd.objects import ObjectFilter  # noqa: E402

pytestmark = pytest.mark.gpu
WIDTHS = (64, 128)
BAD = 0x10                       # a 16-byte aligned address no process has mapped: reading it would fault


@functools.lru_cache(maxsize=None)
def handle(W):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return cvlib.Handle(W, 1)


@functools.lru_cache(maxsize=None)
def pattern_batch(W):
    """(names, masks (P,W,W) uint8 with set bytes of several nonzero values, values (P,W,W) uint8; `full` under values of 255)."""
    P = OT.patterns(W)
    names = tuple(P)
    rng = np.random.default_rng(5 + W)
    masks = np.stack([P[n] for n in names]).astype(np.uint8) * rng.integers(1, 256, size=(len(names), W, W)).astype(np.uint8)
    values = rng.integers(0, 256, size=masks.shape).astype(np.uint8)
    values[names.index("full")] = 255
    return names, masks, values


@functools.lru_cache(maxsize=None)
def host_ref(W, conn, fname, M=32, with_values=True):
    names, masks, values = pattern_batch(W)
    filt = ObjectFilter(connectivity=conn, max_objects=M, **dict(OT.filters())[fname])
    return filt, ob.objects_host(masks, filt, values if with_values else None)


def to_host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def check(dev, ref, W, what):
    dev = to_host(dev) if torch.is_tensor(next(iter(dev.values()))) else dev
    for k in ("mask", "labels", "table"):
        if k in dev:
            assert dev[k].dtype == ref[k].dtype and np.array_equal(dev[k], ref[k]), (what, k, np.argwhere(dev[k] != ref[k])[:4].tolist())
    assert np.array_equal(dev["info"][:, :3], ref["info"][:, :3]), (what, "info", dev["info"][:4].tolist(), ref["info"][:4].tolist())
    passes = dev["info"][:, 3]
    assert (passes >= 1).all() and (passes <= W * W + 1).all(), (what, passes.tolist())
    return passes


@pytest.mark.parametrize("fname", ("off", "on"))
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("W", WIDTHS)
def test_every_pattern_equals_the_host_statement(W, conn, fname):
    names, masks, values = pattern_batch(W)
    filt, ref = host_ref(W, conn, fname)
    r = ob.mask_objects(masks, filt, values=values, labels=True)
    passes = check(r, ref, W, (W, conn, fname))
    worst = int(np.argmax(passes))
    print(f"W={W} conn={conn} filter={fname}: passes max {passes.max()} ({names[worst]}), "
          + ", ".join(f"{n}={p}" for n, p in zip(names, passes.tolist())))
    if fname == "off":
        full = names.index("full")
        assert r["table"][full, 0].tolist() == [W * W, 0, 0, W - 1, W - 1, W * W * (W - 1) // 2, W * W * (W - 1) // 2, 255 * W * W]
        assert int(r["info"][names.index("checker"), 1]) == (W * W // 2 if conn == 4 else 1)          # far more objects than rows


@pytest.mark.parametrize("M", (1, 32, 64))
def test_table_rows(M):
    W = 64
    names, masks, values = pattern_batch(W)
    for conn in (4, 8):
        filt, ref = host_ref(W, conn, "off", M)
        check(ob.mask_objects(masks, filt, values=values, labels=True), ref, W, (M, conn))
    filt, ref = host_ref(128, 4, "on", M)
    check(ob.mask_objects(pattern_batch(128)[1], filt, values=pattern_batch(128)[2], labels=True), ref, 128, (M, "128 on"))


@pytest.mark.parametrize("W", WIDTHS)
def test_optional_arguments_null(W):
    names, masks, values = pattern_batch(W)
    filt, ref = host_ref(W, 8, "on")
    _, ref_nv = host_ref(W, 8, "on", 32, False)
    assert not np.array_equal(ref["table"], ref_nv["table"]) and np.array_equal(ref["table"][..., :7], ref_nv["table"][..., :7])
    check(ob.mask_objects(masks, filt, labels=True), ref_nv, W, "no values")
    H, B = handle(W), masks.shape[0]
    m, v = torch.from_numpy(masks).cuda(), torch.from_numpy(values).cuda()
    for drop in (("mask",), ("labels",), ("table",), ("mask", "labels", "table")):
        out = {"mask": torch.full((B, W, W), 7, dtype=torch.uint8, device="cuda"),
               "labels": torch.full((B, W, W), 7, dtype=torch.uint16, device="cuda"),
               "table": torch.full((B, 32, 8), 7, dtype=torch.int32, device="cuda"),
               "info": torch.full((B, 4), 7, dtype=torch.int32, device="cuda")}
        H.mask_objects(B, m, filt.params(), out["info"], values=v, mask_out=None if "mask" in drop else out["mask"],
                       labels=None if "labels" in drop else out["labels"], table=None if "table" in drop else out["table"])
        got = to_host(out)
        for g in drop:
            assert (got.pop(g) == 7).all(), (drop, g)          # an output that was not passed is not written
        check(got, ref, W, ("null", drop))


def test_batches_and_slots():
    for W in WIDTHS:
        names, masks, values = pattern_batch(W)
        filt, ref = host_ref(W, 4, "on")
        pick = [names.index(n) for n in ("bernoulli_0.593", "ring_in_ring", "spiral_180")]
        for B in (1, 2, 3):
            idx = pick[:B]
            r = to_host(ob.mask_objects(masks[idx], filt, values=values[idx], labels=True))
            check(r, {k: v[idx] for k, v in ref.items()}, W, ("batch", W, B))
        # the same frame at slots 0, 1 and B - 1 among other patterns: bit-equal results, and equal to its result alone
        k = names.index("bernoulli_0.5")
        idx = [k, k] + [i for i in range(len(names)) if i != k] + [k]
        r = to_host(ob.mask_objects(masks[idx], filt, values=values[idx], labels=True))
        check(r, {key: v[idx] for key, v in ref.items()}, W, ("slots", W))
        for key in ("mask", "labels", "table", "info"):
            assert np.array_equal(r[key][0], r[key][1]) and np.array_equal(r[key][0], r[key][-1]), (W, key)


@pytest.mark.parametrize("W", WIDTHS)
def test_object_overlap_equals_numpy(W):
    names, masks, _ = pattern_batch(W)
    a = host_ref(W, 8, "off")[1]["labels"]
    b = host_ref(W, 4, "off")[1]["labels"]                    # the same masks under 4: objects split, labels far past M
    b2 = np.roll(host_ref(W, 4, "on")[1]["labels"], (3, 5), (1, 2))
    assert int(b.max()) > 64 and int(a.max()) > 64
    for la, lb in ((a, b), (b, a), (a, b2)):
        for M in (1, 7, 32, 64):
            got = ob.object_overlap(la, lb, M).cpu().numpy()
            ref = ob.overlap_host(la, lb, M)
            assert got.dtype == np.int32 and np.array_equal(got, ref), (W, M)
    assert not np.array_equal(ob.overlap_host(a, b, 32), ob.overlap_host(b, a, 32))


def _vae_and_critic(golden_dir, max_batch):
    vae = VariationalAutoencoder(max_batch=max_batch, seed=0).to("cuda")
    vae.load_reference_params(synth.make_params(0))
    cw = np.load(os.path.join(golden_dir, "critic_real_b8.npz"))
    critic = Critic(64, handle=cvlib.Handle(64, max_batch)).to("cuda")
    critic.load_state_dict({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")})
    return vae, critic, cw


def _same_value(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def _host_route(mask, gt, u8, filt):
    """objects_host on the mask and on gt, overlap_host, match, panoptic, and the filtered mask's pixel IoU."""
    o = ob.objects_host(mask, filt, u8)
    g = ob.objects_host(gt, ObjectFilter(connectivity=filt.connectivity, max_objects=filt.max_objects))
    inter = ob.overlap_host(o["labels"], g["labels"], filt.max_objects)
    p = ob.panoptic(ob.match(o["table"], o["info"][:, 1], g["table"], g["info"][:, 1], inter))
    p["iou"] = seg.iou(gt, o["mask"])
    return p, o, g


def test_eval_frames_objects_on_the_real_frames(golden_dir):
    fx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    gt = fx["gt"]
    vae, critic, _ = _vae_and_critic(golden_dir, 32)
    filt = ObjectFilter(min_area=4, fill_holes=True)
    plain = seg.eval_frames(u8, vae, gt, critic=critic, t=50)
    r = seg.eval_frames(u8, vae, gt, critic=critic, t=50, objects=filt)
    assert set(r) == set(plain) | {"objects"} and set(r["objects"]) == {"thr", "crf"}
    for k in plain:
        assert _same_value(plain[k], r[k]), k
    for kind in ("thr", "crf"):
        e = r["objects"][kind]
        p, o, g = _host_route(r[f"{kind}_masks"], gt, r["diff_u8"], filt)
        for k in ("iou", "pq", "sq", "rq", "precision", "recall", "tp", "fp", "fn", "truncated_frames"):
            assert e[k] == p[k], (kind, k, e[k], p[k])
        check({k: e[k] for k in ("mask", "labels", "table", "info")}, o, 64, kind)
        assert np.array_equal(e["gt_table"].cpu().numpy(), g["table"]) and np.array_equal(e["gt_info"].cpu().numpy()[:, :3], g["info"][:, :3])
        assert e["table"].is_cuda and e["tp"] + e["fn"] == int(g["info"][:, 1].sum())
        print(f"{kind}: iou {e['iou']} pq {e['pq']:.3f} sq {e['sq']:.3f} rq {e['rq']:.3f} tp {e['tp']} fp {e['fp']} fn {e['fn']} "
              f"(synthetic ground truth)")


def test_every_einval_case_returns_before_the_device():
    H = handle(64)
    ok = ObjectFilter()

    def params(**kw):
        p = ok.params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def objects(B=1, mask=BAD, p=ok.params(), info=BAD, flags=0, values=BAD, mask_out=BAD, labels=BAD, table=BAD):
        with pytest.raises(cvlib.CvaeError) as e:
            H.mask_objects(B, mask, p, info, values=values, mask_out=mask_out, labels=labels, table=table, flags=flags)
        return str(e.value)

    assert "null" in objects(mask=None) and "null" in objects(info=None) and "null" in objects(p=None)
    assert "flags" in objects(flags=1)
    for c in (0, 6, -8, 5):
        assert "connectivity" in objects(p=params(connectivity=c))
    assert "fill_holes" in objects(p=params(fill_holes=2))
    assert "min_area" in objects(p=params(min_area=0)) and "min_area" in objects(p=params(min_area=-3))
    assert "keep_largest" in objects(p=params(keep_largest=-1))
    for m in (0, -1, 65):
        assert "max_objects" in objects(p=params(max_objects=m))
    for B in (0, -1, 1 << 19, (1 << 31) - 1):                 # 2^19 * 64 * 64 = 2^31
        assert "batch" in objects(B=B)
    assert "aligned" in objects(mask=BAD + 4) and "aligned" in objects(labels=BAD + 8) and "aligned" in objects(info=BAD + 2)

    def overlap(B=1, a=BAD, b=BAD, M=8, inter=BAD, flags=0):
        with pytest.raises(cvlib.CvaeError) as e:
            H.object_overlap(B, a, b, M, inter, flags=flags)
        return str(e.value)

    assert "null" in overlap(a=None) and "null" in overlap(b=None) and "null" in overlap(inter=None)
    assert "flags" in overlap(flags=2) and "max_objects" in overlap(M=0) and "max_objects" in overlap(M=65)
    assert "batch" in overlap(B=0) and "batch" in overlap(B=1 << 19) and "aligned" in overlap(a=BAD + 2)
    H128 = handle(128)
    with pytest.raises(cvlib.CvaeError, match="batch"):
        H128.mask_objects(1 << 17, BAD, ok.params(), BAD)
    # a batch above the handle's max_batch (1) is fine
    m = torch.from_numpy(pattern_batch(64)[1][:3]).cuda()
    assert ob.mask_objects(m)["info"].shape == (3, 4)


def test_side_stream_with_the_null_stream_busy():
    for name in ("cvae_mask_objects", "cvae_object_overlap"):
        assert name not in stream_tools.header_stream_entries()          # they end in (stream, flags): the registry does not see them
    W = 64
    names, masks, values = pattern_batch(W)
    filt, ref = host_ref(W, 8, "on")
    H, B = handle(W), masks.shape[0]
    m, v = torch.from_numpy(masks).cuda(), torch.from_numpy(values).cuda()
    info = torch.zeros(B, 4, dtype=torch.int32, device="cuda")
    table = torch.zeros(B, 32, 8, dtype=torch.int32, device="cuda")
    labels = torch.zeros(B, W, W, dtype=torch.uint16, device="cuda")
    got = on_side_stream_with_null_busy(lambda: H.mask_objects(B, m, filt.params(), info, values=v, labels=labels, table=table), table)
    assert np.array_equal(got.numpy(), ref["table"])
    la = torch.from_numpy(ref["labels"]).cuda()
    lb = torch.from_numpy(host_ref(W, 4, "off")[1]["labels"]).cuda()
    inter = torch.zeros(B, 16, 16, dtype=torch.int32, device="cuda")
    got = on_side_stream_with_null_busy(lambda: H.object_overlap(B, la, lb, 16, inter), inter)
    assert np.array_equal(got.numpy(), ob.overlap_host(ref["labels"], host_ref(W, 4, "off")[1]["labels"], 16))


def test_cli_objects_out_equals_the_api(golden_dir, tmp_path, capsys):
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    gt = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))["gt"]
    n = 100 + 2 * 68                                          # load_episode keeps frames 100, 102, ...: the 68 frames
    X = np.zeros((n, 64, 64, 3), np.uint8)
    Y = np.zeros((n, 64, 64, 3), np.uint8)
    X[100::2], Y[100::2] = u8, gt[..., None]
    np.save(tmp_path / "X.npy", X)
    np.save(tmp_path / "Y.npy", Y)
    _, critic, cw = _vae_and_critic(golden_dir, 68)
    torch.save({k[2:]: torch.from_numpy(cw[k]) for k in cw.files if k.startswith("w/")}, tmp_path / "critic.pt")
    out = tmp_path / "objects.npz"
    argv = ["-video", "--frames", str(tmp_path / "X.npy"), "--gt", str(tmp_path / "Y.npy"), "--critic", str(tmp_path / "critic.pt"),
            "--mask-source", "critic-grad", "--networks", str(tmp_path / "none"), "--chunk", "68", "--objects", "--connectivity", "4",
            "--fill-holes", "--min-area", "4", "--max-objects", "16", "--objects-out", str(out)]
    assert seg.main(argv) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 4 and lines[2].startswith("objects thr: iou=") and lines[3].startswith("objects crf: iou=")
    preds, maps, maxv = seg.critic_maps(u8, critic, "grad", chunk=68)
    filt = ObjectFilter(4, True, 4, 0, 16)
    r = seg.eval_maps(u8, maps, maxv, preds, gt, objects=filt)
    z = np.load(out)
    assert set(z.files) == {f"{k}_{a}" for k in ("thr", "crf", "gt") for a in ("info", "table", "centroids")}
    for kind in ("thr", "crf"):
        e = r["objects"][kind]
        assert np.array_equal(z[f"{kind}_info"][:, :3], e["info"].cpu().numpy()[:, :3]) and np.array_equal(z[f"{kind}_table"], e["table"].cpu().numpy())
        assert np.array_equal(z[f"{kind}_centroids"], ob.centroids(e["table"]), equal_nan=True)
        assert f"tp={e['tp']}, fp={e['fp']}, fn={e['fn']}" in lines[2 if kind == "thr" else 3]
    assert np.array_equal(z["gt_table"], r["objects"]["thr"]["gt_table"].cpu().numpy())
