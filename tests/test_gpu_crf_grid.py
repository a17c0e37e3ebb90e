"""cvae_crf_grid on the MI355X (critic_vae_amd.segment.crf_grid / crf_search): every variant of one call against the float64
reference of tests/crf_ref.py at the bar of segment_tools.crf_bar, the integer counts exactly, snapshots against separate calls,
bitwise independence of a (frame, variant) result from everything else in the call, the scratch, the argument checks, and the
search against the existing route (dense_crf / sweep_maps) on the 68 real frames."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crf_grid_tools as gt_tools  # noqa: E402
import segment_tools as st  # noqa: E402
from crf_ref import crf_ref  # noqa: E402

from critic_vae_amd import lib as cvlib  # noqa: E402
from critic_vae_amd import segment as seg  # noqa: E402
from critic_vae_amd import synth  # noqa: E402
from critic_vae_amd.nets import VariationalAutoencoder  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = st.BAR
_cache = {}


def G():
    return seg._handle(64).crf_grid_group()


def _inputs(w=64):
    if ("in", w) not in _cache:
        fr, pr = st.case_frames(w)
        _cache[("in", w)] = (fr, pr, gt_tools.diff_u8_of(pr))
    return _cache[("in", w)]


def _ref(w, frame, variant, it):
    """float64 reference of one (frame, variant, iteration count), computed once"""
    key = ("ref", w, frame, variant, it)
    if key not in _cache:
        fr, pr, u8 = _inputs(w)
        prob = gt_tools.variant_prob(variant, pr[frame], u8[frame])
        _cache[key] = crf_ref(fr[frame], prob, gt_tools.variant_params(variant, it), variant[1], device="cuda")
    return _cache[key]


def _random_gt(shape, seed=7):
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array([0, 0, 0, 1, 1, 2, 128, 255], np.uint8), size=shape)
    assert {0, 1, 2, 128, 255} <= set(np.unique(g).tolist())
    return g


def _check_variants(labels, q1, w, frames, variants, it, slots=None):
    for k, v in enumerate(variants):
        if slots is not None and k not in slots:
            continue
        worst, bad = 0.0, 0
        for i, f in enumerate(frames):
            lr, qr = _ref(w, f, v, it)
            e, b = st.crf_bar(labels[k, i], q1[k, i], lr, qr)
            worst, bad = max(worst, e), bad + b
        print(f"slot {k} variant {v} it {it}: worst |Q(1) - ref| {worst:.2e}, labels off {bad}")
        assert worst < BAR and bad == 0, (k, v, worst, bad)


def test_variants_against_float64():
    fr, pr, u8 = _inputs()
    vs = gt_tools.variants(2 * G() + 1)                                   # two full groups and a ragged third
    _, labels, q1 = seg.crf_grid(fr, None, gt_tools.KERNEL, vs, (gt_tools.IT,), prob1=pr, diff_u8=u8, labels=True, q1=True)
    assert labels.shape == (len(vs), 3, 64, 64) and q1.shape == labels.shape
    _check_variants(labels.cpu().numpy(), q1.cpu().numpy(), 64, (0, 1, 2), vs, gt_tools.IT)


def test_counts_exact_and_counts_only():
    fr, pr, u8 = _inputs()
    vs = gt_tools.variants(2 * G() + 1)
    gt = _random_gt((3, 64, 64))
    counts, labels = seg.crf_grid(fr, gt, gt_tools.KERNEL, vs, (gt_tools.IT,), prob1=pr, diff_u8=u8, labels=True)
    assert counts.shape == (1, len(vs), 3, 3) and counts.dtype == torch.int64
    lab = labels.cpu().numpy()
    for k in range(len(vs)):
        assert np.array_equal(counts[0, k].cpu().numpy(), st.counts_ref(lab[k], gt)), k
    only = seg.crf_grid(fr, gt, gt_tools.KERNEL, vs, (gt_tools.IT,), prob1=pr, diff_u8=u8)
    assert torch.equal(only, counts)


def test_snapshots_equal_separate_calls():
    fr, pr, u8 = _inputs()
    vs = list(gt_tools.BASE_VARIANTS)
    gt = _random_gt((3, 64, 64), 8)
    snaps = (0, 1, 2, 3)
    counts = seg.crf_grid(fr, gt, gt_tools.KERNEL, vs, snaps, prob1=pr, diff_u8=u8)
    assert counts.shape == (4, len(vs), 3, 3)
    for s in snaps:
        c1, labels, q1 = seg.crf_grid(fr, gt, gt_tools.KERNEL, vs, (s,), prob1=pr, diff_u8=u8, labels=True, q1=True)
        assert torch.equal(c1[0], counts[s]), s
        lab = labels.cpu().numpy()
        for k in range(len(vs)):
            assert np.array_equal(c1[0, k].cpu().numpy(), st.counts_ref(lab[k], gt)), (s, k)
        _check_variants(lab, q1.cpu().numpy(), 64, (0, 1, 2), vs, s)
        if s == 0:
            for k, v in enumerate(vs):
                p = np.stack([gt_tools.variant_prob(v, pr[i], u8[i]) for i in range(3)])
                away = np.abs(p - 0.5) >= BAR
                assert np.array_equal(lab[k][away], (p > 0.5)[away]), k


@pytest.mark.parametrize("variant", [gt_tools.BASE_VARIANTS[0], gt_tools.BASE_VARIANTS[8]])
def test_bitwise_independent_of_slot_group_batch_and_run(variant):
    fr, pr, u8 = _inputs()
    g = G()
    kw = dict(labels=True, q1=True)
    _, l1, q1 = seg.crf_grid(fr, None, gt_tools.KERNEL, [variant], (gt_tools.IT,), prob1=pr, diff_u8=u8, **kw)
    slots = (0, g - 1, g, 2 * g)
    vs = gt_tools.variants(2 * g + 1)
    others = [v for v in gt_tools.BASE_VARIANTS if v != variant]
    vs = [variant if k in slots else others[k % len(others)] for k in range(len(vs))]
    _, lm, qm = seg.crf_grid(fr, None, gt_tools.KERNEL, vs, (gt_tools.IT,), prob1=pr, diff_u8=u8, **kw)
    _, lm2, qm2 = seg.crf_grid(fr, None, gt_tools.KERNEL, vs, (gt_tools.IT,), prob1=pr, diff_u8=u8, **kw)
    assert torch.equal(lm, lm2) and torch.equal(qm, qm2)                 # across two runs
    for k in slots:
        assert torch.equal(lm[k], l1[0]) and torch.equal(qm[k], q1[0]), k
    sel = [0, 1, 2, 1, 0]
    _, lb, qb = seg.crf_grid(fr[sel], None, gt_tools.KERNEL, vs[:g + 1], (gt_tools.IT,), prob1=pr[sel], diff_u8=u8[sel], **kw)
    for pos, f in enumerate(sel):
        for k in (0, g - 1, g):
            assert torch.equal(lb[k, pos], l1[0, f]) and torch.equal(qb[k, pos], q1[0, f]), (pos, k)


def test_width_128():
    fr, pr, u8 = _inputs(128)
    g = G()
    vs = gt_tools.variants(g + 1)
    _, labels, q1 = seg.crf_grid(fr[1:2], None, gt_tools.KERNEL, vs, (gt_tools.IT,), prob1=pr[1:2], diff_u8=u8[1:2],
                                 labels=True, q1=True)
    _check_variants(labels.cpu().numpy(), q1.cpu().numpy(), 128, (1,), vs, gt_tools.IT, slots=(0, g - 1, g))


def _raw_call(h, B, frames, prob1, u8, gt, kernel, variants, snaps, counts, labels, q1, scratch, n_variants=None, n_snaps=None):
    """cvae_crf_grid itself; tensors or None, `scratch` a tensor, an address or None"""
    va = (cvlib.CrfVariant * max(1, len(variants)))(*[cvlib.CrfVariant(int(t), float(pf), float(a), float(b)) for t, pf, a, b in variants])
    sa = (C.c_int32 * max(1, len(snaps)))(*[int(s) for s in snaps])
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())      # noqa: E731
    return h.lib.cvae_crf_grid(h.h, B, ptr(frames), ptr(prob1), ptr(u8), ptr(gt), float(kernel[0]), float(kernel[1]),
                               float(kernel[2]), va, len(variants) if n_variants is None else n_variants, sa,
                               len(snaps) if n_snaps is None else n_snaps, ptr(counts), ptr(labels), ptr(q1), ptr(scratch),
                               torch.cuda.current_stream().cuda_stream)


def test_poisoned_scratch_gives_the_same_bits():
    fr, pr, u8 = (torch.from_numpy(a).cuda() for a in _inputs())
    gt = torch.from_numpy(_random_gt((3, 64, 64), 9)).cuda()
    h = seg._handle(64)
    vs = gt_tools.variants(G() + 3)
    snaps = (0, 2, 3)
    nbytes = h.crf_grid_scratch_bytes(3, len(vs))
    res = []
    for fill in (0x00, 0xFF):
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
        counts = torch.full((len(snaps), len(vs), 3, 3), -1, dtype=torch.int64, device="cuda")
        labels = torch.full((len(vs), 3, 64, 64), 0xAB, dtype=torch.uint8, device="cuda")
        q1 = torch.full((len(vs), 3, 64, 64), float("nan"), device="cuda")
        assert _raw_call(h, 3, fr, pr, u8, gt, gt_tools.KERNEL, vs, snaps, counts, labels, q1, scratch) == 0
        torch.cuda.synchronize()
        res.append((counts, labels, q1.view(torch.int32)))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert int(res[0][1].max()) <= 1 and not torch.isnan(res[0][2].view(torch.float32)).any()       # fully written
    _check_variants(res[1][1].cpu().numpy(), res[1][2].view(torch.float32).cpu().numpy(), 64, (0, 1, 2), vs, 3, slots=(0, G()))


def test_rejected_arguments_leave_outputs_untouched():
    fr, pr, u8 = (torch.from_numpy(a).cuda() for a in _inputs())
    gt = torch.from_numpy(_random_gt((3, 64, 64), 9)).cuda()
    h = seg._handle(64)
    good_v = [(-1, 1e-5, 6, 4), (50, 1e-5, 6, 4)]
    scratch = torch.empty(h.crf_grid_scratch_bytes(3, 64) + 256, dtype=torch.uint8, device="cuda")
    counts = torch.full((8, 64, 3, 3), -7, dtype=torch.int64, device="cuda")
    labels = torch.full((64, 3, 64, 64), 0xAB, dtype=torch.uint8, device="cuda")
    q1 = torch.full((64, 3, 64, 64), 123.0, device="cuda")
    base = dict(B=3, frames=fr, prob1=pr, u8=u8, gt=gt, kernel=gt_tools.KERNEL, variants=good_v, snaps=(0, 2), counts=counts,
                labels=labels, q1=q1, scratch=scratch)
    nan, inf = float("nan"), float("inf")
    bad = {
        "prob1 variant without prob1": dict(prob1=None),
        "threshold variant without diff_u8": dict(u8=None),
        "thr -2": dict(variants=[(-2, 1e-5, 6, 4)]),
        "thr 256": dict(variants=[(256, 1e-5, 6, 4)]),
        "counts without gt": dict(gt=None),
        "no output": dict(counts=None, labels=None, q1=None),
        "unsorted snapshots": dict(snaps=(2, 1)),
        "repeated snapshots": dict(snaps=(1, 1)),
        "negative snapshot": dict(snaps=(-1, 1)),
        "snapshot over 10000": dict(snaps=(1, 10001)),
        "n_variants 0": dict(n_variants=0),
        "n_variants 65": dict(variants=[good_v[0]] * 65),
        "n_snaps 0": dict(n_snaps=0),
        "n_snaps 9": dict(snaps=tuple(range(9))),
        "nan alpha": dict(kernel=(nan, 40, 24)),
        "inf beta": dict(kernel=(48, inf, 24)),
        "nan gamma": dict(kernel=(48, 40, nan)),
        "zero alpha": dict(kernel=(0, 40, 24)),
        "negative gamma": dict(kernel=(48, 40, -1)),
        "nan w1": dict(variants=[(-1, 1e-5, nan, 4)]),
        "inf w2": dict(variants=[(-1, 1e-5, 6, inf)]),
        "negative w1": dict(variants=[(-1, 1e-5, -1, 4)]),
        "nan p_floor": dict(variants=[(-1, nan, 6, 4)]),
        "p_floor 0": dict(variants=[(-1, 0.0, 6, 4)]),
        "p_floor over 1": dict(variants=[(-1, 1.5, 6, 4)]),
        "bad variant in a later group": dict(variants=[good_v[0]] * 9 + [(300, 1e-5, 6, 4)]),
        "null frames": dict(frames=None),
        "null scratch": dict(scratch=None),
        "misaligned scratch": dict(scratch=scratch.data_ptr() + 1),
        "batch 0": dict(B=0),
        "batch too large": dict(B=2 ** 31 // 4096),
    }
    assert _raw_call(h, **dict(base, counts=None, q1=None)) == 0          # the base call itself is accepted
    torch.cuda.synchronize()
    labels.fill_(0xAB)
    for name, over in bad.items():
        assert _raw_call(h, **dict(base, **over)) == -1, name             # CVAE_EINVAL
        assert h.lib.cvae_last_error(), name
    torch.cuda.synchronize()
    assert (counts == -7).all() and (labels == 0xAB).all() and (q1 == 123.0).all()
    assert h.lib.cvae_crf_grid_scratch_bytes(h.h, 3, 0) == -1 and h.lib.cvae_crf_grid_scratch_bytes(h.h, 3, 65) == -1
    assert h.lib.cvae_crf_grid_scratch_bytes(h.h, 0, 1) == -1 and h.lib.cvae_crf_grid_group(None) == -1
    assert h.crf_grid_scratch_bytes(3, 1) < h.crf_grid_scratch_bytes(3, G()) == h.crf_grid_scratch_bytes(3, 64)


def _real_maps(golden_dir):
    fx = np.load(os.path.join(golden_dir, "segment_real_b68.npz"))
    u8 = np.load(os.path.join(golden_dir, "step_real_b68.npz"))["u8"]
    vae = VariationalAutoencoder(max_batch=68, seed=0).to("cuda")
    vae.load_reference_params(synth.make_params(0))
    _, diff, maxv = seg._infer(u8, vae, None, fx["preds"], None)
    return u8, diff, maxv, fx["gt"]


def _grid_order_key(r):
    tp, fn, fp = r["counts"]
    return (-r["crf_iou"], -(tp / (tp + fn + fp) if tp + fn + fp else 1.0), seg.SWEEP.index(r["thr"]))


def test_search_against_the_existing_route(golden_dir):
    frames, diff, maxv, gt = _real_maps(golden_dir)
    rows = seg.crf_search(frames, diff, maxv, gt, thresholds=seg.SWEEP)
    assert len(rows) == len(seg.SWEEP) and {r["thr"] for r in rows} == set(seg.SWEEP)
    assert all(r["params"] == seg.CRF_REF and r["p_floor"] == seg.P_FLOOR for r in rows)
    keys = [_grid_order_key(r) for r in rows]
    assert keys == sorted(keys)                                           # best first, unrounded ratio, then grid order
    by_thr = {r["thr"]: r for r in rows}
    sweep = seg.sweep_maps(frames, diff, maxv, gt)
    for t, thr_iou, _ in sweep:
        assert by_thr[t]["thr_iou"] == thr_iou, t
    u8d, _ = seg.normalize_diffs(diff, maxv)
    variants = [(t, seg.P_FLOOR, seg.CRF_REF[0], seg.CRF_REF[3]) for t in seg.SWEEP]
    kern = (seg.CRF_REF[1], seg.CRF_REF[2], seg.CRF_REF[4])
    counts, labels, q1 = seg.crf_grid(frames, gt, kern, variants, (seg.CRF_REF[5],), diff_u8=u8d, labels=True, q1=True)
    for k, t in enumerate(seg.SWEEP):
        assert by_thr[t]["counts"] == tuple(counts[0, k].sum(0).tolist()), t
        ld, qd = seg.dense_crf(frames, (u8d > t), return_q1=True)
        firm = (qd - 0.5).abs() >= 2 * BAR
        print(f"thr {t}: {int((~firm).sum())} pixels within 2 BAR of 0.5, max |q1 - q1_dense| {float((q1[k] - qd).abs().max()):.2e}")
        assert torch.equal(labels[k][firm], ld[firm]), t
    half = seg.crf_search(frames, diff, maxv, gt, thresholds=seg.SWEEP, skip=2)
    assert half == seg.crf_search(frames[::2], diff[::2], maxv[::2], gt[::2], thresholds=seg.SWEEP)
    assert half != rows
