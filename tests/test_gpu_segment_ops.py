"""The evaluation-path kernels one by one on the MI355X: cvae_dense_crf at parameters whose filters reach across the
frame, with either filter alone, at 0-3 iterations and at the ends of the documented parameter ranges, against the
float64 restatement of tests/crf_ref.py; cvae_diff_grey, cvae_diff_normalize and cvae_mask_counts against exact
references (tests/segment_tools.py), on truncation boundaries, at the clip and with every admitted output combination.

tests/test_host_segment_tools.py shows on the CPU that the CRF cases below would fail this comparison if the kernel
dropped its far Gaussian taps, its far bilateral rows, an LDS chunk or the frame offset.

Measured max |Q(1) - reference| per case (B = 3: a real frame, a structured frame, a white frame; bar 1e-4):

    case          frame 0   frame 1   frame 2         case          frame 0   frame 1   frame 2
    wideA         1.0e-7    9.1e-8    5.5e-8          it2           4.7e-7    1.5e-6    2.6e-9
    wideB         5.8e-7    3.7e-6    2.6e-9          narrow        1.2e-7    1.2e-7    1.7e-8
    wideC         1.1e-7    1.5e-7    2.2e-8          tiny_gamma    7.1e-7    7.3e-6    9.1e-10
    g_only        1.8e-7    8.9e-8    6.0e-8          tiny_alpha    2.3e-6    2.1e-6    1.3e-9
    b_only        5.6e-7    3.7e-6    5.0e-8          tiny_beta     2.0e-6    2.2e-6    2.6e-9
    none          7.5e-8    7.5e-8    1.4e-8          small_alpha   2.3e-6    2.1e-6    1.3e-9
    it1           1.5e-7    5.5e-7    2.6e-9          huge          9.1e-8    9.9e-8    5.2e-8
    wideB at 128 x 128: 3.9e-6; wideB with B = 5: as wideB; p_floor runs (1e-30, 1e-5, 0.5, 1): at most 3.2e-7

No label differed from the reference in any case.  Before the scales of run_crf were clamped, tiny_gamma, tiny_alpha,
tiny_beta (and small_alpha) gave NaN in every Q(1) of every frame; tiny_gamma now equals gamma = 0.05 bit for bit.
cvae_diff_grey used at most 0.62 of its error bound.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_tools as st  # noqa: E402
from crf_ref import crf_ref  # noqa: E402

from critic_vae_amd import segment as seg  # noqa: E402
from critic_vae_amd.lib import Handle  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1
_cache = {}


def _case_frames(w=64):
    if w not in _cache:
        _cache[w] = st.case_frames(w)
    return _cache[w]


def _ref(case, i):
    """the float64 reference of frame i of a 64-wide case, computed once on the device and shared"""
    if (case, i) not in _cache:
        fr, pr = _case_frames()
        _cache[(case, i)] = crf_ref(fr[i], pr[i], st.CRF_CASES[case], st.CASE_P_FLOOR, device="cuda")
    return _cache[(case, i)]


def _run(frames, prob1, params, p_floor=st.CASE_P_FLOOR):
    labels, q1 = seg.dense_crf(frames, prob1, params, p_floor, return_q1=True)
    return labels.cpu().numpy(), q1.cpu().numpy()


def _check(name, labels, q1, refs):
    """the bar of test_gpu_segment._check_against_ref on every frame; prints the figures before it asserts"""
    res = [st.crf_bar(labels[i], q1[i], *refs[i]) for i in range(len(refs))]
    print(f"{name}: max |Q(1) - ref| " + " ".join(f"{e:.2e}" for e, _ in res) + f"  labels off {[b for _, b in res]}")
    assert np.isfinite(q1).all(), name
    for i, (err, bad) in enumerate(res):
        assert err < st.BAR, (name, i, err)
        assert bad == 0, (name, i, bad)


# ---- dense CRF ----
@pytest.mark.parametrize("case", list(st.CRF_CASES))
def test_crf_case(case):
    fr, pr = _case_frames()
    params = st.CRF_CASES[case]
    labels, q1 = _run(fr, pr, params)
    _check(case, labels, q1, [_ref(case, i) for i in range(3)])
    if case == "none":                                   # Q stays softmax(-u) whatever the iteration count
        clear = np.abs(pr - 0.5) > 1e-6
        assert np.array_equal(labels[clear], (pr > 0.5)[clear])
        l0, q0 = _run(fr, pr, params[:5] + (0,))
        assert np.abs(q1 - q0).max() < 1e-6 and np.array_equal(labels, l0)
    if case == "tiny_gamma":                             # an identity Gaussian filter, as at gamma = 0.05
        l5, q5 = _run(fr, pr, params[:4] + (0.05, params[5]))
        d = np.abs(q1.astype(np.float64) - q5)
        print(f"tiny_gamma vs gamma = 0.05: {d.max():.2e}")
        assert np.isfinite(q5).all() and d.max() < st.BAR
        away = np.abs(q5 - 0.5) >= st.BAR
        assert np.array_equal(labels[away], l5[away])


def test_crf_wide_128():
    fr, pr = _case_frames(128)
    labels, q1 = _run(fr[1:2], pr[1:2], st.WIDE_B)
    ref = crf_ref(fr[1], pr[1], st.WIDE_B, st.CASE_P_FLOOR, device="cuda")
    q = ref[1]
    print(f"wideB 128: mid-range {((q > 0.05) & (q < 0.95)).mean():.3f} label 1 {ref[0].mean():.3f}")
    _check("wideB 128", labels, q1, [ref])


def test_crf_wide_repeated_frame_is_bitwise_equal():
    fr, pr = _case_frames()
    sel = [0, 1, 2, 1, 0]
    l5 = seg.dense_crf(fr[sel], pr[sel], st.WIDE_B, st.CASE_P_FLOOR, return_q1=True)
    l3 = seg.dense_crf(fr, pr, st.WIDE_B, st.CASE_P_FLOOR, return_q1=True)
    for out5, out3 in zip(l5, l3):
        assert torch.equal(out5[0], out5[4]) and torch.equal(out5[1], out5[3])
        assert torch.equal(out5[:3], out3)
    _check("wideB B=5", l5[0].cpu().numpy(), l5[1].cpu().numpy(), [_ref("wideB", i) for i in sel])


def _floor_map(p_floor, w=64):
    """prob1 (w,w) float32 of whole rows: 0, 1, 0.5, p_floor, 1 - p_floor, the float32 neighbours of those two on
    both sides, -1e-3 and 1 + 1e-3, repeated down the frame"""
    f = np.float32
    pf, one_m = f(p_floor), f(1) - f(p_floor)
    vals = [f(0), f(1), f(0.5), pf, one_m]
    for v in (pf, one_m):
        vals += [np.nextafter(v, f(-np.inf)), np.nextafter(v, f(np.inf))]
    vals += [f(-1e-3), f(1 + 1e-3)]
    rows = np.array([vals[r % len(vals)] for r in range(w)], f)
    return np.repeat(rows[:, None], w, axis=1)


@pytest.mark.parametrize("p_floor", [1e-30, 1e-5, 0.5, 1.0])
def test_crf_p_floor_range(p_floor):
    fr = _case_frames()[0][1:2]
    prob = _floor_map(p_floor)[None]
    for it in (0, 2):
        params = st.WIDE_B[:5] + (it,)
        labels, q1 = _run(fr, prob, params, p_floor)
        _check(f"p_floor {p_floor:g} it {it}", labels, q1, [crf_ref(fr[0], prob[0], params, p_floor, device="cuda")])
        if it == 0:
            # prob1 > 0.5 with 0 on the tie: at p_floor = 1 only outside [0, 1], where max(prob, 1) is not 1 on both labels
            expect = prob > 0.5 if p_floor < 1 else prob > 1
            assert np.array_equal(labels, expect), p_floor
    if p_floor == 1.0:
        # u(0) = u(1) = 0 for every probability in [0, 1]: Q(1) is exactly 0.5 and every label 0, at any iteration count
        inside = np.clip(prob, 0, 1)
        for it in (0, 1, 2, 3):
            labels, q1 = _run(fr, inside, st.WIDE_B[:5] + (it,), p_floor)
            assert (q1 == 0.5).all() and not labels.any(), it


def test_crf_rejected_arguments_leave_outputs_untouched():
    fr, pr = _case_frames()
    h = Handle(64, 1)
    frames, prob1 = torch.from_numpy(fr).cuda(), torch.from_numpy(pr).cuda()
    labels = torch.full((3, 64, 64), 0xAB, dtype=torch.uint8, device="cuda")
    q1 = torch.full((3, 64, 64), -7.0, device="cuda")
    scratch = torch.empty(h.crf_scratch_bytes(3) + 256, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 256 == 0

    def call(p, scratch_ptr=scratch.data_ptr(), q=q1):
        rc = h.lib.cvae_dense_crf(h.h, 3, frames.data_ptr(), prob1.data_ptr(), C.byref(p), labels.data_ptr(),
                                  None if q is None else q.data_ptr(), scratch_ptr, None)
        torch.cuda.synchronize()
        return rc

    for change in (dict(w1=-1.0), dict(gamma=0.0), dict(p_floor=0.0), dict(iterations=10001)):
        p = seg.crf_params(st.WIDE_B)
        for k, v in change.items():
            setattr(p, k, v)
        assert call(p) == EINVAL, change
    assert call(seg.crf_params(st.WIDE_B), scratch_ptr=scratch.data_ptr() + 4) == EINVAL
    assert (labels == 0xAB).all() and (q1 == -7.0).all()
    assert call(seg.crf_params(st.WIDE_B), q=None) == 0                 # q1 is optional: the same labels without it
    assert (q1 == -7.0).all()
    both = seg.dense_crf(fr, pr, st.WIDE_B, return_q1=True)[0]
    assert torch.equal(labels.bool(), both) and ((labels == 0) | (labels == 1)).all()


# ---- cvae_diff_grey ----
@pytest.mark.parametrize("w", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_diff_grey_against_float64(w, B):
    rng = np.random.default_rng(100 * w + B)
    a = np.tanh(rng.normal(0, 1.5, size=(B, 3, w, w))).astype(np.float32)
    b = np.tanh(rng.normal(0, 1.5, size=(B, 3, w, w))).astype(np.float32)
    b[:, :, 0:3] = a[:, :, 0:3]                                          # equal inputs: exactly 0
    a[:, :, 1, ::2], b[:, :, 1, ::2] = -0.0, 0.0                         # -0.0 against 0.0, both ways round
    a[:, :, 2, ::2], b[:, :, 2, ::2] = 0.0, -0.0
    b[:, 1, 3] = a[:, 1, 3]                                              # one channel equal
    nan_at = (B - 1, 2, w - 1, w - 2)
    b[nan_at] = np.nan
    h = Handle(w, 1)
    out = torch.full((B, w, w), -7.0, device="cuda")
    h.diff_grey(B, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), out)
    out = out.cpu().numpy()
    nan_px = (nan_at[0], nan_at[2], nan_at[3])
    assert np.isnan(out[nan_px])
    ok = np.ones(out.shape, bool)
    ok[nan_px] = False
    assert np.isfinite(out[ok]).all()
    ref, bound = st.grey_ref(a, b), st.grey_bound(a, b)
    err = np.abs(out.astype(np.float64) - ref)
    print(f"diff_grey w {w} B {B}: max err / bound {np.nanmax(err[ok] / np.maximum(bound[ok], 1e-300)):.3f}")
    assert (err[ok] <= bound[ok]).all()
    assert (out[:, 0:3] == 0).all() and not np.signbit(out[:, 0:3]).any()


# ---- cvae_diff_normalize ----
def _normalize_inputs(w, mean_max, factor, B=3):
    rng = np.random.default_rng(w)
    scale = mean_max if mean_max > 0 else 1.0
    diff = (rng.gamma(0.8, 0.5, size=(B, w, w)) * scale).astype(np.float32)
    edge, names = st.boundary_diffs(mean_max, factor)
    pos = rng.choice(w * w, size=len(edge), replace=False)               # each boundary value in every frame,
    for i in range(B):                                                   # at scattered places
        diff[i].reshape(-1)[np.roll(pos, i)] = edge
    gt = (rng.random((B, w, w)) < 0.4)
    gt[B - 1] = False
    return diff, gt.astype(np.uint8) * np.array([1, 2, 255], np.uint8)[rng.integers(0, 3, size=(B, w, w))]


@pytest.mark.parametrize("w", [64, 128])
@pytest.mark.parametrize("mean_max,factor", [(255.0, 1 / 255.0), (0.7431, 1 / 0.7431), (49.0, 1 / 49.0), (0.0, 0.0)])
def test_diff_normalize_boundaries_thresholds_and_outputs(w, mean_max, factor):
    B = 3
    diff, gt = _normalize_inputs(w, mean_max, factor)
    ref = st.diff_u8_ref(diff, mean_max, factor)
    if mean_max == 255.0:
        assert {0, 1, 49, 50, 51, 253, 254, 255} <= set(np.unique(ref).tolist())
    if mean_max == 49.0:
        assert ref.max() == 254                                          # (49 * (1 / 49)) * 255 < 255 in float64
    h = Handle(w, 1)
    dd, gtd = torch.from_numpy(diff).cuda(), torch.from_numpy(gt).cuda()
    g = gt != 0
    hist_ref = np.stack([np.bincount(ref[g], minlength=256), np.bincount(ref[~g], minlength=256)]).astype(np.int64)

    def run(thr, mask, counts, hist, with_gt=True):
        u8 = torch.full((B, w, w), 0xAB, dtype=torch.uint8, device="cuda")
        m = torch.full((B, w, w), 0xAB, dtype=torch.uint8, device="cuda") if mask else None
        c = torch.full((B, 3), -7, dtype=torch.int64, device="cuda") if counts else None
        hh = torch.full((2, 256), 5, dtype=torch.int64, device="cuda") if hist else None
        h.diff_normalize(B, dd, mean_max, factor, thr, gtd if with_gt else None, u8, m, c, hh)
        assert np.array_equal(u8.cpu().numpy(), ref), thr
        if mask:
            assert np.array_equal(m.cpu().numpy(), (ref > thr).astype(np.uint8)), thr
        if counts:
            assert np.array_equal(c.cpu().numpy(), st.counts_ref(ref > thr, gt)), thr
        if hist:
            assert np.array_equal(hh.cpu().numpy(), hist_ref + 5), thr    # added to what the buffer held

    for thr in (0, 1, 49, 50, 254, 255):
        run(thr, True, True, True)
        assert thr < 255 or not (ref > thr).any()                         # at 255 the mask is all clear
    for with_gt in (True, False):                                         # every admitted combination of outputs
        run(50, True, False, False, with_gt)
        run(50, False, False, False, with_gt)
    run(50, False, True, False)
    run(50, False, False, True)
    run(51, True, False, True)


def test_diff_normalize_rejected_arguments_leave_outputs_untouched():
    w, B = 64, 2
    h = Handle(w, 1)
    diff = torch.rand(B, w, w, device="cuda")
    gt = torch.ones(B, w, w, dtype=torch.uint8, device="cuda")
    u8 = torch.full((B, w, w), 0xAB, dtype=torch.uint8, device="cuda")
    mask = torch.full((B, w, w), 0xAB, dtype=torch.uint8, device="cuda")
    counts = torch.full((B, 3), -7, dtype=torch.int64, device="cuda")
    hist = torch.full((2, 256), -7, dtype=torch.int64, device="cuda")

    def call(mean_max, thr, gt_ptr):
        rc = h.lib.cvae_diff_normalize(h.h, B, diff.data_ptr(), mean_max, 1.0, thr, gt_ptr, u8.data_ptr(), mask.data_ptr(),
                                       counts.data_ptr(), hist.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    assert call(1.0, -1, gt.data_ptr()) == EINVAL
    assert call(1.0, 256, gt.data_ptr()) == EINVAL
    assert call(1.0, 50, None) == EINVAL                                  # counts and histogram without gt
    assert call(float("nan"), 50, gt.data_ptr()) == EINVAL
    assert (u8 == 0xAB).all() and (mask == 0xAB).all() and (counts == -7).all() and (hist == -7).all()
    assert call(1.0, 50, gt.data_ptr()) == 0
    assert not (u8 == 0xAB).all() and (counts >= 0).all()


# ---- cvae_mask_counts ----
@pytest.mark.parametrize("w", [64, 128])
@pytest.mark.parametrize("B", [1, 3])
def test_mask_counts_any_nonzero_byte_is_set(w, B):
    rng = np.random.default_rng(7 * w + B)
    byte = np.array([0, 1, 2, 128, 255], np.uint8)
    n = B + 4                                                             # B drawn frames, then set / clear pairings
    mask, gt = byte[rng.integers(0, 5, size=(n, w, w))], byte[rng.integers(0, 5, size=(n, w, w))]
    mask[B], gt[B] = 255, 128                                             # all set against all set
    mask[B + 1], gt[B + 1] = 0, 0                                         # all clear against all clear
    mask[B + 2] = 2                                                       # all set against drawn
    gt[B + 3] = 0                                                         # drawn against all clear
    for s in range(0, n, B):
        m, g = mask[s:s + B], gt[s:s + B]
        c = seg.mask_counts(m, g).cpu().numpy()
        assert np.array_equal(c, st.counts_ref(m, g)), s
    ref = st.counts_ref(mask, gt)
    assert ref[B].tolist() == [w * w, 0, 0] and ref[B + 1].tolist() == [0, 0, 0]
    assert ref[B + 2, 1] == 0 and ref[B + 3, :2].tolist() == [0, 0]
