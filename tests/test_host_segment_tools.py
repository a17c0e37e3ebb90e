"""The tools of the segmentation GPU tests (tests/segment_tools.py), checked on the CPU: every case of CRF_CASES is
non-degenerate (a), resolved by float32 arithmetic a decade below the bar (b) and moved a hundred bars by each
knockout of the reference that applies to it (c); the two parameter sets of test_gpu_segment.py are not (the gap);
the pixel and integer references against hand-computed values.

Measured here (frames 0 / 1 of case_frames(64); knockout = max change of the reference's Q(1)):

    case     mid-range    label 1      float32   gauss_far  bilateral_far_rows  last_chunk   frame_offset
    wideA    1.00 / 1.00  0.52 / 0.45  1.0e-7    1.7e-1     1.6e-2              3.3e-2       8.6e-1
    wideB    0.98 / 0.56  0.67 / 0.49  3.7e-6    4.6e-1     4.8e-1              8.7e-1       1.0e+0
    wideC    1.00 / 1.00  0.50 / 0.23  1.7e-7    2.8e-1     3.3e-2              1.3e-1       9.5e-1
    g_only   1.00 / 1.00  0.43 / 0.35  2.1e-7    5.8e-1     -                   -            9.1e-1
    b_only   0.99 / 0.56  0.65 / 0.51  3.7e-6    -          4.3e-1              8.0e-1       9.9e-1
    it1      1.00 / 1.00  0.51 / 0.50  5.6e-7    -          -                   -            9.4e-1
    it2      1.00 / 0.79  0.55 / 0.50  1.5e-6    -          -                   -            9.9e-1
    narrow   0.98 / 0.99  0.50 / 0.50  1.2e-7    -          -                   -            3.5e-1

narrow was retuned: with the weights 4 / 3 of the first draft the mean field saturates (3.7 % of pixels mid-range),
with 0.6 / 0.4 it does not.  last_chunk moves the real frame alone by only 3.2e-3 (wideA) and 2.4e-3 (wideC), still
twenty bars; the structured frame of the same call carries the case over 1e-2.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_tools as st  # noqa: E402
from crf_ref import CRF_REF, crf_ref  # noqa: E402

CONDITIONED = [c for c in st.CRF_CASES if c not in st.UNCONDITIONED]
_cache = {}


def _frames():
    if "frames" not in _cache:
        _cache["frames"] = st.case_frames(64)
    return _cache["frames"]


def _ref(case, i):
    """the float64 reference of frame i of a case, computed once"""
    if (case, i) not in _cache:
        fr, pr = _frames()
        _cache[(case, i)] = crf_ref(fr[i], pr[i], st.CRF_CASES[case], st.CASE_P_FLOOR)
    return _cache[(case, i)]


def test_case_table_and_inputs():
    assert st.CRF_CASES["it1"] == (6, 48, 40, 4, 24, 1) and st.CRF_CASES["it2"] == (6, 48, 40, 4, 24, 2)
    assert set(st.KNOCKOUTS["frame_offset"]) == set(CONDITIONED) and len(CONDITIONED) == 8
    fr, pr = _frames()
    assert fr.shape == (3, 64, 64, 3) and fr.dtype == np.uint8 and pr.shape == (3, 64, 64) and pr.dtype == np.float32
    assert (fr[2] == 255).all() and (pr[2] == 1).all()
    assert len({fr[i].tobytes() for i in range(3)}) == 3
    for w, seed in ((64, 2), (64, 10), (128, 2)):
        p = st.soft_prob(w, seed)
        assert p.shape == (w, w) and abs(p.min() - 0.05) < 1e-6 and abs(p.max() - 0.95) < 1e-6
        assert abs(np.median(p) - 0.5) < 1e-3
        assert np.abs(np.diff(p, axis=0)).max() < 0.2 and np.abs(np.diff(p, axis=1)).max() < 0.2     # smooth
    fr128, pr128 = st.case_frames(128)
    assert fr128.shape == (3, 128, 128, 3) and pr128.shape == (3, 128, 128)


@pytest.mark.parametrize("case", CONDITIONED)
def test_case_is_non_degenerate_and_resolved_by_float32(case):
    fr, pr = _frames()
    for i in (0, 1):
        lab, q = _ref(case, i)
        mid = ((q > 0.05) & (q < 0.95)).mean()
        l32, q32 = st.crf_f32(fr[i], pr[i], st.CRF_CASES[case], st.CASE_P_FLOOR)
        err, bad = st.crf_bar(l32, q32, lab, q)
        print(f"{case} frame {i}: mid-range {mid:.3f}, label 1 {lab.mean():.3f}, float32 {err:.2e}")
        assert mid >= 0.5, (case, i, mid)                                    # a
        assert 0.1 <= lab.mean() <= 0.9, (case, i, lab.mean())               # a
        assert err <= 1e-5 and bad == 0, (case, i, err, bad)                 # b


@pytest.mark.parametrize("case", CONDITIONED)
def test_knockouts_bite(case):
    """c, and what the GPU test's comparison would say of a kernel with that error: it fails the bar"""
    fr, pr = _frames()
    for kind in ("gauss_far", "bilateral_far_rows", "last_chunk"):
        if case not in st.KNOCKOUTS[kind]:
            continue
        moved = []
        for i in (0, 1):
            lk, qk = st.crf_ref_knockout(fr[i], pr[i], st.CRF_CASES[case], st.CASE_P_FLOOR, kind)
            moved.append(st.crf_bar(lk, qk, *_ref(case, i))[0])
        print(f"{case} {kind}: {moved[0]:.2e} {moved[1]:.2e}")
        assert max(moved) >= 1e-2, (case, kind, moved)
        assert min(moved) >= 10 * st.BAR, (case, kind, moved)                # each frame alone fails the bar too
    lk, qk = st.crf_ref_knockout(fr, pr, st.CRF_CASES[case], st.CASE_P_FLOOR, "frame_offset")
    moved = [st.crf_bar(lk[i], qk[i], *_ref(case, i))[0] for i in (0, 1)]
    print(f"{case} frame_offset: {moved[0]:.2e} {moved[1]:.2e}")
    assert min(moved) >= 1e-2, (case, moved)


def test_frame_offset_of_one_frame_is_the_reference():
    fr, pr = _frames()
    lk, qk = st.crf_ref_knockout(fr[1:2], pr[1:2], st.CRF_CASES["wideB"], st.CASE_P_FLOOR, "frame_offset")
    lab, q = _ref("wideB", 1)
    assert np.abs(qk[0] - q).max() < 1e-12 and np.array_equal(lk[0] | (np.abs(q - 0.5) < 1e-9), lab | (np.abs(q - 0.5) < 1e-9))


def test_knockout_restores_the_reference():
    import crf_ref as mod
    orig = mod._kernel_rows
    fr, pr = _frames()
    st.crf_ref_knockout(fr[1][:16, :16], pr[1][:16, :16], (1, 4, 40, 1, 4, 1), 1e-5, "gauss_far")
    assert mod._kernel_rows is orig
    # on a 16 x 16 frame no two rows are more than 40 apart: bilateral_far_rows cuts nothing
    a = crf_ref(fr[1][:16, :16], pr[1][:16, :16], (1, 4, 40, 1, 4, 1), 1e-5)[1]
    b = st.crf_ref_knockout(fr[1][:16, :16], pr[1][:16, :16], (1, 4, 40, 1, 4, 1), 1e-5, "bilateral_far_rows")[1]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("params,p_floor", [(CRF_REF, 1e-5), ((5, 6, 20.0, 3, 3.0, 4), 1e-3)])
def test_the_gap_short_range_sets_cannot_see_far_terms(params, p_floor):
    """At the two sets of test_gpu_segment.py a reference without its far terms still passes the bar: those
    comparisons cannot tell whether the kernel computes them."""
    fr, masks = st._structured_frames(3, 64, 11)
    for i, prob in ((2, masks[2]), (1, st.soft_prob(64, 2))):
        lab, q = crf_ref(fr[i], prob, params, p_floor)
        for kind in ("gauss_far", "bilateral_far_rows"):
            lk, qk = st.crf_ref_knockout(fr[i], prob, params, p_floor, kind)
            err, bad = st.crf_bar(lk, qk, lab, q)
            print(f"{params} frame {i} {kind}: {err:.2e}")
            assert err < st.BAR and bad == 0, (params, i, kind, err, bad)


def test_crf_bar_counts_labels_away_from_ties_only():
    qr = np.array([[0.2, 0.5 + 5e-5], [0.9, 0.50011]])
    lr = qr > 0.5
    assert st.crf_bar(lr, qr, lr, qr) == (0.0, 0)
    assert st.crf_bar(~lr, qr, lr, qr) == (0.0, 3)             # the pixel within 1e-4 of 0.5 may take either label
    err, bad = st.crf_bar(lr, qr + np.array([[2e-4, 0], [0, 0]]), lr, qr)
    assert abs(err - 2e-4) < 1e-12 and bad == 0


def test_grey_ref_and_bound():
    a = np.zeros((1, 3, 1, 2), np.float32)
    b = np.zeros((1, 3, 1, 2), np.float32)
    b[0, :, 0, 0] = (1.0, -2.0, 0.5)
    a[0, :, 0, 1] = (0.25, 0.25, 0.25)
    g = st.grey_ref(a, b)
    assert g.dtype == np.float64 and g.shape == (1, 1, 2)
    assert g[0, 0, 0] == 0.2989 * 1.0 + 0.5870 * 2.0 + 0.1140 * 0.5
    assert g[0, 0, 1] == 0.2989 * 0.25 + 0.5870 * 0.25 + 0.1140 * 0.25
    assert np.array_equal(st.grey_bound(a, b), 5 * 2.0 ** -24 * g)
    assert (st.grey_ref(a, a) == 0).all()


def test_diff_u8_ref_hand_values():
    d = np.array([0.0, -0.0, 1.0, 50.0, 50.999, 51.0, 254.999, 255.0, 300.0, np.inf, 1e-45], np.float32)
    assert st.diff_u8_ref(d, 255.0, 1 / 255.0).tolist() == [0, 0, 1, 50, 50, 51, 254, 255, 255, 255, 0]
    assert st.diff_u8_ref(d, 0.0, 0.0).tolist() == [0] * len(d)
    assert st.diff_u8_ref(np.array([0.5, 1.0, 2.0], np.float32), 1.0, 1.0).tolist() == [127, 255, 255]
    # (49 * (1 / 49)) * 255 = 254.99999999999997 in float64: the clip itself truncates to 254, as numpy does
    assert (49.0 * (1 / 49.0)) * 255 < 255 and st.diff_u8_ref(np.array([60.0], np.float32), 49.0, 1 / 49.0).tolist() == [254]
    assert d[0] == 0                                           # the input is left as it was


def test_boundary_diffs():
    # mean_max = 255, factor = 1 / 255: d = k gives exactly k for every k of the list
    v, names = st.boundary_diffs(255.0, 1 / 255.0)
    assert names == ["1", "1-", "50", "50-", "51", "51-", "254", "254-", "255", "255-",
                     "mean_max", "mean_max+", "inf", "0", "-0", "subnormal"]
    assert v.dtype == np.float32
    for k in (1, 50, 51, 254, 255):
        assert (k * (1 / 255.0)) * 255 == k
        d, below = v[names.index(str(k))], v[names.index(f"{k}-")]
        assert d == k and below == np.nextafter(np.float32(k), np.float32(0))
    assert st.diff_u8_ref(v, 255.0, 1 / 255.0).tolist() == [1, 0, 50, 49, 51, 50, 254, 253, 255, 254, 255, 255, 255, 0, 0, 0]
    assert v[10] == 255 and v[11] == np.nextafter(np.float32(255), np.float32(np.inf)) and np.isinf(v[12])
    assert v[13] == 0 and not np.signbit(v[13]) and v[14] == 0 and np.signbit(v[14]) and v[15] == np.float32(1e-45)
    # any other normalisation: each pair straddles its boundary, whatever the float64 products round to
    for mean_max in (0.7431, 1.9, 3e-3, 49.0):
        factor = 1 / mean_max
        v, names = st.boundary_diffs(mean_max, factor)
        u8 = st.diff_u8_ref(v, mean_max, factor)
        top = int((mean_max * factor) * 255)
        for k in (1, 50, 51, 254, 255):
            i = names.index(str(k))
            assert v[i + 1] == np.nextafter(v[i], np.float32(0))
            if k <= top:
                assert (u8[i], u8[i + 1]) == (k, k - 1), (mean_max, k)
            else:
                assert u8[i] == top and v[i] <= mean_max < np.nextafter(v[i], np.float32(np.inf))
        assert u8[names.index("mean_max+")] == u8[names.index("inf")] == top
    v, names = st.boundary_diffs(0.0, 0.0)
    assert len(v) == 16 and (st.diff_u8_ref(v, 0.0, 0.0) == 0).all()


def test_counts_ref_nonzero_is_set():
    mask = np.array([[[0, 1], [2, 255]], [[0, 0], [0, 0]], [[7, 7], [7, 7]]], np.uint8)
    gt = np.array([[[128, 0], [1, 0]], [[1, 0], [0, 3]], [[0, 9], [0, 0]]], np.uint8)
    assert st.counts_ref(mask, gt).tolist() == [[1, 1, 2], [0, 2, 0], [1, 0, 3]]
    assert st.counts_ref(mask, gt).dtype == np.int64
    assert st.counts_ref(mask != 0, gt != 0).tolist() == [[1, 1, 2], [0, 2, 0], [1, 0, 3]]
