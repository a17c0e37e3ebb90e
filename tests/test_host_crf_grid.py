"""The host side of the CRF grid search (critic_vae_amd.segment: grid_plan, rank_rows, crf_search's skip, the -search CLI),
without a GPU, and the qualification of the variant list of tests/crf_grid_tools.py with segment_tools.crf_f32 on the CPU.

Qualification as measured on frames 0 / 1 (mid-range: share of pixels with Q(1) in (0.05, 0.95) in the float64 reference):

    variant (thr, p_floor, w1, w2)   mid-range     label 1       float32 restatement
    (-1, 1e-5, 6, 4)                 0.98 / 0.56   0.67 / 0.49   5.8e-7 / 3.7e-6
    (-1, 1e-5, 0, 4)                 1.00 / 1.00   0.48 / 0.45   1.4e-7 / 1.1e-7
    (-1, 1e-5, 6, 0)                 0.99 / 0.56   0.65 / 0.51   5.6e-7 / 3.7e-6
    (-1, 1e-5, 0, 0)                 1.00 / 1.00   0.50 / 0.50   6.0e-8 / 6.0e-8
    (-1, 1e-5, 3, 2)                 1.00 / 1.00   0.53 / 0.49   2.7e-7 / 8.5e-7
    (-1, 0.5, 6, 4)                  1.00 / 0.79   0.68 / 0.49   4.6e-7 / 1.9e-6
    (-1, 1e-30, 6, 4)                0.98 / 0.56   0.67 / 0.49   5.8e-7 / 3.7e-6
    (0, 0.3, 0.6, 0.4)               1.00 / 1.00   1.00 / 1.00   1.3e-7 / 1.7e-7   (input mask all set)
    (127, 0.3, 0.6, 0.4)             1.00 / 1.00   0.50 / 0.50   8.3e-8 / 1.4e-7
    (254 | 255, 0.3, 0.6, 0.4)       1.00 / 1.00   0.00 / 0.00   7.3e-8 / 1.2e-7   (input mask all clear)

The thresholded variants were first drafted with the floor and weights of wideB, (127, 1e-5, 6, 4): no pixel mid-range (a 0/1
input under that floor is decided by its unary alone), so they were replaced by the floor 0.3 and weights 0.6 / 0.4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crf_grid_tools as gt_tools  # noqa: E402
import segment_tools as st  # noqa: E402
from crf_ref import crf_ref  # noqa: E402

from critic_vae_amd import segment as seg  # noqa: E402


# ---- the grid as calls ----
def test_grid_plan_groups_by_kernel():
    rows, calls = seg.grid_plan(thresholds=(10, 50), w1=(22, 5), alpha=(12, 30), beta=(3.1,), w2=(8, 2), gamma=(1.8, 3.0),
                                it=(10, 5), p_floor=(1e-5, 1e-3))
    assert len(rows) == 2 * 2 * 2 * 1 * 2 * 2 * 2 * 2
    kernels = [c[0] for c in calls]
    assert kernels == [(12.0, 3.1, 1.8), (12.0, 3.1, 3.0), (30.0, 3.1, 1.8), (30.0, 3.1, 3.0)]         # order of first use
    for kern, variants, its in calls:
        assert its == [5, 10]                                             # every `it` is a snapshot, ascending
        assert len(variants) == 2 * 2 * 2 * 2 and len(set(variants)) == len(variants)
        assert set(variants) == {(t, pf, a, d) for t in (10, 50) for pf in (1e-5, 1e-3) for a in (22.0, 5.0) for d in (8.0, 2.0)}
    # grid order: thr, p_floor, then the reference's nesting w1, alpha, beta, w2, gamma, it
    assert rows[0][:3] == (10, (22, 12, 3.1, 8, 1.8, 10), 1e-5) and rows[1][:3] == (10, (22, 12, 3.1, 8, 1.8, 5), 1e-5)
    assert rows[2][1] == (22, 12, 3.1, 8, 3.0, 10) and rows[4][1] == (22, 12, 3.1, 2, 1.8, 10) and rows[8][1] == (22, 30, 3.1, 8, 1.8, 10)
    assert rows[16][1][0] == 5 and rows[32][2] == 1e-3 and rows[64][0] == 50
    seen = set()
    for t, params, pf, ci, vi, si in rows:
        w1, alpha, beta, w2, gamma, it = params
        kern, variants, its = calls[ci]
        assert kern == (alpha, beta, gamma) and variants[vi] == (t, pf, w1, w2) and its[si] == it
        seen.add((t, params, pf))
    assert len(seen) == len(rows)


def test_grid_plan_defaults_are_the_reference_and_one_call():
    rows, calls = seg.grid_plan()
    assert len(calls) == 1 and calls[0][0] == (12.0, 3.1, 1.8) and calls[0][2] == [10]
    assert calls[0][1] == [(t, seg.P_FLOOR, 22.0, 8.0) for t in seg.SWEEP]
    assert [r[0] for r in rows] == list(seg.SWEEP) and all(r[1] == seg.CRF_REF for r in rows)
    _, calls = seg.grid_plan(thresholds=(50,), w1=(22, 22), it=(10, 10))           # repeats share a variant and a snapshot
    assert calls[0][1] == [(50, seg.P_FLOOR, 22.0, 8.0)] and calls[0][2] == [10]


# ---- the order of the result ----
def _row(name, tp, fn, fp):
    return {"name": name, "counts": (tp, fn, fp), "crf_iou": seg.iou_from_counts(tp, fn, fp)}


def test_rank_rows_best_first_ties_by_unrounded_ratio_then_grid_order():
    rows = [_row("a", 500, 500, 0),             # 0.5
            _row("b", 5004, 4996, 0),           # 0.5004 -> 0.5: above a by the unrounded ratio
            _row("c", 900, 100, 0),             # 0.9
            _row("d", 1, 1, 0),                 # 0.5 exactly: ties with a, grid order keeps a first
            _row("e", 0, 0, 0),                 # empty union: 1
            _row("f", 5004, 4996, 0)]           # ties with b in both: grid order
    assert [r["crf_iou"] for r in rows] == [0.5, 0.5, 0.9, 0.5, 1, 0.5]
    assert [r["name"] for r in seg.rank_rows(rows)] == ["e", "c", "b", "f", "a", "d"]
    assert [r["name"] for r in rows] == list("abcdef")                    # the input list is left as it was


def test_crf_search_skip_slices_every_input(monkeypatch):
    """crf_search(skip=n) hands [::n] of the frames, maps, maxima and ground truth on, as crf() does; checked without a GPU
    by standing in for the three device steps."""
    import torch
    seen = {}
    monkeypatch.setattr(seg, "_cuda", lambda a, dtype: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dtype))

    def normalize(diff, maxv, t, gt=None, hist=None, **kw):
        seen["norm"] = (diff.clone(), maxv.clone(), gt.clone())
        return torch.zeros(diff.shape, dtype=torch.uint8), None, None, 1.0

    def grid(frames, gt, kern, vs, its, diff_u8=None, **kw):
        seen.setdefault("grid", []).append((frames.clone(), gt.clone()))
        return torch.ones(len(its), len(vs), frames.shape[0], 3, dtype=torch.int64)

    class H:
        def crf_grid_scratch_bytes(self, B, K):
            return 1 << 20

    monkeypatch.setattr(seg, "_normalize", normalize)
    monkeypatch.setattr(seg, "crf_grid", grid)
    monkeypatch.setattr(seg, "_handle", lambda w: H())
    B = 7
    frames = np.arange(B * 4 * 4 * 3, dtype=np.uint8).reshape(B, 4, 4, 3)
    maps = np.arange(B * 16, dtype=np.float32).reshape(B, 4, 4)
    maxv = np.arange(B, dtype=np.float32)
    gt = (np.arange(B * 16).reshape(B, 4, 4) % 3 == 0)
    rows = seg.crf_search(frames, maps, maxv, gt, thresholds=(10, 20), skip=3, chunk=2)
    assert np.array_equal(seen["norm"][0].numpy(), maps[::3]) and np.array_equal(seen["norm"][1].numpy(), maxv[::3])
    assert np.array_equal(seen["norm"][2].numpy(), gt[::3].astype(np.uint8))
    assert [f.shape[0] for f, _ in seen["grid"]] == [2, 1]               # 3 frames in chunks of 2
    assert np.array_equal(np.concatenate([f.numpy() for f, _ in seen["grid"]]), frames[::3])
    assert np.array_equal(np.concatenate([g.numpy() for _, g in seen["grid"]]), gt[::3].astype(np.uint8))
    assert [r["counts"] for r in rows] == [(3, 3, 3)] * 2                # summed over the frames that were evaluated
    with pytest.raises(ValueError):
        seg.crf_search(frames, maps, maxv, gt, skip=0)


# ---- the CLI ----
def test_cli_defaults_leave_the_reference_values():
    a = seg.parse_args(["-video"])
    assert (a.thr, a.crf, a.p_floor) == (seg.THRESHOLD, seg.CRF_REF, seg.P_FLOOR) and not a.search
    assert (a.skip, a.top) == (1, 10)
    assert a.grid == {"thresholds": seg.SWEEP, "w1": (22.0,), "alpha": (12.0,), "beta": (3.1,), "w2": (8.0,), "gamma": (1.8,),
                      "it": (10,), "p_floor": (seg.P_FLOOR,)}
    # what main() passes on are eval_maps' own defaults
    import inspect
    d = {k: p.default for k, p in inspect.signature(seg.eval_maps).parameters.items()}
    assert (d["t"], d["crf_params"], d["p_floor"]) == (a.thr, a.crf, a.p_floor)
    d = {k: p.default for k, p in inspect.signature(seg.sweep_maps).parameters.items()}
    assert (d["crf_params"], d["p_floor"]) == (a.crf, a.p_floor)


def test_cli_flags_parse():
    a = seg.parse_args(["-video", "--thr", "70", "--crf", "5,6,20,3,3.5,4", "--p-floor", "1e-3"])
    assert (a.thr, a.crf, a.p_floor) == (70, (5.0, 6.0, 20.0, 3.0, 3.5, 4), 1e-3) and isinstance(a.crf[5], int)
    a = seg.parse_args(["-video", "-thresh", "--crf", "5,6,20,3,3.5,4"])
    assert a.thresh and a.crf[0] == 5.0
    a = seg.parse_args(["-video", "-search", "--grid-thr", "40,50", "--grid-w1", "10,22", "--grid-w2", "4,8", "--grid-it", "5,10",
                        "--grid-alpha", "12,24", "--grid-beta", "3.1", "--grid-gamma", "1.8", "--grid-p-floor", "1e-5,1e-3",
                        "--skip", "4", "--top", "3", "--mask-source", "critic-ig"])
    assert a.search and (a.skip, a.top) == (4, 3)
    assert a.grid == {"thresholds": (40, 50), "w1": (10.0, 22.0), "alpha": (12.0, 24.0), "beta": (3.1,), "w2": (4.0, 8.0),
                      "gamma": (1.8,), "it": (5, 10), "p_floor": (1e-5, 1e-3)}
    rows, calls = seg.grid_plan(**a.grid)
    assert len(calls) == 2 and len(rows) == 2 * 2 * 2 * 2 * 2 * 2
    assert seg.parse_args(["-video", "-search", "--second"]).second


@pytest.mark.parametrize("argv", [
    ["-video", "-search", "--out", "d"],
    ["-video", "-search", "-thresh"],
    ["-video", "-search", "--thr", "60"],
    ["-video", "-search", "--crf", "5,6,20,3,3.5,4"],
    ["-video", "-search", "--p-floor", "1e-3"],
    ["-video", "-search", "--skip", "0"],
    ["-video", "-search", "--top", "0"],
    ["-video", "-search", "--grid-thr", "a,b"],
    ["-video", "-search", "--grid-it", "2.5"],
    ["-video", "-thresh", "--thr", "60"],
    ["-video", "--thr", "256"],
    ["-video", "--thr", "-1"],
    ["-video", "--crf", "5,6,20,3,3.5"],
    ["-video", "--crf", "5,6,20,3,3.5,4.5"],
    ["-search"],
])
def test_cli_refusals(argv):
    with pytest.raises(SystemExit):
        seg.parse_args(argv)


def test_print_search_prints_the_top_rows(capsys):
    rows = [{"thr": t, "params": seg.CRF_REF, "p_floor": seg.P_FLOOR, "thr_iou": 0.1, "crf_iou": 0.2, "counts": (1, 2, 3)} for t in (50, 60, 70)]
    seg.print_search(rows, 2)
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 3 and "3 candidates" in out[0]
    assert out[1] == "thr=50, w1=22, alpha=12, beta=3.1, w2=8, gamma=1.8, it=10, p_floor=1e-05, thr_iou=0.1, crf_iou=0.2"


# ---- the variants of the GPU test ----
def test_variant_list():
    assert len(gt_tools.BASE_VARIANTS) == 11 and gt_tools.BASE_VARIANTS[0] == (-1, st.CASE_P_FLOOR, st.WIDE_B[0], st.WIDE_B[3])
    assert gt_tools.KERNEL == (48, 40, 24) and gt_tools.IT == 3
    assert [v[0] for v in gt_tools.BASE_VARIANTS[7:]] == [0, 127, 254, 255]
    assert gt_tools.variants(17)[11:] == list(gt_tools.BASE_VARIANTS[:6])
    fr, pr = st.case_frames(64)
    u8 = gt_tools.diff_u8_of(pr)
    assert u8.dtype == np.uint8 and (u8[0].min(), u8[0].max()) == (12, 242) and (u8[2] == 255).all()
    assert np.array_equal(gt_tools.variant_prob((127, 0, 0, 0), pr, u8), (u8 > 127).astype(np.float32))
    assert gt_tools.variant_prob((-1, 0, 0, 0), pr, u8) is not None and gt_tools.variant_params((0, 0.3, 0.6, 0.4)) == (0.6, 48, 40, 0.4, 24, 3)


@pytest.mark.parametrize("variant", gt_tools.BASE_VARIANTS, ids=lambda v: "thr%d_pf%g_w%g_%g" % v)
def test_variant_is_non_degenerate_and_resolved_by_float32(variant):
    fr, pr = st.case_frames(64)
    u8 = gt_tools.diff_u8_of(pr)
    params = gt_tools.variant_params(variant)
    for i in (0, 1):
        prob = gt_tools.variant_prob(variant, pr[i], u8[i])
        lab, q = crf_ref(fr[i], prob, params, variant[1])
        l32, q32 = st.crf_f32(fr[i], prob, params, variant[1])
        err, bad = st.crf_bar(l32, q32, lab, q)
        mid = ((q > 0.05) & (q < 0.95)).mean()
        print(f"{variant} frame {i}: mid-range {mid:.3f}, label 1 {lab.mean():.3f}, input set {(prob > 0.5).mean():.3f}, float32 {err:.2e}")
        assert mid > 0, (variant, i)
        both_in = 0 < (prob > 0.5).mean() < 1
        assert both_in == (variant[0] not in gt_tools.SATURATING), (variant, i)
        assert (0 < lab.mean() < 1) == both_in, (variant, i, lab.mean())
        assert err <= st.BAR / 10 and bad == 0, (variant, i, err, bad)
