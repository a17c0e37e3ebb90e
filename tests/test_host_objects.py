"""Objects from masks without a device: objects_host (the numpy statement the GPU tests compare with) against scipy.ndimage on
every pattern, the ObjectFilter range checks, the arithmetic of match / panoptic on hand-made tables, the mutants — each
plausible mistake must change at least one output on the pattern set — and the command line."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_tools as OT  # noqa: E402

from critic_vae_amd import objects as ob  # noqa: E402
from critic_vae_amd import segment as seg  # noqa: E402
from critic_vae_amd.objects import ObjectFilter  # noqa: E402

WIDTHS = (64, 128)
M = 32


def _values(W):
    return np.random.default_rng(7).integers(0, 256, size=(W, W), dtype=np.uint8)


def scipy_objects(mask, filt, values):
    """One frame through scipy.ndimage: label / binary_fill_holes / sum / find_objects."""
    ndi = pytest.importorskip("scipy.ndimage")
    full, cross = np.ones((3, 3), bool), ndi.generate_binary_structure(2, 1)
    st, comp = (full, cross) if filt.connectivity == 8 else (cross, full)
    cur = ndi.binary_fill_holes(mask, structure=comp) if filt.fill_holes else mask
    lab, n = ndi.label(cur, structure=st)
    idx = np.arange(1, n + 1)
    area = np.asarray(ndi.sum(cur, lab, idx), np.int64).reshape(-1)
    keep = area >= filt.min_area
    if filt.keep_largest and keep.sum() > filt.keep_largest:
        order = np.lexsort((idx - 1, -area))                  # area descending, then label ascending
        order = [c for c in order if keep[c]][:filt.keep_largest]
        keep = np.zeros(n, bool)
        keep[order] = True
    new = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)])
    fin = new[lab]
    kept = int(keep.sum())
    table = np.zeros((filt.max_objects, 8), np.int64)
    yy, xx = np.mgrid[0:mask.shape[0], 0:mask.shape[1]]
    for i, sl in enumerate(ndi.find_objects(fin.astype(np.int32))[:filt.max_objects]):
        sel = fin == i + 1
        table[i] = (sel.sum(), sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1, ndi.sum(xx, fin, i + 1), ndi.sum(yy, fin, i + 1),
                    ndi.sum(values.astype(np.int64), fin, i + 1))
    return {"mask": (fin > 0).astype(np.uint8)[None], "labels": fin.astype(np.uint16)[None],
            "info": np.array([[n, kept, int(cur.sum() - mask.sum()), 0]], np.int32), "table": table.astype(np.int32)[None]}


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("conn", (4, 8))
def test_objects_host_equals_scipy_on_every_pattern(W, conn):
    pytest.importorskip("scipy.ndimage")
    vals = _values(W)
    for name, m in OT.patterns(W).items():
        for fname, kw in OT.filters():
            filt = ObjectFilter(connectivity=conn, max_objects=M, **kw)
            ours, ref = ob.objects_host(m[None], filt, vals[None]), scipy_objects(m, filt, vals)
            assert OT.same(ours, ref), (name, fname)
            assert ours["mask"].dtype == np.uint8 and ours["labels"].dtype == np.uint16 and ours["table"].dtype == np.int32


def test_pattern_set_has_what_it_names():
    for W in WIDTHS:
        P = OT.patterns(W)
        n4 = {k: ob._label(v, 4)[1] for k, v in P.items()}
        n8 = {k: ob._label(v, 8)[1] for k, v in P.items()}
        assert n4["checker"] == W * W // 2 and n8["checker"] == 1 and n4["diagonal"] == W and n8["diagonal"] == 1
        for k in ("serpentine", "serpentine_lr", "serpentine_ud", "serpentine_t", "spiral", "spiral_180", "u", "ring", "full"):
            assert n4[k] == n8[k] == 1, k
        assert n4["corners"] == 4 and n4["empty"] == 0
        # the diagonal gap: filled when the set pixels are 8-connected (background 4), open when they are 4-connected (background 8)
        g = P["diag_gap"]
        assert ob.fill_holes_host(g, 8).sum() > g.sum() and ob.fill_holes_host(g, 4).sum() == g.sum()
        # fill swallows the ring inside the ring's hole
        r = ob.objects_host(P["ring_in_ring"][None], ObjectFilter(fill_holes=True))
        assert r["info"][0, 0] == 1 and ob.objects_host(P["ring_in_ring"][None])["info"][0, 0] == 3
        # a ring that touches the border still has a hole
        assert ob.objects_host(P["ring_at_border"][None], ObjectFilter(fill_holes=True))["info"][0, 2] == 19 * 19 + 13 * 19
        full = ob.objects_host(P["full"][None], ObjectFilter(max_objects=1), np.full((1, W, W), 255, np.uint8))["table"][0, 0]
        assert full.tolist() == [W * W, 0, 0, W - 1, W - 1, W * W * (W - 1) // 2, W * W * (W - 1) // 2, 255 * W * W]


def test_filter_rules_by_hand():
    m = np.zeros((1, 64, 64), bool)
    m[0, 2, 2:6] = True          # area 4, first
    m[0, 10, 10:14] = True       # area 4, second
    m[0, 20, 20:25] = True       # area 5, third
    m[0, 30, 30:34] = True       # area 4, fourth
    m[0, 40, 40:43] = True       # area 3
    r = ob.objects_host(m, ObjectFilter(min_area=4, keep_largest=3, max_objects=4))
    assert r["info"][0].tolist() == [5, 3, 0, 0]
    assert r["table"][0, :, 0].tolist() == [4, 4, 5, 0]                         # the tie goes to the two EARLIER blobs of area 4
    assert r["table"][0, 2].tolist() == [5, 20, 20, 24, 20, 110, 100, 0]        # an inclusive box
    assert r["labels"][0, 30, 30] == 0 and r["labels"][0, 20, 20] == 3
    r = ob.objects_host(m, ObjectFilter(max_objects=2))
    assert r["info"][0, 1] == 5 and r["labels"].max() == 5 and (r["table"][0, :, 0] > 0).all()       # truncated table, complete labels


def test_object_filter_range_checks():
    f = ObjectFilter()
    assert tuple(f) == (8, False, 1, 0, 32)
    p = ObjectFilter(4, True, 7, 2, 64).params()
    assert (p.connectivity, p.fill_holes, p.min_area, p.keep_largest, p.max_objects) == (4, 1, 7, 2, 64)
    for kw in (dict(connectivity=6), dict(connectivity=0), dict(min_area=0), dict(min_area=-1), dict(keep_largest=-1), dict(max_objects=0),
               dict(max_objects=65), dict(min_area=1.5), dict(max_objects=True), dict(min_area=2 ** 31)):
        with pytest.raises(ValueError):
            ObjectFilter(**kw)


def _table(areas, M_):
    t = np.zeros((1, M_, 8), np.int32)
    t[0, :len(areas), 0] = areas
    return t


def test_match_and_panoptic_arithmetic():
    # a: areas 10, 6, 4; b: areas 10, 2.  (0,0) overlap 8: IoU 8/12 matches.  (1,1) overlap 2: IoU 2/6 does not.
    ta, tb = _table([10, 6, 4], 4), _table([10, 2], 4)
    inter = np.zeros((1, 4, 4), np.int32)
    inter[0, 0, 0], inter[0, 1, 1] = 8, 2
    m = ob.match(ta, [3], tb, [2], inter)
    assert (m["tp"][0], m["fp"][0], m["fn"][0]) == (1, 2, 1) and m["pairs"][0].tolist() == [[0, 0]] and not m["truncated"][0]
    assert m["ious"][0].tolist() == [8 / 12]
    p = ob.panoptic(m)
    assert p["sq"] == 8 / 12 and p["rq"] == 1 / 2.5 and p["pq"] == (8 / 12) * (1 / 2.5) and p["precision"] == 1 / 3 and p["recall"] == 1 / 2
    # IoU exactly 0.5 must NOT match: areas 6 and 6, overlap 4 -> 4 / 8
    inter[:] = 0
    inter[0, 0, 0] = 4
    m = ob.match(_table([6], 4), [1], _table([6], 4), [1], inter)
    assert m["tp"][0] == 0 and m["fp"][0] == 1 and m["fn"][0] == 1 and ob.panoptic(m)["pq"] == 0
    inter[0, 0, 0] = 5                                        # 5 / 7 does
    assert ob.match(_table([6], 4), [1], _table([6], 4), [1], inter)["tp"][0] == 1
    # empty on both sides: everything is 1
    m = ob.match(_table([], 4), [0], _table([], 4), [0], np.zeros((1, 4, 4), np.int32))
    p = ob.panoptic(m)
    assert (p["pq"], p["sq"], p["rq"], p["precision"], p["recall"], p["tp"], p["fp"], p["fn"], p["truncated_frames"]) == (1, 1, 1, 1, 1, 0, 0, 0, 0)
    # truncation: the true counts enter fp and fn, the flag is set
    inter = np.zeros((1, 2, 2), np.int32)
    inter[0, 0, 0] = 9
    m = ob.match(_table([10, 5], 2), [7], _table([9, 3], 2), [2], inter)
    assert (m["tp"][0], m["fp"][0], m["fn"][0], bool(m["truncated"][0])) == (1, 6, 1, True)
    assert ob.panoptic(m)["truncated_frames"] == 1
    # pooled over frames: counts add, sq is the mean over all matches
    two = {"tp": np.array([1, 1]), "fp": np.array([0, 2]), "fn": np.array([1, 0]), "ious": [np.array([0.6]), np.array([0.8])],
           "truncated": np.array([False, False])}
    p = ob.panoptic(two)
    assert abs(p["sq"] - 0.7) < 1e-15 and p["rq"] == 2 / 3.5 and p["precision"] == 0.5 and p["recall"] == 2 / 3
    assert np.array_equal(ob.centroids(np.array([[4, 0, 0, 0, 0, 10, 6, 0], [0] * 8]))[0], [2.5, 1.5])
    assert np.isnan(ob.centroids(np.array([[0] * 8]))).all()


MUTANTS = ("swap_conn", "same_conn_holes", "filter_first", "tie_later", "exclusive_box", "by_area")


@pytest.mark.parametrize("kind", MUTANTS)
def test_each_mutant_differs_somewhere_on_the_pattern_set(kind):
    W = 64
    vals = _values(W)[None]
    hits = []
    for name, m in OT.patterns(W).items():
        for conn in (4, 8):
            for fname, kw in OT.filters():
                filt = ObjectFilter(connectivity=conn, max_objects=M, **kw)
                if not OT.same(ob.objects_host(m[None], filt, vals), OT.mutant(kind, m[None], filt, vals)):
                    hits.append((name, conn, fname))
    assert hits, f"no pattern tells {kind} from the true reference"
    print(kind, len(hits), hits[:6])


def test_overlap_mutant_transposed():
    P = OT.patterns(64)
    a = ob.objects_host(P["equal_blobs"][None])["labels"]
    first = P["equal_blobs"].copy()
    first[0, 0] = True                                        # one more object in front: b's labels are a's plus one
    b = ob.objects_host(first[None])["labels"]
    o = ob.overlap_host(a, b, 8)
    assert o.sum() == (P["equal_blobs"]).sum() and not np.array_equal(o, o.transpose(0, 2, 1))
    assert all(o[0, i, i + 1] > 0 for i in range(5)) and np.trace(o[0]) == 0
    assert ob.overlap_host(a, b, 2).sum() < o.sum()          # labels past M are ignored


def test_cli_flags():
    a = seg.parse_args(["-video"])
    assert a.object_filter is None and not a.objects and a.objects_out is None
    a = seg.parse_args(["-video", "--objects", "--connectivity", "4", "--fill-holes", "--min-area", "4", "--keep-largest", "3",
                        "--max-objects", "16", "--objects-out", "o.npz", "--mask-source", "critic-ig"])
    assert a.object_filter == ObjectFilter(4, True, 4, 3, 16) and a.objects_out == "o.npz"
    assert seg.parse_args(["-video", "--objects", "--second"]).object_filter == ObjectFilter()
    for argv in (["-video", "--fill-holes"], ["-video", "--objects-out", "o.npz"], ["-video", "--min-area", "3"],
                 ["-video", "--objects", "-thresh"], ["-video", "--objects", "-search"], ["-video", "--objects", "--max-objects", "65"],
                 ["-video", "--objects", "--min-area", "0"], ["-video", "--objects", "--connectivity", "6"]):
        with pytest.raises(SystemExit):
            seg.parse_args(argv)


def test_header_bindings_and_build_list():
    from critic_vae_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cvae.h")).read()
    for name in ("cvae_mask_objects", "cvae_object_overlap"):
        assert name in lib.EXPORTS and name + "(" in hdr
        assert hasattr(lib.load(), name)
    assert "components.hip" in open(os.path.join(root, "critic-vae_amd", "csrc", "Makefile")).read()
    import ctypes as C
    assert C.sizeof(lib.ObjectParams) == 20 and lib.OBJECTS_MAX == 64 and "#define CVAE_OBJECTS_MAX 64" in hdr
