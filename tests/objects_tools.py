"""Pattern generators and deliberately wrong references ("mutants") of the objects-from-masks tests (numpy, no GPU).

patterns(W) returns {name: (W,W) bool}: the shapes at which a labelling, a hole fill or a filter can go wrong — one-pixel paths
along which the minimum index has to travel the whole length forwards and backwards, holes that are open under one connectivity
and closed under the other, equal areas for the tie rule, areas on both sides of the area filter, far more objects than table
rows, random masks around the percolation threshold.  FILTER_MIN_AREA is the area the "filter on" configuration uses; the
min-area blobs are cut for it.
"""
import numpy as np

from critic_vae_amd.objects import ObjectFilter, _label, fill_holes_host, objects_host

FILTER_MIN_AREA = 4
BERNOULLI = (0.3, 0.5, 0.593, 0.7)


def serpentine(W):
    """A one-pixel path: every other row full, joined at alternating ends."""
    m = np.zeros((W, W), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, W - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(W):
    """A one-pixel rectangular spiral from the top-left corner inwards, one clear pixel between its turns."""
    m = np.zeros((W, W), bool)
    x0, y0, x1, y1 = 0, 0, W - 1, W - 1
    m[0, :] = True
    while True:
        if y1 - y0 < 2:
            break
        m[y0:y1 + 1, x1] = True              # down the right side
        if x1 - x0 < 2:
            break
        m[y1, x0:x1 + 1] = True              # along the bottom
        y0 += 2
        if y1 - y0 < 0:
            break
        m[y0:y1 + 1, x0] = True              # up the left side
        x1 -= 2
        if x1 - x0 < 1:
            break
        m[y0, x0:x1 + 1] = True              # along the next top
        x0 += 2
        y1 -= 2
    return m


def ring(W, y0, x0, y1, x1):
    m = np.zeros((W, W), bool)
    m[y0:y1 + 1, x0:x1 + 1] = True
    m[y0 + 1:y1, x0 + 1:x1] = False
    return m


def patterns(W):
    rng = np.random.default_rng(1000 + W)
    P = {}
    P["empty"] = np.zeros((W, W), bool)
    P["full"] = np.ones((W, W), bool)
    c = np.zeros((W, W), bool)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True
    P["corners"] = c
    yy, xx = np.mgrid[0:W, 0:W]
    P["checker"] = (yy + xx) % 2 == 0
    P["diagonal"] = yy == xx
    s = serpentine(W)
    P["serpentine"], P["serpentine_lr"], P["serpentine_ud"], P["serpentine_t"] = s, s[:, ::-1].copy(), s[::-1].copy(), s.T.copy()
    sp = spiral(W)
    P["spiral"], P["spiral_180"] = sp, sp[::-1, ::-1].copy()
    u = np.zeros((W, W), bool)
    u[4:W - 4, 5] = u[4:W - 4, W - 6] = True
    u[W - 5, 5:W - 5] = True
    P["u"] = u
    P["ring"] = ring(W, 8, 8, W - 9, W - 9)
    P["ring_in_ring"] = ring(W, 4, 4, W - 5, W - 5) | ring(W, 12, 12, W - 13, W - 13) | (ring(W, 20, 20, 30, 30))
    g = ring(W, 10, 10, 30, 30)                  # one corner pixel of a ring removed: the hole meets the outside, and through it the
    g[10, 10] = False                            # border, across a diagonal only: open for an 8-connected background, closed for a 4-connected one
    P["diag_gap"] = g
    P["ring_at_border"] = ring(W, 0, 0, 20, 20) | ring(W, W - 15, 30, W - 1, 50)
    b = np.zeros((W, W), bool)                   # four blobs of 12 pixels, none first in raster order by accident of shape
    b[40:43, 30:34] = b[10:14, 50:53] = b[10:12, 5:11] = b[50:56, 8:10] = True
    b[30:35, 30:35] = True                       # and one larger
    P["equal_blobs"] = b
    a = np.zeros((W, W), bool)
    a[5, 5:5 + FILTER_MIN_AREA] = True           # exactly min_area
    a[9, 5:5 + FILTER_MIN_AREA - 1] = True       # min_area - 1
    a[20:22, 20:22] = True                       # min_area as a square
    a[30, 30] = a[31, 31] = a[32, 32] = a[33, 33] = True      # min_area under 8, four singles under 4
    P["min_area"] = a
    for p in BERNOULLI:
        P[f"bernoulli_{p}"] = rng.random((W, W)) < p
    return P


def filters():
    """(name, kwargs) of the two configurations every pattern runs under, per connectivity."""
    return (("off", dict()), ("on", dict(fill_holes=True, min_area=FILTER_MIN_AREA, keep_largest=3)))


# ---- mutants: objects_host with one plausible mistake ----
def mutant(kind, mask, filt, values=None):
    """objects_host(mask (B,W,W), filt, values) with one mistake:
        "swap_conn"       4 and 8 swapped
        "same_conn_holes" holes under the set pixels' connectivity instead of the complementary one
        "filter_first"    the area filter before the hole fill
        "tie_later"       keep_largest ties to the later component
        "exclusive_box"   x1, y1 one past the last pixel
        "by_area"         final labels by descending area instead of raster order"""
    mask = np.asarray(mask) != 0
    if kind == "swap_conn":
        return objects_host(mask, filt._replace(connectivity=12 - filt.connectivity), values)
    if kind == "same_conn_holes":
        if not filt.fill_holes:
            return objects_host(mask, filt, values)
        filled = np.stack([fill_holes_host(m, 12 - filt.connectivity) for m in mask])
        r = objects_host(filled, filt._replace(fill_holes=False), values)
        r["info"][:, 2] = filled.sum((1, 2)) - mask.sum((1, 2))
        return r
    if kind == "filter_first":
        pre = objects_host(mask, filt._replace(fill_holes=False, keep_largest=0), values)["mask"] != 0
        r = objects_host(pre, filt._replace(min_area=1), values)
        return r
    if kind == "tie_later":
        r = objects_host(mask[:, ::-1, ::-1], filt, None if values is None else np.asarray(values)[:, ::-1, ::-1])
        keep = r["mask"][:, ::-1, ::-1] != 0                      # the survivors when ties go to the LATER component
        return objects_host(mask & keep, filt._replace(fill_holes=False, min_area=1, keep_largest=0), values)
    if kind == "exclusive_box":
        r = objects_host(mask, filt, values)
        nz = r["table"][:, :, 0] > 0
        r["table"][:, :, 3][nz] += 1
        r["table"][:, :, 4][nz] += 1
        return r
    if kind == "by_area":
        r = objects_host(mask, filt, values)
        for f in range(mask.shape[0]):
            lab = r["labels"][f].astype(np.int64)
            n = int(lab.max())
            area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            order = sorted(range(n), key=lambda c: (-int(area[c]), c))
            new = np.zeros(n + 1, np.int64)
            new[np.array(order, np.int64) + 1] = np.arange(1, n + 1)
            r["labels"][f] = new[lab]
        return r
    raise ValueError(kind)


def same(a, b, passes=False):
    """Whole-array equality of two objects results (the passes column of info aside)."""
    keys = ("mask", "labels", "table")
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys if k in a and k in b) and \
        np.array_equal(np.asarray(a["info"])[:, :3], np.asarray(b["info"])[:, :3])


__all__ = ["patterns", "filters", "mutant", "same", "ObjectFilter", "_label", "FILTER_MIN_AREA", "BERNOULLI"]
