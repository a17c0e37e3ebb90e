"""Objects from masks: connected components, hole fill, area filter, per-object tables and panoptic quality.

The device side is cvae_mask_objects / cvae_object_overlap (include/cvae.h, csrc/components.hip): one launch for a whole set of
(B,W,W) masks, one workgroup per frame.  `mask_objects` and `object_overlap` call them; `match` and `panoptic` turn the tables
and the overlap matrix into object-level precision, recall and PQ = SQ * RQ on the host from one read; `objects_host` is the
numpy statement of what the device computes (a plain breadth-first labelling, no scipy), which the tests compare by equality.

Per frame, in this order: hole fill (clear regions not connected to the frame border, under the COMPLEMENTARY connectivity),
labelling, min-area filter, keep-largest (ties to the component whose first pixel comes earlier in raster order), relabelling
1..kept in raster order of each component's first pixel — scipy.ndimage.label's order.
"""
from collections import namedtuple

import numpy as np
import torch

from .lib import OBJECTS_MAX, ObjectParams

INFO_FOUND, INFO_KEPT, INFO_FILLED, INFO_PASSES = 0, 1, 2, 3
TABLE_COLS = ("area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "sum_value")


class ObjectFilter(namedtuple("ObjectFilter", "connectivity fill_holes min_area keep_largest max_objects")):
    """The parameters of cvae_mask_objects, range-checked: connectivity 4 or 8 (of the set pixels), fill_holes, min_area >= 1,
    keep_largest 0 (all) or k >= 1, max_objects 1..64 (table rows)."""
    __slots__ = ()

    def __new__(cls, connectivity=8, fill_holes=False, min_area=1, keep_largest=0, max_objects=32):
        if connectivity not in (4, 8):
            raise ValueError(f"connectivity {connectivity!r}: 4 or 8")
        for name, v in (("min_area", min_area), ("keep_largest", keep_largest), ("max_objects", max_objects)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{name} {v!r}: an integer")
        if not 1 <= min_area < 2 ** 31:
            raise ValueError(f"min_area {min_area}: at least 1")
        if not 0 <= keep_largest < 2 ** 31:
            raise ValueError(f"keep_largest {keep_largest}: 0 (all) or the number of objects to keep")
        if not 1 <= max_objects <= OBJECTS_MAX:
            raise ValueError(f"max_objects {max_objects}: 1..{OBJECTS_MAX}")
        return super().__new__(cls, int(connectivity), bool(fill_holes), int(min_area), int(keep_largest), int(max_objects))

    def params(self):
        return ObjectParams(self.connectivity, int(self.fill_holes), self.min_area, self.keep_largest, self.max_objects)


def _handle(width):
    from .segment import _handle as seg_handle
    return seg_handle(width)


def _cuda(a, dtype):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype).contiguous()


# ---- the device route ----
def mask_objects(mask, filt=None, values=None, labels=False):
    """cvae_mask_objects on a (B,W,W) mask (nonzero / True = set), W = 64 or 128.  Returns device tensors: "mask" (B,W,W) uint8
    0/1 after fill and filters, "info" (B,4) int32 (found, kept, filled, passes), "table" (B,M,8) int32 (TABLE_COLS; sum_value
    over `values` (B,W,W) uint8, 0 without), and with labels=True "labels" (B,W,W) uint16."""
    filt = ObjectFilter() if filt is None else filt
    m = _cuda(mask, torch.uint8)
    B, W = m.shape[0], m.shape[-1]
    assert m.shape == (B, W, W), tuple(m.shape)
    v = None if values is None else _cuda(values, torch.uint8)
    assert v is None or v.shape == m.shape, tuple(v.shape)
    out = {"mask": torch.empty_like(m), "info": torch.empty(B, 4, dtype=torch.int32, device=m.device),
           "table": torch.empty(B, filt.max_objects, 8, dtype=torch.int32, device=m.device)}
    if labels:
        out["labels"] = torch.empty(B, W, W, dtype=torch.uint16, device=m.device)
    _handle(W).mask_objects(B, m, filt.params(), out["info"], values=v, mask_out=out["mask"], labels=out.get("labels"),
                            table=out["table"])
    return out


def object_overlap(labels_a, labels_b, M):
    """cvae_object_overlap: (B,M,M) int32 on the device, [b,i,j] = pixels with labels_a == i + 1 and labels_b == j + 1."""
    a, b = _cuda(labels_a, torch.uint16), _cuda(labels_b, torch.uint16)
    B, W = a.shape[0], a.shape[-1]
    assert a.shape == (B, W, W) and b.shape == a.shape, (tuple(a.shape), tuple(b.shape))
    inter = torch.empty(B, int(M), int(M), dtype=torch.int32, device=a.device)
    _handle(W).object_overlap(B, a, b, M, inter)
    return inter


# ---- matching and panoptic quality, on the host ----
def _host(*arrays):
    """Host int64 arrays of tensors / arrays; device tensors come over in ONE read."""
    dev = [i for i, a in enumerate(arrays) if torch.is_tensor(a) and a.is_cuda]
    out = [None if torch.is_tensor(a) and a.is_cuda else np.asarray(a.numpy() if torch.is_tensor(a) else a).astype(np.int64) for a in arrays]
    if dev:
        flat = torch.cat([arrays[i].reshape(-1).to(torch.int64) for i in dev]).cpu().numpy()
        pos = 0
        for i in dev:
            n = arrays[i].numel()
            out[i] = flat[pos:pos + n].reshape(tuple(arrays[i].shape))
            pos += n
    return out


def match(table_a, kept_a, table_b, kept_b, inter):
    """Objects of a (the prediction) matched with objects of b (the ground truth): a pair matches when its IoU > 0.5, decided in
    integers as 3 * inter > area_a + area_b; such matches are unique, so there is no greedy step.  table_* (B,M,8), kept_* (B)
    the TRUE kept counts (info[:, 1]), inter (B,M,M).  Returns {"tp", "fp", "fn": (B,) int64 with fp = kept_a - tp and
    fn = kept_b - tp, "ious": a list of B float64 arrays (the matched IoUs in row order), "pairs": a list of B (n,2) int arrays,
    "truncated": (B,) bool, set where either count exceeds M (objects past M cannot match: they count as fp / fn)}."""
    ta, ka, tb, kb, it = _host(table_a, kept_a, table_b, kept_b, inter)
    B, M = ta.shape[0], ta.shape[1]
    ka, kb = ka.reshape(B), kb.reshape(B)
    assert tb.shape == ta.shape and it.shape == (B, M, M), (ta.shape, tb.shape, it.shape)
    tp = np.zeros(B, np.int64)
    ious, pairs = [], []
    for f in range(B):
        na, nb = min(int(ka[f]), M), min(int(kb[f]), M)
        aa, ab, x = ta[f, :na, 0], tb[f, :nb, 0], it[f, :na, :nb]
        hit = 3 * x > aa[:, None] + ab[None, :]
        i, j = np.nonzero(hit)
        tp[f] = len(i)
        ious.append(x[i, j] / (aa[i] + ab[j] - x[i, j]).astype(np.float64))
        pairs.append(np.stack([i, j], 1))
    return {"tp": tp, "fp": ka - tp, "fn": kb - tp, "ious": ious, "pairs": pairs, "truncated": (ka > M) | (kb > M)}


def panoptic(matches):
    """Set-wide panoptic quality of `match`'s result, the counts pooled over the frames: sq = the mean matched IoU, rq = tp /
    (tp + fp / 2 + fn / 2), pq = sq * rq, precision = tp / (tp + fp), recall = tp / (tp + fn), plus tp, fp, fn and
    truncated_frames.  With no objects on either side all five are 1, as iou_from_counts is for an empty union; a ratio whose
    denominator alone is empty (nothing predicted: precision; nothing to find: recall) is 1 too; sq without a match but with
    objects is 0."""
    tp, fp, fn = (int(np.sum(matches[k])) for k in ("tp", "fp", "fn"))
    allv = np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in matches["ious"]]) if matches["ious"] else np.zeros(0)
    if tp + fp + fn == 0:
        sq = rq = 1.0
    else:
        sq = float(allv.mean()) if tp else 0.0
        rq = tp / (tp + fp / 2 + fn / 2)
    return {"pq": sq * rq, "sq": sq, "rq": rq, "precision": tp / (tp + fp) if tp + fp else 1.0,
            "recall": tp / (tp + fn) if tp + fn else 1.0, "tp": tp, "fp": fp, "fn": fn,
            "truncated_frames": int(np.sum(matches["truncated"]))}


def centroids(table):
    """(…,M,2) float64 (sum_x / area, sum_y / area) of a table; NaN for an empty row."""
    t = table.cpu().numpy() if torch.is_tensor(table) else np.asarray(table)
    area = t[..., 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([t[..., 5] / area, t[..., 6] / area], -1)


# ---- the numpy statement ----
def _label(mask, connectivity):
    """(labels int32, n): the components of a 2-D boolean mask, numbered in raster order of their first pixel.  Breadth first."""
    H, W = mask.shape
    P = W + 2
    pad = np.zeros((H + 2, P), bool)
    pad[1:-1, 1:-1] = mask
    todo = pad.ravel().tolist()
    lab = [0] * len(todo)
    offs = (-P, -1, 1, P) + ((-P - 1, -P + 1, P - 1, P + 1) if connectivity == 8 else ())
    n = 0
    for s in np.flatnonzero(pad).tolist():
        if not todo[s]:
            continue
        n += 1
        todo[s] = False
        lab[s] = n
        queue, head = [s], 0
        while head < len(queue):
            p = queue[head]
            head += 1
            for o in offs:
                q = p + o
                if todo[q]:
                    todo[q] = False
                    lab[q] = n
                    queue.append(q)
    return np.array(lab, np.int32).reshape(H + 2, P)[1:-1, 1:-1], n


def fill_holes_host(mask, connectivity):
    """The mask with every clear region that does not reach the border set; clear pixels connect under the complement of
    `connectivity` (the set pixels')."""
    clear = ~mask
    lab, _ = _label(clear, 4 if connectivity == 8 else 8)
    edge = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    open_ = np.isin(lab, np.unique(edge[edge > 0]))
    return mask | (clear & ~open_)


def objects_host(mask, filt=None, values=None):
    """What cvae_mask_objects computes, in numpy: {"mask" (B,W,W) uint8, "labels" (B,W,W) uint16, "info" (B,4) int32 with the
    passes column 0, "table" (B,M,8) int32}.  Any frame size."""
    filt = ObjectFilter() if filt is None else filt
    m = (mask.cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)) != 0
    v = None if values is None else (values.cpu().numpy() if torch.is_tensor(values) else np.asarray(values)).astype(np.int64)
    B, H, W = m.shape
    M = filt.max_objects
    out = {"mask": np.zeros((B, H, W), np.uint8), "labels": np.zeros((B, H, W), np.uint16), "info": np.zeros((B, 4), np.int32),
           "table": np.zeros((B, M, 8), np.int32)}
    for f in range(B):
        cur = fill_holes_host(m[f], filt.connectivity) if filt.fill_holes else m[f]
        filled = int(cur.sum() - m[f].sum())
        lab, n = _label(cur, filt.connectivity)
        area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        keep = area >= filt.min_area
        if filt.keep_largest > 0 and keep.sum() > filt.keep_largest:
            order = sorted(np.flatnonzero(keep).tolist(), key=lambda c: (-int(area[c]), c))[:filt.keep_largest]
            keep = np.zeros(n, bool)
            keep[order] = True
        new = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)]).astype(np.int64)
        fin = new[lab]
        kept = int(keep.sum())
        out["mask"][f] = fin > 0
        out["labels"][f] = fin
        out["info"][f] = (n, kept, filled, 0)
        ys, xs = np.nonzero((fin > 0) & (fin <= M))
        r = fin[ys, xs] - 1
        t = np.zeros((M, 8), np.int64)
        t[:min(kept, M), 1:3] = max(H, W)
        np.add.at(t[:, 0], r, 1)
        np.minimum.at(t[:, 1], r, xs)
        np.minimum.at(t[:, 2], r, ys)
        np.maximum.at(t[:, 3], r, xs)
        np.maximum.at(t[:, 4], r, ys)
        np.add.at(t[:, 5], r, xs)
        np.add.at(t[:, 6], r, ys)
        if v is not None:
            np.add.at(t[:, 7], r, v[f][ys, xs])
        out["table"][f] = t
    return out


def overlap_host(labels_a, labels_b, M):
    """cvae_object_overlap in numpy: (B,M,M) int32."""
    a, b = np.asarray(labels_a).astype(np.int64), np.asarray(labels_b).astype(np.int64)
    B = a.shape[0]
    out = np.zeros((B, M, M), np.int32)
    for f in range(B):
        sel = (a[f] >= 1) & (a[f] <= M) & (b[f] >= 1) & (b[f] <= M)
        np.add.at(out[f], (a[f][sel] - 1, b[f][sel] - 1), 1)
    return out
