"""The data-side kernels of dataset.hip one by one on the MI355X, past their first loop trip:

(a) cvae_curate_select / cvae_curate_select_recon on walks of 63 .. 700 short trajectories (tests/dataset_ops_tools.py; what
    each case is, is proved on the CPU in tests/test_host_dataset_ops_tools.py): the cut lands in a chosen wave of 64 or round
    of 256 trajectories of curate_cut_kernel, so that the cross-wave prefix, the second scan over frames, the carry between
    rounds and the backward search across rounds run with data.  Every output array exactly as the plain restatement.
(b) the same calls entered with the running count at or past total_images, and with counts past 2^33.
(c) cvae_gather_frames_u8 with its three skip guards taken, (d) cvae_preprocess_u8_gather with indices outside [0, n),
(e) cvae_recon_zcat against numpy with rows outside [0, n_sel) — bit for bit, guard bands intact."""
import numpy as np
import pytest
import torch

import dataset_ops_tools as D
from critic_vae_amd.lib import Handle

pytestmark = pytest.mark.gpu
DEV = D.DEV
GUARD = 65536                         # bytes of guard band


@pytest.fixture(scope="module")
def handle():
    return Handle(64, 1)


@pytest.fixture(scope="module")
def handle256():
    return Handle(64, 256)


def _walk(h, trajs, collect, total, bounds, recon, running0=0):
    raw = []
    fn = D.device_select_recon if recon else D.device_select
    got = fn(h, trajs, collect, total, len(bounds) - 1, bounds=bounds, running0=running0, raw=raw)
    return got, raw


def _check_walk(h, trajs, collect, total, bounds, recon, what, running0=0):
    """One walk on the device against expected_chunks: every output of every call exactly, nothing written past the spans."""
    (rows, first, counts, running), raw = _walk(h, trajs, collect, total, bounds, recon, running0)
    want = D.expected_chunks(trajs, collect, total, bounds, recon, running0)
    assert len(raw) == len(want)
    for c, (got, exp) in enumerate(zip(raw, want)):
        w = f"{what} call {c}"
        assert got["span"].tolist() == exp["span"].tolist(), w
        assert got["running"] == exp["running"], w
        np.testing.assert_array_equal(got["first"], exp["first"], err_msg=w)
        np.testing.assert_array_equal(got["counts"], exp["counts"], err_msg=w)
        ne = int(exp["span"][1])
        keys = ("ent_frame", "ent_kind", "ent_sel") if recon else ("ent_frame",)
        for k in keys:
            np.testing.assert_array_equal(got[k][:ne], exp[k], err_msg=f"{w} {k}")
            assert (got[k][ne:] == D.FILL).all(), f"{w}: {k} written past span[1]"
        if recon:
            ns = int(exp["span"][2])
            np.testing.assert_array_equal(got["sel"][:ns], exp["sel"], err_msg=f"{w} sel")
            assert (got["sel"][ns:] == D.FILL).all(), f"{w}: sel written past span[2]"
            np.testing.assert_array_equal(got["sel_first"], exp["sel_first"], err_msg=f"{w} sel_first")
    # ... and the whole walk as the restatement states it
    sizes, ref_rows, ref_counts = D.host_select(trajs, collect, total - running0, recon)
    assert rows == ref_rows, what
    assert first == [running0 + s for s in sizes] + [-1] * (len(trajs) - len(sizes)), what
    np.testing.assert_array_equal(counts, ref_counts, err_msg=what)
    assert running == running0 + len(ref_rows), what
    return raw


# ---- (a) ----

@pytest.mark.parametrize("recon", [False, True], ids=["plain", "recon"])
@pytest.mark.parametrize("n_traj", D.N_TRAJ)
def test_curation_scan_past_one_wave_and_round(handle, n_traj, recon):
    trajs = D.family(n_traj)
    n = 0
    for collect in D.COLLECTS:
        cuts = D.named_cuts(n_traj, collect, recon)
        assert list(cuts) == D.CASES[n_traj]
        for name, total in cuts.items():
            for bounds in ([0, n_traj], D.chunk_bounds(n_traj)):
                _check_walk(handle, trajs, collect, total, bounds, recon, f"n_traj {n_traj} collect {collect} {name} ({total}) bounds {bounds}")
                n += 1
    assert n == 6 * len(D.CASES[n_traj])


# ---- (b) ----

@pytest.mark.parametrize("recon", [False, True], ids=["plain", "recon"])
def test_curation_entered_at_or_past_the_cut(handle, recon):
    """running >= total_images on entry: every first is -1, every count 0, span = (running, 0[, 0]), running unchanged and
    no selection array touched."""
    trajs = D.family(257)
    for r0, total in ((50, 50), (51, 50), (2 ** 33 + 40, 2 ** 33 + 40)):
        for bounds in ([0, 257], D.chunk_bounds(257)):
            raw = _check_walk(handle, trajs, 2, total, bounds, recon, f"running {r0} total {total} bounds {bounds}", running0=r0)
            for got in raw:
                assert (got["first"] == -1).all() and (got["counts"] == 0).all() and got["running"] == r0
                assert got["span"].tolist() == [r0, 0] + ([0] if recon else [])
                for k in (("ent_frame", "ent_kind", "ent_sel", "sel") if recon else ("ent_frame",)):
                    assert (got[k] == D.FILL).all(), k


@pytest.mark.parametrize("recon", [False, True], ids=["plain", "recon"])
def test_curation_counts_past_2_33(handle, recon):
    """running = 2^33 + 3, total_images = 2^33 + 40: the slots are 64-bit, sel stays chunk-relative."""
    r0, total = 2 ** 33 + 3, 2 ** 33 + 40
    for n_traj in (257, 513):
        trajs = D.family(n_traj)
        for bounds in ([0, n_traj], D.chunk_bounds(n_traj), [0, 3, 5, n_traj]):
            raw = _check_walk(handle, trajs, 2, total, bounds, recon, f"n_traj {n_traj} bounds {bounds} past 2^33", running0=r0)
            visited = np.concatenate([g["first"] for g in raw])
            visited = visited[visited >= 0]
            assert len(visited) > 3 and visited.min() == r0 and visited.max() < total
            assert max(g["running"] for g in raw) >= total
            for g in raw:
                ne = int(g["span"][1])
                assert g["span"][0] >= r0 and (g["ent_frame"][:ne] >= 0).all() and (g["ent_frame"][:ne] < 2 ** 31).all()


# ---- (c) cvae_gather_frames_u8 ----

def _banded(n_bytes, dtype, fill):
    """A buffer of n_bytes between two guard bands; returns (whole uint8 buffer, the middle as dtype)."""
    whole = torch.full((GUARD + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    mid = whole[GUARD:GUARD + n_bytes].view(dtype)
    assert fill.dtype == dtype and whole.data_ptr() % 16 == 0
    mid.copy_(fill.reshape(-1))
    return whole, mid


def _bands_intact(whole, n_bytes):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[GUARD + n_bytes:] == 0xA5).all())


@pytest.mark.parametrize("w", [64, 128])
def test_gather_frames_skip_guards(w):
    """9 source frames, capacity 12, span = (8, 6), max_count = 7: candidate 6 lies past span[1], candidates 4 and 5 would go
    to slots 12 and 13 past the capacity, candidate 1 has sel = -1 and candidate 3 sel = 9 = n_src.  With
    sel = [3, -1, 8, 9, 0, 5, 2] only slots 8 and 10 change — slot 11 belongs to the out-of-range candidate 3 and keeps its
    pattern like slot 9; with candidate 3 in range ([.., 7, ..]) exactly slots 8, 10 and 11 change.  Both are run."""
    rng = np.random.default_rng(w)
    n_src, cap, fb = 9, 12, w * w * 3
    src = torch.from_numpy(rng.integers(0, 256, size=(n_src, w, w, 3), dtype=np.uint8)).to(DEV)
    src_p = torch.from_numpy(rng.random((n_src, 1), dtype=np.float32)).to(DEV)
    pattern = torch.from_numpy(rng.integers(0, 256, size=(cap, w, w, 3), dtype=np.uint8)).to(DEV)
    pattern_p = torch.from_numpy(-1 - rng.random((cap, 1), dtype=np.float32)).to(DEV)
    h = Handle(w, 1)
    span = torch.tensor([8, 6], dtype=torch.int64, device=DEV)
    for sel, changed in (([3, -1, 8, 9, 0, 5, 2], {8: 3, 10: 8}), ([3, -1, 8, 7, 0, 5, 2], {8: 3, 10: 8, 11: 7})):
        whole, flat = _banded(cap * fb, torch.uint8, pattern)
        whole_p, flat_p = _banded(cap * 4, torch.float32, pattern_p)
        dst, dst_p = flat.view(cap, w, w, 3), flat_p.view(cap, 1)
        h.gather_frames_u8(src, src_p, torch.tensor(sel, dtype=torch.int64, device=DEV), 7, span, dst, dst_p)
        torch.cuda.synchronize()
        want, want_p = pattern.clone(), pattern_p.clone()
        for slot, s in changed.items():
            want[slot], want_p[slot] = src[s], src_p[s]
        assert torch.equal(dst, want), (w, sel, [i for i in range(cap) if not torch.equal(dst[i], want[i])])
        assert torch.equal(dst_p.view(torch.int32), want_p.view(torch.int32)), (w, sel)
        assert [i for i in range(cap) if not torch.equal(dst[i], pattern[i])] == sorted(changed), (w, sel)
        assert _bands_intact(whole, cap * fb) and _bands_intact(whole_p, cap * 4), (w, sel)


# ---- (d) cvae_preprocess_u8_gather ----

@pytest.mark.parametrize("w", [64, 128])
def test_preprocess_u8_gather_out_of_range(w):
    rng = np.random.default_rng(10 + w)
    n, B = 11, 5
    frames = torch.from_numpy(rng.integers(0, 256, size=(n, w, w, 3), dtype=np.uint8)).to(DEV)
    preds = torch.from_numpy(rng.random((n, 1), dtype=np.float32)).to(DEV)
    idx = [2, -1, n, 0, n - 1]
    h = Handle(w, 8)
    row = 3 * w * w * 4
    whole, x = _banded((B + 1) * row, torch.float32, torch.full(((B + 1) * 3 * w * w,), -3.0, device=DEV))
    whole_p, p = _banded((B + 1) * 4, torch.float32, torch.full((B + 1,), -3.0, device=DEV))
    x, p = x.view(B + 1, 3, w, w), p.view(B + 1, 1)
    h.preprocess_u8_gather(B, frames, preds, torch.tensor(idx, dtype=torch.int64, device=DEV), x, p)
    torch.cuda.synchronize()
    for b, i in enumerate(idx):
        if 0 <= i < n:
            ref = torch.empty(1, 3, w, w, device=DEV)
            h.preprocess_u8(1, frames[i:i + 1].contiguous(), ref)
            assert torch.equal(x[b].view(torch.int32), ref[0].view(torch.int32)), (w, b)
            assert torch.equal(p[b].view(torch.int32), preds[i].view(torch.int32)), (w, b)
        else:
            assert bool(torch.isnan(x[b]).all()) and bool(torch.isnan(p[b]).all()), (w, b)
    assert bool((x[B] == -3.0).all()) and bool((p[B] == -3.0).all()), "a row past the batch was written"
    assert _bands_intact(whole, (B + 1) * row) and _bands_intact(whole_p, (B + 1) * 4)


# ---- (e) cvae_recon_zcat ----

@pytest.mark.parametrize("n_entries", [1, 7, 8, 31, 32, 256])
def test_recon_zcat_against_numpy(handle256, n_entries):
    """33 floats per row: 7 / 8 and 31 / 32 rows end just inside / outside a 256-thread workgroup (231 | 264, 1023 | 1056)."""
    rng = np.random.default_rng(n_entries)
    n_sel = 40
    mu = (rng.random((n_sel, 32), dtype=np.float32) * 4 - 2).astype(np.float32)
    mu.view(np.uint32)[5, :4] = [0x7fc00001, 0xffffffff, 0x00000001, 0x80000000]          # a NaN payload, a denormal, -0: bit copies
    spred = rng.random(n_sel, dtype=np.float32)
    h = handle256
    d_mu, d_spred = torch.from_numpy(mu).to(DEV), torch.from_numpy(spred).to(DEV)
    layouts = [None]
    if n_entries == 1:
        layouts = [None, {0: -1}, {0: n_sel}]
    for bad in layouts:
        es = rng.integers(0, n_sel, size=n_entries).astype(np.int64)
        es[0] = 5
        kind = (np.arange(n_entries) % 2).astype(np.int32) if n_entries > 1 else np.zeros(1, np.int32)
        rng.shuffle(kind)
        if bad is None and n_entries > 1:
            bad = {2: -1, n_entries - 2: n_sel}
        for e, v in (bad or {}).items():
            es[e] = v
        n_bytes = n_entries * 33 * 4
        whole, z = _banded(n_bytes, torch.float32, torch.full((n_entries * 33,), -3.0, device=DEV))
        h.recon_zcat(n_entries, torch.from_numpy(es).to(DEV), torch.from_numpy(kind).to(DEV), d_mu, d_spred, z)
        torch.cuda.synchronize()
        got = z.cpu().numpy().reshape(n_entries, 33)
        want = np.empty((n_entries, 33), np.float32)
        ok = (es >= 0) & (es < n_sel)
        safe = np.where(ok, es, 0)
        want[:, :32] = mu[safe]
        want[:, 32] = np.where(kind == 0, spred[safe], np.float32(0.0))
        assert ok.sum() == n_entries - len(bad or {})
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (n_entries, bad)
        assert np.isnan(got[~ok]).all(), (n_entries, bad)
        assert _bands_intact(whole, n_bytes), (n_entries, bad)
    if n_entries > 1:
        assert (kind == 0).any() and (kind == 1).any()
