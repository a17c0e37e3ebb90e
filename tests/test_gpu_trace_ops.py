"""cvae_tensor_stats and cvae_trace_push on the GPU, against NumPy float64 on the same buffers.

Shapes come from cvae_tensor_stats_plan (chunk CH, items, grid), never from a number written here: tensors of 1, 3, 4, 5, CH - 1,
CH, CH + 1 and 2 CH + 7 elements that begin at every alignment mod 4, 32 tensors (the cap), and one tensor of (grid + 1) CH + 5
elements, so that a workgroup takes a second item.

Bounds.  Squares of fp32 values are exact in fp64 (24-bit significands give 48-bit products), so g2 and p2 differ from NumPy's
sum only by the order of n_t additions of non-negative terms: each addition rounds by at most 2^-53 relative, n_t of them by
less than n_t * 2^-52 of the (all-positive) sum.  u = step_size * (m / (sqrtf(v) / sqrt_bc2 + eps)): the sum of denom is of
two positive terms, so the roundings of sqrt, quotient and sum stay one relative rounding of denom (counted once: 2^-24), and
the quotient and the product add one each: three roundings, 3 * 2^-24 relative in u, 6 * 2^-24 in u^2, below 8 * 2^-24 with
the summation's own error (n_t * 2^-52, negligible beside it).  Counts and maxima are exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from critic_vae_amd import lib as cvlib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS = 5e-5, 0.9, 0.999, 1e-8
GAPS = (1, 0, 0, 3, 3, 0, 1)              # between the eight edge tensors: begins then fall on every alignment mod 4


def entry(obj, name):
    if not hasattr(obj, name):
        pytest.fail(f"the library binding has no {name}: the training trace (cvae_trace_push / cvae_tensor_stats) is missing")
    return getattr(obj, name)


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    h = cvlib.Handle(64, 4)
    entry(h, "tensor_stats"), entry(h, "trace_push")
    return h


@functools.lru_cache(maxsize=None)
def plan_of(ranges):
    return entry(cvlib, "tensor_stats_plan")(list(ranges))


@functools.lru_cache(maxsize=None)
def chunk():
    return plan_of(((0, 1),))["chunk"]


@functools.lru_cache(maxsize=None)
def table(kind):
    CH = chunk()
    if kind == "edge":
        lens, gaps = [1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7], GAPS + (0,)
    elif kind == "cap":
        lens, gaps = [1 + (7 * k) % 11 for k in range(32)], tuple((0, 1, 3)[k % 3] for k in range(32))
    else:                                   # "long": more items than workgroups
        grid = plan_of(((0, 1024 * CH),))["grid"]          # the launcher's cap on this device
        lens, gaps = [(grid + 1) * CH + 5], (0,)
    out, b = [], (2 if kind == "long" else 0)
    for n, gap in zip(lens, gaps):
        out.append((b, b + n))
        b += n + gap
    return tuple(out)


def test_the_tables_are_what_the_docstring_says():
    CH, edge = chunk(), table("edge")
    assert {b % 4 for b, _ in edge} == {0, 1, 2, 3}
    assert plan_of(edge)["items"] == 4 + 1 + 1 + 2 + 3
    assert len(table("cap")) == 32 == cvlib.TRACE_MAX_TENSORS
    p = plan_of(table("long"))
    assert p["items"] == p["grid"] + 2 and table("long")[0][0] % 4 == 2


@functools.lru_cache(maxsize=None)
def buffers(kind):
    """p, g, m, v as test_gpu_optim.py builds them, NaN and 1e30 in every element outside the tensors; never modified."""
    ranges = table(kind)
    n = (ranges[-1][1] + 3 + 3) // 4 * 4
    gen = torch.Generator().manual_seed(n % 9973 + 1)
    p, g, m, v = (torch.rand(n, generator=gen) for _ in range(4))
    host = [p, (g - 0.5) * 2e-2, (m - 0.5) * 1e-2, v * 1e-4]
    inside = torch.zeros(n, dtype=torch.bool)
    for b, e in ranges:
        inside[b:e] = True
    poison = torch.where(torch.arange(n) % 2 == 0, torch.tensor(float("nan")), torch.tensor(1e30))
    assert int((~inside).sum()) >= 3
    return tuple(torch.where(inside, t, poison).to(DEV) for t in host)


def scalars_at(step, lr=LR):
    """cvae_adam_step's host arithmetic: lr and the betas arrive as C floats and are widened to double."""
    lr, b1, b2 = (float(np.float32(t)) for t in (lr, B1, B2))
    return np.float32(lr / (1.0 - b1 ** step)), np.float32(np.sqrt(1.0 - b2 ** step))


def expected(bufs, ranges, gscale, step_size, sqrt_bc2, apply=True):
    """NumPy: fp32 for what the kernel computes in fp32, float64 sums."""
    p, g, m, v = (t.cpu().numpy() for t in bufs)
    out = []
    for b, e in ranges:
        pt, graw, mt, vt = p[b:e], g[b:e], m[b:e], v[b:e]
        with np.errstate(all="ignore"):
            gs = graw * np.float32(gscale)
            u = np.float32(step_size) * (mt / (np.sqrt(vt) / np.float32(sqrt_bc2) + np.float32(EPS))) if apply else np.zeros_like(mt)
            ga, pa = np.abs(gs), np.abs(pt)
            out.append(dict(g2=float(np.sum(gs.astype(np.float64) ** 2)), p2=float(np.sum(pt.astype(np.float64) ** 2)),
                            u2=float(np.sum(u.astype(np.float64) ** 2)),
                            gmax=np.float32(ga[~np.isnan(ga)].max(initial=0.0)), pmax=np.float32(pa[~np.isnan(pa)].max(initial=0.0)),
                            gnf=int((~np.isfinite(graw)).sum()), pnf=int((~np.isfinite(pt)).sum()), n=e - b))
    return out


def run_stats(H, bufs, ranges, step=3, grad_scale=0.5, guard=None, lr=LR):
    """One launch into fresh, pattern-filled output and scratch -> the raw bytes (n_tensors, 48) on the host."""
    p, g, m, v = bufs
    out = torch.full((len(ranges) * 48,), 0xA5, dtype=torch.uint8, device=DEV)
    scratch = torch.full((cvlib.tensor_stats_scratch_bytes(list(ranges)),), 0x5A, dtype=torch.uint8, device=DEV)     # may hold anything
    H.tensor_stats(p, g, m, v, list(ranges), step, out, scratch, lr=lr, b1=B1, b2=B2, eps=EPS, grad_scale=grad_scale, guard=guard)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(ranges), 48)


def records(raw):
    return [cvlib.TensorStat.from_buffer_copy(row.tobytes()) for row in raw]


def check(raw, want, step):
    for k, (r, w) in enumerate(zip(records(raw), want)):
        assert (r.g_nonfinite, r.p_nonfinite, r.step) == (w["gnf"], w["pnf"], step), k
        assert np.float32(r.gmax) == w["gmax"] and np.float32(r.pmax) == w["pmax"], k
        if w["gnf"] == 0:
            err = abs(r.g2 - w["g2"]) / w["g2"]
            print(f"tensor {k} n {w['n']}: g2 rel err {err:.3e} (bound {w['n'] * 2.0 ** -52:.3e})")
            assert err <= w["n"] * 2.0 ** -52, k
        else:
            assert not np.isfinite(r.g2) and not np.isfinite(w["g2"]), k
        if w["pnf"] == 0:
            err_p = abs(r.p2 - w["p2"]) / w["p2"]
            assert err_p <= w["n"] * 2.0 ** -52, (k, err_p)
        else:
            assert not np.isfinite(r.p2) and not np.isfinite(w["p2"]), k
        if w["u2"] == 0.0:
            assert r.u2 == 0.0, k
        else:
            err_u = abs(r.u2 - w["u2"]) / w["u2"]
            print(f"tensor {k}: u2 rel err {err_u:.3e} (bound {8 * 2.0 ** -24:.3e})")
            assert err_u <= 8 * 2.0 ** -24, k


@pytest.mark.parametrize("kind", ["edge", "cap", "long"])
def test_tensor_stats_against_float64(H, kind):
    ranges, bufs, step = table(kind), buffers(kind), 3
    raw = run_stats(H, bufs, ranges, step=step, grad_scale=0.5)
    ss, bc = scalars_at(step)
    check(raw, expected(bufs, ranges, 0.5, ss, bc), step)
    again = run_stats(H, bufs, ranges, step=step, grad_scale=0.5)
    assert np.array_equal(raw, again), "the same buffers must give the same bits"


def test_unaligned_buffers_take_the_scalar_path(H):
    """The four arrays one float past a 16-byte boundary: element by element, the same numbers."""
    ranges, step = table("edge"), 2
    shifted = tuple(torch.cat([t.new_zeros(1), t])[1:] for t in buffers("edge"))
    assert all(t.data_ptr() % 16 == 4 for t in shifted)
    raw = run_stats(H, shifted, ranges, step=step, grad_scale=1.0)
    ss, bc = scalars_at(step)
    check(raw, expected(shifted, ranges, 1.0, ss, bc), step)
    assert np.array_equal(raw, run_stats(H, shifted, ranges, step=step, grad_scale=1.0))


def test_nonfinite_elements_are_counted_where_they_are(H):
    ranges, step = table("edge"), 3
    clean = run_stats(H, buffers("edge"), ranges, step=step)
    p, g, m, v = (t.clone() for t in buffers("edge"))
    two, one = 7, 5                                        # the 2 CH + 7 tensor and the CH tensor
    g[ranges[two][0]] = float("nan")
    g[ranges[two][1] - 1] = float("nan")
    g[(ranges[one][0] + ranges[one][1]) // 2] = float("inf")
    p[ranges[3][0] + 2] = float("-inf")
    raw = run_stats(H, (p, g, m, v), ranges, step=step)
    rec = records(raw)
    assert rec[two].g_nonfinite == 2 and rec[one].g_nonfinite == 1 and rec[3].p_nonfinite == 1
    assert np.isnan(rec[two].g2) and np.isinf(rec[one].g2) and np.isinf(rec[one].gmax) and np.isinf(rec[3].pmax)
    assert rec[two].gmax == records(clean)[two].gmax or rec[two].gmax < records(clean)[two].gmax      # the NaNs did not enter
    for k in range(len(ranges)):
        if k not in (two, one, 3):
            assert np.array_equal(raw[k], clean[k]), k
    ss, bc = scalars_at(step)
    check(raw, expected((p, g, m, v), ranges, 0.5, ss, bc), step)


def test_with_a_guard_state(H):
    ranges, bufs = table("edge"), buffers("edge")
    p, g, m, v = (t.clone() for t in bufs)
    inside = torch.zeros(g.numel(), dtype=torch.bool, device=DEV)
    for b, e in ranges:
        inside[b:e] = True
    g = torch.where(inside, g, torch.zeros_like(g))        # the guard reads the whole flat gradient: finite padding, as in a trainer
    state = H.guard_state(DEV)
    H.grad_stats(g, state, grad_scale=0.5, max_norm=1e-3, skip_nonfinite=True, lr=LR, b1=B1, b2=B2)      # clips: the norm is ~0.4
    rec = H.guard_record(state)
    raw = run_stats(H, (p, g, m, v), ranges, step=9, grad_scale=123.0, guard=state, lr=77.0)      # scale, lr and step are the record's
    assert rec.apply == 1 and 0.0 < rec.coef < 1.0 and rec.gscale == np.float32(np.float32(0.5) * np.float32(rec.coef))
    check(raw, expected((p, g, m, v), ranges, rec.gscale, rec.step_size, rec.sqrt_bc2), 9)
    total = sum(r.g2 for r in records(raw))
    assert abs(np.sqrt(total) - rec.norm64 * rec.coef) <= 1e-6 * rec.norm64 * rec.coef      # the clipped gradient's norm
    assert H.guard_record(state).ticket == 0 and bytes(H.guard_record(state)) == bytes(rec)      # the record is only read
    g[ranges[2][0]] = float("nan")                          # a skipped step: apply == 0
    H.grad_stats(g, state, grad_scale=0.5, max_norm=float("inf"), skip_nonfinite=True, lr=LR, b1=B1, b2=B2)
    raw = run_stats(H, (p, g, m, v), ranges, step=10, guard=state)
    assert H.guard_record(state).apply == 0
    got = records(raw)
    assert all(r.u2 == 0.0 for r in got) and got[2].g_nonfinite == 1 and sum(r.g_nonfinite for r in got) == 1
    assert all(r.p2 > 0.0 for r in got)


# ---- cvae_trace_push ----
def row_of(ring, k):
    return cvlib.TraceRow.from_buffer_copy(ring.cpu().numpy()[128 * k:128 * (k + 1)].tobytes())


def test_trace_push_rows_and_wrap(H):
    cap = 3
    ring = torch.full((cap * 128,), 0xC3, dtype=torch.uint8, device=DEV)
    gen = torch.Generator().manual_seed(5)
    scal = [torch.rand(16, generator=gen).to(DEV) for _ in range(4)]
    scal[1][3] = float("nan")
    H.trace_push(ring, cap, 1, 1e-4, scal[0], 16)
    torch.cuda.synchronize()
    host = ring.cpu().numpy()
    assert (host[128:] == 0xC3).all(), "a push writes its own row only"
    r = row_of(ring, 0)
    assert (r.step, r.applied, r.nonfinite, r.n_scalars) == (1, 1, 0, 16) and r.lr == np.float32(1e-4) and r.coef == 1.0
    assert np.isnan(r.grad_norm) and bytes(r.reserved) == bytes(32)
    assert np.array_equal(np.frombuffer(bytes(r.scalars), np.uint32), scal[0].cpu().numpy().view(np.uint32))
    state = H.guard_state(DEV)
    g = torch.full((1024,), 0.25, device=DEV)
    H.grad_stats(g, state, grad_scale=1.0, max_norm=2.0, skip_nonfinite=True, lr=LR, b1=B1, b2=B2)      # norm 8: coef 0.25
    H.trace_push(ring, cap, 2, 2e-4, scal[1], 4, guard=state)
    rec = H.guard_record(state)
    torch.cuda.synchronize()
    assert (ring.cpu().numpy()[256:] == 0xC3).all()
    r = row_of(ring, 1)
    assert (r.step, r.applied, r.nonfinite, r.n_scalars) == (2, rec.apply, rec.nonfinite, 4) == (2, 1, 0, 4)
    assert r.grad_norm == rec.norm == 8.0 and r.coef == rec.coef and r.lr == np.float32(2e-4)
    got = np.frombuffer(bytes(r.scalars), np.uint32)
    assert np.array_equal(got[:4], scal[1].cpu().numpy().view(np.uint32)[:4]) and not got[4:].any()      # bit for bit, the NaN too
    assert bytes(H.guard_record(state)) == bytes(rec)
    H.trace_push(ring, cap, 3, 3e-4, scal[2], 0)
    before = ring.cpu().numpy().copy()
    H.trace_push(ring, cap, 2 ** 33 + 1 + cap - (2 ** 33) % cap, 4e-4, scal[3], 16)      # (step - 1) % cap == 0: the ring wraps, 64-bit step
    torch.cuda.synchronize()
    after = ring.cpu().numpy()
    assert np.array_equal(before[128:], after[128:]) and row_of(ring, 2).n_scalars == 0 and not any(row_of(ring, 2).scalars)
    r = row_of(ring, 0)
    assert r.step == 2 ** 33 + 1 + cap - (2 ** 33) % cap and (r.step - 1) % cap == 0 and r.lr == np.float32(4e-4)
    assert np.array_equal(np.frombuffer(bytes(r.scalars), np.uint32), scal[3].cpu().numpy().view(np.uint32))


# ---- CVAE_EINVAL: nothing is launched ----
def test_einval_launches_nothing(H):
    ranges, (p, g, m, v) = table("edge"), buffers("edge")
    n = p.numel()
    out = torch.full((len(ranges) * 48,), 0xA5, dtype=torch.uint8, device=DEV)
    scratch = torch.full((cvlib.tensor_stats_scratch_bytes(list(ranges)),), 0x5A, dtype=torch.uint8, device=DEV)
    ring = torch.full((4 * 128,), 0xC3, dtype=torch.uint8, device=DEV)
    scal = torch.zeros(16, device=DEV)
    lib, st = H.lib, torch.cuda.current_stream().cuda_stream

    def arrays(rs):
        return len(rs), (C.c_int64 * max(len(rs), 1))(*[b for b, _ in rs]), (C.c_int64 * max(len(rs), 1))(*[e for _, e in rs])

    def stats(rs=ranges, h=H.h, p_=p, g_=g, m_=m, v_=v, n_=n, step=1, out_=out, scratch_=scratch, begin=True, end=True):
        nt, b, e = arrays(list(rs))
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return lib.cvae_tensor_stats(h, ptr(p_), ptr(g_), ptr(m_), ptr(v_), n_, nt, b if begin else None, e if end else None, step,
                                     LR, B1, B2, EPS, 1.0, None, ptr(out_), ptr(scratch_), st)

    bad = [dict(h=None), dict(p_=None), dict(g_=None), dict(m_=None), dict(v_=None), dict(out_=None), dict(scratch_=None),
           dict(begin=False), dict(end=False), dict(step=0), dict(step=-4), dict(rs=[]), dict(rs=[(k, k + 1) for k in range(33)]),
           dict(rs=[(5, 5)]), dict(rs=[(9, 4)]), dict(rs=[(0, 8), (7, 12)]), dict(rs=[(20, 24), (0, 4)]), dict(rs=[(n - 2, n + 1)]),
           dict(n_=ranges[-1][1] - 1)]
    for kw in bad:
        assert stats(**kw) == -1, kw
        assert lib.cvae_last_error(), kw
    push = lambda **kw: lib.cvae_trace_push(kw.get("h", H.h), kw.get("ring", ring.data_ptr()), kw.get("cap", 4), kw.get("step", 1), LR,      # noqa: E731
                                            kw.get("scal", scal.data_ptr()), kw.get("ns", 16), None, st)
    for kw in (dict(h=None), dict(ring=None), dict(scal=None), dict(cap=0), dict(cap=-1), dict(step=0), dict(ns=-1), dict(ns=17)):
        assert push(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and (scratch.cpu().numpy() == 0x5A).all() and (ring.cpu().numpy() == 0xC3).all()
    assert stats() == 0 and push() == 0                    # the same calls with good arguments do write
    torch.cuda.synchronize()
    assert not (out.cpu().numpy() == 0xA5).all() and not (ring.cpu().numpy()[:128] == 0xC3).all()
