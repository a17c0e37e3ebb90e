"""The stream contract of the C-ABI (include/cvae.h: "all work is enqueued on the caller's hipStream_t", "no allocation, no device
synchronisation inside", "distinct handles are independent"), held on a side stream while the legacy null stream is kept busy.

Every other GPU test runs on the null stream, which hides exactly the faults this contract is about: a launch that goes to stream 0
instead of the caller's is ordered correctly anyway when the caller's stream IS stream 0.  torch.cuda.Stream() objects are created
non-blocking, so the null stream does not order them.  Here:

  independent_stream()  finds a side stream that provably runs ahead of a blocked null stream (the control, part of the result file);
  Harness.run           one scenario = one closure of a few entry points: reference run on the default stream, then on the side stream
                        with the null stream blocked (assertions a-d) and with the side stream itself blocked (e, f);
  SCENARIOS             the registry: every scenario declares the exported functions it calls, and tests/test_host_streams.py holds the
                        union against every function of include/cvae.h whose last parameter is `void* stream`.

The scenarios run in fresh child processes (tests/stream_worker.py, one per group) and leave a JSON record; tests/test_gpu_streams.py
asserts on it.  Importing this module needs neither torch nor a GPU: the builders import what they need when they run.

The six assertions of a scenario (the blocker's end event must be INCOMPLETE whenever it is queried; a complete one is a failure that
says the run was inconclusive, never a pass):
  a  null stream blocked: the end event is incomplete when the call returns on the host        -> no device-wide synchronisation
  b  ... and still incomplete once the side stream has finished                                 -> nothing it needed sat on the null stream
  c  the outputs, copied to the host on the side stream, equal the reference run bit for bit   -> a stray null-stream launch leaves poison
  d  after a device synchronize the outputs still hold those bits                              -> nothing ran late
  e  side stream blocked: its end event is incomplete when the call returns                    -> no host wait on the caller's stream
  f  after a synchronize the outputs equal the reference                                        -> a stray null-stream launch ran early, on poison
Outputs, workspace and scratch are filled with ws_tools.ALL_ONES before EVERY run, the reference run included, so memory a call
never writes (alignment padding, unused partial slots) holds the same bytes in every run."""
import os
import re
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "cvae.h")

HW_QUEUES = 8                 # GPU_MAX_HW_QUEUES of the worker's environment: the side stream gets a hardware queue of its own
CANDIDATES = 8                # side streams the control tries
BLOCK_MIN, BLOCK_MAX, BLOCK_FACTOR = 0.5, 3.0, 20.0       # blocker seconds: max(BLOCK_MIN, BLOCK_FACTOR x duration), capped
NOT_RUN = "not run"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the header: every exported function whose last parameter is `void* stream`
# ---------------------------------------------------------------------------------------------------------------------------------------
def header_stream_entries(path=HEADER):
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    names = []
    for m in re.finditer(r"\b(cvae_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        params = m.group(2)
        if re.search(r"void\s*\*\s*stream\s*$", params.strip()):
            names.append(m.group(1))
    assert len(names) == len(set(names)), "a function is declared twice"
    return sorted(names)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """A stand-in for the ctypes library object of a Handle that notes which stream-taking entry points are called, so that a
    scenario's declared entry points are the ones it really calls."""

    def __init__(self, lib, names, called):
        self.__dict__.update(_lib=lib, _names=frozenset(names), _called=called)

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in self._names:
            return f
        called = self._called

        def call(*args):
            called.add(name)
            return f(*args)
        return call


class Built:
    """What a scenario's builder returns: fn() enqueues the scenario's calls on the CURRENT stream and restores whatever state they
    change first; outputs: [(name, tensor)] compared bit for bit; scratch: tensors that are poisoned with the outputs."""

    def __init__(self, fn, outputs, scratch=()):
        self.fn, self.outputs, self.scratch = fn, list(outputs), list(scratch)
        for name, t in self.outputs:
            assert t.is_cuda and t.is_contiguous(), name


def raw(t):
    import torch
    return t.reshape(-1).view(torch.uint8)


class Harness:
    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        self.torch = torch
        self.called = set()
        self.names = header_stream_entries()
        self._handles = {}
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        self.blocker_kind, self.per_second = self._calibrate()
        self.control = []
        self.stream, self.independent = self.independent_stream()

    # ---- handles ----
    def record(self, handle):
        if not isinstance(handle.lib, Recorder):
            handle.lib = Recorder(handle.lib, self.names, self.called)
        return handle

    def handle(self, width=64, max_batch=8, precision="f32", overlap=False):
        from critic_vae_amd import lib as cvlib
        key = (width, max_batch, precision, overlap)
        if key not in self._handles:
            self._handles[key] = self.record(cvlib.Handle(width, max_batch, overlap_wgrad=overlap, precision=precision))
        return self._handles[key]

    # ---- the blocker ----
    def _timed(self, enqueue):
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enqueue()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / 1000.0

    def _mm_chain(self, n):
        for _ in range(int(n)):
            self.torch.mm(self._mm_a, self._mm_a, out=self._mm_b)

    def _calibrate(self):
        """Units of the blocker per second, measured once per process: spin cycles of torch.cuda._sleep, or, where that does not
        behave (a 0.2 s request that is off by more than 2x), large torch.mm calls."""
        torch = self.torch
        try:
            torch.cuda._sleep(1_000_000)
            torch.cuda.synchronize()
            n = 20_000_000
            rate = n / max(self._timed(lambda: torch.cuda._sleep(n)), 1e-9)
            got = self._timed(lambda: torch.cuda._sleep(int(0.2 * rate)))
            print(f"stream-blocker: torch.cuda._sleep, {rate:.4g} cycles / s; a 0.2 s request took {got:.3f} s")
            if 0.1 <= got <= 0.4:
                return "sleep", rate
        except Exception as e:                                   # noqa: BLE001 -- any failure of the private helper: use the matmuls
            print(f"stream-blocker: torch.cuda._sleep is not usable here ({e!r})")
        self._mm_a = torch.randn(4096, 4096, device="cuda") * 0.01
        self._mm_b = torch.empty_like(self._mm_a)
        self._mm_chain(4)
        torch.cuda.synchronize()
        rate = 32 / max(self._timed(lambda: self._mm_chain(32)), 1e-9)
        print(f"stream-blocker: torch.mm chain, {rate:.4g} products / s")
        return "mm", rate

    def block(self, seconds):
        """Enqueue `seconds` of work on the CURRENT stream and an end event behind it."""
        n = max(1, int(seconds * self.per_second))
        if self.blocker_kind == "sleep":
            self.torch.cuda._sleep(n)
        else:
            self._mm_chain(n)
        ev = self.torch.cuda.Event()
        ev.record()
        return ev

    @staticmethod
    def blocker_seconds(duration):
        return min(BLOCK_MAX, max(BLOCK_MIN, BLOCK_FACTOR * duration))

    # ---- the control ----
    def independent_stream(self):
        """The first of up to CANDIDATES torch side streams on which a tiny kernel completes while the null stream is blocked."""
        torch = self.torch
        probe = torch.zeros(64, device="cuda")
        last = None
        for k in range(CANDIDATES):
            s = torch.cuda.Stream()
            last = s
            with torch.cuda.stream(s):
                probe.add_(1.0)
            torch.cuda.synchronize()
            end = self.block(BLOCK_MIN)
            t0 = time.perf_counter()
            with torch.cuda.stream(s):
                probe.add_(1.0)
                done = torch.cuda.Event()
                done.record()
            done.synchronize()
            waited = time.perf_counter() - t0
            ahead = not end.query()
            torch.cuda.synchronize()
            self.control.append(dict(candidate=k, ran_ahead=bool(ahead), waited_s=round(waited, 4)))
            print(f"stream-control: candidate {k}: side stream done after {waited * 1e3:.2f} ms, null stream still blocked: {ahead}")
            if ahead:
                return s, True
        return last, False

    # ---- one scenario ----
    def _poison(self, b):
        from ws_tools import ALL_ONES, poison
        for _, t in b.outputs:
            poison(t, ALL_ONES)
        for t in b.scratch:
            poison(t, ALL_ONES)
        self.torch.cuda.synchronize()

    def _differs(self, b, ref, host=None):
        """Names of the outputs whose bytes differ from the reference (on the device, or the pinned host copies)."""
        torch = self.torch
        bad = []
        for i, (name, t) in enumerate(b.outputs):
            got = raw(t) if host is None else host[i]
            want = ref[i] if host is None else ref[i].cpu()
            if not torch.equal(got, want):
                bad.append(f"{name} ({int((got != want).sum())} of {got.numel()} bytes)")
        return bad

    def run(self, sc, b):
        torch, S = self.torch, self.stream
        rec = dict(name=sc.name, asserts={}, messages=[], declared=sorted(sc.entries))
        A, msg = rec["asserts"], rec["messages"]
        # 1. reference on the default stream (a first call before it: lazy kernel attributes, the library's side stream)
        self._poison(b)
        b.fn()
        torch.cuda.synchronize()
        self._poison(b)
        self.called.clear()
        dur = self._timed(b.fn)
        torch.cuda.synchronize()
        ref = [raw(t).clone() for _, t in b.outputs]
        host = [torch.empty(r.numel(), dtype=torch.uint8).pin_memory() for r in ref]
        length = self.blocker_seconds(dur)
        rec.update(duration_ms=dur * 1e3, blocker_s=length)
        # 2. the side stream without a blocker: its allocator pool and every first-call effect are behind us
        self._poison(b)
        with torch.cuda.stream(S):
            b.fn()
        torch.cuda.synchronize()
        bad = self._differs(b, ref)
        A["plain"] = not bad
        if bad:
            msg.append("side stream, nothing blocked: differs from the default-stream run: " + ", ".join(bad))
        # 3. null stream busy
        self._poison(b)
        e1 = self.block(length)
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            b.fn()
            done = torch.cuda.Event()
            done.record()
        a_ok = not e1.query()
        host_s = time.perf_counter() - t0
        if sc.host_async:
            A["a"] = a_ok
            if not a_ok:
                msg.append(f"a: the null stream's blocker ({length:.2f} s) had ended when the call returned after {host_s:.3f} s on the host: "
                           "a device-wide synchronisation inside the call (inconclusive if the host time is far below the blocker's)")
        else:
            A["a"] = NOT_RUN
        if self.independent:
            done.synchronize()
            A["b"] = not e1.query()
            if not A["b"]:
                msg.append(f"b: the side stream finished only after the null stream's blocker ({length:.2f} s): something it needed was "
                           "on the null stream (or the run was inconclusive)")
            with torch.cuda.stream(S):
                for h, (_, t) in zip(host, b.outputs):
                    h.copy_(raw(t), non_blocking=True)
            S.synchronize()
            still = not e1.query()
            bad = self._differs(b, ref, host)
            A["c"] = still and not bad
            if bad:
                msg.append("c: read on the side stream while the null stream was blocked: " + ", ".join(bad))
            if not still:
                msg.append("c: inconclusive, the null stream's blocker had ended when the outputs were read")
            torch.cuda.synchronize()
            bad = self._differs(b, ref)
            A["d"] = not bad
            if bad:
                msg.append("d: after the device synchronize: " + ", ".join(bad))
        else:
            torch.cuda.synchronize()
            A.update(b=NOT_RUN, c=NOT_RUN, d=NOT_RUN)
        # 4. own stream busy
        self._poison(b)
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            e2 = self.block(length)
            b.fn()
        e_ok = not e2.query()
        host_s = time.perf_counter() - t0
        if sc.host_async:
            A["e"] = e_ok
            if not e_ok:
                msg.append(f"e: the caller's stream was blocked for {length:.2f} s and had drained when the call returned after {host_s:.3f} s: "
                           "a host wait on the caller's stream inside the call or its wrapper")
        else:
            A["e"] = NOT_RUN
        torch.cuda.synchronize()
        if self.independent:
            bad = self._differs(b, ref)
            A["f"] = not bad
            if bad:
                msg.append("f: caller's stream blocked first: " + ", ".join(bad))
        else:
            A["f"] = NOT_RUN
        rec["called"] = sorted(self.called)
        if not sc.host_async:
            msg.append(f"a, e not asserted: {sc.why_not_async}")
        print(f"stream-scenario {sc.name}: duration {dur * 1e3:.3f} ms, blocker {length:.2f} s, "
              + " ".join(f"{k}={v}" for k, v in A.items()))
        return rec


# ---------------------------------------------------------------------------------------------------------------------------------------
# the registry
# ---------------------------------------------------------------------------------------------------------------------------------------
class Scenario:
    def __init__(self, name, group, entries, build, host_async=True, why_not_async=""):
        assert host_async or why_not_async, name
        self.name, self.group, self.entries, self.build = name, group, tuple(entries), build
        self.host_async, self.why_not_async = host_async, why_not_async


SCENARIOS = []
# Entry points with a stream parameter that deliberately have no scenario: name -> reason.  At most MAX_EXCLUDED.
EXCLUDED = {}
MAX_EXCLUDED = 3


def scenario(name, group, entries, **kw):
    def deco(build):
        assert all(s.name != name for s in SCENARIOS), name
        SCENARIOS.append(Scenario(name, group, entries, build, **kw))
        return build
    return deco


def registry_entries():
    return sorted({e for s in SCENARIOS for e in s.entries})


def groups():
    out = []
    for s in SCENARIOS:
        if s.group not in out:
            out.append(s.group)
    return out


def group_timeout(group):
    """Seconds a worker may take: start-up and the control, then per scenario two blockers at their cap plus the runs."""
    return 90 + 10 * sum(1 for s in SCENARIOS if s.group == group)


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def _rand(seed, *shape, lo=0.0, hi=1.0):
    import torch
    return (torch.rand(*shape, generator=_gen(seed)) * (hi - lo) + lo).cuda()


def _randn(seed, *shape, scale=1.0):
    import torch
    return (torch.randn(*shape, generator=_gen(seed)) * scale).cuda()


def _u8(seed, *shape):
    import torch
    return torch.randint(0, 256, shape, generator=_gen(seed), dtype=torch.uint8).cuda()


def _empty(*shape, dtype=None):
    import torch
    return torch.empty(*shape, dtype=dtype or torch.float32, device="cuda")


def _named(**kw):
    return list(kw.items())


# ---- the step through the Handle ----
STEP_ENTRIES = ("cvae_forward", "cvae_loss", "cvae_backward", "cvae_adam_step")
STEP_CASES = ([(64, 5, p) for p in ("f32", "bf16", "bf16x9", "bf16x6")] + [(128, 3, p) for p in ("f32", "bf16")])


def _rig(H, W, B, precision, overlap):
    """ws_tools.StepRig's buffers around a model whose handle runs the weight gradients on the library's side stream or not."""
    import torch
    from critic_vae_amd import synth
    from critic_vae_amd.lib import SYNC_DOUBLES
    from critic_vae_amd.nets import VariationalAutoencoder
    vae = VariationalAutoencoder(max_batch=B, seed=0, width=W, precision=precision, overlap_wgrad=overlap).cuda()
    vae.load_reference_params(synth.make_params(0, W))
    assert vae.handle.overlap_wgrad == overlap
    H.record(vae.handle)

    class Rig:
        pass
    r = Rig()
    r.vae, r.h, r.B, r.W = vae, vae.handle, B, W
    r.theta = vae.theta.data
    r.theta0, r.bn0 = r.theta.clone(), vae.bn_state.clone()
    r.bn = vae.bn_state
    r.ws = vae._workspace(B)
    r.mu, r.logvar, r.d_mu, r.d_logvar = (_empty(B, 32) for _ in range(4))
    r.recon, r.d_recon = _empty(B, 3, W, W), _empty(B, 3, W, W)
    r.scalars = _empty(16)
    r.grads, r.grads_seen = torch.empty_like(r.theta), torch.empty_like(r.theta)
    r.m, r.v = torch.empty_like(r.theta), torch.empty_like(r.theta)
    r.sync = _empty(SYNC_DOUBLES, dtype=torch.float64)
    r.x, r.pred, r.eps = (torch.from_numpy(a).cuda() for a in synth.make_batch(11, 0, B, W))

    def restore():
        r.theta.copy_(r.theta0)
        r.bn.copy_(r.bn0)
        r.m.zero_()
        r.v.zero_()
    r.restore = restore

    def fwd_loss():
        r.h.forward(B, r.x, r.pred, r.eps, r.theta, r.bn, r.mu, r.logvar, r.recon, r.ws, train=True)
        r.h.loss(B, r.x, r.mu, r.logvar, r.recon, r.ws, r.scalars, r.d_recon, r.d_mu, r.d_logvar)
    r.fwd_loss = fwd_loss
    r.bwd_args = lambda: (B, r.x, r.pred, r.eps, r.theta, r.logvar, r.recon, r.d_recon, r.d_mu, r.d_logvar, r.ws)
    r.outputs = _named(mu=r.mu, logvar=r.logvar, recon=r.recon, scalars=r.scalars, d_recon=r.d_recon, d_mu=r.d_mu, d_logvar=r.d_logvar,
                       grads=r.grads, grads_seen=r.grads_seen, theta=r.theta, m=r.m, v=r.v, bn_state=r.bn)
    r.scratch = [r.ws, r.sync]
    return r


def _step_builder(W, B, precision, overlap):
    def build(H):
        r = _rig(H, W, B, precision, overlap)

        def fn():
            r.restore()
            r.fwd_loss()
            r.h.backward(*r.bwd_args(), r.grads)
            r.grads_seen.copy_(r.grads)            # the gradient is read on the caller's stream straight behind cvae_backward
            r.h.adam_step(r.theta, r.grads, r.m, r.v, 1, 1e-3)
        return Built(fn, r.outputs, r.scratch)
    return build


for _W, _B, _p in STEP_CASES:
    for _ov in (False, True):
        scenario(f"step-w{_W}-b{_B}-{_p}-{'overlap' if _ov else 'inline'}", f"step{_W}", STEP_ENTRIES)(_step_builder(_W, _B, _p, _ov))


def _staged_builder(precision):
    def build(H):
        r = _rig(H, 64, 5, precision, True)
        h, B = r.h, r.B

        def fn():
            r.restore()
            for k in range(5):
                h.forward_stage(k, B, r.x, r.pred, r.eps, r.theta, r.bn, r.mu, r.logvar, r.recon, r.ws, r.sync)
            for k in range(2):
                h.loss_stage(k, B, r.x, r.mu, r.logvar, r.recon, r.ws, r.scalars, r.d_recon, r.d_mu, r.d_logvar, r.sync)
            for k in range(5):
                h.backward_stage(k, *r.bwd_args(), r.grads, r.sync)
            r.grads_seen.copy_(r.grads)
        return Built(fn, r.outputs + [("sync", r.sync)], [r.ws])
    return build


for _p in ("f32", "bf16"):
    scenario(f"staged-w64-b5-{_p}-overlap", "step64", ("cvae_forward_stage", "cvae_loss_stage", "cvae_backward_stage"))(_staged_builder(_p))


def _phases_builder(W, B, precision):
    def build(H):
        import torch
        from critic_vae_amd.lib import _ptr, _stream
        r = _rig(H, W, B, precision, True)
        h = r.h
        g16 = torch.empty(r.grads.numel(), dtype=torch.bfloat16, device="cuda")
        back = torch.empty_like(r.grads)

        def phase(ph, zero_padding):
            """Handle.backward_phase, with bit 3 (write 0 into the alignment padding of `grads`: one more launch) where asked."""
            n, x, pred, eps, theta, logvar, recon, d_recon, d_mu, d_logvar, ws = r.bwd_args()
            h._check(h.lib.cvae_backward_phases(h.h, n, _ptr(x), _ptr(pred), _ptr(eps), _ptr(theta), _ptr(logvar), _ptr(recon),
                                                _ptr(d_recon), _ptr(d_mu), _ptr(d_logvar), _ptr(ws), _ptr(r.grads),
                                                (1 << ph) | (8 if zero_padding else 0), _stream()))

        def fn():
            r.restore()
            r.fwd_loss()
            for ph in range(3):
                phase(ph, ph == 0)
                off, n = h.grad_bucket(ph)
                h.grads_to_bf16(r.grads[off:off + n], g16[off:off + n])
                h.grads_from_bf16(g16[off:off + n], back[off:off + n])
        return Built(fn, r.outputs + [("grads16", g16), ("grads_back", back)], r.scratch)
    return build


# The bucket is read straight behind its phase.  With the weight gradients on the library's side stream, phase 0 alone ends in a join
# that a whole cvae_backward would still reach at the end of its later phases: only here does a missing one show.
PHASE_CASES = ((64, 5, "f32"), (64, 5, "bf16"), (128, 3, "f32"), (128, 3, "bf16"))
for _W, _B, _p in PHASE_CASES:
    scenario(f"phases-w{_W}-b{_B}-{_p}-overlap", f"step{_W}",
             ("cvae_forward", "cvae_loss", "cvae_backward_phases", "cvae_grads_to_bf16", "cvae_grads_from_bf16"))(_phases_builder(_W, _B, _p))


# ---- optimizer ----
def _opt_state(n, seed):
    import torch
    p, g = _randn(seed, n, scale=0.1), _randn(seed + 1, n, scale=0.01)
    m, v = _randn(seed + 2, n, scale=0.01), _rand(seed + 3, n, hi=1e-4)
    live = dict(p=torch.empty_like(p), m=torch.empty_like(m), v=torch.empty_like(v))
    init = dict(p=p, m=m, v=v)

    def restore():
        for k in live:
            live[k].copy_(init[k])
    return live, g, restore


N_BIG = 2_097_152 + 1028      # the second trip of the grid-stride loops (test_gpu_optim.py)


@scenario("optim-guarded-opt-2m","optim", ("cvae_guard_init", "cvae_grad_stats", "cvae_adam_step_guarded_opt"))
def _optim_big(H):
    import torch
    h, n = H.handle(), N_BIG
    live, g, restore = _opt_state(n, 100)
    ema0, aux, aux0 = _randn(110, n, scale=0.1), _randn(111, 960), _randn(112, 960)
    ema, aux_ema = torch.empty_like(ema0), torch.empty_like(aux0)
    state = torch.empty((h.lib.cvae_guard_state_bytes() + 7) // 8, dtype=torch.int64, device="cuda")
    step = n // 16
    opt = dict(decay_mul=0.999, ema_omd=0.01, ranges=[(k * step + 3, k * step + step // 2 + 1) for k in range(16)])

    def fn():
        restore()
        ema.copy_(ema0)
        aux_ema.copy_(aux0)
        h.guard_init(state, 3, 1)
        h.grad_stats(g, state, 1.0, 1.0, True, 1e-3)
        h.adam_step_guarded_opt(live["p"], g, live["m"], live["v"], state, opt=opt, ema=ema, aux=aux, aux_ema=aux_ema)
    return Built(fn, _named(ema=ema, aux_ema=aux_ema, guard=state, **live))


@scenario("optim-plain-forms-1028", "optim", ("cvae_adam_step", "cvae_adam_step_opt", "cvae_guard_init", "cvae_grad_stats", "cvae_adam_step_guarded"))
def _optim_small(H):
    import torch
    h, n = H.handle(), 1028
    sets = [_opt_state(n, 200 + 10 * k) for k in range(3)]
    ema0 = _randn(240, n, scale=0.1)
    ema = torch.empty_like(ema0)
    state = torch.empty((h.lib.cvae_guard_state_bytes() + 7) // 8, dtype=torch.int64, device="cuda")
    opt = dict(decay_mul=0.99, ema_omd=0.05, ranges=[(5, 300), (301, 1027)])

    def fn():
        for _, _, restore in sets:
            restore()
        ema.copy_(ema0)
        (a, ga, _), (b, gb, _), (c, gc, _) = sets
        h.adam_step(a["p"], ga, a["m"], a["v"], 3, 1e-3)
        h.adam_step_opt(b["p"], gb, b["m"], b["v"], 3, 1e-3, opt=opt, ema=ema)
        h.guard_init(state)
        h.grad_stats(gc, state, 1.0, 0.05, True, 1e-3)
        h.adam_step_guarded(c["p"], gc, c["m"], c["v"], state)
    outs = [(f"{k}{i}", t) for i, (live, _, _) in enumerate(sets) for k, t in live.items()]
    return Built(fn, outs + [("ema", ema), ("guard", state)])


@scenario("scale-loss-grads", "optim", ("cvae_scale_loss_grads",))
def _scale(H):
    h, B = H.handle(), 5
    g, dr, dm, dl = _rand(300, 1, lo=0.5, hi=2.0), _randn(301, B, 3, 64, 64), _randn(302, B, 32), _randn(303, B, 32)
    o = dict(d_recon=_empty(B, 3, 64, 64), d_mu=_empty(B, 32), d_logvar=_empty(B, 32))
    return Built(lambda: h.scale_loss_grads(B, g, dr, dm, dl, o["d_recon"], o["d_mu"], o["d_logvar"]), _named(**o))


# ---- inference and scores ----
def _infer(H, B=5):
    """An eval-mode model and one batch with its (mu, logvar, recon), computed once on the default stream."""
    import torch
    if not hasattr(H, "_infer"):
        r = _rig(H, 64, 8, "f32", False)
        r.h.forward(B, r.x[:B], r.pred[:B], r.eps[:B], r.theta, r.bn, r.mu, r.logvar, r.recon, r.ws, train=False)
        torch.cuda.synchronize()
        r.mu_in, r.logvar_in, r.recon_in = r.mu.clone(), r.logvar.clone(), r.recon.clone()
        H._infer = r
    return H._infer


@scenario("forward-eval", "infer", ("cvae_forward",))
def _forward_eval(H):
    r, B = _infer(H), 5
    return Built(lambda: r.h.forward(B, r.x, r.pred, r.eps, r.theta, r.bn, r.mu, r.logvar, r.recon, r.ws, train=False),
                 _named(mu=r.mu[:B], logvar=r.logvar[:B], recon=r.recon[:B]), [r.ws])


@scenario("decode-caller-zcat", "infer", ("cvae_decode",))
def _decode(H):
    r, B = _infer(H), 5
    zcat, recon = _randn(400, B, 33), _empty(B, 3, 64, 64)
    return Built(lambda: r.h.decode(B, zcat, r.theta, recon, r.ws), [("recon", recon)], [r.ws])


@scenario("loss-obj", "infer", ("cvae_loss_obj",))
def _loss_obj(H):
    r, B = _infer(H), 5
    o = dict(scalars=_empty(16), d_recon=_empty(B, 3, 64, 64), d_mu=_empty(B, 32), d_logvar=_empty(B, 32))
    return Built(lambda: r.h.loss_obj(B, r.x, r.mu_in, r.logvar_in, r.recon_in, r.ws, (0.7, 0.3, 0.002, 1), o["scalars"], o["d_recon"],
                                      o["d_mu"], o["d_logvar"]), _named(**o), [r.ws])


@scenario("score-init-score-finish", "infer", ("cvae_score_init", "cvae_score", "cvae_score_finish"))
def _score(H):
    import torch
    r, B = _infer(H), 5
    state = _empty(r.h.score_state_bytes() // 8, dtype=torch.float64)
    rows, scalars = _empty(B, 8), _empty(16)

    def fn():
        r.h.score_init(state)
        r.h.score(B, r.x, r.mu_in, r.logvar_in, r.recon_in, r.ws, per_image=rows, state=state)
        r.h.score_finish(state, scalars)
    return Built(fn, _named(state=state, rows=rows, scalars=scalars), [r.ws])


@scenario("inject-zcat", "infer", ("cvae_inject_zcat",))
def _inject(H):
    r = _infer(H)
    mu, rewards, zcat = _randn(410, 2, 32), _rand(411, 3), _empty(6, 33)
    return Built(lambda: r.h.inject_zcat(2, 3, mu, rewards, zcat), [("zcat", zcat)])


@scenario("recon-zcat", "infer", ("cvae_recon_zcat",))
def _recon_zcat(H):
    import torch
    r = _infer(H)
    ent_sel = torch.tensor([0, 0, 1, 2, 3, 3, 4], dtype=torch.int64).cuda()
    ent_kind = torch.tensor([0, 1, 0, 1, 0, 1, 0], dtype=torch.int32).cuda()
    mu, preds, zcat = _randn(420, 5, 32), _rand(421, 5), _empty(7, 33)
    return Built(lambda: r.h.recon_zcat(7, ent_sel, ent_kind, mu, preds, zcat), [("zcat", zcat)])


# ---- critic ----
CRITIC_BATCHES = (5, 257)     # 257: the second image of a workgroup of the persistent kernels on a device of up to 256 compute units


def _critic(H, B):
    h = H.handle(64, 264)
    n = h.lib.cvae_critic_param_count()
    return h, _randn(500, n, scale=0.1), _rand(501 + B, B, 3, 64, 64)


def _critic_scenarios(B):
    import_name = f"b{B}"

    @scenario(f"critic-forward-{import_name}", "critic", ("cvae_critic_forward",))
    def _fwd(H):
        h, w, x = _critic(H, B)
        pred = _empty(B)
        return Built(lambda: h.critic_forward(B, x, w, pred), [("pred", pred)])

    @scenario(f"critic-grad-{import_name}", "critic", ("cvae_critic_grad",))
    def _grad(H):
        import torch
        from critic_vae_amd import lib as cvlib
        h, w, x = _critic(H, B)
        target = _rand(510, B)
        keep = (_rand(511, B, cvlib.CRITIC_KEEP) >= 0.3).to(torch.uint8)
        o = dict(grads=_empty(cvlib.CRITIC_TRAIN_FLOATS), pred=_empty(B), scalars=_empty(4),
                 decisions=_empty(B, cvlib.CRITIC_DECISIONS, dtype=torch.uint8))
        scratch = _empty(h.critic_grad_scratch_bytes(B), dtype=torch.uint8)
        return Built(lambda: h.critic_grad(B, x, target, keep, 0.3, 0, w, o["grads"], o["pred"], o["scalars"], scratch, decisions=o["decisions"]),
                     _named(**o), [scratch])

    @scenario(f"critic-score-{import_name}", "critic", ("cvae_critic_score_init", "cvae_critic_score"))
    def _score_(H):
        import torch
        h, w, _ = _critic(H, B)
        n = B + 3
        frames, targets = _u8(520, n, 64, 64, 3), _rand(521, n)
        idx = torch.randint(0, n, (B,), generator=_gen(522), dtype=torch.int64).cuda()
        state = _empty(h.lib.cvae_critic_score_state_bytes() // 8, dtype=torch.float64)
        rows = _empty(B, 8)

        def fn():
            h.critic_score_init(state)
            h.critic_score(B, frames, targets, w, idx=idx, per_frame=rows, state=state)
        return Built(fn, _named(state=state, rows=rows))

    @scenario(f"critic-collect-{import_name}", "critic", ("cvae_critic_collect",))
    def _collect(H):
        from critic_vae_amd import lib as cvlib
        h, w, x = _critic(H, B)
        pred = _empty(B)
        emb = [_empty(B, *s) for s in cvlib.CRITIC_EMBED_SHAPES]
        return Built(lambda: h.critic_collect(B, x, w, pred, emb), [("pred", pred)] + [(f"e{i + 1}", e) for i, e in enumerate(emb)])

    @scenario(f"critic-saliency-{import_name}", "critic", ("cvae_critic_saliency",))
    def _saliency(H):
        import torch
        from critic_vae_amd import lib as cvlib
        h, w, x = _critic(H, B)
        o = {}
        for steps in (1, 4):
            o.update({f"pred{steps}": _empty(B), f"map{steps}": _empty(B, 64, 64), f"max{steps}": _empty(B), f"grad{steps}": _empty(B, 3, 64, 64),
                      f"dec{steps}": _empty(B, cvlib.CRITIC_DECISIONS, dtype=torch.uint8)})

        def fn():
            for s in (1, 4):
                h.critic_saliency(B, x, w, s, o[f"pred{s}"], o[f"map{s}"], o[f"max{s}"], grad=o[f"grad{s}"], decisions=o[f"dec{s}"])
        return Built(fn, _named(**o))

    @scenario(f"critic-occlusion-{import_name}", "critic", ("cvae_critic_occlusion",))
    def _occlusion(H):
        h, w, x = _critic(H, B)
        o = dict(pred=_empty(B), drop=_empty(B, 4, 4), map=_empty(B, 64, 64), max=_empty(B))
        return Built(lambda: h.critic_occlusion(B, x, w, 16, (0.25, 0.5, 0.125), o["pred"], o["drop"], o["map"], o["max"]), _named(**o))


for _B in CRITIC_BATCHES:
    _critic_scenarios(_B)


# ---- data ----
@scenario("preprocess-u8", "data", ("cvae_preprocess_u8",))
def _preprocess(H):
    h, B = H.handle(), 5
    frames, x = _u8(600, B, 64, 64, 3), _empty(B, 3, 64, 64)
    return Built(lambda: h.preprocess_u8(B, frames, x), [("x", x)])


def _trajectories():
    import torch
    offsets = torch.tensor([0, 40, 100, 130], dtype=torch.int64).cuda()
    return offsets, _rand(610, 130), 130, 3


@scenario("curate-select-gather-frames", "data", ("cvae_curate_select", "cvae_gather_frames_u8"))
def _curate(H):
    import torch
    h = H.handle()
    offsets, preds, n, nt = _trajectories()
    i64 = lambda *s: _empty(*s, dtype=torch.int64)      # noqa: E731
    running = i64(1)
    o = dict(running=running, counts=i64(nt, 3), first=i64(nt), span=i64(2), sel=i64(n),
             dst=_empty(200, 64, 64, 3, dtype=torch.uint8), dst_preds=_empty(200))
    src = _u8(611, n, 64, 64, 3)

    def fn():
        running.fill_(7)
        h.curate_select(offsets, preds, 5, 1000, running, o["counts"], o["first"], o["span"], o["sel"])
        h.gather_frames_u8(src, preds, o["sel"], n, o["span"], o["dst"], o["dst_preds"])
    return Built(fn, _named(**o))


@scenario("curate-select-recon", "data", ("cvae_curate_select_recon",))
def _curate_recon(H):
    import torch
    h = H.handle()
    offsets, preds, n, nt = _trajectories()
    i64 = lambda *s: _empty(*s, dtype=torch.int64)      # noqa: E731
    running = i64(1)
    o = dict(running=running, counts=i64(nt, 3), first=i64(nt), sel_first=i64(nt), span=i64(3), ent_frame=i64(2 * n),
             ent_kind=_empty(2 * n, dtype=torch.int32), ent_sel=i64(2 * n), sel=i64(n))

    def fn():
        running.fill_(0)
        h.curate_select_recon(offsets, preds, 5, 1000, running, o["counts"], o["first"], o["sel_first"], o["span"], o["ent_frame"],
                              o["ent_kind"], o["ent_sel"], o["sel"])
    return Built(fn, _named(**o))


AUG = (0x1234_5678_9ABC, 1 << 23, 4, 6553)        # key, flip with probability 1/2, shifts up to 4 pixels, brightness 0.1


@scenario("gathers-u8", "data", ("cvae_preprocess_u8_gather", "cvae_preprocess_u8_gather_aug"))
def _gather_u8(H):
    import torch
    h, B, n = H.handle(), 5, 11
    frames, preds = _u8(620, n, 64, 64, 3), _rand(621, n)
    idx = torch.randint(0, n, (B,), generator=_gen(622), dtype=torch.int64).cuda()
    o = dict(x=_empty(B, 3, 64, 64), pred=_empty(B), xa=_empty(B, 3, 64, 64), preda=_empty(B), applied=_empty(B, 4, dtype=torch.int32))

    def fn():
        h.preprocess_u8_gather(B, frames, preds, idx, o["x"], o["pred"])
        h.preprocess_u8_gather_aug(B, frames, preds, idx, AUG, o["xa"], o["preda"], o["applied"])
    return Built(fn, _named(**o))


@scenario("gathers-f32", "data", ("cvae_gather_f32", "cvae_gather_f32_aug"))
def _gather_f32(H):
    import torch
    h, B, n = H.handle(), 5, 11
    frames, preds = _rand(630, n, 3, 64, 64, lo=-1.0), _rand(631, n)
    idx = torch.randint(0, n, (B,), generator=_gen(632), dtype=torch.int64).cuda()
    o = dict(x=_empty(B, 3, 64, 64), pred=_empty(B), xa=_empty(B, 3, 64, 64), preda=_empty(B), applied=_empty(B, 4, dtype=torch.int32))

    def fn():
        h.gather_f32(B, frames, preds, idx, o["x"], o["pred"])
        h.gather_f32_aug(B, frames, preds, idx, AUG[:3] + (0,), o["xa"], o["preda"], o["applied"])
    return Built(fn, _named(**o))


# ---- segmentation ----
@scenario("diff-grey-normalize-counts", "segment", ("cvae_diff_grey", "cvae_diff_normalize", "cvae_mask_counts"))
def _diff(H):
    import torch
    h, B = H.handle(), 3
    r1, r0 = _rand(700, B, 3, 64, 64, lo=-1.0), _rand(701, B, 3, 64, 64, lo=-1.0)
    gt = (_rand(702, B, 64, 64) > 0.6).to(torch.uint8)
    u8 = lambda: _empty(B, 64, 64, dtype=torch.uint8)      # noqa: E731
    o = dict(diff=_empty(B, 64, 64), diff_u8=u8(), mask=u8(), counts=_empty(B, 3, dtype=torch.int64), hist=_empty(2, 256, dtype=torch.int64),
             counts2=_empty(B, 3, dtype=torch.int64))

    def fn():
        o["hist"].zero_()                          # the histogram is ADDED to
        h.diff_grey(B, r1, r0, o["diff"])
        h.diff_normalize(B, o["diff"], 0.6, 1.0 / 0.6, 40, gt, o["diff_u8"], o["mask"], o["counts"], o["hist"])
        h.mask_counts(B, o["mask"], gt, o["counts2"])
    return Built(fn, _named(**o))


def _crf_inputs(B):
    import torch
    return _u8(710, B, 64, 64, 3), _rand(711, B, 64, 64), _u8(712, B, 64, 64), (_rand(713, B, 64, 64) > 0.5).to(torch.uint8)


@scenario("dense-crf", "segment", ("cvae_dense_crf",))
def _crf(H):
    import torch
    from critic_vae_amd import lib as cvlib
    h, B = H.handle(), 2
    frames, prob1, _, _ = _crf_inputs(B)
    params = cvlib.CrfParams(5.0, 20.0, 13.0, 3.0, 3.0, 1e-5, 2)
    labels, q1 = _empty(B, 64, 64, dtype=torch.uint8), _empty(B, 64, 64)
    scratch = _empty(h.crf_scratch_bytes(B), dtype=torch.uint8)
    return Built(lambda: h.dense_crf(B, frames, prob1, params, labels, q1, scratch), _named(labels=labels, q1=q1), [scratch])


@scenario("crf-grid-k9", "segment", ("cvae_crf_grid",))
def _crf_grid(H):
    import torch
    h, B, K = H.handle(), 2, 9
    frames, prob1, diff_u8, gt = _crf_inputs(B)
    assert K > h.crf_grid_group(), "K = 9 no longer spans two variant groups"
    variants = [(-1 if k % 3 == 0 else 40 + 20 * k, 1e-5, 3.0 + k, 1.0 + 0.5 * k) for k in range(K)]
    o = dict(counts=_empty(2, K, B, 3, dtype=torch.int64), labels=_empty(K, B, 64, 64, dtype=torch.uint8), q1=_empty(K, B, 64, 64))
    scratch = _empty(h.crf_grid_scratch_bytes(B, K), dtype=torch.uint8)
    return Built(lambda: h.crf_grid(B, frames, prob1, diff_u8, gt, (20.0, 13.0, 3.0), variants, (1, 2), o["counts"], o["labels"], o["q1"], scratch),
                 _named(**o), [scratch])


# ---- pictures and trace ----
@scenario("compose-frames", "render", ("cvae_compose_frames",))
def _compose(H):
    import torch
    from critic_vae_amd import lib as cvlib
    h, B, W = H.handle(), 3, 64
    recon, frames = _rand(800, B, 3, W, W, lo=-1.0), _u8(801, B, W, W, 3)
    mask = (_rand(802, B, W, W) > 0.5).to(torch.uint8)
    overlay = (_rand(803, 2 * W, 3 * W) > 0.9).to(torch.uint8)
    out = _empty(B, 2 * W, 3 * W, 3, dtype=torch.uint8)
    panels = [(cvlib.PANEL_F32_CHW, recon, 3 * W * W), (cvlib.PANEL_U8_HWC, frames, 3 * W * W), (cvlib.PANEL_MASK, mask, W * W)]
    return Built(lambda: h.compose_frames(B, panels, W, out, overlay=overlay), [("out", out)])


@scenario("trace-push-tensor-stats", "render", ("cvae_trace_push", "cvae_tensor_stats"))
def _trace(H):
    import torch
    from critic_vae_amd import lib as cvlib
    h, n = H.handle(), 70_000
    p, g, m, v = _randn(810, n, scale=0.1), _randn(811, n, scale=0.01), _randn(812, n, scale=0.01), _rand(813, n, hi=1e-4)
    scalars = _rand(814, 16)
    ranges = [(1, 3000), (3003, 66_001), (66_004, n)]
    ring, out = _empty(4 * 128, dtype=torch.uint8), _empty(48 * len(ranges), dtype=torch.uint8)
    scratch = _empty(cvlib.tensor_stats_scratch_bytes(ranges), dtype=torch.uint8)

    def fn():
        h.trace_push(ring, 4, 6, 1e-3, scalars)
        h.tensor_stats(p, g, m, v, ranges, 6, out, scratch, lr=1e-3)
    return Built(fn, _named(ring=ring, stats=out), [scratch])


# ---- per-op entry points ----
def _links(rig, layer):
    """test_gpu_conv_dispatch.links: the operands the step left for conv layer 1..7, as clones."""
    from bf16_ops_tools import geom
    h, W, B = rig.h, rig.W, rig.B
    cin, cout, ho, _, hi = geom(layer, W)
    per = 2 if h.precision == "bf16" else 1
    n_in, n_out = B * hi * hi * cin // per, B * ho * ho * cout // per
    i = layer - 4
    src = f"a{layer - 1}" if layer < 4 else ("h" if i == 0 else f"o{i - 1}")
    d_dst = f"d_y{layer}" if layer < 4 else f"d_o{i}"
    name = f"enc{layer}" if layer < 4 else f"dec{i}"
    (ow, nw), (ob, nb) = h.layout[name + ".w"], h.layout[name + ".b"]
    view = lambda nm, n: h.ws_view(rig.ws, B, nm, n).clone()      # noqa: E731
    return view(src, n_in), view(d_dst, n_out), rig.theta[ow:ow + nw].clone(), rig.theta[ob:ob + nb].clone(), n_in, n_out, nw, nb


def _stepped_rig(H, precision):
    import torch
    r = _rig(H, 64, 5, precision, False)
    r.restore()
    r.fwd_loss()
    r.h.backward(*r.bwd_args(), r.grads)
    torch.cuda.synchronize()
    return r


def _op_conv_builder(precision):
    def build(H):
        r = _stepped_rig(H, precision)
        h, B = r.h, r.B
        scratch = _empty(h.op_scratch_floats(B))
        jobs, outs = [], []
        for layer in (2, 6):          # one layer of each row of the conv table: E2..E4 / D0 and D1..D3
            x, dy, w, b, n_in, n_out, nw, nb = _links(r, layer)
            part = _empty(h.op_bn_partial_floats(layer, B)) if layer < 4 else None
            o = dict(out=_empty(n_out), din=_empty(n_in), dw=_empty(nw), db=_empty(nb))
            jobs.append((layer, x, dy, w, b, part, o))
            outs += [(f"L{layer}.{k}", t) for k, t in o.items()] + ([(f"L{layer}.part", part)] if part is not None else [])

        def fn():
            for layer, x, dy, w, b, part, o in jobs:
                h.op_conv_fwd(layer, B, x, w, b, o["out"], part, scratch)
                h.op_conv_dgrad(layer, B, dy, w, x if layer >= 5 else None, o["din"], scratch)
                h.op_conv_wgrad(layer, B, x, dy, o["dw"], o["db"], scratch)
        return Built(fn, outs, [scratch])
    return build


for _p in ("f32", "bf16", "bf16x9", "bf16x6"):
    scenario(f"op-conv-{_p}", "ops", ("cvae_op_conv_fwd", "cvae_op_conv_dgrad", "cvae_op_conv_wgrad"))(_op_conv_builder(_p))


@scenario("op-d4-bwd", "ops", ("cvae_op_d4_bwd",))
def _op_d4(H):
    r = _stepped_rig(H, "f32")
    h, B, W = r.h, r.B, r.W
    n_o3 = B * 32 * (W // 2) ** 2
    o3 = h.ws_view(r.ws, B, "o3", n_o3).clone()
    ow, nw = h.layout["dec4.w"]
    w, recon, d_recon = r.theta[ow:ow + nw].clone(), r.recon.clone(), r.d_recon.clone()
    o = dict(dout=_empty(B, 3, W, W), d_o3=_empty(n_o3), dw=_empty(nw), db=_empty(3))
    scratch = _empty(h.op_scratch_floats(B))
    return Built(lambda: h.op_d4_bwd(B, o3, d_recon, recon, w, o["dout"], o["d_o3"], o["dw"], o["db"], scratch), _named(**o), [scratch])


@scenario("op-e1-wgrad-fused", "ops", ("cvae_op_e1_wgrad_fused",))
def _op_e1_fused(H):
    """The step's fused E1 weight gradient on the operands a step left: the fp32 kernel (its y0 from the workspace), the bf16 kernel
    (no y0) from the fp32 frame and, with flag bit 0, from the packed frame that the entry's statistics pass writes into scratch."""
    jobs, outs, scr = [], [], []
    for p in ("f32", "bf16"):
        r = _stepped_rig(H, p)
        h, B, W = r.h, r.B, r.W
        per = 2 if p == "bf16" else 1
        n_pool = B * (W // 2) ** 2 * 32 // per
        y0 = h.ws_view(r.ws, B, "y0", B * W * W * 32).clone() if p == "f32" else None
        a0, d_a0 = h.ws_view(r.ws, B, "a0", n_pool).clone(), h.ws_view(r.ws, B, "d_a0", n_pool).clone()
        coef0, bcoef0 = h.ws_view(r.ws, B, "coef0", 128).clone(), _randn(930, 64, scale=0.01)
        (ow, nw), (ob, nb) = h.layout["enc0.w"], h.layout["enc0.b"]
        w1, b1 = r.theta[ow:ow + nw].clone(), r.theta[ob:ob + nb].clone()
        scratch = _empty(h.op_scratch_floats(B))
        scr.append(scratch)
        for flags in ((0,) if p == "f32" else (0, 1)):
            o = dict(dw=_empty(nw), db=_empty(nb))
            jobs.append((h, B, r.x.clone(), y0, a0, d_a0, coef0, bcoef0, w1, b1, o, scratch, flags))
            outs += [(f"{p}.f{flags}.{k}", t) for k, t in o.items()]

    def fn():
        for h, B, x, y0, a0, d_a0, coef0, bcoef0, w1, b1, o, scratch, flags in jobs:
            h.op_e1_wgrad_fused(B, x, y0, a0, d_a0, coef0, bcoef0, w1, b1, o["dw"], o["db"], scratch, flags)
    return Built(fn, outs, scr)


@scenario("op-bn", "ops", ("cvae_op_bn_pool_act_fwd", "cvae_op_bn_fwd_finalize", "cvae_op_bn_pool_act_bwd"))
def _op_bn(H):
    import torch
    from bf16_ops_tools import geom
    r = _stepped_rig(H, "f32")
    h, B, layer = r.h, r.B, 3
    x, _, w, b, n_in, n_out, _, _ = _links(r, layer)
    C, ho = geom(layer, r.W)[1], geom(layer, r.W)[2]
    y, part = _empty(n_out), _empty(h.op_bn_partial_floats(layer, B))
    scratch = _empty(h.op_scratch_floats(B))
    h.op_conv_fwd(layer, B, x, w, b, y, part, scratch)
    torch.cuda.synchronize()
    tpp = h.op_conv_tiles_per_partial(layer, B)
    gamma, beta, da = _rand(900, C, lo=0.5, hi=1.5), _rand(901, C, lo=-0.5, hi=0.5), _randn(902, n_out // 4)
    stats0 = torch.cat((_rand(903, C, lo=-0.3, hi=0.3), _rand(904, C, lo=0.5, hi=1.5)))
    o = dict(stats=_empty(2 * C), stats2=_empty(2 * C), coef=_empty(4 * C), coef2=_empty(4 * C), a=_empty(n_out // 4), dy=_empty(n_out),
             dgamma=_empty(C), dbeta=_empty(C), dbias=_empty(C))
    assert ho % 2 == 0

    def fn():
        o["stats"].copy_(stats0)
        o["stats2"].copy_(stats0)
        h.op_bn_pool_act_fwd(layer, B, y, part, gamma, beta, o["stats"][:C], o["stats"][C:], o["coef"], o["a"], scratch, True)
        h.op_bn_fwd_finalize(layer, B, part, tpp, gamma, beta, o["stats2"][:C], o["stats2"][C:], o["coef2"], scratch, True)
        h.op_bn_pool_act_bwd(layer, B, y, o["a"], da, o["coef"], gamma, o["dy"], o["dgamma"], o["dbeta"], o["dbias"], scratch)
    return Built(fn, _named(**o), [scratch])


@scenario("op-msssim", "ops", ("cvae_op_msssim",))
def _op_msssim(H):
    h, B = H.handle(), 5
    a, b = _rand(910, B, 3, 64, 64), _rand(911, B, 3, 64, 64)
    ws = _empty(h.op_msssim_ws_floats(B))
    o = dict(scalars=_empty(16), d_img1=_empty(B, 3, 64, 64))
    return Built(lambda: h.op_msssim(B, a, b, ws, o["scalars"], o["d_img1"]), _named(**o), [ws])


@scenario("op-latent", "ops", ("cvae_op_fc_fwd", "cvae_op_fc_bwd", "cvae_op_decin_fwd", "cvae_op_decin_bwd"))
def _op_latent(H):
    h, B, K = H.handle(), 5, 4096
    flat, wfc, bfc = _randn(920, B, K, scale=0.5), _randn(921, K, 64, scale=0.02), _randn(922, 64, scale=0.1)
    eps, pred = _randn(923, B, 32), _rand(924, B, 1)
    wd, bd, dh = _randn(925, 33, K, scale=0.1), _randn(926, K, scale=0.1), _randn(927, B, K, scale=0.1)
    dmu, dlv = _randn(928, B, 32, scale=0.01), _randn(929, B, 32, scale=0.01)
    o = dict(mu=_empty(B, 32), logvar=_empty(B, 32), zcat=_empty(B, 33), h=_empty(B, K), dwd=_empty(33, K), dbd=_empty(K), dzcat=_empty(B, 33),
             dwfc=_empty(K, 64), dbfc=_empty(64), dflat=_empty(B, K))
    scratch = _empty(h.op_latent_scratch_floats(B))

    def fn():
        h.op_fc_fwd(B, flat, wfc, bfc, eps, pred, o["mu"], o["logvar"], o["zcat"], scratch)
        h.op_decin_fwd(B, o["zcat"], wd, bd, o["h"])
        h.op_decin_bwd(B, o["zcat"], dh, wd, o["dwd"], o["dbd"], o["dzcat"], scratch)
        h.op_fc_bwd(B, flat, wfc, o["dzcat"], eps, o["logvar"], dmu, dlv, o["dwfc"], o["dbfc"], o["dflat"], scratch)
    return Built(fn, _named(**o), [scratch])


# ---- the Python layers ----
TRAINER_ENTRIES = ("cvae_forward", "cvae_loss", "cvae_backward", "cvae_grad_stats", "cvae_adam_step_guarded_opt", "cvae_trace_push",
                   "cvae_tensor_stats")


def _snapshots(pairs):
    """[(tensor, clone)] -> a function that copies every clone back, on the current stream."""
    saved = [(t, t.clone()) for t in pairs]

    def restore():
        for t, c in saved:
            t.copy_(c)
    return restore


def _trainer_builder(precision):
    def build(H):
        import torch
        from critic_vae_amd import synth
        from critic_vae_amd.nets import VariationalAutoencoder
        from critic_vae_amd.optim import Optim
        from critic_vae_amd.trace import Trace
        from critic_vae_amd.train import FusedTrainer
        B, W = 5, 64
        vae = VariationalAutoencoder(max_batch=B, seed=0, width=W, precision=precision, overlap_wgrad=False).cuda()
        vae.load_reference_params(synth.make_params(0, W))
        H.record(vae.handle)
        trace = Trace(capacity=4, every=1, tensors_every=1)
        tr = FusedTrainer(vae, optim=Optim("cosine", warmup=2, total=10, weight_decay=0.01, ema=0.99), skip_nonfinite=True,
                          max_grad_norm=1.0, trace=trace)
        x, pred, eps = (torch.from_numpy(a).cuda() for a in synth.make_batch(11, 0, B, W))
        tr.step(x, pred, eps)                      # creates the guard state, the averages and the trace's rings
        torch.cuda.synchronize()
        theta = vae.theta.data
        state = dict(theta=theta, bn_state=vae.bn_state, m=tr.m, v=tr.v, ema=tr.ema, aux_ema=tr.aux_ema, guard=tr.guard)
        restore = _snapshots(list(state.values()))
        nbt = vae.num_batches_tracked

        def fn():
            restore()
            tr.step_count, vae.num_batches_tracked = 1, nbt
            tr.step(x, pred, eps)
        outs = _named(scalars=tr.scalars, grads=tr.grads, mu=tr.mu, logvar=tr.logvar, recon=tr.recon, ring=trace._ring, tensor_ring=trace._tring,
                      **state)
        return Built(fn, outs, [tr.ws, tr.d_recon, tr.d_mu, tr.d_logvar, trace._scratch])
    return build


for _p in ("f32", "bf16"):
    scenario(f"fused-trainer-step-{_p}", "python", TRAINER_ENTRIES)(_trainer_builder(_p))


@scenario("critic-trainer-step", "python", ("cvae_critic_grad", "cvae_adam_step"))
def _critic_trainer(H):
    import torch
    from critic_vae_amd import lib as cvlib
    from critic_vae_amd.critic import Critic
    from critic_vae_amd.critic_train import CriticTrainer
    B = 5
    h = H.handle(64, 8)
    critic = Critic(handle=h).to("cuda")
    critic.flat.copy_(_randn(1000, critic.flat.numel(), scale=0.1))
    tr = CriticTrainer(critic)
    x, target = _rand(1001, B, 3, 64, 64), _rand(1002, B)
    keep = (_rand(1003, B, cvlib.CRITIC_KEEP) >= 0.3).to(torch.uint8)
    tr.step(x, target, keep=keep)
    torch.cuda.synchronize()
    state = dict(theta=tr.theta, m=tr.m, v=tr.v)
    restore = _snapshots(list(state.values()))

    def fn():
        restore()
        tr.step_count = 1
        tr.step(x, target, keep=keep)
    return Built(fn, _named(scalars=tr.scalars, grads=tr.grads, pred=tr._pred, **state), [tr._scratch])


@scenario("frame-feeder-handoff", "python", ("cvae_preprocess_u8",))
def _feeder(H):
    import numpy as np
    from critic_vae_amd.feeder import FrameFeeder
    B = 5
    h = H.handle(64, 8)
    frames = np.random.default_rng(1100).integers(0, 256, (12, 64, 64, 3), dtype=np.uint8)
    feeder = FrameFeeder(frames, B, "cuda:0", h, critic=None)
    assert feeder.copy_stream != H.stream, "the feeder's copy stream must be a third stream"
    order = [np.arange(0, 5), np.arange(6, 11)]
    outs = [_empty(B, 3, 64, 64) for _ in order]

    def fn():
        for o, (x, _) in zip(outs, feeder.batches(order)):
            o.copy_(x)
    return Built(fn, [(f"x{i}", o) for i, o in enumerate(outs)], list(feeder.x))


# ---------------------------------------------------------------------------------------------------------------------------------------
# running a group (the worker)
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_group(group):
    """Every scenario of `group`, in registry order -> the JSON-able record.  An exception that is not a library refusal or a failed
    assertion of a builder ends the group: whatever raised it may have faulted the device, and nothing more is started."""
    from critic_vae_amd.lib import CvaeError
    H = Harness()
    res = dict(group=group, control=H.control, independent=H.independent, blocker=H.blocker_kind, scenarios={}, stopped=None)
    for sc in SCENARIOS:
        if sc.group != group:
            continue
        try:
            built = sc.build(H)
            H.torch.cuda.synchronize()
            res["scenarios"][sc.name] = H.run(sc, built)
        except (CvaeError, AssertionError):
            res["scenarios"][sc.name] = dict(name=sc.name, error=traceback.format_exc())
            H.torch.cuda.synchronize()
        except Exception:                                        # noqa: BLE001
            res["scenarios"][sc.name] = dict(name=sc.name, error=traceback.format_exc())
            res["stopped"] = sc.name
            break
    return res


# ---------------------------------------------------------------------------------------------------------------------------------------
# two threads, two handles
# ---------------------------------------------------------------------------------------------------------------------------------------
THREAD_STEPS = 20
THREAD_CASES = (("f32", True), ("bf16x9", False))       # (precision, probe armed)
PROBE_ID = 2                                            # kind 0 (forward), conv layer 2


class _ThreadRun:
    """20 steps at 64 x 64, B = 5 through the Handle calls on one handle with its own buffers."""

    def __init__(self, precision, probe):
        import torch
        from critic_vae_amd import synth
        from critic_vae_amd.nets import VariationalAutoencoder
        B, W = 5, 64
        self.B, self.probe = B, probe
        vae = VariationalAutoencoder(max_batch=B, seed=0, width=W, precision=precision, overlap_wgrad=False).cuda()
        vae.load_reference_params(synth.make_params(0, W))
        self.vae, self.h = vae, vae.handle
        self.theta, self.bn = vae.theta.data, vae.bn_state
        self.ws = vae._workspace(B)
        self.mu, self.logvar, self.d_mu, self.d_logvar = (_empty(B, 32) for _ in range(4))
        self.recon, self.d_recon = _empty(B, 3, W, W), _empty(B, 3, W, W)
        self.scalars, self.losses = _empty(16), _empty(THREAD_STEPS, 16)
        self.grads = torch.zeros_like(self.theta)
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.batches = [tuple(torch.from_numpy(a).cuda() for a in synth.make_batch(11, s, B, W)) for s in range(THREAD_STEPS)]
        self.errors = []
        self.probe_count = 0
        torch.cuda.synchronize()

    def steps(self, stream, barrier=None, refuse_at=None):
        import torch
        from critic_vae_amd.lib import CvaeError
        h, B = self.h, self.B
        if barrier is not None:
            barrier.wait()
        with torch.cuda.stream(stream):
            if self.probe:
                h.probe_config([PROBE_ID])
            for s, (x, pred, eps) in enumerate(self.batches):
                if s == refuse_at:
                    try:                   # a batch above max_batch: refused before any device access
                        h.forward(B + 1, x, pred, eps, self.theta, self.bn, self.mu, self.logvar, self.recon, self.ws, train=True)
                        self.errors.append("a batch above max_batch was not refused")
                    except CvaeError:
                        pass
                h.forward(B, x, pred, eps, self.theta, self.bn, self.mu, self.logvar, self.recon, self.ws, train=True)
                h.loss(B, x, self.mu, self.logvar, self.recon, self.ws, self.scalars, self.d_recon, self.d_mu, self.d_logvar)
                h.backward(B, x, pred, eps, self.theta, self.logvar, self.recon, self.d_recon, self.d_mu, self.d_logvar, self.ws, self.grads)
                h.adam_step(self.theta, self.grads, self.m, self.v, s + 1, 1e-3)
                self.losses[s].copy_(self.scalars)
            self.last_error = h.lib.cvae_last_error().decode()
            stream.synchronize()
            if self.probe:
                self.probe_count = len(h.probe_read(PROBE_ID))
                h.probe_config([])

    def result(self):
        return dict(theta=self.theta, m=self.m, v=self.v, bn_state=self.bn, losses=self.losses)


def run_threads():
    """Both handles alone, one after the other, then the same 20 steps from two threads released together."""
    import threading
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    alone = []
    for precision, probe in THREAD_CASES:
        r = _ThreadRun(precision, probe)
        r.steps(torch.cuda.Stream())
        torch.cuda.synchronize()
        alone.append({k: raw(t).cpu() for k, t in r.result().items()})
    runs = [_ThreadRun(precision, probe) for precision, probe in THREAD_CASES]
    streams = [torch.cuda.Stream() for _ in runs]
    barrier = threading.Barrier(len(runs))
    raised = [None] * len(runs)

    def work(i):
        try:
            runs[i].steps(streams[i], barrier, refuse_at=10 if i == 1 else None)
        except BaseException:                                    # noqa: BLE001 -- reported, the other thread goes on
            raised[i] = traceback.format_exc()
            barrier.abort()
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(runs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    res = dict(cases=[list(c) for c in THREAD_CASES], steps=THREAD_STEPS, threads=[])
    for i, r in enumerate(runs):
        differs = [k for k, t in r.result().items() if not torch.equal(raw(t).cpu(), alone[i][k])] if raised[i] is None else None
        res["threads"].append(dict(precision=THREAD_CASES[i][0], raised=raised[i], differs=differs, errors=r.errors,
                                   last_error=getattr(r, "last_error", None), probe_count=r.probe_count))
        print(f"stream-threads {THREAD_CASES[i][0]}: differs from the run alone: {differs}, last error {getattr(r, 'last_error', None)!r}, "
              f"probe records {r.probe_count}")
    return res
