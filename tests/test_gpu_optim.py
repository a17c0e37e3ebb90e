"""The optimizer options on the GPU: cvae_adam_step_opt / cvae_adam_step_guarded_opt against the project's own plain Adam
kernel (bit for bit: same bits without options, the decay mask exactly), against torch.optim.AdamW, the EMA against its fp64
value, the guarded skip; then both trainers under an optim.Optim — nothing moves without one, the critic's decayed tensors, the
schedule, resume in the middle of a schedule, evaluation and files of the averaged weights.

Sizes: 4 | 1028 = one workgroup's stride plus one float4 | 2 097 152 + 1028 = one float4 row past the launcher's cap of 2 048
workgroups, so that the grid-stride loop takes a second trip."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from critic_vae_amd import critic_train as CT
from critic_vae_amd import episodes as E
from critic_vae_amd import lib as cvlib
from critic_vae_amd import train as T
from critic_vae_amd.critic import CRITIC_KEYS, Critic
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
WRAP = 2048 * 256 * 4                        # 2 097 152: the first element of the grid-stride loop's second trip
SIZES = [4, 1028, WRAP + 1028]
LR, B1, B2, EPS = 5e-5, 0.9, 0.999, 1e-8
DECAY = 0.75                                 # a decay_mul no test can mistake for 1


def optim_module():
    try:
        from critic_vae_amd import optim
    except ImportError as e:
        pytest.fail(f"critic_vae_amd.optim is missing ({e}): no LR schedule, weight decay or EMA")
    return optim


def opt_entry(H, name):
    if not hasattr(H, name):
        pytest.fail(f"the library binding has no {name}: the optimizer options (cvae_adam_step_opt / cvae_adam_step_guarded_opt) are missing")
    return getattr(H, name)


def opt_trainer(cls, model, **kw):
    try:
        return cls(model, **kw)
    except TypeError as e:
        pytest.fail(f"{cls.__name__} takes no optim ({e}): the optimizer is the reference's fixed recipe")


@pytest.fixture(scope="module")
def H():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return cvlib.Handle(64, 4)


@functools.lru_cache(maxsize=None)
def buffers(n):
    """p, g, m, v (and a starting EMA) from torch.rand, on the device; never modified: every test works on clones."""
    gen = torch.Generator().manual_seed(n % 9973 + 1)
    p, g, m, v, e = (torch.rand(n, generator=gen) for _ in range(5))
    return tuple(t.to(DEV) for t in (p, (g - 0.5) * 2e-2, (m - 0.5) * 1e-2, v * 1e-4, e))


def clones(n):
    return [t.clone() for t in buffers(n)]


def ranges_for(n, which):
    table = {"one": [(1, 2)], "six": [(3, 9)], "edge": [(1023, 1025)], "tail": [(n - 3, n)], "wrap": [(WRAP - 5, WRAP + 3)],
             "sixteen": [(3 * k + (k * k) % 3, 3 * k + 2 + (k % 2)) for k in range(16)], "none": []}[which]
    return [(b, e) for b, e in table if 0 <= b < e <= n]


KINDS = ("one", "six", "edge", "tail", "wrap", "sixteen", "none")
FULL = {"one": 1, "six": 1, "edge": 1, "tail": 1, "wrap": 1, "sixteen": 16, "none": 0}
# every (n, table) at which the whole table fits into [0, n): n = 4 takes [1, 2), its tail and the empty table
MASK_CASES = [(n, k) for n in SIZES for k in KINDS if len(ranges_for(n, k)) == FULL[k]]


def mask_of(n, ranges):
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    for b, e in ranges:
        mask[b:e] = True
    return mask


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. the same bits as the plain kernels ----
@pytest.mark.parametrize("n", SIZES)
def test_no_option_gives_adam_step_bits(H, n):
    step_opt = opt_entry(H, "adam_step_opt")
    p, g, m, v, _ = clones(n)
    q, _, mq, vq, _ = clones(n)
    for t in range(1, 4):
        H.adam_step(p, g, m, v, t, LR, B1, B2, EPS, grad_scale=0.5)
        step_opt(q, g, mq, vq, t, LR, B1, B2, EPS, grad_scale=0.5, opt=cvlib.opt_args(1.0, 0.0, []))
    torch.cuda.synchronize()
    assert same(p, q) and same(m, mq) and same(v, vq)


@pytest.mark.parametrize("n", SIZES)
def test_no_option_gives_adam_step_guarded_bits(H, n):
    step_opt = opt_entry(H, "adam_step_guarded_opt")
    p, g, m, v, _ = clones(n)
    q, _, mq, vq, _ = clones(n)
    s1, s2 = H.guard_state(g.device), H.guard_state(g.device)
    for t in range(3):
        gt = g * (t + 1)
        H.grad_stats(gt, s1, 0.5, 1.0, True, LR, B1, B2)
        H.adam_step_guarded(p, gt, m, v, s1, EPS)
        H.grad_stats(gt, s2, 0.5, 1.0, True, LR, B1, B2)
        step_opt(q, gt, mq, vq, s2, EPS, opt=cvlib.opt_args(1.0, 0.0, []))
    torch.cuda.synchronize()
    assert same(p, q) and same(m, mq) and same(v, vq)
    assert bytes(H.guard_record(s1)) == bytes(H.guard_record(s2)) and H.guard_record(s2).t == 3


# ---- 2. the decay mask, exactly ----
@pytest.mark.parametrize("n, which", MASK_CASES)
def test_decay_mask_is_exact(H, n, which):
    """Reference: the plain kernel on a copy whose masked elements were multiplied by decay_mul with one torch fp32 product."""
    step_opt = opt_entry(H, "adam_step_opt")
    ranges = ranges_for(n, which)
    assert len(ranges) == FULL[which]
    p, g, m, v, _ = clones(n)
    q, _, mq, vq, _ = clones(n)
    mask = mask_of(n, ranges)
    p[mask] = p[mask] * torch.tensor(DECAY, dtype=torch.float32, device=DEV)
    H.adam_step(p, g, m, v, 2, LR, B1, B2, EPS)
    step_opt(q, g, mq, vq, 2, LR, B1, B2, EPS, opt=cvlib.opt_args(DECAY, 0.0, ranges))
    torch.cuda.synchronize()
    wrong = (p.view(torch.int32) != q.view(torch.int32)).nonzero().flatten()[:8].tolist()
    assert same(p, q), f"{which} on n = {n}: params differ at elements {wrong}"
    assert same(m, mq) and same(v, vq)
    if which == "none":
        plain = clones(n)
        H.adam_step(plain[0], g, plain[2], plain[3], 2, LR, B1, B2, EPS)
        assert same(q, plain[0]), "an empty table decayed something"


@pytest.mark.parametrize("n", SIZES)
def test_decay_mask_is_exact_in_the_guarded_form(H, n):
    step_opt = opt_entry(H, "adam_step_guarded_opt")
    ranges = [r for k in ("one", "six", "edge", "tail", "wrap") for r in ranges_for(n, k)]
    ranges = sorted(set(ranges))
    ranges = [r for i, r in enumerate(ranges) if i == 0 or r[0] >= ranges[i - 1][1]]
    p, g, m, v, _ = clones(n)
    q, _, mq, vq, _ = clones(n)
    mask = mask_of(n, ranges)
    s1, s2 = H.guard_state(g.device), H.guard_state(g.device)
    p[mask] = p[mask] * torch.tensor(DECAY, dtype=torch.float32, device=DEV)
    H.grad_stats(g, s1, 1.0, 0.5, True, LR, B1, B2)
    H.adam_step_guarded(p, g, m, v, s1, EPS)
    H.grad_stats(g, s2, 1.0, 0.5, True, LR, B1, B2)
    step_opt(q, g, mq, vq, s2, EPS, opt=cvlib.opt_args(DECAY, 0.0, ranges))
    torch.cuda.synchronize()
    assert same(p, q) and same(m, mq) and same(v, vq)


# ---- 3. against torch.optim.AdamW ----
def test_adamw_matches_torch(H):
    """torch.optim.AdamW on the CPU, two parameter groups (decayed / weight_decay = 0), 5 steps, the magnitudes and the 1e-7
    of test_adam_matches_torch (tests/test_gpu_ops.py)."""
    from test_gpu_ops import check, dev, rnd
    step_opt = opt_entry(H, "adam_step_opt")
    n, cut, wd, lr = 4096, 1026, 0.1, 5e-5
    p0, g = rnd("ap", (n,)), rnd("ag", (n,), -1e-2, 1e-2)
    a, b = p0[:cut].clone().requires_grad_(True), p0[cut:].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [a], "weight_decay": wd}, {"params": [b], "weight_decay": 0.0}], lr=lr)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    args = optim_module().Optim(weight_decay=wd).args_at(0, lr, [(0, cut)])
    for step in range(1, 6):
        gs = g * step
        a.grad, b.grad = gs[:cut].clone(), gs[cut:].clone()
        opt.step()
        step_opt(p, dev(gs * 2.0), m, v, step, lr, grad_scale=0.5, opt=args)
    torch.cuda.synchronize()
    want = torch.cat([a.detach(), b.detach()])
    print("adamw max |err|", (p.cpu().double() - want.double()).abs().max().item())
    check(p, want, "adamw params", 1e-7)


# ---- 4. the EMA ----
def ema_bound(e_old, p_new, e_new, omd):
    want = e_old.double() + (p_new.double() - e_old.double()) * float(np.float32(omd))
    tol = 3 * 2.0 ** -24 * (e_old.double().abs() + p_new.double().abs())
    worst = ((e_new.double() - want).abs() - tol).max().item()
    return worst


@pytest.mark.parametrize("n", SIZES)
def test_ema_follows_the_written_params(H, n):
    step_opt = opt_entry(H, "adam_step_opt")
    omd = 0.0625 + 1e-3
    ranges = ranges_for(n, "six") + ranges_for(n, "edge")
    p, g, m, v, e = clones(n)
    q, _, mq, vq, e0 = clones(n)
    step_opt(p, g, m, v, 3, LR, B1, B2, EPS, opt=cvlib.opt_args(DECAY, omd, ranges), ema=e)
    step_opt(q, g, mq, vq, 3, LR, B1, B2, EPS, opt=cvlib.opt_args(DECAY, omd, ranges))
    torch.cuda.synchronize()
    assert same(p, q) and same(m, mq) and same(v, vq), "p, m, v depend on whether an EMA is kept"
    assert not same(e, e0)
    worst = ema_bound(e0, p, e, omd)
    print(f"n = {n}: EMA error minus bound {worst:.3e}")
    assert worst <= 0.0
    keep = e.clone()
    step_opt(p, g, m, v, 4, LR, B1, B2, EPS, opt=cvlib.opt_args(DECAY, 0.0, ranges), ema=e)       # ema_omd = 0: e keeps its bits
    torch.cuda.synchronize()
    assert same(e, keep) and not same(p, q)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("n_aux", [1, 3, 960, 4096])
def test_aux_ema(H, n_aux, guarded):
    n, omd = 1028, 0.37
    gen = torch.Generator().manual_seed(n_aux)
    aux = torch.rand(n_aux + 1, generator=gen).to(DEV)[1:]           # off the 16-byte grid: no float4 is assumed
    ae = torch.rand(n_aux + 9, generator=gen).to(DEV)
    aux0, ae0 = aux.clone(), ae.clone()
    p, g, m, v, e = clones(n)
    q, _, mq, vq, e0 = clones(n)
    if guarded:
        step_opt = opt_entry(H, "adam_step_guarded_opt")
        st = H.guard_state(g.device)
        H.grad_stats(g, st, 1.0, float("inf"), True, LR, B1, B2)
        step_opt(p, g, m, v, st, EPS, opt=cvlib.opt_args(1.0, omd, []), ema=e, aux=aux.contiguous(), aux_ema=ae[:n_aux], n_aux=n_aux)
        st = H.guard_state(g.device)
        H.grad_stats(g, st, 1.0, float("inf"), True, LR, B1, B2)
        step_opt(q, g, mq, vq, st, EPS, opt=cvlib.opt_args(1.0, omd, []), ema=e0.clone(), n_aux=0)
    else:
        step_opt = opt_entry(H, "adam_step_opt")
        step_opt(p, g, m, v, 1, LR, B1, B2, EPS, opt=cvlib.opt_args(1.0, omd, []), ema=e, aux=aux.contiguous(), aux_ema=ae[:n_aux], n_aux=n_aux)
        step_opt(q, g, mq, vq, 1, LR, B1, B2, EPS, opt=cvlib.opt_args(1.0, omd, []), ema=e0.clone(), n_aux=0)      # null aux pointers
    torch.cuda.synchronize()
    assert same(aux, aux0), "aux is read only"
    assert same(ae[n_aux:], ae0[n_aux:]), "aux_ema was written past n_aux"
    assert ema_bound(ae0[:n_aux], aux0, ae[:n_aux], omd) <= 0.0 and not same(ae[:n_aux], ae0[:n_aux])
    assert same(p, q) and same(m, mq) and same(v, vq) and ema_bound(e0, p, e, omd) <= 0.0


# ---- 5. the guarded skip ----
def test_guarded_skip_writes_nothing_and_the_next_step_writes_all(H):
    step_opt = opt_entry(H, "adam_step_guarded_opt")
    n, n_aux = WRAP + 1028, 960
    p, g, m, v, e = clones(n)
    aux, ae = torch.rand(n_aux, device=DEV), torch.rand(n_aux, device=DEV)
    before = [t.clone() for t in (p, m, v, e, ae)]
    bad = g.clone()
    bad[WRAP + 7] = float("nan")
    st = H.guard_state(g.device)
    args = cvlib.opt_args(DECAY, 0.25, ranges_for(n, "six") + ranges_for(n, "wrap"))
    H.grad_stats(bad, st, 1.0, 1.0, True, LR, B1, B2)
    step_opt(p, bad, m, v, st, EPS, opt=args, ema=e, aux=aux, aux_ema=ae)
    torch.cuda.synchronize()
    rec = H.guard_record(st)
    assert (rec.apply, rec.skipped, rec.t) == (0, 1, 0)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema", "aux_ema"), before, (p, m, v, e, ae)):
        assert same(a, b), f"a skipped step wrote {name}"
    H.grad_stats(g, st, 1.0, 1.0, True, LR, B1, B2)
    step_opt(p, g, m, v, st, EPS, opt=args, ema=e, aux=aux, aux_ema=ae)
    torch.cuda.synchronize()
    rec = H.guard_record(st)
    assert (rec.apply, rec.skipped, rec.t) == (1, 1, 1)
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema", "aux_ema"), before, (p, m, v, e, ae)):
        assert not same(a, b), f"the applied step left {name} alone"
    assert torch.isfinite(p).all() and torch.isfinite(e).all()


# ---- the trainers ----
B = 4


@functools.lru_cache(maxsize=None)
def real_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))


@functools.lru_cache(maxsize=None)
def batch(s):
    """Real frames s * B .. (s + 1) * B of step_real_b68.npz with their critic values, eps from a seeded generator (noise
    frames against an untrained decoder give a NaN loss after one step: two NaN runs would be 'equal' whatever ran)."""
    fx = real_fixture()
    x = torch.from_numpy(fx["u8"][s * B:(s + 1) * B].copy()).permute(0, 3, 1, 2).float().div(255.0).contiguous()
    pred = torch.from_numpy(fx["pred"][s * B:(s + 1) * B].copy()).float().reshape(B, 1)
    eps = torch.randn(B, 32, generator=torch.Generator().manual_seed(100 + s))
    return x.to(DEV), pred.to(DEV), eps.to(DEV)


def vae_trainer(precision="f32", seed=None, **kw):
    """seed None: the weights the real-frames fixtures train from (test_gpu_step: the loss stays finite); else fresh ones."""
    from test_oracle import real_frames_params
    fx = real_fixture()
    vae = VariationalAutoencoder(max_batch=B, seed=int(fx["wseed"]) if seed is None else seed, precision=precision).to(DEV)
    if seed is None:
        vae.load_reference_params(real_frames_params(fx))
    return opt_trainer(FusedTrainer, vae, **kw) if "optim" in kw else FusedTrainer(vae, **kw)


def run(tr, steps):
    for s in steps:
        tr.step(*batch(s))
    torch.cuda.synchronize()
    assert torch.isfinite(tr.vae.theta.data).all() and torch.isfinite(tr.vae.bn_state).all(), "the run itself went non-finite"
    return tr


def vae_state(tr):
    return [tr.vae.theta.data, tr.m, tr.v, tr.vae.bn_state]


@functools.lru_cache(maxsize=None)
def critic_fixture():
    ck = np.load(os.path.join(ROOT, "tests", "golden", "critic_real_b8.npz"))
    u8 = np.load(os.path.join(ROOT, "tests", "golden", "step_real_b68.npz"))["u8"]
    w = {k: torch.from_numpy(np.asarray(ck["w/" + k])) for k, _ in CRITIC_KEYS}
    x = torch.from_numpy(u8[:4 * B]).to(DEV).permute(0, 3, 1, 2).float().div(255.0).contiguous()
    target = torch.linspace(0.1, 0.9, 4 * B, device=DEV)
    keep = (torch.rand(4 * B, cvlib.CRITIC_KEEP, generator=torch.Generator().manual_seed(2)) >= 0.3).to(torch.uint8).to(DEV)
    return cvlib.Handle(64, 16), w, x, target, keep, torch.from_numpy(u8).to(DEV)


def critic_trainer(**kw):
    h, w, *_ = critic_fixture()
    critic = Critic(handle=h).to(DEV)
    critic.load_state_dict(w)
    return opt_trainer(CT.CriticTrainer, critic, **kw) if "optim" in kw else CT.CriticTrainer(critic, **kw)


def critic_run(tr, steps):
    _, _, x, target, keep, _ = critic_fixture()
    for s in steps:
        tr.step(x[s * B:(s + 1) * B], target[s * B:(s + 1) * B], keep=keep[s * B:(s + 1) * B].contiguous())
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_vae_trainer_without_the_option_is_unchanged(precision):
    a = run(vae_trainer(precision), range(3))
    b = run(vae_trainer(precision, optim=None), range(3))
    assert b.optim is None and b.ema is None
    assert all(same(s, t) for s, t in zip(vae_state(a), vae_state(b)))
    c = run(vae_trainer(precision, optim=optim_module().Optim()), range(3))      # the _opt kernel with nothing to do: the same bits
    assert all(same(s, t) for s, t in zip(vae_state(a), vae_state(c)))


def test_critic_trainer_without_the_option_is_unchanged():
    a, b = critic_run(critic_trainer(), range(3)), critic_run(critic_trainer(optim=None), range(3))
    assert all(same(s, t) for s, t in zip((a.theta, a.m, a.v), (b.theta, b.m, b.v)))


def test_critic_decay_touches_the_seven_weight_tensors_only():
    O = optim_module()
    wd, lr = 50.0, 1e-3
    plain, decayed = critic_trainer(lr=lr), critic_trainer(lr=lr, optim=O.Optim(weight_decay=wd))
    theta0 = plain.theta.clone()
    critic_run(plain, [0])
    critic_run(decayed, [0])
    assert same(plain.grads, decayed.grads)
    ranges = O.decay_ranges(O.critic_layout())
    assert len(ranges) == 7 and ranges == decayed.decay_ranges
    mask = mask_of(theta0.numel(), ranges)
    mul = O.Optim(weight_decay=wd).args_at(0, lr)["decay_mul"]
    assert 0.9 < mul < 0.96
    ref = theta0.clone()
    ref[mask] = ref[mask] * torch.tensor(mul, dtype=torch.float32, device=DEV)
    m, v = torch.zeros_like(ref), torch.zeros_like(ref)
    plain.h.adam_step(ref, plain.grads, m, v, 1, lr, B1, B2, plain.eps)
    torch.cuda.synchronize()
    assert same(ref, decayed.theta) and same(m, decayed.m) and same(v, decayed.v)
    assert same(decayed.theta[~mask], plain.theta[~mask]), "a bias (or the padding) was decayed"
    assert not same(decayed.theta[mask], plain.theta[mask])
    assert (decayed.theta[-3:] == 0).all()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_schedule_equals_setting_lr_by_hand(precision):
    O = optim_module()
    lr = 2e-4
    sched = O.Optim(schedule="cosine", warmup=2, total=4, lr_min=1e-5, weight_decay=0.05, ema=0.9)
    a = run(vae_trainer(precision, lr=lr, optim=sched), range(4))
    b = vae_trainer(precision, lr=lr, optim=O.Optim(weight_decay=0.05, ema=0.9))
    rates = [sched.lr_at(s, lr) for s in range(4)]
    assert rates[1] == lr and rates[2] == lr and rates[0] == lr / 2 and 1e-5 < rates[3] < lr
    for s in range(4):
        b.lr = rates[s]
        run(b, [s])
    for name, x, y in zip(("theta", "m", "v", "bn_state", "ema", "aux_ema"), vae_state(a) + [a.ema, a.aux_ema], vae_state(b) + [b.ema, b.aux_ema]):
        assert same(x, y), name
    plain = run(vae_trainer(precision, lr=lr), range(4))
    assert not same(plain.vae.theta.data, a.vae.theta.data)


@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_resume_in_the_middle_of_a_schedule(precision, guarded, tmp_path):
    O = optim_module()
    kw = dict(lr=2e-4, optim=O.Optim(schedule="cosine", warmup=3, total=4, lr_min=1e-5, weight_decay=0.05, ema=0.9, ema_warmup=True))
    if guarded:
        kw.update(skip_nonfinite=True, max_grad_norm=1.0)
    whole = run(vae_trainer(precision, **kw), range(4))
    first = run(vae_trainer(precision, **kw), range(2))
    T.save_networks(first.vae, str(tmp_path))
    path = T.save_trainer(first, str(tmp_path / "trainer.pt"))
    kw2 = dict(kw, optim=None)                                               # the state's options are what continues
    second = vae_trainer(precision, seed=5, **kw2)
    T.load_networks(second.vae, str(tmp_path))
    T.load_trainer(second, path)
    assert second.optim == kw["optim"] and same(second.ema, first.ema) and same(second.aux_ema, first.aux_ema)
    run(second, range(2, 4))
    for name, x, y in zip(("theta", "m", "v", "bn_state", "ema", "aux_ema"), vae_state(whole) + [whole.ema, whole.aux_ema],
                          vae_state(second) + [second.ema, second.aux_ema]):
        assert same(x, y), name
    assert not same(whole.ema, whole.vae.theta.data) and not same(whole.aux_ema, whole.vae.bn_state)
    if guarded:
        assert whole.guard_stats()["applied"] == second.guard_stats()["applied"] == 4


def test_critic_resume_with_all_options():
    O = optim_module()
    kw = dict(lr=1e-3, skip_nonfinite=True, optim=O.Optim(schedule="linear", warmup=1, total=4, weight_decay=0.1, ema=0.8))
    whole = critic_run(critic_trainer(**kw), range(4))
    first = critic_run(critic_trainer(**kw), range(2))
    second = critic_trainer(**kw)
    second.load_state_dict(first.state_dict())
    critic_run(second, range(2, 4))
    for name in ("theta", "m", "v", "ema"):
        assert same(getattr(whole, name), getattr(second, name)), name
    assert whole.aux_ema is None and not same(whole.ema, whole.theta)


def small_dataset(lo, hi, traj=0):
    fx = real_fixture()
    n = hi - lo
    source = np.stack([np.full(n, traj, np.int64), np.arange(n, dtype=np.int64)], 1)
    return E.DeviceDataset(torch.from_numpy(fx["u8"][lo:hi].copy()).to(DEV), torch.from_numpy(fx["pred"][lo:hi].copy()).to(DEV), source)


def real_trainer(precision, **kw):
    return vae_trainer(precision, **kw)


def fit(tr, ds, **kw):
    np.random.seed(5)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    return tr.fit_device(ds, B, 1, generator=gen, **kw)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_evaluate_ema_and_the_saved_files(precision, tmp_path):
    O = optim_module()
    train, val = small_dataset(0, 12), small_dataset(12, 22, 1)
    kw = dict(optim=O.Optim(weight_decay=0.01, ema=0.5))
    plain, watched = real_trainer(precision, **kw), real_trainer(precision, **kw)
    fit(plain, train)
    fit(watched, train, val=val, val_every=2)
    torch.cuda.synchronize()
    assert torch.isfinite(plain.vae.theta.data).all(), "the run itself went non-finite"
    for name, x, y in zip(("theta", "m", "v", "bn_state", "ema", "aux_ema"), vae_state(plain) + [plain.ema, plain.aux_ema],
                          vae_state(watched) + [watched.ema, watched.aux_ema]):
        assert same(x, y), f"{name} differs once validation runs between the steps"
    assert [t for t, _ in watched.val_history] == [2] and all(r["weights"] == "ema" for _, r in watched.val_history)
    assert not same(watched.ema, watched.vae.theta.data) and not same(watched.aux_ema, watched.vae.bn_state)
    # evaluate(ema=True) == evaluate of a trainer whose VAE holds the averaged theta and bn_state; nothing of the trainer moves
    before = [t.clone() for t in vae_state(watched) + [watched.ema, watched.aux_ema]]
    steps, nbt = watched.step_count, watched.vae.num_batches_tracked
    got, live = watched.evaluate(val, B, ema=True), watched.evaluate(val, B)
    assert all(same(a, b) for a, b in zip(before, vae_state(watched) + [watched.ema, watched.aux_ema]))
    assert (watched.step_count, watched.vae.num_batches_tracked) == (steps, nbt)
    other = real_trainer(precision)
    other.vae.theta.data.copy_(watched.ema)
    other.vae.bn_state.copy_(watched.aux_ema)
    want = other.evaluate(val, B)
    assert got == want and got != live
    # the files of the save path load through load_networks, and a batch through them is the EMA evaluation
    out = T.save_ema_networks(watched, str(tmp_path / "ema"))
    assert all(same(a, b) for a, b in zip(before, vae_state(watched) + [watched.ema, watched.aux_ema]))
    loaded = VariationalAutoencoder(max_batch=B, seed=3, precision=precision).to(DEV)
    T.load_networks(loaded, out)
    assert same(loaded.theta.data, watched.ema) and same(loaded.bn_state, watched.aux_ema)
    assert FusedTrainer(loaded).evaluate(val, B) == want
    with pytest.raises(ValueError, match="ema"):
        real_trainer(precision).evaluate(val, B, ema=True)
    live_only = real_trainer(precision, optim=O.Optim(weight_decay=0.01))
    fit(live_only, train, val=val)
    assert [r["weights"] for _, r in live_only.val_history] == ["live"]


def test_critic_evaluate_ema_and_its_checkpoint(tmp_path):
    O = optim_module()
    _, _, _, _, _, frames = critic_fixture()
    n = 24
    source = np.stack([np.zeros(n, np.int64), np.arange(n, dtype=np.int64)], 1)
    ds = E.DeviceDataset(frames[:n].contiguous(), torch.linspace(0.05, 0.95, n, device=DEV).reshape(n, 1), source)
    tr = critic_run(critic_trainer(lr=1e-3, optim=O.Optim(ema=0.5)), range(3))
    before = [t.clone() for t in (tr.theta, tr.m, tr.v, tr.ema)]
    got, live = tr.evaluate(ds, 16, ema=True), tr.evaluate(ds, 16)
    assert all(same(a, b) for a, b in zip(before, (tr.theta, tr.m, tr.v, tr.ema))) and tr.step_count == 3
    path = T._save_critic(tr.critic, str(tmp_path / "ema"), ema=tr)
    other = Critic(handle=tr.h).to(DEV)
    other.load_state_dict(torch.load(path, map_location="cpu"))
    assert same(other.flat, tr.ema[:other.flat.numel()])
    want = CT.CriticTrainer(other).evaluate(ds, 16)
    for k in ("loss", "bce", "mse", "mae", "pearson", "worst", "frames"):
        assert got[k] == want[k] and (k == "frames" or got[k] != live[k]), k
    assert np.array_equal(got["confusion"], want["confusion"])


def test_reading_the_averages_before_the_first_step_keeps_nothing(tmp_path):
    """evaluate(ema=True) and the save paths on a trainer that has not stepped work on temporaries: the averages are still
    created by the first update, from the parameters as they stand THEN — a load_networks in between cannot leave them stale."""
    O = optim_module()
    val = small_dataset(12, 20, 1)
    tr = vae_trainer(optim=O.Optim(ema=0.5))
    early = tr.evaluate(val, B, ema=True)
    T.save_ema_networks(tr, str(tmp_path / "ema"))
    assert tr.ema is None and tr.aux_ema is None and early == tr.evaluate(val, B)
    donor = run(vae_trainer(), range(1))                                     # other weights arrive after the early evaluation
    T.save_networks(donor.vae, str(tmp_path / "nets"))
    T.load_networks(tr.vae, str(tmp_path / "nets"))
    theta0, bn0 = tr.vae.theta.data.clone(), tr.vae.bn_state.clone()
    run(tr, [1])
    want = theta0.double() + (tr.vae.theta.data.double() - theta0.double()) * 0.5
    assert (tr.ema.double() - want).abs().max().item() <= 3 * 2.0 ** -24 * (theta0.abs().max().item() + tr.vae.theta.data.abs().max().item())
    assert not same(bn0, tr.aux_ema)
    ct = critic_trainer(optim=O.Optim(ema=0.5))
    T._save_critic(ct.critic, str(tmp_path / "c"), ema=ct)
    assert ct.ema is None


def test_two_ranks_share_the_averaged_weights():
    """Both ranks on device 0 with gloo, as the project's other two-rank tests run (tests/optim_dp_worker.py)."""
    env = dict(os.environ, CVAE_DIST_BACKEND="gloo", CVAE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nnodes=1", "--nproc-per-node=2", os.path.join(ROOT, "tests", "optim_dp_worker.py")],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "OPTIM_DP_OK rank 0" in r.stdout and "OPTIM_DP_OK rank 1" in r.stdout
