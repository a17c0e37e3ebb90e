"""CPU: host-side logic that needs no GPU — the C-ABI library loads and exports every symbol
include/cvae.h declares, layout conversions are exact inverses, the DP path (gloo, 2 ranks)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from critic_vae_amd import layout as L
from critic_vae_amd import lib as cvlib
from critic_vae_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = cvlib.load()                       # raises if the .so is missing: no CPU fallback exists
    hdr = open(os.path.join(ROOT, "include", "cvae.h")).read()
    declared = set(re.findall(r"\b(cvae_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/cvae.h but not exported"
    assert set(cvlib.EXPORTS) <= declared
    assert b"gfx950" in lib.cvae_version()


def test_flat_layout_and_reference_round_trip():
    h = cvlib.Handle(64, 8)
    assert sum(n for _, n in h.layout.values()) == 2583971
    assert all(off % 64 == 0 for off, _ in h.layout.values())
    ref = {k: torch.from_numpy(v) for k, v in synth.make_params(3).items()}
    flat = L.ref_to_native(h.layout, h.param_total, ref)
    back = L.native_to_ref(h.layout, flat)
    assert set(back) == set(ref)
    for k in ref:
        assert back[k].shape == ref[k].shape and torch.equal(back[k], ref[k]), k
    # spot-check the permutations against their definitions
    w = ref["encoder.model.4.weight"]                                # (64, 32, 5, 5)
    off, _ = h.layout["enc1.w"]
    assert flat[off + ((2 * 5 + 3) * 32 + 7) * 64 + 11] == w[11, 7, 2, 3]
    off, _ = h.layout["fc.w"]
    c, hh, ww = 37, 2, 3
    k = (hh * 4 + ww) * 256 + c
    assert flat[off + k * 64 + 5] == ref["encoder.fc_mu.weight"][5, c * 16 + hh * 4 + ww]
    assert flat[off + k * 64 + 32 + 5] == ref["encoder.fc_var.weight"][5, c * 16 + hh * 4 + ww]
    off, _ = h.layout["decin.w"]
    assert flat[off + 32 * 4096 + k] == ref["decoder.decoder_input.weight"][c * 16 + hh * 4 + ww, 32]


def test_bad_arguments_return_errors_not_crashes():
    h = cvlib.Handle(64, 4)
    with pytest.raises(cvlib.CvaeError):
        cvlib.Handle(96, 4)                                          # unsupported width
    rc = h.lib.cvae_forward(h.h, 9, None, None, None, None, None, None, None, None, None, 1, None)
    assert rc != 0 and b"batch" in h.lib.cvae_last_error()
    assert h.workspace_bytes(4) > 0 and h.workspace_bytes(4) % 4 == 0


# cvae_conv_route of every (precision, width) at B = 8, 256, 2048, edge - 1, edge (edge: the first batch whose larger tensor of the layer has 2^31
# bytes), one string per (layer, dgrad) = (1, 0) (1, 1) (2, 0) (2, 1) (3, 0) (3, 1): 0 per-tile, 1 two-workgroup persistent, 2 big-tile persistent
CONV_ROUTES = {
    (0, 64): ["11110", "00000", "11110", "11110", "11110", "11110"],
    (0, 128): ["11010", "00000", "11110", "11110", "00000", "00000"],
    (1, 64): ["22220"] * 6,
    (1, 128): ["22220"] * 6,
    (2, 64): ["00000"] * 6,
    (2, 128): ["00000"] * 6,
    (3, 64): ["00000"] * 6,
    (3, 128): ["00000"] * 6,
}
# the packed-frame row (layer 0, bf16 mode) at B = 8, 256, 1024, 2048, edge - 1, edge (edge: the first batch whose packed frame plus its
# descriptor bias, B * W * W * 8 + (2W + 2) * 8 bytes, reaches 2^31): 1 = E1 stages the packed bf16 frame, 0 = the fp32 frame
XP_EDGE = {64: 65536, 128: 16384}
XP_ROUTES = {64: "111110", 128: "111110"}


def test_persistent_conv_kernels_refuse_tensors_of_two_gib():
    """The persistent conv kernels (conv_bf16_big.hip, conv_bf16_ps.hip, conv_mfma_ps.hip) address their tensors with 32-bit byte offsets
    and buffer descriptors; their launchers must hand an activation of 2 GiB or more to the per-tile kernels (64-bit addressing).
    cvae_conv_route reads the route table the launchers read (conv_route, no device access): the family changes exactly where
    the larger of a layer's two tensors crosses 2^31 bytes.  The whole route table is pinned (CONV_ROUTES), and CVAE_CONV_PER_TILE=1 sends
    every pass to the per-tile kernels.  The packed bf16 frame of E1 (XP_ROUTES, layer 0 of bf16 mode; negative in every other mode) is
    addressed the same way and is left for the fp32 frame from the batch on whose descriptor reaches 2^31 bytes.  Child processes, so that no CVAE_* switch of the caller changes the routes."""
    code = """
import json, os, sys
sys.path.insert(0, %r)
from critic_vae_amd import lib as cvlib
lib = cvlib.load()
r = lib.cvae_conv_route
ch = {1: (32, 64), 2: (64, 128), 3: (128, 256)}
tab = {}
for prec in range(4):
    elt = 2 if prec == 1 else 4
    for width in (64, 128):
        row = []
        for layer in (1, 2, 3):
            H = (width // 2) >> (layer - 1)
            edge = (1 << 31) // (H * H * max(ch[layer]) * elt)          # first batch whose larger tensor has 2^31 bytes
            for dgrad in (0, 1):
                row.append("".join(str(r(prec, width, layer, dgrad, b)) for b in (8, 256, 2048, edge - 1, edge)))
                small, below, at = r(prec, width, layer, dgrad, 8), r(prec, width, layer, dgrad, edge - 1), r(prec, width, layer, dgrad, edge)
                assert small == below, (prec, width, layer, dgrad, small, below)
                assert at == 0 and r(prec, width, layer, dgrad, 4 * edge) == 0, (prec, width, layer, dgrad, at)
        tab["%%d,%%d" %% (prec, width)] = row
        for b in (8, 2048, (1 << 31) - 1):
            assert prec == 1 or (r(prec, width, 0, 0, b) < 0 and r(prec, width, 0, 1, b) < 0), (prec, width, b)
for width in (64, 128):
    edge = -(-((1 << 31) - (2 * width + 2) * 8) // (width * width * 8))
    tab["xp,%%d" %% width] = [edge, "".join(str(r(1, width, 0, 0, b)) for b in (8, 256, 1024, 2048, edge - 1, edge))]
    assert r(1, width, 0, 1, 8) < 0 and r(1, width, 0, 0, 4 * edge) == 0
if os.environ.get("CVAE_CONV_PER_TILE") != "1":
    # the default configuration does use them below the edge: fp32 E2..E4 forward on the two-workgroup kernel, bf16 E2..E4 (64 x 64) on the big-tile kernel
    assert [r(0, 64, l, 0, 256) for l in (1, 2, 3)] == [1, 1, 1] and r(0, 64, 1, 1, 256) == 0
    assert [r(1, 64, l, d, 2048) for l in (1, 2, 3) for d in (0, 1)] == [2] * 6 and r(1, 128, 1, 0, 1024) == 2 and r(1, 128, 1, 1, 1024) == 2
    assert r(1, 64, 1, 0, 16383) == 2 and r(1, 64, 1, 0, 16384) == 0 and r(0, 64, 1, 0, 8191) == 1 and r(0, 64, 1, 0, 8192) == 0
assert r(2, 64, 1, 0, 256) == 0 and r(1, 32, 1, 0, 8) < 0 and r(1, 64, 4, 0, 8) < 0 and r(1, 64, 1, 0, 0) < 0 and r(1, 64, 1, 0, 1 << 32) < 0
print(json.dumps(tab))
print("ok")
""" % ROOT
    want = {f"{p},{w}": row for (p, w), row in CONV_ROUTES.items()}
    xp = {f"xp,{w}": [XP_EDGE[w], XP_ROUTES[w]] for w in XP_EDGE}          # not a conv pass: CVAE_CONV_PER_TILE leaves it alone
    for per_tile in ("0", "1"):
        env = {k: v for k, v in os.environ.items() if not k.startswith("CVAE_")}
        if per_tile == "1":
            env["CVAE_CONV_PER_TILE"] = "1"
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
        got = json.loads(r.stdout.strip().splitlines()[-2])
        assert got == dict(want if per_tile == "0" else {k: ["00000"] * 6 for k in want}, **xp), (per_tile, got)


def test_latent_ops_refuse_bad_batches_and_null_scratch():
    """cvae_op_fc_fwd / decin_fwd / decin_bwd / fc_bwd and their scratch query: batch < 1, batch > max_batch or a null scratch is
    CVAE_EINVAL before anything is launched (the pointers here are not device memory)."""
    h = cvlib.Handle(64, 8)
    p = 0x1000
    for B in (0, -1, 9):
        assert h.lib.cvae_op_latent_scratch_floats(h.h, B) == -1
        assert h.lib.cvae_op_fc_fwd(h.h, B, *[p] * 9, None) == -1
        assert h.lib.cvae_op_decin_fwd(h.h, B, *[p] * 4, None) == -1
        assert h.lib.cvae_op_decin_bwd(h.h, B, *[p] * 7, None) == -1
        assert h.lib.cvae_op_fc_bwd(h.h, B, *[p] * 11, None) == -1
        assert b"batch" in h.lib.cvae_last_error()
    assert h.lib.cvae_op_fc_fwd(h.h, 8, *[p] * 8, None, None) == -1
    assert h.lib.cvae_op_decin_bwd(h.h, 8, *[p] * 6, None, None) == -1
    assert h.lib.cvae_op_fc_bwd(h.h, 8, *[p] * 10, None, None) == -1
    with pytest.raises(cvlib.CvaeError):
        h.op_latent_scratch_floats(9)
    # fc.hip: the larger of the FC_KS forward slabs and the decoder_input slabs, then dml and its column sums
    for B in (1, 8):
        assert h.op_latent_scratch_floats(B) >= max(32 * B * 64, 34 * 4096) + B * 64


@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("precision", ["f32", "bf16", "bf16x9", "bf16x6"])
def test_conv_ops_refuse_bad_handles_layers_batches_and_null_scratch(precision, W):
    """cvae_op_conv_fwd / dgrad / wgrad: a null handle, a layer outside the entry's range, batch < 1, batch > max_batch, or a null
    scratch on a pass whose row of the conv table uses scratch is CVAE_EINVAL before anything is launched, and the error string names
    the cause (the pointers here are not device memory; no call below is one that is accepted)."""
    h = cvlib.Handle(W, 8, precision=precision)
    lib, p = h.lib, 0x1000
    entries = [("cvae_op_conv_fwd", lib.cvae_op_conv_fwd, 5, range(0, 9)), ("cvae_op_conv_dgrad", lib.cvae_op_conv_dgrad, 4, range(1, 8)),
               ("cvae_op_conv_wgrad", lib.cvae_op_conv_wgrad, 4, range(0, 8))]

    def refused(name, fn, n_ptr, handle, layer, B, scratch, cause):
        assert fn(handle, layer, B, *[p] * n_ptr, scratch, None) == -1, (name, layer, B, scratch)
        err = lib.cvae_last_error().decode()
        assert name in err and cause in err, (name, layer, B, scratch, err)

    for name, fn, n_ptr, layers in entries:
        refused(name, fn, n_ptr, None, layers[0], 8, p, "null handle")
        for layer in layers:
            for B in (0, -1, 9):
                refused(name, fn, n_ptr, h.h, layer, B, p, f"batch {B} outside [1, 8]")
        for layer in (layers[0] - 1, layers[-1] + 1, 100):
            refused(name, fn, n_ptr, h.h, layer, 8, p, f"layer {layer} outside [{layers[0]}, {layers[-1]}]")
    # a null scratch: every weight gradient; forward and input gradient of every bf16 or emulated pass (layers 1..7 of a bf16 handle, 1..4
    # of the emulation modes), of every up-conv pass (layers 5..7) and of D0 at 64 x 64 in fp32
    fd_layers = {"f32": [5, 6, 7] + ([4] if W == 64 else []), "bf16": list(range(1, 8))}.get(precision, list(range(1, 8)))
    for name, fn, n_ptr, layers in entries:
        for layer in (layers if name == "cvae_op_conv_wgrad" else fd_layers):
            refused(name, fn, n_ptr, h.h, layer, 8, None, "null scratch")


def test_two_handles_do_not_share_state():
    """include/cvae.h: one handle per device / configuration, no global state."""
    a, b = cvlib.Handle(64, 4), cvlib.Handle(128, 2, precision="bf16")
    assert a.h.value != b.h.value
    assert a.layout["fc.w"][1] == 4096 * 64 and b.layout["fc.w"][1] == 16384 * 64
    wa = a.workspace_bytes(4)
    del b
    assert a.workspace_bytes(4) == wa and a.lib.cvae_param_count(a.h) == 30
    # the documented names are the library's native ones (include/cvae.h), not reference state_dict keys
    assert a.lib.cvae_param_name(a.h, 0) == b"enc0.w" and "decin.b" in a.layout


def test_bench_dump_outputs_float32_within_budget_and_repeatable(tmp_path):
    """bench.py --dump-outputs: every array of the timed path (loss scalars, mu, logvar, recon, each parameter and gradient,
    BatchNorm statistics) as float32 .npy, the total inside the budget (a fixed-seed sample when it would not fit), and the
    same files for the same state.  A child process: importing bench.py sets an environment default."""
    code = """
import os, sys
import numpy as np
sys.path.insert(0, %r)
import bench
from critic_vae_amd import synth
from critic_vae_amd.nets import VariationalAutoencoder
from critic_vae_amd.train import FusedTrainer
vae = VariationalAutoencoder(max_batch=8, seed=0)
tr = FusedTrainer(vae)
for t in (tr.scalars, tr.mu, tr.logvar, tr.recon, tr.grads):
    t.normal_()
for budget, sampled in ((bench.DUMP_BUDGET_BYTES, False), (400000, True)):
    a, b = (os.path.join(%r, f"{budget}_{i}") for i in (0, 1))
    info = bench.dump_outputs(a, tr, vae, budget_bytes=budget)
    bench.dump_outputs(b, tr, vae, budget_bytes=budget)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == info["arrays"] == 4 + 2 * len(synth.make_params(0)) + 8, names
    assert (info["sampled_to_elements"] is not None) == sampled
    arrs = [np.load(os.path.join(a, n)) for n in names]
    assert all(x.dtype == np.float32 for x in arrs) and sum(x.nbytes for x in arrs) <= budget
    assert all(np.array_equal(x, np.load(os.path.join(b, n))) for x, n in zip(arrs, names))
    if not sampled:
        assert np.array_equal(np.load(os.path.join(a, "recon.npy")), tr.recon.numpy())
print("ok")
""" % (ROOT, str(tmp_path))
    env = {k: v for k, v in os.environ.items() if not k.startswith("CVAE_")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]


def test_data_parallel_two_ranks_gloo():
    """N-rank all-reduced gradient == mean over ranks of the single-rank (oracle) gradient on that
    rank's shard, through the same flat native buffer the GPU path reduces."""
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
                        "--nnodes=1", "--nproc-per-node=2",           # --standalone: torchrun picks a free rendezvous port
                        os.path.join(ROOT, "tests", "dp_worker.py")], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "DP_OK rank 0" in r.stdout and "DP_OK rank 1" in r.stdout
