"""Completeness of the stream scenarios (tests/stream_tools.py): every exported function of include/cvae.h whose last parameter is
`void* stream` is called by at least one scenario of the registry, or stands in the explicit exclusion list with its reason.  A new
entry point with a stream parameter fails here until it has a scenario.  No GPU."""
import re

import stream_tools as ST


def test_header_parse_finds_the_stream_entries():
    names = ST.header_stream_entries()
    with open(ST.HEADER) as f:
        text = f.read()
    assert len(names) == len(re.findall(r"void\*\s*stream\)", text)) == 59
    for known in ("cvae_forward", "cvae_decode", "cvae_crf_grid", "cvae_tensor_stats", "cvae_op_msssim", "cvae_op_fc_bwd", "cvae_guard_init"):
        assert known in names
    for host_only in ("cvae_create", "cvae_ws_offset", "cvae_probe_config", "cvae_op_latent_plan", "cvae_grad_bucket", "cvae_sync_slot"):
        assert host_only not in names


def test_every_stream_entry_point_has_a_scenario():
    header, registry, excluded = set(ST.header_stream_entries()), set(ST.registry_entries()), set(ST.EXCLUDED)
    assert len(excluded) <= ST.MAX_EXCLUDED and all(ST.EXCLUDED[k].strip() for k in excluded)
    assert excluded <= header, f"excluded, but not an entry point with a stream: {sorted(excluded - header)}"
    assert not (registry & excluded), f"excluded and called: {sorted(registry & excluded)}"
    assert not (registry - header), f"scenarios declare functions the header does not export with a stream: {sorted(registry - header)}"
    assert registry == header - excluded, f"no scenario calls: {sorted(header - excluded - registry)}"


def test_registry_is_well_formed():
    names = [s.name for s in ST.SCENARIOS]
    assert len(names) == len(set(names))
    for s in ST.SCENARIOS:
        assert s.entries and s.group in ST.groups()
        assert s.host_async or s.why_not_async
        assert re.fullmatch(r"[a-z0-9.-]+", s.name), s.name
    # the cases the contract names: both frame sizes, every precision at 64 x 64, the library's side stream off and on
    for W, B, p in ST.STEP_CASES:
        for mode in ("inline", "overlap"):
            assert f"step-w{W}-b{B}-{p}-{mode}" in names
    assert {p for W, _, p in ST.STEP_CASES if W == 64} == {"f32", "bf16", "bf16x9", "bf16x6"}
    assert {p for W, _, p in ST.STEP_CASES if W == 128} == {"f32", "bf16"}
    assert 1 <= ST.HW_QUEUES <= 32


def test_blocker_length_rule():
    assert ST.Harness.blocker_seconds(0.0) == 0.5
    assert ST.Harness.blocker_seconds(0.01) == 0.5
    assert abs(ST.Harness.blocker_seconds(0.05) - 1.0) < 1e-12
    assert ST.Harness.blocker_seconds(1.0) == 3.0
