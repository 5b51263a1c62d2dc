"""The float64 slot-schedule model (tests/helpers/stream_slots_ref.py) on the CPU: every session of a schedule with admissions,
a pause, a free slot and a release + admit in one tick equals attn_stream_ref.reference of that session alone, and every planted
defect is rejected by the check named for it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_stream_ref as SR  # noqa: E402
import stream_slots_ref as SS  # noqa: E402

B, H, DH, TMAX, C, K, DC = 3, 2, 4, 24, 4, 5, 6
LENGTHS = {"s0": (12, 10), "s1": (8, 8), "s2": (16, 16), "s3": (8, 5)}       # frames, valid frames
# s0 enters slot 0; s1 enters slot 2 one tick later and is paused the tick after; slot 1 stays free for four ticks, then takes s3;
# s0 ends after three pushes and is released, s2 enters slot 0 in the same tick
TICKS = [{"admit": {0: "s0"}}, {"admit": {2: "s1"}}, {"pause": [2]}, {"release": [0], "admit": {0: "s2"}}, {"admit": {1: "s3"}}, {}, {}, {}]


def make(causal, defect=None):
    qkv, pkh, u, v, scale = SR.inputs(1, 64, H, DH, TMAX)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(DC, K, generator=g, dtype=torch.float64)
    sessions, at = {}, 0
    for name, (T, L) in LENGTHS.items():
        sessions[name] = dict(qkv=qkv[0, at:at + T].double(), glu=torch.randn(T, DC, generator=g, dtype=torch.float64), len=L)
        at += T
    model = SS.Slots(B, H, DH, TMAX, pkh, u, v, scale, causal, conv_w=w, defect=defect)
    return model, sessions


@pytest.mark.parametrize("causal", [1, 4])
def test_sessions_equal_the_session_alone(causal):
    model, sessions = make(causal)
    got = SS.run_schedule(model, sessions, TICKS, C)
    for name, (T, _) in LENGTHS.items():
        assert got[name][0].shape[0] == T and got[name][1].shape[0] == T, name       # the schedule pushes every frame of every session
    res = SS.run_checks(model, sessions, got, C)
    assert all(not v for v in res.values()), res
    assert any(not all(a) for a, _, _ in model.trace) and len(model.trace) == len(TICKS)


@pytest.mark.parametrize("defect", sorted(SS.DEFECTS))
@pytest.mark.parametrize("causal", [1, 4])
def test_planted_defect_is_rejected_by_its_check(defect, causal):
    model, sessions = make(causal, defect)
    got = SS.run_schedule(model, sessions, TICKS, C)
    res = SS.run_checks(model, sessions, got, C)
    assert res[SS.DEFECTS[defect]], (defect, res)


def test_idle_slot_rows_are_zero_and_offsets_array():
    model, sessions = make(1)
    model.admit(0)
    qkv = torch.randn(B, C, 3 * H * DH, dtype=torch.float64)
    assert model.offsets([True, False, False]) == [0, -1, -1]
    out, z = model.push(qkv, torch.randn(B, C, DC, dtype=torch.float64), [True, False, False])
    assert bool((out[1:] == 0).all()) and bool((z[1:] == 0).all()) and bool(out[0].abs().sum() > 0)
    assert model.t0 == [C, 0, 0] and bool(torch.isnan(model.kc[1:]).all())
