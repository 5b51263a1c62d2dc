"""The float64 helper of the wide beam search (tests/helpers/beam_wide_ref.py) and the host-side surface of the feature, without a GPU:
every tested case meets beam_case_ok in fp32 and on the bf16-rounded weights (so the GPU tests may compare hypotheses exactly), the helper
equals beam_lm_ref.beam_search_lm and the reference's hypotheses in tests/golden/c1_beam_wide.npz, the entry points are declared, and the
workspace and LDS formulas of ops are the documented ones."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beam_lm_ref as BL  # noqa: E402
import beam_wide_ref as BW  # noqa: E402

RUNS = [(name, beam) for name, c in BW.CASES.items() for beam in c["runs"]]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,beam", RUNS)
def test_every_case_meets_beam_case_ok(name, beam, bf16):
    res = BW.run_case(name, beam, bf16)
    ok, peak, n_long, per_frame, mm = BW.beam_case_ok(res, BW.CASES[name]["T"])
    print(f"{name} beam {beam} bf16={bf16}: peak {peak}, utterances with >= 4 tokens {n_long}, expansions per frame {per_frame:.2f}, margin {mm:.2e}")
    assert ok, (peak, n_long, per_frame, mm)
    for r in res:
        assert len(r["nbest"]) == len(r["scores"]) == len(r["frames"]) <= BW.NBEST
        for toks, fr in zip(r["nbest"], r["frames"]):
            assert len(toks) == len(fr) and fr == sorted(fr) and all(0 <= t < BW.CASES[name]["T"] for t in fr)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lm_case", list(BW.LM_CASES))
def test_lm_cases_meet_beam_case_ok_and_change_the_hypotheses(lm_case, bf16):
    c = BW.LM_CASES[lm_case]
    fused = BW.run_case(c["case"], c["beam"], bf16, lm_case)
    plain = BW.run_case(c["case"], c["beam"], bf16, None, BW.NBEST, c["run"])
    ok, peak, n_long, per_frame, mm = BW.beam_case_ok(fused, BW.CASES[c["case"]]["T"])
    print(f"{lm_case} bf16={bf16}: peak {peak}, long {n_long}, expansions per frame {per_frame:.2f}, margin {mm:.2e}")
    assert ok, (peak, n_long, per_frame, mm)
    assert any(f["nbest"] != p["nbest"] for f, p in zip(fused, plain))


def test_helper_equals_the_lm_helper_it_restates():
    """Same n-best and the same score bits as beam_lm_ref.beam_search_lm, with and without an LM."""
    for lm_case in (None, "v100_l2b1"):
        run = BW.LM_CASES[lm_case]["run"] if lm_case else None
        net = BW.case_net("v100", 4, False, run)
        lw = BW.lm_weights(lm_case) if lm_case else None
        ours = BW.run_case("v100", 4, False, lm_case)
        for b, r in enumerate(ours):
            toks, sc = BL.beam_search_lm(net["enc"][b], net, lw, 0.3 if lm_case else 0.0, 4, nbest=BW.NBEST)
            assert toks == r["nbest"] and sc == r["scores"], (lm_case, b)


def test_helper_equals_the_reference_fixture(golden):
    """tests/golden/c1_beam_wide.npz (tools/gen_golden_beam_wide.py): the reference's own searcher, beam 4, nbest 3, float32."""
    g = golden["c1_beam_wide"]
    for name in BW.FIXTURE_CASES:
        for b, r in enumerate(BW.run_case(name, 4)):
            lens = g[f"{name}_lens"][b]
            want = [g[f"{name}_hyps"][b, k, : int(lens[k])].tolist() for k in range(BW.NBEST) if lens[k] >= 0]
            assert r["nbest"] == want, (name, b)
            np.testing.assert_allclose(r["scores"], g[f"{name}_scores"][b, : len(want)], rtol=0, atol=1e-4)


def test_entry_points_are_declared_and_prototyped(pkg):
    capi = importlib.import_module("ts-asr_amd._capi")
    header = open(os.path.join(ROOT, "include", "tsasr_hip.h")).read()
    declared = set(re.findall(r"\b(tsasr_[a-z0-9_]+)\s*\(", header))
    for name in ("tsasr_greedy_decode", "tsasr_beam_search", "tsasr_beam_search_workspace_bytes"):
        assert name in declared and name in capi.exported_symbols(), name
    # the thirteen entry points folded into those three: none is declared, prototyped or exported
    gone = ["tsasr_greedy_decode" + s for s in ("_stream", "_wide", "_stream_wide")]
    gone += ["tsasr_beam_search" + s for s in ("_stream", "_timed", "_stream_timed", "_lm", "_wide", "_bias")]
    gone += ["tsasr_beam_search" + s + "_workspace_bytes" for s in ("_timed", "_lm", "_wide", "_bias")]
    assert len(gone) == 13
    for name in gone:
        assert name not in declared and name not in capi.exported_symbols() and not hasattr(capi.lib(), name), name


def test_workspace_and_lds_formulas(pkg):
    """ops.beam_workspace_bytes with ``wide`` / beam_wide_lds_bytes against the formulas of include/tsasr_hip.h, written out here."""
    ops = importlib.import_module("ts-asr_amd.ops")
    a16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    for B, T, H, J, V, beam, cap, Ll, Hl, times in ((3, 24, 64, 64, 100, 4, 512, 0, 0, False), (2, 12, 512, 640, 1024, 4, 512, 2, 1024, True),
                                                    (1, 4096, 64, 64, 101, 15, 33, 1, 32, True)):
        nodes = 1 + (T + 1) * beam + cap
        lmw = (V + 3) // 4 * 4 + 2 * Ll * Hl if Ll else 0
        want = B * (a16(64 + 24 * beam) + a16(8 * nodes) + 4 * (cap + beam) * (J + 2 * H + lmw) + (a16(4 * nodes) if times else 0))
        assert ops.beam_workspace_bytes(B, T, H, J, V, beam, cap, Ll, Hl, times, wide=True) == want
    assert ops.beam_workspace_bytes(0, 24, 64, 64, 100, 4, 512, wide=True) == 0
    # H = 512, J = 640, V = 1024, E = 1023, cap 512, a 2 x 1024 LM (emb 1024, no dnn block), timed
    base = 4 * (6 * 512 + 2 * 640 + 1024 + 1024 + 96) + 512 * (16 + 28)
    assert ops.beam_wide_lds_bytes(512, 640, 1023, 1024, 512) == base
    assert ops.beam_wide_lds_bytes(512, 640, 1023, 1024, 512, (1024, 1024, 1024)) == base + 4 * (1024 + 2048 + 4096 + 2048 + 2)
    assert ops.beam_wide_lds_bytes(512, 640, 1023, 1024, 512, (1024, 1024, 1024)) <= ops.BEAM_WIDE_LDS_MAX
