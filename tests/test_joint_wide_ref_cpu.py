"""The float64 helper of the wide-vocabulary joint (tests/helpers/joint_wide_ref.py) against the oracle and autograd, the reference-pin
fixture against the oracle, and the C-ABI declarations of the wide entry points. No GPU."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import tsasr_ref as R
from oracle.golden_recipe import det_tensor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import joint_wide_ref as JW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_SYMBOLS = ("tsasr_joint_wide_fwd", "tsasr_joint_wide_bwd_workspace_bytes", "tsasr_joint_wide_bwd")
SHAPES = [(1, 1, 1, 32, 33), (2, 7, 5, 64, 100), (2, 3, 4, 160, 257)]


def case(B, T, U1, J, V):
    f64 = lambda name, shape, scale: torch.from_numpy(det_tensor(name, shape, scale)).double()  # noqa: E731
    return (f64("jw.enc", (B, T, J), 1.0), f64("jw.dec", (B, U1, J), 1.0), f64("jw.W", (V, J), 1.0 / np.sqrt(J)), f64("jw.b", (V,), 0.1),
            f64("jw.g", (B, T, U1, V), 1.0))


@pytest.mark.parametrize("B,T,U1,J,V", SHAPES)
def test_unrounded_forward_is_the_oracle(B, T, U1, J, V):
    enc, dec, W, b, _ = case(B, T, U1, J, V)
    ref = R.joint_logits(enc, dec, {"w.weight": W, "w.bias": b}, "")
    assert ref.dtype == torch.float64
    torch.testing.assert_close(JW.forward(enc, dec, W, b, rounded=False), ref, atol=1e-12, rtol=1e-12)


@pytest.mark.parametrize("B,T,U1,J,V", SHAPES)
def test_analytic_gradients_are_autograd(B, T, U1, J, V):
    enc, dec, W, b, g = case(B, T, U1, J, V)
    leaves = [t.clone().requires_grad_() for t in (enc, dec, W, b)]
    (R.joint_logits(leaves[0], leaves[1], {"w.weight": leaves[2], "w.bias": leaves[3]}, "") * g).sum().backward()
    for got, leaf, name in zip(JW.backward(enc, dec, W, g, rounded=False), leaves, ("denc", "ddec", "dW", "dbias")):
        err = float((got - leaf.grad).abs().max())
        print(f"{name}: max |analytic - autograd| = {err:.2e}")
        assert err <= 1e-10, (name, err)


def test_rounded_forward_rounds_only_the_two_operands():
    """bf16-representable activations whose sums and LeakyReLU images are bf16-representable too, bf16-representable weights: nothing is left
    to round, so the rounded and the plain forward agree to float64 precision - the rounding sits on h and W and nowhere else."""
    B, T, U1, J, V = 2, 3, 4, 32, 40
    rng = np.random.default_rng(5)
    enc = torch.from_numpy(rng.integers(0, 8, size=(B, T, J)).astype(np.float64))        # x = e + d >= 0: h = x, a small integer
    dec = torch.from_numpy(rng.integers(0, 8, size=(B, U1, J)).astype(np.float64))
    W = torch.from_numpy(rng.integers(-8, 8, size=(V, J)).astype(np.float64) / 16)
    b = torch.from_numpy(rng.standard_normal(V))
    torch.testing.assert_close(JW.forward(enc, dec, W, b), JW.forward(enc, dec, W, b, rounded=False), atol=1e-12, rtol=0)
    g = torch.from_numpy(rng.integers(-4, 4, size=(B, T, U1, V)).astype(np.float64))
    for a, r in zip(JW.backward(enc, dec, W, g), JW.backward(enc, dec, W, g, rounded=False)):
        torch.testing.assert_close(a, r, atol=1e-12, rtol=0)


@pytest.mark.parametrize("V", JW.FIXTURE_VOCABS)
def test_fixture_is_the_oracle_function(golden, V):
    """The reference's own joiner + head (fp32, stored) computes the function the helper restates: fp32 rounding of a 64-term sum apart."""
    enc, dec, W, b = (torch.from_numpy(x) for x in JW.fixture_inputs(V))
    stored = torch.from_numpy(golden["c1_wide_vocab"][f"logits_v{V}"])
    assert stored.shape == (*JW.FIXTURE_SHAPE[:3], V) and stored.dtype == torch.float32
    torch.testing.assert_close(stored.double(), JW.forward(enc, dec, W, b, rounded=False), atol=2e-6, rtol=2e-6)


def test_wide_entry_points_are_declared(pkg):
    capi = importlib.import_module("ts-asr_amd._capi")
    header = open(os.path.join(ROOT, "include", "tsasr_hip.h")).read()
    declared = set(re.findall(r"\b(tsasr_[a-z0-9_]+)\s*\(", header))
    for name in WIDE_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/tsasr_hip.h"
        assert name in capi.exported_symbols(), f"{name} has no prototype in _capi"


# ---- the float64 greedy search of the helper ----
class _Emb(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, tok):
        return self.table[tok.long()]


class _Dec(torch.nn.Module):
    def __init__(self, rnn):
        super().__init__()
        self.rnn = rnn

    def forward(self, x, hx=None):
        return self.rnn(x, hx)


@pytest.mark.parametrize("name", ["v64", "v100", "v100_e128"])
def test_helper_greedy_is_the_host_loop(name):
    """decoders.TransducerBeamSearcher's step-wise greedy loop over plain float64 CPU modules (torch.nn LSTM / Linear with the case's
    weights, the package's own joiner) emits the helper's tokens at the helper's frames."""
    dec = importlib.import_module("ts-asr_amd.decoders")
    rn = importlib.import_module("ts-asr_amd.rnnt")
    V, _, H, J, _ = JW.GREEDY_CASES[name]
    net = {k: torch.from_numpy(v).double() for k, v in JW.greedy_net(name).items()}
    rnn = torch.nn.LSTM(net["emb"].shape[1], H, batch_first=True).double()
    rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]})
    proj, head = torch.nn.Linear(H, J).double(), torch.nn.Linear(J, V).double()
    proj.load_state_dict({"weight": net["w_proj"], "bias": net["b_proj"]})
    head.load_state_dict({"weight": net["w_head"], "bias": net["b_head"]})
    s = dec.TransducerBeamSearcher([_Emb(net["emb"]), _Dec(rnn), proj], rn.Transducer_joint(), [head], blank_id=0, beam_size=1)
    assert not s._device_greedy_ok(net["enc"])
    hyps, _, _, _, frames, _ = s.forward_timed(net["enc"])
    ours = JW.greedy(JW.greedy_net(name))
    assert hyps == [r["tokens"] for r in ours] and frames == [r["frames"] for r in ours]


@pytest.mark.parametrize("name", list(JW.GREEDY_CASES))
def test_search_cases_meet_their_conditions(golden, name):
    """Every search case: a quarter blank and a quarter emitting decisions at least, float64 top-2 margin >= 1e-4 at every decision - in
    fp32 and with the matrices and the encoder output rounded to bf16 (what the bf16 device run reads); the fixture cases also give the
    reference searcher's stored hypotheses."""
    net = JW.greedy_net(name)
    for rounded in (False, True):
        res = JW.greedy(JW.greedy_net_bf16(net) if rounded else net)
        ok, fb, fe, mm = JW.greedy_case_ok(res)
        print(f"{name} bf16={rounded}: blank {fb:.3f} emit {fe:.3f} smallest margin {mm:.2e}")
        assert ok, (fb, fe, mm)
        if name in JW.FIXTURE_GREEDY and not rounded:
            g = golden["c1_wide_vocab"]
            stored = [list(map(int, row[:n])) for row, n in zip(g[f"greedy_{name}_hyps"], g[f"greedy_{name}_lens"])]
            assert [r["tokens"] for r in res] == stored


def test_greedy_entry_points_are_declared(pkg):
    capi = importlib.import_module("ts-asr_amd._capi")
    header = open(os.path.join(ROOT, "include", "tsasr_hip.h")).read()
    declared = set(re.findall(r"\b(tsasr_[a-z0-9_]+)\s*\(", header))
    assert "tsasr_greedy_decode" in declared and "tsasr_greedy_decode" in capi.exported_symbols()
    for suffix in ("_stream", "_wide", "_stream_wide"):          # folded into the one entry point (state / n_valid NULL, wide)
        name = "tsasr_greedy_decode" + suffix
        assert name not in declared and name not in capi.exported_symbols() and not hasattr(capi.lib(), name), name
