"""The float64 CTC helper of the GPU tests (tests/helpers/ctc_ref.py) against two independent statements of the same loss - brute force over
all V^T frame labellings, and torch.nn.functional.ctc_loss(log_softmax(x), zero_infinity=True) in float64 on the CPU, values and
autograd gradient, on the case list the kernels are tested on - plus the host side that needs no GPU: the five reductions of
``ctc_loss`` and the hparams aliases. (The reference's vendored package does not import without hyperpyyaml, so the reductions are
pinned against torch's CPU function, combined exactly as speechbrain/nnet/losses.py:270-296 combines it.)"""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import ctc_cases, ctc_ref  # noqa: E402


def test_helper_equals_brute_force():
    rng = np.random.default_rng(3)
    n = 0
    for T, V in itertools.product((1, 2, 3, 4, 5), (2, 3)):
        for blank in (0, V - 1):
            labels = [v for v in range(V) if v != blank]
            for U in (0, 1, 2):
                for y in itertools.product(labels, repeat=U):
                    x = rng.standard_normal((1, T, V)) * 2
                    want, ok = ctc_ref.brute_force(x[0], y, blank)
                    got = ctc_ref.ctc_ref(x, np.array([y], np.int64).reshape(1, U), [T], [U], blank)
                    assert bool(got["feasible"][0]) == ok, (T, V, y)
                    assert got["costs"][0] == pytest.approx(want, abs=1e-12, rel=1e-12), (T, V, y)
                    if ok:      # occupancies of a frame sum to one; the gradient's rows to zero
                        np.testing.assert_allclose(got["occ"][0].sum(-1), 1.0, atol=1e-12)
                    n += 1
    assert n >= 100


def torch_reference(case):
    """torch's own CPU function in float64 on the clamped lengths and ids: (costs, gscale-weighted gradient w.r.t. the raw scores)."""
    x = torch.from_numpy(ctc_cases.seen(case)).requires_grad_()
    B, T, V = x.shape
    tl, ul = ctc_ref.lengths(case["tlen"], case["ulen"], T, case["targets"].shape[1])
    tg = torch.from_numpy(np.clip(case["targets"], 0, V - 1))
    costs = torch.nn.functional.ctc_loss(torch.log_softmax(x, -1).transpose(0, 1), tg, torch.from_numpy(tl), torch.from_numpy(ul), case["blank"],
                                         reduction="none", zero_infinity=True)
    costs.backward(torch.from_numpy(case["gscale"]))
    return costs.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("name", ctc_cases.NAMES)
def test_helper_equals_torch_float64(name):
    case = ctc_cases.get(name)
    ref = ctc_ref.ctc_ref(ctc_cases.seen(case), case["targets"], case["tlen"], case["ulen"], case["blank"], case["gscale"])
    costs, grad = torch_reference(case)
    assert sorted(np.nonzero(~ref["feasible"])[0]) == sorted(case["infeasible"]) or name.startswith("grid")
    np.testing.assert_allclose(ref["costs"], costs, rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(ref["grad"], grad, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(case["gscale"]).max()))
    assert np.all(ref["costs"][~ref["feasible"]] == 0) and np.all(ref["grad"][~ref["feasible"]] == 0)


def test_limit_case_is_the_single_path():
    case = ctc_cases.get("limit")
    ref = ctc_ref.ctc_ref(case["x"], case["targets"], case["tlen"], case["ulen"])
    lp = ctc_ref.log_softmax(case["x"][0, :9])
    assert ref["costs"][0] == pytest.approx(-sum(lp[t, k] for t, k in enumerate(ctc_cases.LIMIT_PATH)), rel=1e-12)
    assert list(ref["feasible"]) == [True, False, True] and ref["costs"][1] == 0


def test_reductions_match_the_reference_function(monkeypatch):
    """``ctc_loss``'s reductions on the CPU: the kernel call is replaced by the float64 helper (the kernels are tested on the GPU), lengths
    are RELATIVE and rounded as the reference rounds them; expected = torch's CPU function combined as losses.py:270-296 does."""
    ctc = importlib.import_module("ts-asr_amd.ctc")
    rng = np.random.default_rng(5)
    B, T, U, V = 4, 12, 5, 6
    x = torch.from_numpy(rng.standard_normal((B, T, V)))
    tg = torch.from_numpy(rng.integers(1, V, (B, U)))
    rel_t, rel_u = torch.tensor([1.0, 0.74, 0.5, 0.3]), torch.tensor([1.0, 0.6, 0.49, 0.8])

    def costs_ref(logits, targets, tl, ul, blank=0):
        return torch.from_numpy(ctc_ref.ctc_ref(logits.numpy(), targets.numpy(), tl.numpy(), ul.numpy(), blank)["costs"])

    monkeypatch.setattr(ctc, "ctc_costs", costs_ref)
    il, tl = (rel_t * T).round().int(), (rel_u * U).round().int()
    lp = torch.log_softmax(x, -1)
    for red in ("mean", "sum", "none", "batchmean", "batch"):
        inner = {"batchmean": "sum", "batch": "none"}.get(red, red)
        want = torch.nn.functional.ctc_loss(lp.transpose(0, 1), tg, il, tl, 0, zero_infinity=True, reduction=inner)
        if red == "batchmean":
            want = want / B
        elif red == "batch":
            want = want.view(B, -1).sum(1) / tl.view(B, -1).sum(1)
        for scores in (x, lp):       # raw scores and log-probs give the same value: the rows are normalised inside
            got = ctc.ctc_loss(scores, tg, rel_t, rel_u, 0, reduction=red)
            torch.testing.assert_close(got.double(), want.double(), rtol=1e-10, atol=1e-10)
    with pytest.raises(ValueError):
        ctc.ctc_loss(x, tg, rel_t, rel_u, 0, reduction="median")


def test_aliases_resolve_and_the_reference_block_loads():
    hp = importlib.import_module("ts-asr_amd.hparams")
    ctc = importlib.import_module("ts-asr_amd.ctc")
    nnet = importlib.import_module("ts-asr_amd.nnet")
    assert hp._import("speechbrain.nnet.losses.ctc_loss") is ctc.ctc_loss
    assert hp._import("speechbrain.nnet.activations.Softmax") is ctc.Softmax
    text = """
joint_dim: 64
output_neurons: 30
blank_index: 0
ctc_weight: 0.3
number_of_ctc_epochs: 60
proj_ctc: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <joint_dim>
    n_neurons: !ref <output_neurons>
ctc_cost: !name:speechbrain.nnet.losses.ctc_loss
    blank_index: !ref <blank_index>
    reduction: mean
log_softmax: !new:speechbrain.nnet.activations.Softmax
    apply_log: True
modules:
    proj_ctc: !ref <proj_ctc>
"""
    h = hp.load_hyperpyyaml(text)
    assert isinstance(h["proj_ctc"], nnet.Linear) and h["modules"]["proj_ctc"] is h["proj_ctc"] and h["proj_ctc"].w.weight.shape == (30, 64)
    assert h["ctc_cost"].func is ctc.ctc_loss and h["ctc_cost"].keywords == {"blank_index": 0, "reduction": "mean"}
    assert isinstance(h["log_softmax"], ctc.Softmax) and h["log_softmax"].apply_log
    x = torch.randn(2, 3, 5)
    torch.testing.assert_close(h["log_softmax"](x), torch.log_softmax(x, -1))
    for name in ("conformer-t_scratch_mi355x.yaml", "conformer-t_wavlm_mi355x.yaml", "conformer-t_none_mi355x.yaml"):
        with open(os.path.join(ROOT, "hparams", name)) as f:
            txt = f.read()
        assert "ctc_weight: 0.0" in txt and "number_of_ctc_epochs: 0" in txt and "ctc_cost: !name:speechbrain.nnet.losses.ctc_loss" in txt
