"""The recipe on the lazy joint logits (hparams joint_logits: lazy -> rnnt.JointLogits -> the fused joint + loss kernels of
csrc/joint_wide.hip) against the default, materialised route on the same small subword brain (tests/test_recipe_wide_gpu.py's): one
training step, the VALID stage's hypotheses, forced alignment; and a brain without the key is untouched."""
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(d_model=64, nhead=4, encoder_num_layers=2, speaker_num_layers=1, d_ffn=256, joint_dim=64, decoder_neurons=64, vocab_size=96,
            compute_dtype="bf16", dropout=0.0)
SYN = dict(syn_batch=3, syn_seconds=2.0, syn_enroll_seconds=1.0, syn_tokens=10)


def make_brain(**over):
    hp = importlib.import_module("ts-asr_amd.hparams")
    tsasr = importlib.import_module("ts-asr_amd.recipes.tsasr")
    torch.manual_seed(11)                  # the two brains of the comparison start from the same weights
    ov = dict(TINY, **over)
    with open(os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml")) as f:
        h = hp.load_hyperpyyaml(f, dict(ov))
    return tsasr.TSASR(h["modules"], h["opt_class"], h, {"device": DEV, "compute_dtype": ov["compute_dtype"]}), h


def test_lazy_recipe_against_the_default_route():
    tt = importlib.import_module("train_tsasr")
    core = importlib.import_module("ts-asr_amd.core")
    rn = importlib.import_module("ts-asr_amd.rnnt")
    ops = importlib.import_module("ts-asr_amd.ops")
    ops.LIB_FALLBACKS.clear()
    got = {}
    for route in ("default", "lazy"):
        brain, h = make_brain(**({"joint_logits": "lazy"} if route == "lazy" else {}))
        assert ("joint_logits" in h) == (route == "lazy")
        batch = tt.synthetic_loader(1, h, dict(tt.EXTRA, **SYN), 99, brain.device)[0]
        # forward and evaluation before the step, on identical weights
        brain.modules.eval()
        with torch.no_grad():
            first, hyps = brain.compute_forward(batch, core.Stage.VALID)
        assert isinstance(first, rn.JointLogits) == (route == "lazy") and torch.is_tensor(first) == (route == "default")
        B, U = batch.tokens.data.shape
        assert tuple(first.shape) == (B, first.shape[1], U + 1, 96)
        frames, scores = brain.align_batch(batch)
        eval_loss = float(brain.evaluate_batch(batch, core.Stage.VALID))
        # one fit_batch: with two micro-batches per optimizer step the first one leaves its gradients (of loss / 2, in both routes) in place
        brain.modules.train()
        brain.grad_accumulation_factor = 2
        loss = brain.fit_batch(batch)
        torch.cuda.synchronize()
        assert brain.optimizer_step == 0
        grads = {n: p.grad.detach().float().clone() for n, p in brain.modules.named_parameters() if p.requires_grad and p.grad is not None}
        step_loss = float(brain.fit_batch(batch))            # the same weights again, now with the optimizer's step behind it
        assert brain.optimizer_step == 1 and brain.flush_nonfinite() == 0
        got[route] = dict(hyps=hyps, frames=frames.cpu(), scores=scores.cpu(), eval_loss=eval_loss, loss=float(loss), grads=grads, step_loss=step_loss)
    d, z = got["default"], got["lazy"]
    print(f"loss default {d['loss']:.6f} lazy {z['loss']:.6f}; fit_batch default {d['step_loss']:.6f} lazy {z['step_loss']:.6f}; "
          f"eval default {d['eval_loss']:.6f} lazy {z['eval_loss']:.6f}")
    assert z["loss"] == pytest.approx(d["loss"], rel=1e-4) and z["step_loss"] == pytest.approx(d["step_loss"], rel=1e-4)
    assert z["eval_loss"] == pytest.approx(d["eval_loss"], rel=1e-4)
    assert set(z["grads"]) == set(d["grads"]) and len(d["grads"]) > 10
    worst = max(((float((z["grads"][n] - g).norm() / g.norm()), n) for n, g in d["grads"].items() if float(g.norm()) > 0), default=(0.0, ""))
    print(f"worst parameter-gradient relative L2 between the routes: {worst[0]:.3e} ({worst[1]})")
    for n, g in d["grads"].items():
        if float(g.norm()) > 0:
            assert float((z["grads"][n] - g).norm() / g.norm()) < 1.2e-2, n
        else:
            assert float(z["grads"][n].norm()) == 0, n
    assert z["hyps"] == d["hyps"] and len(d["hyps"]) == 3
    assert torch.equal(z["frames"], d["frames"])
    assert torch.all((z["scores"] - d["scores"]).abs() <= 1e-4 + 2e-5 * d["scores"].abs())
    bad = [k for k in ops.LIB_FALLBACKS if any(w in k.lower() for w in ("joint", "loss", "rnnt"))]
    assert not bad, ops.LIB_FALLBACKS


def test_lazy_recipe_captured_in_a_graph():
    """The lazy step replayed as one hipGraph gives the eager steps' losses (the rule of tests/test_recipe_wide_gpu.py's replay test)."""
    import numpy as np
    tt = importlib.import_module("train_tsasr")
    losses = {}
    for mode in ("eager", "graph"):
        brain, h = make_brain(joint_logits="lazy")
        brain.modules.train()
        if mode == "graph":
            brain.enable_hip_graph(warmup_steps=1)
        batch = tt.synthetic_loader(1, h, dict(tt.EXTRA, **SYN), 99, brain.device)[0]
        losses[mode] = [float(brain.fit_batch(batch)) for _ in range(3)]
        assert brain.optimizer_step == 3 and brain.flush_nonfinite() == 0
        if mode == "graph":
            assert brain._graph is not None
    print("losses", losses)
    assert all(np.isfinite(losses["eager"])) and losses["eager"][2] < losses["eager"][0]
    np.testing.assert_allclose(losses["graph"], losses["eager"], rtol=1e-6)
