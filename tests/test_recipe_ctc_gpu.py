"""The recipe's auxiliary CTC branch (hparams ctc_weight / number_of_ctc_epochs / ctc_cost, modules proj_ctc) on a tiny brain and a
--synthetic-shaped batch: the step's loss is ctc_weight * CTC + (1 - ctc_weight) * transducer, the head and the encoder receive the CTC
gradient, both joint routes carry the same CTC term, the VALID stage scores the head's greedy decoding, a captured step reproduces the
eager one - and with ctc_weight = 0 nothing is built and nothing changes."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = dict(d_model=64, nhead=4, encoder_num_layers=2, speaker_num_layers=1, d_ffn=256, joint_dim=64, decoder_neurons=64, compute_dtype="bf16",
            dropout=0.0)
SYN = dict(syn_batch=3, syn_seconds=2.0, syn_enroll_seconds=1.0, syn_tokens=10)
CTC = dict(ctc_weight=0.3, number_of_ctc_epochs=5)


def make_brain(**over):
    hp = importlib.import_module("ts-asr_amd.hparams")
    tsasr = importlib.import_module("ts-asr_amd.recipes.tsasr")
    torch.manual_seed(11)                  # brains of a comparison start from the same weights (proj_ctc is drawn after all the others)
    ov = dict(TINY, **over)
    with open(os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml")) as f:
        h = hp.load_hyperpyyaml(f, dict(ov))
    return tsasr.TSASR(h["modules"], h["opt_class"], h, {"device": DEV, "compute_dtype": ov["compute_dtype"]}), h


def batch_for(brain, h):
    tt = importlib.import_module("train_tsasr")
    return tt.synthetic_loader(1, h, dict(tt.EXTRA, **SYN), 99, brain.device)[0]


def parts(brain, h, batch, epoch):
    """(step loss, transducer loss, CTC loss or None) from ONE forward in training mode, each term computed separately."""
    core = importlib.import_module("ts-asr_amd.core")
    h["epoch_counter"].current = epoch
    brain.on_fit_start()
    brain.modules.train()
    with torch.no_grad():
        out = brain.compute_forward(batch, core.Stage.TRAIN)
        loss = float(brain.compute_objectives(out, batch, core.Stage.TRAIN))
        tokens, tokens_lens = batch.tokens
        trans = float(h["transducer_loss"](out[0], tokens, batch.mixed_sig.lengths, tokens_lens))
        c = None if len(out) < 3 or out[2] is None else float(h["ctc_cost"](out[2], tokens, batch.mixed_sig.lengths, tokens_lens))
    return loss, trans, c, out


def test_step_loss_is_the_weighted_sum_and_stops_after_the_ctc_epochs():
    ops = importlib.import_module("ts-asr_amd.ops")
    ops.LIB_FALLBACKS.clear()
    brain, h = make_brain(**CTC)
    assert "proj_ctc" in brain.modules and brain.modules.proj_ctc.w.weight.shape == (29, 64)
    batch = batch_for(brain, h)
    loss, trans, c, out = parts(brain, h, batch, epoch=1)
    B, T = out[0].shape[:2]
    assert len(out) == 3 and tuple(out[2].shape) == (B, T, 29) and np.isfinite([loss, trans, c]).all() and c > 0
    print(f"loss {loss:.6f} = 0.3 * {c:.6f} + 0.7 * {trans:.6f}")
    assert loss == pytest.approx(0.3 * c + 0.7 * trans, rel=1e-6)
    loss5 = parts(brain, h, batch, epoch=5)[0]
    assert loss5 == pytest.approx(loss, rel=1e-6)                 # the last CTC epoch
    loss6, trans6, c6, out6 = parts(brain, h, batch, epoch=6)     # beyond number_of_ctc_epochs: the term is gone, the factor stays
    assert len(out6) == 3 and out6[2] is None and c6 is None
    assert loss6 == pytest.approx(0.7 * trans6, rel=1e-6) and trans6 == pytest.approx(trans, rel=1e-6)
    bad = [k for k in ops.LIB_FALLBACKS if "matmul" in k.lower() or "ctc" in k.lower()]
    assert not bad, ops.LIB_FALLBACKS                             # the 29-row head ran on the hand-written GEMM


def test_ctc_weight_zero_builds_nothing():
    core = importlib.import_module("ts-asr_amd.core")
    plain, hp0 = make_brain()
    zero, hz = make_brain(ctc_weight=0.0, number_of_ctc_epochs=3)
    on, _ = make_brain(**CTC)
    names = [n for n, _ in plain.modules.named_parameters()]
    assert "proj_ctc" not in plain.modules and "proj_ctc" not in zero.modules and hp0["ctc_weight"] == 0.0
    assert [n for n, _ in zero.modules.named_parameters()] == names
    assert sum(p.numel() for p in zero.modules.parameters()) == sum(p.numel() for p in plain.modules.parameters())
    assert list(zero.modules.state_dict()) == list(plain.modules.state_dict())
    assert [n for n, _ in on.modules.named_parameters()] == names + ["proj_ctc.w.weight", "proj_ctc.w.bias"]
    for (n, p), (_, q) in zip(plain.modules.named_parameters(), on.modules.named_parameters()):
        assert torch.equal(p, q), n                               # the same draw for every other weight
    batch = batch_for(zero, hz)
    zero.modules.eval()
    with torch.no_grad():
        assert len(zero.compute_forward(batch, core.Stage.VALID)) == 2
    loss, trans, c, out = parts(zero, hz, batch, epoch=1)
    assert len(out) == 2 and c is None and loss == trans


def _one_accumulate_step(**over):
    brain, h = make_brain(**over)
    h["epoch_counter"].current = 1
    batch = batch_for(brain, h)
    brain.modules.train()
    brain.grad_accumulation_factor = 2        # the first micro-batch leaves its gradients (of loss / 2) in place
    loss = float(brain.fit_batch(batch))
    torch.cuda.synchronize()
    assert brain.optimizer_step == 0 and brain.flush_nonfinite() == 0
    return loss, {n: p.grad.detach().float().cpu().clone() for n, p in brain.modules.named_parameters() if p.grad is not None}


def test_ctc_gradient_reaches_the_head_and_the_encoder():
    loss0, g0 = _one_accumulate_step()
    loss1, g1 = _one_accumulate_step(**CTC)
    assert np.isfinite(loss1) and loss1 != loss0
    for n in ("proj_ctc.w.weight", "proj_ctc.w.bias"):
        assert n in g1 and n not in g0 and torch.isfinite(g1[n]).all() and float(g1[n].abs().max()) > 0, n
    enc = [n for n in g0 if n.startswith(("encoder.", "encoder_proj.", "frontend."))]
    assert len(enc) > 10 and all(torch.isfinite(g1[n]).all() for n in g1)
    changed = [n for n in enc if float(g0[n].norm()) > 0 and not torch.equal(g0[n], g1[n])]
    assert len(changed) > len(enc) // 2, (len(changed), len(enc))
    # the predictor sees the transducer term alone: its gradient is 0.7 x the plain step's
    dec = [n for n in g0 if n.startswith("decoder.") and float(g0[n].norm()) > 0]
    assert dec
    for n in dec:
        assert float((g1[n] - 0.7 * g0[n]).norm() / g0[n].norm()) < 2e-2, n


def test_lazy_joint_route_carries_the_same_ctc_term():
    got = {}
    for route in ("materialized", "lazy"):
        brain, h = make_brain(vocab_size=96, joint_logits=route, **CTC)
        batch = batch_for(brain, h)
        got[route] = parts(brain, h, batch, epoch=1)[:3]
    (lm, tm, cm), (lz, tz, cz) = got["materialized"], got["lazy"]
    print(f"materialized {got['materialized']} lazy {got['lazy']}")
    assert cz == cm and tz == pytest.approx(tm, rel=1e-4)
    assert lz == pytest.approx(0.3 * cz + 0.7 * tz, rel=1e-6) and lm == pytest.approx(0.3 * cm + 0.7 * tm, rel=1e-6)
    loss, grads = _one_accumulate_step(vocab_size=96, joint_logits="lazy", **CTC)
    assert np.isfinite(loss) and float(grads["proj_ctc.w.weight"].abs().max()) > 0


def test_valid_stage_scores_the_ctc_head():
    core = importlib.import_module("ts-asr_amd.core")
    metrics = importlib.import_module("ts-asr_amd.metrics")
    ctc = importlib.import_module("ts-asr_amd.ctc")
    brain, h = make_brain(**CTC)
    batch = batch_for(brain, h)
    brain.on_fit_start()
    brain._eval_loop([batch], core.Stage.VALID, 1)
    assert "ctc_TER" in brain.valid_stats and 0 <= brain.valid_stats["ctc_TER"]        # token ids against batch.tokens without a tokenizer
    hyps = brain.last_ctc_hyps
    assert len(hyps) == 3 and all(isinstance(x, list) for x in hyps)
    tok = metrics.CharTokenizer(["<blank>", "▁"] + list("abcdefghijklmnopqrstuvwxyz'"))
    brain.tokenizer = tok
    batch.target_words = tok(metrics.undo_padding(batch.tokens.data.cpu(), batch.tokens.lengths.cpu()), task="decode_from_list")
    brain._eval_loop([batch], core.Stage.VALID, 1)
    assert {"ctc_CER", "ctc_WER"} <= set(brain.valid_stats) and np.isfinite(brain.valid_stats["ctc_CER"])
    assert brain.last_ctc_hyps == hyps
    # what was scored is the greedy decoding of the head's scores on the VALID forward
    brain.modules.eval()
    with torch.no_grad():
        out = brain.compute_forward(batch, core.Stage.VALID)
    assert ctc.ctc_greedy_decode(out[2], batch.mixed_sig.lengths, 0) == hyps


def test_graph_replay_matches_eager_with_ctc():
    """The CTC step replayed as one hipGraph gives the eager steps' losses (the rule of tests/test_recipe_lazy_gpu.py's and
    tests/test_recipe_wide_gpu.py's replay tests: rtol 1e-6 over three optimizer steps); after the CTC epochs another graph is captured."""
    losses = {}
    for mode in ("eager", "graph"):
        brain, h = make_brain(**dict(CTC, number_of_ctc_epochs=1))
        h["epoch_counter"].current = 1
        brain.modules.train()
        if mode == "graph":
            brain.enable_hip_graph(warmup_steps=1)
        batch = batch_for(brain, h)
        losses[mode] = [float(brain.fit_batch(batch)) for _ in range(3)]
        assert brain.optimizer_step == 3 and brain.flush_nonfinite() == 0
        if mode == "graph":
            assert brain._graph is not None and len(brain._graphs) == 1
        h["epoch_counter"].current = 2            # beyond the CTC epochs: the term leaves the step (and the captured graph is not reused)
        losses[mode] += [float(brain.fit_batch(batch)) for _ in range(3)]
        if mode == "graph":
            assert len(brain._graphs) == 2
    print("losses", losses)
    assert all(np.isfinite(losses["eager"])) and losses["eager"][2] < losses["eager"][0]
    np.testing.assert_allclose(losses["graph"], losses["eager"], rtol=1e-6)
