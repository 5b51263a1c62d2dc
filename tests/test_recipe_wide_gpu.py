"""The recipe with a subword vocabulary (vocab_size 96: the wide joint kernels of csrc/joint_wide.hip, the wide greedy search of
csrc/search.hip): captured training steps against eager ones, a VALID stage decoded on the device, forced alignment, no library route."""
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


@pytest.mark.parametrize("V,H,dtype,onehot_gates", [
    (1024, 64, "bf16", False),      # the widest one-hot predictor input, E = 1023: embedding rows + the bf16 LSTM (_LstmFn) with a padded inner dimension
    (1024, 512, "bf16", False),     # the recipe's predictor width at the widest vocabulary
    (512, 1024, "bf16", True),      # V + 1 <= H: the one-launch one-hot input projection (tsasr_lstm_onehot_gates) at E = 511
    (300, 64, "fp32", False),       # the fp32 predictor (lstm_f32) at E = 299, the wide joint with fp32 storage
])
def test_predictor_widths_train_and_decode(V, H, dtype, onehot_gates):
    """One training step and a VALID decode at the predictor widths a subword vocabulary brings (E = V - 1 up to 1023): every route stays on
    the hand-written kernels, no launcher's argument check fires in the step, the loss is finite and falls, the device greedy search decodes."""
    tt = importlib.import_module("train_tsasr")
    core = importlib.import_module("ts-asr_amd.core")
    ops = importlib.import_module("ts-asr_amd.ops")
    ops.LIB_FALLBACKS.clear()
    brain, h = make_brain(vocab_size=V, decoder_neurons=H, compute_dtype=dtype)
    m = brain.modules
    assert m.embedding.embedding_dim == V - 1 and m.decoder.rnn.input_size == V - 1 and m.decoder.rnn.hidden_size == H
    batch = tt.synthetic_loader(1, h, dict(tt.EXTRA, **SYN), 99, brain.device)[0]
    assert bool(dtype == "bf16" and ops.lstm_onehot_supported(batch.tokens_bos.data, m.decoder.rnn, V)) == onehot_gates
    m.train()
    losses = [float(brain.fit_batch(batch)) for _ in range(2)]
    assert all(np.isfinite(losses)) and losses[1] < losses[0] and brain.flush_nonfinite() == 0
    searcher = h["greedy_searcher"]
    m.eval()
    with torch.no_grad():
        logits, hyps = brain.compute_forward(batch, core.Stage.VALID)
    assert logits.shape[-1] == V and logits.stride(-2) == (V + 31) // 32 * 32
    assert searcher._greedy_is_wide() and searcher._device_greedy_ok(torch.zeros(1, 1, TINY["joint_dim"], device=DEV))
    assert len(hyps) == batch.tokens.data.shape[0] and all(0 < t < V for hyp in hyps for t in hyp)
    assert ops.LIB_FALLBACKS == {}, ops.LIB_FALLBACKS


def test_graph_recipe_with_a_subword_vocabulary():
    tt = importlib.import_module("train_tsasr")
    core = importlib.import_module("ts-asr_amd.core")
    ops = importlib.import_module("ts-asr_amd.ops")
    ops.LIB_FALLBACKS.clear()
    losses = {}
    for mode in ("eager", "graph"):
        brain, h = make_brain()
        assert brain.modules.transducer_head.w.out_features == 96 and brain.modules.embedding.embedding_dim == 95
        brain.modules.train()
        if mode == "graph":
            brain.enable_hip_graph(warmup_steps=1)
        batch = tt.synthetic_loader(1, h, dict(tt.EXTRA, **SYN), 99, brain.device)[0]
        losses[mode] = [float(brain.fit_batch(batch)) for _ in range(3)]
        assert brain.optimizer_step == 3 and brain.flush_nonfinite() == 0
        if mode == "graph":
            assert brain._graph is not None
    print("losses", losses)
    assert all(np.isfinite(losses["eager"]))
    np.testing.assert_allclose(losses["graph"], losses["eager"], rtol=1e-6)      # the rule of tests/test_model_gpu.py's replay test

    # VALID stage: the greedy searcher decodes on the device (the wide kernel: V = 96 > 63, 95 embedding columns)
    searcher = h["greedy_searcher"]
    calls = []
    on_device = searcher._greedy_on_device
    searcher._greedy_on_device = lambda *a, **k: (calls.append(1), on_device(*a, **k))[1]
    try:
        brain.modules.eval()
        with torch.no_grad():
            logits, hyps = brain.compute_forward(batch, core.Stage.VALID)
    finally:
        del searcher._greedy_on_device
    B, U = batch.tokens.data.shape
    assert logits.shape[0] == B and logits.shape[2] == U + 1 and logits.shape[3] == 96 and logits.stride(-2) == 96
    assert calls == [1] and searcher._greedy_is_wide()
    assert isinstance(hyps, list) and len(hyps) == B and all(0 < t < 96 for hyp in hyps for t in hyp)

    frames, scores = brain.align_batch(batch)
    nnet = importlib.import_module("ts-asr_amd.nnet")
    tl = nnet.abs_lengths_round(batch.mixed_sig.lengths, logits.shape[1]).cpu().tolist()
    ul = nnet.abs_lengths_round(batch.tokens.lengths, U).cpu().tolist()
    fr = frames.cpu().numpy()
    assert fr.shape == (B, U) and torch.isfinite(scores).all()
    for b in range(B):
        f = fr[b, :ul[b]]
        assert np.all(f >= 0) and np.all(f < tl[b]) and np.all(np.diff(f) >= 0) and np.all(fr[b, ul[b]:] == -1)
    bad = [k for k in ops.LIB_FALLBACKS if any(w in k.lower() for w in ("joint", "loss", "rnnt", "lstm", "greedy"))]
    assert not bad, ops.LIB_FALLBACKS
