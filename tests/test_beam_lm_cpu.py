"""Beam search with LM fusion, the parts that need no GPU: the float64 restatement (tests/helpers/beam_lm_ref.py) against the reference's
own hypotheses (tests/golden/c1_beam_lm.npz), nnet.RNNLM's state_dict against the reference's key lists, the searcher's constructor,
the host loop with an LM on CPU modules, and the workspace size of the fused search."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beam_lm_ref as BL  # noqa: E402
from tiny_lm import TinyLM  # noqa: E402

dec = importlib.import_module("ts-asr_amd.decoders")
nnet = importlib.import_module("ts-asr_amd.nnet")


def tolerance(hyps, scores, ref_hyps, ref_scores):
    """The project's rule between two searches of the same utterances: equal sequence or normalised score within 5e-4, every score
    within 1e-3, at least half of the sequences equal."""
    exact = 0
    for b in range(len(ref_hyps)):
        exact += hyps[b] == ref_hyps[b]
        assert hyps[b] == ref_hyps[b] or abs(scores[b] - ref_scores[b]) < 5e-4, b
        assert abs(scores[b] - ref_scores[b]) < 1e-3, b
    assert 2 * exact >= len(ref_hyps), exact
    return exact


CASES = [(name, T, beam) for name in BL.LM_CONFIGS for T in BL.FRAMES for beam in BL.BEAMS]


@pytest.mark.parametrize("name,T,beam", CASES, ids=[BL.case_key(*c) for c in CASES])
def test_float64_search_equals_the_reference(golden, name, T, beam):
    """The float64 restatement gives the reference's n-best exactly (every hypothesis of every rank, and as many of them), scores within
    1e-3 (the reference adds float32 terms; its own float32 and float64 runs differ by up to 2.6e-4 on these cases)."""
    g = golden["c1_beam_lm"]
    enc = golden["c1_chain_cat"]["enc_proj"][:, :T]
    w = BL.predictor_weights(float(g["blank_bias"]))
    lm = BL.lm_weights(name)
    for b in range(enc.shape[0]):
        ref_hyps, ref_scores = BL.fixture_case(g, name, T, beam, b)
        hyps, scores = BL.beam_search_lm(enc[b], w, lm, BL.LM_CONFIGS[name]["weight"], beam)
        assert hyps == ref_hyps, b
        assert np.abs(np.array(scores) - np.array(ref_scores)).max() < 1e-3


def test_the_lm_changes_the_hypotheses(golden):
    """The fixture is about the LM: without it the same search gives other hypotheses on every utterance."""
    g = golden["c1_beam_lm"]
    enc = golden["c1_chain_cat"]["enc_proj"][:, :24]
    w = BL.predictor_weights(float(g["blank_bias"]))
    for b in range(4):
        plain, _ = BL.beam_search_lm(enc[b], w, None, 0.0, 4)
        assert plain != BL.fixture_case(g, "l2b1e72", 24, 4, b)[0]


@pytest.mark.parametrize("name", sorted(BL.LM_CONFIGS))
def test_rnnlm_state_dict_is_the_references(golden, name):
    g = golden["c1_beam_lm"]
    c = BL.LM_CONFIGS[name]
    lm = nnet.RNNLM(29, embedding_dim=c["emb"], rnn_layers=c["layers"], rnn_neurons=c["hidden"], dnn_blocks=c["blocks"], dnn_neurons=c["dnn"])
    sd = lm.state_dict()
    assert list(sd) == [str(k) for k in g[f"keys_{name}"]]
    assert [list(v.shape) for v in sd.values()] == [[int(d) for d in row if d > 0] for row in g[f"shapes_{name}"]]
    assert list(sd) == list(BL.lm_shapes(c))
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in BL.lm_weights(name).items()}, strict=True)


def test_rnnlm_defaults_are_the_references():
    lm = nnet.RNNLM(output_neurons=29)
    assert lm.embedding.embedding_dim == 128 and lm.rnn.rnn.num_layers == 2 and lm.rnn.rnn.hidden_size == 1024 and lm.rnn.rnn.dropout == 0.15
    assert len(lm.dnn_layers()) == 1 and lm.out.w.in_features == 512 and lm.return_hidden is False and lm.dropout.p == 0.15
    assert isinstance(lm.dnn_layers()[0][2], torch.nn.LeakyReLU)
    hp = importlib.import_module("ts-asr_amd.hparams")
    assert hp._import("speechbrain.lobes.models.RNNLM.RNNLM") is nnet.RNNLM


def _searcher(lm=None, lm_weight=0.0, **kw):
    return dec.TransducerBeamSearcher([None, None, None], None, [None], blank_id=0, lm_module=lm, lm_weight=lm_weight, **kw)


def test_constructor_follows_the_reference():
    with pytest.raises(ValueError, match="Language model"):
        _searcher(None, 0.5)
    s = _searcher(TinyLM(7), 0.0)                # an LM with weight 0 is accepted and unused
    assert s.lm_weight == 0.0 and s._beam_start() == ([0], 0.0, None)
    assert _searcher(TinyLM(7), 0.4)._beam_start(True) == ([0], 0.0, None, [], None)
    assert _searcher()._beam_start(True) == ([0], 0.0, None, [])


class _Joint(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.nonlinearity = torch.nn.LeakyReLU(0.01)

    def forward(self, a, b):
        return self.nonlinearity(a + b)


def test_host_loop_with_an_lm_on_cpu_modules():
    """The host loop with a non-RNNLM module on plain CPU modules against the float64 restatement (tolerance rule on every rank);
    lm_weight = 0 gives the bits of the searcher without the LM; the timed form and beam_stream in pieces give the untimed offline
    bits, so the LM state rides behind the frames without disturbing them."""
    torch.manual_seed(3)
    V, H, J = 7, 12, 16
    emb, lstm = torch.nn.Embedding(V, V), torch.nn.LSTM(V, H, batch_first=True)
    proj, head = torch.nn.Linear(H, J), torch.nn.Linear(J, V)
    with torch.no_grad():
        emb.weight.copy_(torch.eye(V))
        for p in list(lstm.parameters()) + list(proj.parameters()) + list(head.parameters()):
            p.mul_(2.0)
        head.bias[0] += 3.0
    lm = TinyLM(V).eval()
    f = lambda t: t.detach().double().numpy()  # noqa: E731
    w = dict(emb=f(emb.weight), w_ih=f(lstm.weight_ih_l0), w_hh=f(lstm.weight_hh_l0), b_ih=f(lstm.bias_ih_l0), b_hh=f(lstm.bias_hh_l0),
             w_proj=f(proj.weight), b_proj=f(proj.bias), w_head=f(head.weight), b_head=f(head.bias))
    make = lambda lm_module, weight: dec.TransducerBeamSearcher([emb, lstm, proj], _Joint(), [head], blank_id=0, beam_size=3, nbest=3,  # noqa: E731
                                                                lm_module=lm_module, lm_weight=weight)
    enc = torch.randn(2, 9, J, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        plain, zero, fused = make(None, 0.0)(enc), make(lm, 0.0)(enc), make(lm, 0.6)(enc)
        assert zero[2] == plain[2] and zero[3] == plain[3]
        assert fused[2] != plain[2]
        for b in range(2):
            ref_hyps, ref_scores = BL.beam_search_lm(enc[b].double().numpy(), w, {}, 0.6, 3, step=lm.numpy_step())
            assert len(fused[2][b]) == len(ref_hyps)
            tolerance(fused[2][b], fused[3][b], ref_hyps, ref_scores)
        s = make(lm, 0.6)
        timed = s.forward_timed(enc)
        assert timed[2] == fused[2] and timed[3] == fused[3]
        assert all(fr == sorted(fr) and len(fr) == len(h) for nb, nf in zip(timed[2], timed[5]) for h, fr in zip(nb, nf))
        for frames in (False, True):
            state = None
            for t0 in range(0, 9, 4):
                _, state = s.beam_stream(enc[:, t0:t0 + 4], state, return_frames=frames)
            assert state["nbest"] == fused[2] and state["scores"] == fused[3]
            assert not frames or state["frames"] == timed[5]


def test_lm_workspace_bytes():
    """The fused search's workspace: the plain (or timed) layout plus 64 + 2 L Hl floats in each of the cap + beam slots; the recipe's
    figure (cap 512, beam 15, the reference-default LM: 527 x (64 + 4096) floats per utterance); C side and wrapper agree."""
    ops = importlib.import_module("ts-asr_amd.ops")
    lib = importlib.import_module("ts-asr_amd._capi").lib()
    a16 = lambda v: -(-v // 16) * 16  # noqa: E731
    for B, T, H, J, beam, cap, L, Hl in ((32, 250, 512, 640, 15, 512, 2, 1024), (1, 1, 4, 4, 2, 2, 1, 4), (3, 40, 128, 160, 4, 37, 3, 40)):
        for times in (0, 1):
            nodes = 1 + (T + 1) * beam + cap
            base = B * (a16(64 + 24 * beam) + a16(8 * nodes) + 4 * (cap + beam) * (J + 2 * H) + times * a16(4 * nodes))
            assert ops.beam_workspace_bytes(B, T, H, J, 29, beam, cap, times=bool(times)) == base
            want = base + B * 4 * (cap + beam) * (64 + 2 * L * Hl)
            assert lib.tsasr_beam_search_workspace_bytes(B, T, H, J, 29, beam, cap, L, Hl, times, 0, 0) == want
            assert ops.beam_workspace_bytes(B, T, H, J, 29, beam, cap, L, Hl, bool(times)) == want
            # lm_layers = 0 means no LM: the LM layout without layers is the plain one (lm_hidden is not read)
            assert lib.tsasr_beam_search_workspace_bytes(B, T, H, J, 29, beam, cap, 0, Hl, times, 0, 0) == base
            assert ops.beam_workspace_bytes(B, T, H, J, 29, beam, cap, 0, Hl, bool(times)) == base
    per_utt = ops.beam_workspace_bytes(1, 250, 512, 640, 29, 15, 512, 2, 1024) - ops.beam_workspace_bytes(1, 250, 512, 640, 29, 15, 512)
    assert per_utt == 527 * (64 + 4096) * 4 == 8_769_280
    assert lib.tsasr_beam_search_workspace_bytes(32, 250, 512, 640, 29, 15, 512, 0, 1024, 0, 0, 0) == \
        lib.tsasr_beam_search_workspace_bytes(32, 250, 512, 640, 29, 15, 512, 0, 0, 0, 0, 0) == 113_355_776
    assert ops.beam_workspace_bytes(32, 250, 512, 640, 29, 15, 512, 2, 0) == 0
