"""tests/helpers/search_times_ref.py (the float64 path log-probability that judges every emission frame the searches report) against the
oracle's brute force over all alignments, and the host side of the timestamp interface that needs no GPU. No GPU."""
import importlib
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import search_times_ref as SR  # noqa: E402
from oracle import rnnt_ref  # noqa: E402


def random_model(rng, V=5, E=5, H=6, J=8):
    g = lambda *s: rng.standard_normal(s) * 0.7  # noqa: E731
    return dict(emb=np.eye(V, E), w_ih=g(4 * H, E), w_hh=g(4 * H, H), b_ih=g(4 * H), b_hh=g(4 * H), w_proj=g(J, H), b_proj=g(J),
                w_head=g(V, J), b_head=g(V))


@pytest.mark.parametrize("T", [3, 4])
@pytest.mark.parametrize("n", [2, 3])
def test_paths_sum_to_the_lattice_total(T, n):
    """exp(path_logp) summed over every non-decreasing frame assignment = exp(-cost) of the oracle's brute force over all monotone
    alignments on the same float64 logits, to 1e-10 relative; the oracle's C forward-backward (float32 logits in) agrees to its input
    rounding. Pins the helper's node indexing (token i is scored at node (f_i, i - 1), frame t's blank at (t, #{f_i <= t}))."""
    rng = np.random.default_rng(1000 * T + n)
    V, blank, slope = 5, 0, 0.01
    for trial in range(3):
        w = random_model(rng, V=V)
        if trial == 2:
            w["b_ih"] = w["b_hh"] = w["b_proj"] = w["b_head"] = None
        enc = rng.standard_normal((T, 8))
        tokens = rng.integers(1, V, size=n).tolist()
        pn = SR.predictor_outputs(tokens, w, blank)
        logits = np.stack([np.stack([SR.joint_logits(enc[t], pn[u], w, slope) for u in range(n + 1)]) for t in range(T)])
        total, count = 0.0, 0
        for frames in itertools.combinations_with_replacement(range(T), n):
            lp, labels = SR.path_logp(enc, tokens, list(frames), w, blank, slope)
            assert labels >= lp            # the blanks only subtract
            total += np.exp(lp)
            count += 1
        want = np.exp(-rnnt_ref.brute_force_cost(logits, tokens, T, n, blank))
        assert count > 1
        assert abs(total - want) <= 1e-10 * want, (total, want)
        cost32, _ = rnnt_ref.rnnt_costs_grads(logits[None].astype(np.float32), np.array([tokens], np.int32), np.array([T], np.int32),
                                              np.array([n], np.int32), blank, want_grads=False)
        assert abs(-np.log(total) - float(cost32[0])) <= 1e-4


def test_path_logp_refuses_bad_frames():
    rng = np.random.default_rng(7)
    w = random_model(rng)
    enc = rng.standard_normal((3, 8))
    for frames in ([1, 0], [0, 3], [-1, 0], [0]):
        with pytest.raises(ValueError):
            SR.path_logp(enc, [1, 2], frames, w, 0, 0.01)
    lp, labels = SR.path_logp(enc, [], [], w, 0, 0.01)      # the empty hypothesis: T blanks from the primed predictor
    assert labels == 0.0 and lp < 0.0


# ---- the host loop and the interface (CPU modules, no kernel) --------------------------------------------------------------------
class _Joint(torch.nn.Module):
    """LeakyReLU(enc + pn), as rnnt.Transducer_joint("sum") (whose kernels run on the device only)."""

    def __init__(self):
        super().__init__()
        self.nonlinearity = torch.nn.LeakyReLU(0.01)

    def forward(self, a, b):
        return self.nonlinearity(a + b)


@pytest.fixture(scope="module")
def host_searcher():
    """A small network of plain torch modules on the CPU (the product's modules run on the device only): the searcher's host routes
    take any modules with the predictor's and the joint's call shapes."""
    dec = importlib.import_module("ts-asr_amd.decoders")
    torch.manual_seed(3)
    V, H, J = 7, 12, 16
    emb = torch.nn.Embedding(V, V)
    lstm = torch.nn.LSTM(V, H, batch_first=True)
    proj, head = torch.nn.Linear(H, J), torch.nn.Linear(J, V)
    with torch.no_grad():
        emb.weight.copy_(torch.eye(V))
        for p in list(lstm.parameters()) + list(proj.parameters()) + list(head.parameters()):
            p.mul_(2.0)
        head.bias[0] += 3.0      # blank stays among the best symbols, so the expansion loop of every frame ends
    mods = torch.nn.ModuleList([emb, lstm, proj, head]).eval()

    def make(beam, nbest=3):
        s = dec.TransducerBeamSearcher([emb, lstm, proj], _Joint(), [head], blank_id=0, beam_size=beam, nbest=nbest, state_beam=2.3,
                                       expand_beam=2.3)
        pn, calls = s._pn, [0]

        def counted(tok, hidden):      # a search that does not end fails the test instead of holding the suite
            calls[0] += 1
            assert calls[0] <= 5000, "the host loop's expansion does not end on these inputs"
            return pn(tok, hidden)
        s._pn = counted
        return s
    return make, mods, (V, H, J)


def _weights(mods):
    emb, lstm, proj, head = mods
    f = lambda t: t.detach().double().numpy()  # noqa: E731
    return dict(emb=f(emb.weight), w_ih=f(lstm.weight_ih_l0), w_hh=f(lstm.weight_hh_l0), b_ih=f(lstm.bias_ih_l0), b_hh=f(lstm.bias_hh_l0),
                w_proj=f(proj.weight), b_proj=f(proj.bias), w_head=f(head.weight), b_head=f(head.bias))


def test_host_loop_frames_cpu(host_searcher):
    """The host loop on the CPU: forward_timed's first four values are forward's; every n-best entry's score x (n + 1) is the float64
    path log-probability of its (tokens, frames) (fp32 modules: 1e-4); greedy frames are strictly increasing; beam_stream and
    greedy_stream in pieces give the offline frames; mixing return_frames within a stream raises."""
    make, mods, (V, H, J) = host_searcher
    torch.manual_seed(11)
    enc = torch.randn(2, 9, J)
    w = _weights(mods)
    with torch.no_grad():
        s = make(3)
        plain, timed = s(enc), s.forward_timed(enc)
        assert timed[0] == plain[0] and timed[2] == plain[2] and timed[3] == plain[3] and float(timed[1]) == float(plain[1])
        assert [n[0] for n in timed[5]] == timed[4]
        for b in range(2):
            for toks, sc, fr in zip(timed[2][b], timed[3][b], timed[5][b]):
                assert len(fr) == len(toks) and all(0 <= f < 9 for f in fr) and fr == sorted(fr)
                lp, _ = SR.path_logp(enc[b].double().numpy(), toks, fr, w, 0, 0.01)
                assert abs(sc * (len(toks) + 1) - lp) <= 1e-4, (sc * (len(toks) + 1), lp)
        state = None
        for t0 in range(0, 9, 4):
            best, state = s.beam_stream(enc[:, t0:t0 + 4], state, return_frames=True)
        assert state["nbest"] == timed[2] and state["frames"] == timed[5]
        with pytest.raises(ValueError, match="return_frames"):
            s.beam_stream(enc[:, :1], state)
        _, plain_state = s.beam_stream(enc[:, :4])
        assert "frames" not in plain_state and len(plain_state["beams"][0][0]) == 3
        with pytest.raises(ValueError, match="return_frames"):
            s.beam_stream(enc[:, 4:8], plain_state, return_frames=True)
        g = make(1)
        gp, gt = g(enc), g.forward_timed(enc)
        assert gt[0] == gp[0] and gt[5] is None and gt[2] is None
        for toks, fr in zip(gt[0], gt[4]):
            assert len(fr) == len(toks) and all(a < b for a, b in zip(fr, fr[1:]))
        state, acc_t, acc_f = None, [[], []], [[], []]
        for t0 in range(0, 9, 4):
            new, new_f, state = g.greedy_stream(enc[:, t0:t0 + 4], state, return_frames=True)
            for b in range(2):
                acc_t[b] += new[b]
                acc_f[b] += new_f[b]
        assert acc_t == gt[0] and acc_f == gt[4]
        with pytest.raises(ValueError, match="return_frames"):      # (an untimed call would leave the frame count behind)
            g.greedy_stream(enc[:, :4], state)
        out = g.greedy_stream(enc[:, :4])
        assert len(out) == 2 and "frames_done" not in out[1]
        with pytest.raises(ValueError, match="return_frames"):
            g.greedy_stream(enc[:, 4:8], out[1], return_frames=True)


def test_streaming_frames_need_timestamps():
    """frames() / nbest_frames() without start(timestamps=True) raise RuntimeError (no device needed to say so)."""
    streaming = importlib.import_module("ts-asr_amd.streaming")
    st = streaming.StreamingTranscriber.__new__(streaming.StreamingTranscriber)
    st.search, st.timestamps, st.B, st.search_state = "beam", False, 1, None
    with pytest.raises(RuntimeError, match="timestamps"):
        st.frames()
    with pytest.raises(RuntimeError, match="timestamps"):
        st.nbest_frames()
    st.timestamps, st.hyp_frames = True, [[3, 4]]
    assert st.frames() == [[3, 4]] and st.nbest_frames() == [[[]]]


def test_timed_workspace_bytes_formula():
    """The timed workspace is the untimed one plus one int per tree node per utterance, 0 for a non-positive argument; the C side and
    the Python wrapper agree."""
    ops = importlib.import_module("ts-asr_amd.ops")
    capi = importlib.import_module("ts-asr_amd._capi")
    lib = capi.lib()
    a16 = lambda v: -(-v // 16) * 16  # noqa: E731
    for B, T, H, J, beam, cap in ((32, 250, 512, 640, 15, 512), (1, 1, 4, 4, 2, 2), (3, 40, 128, 160, 4, 37), (6, 4000, 512, 640, 15, 512)):
        nodes = 1 + (T + 1) * beam + cap
        untimed = B * (a16(64 + 24 * beam) + a16(8 * nodes) + 4 * (cap + beam) * (J + 2 * H))
        want = untimed + B * a16(4 * nodes)
        assert lib.tsasr_beam_search_workspace_bytes(B, T, H, J, 29, beam, cap, 0, 0, 1, 0, 0) == want
        assert ops.beam_workspace_bytes(B, T, H, J, 29, beam, cap, times=True) == want
        assert want >= lib.tsasr_beam_search_workspace_bytes(B, T, H, J, 29, beam, cap, 0, 0, 0, 0, 0) == untimed
    for B, T, H, J, beam, cap in ((0, 250, 512, 640, 15, 512), (32, -1, 512, 640, 15, 512), (32, 250, 512, 640, 15, 0)):
        assert lib.tsasr_beam_search_workspace_bytes(B, T, H, J, 29, beam, cap, 0, 0, 1, 0, 0) == 0
        assert ops.beam_workspace_bytes(B, T, H, J, 29, beam, cap, times=True) == 0


def test_write_hyp_ctm(tmp_path):
    """train_tsasr.write_hyp_ctm: one line per recognised word from the emission frames kept by the TEST stage, with the --align_file
    rules (word pieces through align.word_spans, token ids without a tokenizer, reused utterance ids kept apart)."""
    import types
    tt = importlib.import_module("train_tsasr")
    metrics = importlib.import_module("ts-asr_amd.metrics")
    times = [(["a", "b"], [[1, 2, 3, 1], []], [[0, 0, 2, 5], []]), (["a", "c"], [[3], [2, 2]], [[7], [1, 4]])]
    brain = types.SimpleNamespace(hyp_times=times, tokenizer=None)
    path = tmp_path / "h.ctm"
    assert tt.write_hyp_ctm(brain, {"hop_length": 10}, str(path)) == 7
    assert path.read_text().splitlines() == ["a 1 0.000 0.040 1", "a 1 0.000 0.040 2", "a 1 0.080 0.040 3", "a 1 0.200 0.040 1",
                                             "a-1 1 0.280 0.040 3", "c-1 1 0.040 0.040 2", "c-1 1 0.160 0.040 2"]
    brain.tokenizer = metrics.CharTokenizer(["<b>", "▁", "h", "i"])
    assert tt.write_hyp_ctm(brain, {"hop_length": 10}, str(path)) == 3
    assert path.read_text().splitlines() == ["a 1 0.000 0.120 hi", "a-1 1 0.280 0.040 i", "c-1 1 0.040 0.160 hh"]
