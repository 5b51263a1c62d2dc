"""Contextual biasing of the device beam search on the MI355X (csrc/search.hip: tsasr_beam_search with bias): the device route against the
float64 restatement (tests/helpers/beam_bias_ref.py) and against the host loop, which is the definition; the bit identities (streams in
pieces, timed and untimed, per-utterance graph lists, no graph = today's entry points); workspace bounds; overflow and the host
re-decode; StreamingTranscriber in lockstep and in slots; the launcher's refusals; the recipe."""
import contextlib
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import __graft_entry__ as entry  # noqa: E402
import beam_bias_ref as BB  # noqa: E402
import beam_lm_ref as BL  # noqa: E402
import beam_wide_ref as BW  # noqa: E402
import joint_wide_ref as JW  # noqa: E402
from oracle.golden_recipe import det_tensor  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dec = importlib.import_module("ts-asr_amd.decoders")
ops = importlib.import_module("ts-asr_amd.ops")
nnet = importlib.import_module("ts-asr_amd.nnet")
rnnt = importlib.import_module("ts-asr_amd.rnnt")
capi = importlib.import_module("ts-asr_amd._capi")
biasing = importlib.import_module("ts-asr_amd.biasing")
ContextGraph = biasing.ContextGraph
V = 29
LM_NAME, LM_WEIGHT = "l2b1e72", 0.3


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def bits(scores):
    return [np.array(x, np.float64).tobytes() for x in scores]


def tolerance(hyps, scores, ref_hyps, ref_scores):
    """The project's rule (test_beam_lm_cpu.py::tolerance): equal sequence or normalised score within 5e-4, every score within 1e-3,
    at least half of the sequences equal."""
    exact = 0
    for b in range(len(ref_hyps)):
        exact += hyps[b] == ref_hyps[b]
        assert hyps[b] == ref_hyps[b] or abs(scores[b] - ref_scores[b]) < 5e-4, b
        assert abs(scores[b] - ref_scores[b]) < 1e-3, b
    assert 2 * exact >= len(ref_hyps), exact
    return exact


def tolerance_ranks(nb, sc, ref_nb, ref_sc):
    assert [len(n) for n in nb] == [len(n) for n in ref_nb]
    exact = []
    for r in range(max(len(n) for n in ref_nb)):
        rows = [b for b in range(len(ref_nb)) if len(ref_nb[b]) > r]
        exact.append(tolerance([nb[b][r] for b in rows], [sc[b][r] for b in rows], [ref_nb[b][r] for b in rows], [ref_sc[b][r] for b in rows]))
    return exact


@pytest.fixture(scope="module")
def brains():
    out = {}

    def get(dtype):
        if dtype not in out:
            out[dtype] = entry._config1_brain(DEV, dtype)
        brain, h = out[dtype]
        brain._setup_dtype()           # the compute dtype is process-global
        return brain, h
    yield get
    nnet.set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module")
def lm():
    c = BL.LM_CONFIGS[LM_NAME]
    m = nnet.RNNLM(V, embedding_dim=c["emb"], dropout=0.0, rnn_layers=c["layers"], rnn_neurons=c["hidden"], return_hidden=True,
                   dnn_blocks=c["blocks"], dnn_neurons=c["dnn"])
    m.load_state_dict({k: T(v) for k, v in BL.lm_weights(LM_NAME).items()}, strict=True)
    return m.to(DEV).eval()


def searcher(m, beam, lm=None, lm_weight=0.0, nbest=BB.NBEST, cap=dec.BEAM_CAP):
    return dec.TransducerBeamSearcher([m.embedding, m.decoder, m.decoder_proj], m.joiner, [m.transducer_head], blank_id=0, beam_size=beam,
                                      nbest=nbest, lm_module=lm, lm_weight=lm_weight, state_beam=2.3, expand_beam=2.3, cap=cap)


@contextlib.contextmanager
def blank_shift(head, shift):
    """The golden fixtures raise the head's blank bias so that the search's frames close."""
    with torch.no_grad():
        head.w.bias[0] += shift
    try:
        yield
    finally:
        with torch.no_grad():
            head.w.bias[0] -= shift


def inputs(golden, name):
    c = golden["c1_chain_cat"]["enc_proj"]
    if name == "golden50":
        return np.ascontiguousarray(c)                                    # B = 4, T = 50
    base = np.concatenate([c[:, ::-1], np.roll(c, 1, axis=0)], 0)[:6, :40]
    return base + det_tensor("beam.enc_proj.2", base.shape, 0.05)         # "second": B = 6, T = 40


_REF = {}


def reference(golden, name, beam, with_lm=False):
    """(enc, the batch's graph, float64 biased (n-best, scores) per utterance) of an input, computed once and left unchanged."""
    key = (name, beam, with_lm)
    if key not in _REF:
        enc = inputs(golden, name)
        w = BL.predictor_weights(float(golden["c1_beam_lm"]["blank_bias"]))
        lw, weight = (BL.lm_weights(LM_NAME), LM_WEIGHT) if with_lm else (None, 0.0)
        plain = [BL.beam_search_lm(enc[b], w, lw, weight, beam) for b in range(enc.shape[0])]
        graph = ContextGraph(BB.test_phrases([p[0] for p in plain], V), BB.BIAS_WEIGHT)
        biased = [BB.beam_search_bias(enc[b], w, BB.graph_arrays(graph), beam, lm=lw, lm_weight=weight) for b in range(enc.shape[0])]
        assert any(r[0] != p[0] for r, p in zip(biased, plain))
        _REF[key] = (enc, graph, biased)
    return _REF[key]


# ---- device against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [2, 4, 15])
@pytest.mark.parametrize("name", ["golden50", "second"])
def test_device_bias_vs_float64(brains, golden, name, beam):
    brain, h = brains("fp32")
    enc, graph, ref = reference(golden, name, beam)
    m = brain.modules
    x = T(enc).float().to(DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, beam)
        assert s._device_beam_ok(x, bias=True)
        before = dec.BEAM_HOST_REDECODES["utterances"]
        best, mean, nb, sc = s(x, bias=graph)
        assert dec.BEAM_HOST_REDECODES["utterances"] == before
        assert s(x)[2] != nb
    assert best == [n[0] for n in nb] and float(mean) == float(torch.tensor([q[0] for q in sc]).exp().mean())
    exact = tolerance_ranks(nb, sc, [r[0] for r in ref], [r[1] for r in ref])
    print(f"BIAS {name} beam {beam}: device fp32 vs float64, utterances exact per rank {exact} of {enc.shape[0]}")


@pytest.mark.parametrize("beam", [2, 4, 15])
def test_device_bias_lm_vs_float64(brains, lm, golden, beam):
    brain, h = brains("fp32")
    enc, graph, ref = reference(golden, "second", beam, with_lm=True)
    m = brain.modules
    x = T(enc).float().to(DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, beam, lm, LM_WEIGHT)
        assert s._device_beam_ok(x, bias=True)
        _, _, nb, sc = s(x, bias=graph)
    exact = tolerance_ranks(nb, sc, [r[0] for r in ref], [r[1] for r in ref])
    print(f"BIAS+LM second beam {beam}: device fp32 vs float64, utterances exact per rank {exact} of {enc.shape[0]}")


_WIDE = {}


def wide_case(name, beam=4):
    """(searcher, enc, graph, float64 biased results) of a beam_wide_ref case."""
    if name not in _WIDE:
        Vw, E, H, J, _ = JW.GREEDY_CASES[BW.CASES[name]["net"]]
        net = BW.case_net(name, beam)
        t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in net.items()}
        emb = nnet.Embedding(Vw, consider_as_one_hot=True, blank_id=0) if E is None else nnet.Embedding(Vw, embedding_dim=E)
        if E is not None:
            emb.Embedding.load_state_dict({"weight": t["emb"]})
        lstm = nnet.LSTM(H, input_size=emb.embedding_dim)
        lstm.rnn.load_state_dict({"weight_ih_l0": t["w_ih"], "weight_hh_l0": t["w_hh"], "bias_ih_l0": t["b_ih"], "bias_hh_l0": t["b_hh"]})
        proj, head = nnet.Linear(J, input_size=H), nnet.Linear(Vw, input_size=J)
        proj.load_state_dict({"w.weight": t["w_proj"], "w.bias": t["b_proj"]})
        head.load_state_dict({"w.weight": t["w_head"], "w.bias": t["b_head"]})
        mods = [x.to(DEV).eval() for x in (emb, lstm, proj, head)]
        s = dec.TransducerBeamSearcher(mods[:3], rnnt.Transducer_joint(), [mods[3]], blank_id=0, beam_size=beam, nbest=BB.NBEST)
        plain = BW.run_case(name, beam)
        graph = ContextGraph(BB.test_phrases([r["nbest"] for r in plain], Vw), BB.BIAS_WEIGHT)
        enc = np.asarray(net["enc"])
        ref = [BB.beam_search_bias(enc[b], net, BB.graph_arrays(graph), beam, slope=JW.SLOPE) for b in range(enc.shape[0])]
        assert any(r[0] != p["nbest"] for r, p in zip(ref, plain))
        _WIDE[name] = (s, t["enc"], graph, ref)
    return _WIDE[name]


@pytest.mark.parametrize("name", ["v64", "v100"])
def test_device_bias_wide_vs_float64(name):
    s, enc, graph, ref = wide_case(name)
    x = enc.float().to(DEV)
    with torch.no_grad():
        assert s._beam_is_wide() and s._device_beam_ok(x, bias=True)
        _, _, nb, sc = s(x, bias=graph)
        timed = s.forward_timed(x, bias=graph)
    assert timed[2] == nb and bits(timed[3]) == bits(sc)
    exact = tolerance_ranks(nb, sc, [r[0] for r in ref], [r[1] for r in ref])
    print(f"BIAS wide {name} beam 4: device fp32 vs float64, utterances exact per rank {exact} of {x.shape[0]}")


# ---- device against the host loop ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_bias_equals_host_loop(brains, golden, dtype, monkeypatch):
    """fp32, T = 24: the rule on every rank. bf16, the first 12 frames: at least 3 of 4 utterances identical (the plain beam test's form)."""
    brain, h = brains(dtype)
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    _, graph, _ = reference(golden, "golden50", 4)
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:, : 24 if dtype == "fp32" else 12].to(DEV, dt)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4)
        s.bias = graph
        assert s._device_beam_ok(enc, bias=True)
        _, _, nb_k, sc_k = s(enc)
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        assert not s._device_beam_ok(enc, bias=True)
        _, _, nb_h, sc_h = s(enc)
    if dtype == "fp32":
        print("BIAS device vs host loop fp32: utterances exact per rank", tolerance_ranks(nb_k, sc_k, nb_h, sc_h))
    else:
        same = sum(a == b for a, b in zip(nb_k, nb_h))
        print("BIAS device vs host loop bf16: utterances identical", same)
        assert same >= 3, (same, nb_k, nb_h)


# ---- bit identities -----------------------------------------------------------------------------------------------------------------------
def test_stream_pieces_timed_and_lists_bit_identical(brains, golden):
    """A biased stream in pieces (cuts at 1, 7 and 8 frames, a zero-frame read-out between them) equals one call: n-best, score bits
    and frames; timed equals untimed; a list of per-utterance graphs (one None, one empty) equals single-utterance calls."""
    brain, h = brains("fp32")
    enc_np, graph, _ = reference(golden, "second", 4)
    enc = T(enc_np).float().to(DEV)[:, :24]
    B, Tn = enc.shape[:2]
    other = ContextGraph([[5, 6], [7], [7, 8, 9]], 2.0)
    graphs = [graph, None, other, ContextGraph([], 1.0), graph, other]
    m = brain.modules
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4)
        whole = s(enc, bias=graphs)
        timed = s.forward_timed(enc, bias=graphs)
        assert timed[2] == whole[2] and bits(timed[3]) == bits(whole[3]) and float(timed[1]) == float(whole[1])
        assert all(fr == sorted(fr) and len(fr) == len(hy) for nb, nf in zip(timed[2], timed[5]) for hy, fr in zip(nb, nf))
        plain = s(enc)
        for b in range(B):
            alone = s(enc[b:b + 1], bias=graphs[b])
            assert alone[2][0] == whole[2][b] and bits(alone[3][0]) == bits(whole[3][b]), b
        for b in (1, 3):                                               # None and the empty graph: the plain search's bits
            assert whole[2][b] == plain[2][b] and bits(whole[3][b]) == bits(plain[3][b])
        assert whole[2][0] != plain[2][0]
        for frames in (False, True):
            state, t0 = None, 0
            for n in (1, 7, 0, 8, Tn - 16):
                best, state = s.beam_stream(enc[:, t0:t0 + max(n, 1)], state, torch.full((B,), n, dtype=torch.int32), max_frames=Tn,
                                            return_frames=frames, bias=graphs if t0 != 8 else None)
                if n == 0:
                    assert (state["nbest"], bits(state["scores"])) == before
                before = (state["nbest"], bits(state["scores"]))
                t0 += n
            assert "dev" in state and state["nbest"] == whole[2] and bits(state["scores"]) == bits(whole[3])
            assert best == whole[0]
            assert not frames or state["frames"] == timed[5]
        with pytest.raises(ValueError, match="another graph"):
            s.beam_stream(enc[:, :1], state, bias=[other] * B, return_frames=True)


class _Recorder:
    """Stands in for the loaded library and notes, per tsasr_beam_search call, which form it took: whether n_valid, frames, lm and bias
    were NULL, and the value of wide."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def tsasr_beam_search(self, *a):
        assert len(a) == 40
        self.calls.append(dict(n_valid=a[12] is None, frames=a[35] is None, lm=a[36] is None, bias=a[38] is None, wide=a[39]))
        return self._lib.tsasr_beam_search(*a)

    def __getattr__(self, name):
        return getattr(self._lib, name)


def test_no_graph_is_todays_entry_points(brains, golden, monkeypatch):
    """A batch whose entries are all None or empty graphs equals the plain search, bit for bit, and makes the calls of the plain
    search, each without a graph (bias NULL); a real graph passes its descriptor in every call."""
    brain, h = brains("fp32")
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:, :24].to(DEV)
    rec = _Recorder(capi.lib())
    monkeypatch.setattr(capi, "lib", lambda: rec)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4)
        plain, plain_t = s(enc), s.forward_timed(enc)
        want_calls = list(rec.calls)
        assert want_calls and all(c["bias"] and c["lm"] and c["wide"] == 0 for c in want_calls)
        assert [c["frames"] for c in want_calls if c["n_valid"]] == [True, False]        # the untimed and the timed offline launch
        del rec.calls[:]
        nothing = [None, ContextGraph([], 1.0), None, ContextGraph([], 3.0)]
        a, a_t = s(enc, bias=nothing), s.forward_timed(enc, bias=ContextGraph([], 1.0))
        assert rec.calls == want_calls
        assert a[2] == plain[2] and bits(a[3]) == bits(plain[3]) and float(a[1]) == float(plain[1])
        assert a_t[2] == plain_t[2] and bits(a_t[3]) == bits(plain_t[3]) and a_t[5] == plain_t[5]
        del rec.calls[:]
        s(enc, bias=ContextGraph([[3, 4]], 1.0))
        assert rec.calls and not any(c["bias"] for c in rec.calls)


def test_workspace_bounds_and_garbage_start(brains, golden):
    """The biased search stays inside its tsasr_beam_search_workspace_bytes (a 0xA5 canary behind it is intact), and the offline call
    on a workspace full of garbage gives the bits of the call on a fresh one (it starts the workspace itself, the trie states too)."""
    brain, h = brains("fp32")
    _, graph, _ = reference(golden, "golden50", 4)
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:, :24].to(DEV)
    B, Tn = enc.shape[:2]
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4)
        packed = biasing.pack([graph] * B, enc.device)
        for frames in (False, True):
            need = ops.beam_workspace_bytes(B, Tn, 128, 160, V, 4, s.cap, 0, 0, frames, bias=True)
            assert need == capi.lib().tsasr_beam_search_workspace_bytes(B, Tn, 128, 160, V, 4, s.cap, 0, 0, int(frames), 1, 0)
            ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
            got = s._device_beam_call(enc, ops.beam_search, ws[:need], frames=frames, bias=packed)
            assert got[2].tolist() == [0] * B
            assert bool((ws[need:] == 0xA5).all())
            want = s._device_beam_call(enc, ops.beam_search, frames=frames, bias=packed)
            assert got[0] == want[0] and bits(got[1]) == bits(want[1]) and tuple(got[3:]) == tuple(want[3:])
            with pytest.raises(ValueError, match="workspace"):
                s._device_beam_call(enc, ops.beam_search, ws[: need - 16], frames=frames, bias=packed)


def test_overflow_status_and_host_redecode(brains, golden, monkeypatch):
    """A cap that stops some utterances but not all: status 1 for those, the others bit-equal to the large-cap run; the searcher
    decodes the stopped ones again on the host loop with their own graph."""
    brain, h = brains("fp32")
    enc_np, graph, _ = reference(golden, "second", 4)
    m = brain.modules
    enc = T(enc_np).float()[:, :12].clone()
    enc[3:] = 0.0                      # blank wins every frame there: A never holds more than the beam
    enc = enc.to(DEV)
    other = ContextGraph([[5, 6], [7]], 2.0)
    graphs = [graph, other, graph, graph, None, other]
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, nbest=2)
        packed = biasing.pack(graphs, enc.device)
        full = s._device_beam_call(enc, ops.beam_search, bias=packed)
        assert full[2].tolist() == [0] * 6
        for cap in range(4, 64):
            s.cap = cap
            nb, sc, status = s._device_beam_call(enc, ops.beam_search, bias=packed)
            bad = [b for b in range(6) if status[b] != 0]
            if 0 < len(bad) < 6:
                break
        assert 0 < len(bad) < 6, "no cap separates the utterances"
        assert all(int(status[b]) == 1 for b in bad), status
        assert all(nb[b] == full[0][b] and bits(sc[b]) == bits(full[1][b]) for b in range(6) if b not in bad)
        before = dec.BEAM_HOST_REDECODES["utterances"]
        with pytest.warns(RuntimeWarning) if before == 0 else contextlib.nullcontext():
            _, _, nb_d, sc_d = s(enc, bias=graphs)
        assert dec.BEAM_HOST_REDECODES["utterances"] == before + len(bad)
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        _, _, nb_h, sc_h = s(enc, bias=graphs)
        _, _, nb_plain, _ = s(enc)
        monkeypatch.delenv("TSASR_BEAM_KERNEL")
        for b in bad:
            assert nb_d[b] == nb_h[b] and bits(sc_d[b]) == bits(sc_h[b])
        assert any(nb_h[b] != nb_plain[b] for b in bad)              # the re-decode used the graph


# ---- StreamingTranscriber -----------------------------------------------------------------------------------------------------------------
def _stream_setup(golden):
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal")
    s = h["beam_searcher"]
    s.beam_size, s.nbest = 4, 3
    with torch.no_grad():
        s.classifier_network[0].w.bias[0] += float(golden["c1_beam_lm"]["blank_bias"])
    feats = T(golden["c1_features"]["norm"]).to(DEV)
    spk = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)
    return brain, s, feats, spk


def test_streaming_lockstep_bias_equals_offline(golden, monkeypatch):
    streaming = importlib.import_module("ts-asr_amd.streaming")
    monkeypatch.setattr(ops, "STRICT_HIP", True)
    ops.LIB_FALLBACKS.clear()
    try:
        brain, s, feats, spk = _stream_setup(golden)
        B, F = feats.shape[:2]
        with torch.no_grad():
            def run(bias):
                st = streaming.StreamingTranscriber(brain, search="beam")
                st.start(B, max_frames=(F + 3) // 4, speaker_embs=spk, keep_encoder_out=True, bias=bias)
                for f0 in range(0, F, 32):
                    st.push(feats[:, f0:f0 + 32], last=f0 + 32 >= F)
                return st.finish(), st.nbest(), brain.modules.encoder_proj(st.encoder_out())
            _, (nb0, _), enc = run(None)
            graphs = [ContextGraph(BB.test_phrases([nb0[b]], V), 1.5) if b != 2 else None for b in range(B)]
            hyps, (nb, sc), _ = run(graphs)
            assert s._device_beam_ok(enc, bias=True)
            off_best, _, off_nb, off_sc = s(enc, bias=graphs)
            assert nb != nb0 and nb[2] == nb0[2]
            with pytest.raises(ValueError, match="search='beam'"):
                streaming.StreamingTranscriber(brain, search="greedy").start(B, max_frames=8, bias=graphs[0])
        assert hyps == off_best and nb == off_nb and bits(sc) == bits(off_sc)
        assert ops.LIB_FALLBACKS == {}
    finally:
        nnet.set_compute_dtype(torch.bfloat16)


def test_streaming_slots_bias_sessions(golden):
    """Slots: two sessions with different graphs and one without, admitted at different pushes, then a fourth with a new graph into
    a freed slot while the others run: each equals its own single-session run, bit for bit."""
    streaming = importlib.import_module("ts-asr_amd.streaming")
    NS, PUSH, MAXF, NP = 3, 32, 32, 3
    try:
        brain, s, feats, spk = _stream_setup(golden)
        Sm = spk.shape[1]

        def single(row, slot, graph):
            st = streaming.StreamingTranscriber(brain, search="beam")
            e = torch.zeros(NS, Sm, spk.shape[2], dtype=spk.dtype, device=DEV)
            e[slot] = spk[row]
            st.start(NS, MAXF, speaker_embs=e, speaker_embs_length=torch.ones(NS, dtype=torch.float32, device=DEV),
                     bias=None if graph is None else [graph if b == slot else None for b in range(NS)])
            for p in range(NP):
                f = torch.zeros(NS, PUSH, feats.shape[2], device=DEV)
                f[slot] = feats[row, p * PUSH:(p + 1) * PUSH]
                ml = torch.zeros(NS, dtype=torch.int64)
                ml[slot] = PUSH
                st.push(f, mel_lens=ml)
            nb, sc = st.nbest()
            return nb[slot], bits(sc[slot])

        with torch.no_grad():
            plain = {row: single(row, row % NS, None) for row in range(4)}
            g = {row: ContextGraph(BB.test_phrases([plain[row][0]], V), 1.5) for row in (0, 1, 3)}
            sess = {"a": dict(row=0, slot=0, graph=g[0], at=0), "b": dict(row=1, slot=1, graph=g[1], at=1),
                    "c": dict(row=2, slot=2, graph=None, at=2), "d": dict(row=3, slot=0, graph=g[3], at=3)}
            want = {n: single(v["row"], v["slot"], v["graph"]) for n, v in sess.items()}
            assert any(want[n][0] != plain[sess[n]["row"]][0] for n in "abd")
            assert want["c"] == plain[2]
            st = streaming.StreamingTranscriber(brain, search="beam")
            with pytest.raises(ValueError, match="bias=True"):
                st.start(NS, MAXF, slots=True, max_speaker_frames=Sm, bias=g[0])
            st.start(NS, MAXF, slots=True, max_speaker_frames=Sm, bias=True)
            got, done, owner = {}, {n: 0 for n in sess}, [None] * NS
            for tick in range(7):
                for n, v in sess.items():
                    if owner[v["slot"]] == n and done[n] == NP:
                        st.release(v["slot"])
                        nb, sc = st.nbest()
                        got[n], owner[v["slot"]] = (nb[v["slot"]], bits(sc[v["slot"]])), None
                for n, v in sess.items():
                    if v["at"] == tick:
                        assert owner[v["slot"]] is None
                        st.admit(v["slot"], speaker_embs=spk[v["row"]:v["row"] + 1], speaker_embs_length=torch.ones(1), bias=v["graph"])
                        owner[v["slot"]] = n
                if not any(owner):
                    break
                f = torch.zeros(NS, PUSH, feats.shape[2], device=DEV)
                for b, n in enumerate(owner):
                    if n is not None:
                        f[b] = feats[sess[n]["row"], done[n] * PUSH:(done[n] + 1) * PUSH]
                        done[n] += 1
                st.push(f, mel_lens=torch.full((NS,), PUSH, dtype=torch.int64))
            assert sorted(got) == sorted(sess)
            for n in sess:
                assert got[n] == want[n], n
            with pytest.raises(ValueError, match="bias=True"):
                st2 = streaming.StreamingTranscriber(brain, search="beam")
                st2.start(NS, MAXF, slots=True, max_speaker_frames=Sm)
                st2.admit(0, speaker_embs=spk[0:1], bias=g[0])
            with pytest.raises(ValueError, match="search='beam'"):
                streaming.StreamingTranscriber(brain, search="greedy").start(NS, MAXF, slots=True, max_speaker_frames=Sm, bias=True)
    finally:
        nnet.set_compute_dtype(torch.bfloat16)


# ---- the launcher's refusals --------------------------------------------------------------------------------------------------------------
def test_launcher_refuses_bad_bias_arguments(brains, golden):
    """Wrong dtypes, a base outside the packed rows, a descriptor without rows, a short workspace, a graph with the wrong ``wide``, a
    greedy stream state without counts: an error before anything is launched (the status words keep their fill). A NULL descriptor is
    the unbiased search, bit for bit. Unsorted child_tok is the one thing nobody checks on the device: the header says so,
    ContextGraph guarantees the order."""
    brain, h = brains("fp32")
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:2, :8].to(DEV).contiguous()
    B, Tn, J, H, E = 2, 8, 160, 128, 28
    graph = ContextGraph([[3, 4, 5], [3, 6]], 1.0)
    assert all(np.all(np.diff(graph.child_tok[graph.child_off[s]:graph.child_off[s + 1]]) > 0) for s in range(graph.num_states))
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4)
        table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)
        good = biasing.pack([graph, None], enc.device)

        def call(desc, ws_delta=0, wide=False, out=None):
            need = ops.beam_workspace_bytes(B, Tn, H, J, V, 4, s.cap, bias=True)
            ws = torch.empty(need + ws_delta, dtype=torch.uint8, device=DEV)
            hyps = torch.zeros(B, 3, 32, dtype=torch.int32, device=DEV)
            lens = torch.zeros(B, 3, dtype=torch.int32, device=DEV)
            scores = torch.zeros(B, 3, dtype=torch.float64, device=DEV)
            status = torch.full((B,), 77, dtype=torch.int32, device=DEV)
            rc = ops._beam_launch(enc, ops._beam_ptrs(table, mats, b_ih, b_hh, b_proj, b_head, ws), None,
                                  (capi.ptr(hyps), capi.ptr(lens), capi.ptr(scores), capi.ptr(status)), B, Tn, Tn, J, H, E, V, 0, 4, 3,
                                  s.cap, 32, 2.3, 2.3, 0.01, wdt, None, None, 0.0, desc, wide)
            torch.cuda.synchronize()
            if out is not None:
                out.update(hyps=hyps.cpu(), lens=lens.cpu(), scores=scores.cpu())
            return rc, status.tolist(), capi.lib().tsasr_last_error().decode()

        rc, status, _ = call(ops._beam_bias_desc(good, B, enc.device))
        assert rc == 0 and status == [0, 0]
        got = {}
        rc, status, _ = call(None, out=got)                  # no graph: the unbiased search, here in the biased (larger) workspace
        assert rc == 0 and status == [0, 0]
        plain = ops.beam_search(enc, table, mats, b_ih, b_hh, b_proj, b_head, 0, 0.01, wdt, 4, 3, 2.3, 2.3, s.cap)
        assert plain[2].tolist() == [0, 0]
        rows = [[r for r in range(3) if int(got["lens"][b, r]) >= 0] for b in range(B)]
        assert [[got["hyps"][b, r, : int(got["lens"][b, r])].tolist() for r in rows[b]] for b in range(B)] == plain[0]
        assert [len(h) for h in plain[0]] == [len(r) for r in rows] and all(len(t) <= 32 for h in plain[0] for t in h)
        assert bits([[float(got["scores"][b, r]) for r in rows[b]] for b in range(B)]) == bits(plain[1])
        rc, status, msg = call(ops._beam_bias_desc(good, B, enc.device), wide=True)      # V = 29, E = 28 with a graph is the narrow search
        assert rc == -1 and status == [77, 77] and "wide" in msg
        state = torch.zeros(B, ops.greedy_stream_state_size(H, J), device=DEV)
        preds = torch.full((B, Tn), 77, dtype=torch.int32, device=DEV)
        logp = torch.zeros(B, device=DEV)
        P = capi.ptr
        rc = capi.lib().tsasr_greedy_decode(P(enc), P(table), P(mats[0]), P(mats[1]), P(b_ih), P(b_hh), P(mats[2]), P(b_proj), P(mats[3]),
                                            P(b_head), P(state), None, P(preds), P(logp), B, Tn, J, H, E, V, 0, 0.01, capi.io_dtype(enc), wdt,
                                            capi.stream_ptr(), 0)
        torch.cuda.synchronize()
        assert rc == -1 and bool((preds == 77).all()) and "n_valid" in capi.lib().tsasr_last_error().decode()
        rc, status, msg = call(ops._beam_bias_desc(good, B, enc.device), ws_delta=-16)
        assert rc != 0 and status == [77, 77] and "workspace" in msg
        empty = ops._beam_bias_desc(good, B, enc.device)
        empty.rows = 0
        rc, status, msg = call(empty)
        assert rc != 0 and status == [77, 77] and "bias sizes" in msg
        nulled = ops._beam_bias_desc(good, B, enc.device)
        nulled.pending = None
        rc, status, msg = call(nulled)
        assert rc != 0 and status == [77, 77] and "null bias pointer" in msg
        for key, wrong in (("pending", good["pending"].float()), ("child_tok", good["child_tok"].long()), ("base", good["base"].long()),
                           ("weight", good["weight"].float()), ("child_off", good["child_off"].cpu()), ("base", good["base"][:1]),
                           ("child_to", good["child_to"][:1])):
            with pytest.raises(ValueError, match="bias"):
                ops._beam_bias_desc(dict(good, **{key: wrong}), B, enc.device)
        for base in ([good["rows"], -1], [0, good["rows"] - 1]):
            bad = dict(good, base=torch.tensor(base, dtype=torch.int32, device=DEV), base_host=None)
            with pytest.raises(ValueError, match="base"):
                ops._beam_bias_desc(bad, B, enc.device)
        with pytest.raises(ValueError, match="bias"):
            s._device_beam_call(enc, ops.beam_search, bias={"child_off": good["child_off"]})


# ---- the recipe ---------------------------------------------------------------------------------------------------------------------------
def test_recipe_test_stage_with_bias_file(tmp_path, monkeypatch):
    """A small fp32 recipe run with --bias_file (ids form) / --bias_weight: the TEST stage's searcher carries the graph and goes through
    the biased device search, no library route is taken."""
    main = importlib.import_module("train_tsasr").main
    phrases, wer = tmp_path / "phrases.txt", tmp_path / "wer.txt"
    phrases.write_text("3 4 5\n\n7 8\n3 4\n")
    argv = [os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml"), "--device", "cuda:0", "--synthetic", "2", "--number_of_epochs",
            "1", "--syn_batch", "4", "--syn_seconds", "2.0", "--syn_enroll_seconds", "1.0", "--syn_tokens", "12", "--hip_graph", "False",
            "--lr", "0.002", "--warmup_steps", "5", "--dropout", "0.0", "--beam_size", "3", "--d_model", "144", "--nhead", "4",
            "--encoder_num_layers", "2", "--speaker_num_layers", "2", "--d_ffn", "576", "--joint_dim", "160", "--decoder_neurons", "128",
            "--compute_dtype", "fp32", "--bias_file", str(phrases), "--bias_weight", "1.5", "--wer_file", str(wer)]
    taken = []
    orig = ops.beam_search

    def spy(*a, **kw):
        taken.append(kw.get("bias"))
        return orig(*a, **kw)
    monkeypatch.setattr(ops, "beam_search", spy)
    ops.LIB_FALLBACKS.clear()
    try:
        brain, result = main(argv)
        assert taken and all(t is not None and t["rows"] == 7 for t in taken), "the TEST stage did not take the biased device search"
        assert ops.LIB_FALLBACKS == {}, ops.LIB_FALLBACKS
        g = brain.hparams.beam_searcher.bias
        assert isinstance(g, ContextGraph) and g.phrases == [[3, 4, 5], [7, 8], [3, 4]] and g.weight == 1.5
        assert wer.exists() and "%WER" in wer.read_text()
        with pytest.raises(SystemExit, match="bias_weight"):
            main(argv[:-4] + ["--bias_weight", "0"] + argv[-2:])
    finally:
        nnet.set_compute_dtype(torch.bfloat16)
