"""Contextual biasing of the beam search, the parts that need no GPU: the trie and its step on hand-written cases, the preconditions of
the shared inputs on the float64 restatement (tests/helpers/beam_bias_ref.py), the host loop (the definition) on CPU modules against
that restatement, the bit identities of the host route, and the workspace size of the biased device search."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import beam_bias_ref as BB  # noqa: E402
import beam_lm_ref as BL  # noqa: E402
from oracle.golden_recipe import det_tensor  # noqa: E402

dec = importlib.import_module("ts-asr_amd.decoders")
biasing = importlib.import_module("ts-asr_amd.biasing")
ContextGraph = biasing.ContextGraph
V = 29


def tolerance(hyps, scores, ref_hyps, ref_scores):
    """The project's rule between two searches of the same utterances (test_beam_lm_cpu.py::tolerance): equal sequence or normalised
    score within 5e-4, every score within 1e-3, at least half of the sequences equal."""
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


def bits(scores):
    return [np.array(x, np.float64).tobytes() for x in scores]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the trie
A_, B_, C_, D_ = 1, 2, 3, 4


def test_state_numbering_and_arrays():
    """States are numbered in creation order, phrase by phrase, token by token; the CSR rows hold a state's tokens ascending."""
    g = ContextGraph([[C_, A_], [A_, B_], [C_, B_], [A_, B_, D_]], 0.5)
    # root -C-> 1 -A-> 2 ; root -A-> 3 -B-> 4 ; 1 -B-> 5 ; 4 -D-> 6
    assert g.num_states == 7
    assert g.children[0] == {C_: 1, A_: 3} and g.children[1] == {A_: 2, B_: 5} and g.children[3] == {B_: 4} and g.children[4] == {D_: 6}
    assert g.depth == [0, 1, 2, 1, 2, 2, 3]
    assert g.terminal == [False, False, True, False, True, True, True]
    off, tok, to, pending = g.arrays()
    assert off.dtype == np.int32 and tok.dtype == np.int32 and to.dtype == np.int32 and pending.dtype == np.float64
    assert off.tolist() == [0, 2, 4, 4, 5, 6, 6, 6]
    assert tok.tolist() == [A_, C_, A_, B_, B_, D_] and to.tolist() == [3, 1, 2, 5, 4, 6]
    assert pending.tolist() == [0.0, 0.5, 0.0, 0.5, 0.0, 0.0, 0.0]


def test_pending_at_a_terminal_with_children():
    """A terminal that has children keeps matching the longer phrase; what it earned is committed (pending 0), the states past it owe
    only the tokens since it."""
    w = 0.7
    g = ContextGraph([[A_, B_], [A_, B_, C_, D_]], w)
    assert g.tdepth == [0, 0, 2, 2, 4] and g.terminal == [False, False, True, False, True]
    assert g.pending.tolist() == [0.0, w * 1, 0.0, w * 1, 0.0]
    s, total = 0, 0.0
    for v in (A_, B_, C_):
        s, d = g.step(s, v)
        assert d == w
        total += d
    assert s == 3
    s, d = g.step(s, A_)                  # gives up C only, restarts with A
    assert (s, d) == (1, -g.pending[3] + w) and g.pending[3] == w


def test_cancel_amounts_and_restart_with_match():
    w = 1.25
    g = ContextGraph([[A_, B_, C_, D_], [B_, D_]], w)
    assert g.pending.tolist() == [0.0, w * 1, w * 2, w * 3, 0.0, w * 1, 0.0]
    assert g.pending[3] == w * 3                      # the stored product, never recomputed
    assert g.step(0, D_) == (0, -0.0) and g.step(0, A_) == (1, w)
    assert g.step(3, A_) == (1, -g.pending[3] + w)    # cancel three tokens, A opens a phrase at the root
    assert g.step(3, C_) == (0, -g.pending[3])        # cancel, C opens nothing
    assert g.step(2, B_) == (5, -g.pending[2] + w)    # restart-with-match into the other phrase
    assert g.step(4, A_) == (1, w) and g.step(4, C_) == (0, 0.0)     # after a complete phrase nothing is owed
    arr = BB.graph_arrays(g)
    for s in range(g.num_states):                     # the float64 helper reads the arrays to the same effect
        for v in range(1, 6):
            s2, d2 = BB.step(arr, s, v)
            assert (s2, np.float64(d2).tobytes()) == (g.step(s, v)[0], np.float64(g.step(s, v)[1]).tobytes())


def test_no_failure_links_misses_abac():
    """The documented miss: phrase A B A C on A B A B A C. With failure links the second B would fall back to the state after A B."""
    w = 1.0
    g = ContextGraph([[A_, B_, A_, C_]], w)
    s, total, states = 0, 0.0, []
    for v in (A_, B_, A_, B_, A_, C_):
        s, d = g.step(s, v)
        total += d
        states.append(s)
    assert states == [1, 2, 3, 0, 1, 0]
    assert total == 0.0 and not g.terminal[s]
    assert "failure links" in biasing.__doc__ and "A B A B A C" in biasing.__doc__


def test_duplicates_and_empty_graph():
    g = ContextGraph([[A_, B_], [A_, B_], (A_, B_)], 1.0)
    assert g.num_states == 3 and g.phrases == [[A_, B_]]
    e = ContextGraph([], 1.0)
    assert e.empty and e.num_states == 1 and BB.graph_arrays(e) is None
    assert biasing.as_list(e, 3) == [None, None, None] and biasing.as_list([e, g, None], 3) == [None, g, None]
    s = dec.TransducerBeamSearcher([None, None, None], None, [None], blank_id=0)
    assert s._bias_graphs(e, 2) is None and s._bias_graphs([e, None], 2) is None and s._bias_graphs(g, 2) == [g, g]
    for bad in ([[]], [[A_, -1]], [[1.5]]):
        with pytest.raises(ValueError):
            ContextGraph(bad, 1.0)
    for bad_w in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ContextGraph([[A_]], bad_w)


def test_blank_or_out_of_range_token_raises():
    head = torch.nn.Linear(4, 7)
    s = dec.TransducerBeamSearcher([None, None, None], None, [head], blank_id=0, beam_size=3)
    s.bias = ContextGraph([[1, 6]], 1.0)
    with pytest.raises(ValueError, match="blank"):
        s.bias = ContextGraph([[1, 0]], 1.0)
    with pytest.raises(ValueError, match="vocabulary"):
        s.bias = [None, ContextGraph([[1, 7]], 1.0)]
    with pytest.raises(ValueError, match="vocabulary"):
        dec.TransducerBeamSearcher([None, None, None], None, [head], blank_id=0, bias=ContextGraph([[9]], 1.0))
    with pytest.raises(ValueError, match="blank"), torch.no_grad():
        s(torch.zeros(1, 2, 4), bias=ContextGraph([[0]], 1.0))
    with pytest.raises(ValueError, match="list of 2"):
        s._bias_graphs([ContextGraph([[1]], 1.0)], 2)


def test_from_text():
    pieces = ["<blank>", "a", "b", "ab", " ", "c"]
    g = ContextGraph.from_text(["ab c", "", "1 5 2", "abab"], pieces, 0.5)
    assert g.phrases == [[3, 4, 5], [1, 5, 2], [3, 3]]
    with pytest.raises(ValueError, match="line 2"):
        ContextGraph.from_text(["ab", "a!b"], pieces, 0.5)


def test_pack_layout():
    g1, g2 = ContextGraph([[A_, B_]], 1.0), ContextGraph([[C_], [C_, D_]], 0.25)
    p = biasing.pack([g1, None, g2, g1, ContextGraph([], 1.0)], "cpu")
    assert p["base_host"] == (0, -1, 4, 0, -1) and p["rows"] == 8 and p["edges"] == 4
    assert p["child_off"].tolist() == [0, 1, 2, 2, 2, 3, 4, 4] and p["child_tok"].tolist() == [A_, B_, C_, D_]
    assert p["child_to"].tolist() == [1, 2, 1, 2]                     # the graphs' own state ids
    assert p["pending"].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and p["weight"].tolist() == [1.0, 0.0, 0.25, 1.0, 0.0]
    assert p["child_off"].dtype == torch.int32 and p["pending"].dtype == torch.float64 and p["base"].dtype == torch.int32
    assert biasing.pack([g1, None, g2, g1, None], "cpu") is p         # cached by the graphs' identities
    none = biasing.pack([None, None], "cpu")
    assert none["base_host"] == (-1, -1) and all(none[k].numel() > 0 for k in ("child_off", "child_tok", "child_to", "pending"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the shared inputs
def _inputs(golden):
    c = golden["c1_chain_cat"]["enc_proj"]
    base = np.concatenate([c[:, ::-1], np.roll(c, 1, axis=0)], 0)[:6, :40]
    return {"first": np.ascontiguousarray(c[:, :24]), "second": base + det_tensor("beam.enc_proj.2", base.shape, 0.05)}


_REF = {}


def reference(golden, name, beam):
    """(enc, the batch's graph, float64 unbiased results, float64 biased results) of an input, computed once."""
    if (name, beam) not in _REF:
        enc = _inputs(golden)[name]
        w = BL.predictor_weights(float(golden["c1_beam_lm"]["blank_bias"]))
        plain = [BL.beam_search_lm(enc[b], w, None, 0.0, beam) for b in range(enc.shape[0])]
        graph = ContextGraph(BB.test_phrases([p[0] for p in plain], V), BB.BIAS_WEIGHT)
        biased = [BB.beam_search_bias(enc[b], w, BB.graph_arrays(graph), beam) for b in range(enc.shape[0])]
        _REF[(name, beam)] = (enc, graph, plain, biased)
    return _REF[(name, beam)]


CASES = [(name, beam) for name in ("first", "second") for beam in (4, 15)]


@pytest.mark.parametrize("name,beam", CASES)
def test_preconditions_on_the_float64_reference(golden, name, beam):
    """The inputs exercise the feature: the biased best differs from the unbiased best somewhere, every event occurs, and the
    finalisation changes at least one reported score."""
    enc, graph, plain, biased = reference(golden, name, beam)
    assert any(r[0][0] != p[0][0] for r, p in zip(biased, plain))
    counts = {k: sum(int(r[2][k]) for r in biased) for k in BB.EVENTS}
    finalised = sum(a != b for r in biased for a, b in zip(r[1], r[3]))
    print(name, beam, counts, "finalised scores", finalised)
    assert all(counts[k] >= 1 for k in BB.EVENTS), counts
    assert finalised >= 1
    assert any(graph.terminal[s] and graph.children[s] for s in range(graph.num_states))     # a terminal with children is in the list


# ---------------------------------------------------------------------------------------------------------------------------------------
# the host loop
class _Joint(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.nonlinearity = torch.nn.LeakyReLU(0.01)

    def forward(self, a, b):
        return self.nonlinearity(a + b)


_SEARCHERS = {}


def cpu_searcher(golden, beam, nbest=BB.NBEST):
    """The golden recipe's predictor and head as plain fp32 CPU modules (one-hot embedding, LSTM, two Linear layers)."""
    if "mods" not in _SEARCHERS:
        w = BL.predictor_weights(float(golden["c1_beam_lm"]["blank_bias"]))
        t = lambda k: torch.from_numpy(np.ascontiguousarray(w[k]))  # noqa: E731
        Hd, J = w["w_hh"].shape[1], w["w_proj"].shape[0]
        emb, lstm = torch.nn.Embedding(V, V - 1), torch.nn.LSTM(V - 1, Hd, batch_first=True)
        proj, head = torch.nn.Linear(Hd, J), torch.nn.Linear(J, V)
        with torch.no_grad():
            emb.weight.copy_(t("emb"))
            lstm.weight_ih_l0.copy_(t("w_ih")), lstm.weight_hh_l0.copy_(t("w_hh")), lstm.bias_ih_l0.copy_(t("b_ih")), lstm.bias_hh_l0.copy_(t("b_hh"))
            proj.weight.copy_(t("w_proj")), proj.bias.copy_(t("b_proj")), head.weight.copy_(t("w_head")), head.bias.copy_(t("b_head"))
        _SEARCHERS["mods"] = (emb, lstm, proj, head)
    emb, lstm, proj, head = _SEARCHERS["mods"]
    return dec.TransducerBeamSearcher([emb, lstm, proj], _Joint(), [head], blank_id=0, beam_size=beam, nbest=nbest)


@pytest.mark.parametrize("name,beam", CASES)
def test_host_loop_against_float64(golden, name, beam):
    """The definition (the host loop, fp32 CPU modules) against the float64 restatement, the rule on every rank."""
    enc, graph, plain, biased = reference(golden, name, beam)
    s = cpu_searcher(golden, beam)
    with torch.no_grad():
        _, _, nb, sc = s(torch.from_numpy(enc).float(), bias=graph)
        _, _, nb0, _ = s(torch.from_numpy(enc).float())
    assert nb != nb0
    exact = tolerance_ranks(nb, sc, [r[0] for r in biased], [r[1] for r in biased])
    print(f"{name} beam {beam}: host loop fp32 vs float64, utterances exact per rank {exact} of {enc.shape[0]}")


def test_host_stream_pieces_and_lists_bit_identical(golden):
    """Host beam_stream in pieces (cuts at 1, 7 and 8 frames, a zero-frame call between them) is the one call bit for bit, biased,
    timed and untimed; the timed search gives the untimed bits; a per-utterance list equals each utterance alone; another graph for a
    running stream raises, a reset stream takes a new one."""
    enc, graph, _, _ = reference(golden, "first", 4)
    enc = torch.from_numpy(enc).float()
    B, Tn = enc.shape[:2]
    other = ContextGraph([[5, 6], [7]], 2.0)
    graphs = [graph, None, other, ContextGraph([], 1.0)]
    s = cpu_searcher(golden, 4)
    with torch.no_grad():
        whole = s(enc, bias=graphs)
        timed = s.forward_timed(enc, bias=graphs)
        assert timed[2] == whole[2] and bits(timed[3]) == bits(whole[3]) and float(timed[1]) == float(whole[1])
        plain = s(enc)
        for b in range(B):
            alone = s(enc[b:b + 1], bias=graphs[b]) if graphs[b] is not None else s(enc[b:b + 1])
            assert alone[2][0] == whole[2][b] and bits(alone[3][0]) == bits(whole[3][b])
        assert whole[2][1] == plain[2][1] and bits(whole[3][1]) == bits(plain[3][1])          # None: the plain search
        assert whole[2][3] == plain[2][3] and bits(whole[3][3]) == bits(plain[3][3])          # an empty graph too
        assert whole[2][0] != plain[2][0]
        for frames in (False, True):
            state, t0 = None, 0
            for n in (1, 7, 0, 8, Tn - 16):
                _, state = s.beam_stream(enc[:, t0:t0 + max(n, 1)], state, torch.full((B,), n, dtype=torch.int32), return_frames=frames,
                                         bias=graphs if t0 != 8 else None)
                t0 += n
            assert state["nbest"] == whole[2] and [bits(x) for x in state["scores"]] == [bits(x) for x in whole[3]]
            assert not frames or state["frames"] == timed[5]
        with pytest.raises(ValueError, match="another graph"):
            s.beam_stream(enc[:, :1], state, bias=[graph, other, other, None], return_frames=True)
        with pytest.raises(ValueError, match="without bias"):
            s.beam_stream(enc[:, :1], s.beam_stream(enc[:, :1])[1], bias=graph)
        s.reset_streams(state, [1])
        _, state = s.beam_stream(enc, state, bias=[graph, other, other, None], return_frames=True)
        assert state["nbest"][1] == s(enc[1:2], bias=other)[2][0]


def test_bias_workspace_bytes():
    """The biased layout: that of the same search without a graph (narrow for V <= 63 and E <= 64, wide otherwise) plus one int32 per
    tree node; the C side and the wrapper agree."""
    ops = importlib.import_module("ts-asr_amd.ops")
    a16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    lib = importlib.import_module("ts-asr_amd._capi").lib()
    for B, T, H, J, E, V_, beam, cap in ((32, 250, 512, 640, 28, 29, 15, 512), (1, 1, 4, 4, 1, 2, 2, 2), (3, 40, 128, 160, 99, 100, 4, 37),
                                         (2, 9, 64, 32, 72, 40, 4, 9)):
        wide = V_ > 63 or E > 64
        nodes = a16(4 * (1 + (T + 1) * beam + cap))
        for times in (0, 1):
            for L, Hl in ((0, 0), (2, 40)):
                lm_part = ((V_ + 3) // 4 * 4 if wide else 64) + 2 * L * Hl if L > 0 else 0
                base = B * (a16(64 + 24 * beam) + a16(8 * (1 + (T + 1) * beam + cap)) + 4 * (cap + beam) * (J + 2 * H + lm_part) + times * nodes)
                assert ops.beam_workspace_bytes(B, T, H, J, V_, beam, cap, L, Hl, bool(times), False, wide) == base
                want = base + B * nodes
                assert ops.beam_workspace_bytes(B, T, H, J, V_, beam, cap, L, Hl, bool(times), True, wide) == want
                assert lib.tsasr_beam_search_workspace_bytes(B, T, H, J, V_, beam, cap, L, Hl, times, 1, int(wide)) == want
    assert ops.beam_workspace_bytes(0, 1, 4, 4, 2, 2, 2, bias=True) == 0
    assert lib.tsasr_beam_search_workspace_bytes(2, 8, 128, 160, 29, 4, 16, 1, 0, 0, 1, 0) == 0
    assert ops.beam_wide_lds_bytes(128, 160, 99, 100, 512, bias=True) == ops.beam_wide_lds_bytes(128, 160, 99, 100, 512) + 4 * 512
