"""Float64 restatement of the beam search with contextual biasing (numpy only), and the deterministic phrase lists of its tests.

The search is beam_lm_ref.beam_search_lm's (its predictor, LM and log-softmax steps are imported as they are; the subword nets of
beam_wide_ref carry the same weight names), with the rule ts-asr_amd/biasing.py states: every hypothesis carries a trie state, 0 at the
start; a blank copy keeps state and score; a non-blank extension by v takes step(s, v) = (s', d) and scores
((logp(a) + logp_joint[v]) [+ lm_weight * logp_lm[v]]) + d, d last; the n-best is ranked and reported with (logp - pending[state]) / len.
The graph is read in its device form, the arrays (child_off, child_tok, child_to, pending) and the weight: ``pending`` is never
recomputed here.

Events counted over every extension the search appends (kept or not): ``advance`` a child matched (from the root or deeper),
``complete`` the step reached a state whose pending is 0 (a phrase ended there), ``cancel`` a match with pending > 0 was given up,
``restart_match`` a match failed below the root and the token opened a phrase at the root.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from beam_lm_ref import _log_softmax, f64, lm_step, predictor_step  # noqa: E402

NBEST = 3
BIAS_WEIGHT = 1.0       # nats per matched token in the tests: the smallest of 1.0, 1.5, 2.0, ... at which the preconditions of
#                         tests/test_beam_bias_cpu.py hold on every input (biased best differs, every event occurs, finalisation bites)
EVENTS = ("advance", "complete", "cancel", "restart_match")


def graph_arrays(graph):
    """(child_off, child_tok, child_to, pending, weight) of a biasing.ContextGraph, or None for None / an empty graph."""
    if graph is None or graph.empty:
        return None
    return tuple(graph.arrays()) + (graph.weight,)


def _child(off, tok, to, s, v):
    lo, hi = int(off[s]), int(off[s + 1])
    i = lo + int(np.searchsorted(tok[lo:hi], v))
    return int(to[i]) if i < hi and int(tok[i]) == v else -1


def step(arrays, s, v, counts=None):
    """(s', d) of the graph ``arrays`` in state s on token v."""
    off, tok, to, pending, w = arrays
    c = _child(off, tok, to, s, v)
    if c >= 0:
        if counts is not None:
            counts["advance"] += 1
            counts["complete"] += pending[c] == 0.0
        return c, w
    d = -pending[s]
    if counts is not None:
        counts["cancel"] += pending[s] > 0.0
    c = _child(off, tok, to, 0, v)
    if c >= 0:
        if counts is not None:
            counts["restart_match"] += s != 0
            counts["advance"] += 1
            counts["complete"] += pending[c] == 0.0
        return c, d + w
    return 0, d


def beam_search_bias(enc, weights, graphs_arrays, beam, nbest=NBEST, lm=None, lm_weight=0.0, blank=0, slope=0.01, state_beam=2.3,
                     expand_beam=2.3):
    """One utterance enc [T, J] in float64. ``graphs_arrays``: graph_arrays() of the utterance's graph, or None (the plain search).
    Returns (n-best token lists, their finalised scores (logp - pending[state]) / len, event counts, raw logp / len of the same
    hypotheses)."""
    w = f64(weights)
    use_lm = lm is not None and lm_weight > 0
    lw = f64(lm) if use_lm else None
    g = graphs_arrays
    counts = {k: 0 for k in EVENTS}
    enc = np.asarray(enc, np.float64)
    key = lambda hyp: hyp["logp"] / len(hyp["tokens"])  # noqa: E731
    beam_l = [dict(tokens=[int(blank)], logp=0.0, pred=None, lm=None, cache=None, ctx=0)]
    for t in range(enc.shape[0]):
        A, beam_l = beam_l, []
        while len(beam_l) < beam:
            a = max(A, key=key)
            if beam_l and max(beam_l, key=key)["logp"] >= state_beam + a["logp"]:
                break
            A.remove(a)
            if a["cache"] is None:
                pn, pred = predictor_step(w, a["tokens"][-1], a["pred"])
                lm_lp, lm_state = lm_step(lw, a["tokens"][-1], a["lm"]) if use_lm else (None, None)
                a["cache"] = (pn, pred, lm_lp, lm_state)
            pn, pred, lm_lp, lm_state = a["cache"]
            z = enc[t] + pn
            lg = w["w_head"] @ np.where(z > 0, z, z * slope)
            if w.get("b_head") is not None:
                lg = lg + w["b_head"]
            lp = _log_softmax(lg)
            order = sorted(range(lp.shape[0]), key=lambda v: (-lp[v], v))[:beam]
            best_nonblank = lp[order[0]] if order[0] != blank else lp[order[1]]
            for sym in order:
                if sym == blank:
                    beam_l.append(dict(a, tokens=a["tokens"][:], logp=a["logp"] + lp[sym]))
                elif lp[sym] >= best_nonblank - expand_beam:
                    sc = a["logp"] + lp[sym]
                    if use_lm:
                        sc = sc + lm_weight * lm_lp[sym]
                    ctx = 0
                    if g is not None:
                        ctx, d = step(g, a["ctx"], int(sym), counts)
                        sc = sc + d
                    A.append(dict(tokens=a["tokens"] + [int(sym)], logp=float(sc), pred=pred, lm=lm_state, cache=None, ctx=ctx))
    fin = (lambda hyp: (hyp["logp"] - g[3][hyp["ctx"]]) / len(hyp["tokens"])) if g is not None else key
    ranked = sorted(beam_l, key=fin, reverse=True)[:nbest]
    return [h["tokens"][1:] for h in ranked], [float(fin(h)) for h in ranked], counts, [float(key(h)) for h in ranked]


def test_phrases(ref_nbest, V=29, blank=0):
    """The phrase list of a batch, from ``ref_nbest`` = per utterance the unbiased float64 n-best token lists: per utterance a window
    of (up to) 3 tokens of the rank-2 hypothesis starting where it first differs from rank 1 (moved left if the hypothesis ends
    sooner); then one phrase that extends the first window by 2 tokens (a terminal with children), one that shares its first 2 tokens
    and then diverges (forces a cancel), and one that never occurs."""
    nonblank = [v for v in range(V) if v != blank]
    windows = []
    for nb in ref_nbest:
        if len(nb) < 2 or not nb[1]:
            continue
        r1, r2 = nb[0], nb[1]
        i = next((k for k in range(min(len(r1), len(r2))) if r1[k] != r2[k]), min(len(r1), len(r2)))
        i = max(0, min(i, len(r2) - 3))
        win = [int(v) for v in r2[i:i + 3]]
        if win and win not in windows:
            windows.append(win)
    phrases = [list(p) for p in windows]
    if windows:
        first = windows[0]
        phrases.append(first + [nonblank[(first[-1] + 3) % len(nonblank)], nonblank[(first[0] + 7) % len(nonblank)]])
        other = next(v for v in nonblank if v != first[-1] and v != first[0])
        phrases.append(first[:2] + [other, other])
    phrases.append([nonblank[-1]] * 5)
    return phrases
