"""Float64 restatement of the transducer beam search with LM fusion (numpy only), and the deterministic LMs of its fixture.

The search is the one decoders.py and csrc/search.hip state (speechbrain/decoders/transducer.py:220-373 with lm_weight > 0): per frame,
A = the hypotheses to extend, beam = those that emitted blank here. Until the beam holds beam_size entries: a = the first entry of A with
the largest logp / len; stop once the best beam entry has logp >= state_beam + logp(a); remove a; one predictor step and one LM step on
a's last token (blank is both networks' start symbol) from a's states; the beam_size best symbols of the joint's log-softmax; blank puts
a copy of a (same states) on the beam with the joint's term alone; a non-blank sym within expand_beam of the best non-blank extends a in A
(new states) with (logp(a) + logp_joint[sym]) + lm_weight * logp_lm[sym]. Both steps are functions of (token, parent state), so they are
computed once per hypothesis and kept with it.

The LM is RNNLM's inference path: embedding row -> L stacked LSTM cells (torch gate order i, f, g, o) -> blocks of Linear, LayerNorm,
LeakyReLU -> Linear to V -> log-softmax. Weights are named by the reference's state_dict keys; the blocks after the first are
``linear_0``, ``norm_0``, ... as its Sequential names repeated layers (the fixture records the key lists of the reference itself).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.golden_recipe import CFG1, det_tensor, det_weight  # noqa: E402

# name -> (LSTM layers, dnn blocks, rnn_neurons, embedding_dim, dnn_neurons, scale of the seeded-normal weights, lm_weight of its cases)
LM_CONFIGS = {
    "l2b1e72": dict(layers=2, blocks=1, hidden=64, emb=72, dnn=48, scale=0.5, weight=0.3),     # embedding past the 64-column side operand
    "l1b0": dict(layers=1, blocks=0, hidden=32, emb=16, dnn=32, scale=0.5, weight=0.3),
    "l2b1w1": dict(layers=2, blocks=1, hidden=64, emb=32, dnn=48, scale=0.2, weight=1.0),
    "l3b2h40": dict(layers=3, blocks=2, hidden=40, emb=24, dnn=36, scale=0.3, weight=0.3),     # hidden no multiple of 64
}
FRAMES = (24, 50)
BEAMS = (2, 4, 15)
NBEST = 3
LN_EPS = 1e-5
LM_SLOPE = 0.01


def block_names(k):
    """(linear, norm) names of dnn block k."""
    return ("linear", "norm") if k == 0 else (f"linear_{k - 1}", f"norm_{k - 1}")


def lm_shapes(cfg, V=CFG1["vocab_size"]):
    """{state_dict key: shape} of an RNNLM of ``cfg``, in the module's own order."""
    Hl, E, D = cfg["hidden"], cfg["emb"], cfg["dnn"]
    out = {"embedding.Embedding.weight": (V, E)}
    for l in range(cfg["layers"]):
        out[f"rnn.rnn.weight_ih_l{l}"] = (4 * Hl, E if l == 0 else Hl)
        out[f"rnn.rnn.weight_hh_l{l}"] = (4 * Hl, Hl)
        out[f"rnn.rnn.bias_ih_l{l}"] = (4 * Hl,)
        out[f"rnn.rnn.bias_hh_l{l}"] = (4 * Hl,)
    for k in range(cfg["blocks"]):
        lin, norm = block_names(k)
        out[f"dnn.{lin}.w.weight"] = (D, Hl if k == 0 else D)
        out[f"dnn.{lin}.w.bias"] = (D,)
        out[f"dnn.{norm}.norm.weight"] = (D,)
        out[f"dnn.{norm}.norm.bias"] = (D,)
    out["out.w.weight"] = (V, D)
    out["out.w.bias"] = (V,)
    return out


def lm_weights(name, V=CFG1["vocab_size"]):
    """{key: float32 array}: every tensor of LM ``name`` is det_tensor("lm.<name>.<key>", shape, scale)."""
    cfg = LM_CONFIGS[name]
    return {k: det_tensor(f"lm.{name}.{k}", s, cfg["scale"]) for k, s in lm_shapes(cfg, V).items()}


def predictor_weights(blank_bias=0.0, cfg=CFG1):
    """The golden recipe's predictor, joint head and one-hot embedding table (float32 arrays under search_times_ref's names); the
    head's blank bias raised by ``blank_bias`` as the beam fixtures do."""
    V, Hd, J, blank = cfg["vocab_size"], cfg["decoder_neurons"], cfg["joint_dim"], cfg["blank_index"]
    emb = np.zeros((V, V - 1), np.float32)
    rows = [v for v in range(V) if v != blank]
    emb[rows, np.arange(V - 1)] = 1.0
    w = dict(emb=emb, w_ih=det_weight("decoder.rnn.weight_ih_l0", (4 * Hd, V - 1)), w_hh=det_weight("decoder.rnn.weight_hh_l0", (4 * Hd, Hd)),
             b_ih=det_weight("decoder.rnn.bias_ih_l0", (4 * Hd,)), b_hh=det_weight("decoder.rnn.bias_hh_l0", (4 * Hd,)),
             w_proj=det_weight("decoder_proj.w.weight", (J, Hd)), b_proj=det_weight("decoder_proj.w.bias", (J,)),
             w_head=det_weight("transducer_head.w.weight", (V, J)), b_head=det_weight("transducer_head.w.bias", (V,)).copy())
    w["b_head"][blank] += np.float32(blank_bias)
    return w


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    H = h.shape[0]
    g = w_ih @ x + w_hh @ h
    for b in (b_ih, b_hh):
        if b is not None:
            g = g + b
    i, f, gg, o = _sigmoid(g[:H]), _sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sigmoid(g[3 * H:])
    c2 = f * c + i * gg
    return o * np.tanh(c2), c2


def _log_softmax(v):
    m = v.max()
    return v - m - np.log(np.exp(v - m).sum())


def f64(weights):
    return {k: (None if v is None else np.asarray(v, np.float64)) for k, v in weights.items()}


def predictor_step(w, tok, state):
    """(pn [J], (h, c)) of float64 predictor weights ``w`` (search_times_ref's names) on token ``tok`` from ``state`` (None: zeros)."""
    H = w["w_hh"].shape[1]
    h, c = state if state is not None else (np.zeros(H), np.zeros(H))
    h, c = _lstm_cell(w["emb"][tok], h, c, w["w_ih"], w["w_hh"], w.get("b_ih"), w.get("b_hh"))
    pn = w["w_proj"] @ h
    if w.get("b_proj") is not None:
        pn = pn + w["b_proj"]
    return pn, (h, c)


def lm_step(lw, tok, state, eps=LN_EPS, slope=LM_SLOPE):
    """(log-probabilities [V], state) of float64 LM weights ``lw`` (state_dict keys) on token ``tok`` from ``state`` = list of (h, c) per
    layer (None: zeros)."""
    layers = sum(1 for k in lw if k.startswith("rnn.rnn.weight_hh_l"))
    Hl = lw["rnn.rnn.weight_hh_l0"].shape[1]
    if state is None:
        state = [(np.zeros(Hl), np.zeros(Hl)) for _ in range(layers)]
    x = lw["embedding.Embedding.weight"][tok]
    new = []
    for l in range(layers):
        h, c = _lstm_cell(x, state[l][0], state[l][1], lw[f"rnn.rnn.weight_ih_l{l}"], lw[f"rnn.rnn.weight_hh_l{l}"],
                          lw.get(f"rnn.rnn.bias_ih_l{l}"), lw.get(f"rnn.rnn.bias_hh_l{l}"))
        new.append((h, c))
        x = h
    k = 0
    while f"dnn.{block_names(k)[0]}.w.weight" in lw:
        lin, norm = block_names(k)
        y = lw[f"dnn.{lin}.w.weight"] @ x + lw[f"dnn.{lin}.w.bias"]
        y = (y - y.mean()) / np.sqrt(y.var() + eps) * lw[f"dnn.{norm}.norm.weight"] + lw[f"dnn.{norm}.norm.bias"]
        x = np.where(y > 0, y, y * slope)
        k += 1
    return _log_softmax(lw["out.w.weight"] @ x + lw["out.w.bias"]), new


def beam_search_lm(enc, weights, lm, lm_weight, beam_size, nbest=NBEST, blank=0, slope=0.01, state_beam=2.3, expand_beam=2.3,
                   step=None):
    """n-best (token lists, logp / len) of one utterance enc [T, J] in float64. ``weights``: the predictor and head (search_times_ref's
    names), ``lm``: the LM's weights by state_dict key (None or lm_weight 0: no LM). ``step`` replaces lm_step: (tok, state) -> (logp, state)."""
    w = f64(weights)
    use_lm = lm is not None and lm_weight > 0
    lw = f64(lm) if use_lm and step is None else None
    if use_lm and step is None:
        step = lambda tok, st: lm_step(lw, tok, st)  # noqa: E731
    enc = np.asarray(enc, np.float64)
    key = lambda hyp: hyp["logp"] / len(hyp["tokens"])  # noqa: E731
    beam = [dict(tokens=[int(blank)], logp=0.0, pred=None, lm=None, cache=None)]
    for t in range(enc.shape[0]):
        A, beam = beam, []
        while len(beam) < beam_size:
            a = max(A, key=key)
            if beam and max(beam, key=key)["logp"] >= state_beam + a["logp"]:
                break
            A.remove(a)
            if a["cache"] is None:                       # the steps of this hypothesis: once, reused when it is expanded at a later frame
                pn, pred = predictor_step(w, a["tokens"][-1], a["pred"])
                lm_lp, lm_state = step(a["tokens"][-1], a["lm"]) if use_lm else (None, None)
                a["cache"] = (pn, pred, lm_lp, lm_state)
            pn, pred, lm_lp, lm_state = a["cache"]
            z = enc[t] + pn
            lg = w["w_head"] @ np.where(z > 0, z, z * slope)
            if w.get("b_head") is not None:
                lg = lg + w["b_head"]
            lp = _log_softmax(lg)
            order = sorted(range(lp.shape[0]), key=lambda v: (-lp[v], v))[:beam_size]      # top-k, equal values: the lower index first
            best_nonblank = lp[order[0]] if order[0] != blank else lp[order[1]]
            for sym in order:
                if sym == blank:
                    beam.append(dict(a, tokens=a["tokens"][:], logp=a["logp"] + lp[sym]))
                elif lp[sym] >= best_nonblank - expand_beam:
                    sc = a["logp"] + lp[sym]
                    if use_lm:
                        sc = sc + lm_weight * lm_lp[sym]
                    A.append(dict(tokens=a["tokens"] + [int(sym)], logp=sc, pred=pred, lm=lm_state, cache=None))
    ranked = sorted(beam, key=key, reverse=True)[:nbest]
    return [h["tokens"][1:] for h in ranked], [float(key(h)) for h in ranked]


def case_key(name, T, beam):
    return f"{name}_T{T}_b{beam}"


def fixture_case(g, name, T, beam, b):
    """(n-best token lists, scores) the fixture ``g`` stores for utterance b of a case."""
    k = case_key(name, T, beam)
    n = int(g[k + "_count"][b])
    lens = g[k + "_lens"][b]
    return [g[k + "_hyps"][b, r, : int(lens[r])].tolist() for r in range(n)], [float(g[k + "_scores"][b, r]) for r in range(n)]
