"""Float64 beam search over the subword search cases of joint_wide_ref.greedy_net, with the bookkeeping the wide device search is tested on.

The search is beam_lm_ref.beam_search_lm's (speechbrain/decoders/transducer.py:220-373; its predictor and LM steps are used as they are),
restated here because every value below is taken from inside its loop. Per utterance it returns
  nbest, scores : the n-best token lists and their logp / len,
  frames        : per n-best entry the encoder frame that emitted each token,
  peak          : the largest number of hypotheses a frame's A list held, counted as the device search counts them (the beam that enters
                  the frame plus every extension appended during it; removal does not free an entry): status 1 exactly when peak > cap,
  expansions    : hypotheses expanded, over all frames,
  margin        : the smallest distance to a tie over every comparison the search makes: k-th against (k+1)-th log-probability of each
                  top-k, each expand_beam test, best against second-best key when a is chosen, each state_beam break test, and the
                  adjacent keys of the final ranking. Exactly equal values, which the index rule resolves, are not margins.
With margin >= 1e-4 (beam_case_ok) a float32 search that is right makes every decision the same way, so hypotheses compare exactly.

A random head almost never prefers blank, and a beam search whose frames do not close never ends: each case carries its own extra blank
bias, added to joint_wide_ref's, chosen so that beam_case_ok holds for every beam of the case in fp32 and on the bf16-rounded weights
(tests/test_beam_wide_ref_cpu.py checks that it does).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_lm_ref as BL  # noqa: E402
import joint_wide_ref as JW  # noqa: E402

NBEST = 3
# name -> joint_wide_ref case (the shape), B, T, and per beam (seed name of the weights, extra blank bias): a case is (name, beam)
CASES = {
    # first wide V, one full wave, one-hot E = 63: the side operand. At the shipped seed name only beam 4 meets beam_case_ok in both
    # precisions at any bias (steps of 1/8 from +2 to +5: a margin below 1e-4, too few tokens or more than 128 hypotheses)
    "v64": dict(net="v64", B=3, T=24, runs={2: ("v64_s1", 3.25), 4: ("v64", 4.0), 8: ("v64_s5", 3.75), 15: ("v64_s1", 4.4375)}),
    "v100": dict(net="v100", B=3, T=24, runs={4: ("v100", 2.75)}),                # partial wave, one-hot E = 99: the sparse route
    "v100_e128": dict(net="v100_e128", B=3, T=24, runs={4: ("v100_e128", 2.125)}),   # learned embedding: the dense route
    "v1024_big": dict(net="v1024_big", B=2, T=12, runs={4: ("v1024_big", 3.0)}),  # H = 512, J = 640
}
FIXTURE_CASES = ("v64", "v100")    # pinned to the reference's searcher in tests/golden/c1_beam_wide.npz (beam 4, nbest 3)
# name -> beam_lm_ref LM configuration, lm_weight, case, beam, (seed name, bias): the LM-fused cases. The LM's term lowers every
# extension's score (0.3 * log(1 / 100) on average), so at the unfused bias nothing is emitted: these cases carry a smaller one.
LM_CASES = {
    "v100_l1b0": dict(lm="l1b0", weight=0.3, case="v100", beam=4, run=("v100", 0.875)),
    "v100_l2b1": dict(lm="l2b1e72", weight=0.3, case="v100", beam=4, run=("v100", 0.875)),     # two layers and a dnn block, embedding past 64 columns
}


@functools.lru_cache(maxsize=None)
def case_net(name, beam, bf16=False, run=None):
    """joint_wide_ref.greedy_net of the case's shape under the seed name of (name, beam), with its blank bias raised and enc cut to
    [B, T, J]; ``bf16``: as a bf16 device run reads it; ``run``: another (seed name, bias), the LM cases'."""
    c = CASES[name]
    seed, bias = run or c["runs"][beam]
    net = dict(JW.greedy_net(seed, spec=JW.GREEDY_CASES[c["net"]]))
    net["b_head"] = net["b_head"].copy()
    net["b_head"][0] += np.float32(bias)
    net["enc"] = np.ascontiguousarray(net["enc"][: c["B"], : c["T"]])
    return JW.greedy_net_bf16(net) if bf16 else net


@functools.lru_cache(maxsize=None)
def lm_weights(name, bf16=False):
    """beam_lm_ref.lm_weights of an LM case over the case's vocabulary; ``bf16``: the matrices rounded as the device's bf16 shadows are
    (embedding table, biases and LayerNorm vectors stay fp32)."""
    c = LM_CASES[name]
    lw = BL.lm_weights(c["lm"], V=JW.GREEDY_CASES[CASES[c["case"]]["net"]][0])
    if bf16:
        import torch
        r = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()  # noqa: E731
        lw = {k: (r(v) if v.ndim == 2 and not k.startswith("embedding.") else v) for k, v in lw.items()}
    return lw


def beam_search(enc, weights, beam_size, nbest=NBEST, lm=None, lm_weight=0.0, blank=0, slope=JW.SLOPE, state_beam=2.3, expand_beam=2.3,
                limit=4096):
    """One utterance enc [T, J] in float64; see the module's text for the returned dict. A frame that holds more than ``limit``
    hypotheses raises RuntimeError: with too little blank the search does not end."""
    w = BL.f64(weights)
    use_lm = lm is not None and lm_weight > 0
    lw = BL.f64(lm) if use_lm else None
    enc = np.asarray(enc, np.float64)
    key = lambda hyp: hyp["logp"] / len(hyp["tokens"])  # noqa: E731
    margin = [np.inf]

    def tie(d):
        if d != 0.0:
            margin[0] = min(margin[0], abs(float(d)))

    beam = [dict(tokens=[int(blank)], logp=0.0, pred=None, lm=None, cache=None, frames=[])]
    peak = expansions = 0
    for t in range(enc.shape[0]):
        A, beam = beam, []
        held = len(A)
        while len(beam) < beam_size:
            a = max(A, key=key)
            ka = sorted((key(h) for h in A), reverse=True)
            if len(ka) > 1:
                tie(ka[0] - ka[1])
            if beam:
                best = max(beam, key=key)
                tie(best["logp"] - (state_beam + a["logp"]))
                if best["logp"] >= state_beam + a["logp"]:
                    break
            A.remove(a)
            expansions += 1
            if a["cache"] is None:
                pn, pred = BL.predictor_step(w, a["tokens"][-1], a["pred"])
                lm_lp, lm_state = BL.lm_step(lw, a["tokens"][-1], a["lm"]) if use_lm else (None, None)
                a["cache"] = (pn, pred, lm_lp, lm_state)
            pn, pred, lm_lp, lm_state = a["cache"]
            z = enc[t] + pn
            lp = BL._log_softmax(w["w_head"] @ np.where(z > 0, z, z * slope) + w["b_head"])
            order = sorted(range(lp.shape[0]), key=lambda v: (-lp[v], v))
            if len(order) > beam_size:
                tie(lp[order[beam_size - 1]] - lp[order[beam_size]])
            order = order[:beam_size]
            best_nonblank = lp[order[0]] if order[0] != blank else lp[order[1]]
            for sym in order:
                if sym == blank:
                    beam.append(dict(a, tokens=a["tokens"][:], logp=a["logp"] + lp[sym]))
                    continue
                tie(lp[sym] - (best_nonblank - expand_beam))
                if lp[sym] >= best_nonblank - expand_beam:
                    sc = a["logp"] + lp[sym]
                    if use_lm:
                        sc = sc + lm_weight * lm_lp[sym]
                    A.append(dict(tokens=a["tokens"] + [int(sym)], logp=sc, pred=pred, lm=lm_state, cache=None, frames=a["frames"] + [t]))
                    held += 1
                    if held > limit:
                        raise RuntimeError(f"beam_search: frame {t} holds more than {limit} hypotheses")
        peak = max(peak, held)
    ranked = sorted(beam, key=key, reverse=True)
    for hi, lo in zip(ranked, ranked[1:nbest + 1]):
        tie(key(hi) - key(lo))
    ranked = ranked[:nbest]
    return dict(nbest=[h["tokens"][1:] for h in ranked], scores=[float(key(h)) for h in ranked], frames=[list(h["frames"]) for h in ranked],
                peak=peak, expansions=expansions, margin=float(margin[0]))


@functools.lru_cache(maxsize=None)
def run_case(name, beam, bf16=False, lm_case=None, nbest=NBEST, run=None):
    """The search of every utterance of a case (a tuple of beam_search's dicts); ``lm_case``: fused with that LM_CASES entry, on its
    own (seed name, bias); ``run``: that pair for an unfused search to compare a fused one with."""
    net = case_net(name, beam, bf16, LM_CASES[lm_case]["run"] if lm_case else run)
    lm = lm_weights(lm_case, bf16) if lm_case else None
    weight = LM_CASES[lm_case]["weight"] if lm_case else 0.0
    return tuple(beam_search(net["enc"][b], net, beam, nbest, lm, weight) for b in range(net["enc"].shape[0]))


def beam_case_ok(results, frames):
    """The conditions a tested case meets, ``results`` = run_case's tuple, ``frames`` = T of the case: at most 128 hypotheses in a frame
    (a quarter of the default cap), a best hypothesis of >= 4 tokens in at least two utterances (all but one where there are fewer than
    three), at least 1.25 expansions per frame, every margin >= 1e-4. Returns (ok, peak, long utterances, expansions per frame, margin)."""
    peak = max(r["peak"] for r in results)
    n_long = sum(len(r["nbest"][0]) >= 4 for r in results)
    per_frame = sum(r["expansions"] for r in results) / (frames * len(results))
    mm = min(r["margin"] for r in results)
    return peak <= 128 and n_long >= min(2, len(results)) and per_frame >= 1.25 and mm >= 1e-4, peak, n_long, per_frame, mm
