#!/usr/bin/env python3
"""Golden vectors for the beam transducer search with LM fusion (TEST INFRASTRUCTURE; runs only where the reference is installed).

Imports the reference read-only through oracle/gen_golden.py (import_reference / build) and runs its own TransducerBeamSearcher with its
own RNNLM (lm_module, lm_weight > 0) on the golden encoder output of tests/golden/c1_chain_cat.npz (4 x 50 x 160) with the recipe model
and blank bias of oracle/gen_golden_beam.py. The LMs are the seeded ones of tests/helpers/beam_lm_ref.py (LM_CONFIGS: every tensor is
det_tensor("lm.<cfg>.<key>", shape, scale)), so tests/golden/c1_beam_lm.npz stores only results: per case (LM, frames, beam) the n-best
(nbest 3) hypotheses, their lengths, their logp / len and how many the beam held; per LM the reference's state_dict keys and shapes.

Every case is run twice, with all modules and inputs in float32 and in float64, and the two are compared by the project's tolerance rule
(equal sequence or normalised score within 5e-4; every score within 1e-3; at least half of the utterances exact on every rank): a case
outside it for the reference alone must be replaced, not tolerated. The float32 results are stored.

Run from the repository root:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_beam_lm.py
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "helpers")]
import beam_lm_ref as BL  # noqa: E402
import gen_golden as G  # noqa: E402

BLANK_BIAS = 3.0


def pack(nbest, scores):
    B = len(nbest)
    count = np.array([len(n) for n in nbest], np.int64)
    lens = np.full((B, BL.NBEST), -1, np.int64)
    longest = max([len(h) for n in nbest for h in n] + [1])
    hyps = np.zeros((B, BL.NBEST, longest), np.int16)
    sc = np.zeros((B, BL.NBEST), np.float64)
    for b in range(B):
        for r, h in enumerate(nbest[b]):
            lens[b, r] = len(h)
            hyps[b, r, : len(h)] = h
            sc[b, r] = float(scores[b][r])
    return hyps, lens, sc, count


def agree(a, b):
    """The tolerance rule between two runs ((n-best, scores) each); returns (worst score difference, utterances exact on every rank)."""
    worst, exact = 0.0, 0
    for ha, sa, hb, sb in zip(a[0], a[1], b[0], b[1]):
        assert len(ha) == len(hb), "the two precisions hold different numbers of hypotheses"
        for r in range(len(ha)):
            d = abs(float(sa[r]) - float(sb[r]))
            worst = max(worst, d)
            assert ha[r] == hb[r] or d < 5e-4, (r, d)
            assert d < 1e-3, (r, d)
        exact += ha == hb
    assert 2 * exact >= len(a[0]), exact
    return worst, exact


def main():
    torch.manual_seed(0)
    G.import_reference()
    from speechbrain.decoders.transducer import TransducerBeamSearcher
    from speechbrain.lobes.models.RNNLM import RNNLM

    cfg = G.CFG1
    V = cfg["vocab_size"]
    enc32 = torch.from_numpy(np.load(os.path.join(G.OUT, "c1_chain_cat.npz"))["enc_proj"]).float()
    m = G.build(cfg, "cat", False, "same")
    with torch.no_grad():
        m["transducer_head"].w.bias[0] += BLANK_BIAS
    out = {"blank_bias": np.array(BLANK_BIAS)}
    lms = {}
    for name, c in BL.LM_CONFIGS.items():
        lm = RNNLM(output_neurons=V, embedding_dim=c["emb"], dropout=0.0, rnn_layers=c["layers"], rnn_neurons=c["hidden"], return_hidden=True,
                   dnn_blocks=c["blocks"], dnn_neurons=c["dnn"])
        sd = lm.state_dict()
        out[f"keys_{name}"] = np.array(list(sd))
        out[f"shapes_{name}"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], np.int64)
        lm.load_state_dict({k: torch.from_numpy(v) for k, v in BL.lm_weights(name, V).items()}, strict=True)
        lms[name] = lm.eval()
        print(name, list(sd))
    net = [m["embedding"], m["decoder"], m["decoder_proj"], m["joiner"], m["transducer_head"]]

    def run(dtype):
        res = {}
        for mod in net + list(lms.values()):
            mod.to(dtype)
        for name, c in BL.LM_CONFIGS.items():
            for T in BL.FRAMES:
                for beam in BL.BEAMS:
                    bs = TransducerBeamSearcher(decode_network_lst=net[:3], tjoint=net[3], classifier_network=[net[4]], blank_id=0,
                                                beam_size=beam, nbest=BL.NBEST, lm_module=lms[name], lm_weight=c["weight"], state_beam=2.3,
                                                expand_beam=2.3)
                    t0 = time.time()
                    with torch.no_grad():
                        _, _, nbest, scores = bs(enc32[:, :T].to(dtype))
                    res[BL.case_key(name, T, beam)] = (nbest, [[float(s) for s in row] for row in scores])
                    print(f"{dtype} {BL.case_key(name, T, beam)}: {time.time() - t0:.1f} s, lengths {[[len(h) for h in n] for n in nbest]}", flush=True)
        return res

    r32 = run(torch.float32)
    r64 = run(torch.float64)
    worst_all = 0.0
    for k in r32:
        worst, exact = agree(r32[k], r64[k])
        worst_all = max(worst_all, worst)
        print(f"fp32 vs fp64 {k}: worst score difference {worst:.2e}, {exact} of {len(r32[k][0])} utterances exact on every rank")
        out[k + "_hyps"], out[k + "_lens"], out[k + "_scores"], out[k + "_count"] = pack(*r32[k])
    print(f"fp32 vs fp64 over all cases: worst score difference {worst_all:.2e}")
    np.savez_compressed(os.path.join(G.OUT, "c1_beam_lm.npz"), **out)


if __name__ == "__main__":
    main()
