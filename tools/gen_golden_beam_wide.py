#!/usr/bin/env python3
"""Golden hypotheses for the wide beam search (TEST INFRASTRUCTURE; runs only where the reference is installed).

Imports the reference read-only through oracle/gen_golden.py (import_reference) and runs its own ``TransducerBeamSearcher(beam_size=4,
nbest=3, state_beam=2.3, expand_beam=2.3)`` over its one-hot ``Embedding``, ``LSTM`` and ``Linear`` modules on the ``v64`` and ``v100``
cases of tests/helpers/beam_wide_ref.py (B = 3, T = 24, H = 64, J = 64: the seeded weights and encoder output of ``case_net``, every one a
det_tensor, the head's blank bias raised per case). Each case is run in float32 and in float64: a case where the two differ for the
reference alone, or where the float64 helper disagrees with the reference, is replaced, not tolerated (the generator stops). A stored case
also meets ``beam_case_ok``. tests/golden/c1_beam_wide.npz stores only results: per case ``<case>_hyps`` int16 [3, 3, longest], ``_lens``
int64 [3, 3] (-1: the beam held fewer), ``_scores`` float64 [3, 3] (the float32 run's logp / len).

Run from the repository root:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_beam_wide.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "helpers")]
import gen_golden as G  # noqa: E402
import beam_wide_ref as BW  # noqa: E402
import joint_wide_ref as JW  # noqa: E402

BEAM = 4


def main():
    G.import_reference()
    from speechbrain.decoders.transducer import TransducerBeamSearcher
    from speechbrain.nnet.embedding import Embedding
    from speechbrain.nnet.linear import Linear
    from speechbrain.nnet.RNN import LSTM
    from speechbrain.nnet.transducer.transducer_joint import Transducer_joint

    out = {}
    for name in BW.FIXTURE_CASES:
        V, E, H, J, _ = JW.GREEDY_CASES[BW.CASES[name]["net"]]
        assert E is None
        net = {k: torch.from_numpy(v) for k, v in BW.case_net(name, BEAM).items()}
        emb = Embedding(num_embeddings=V, consider_as_one_hot=True, blank_id=0)
        assert torch.equal(emb.Embedding.weight, net["emb"]), "the helper's one-hot table is not the reference's"
        dec = LSTM(input_shape=[None, None, V - 1], hidden_size=H, num_layers=1)
        dec.rnn.load_state_dict({"weight_ih_l0": net["w_ih"], "weight_hh_l0": net["w_hh"], "bias_ih_l0": net["b_ih"], "bias_hh_l0": net["b_hh"]},
                                strict=True)
        proj = Linear(input_size=H, n_neurons=J)
        proj.load_state_dict({"w.weight": net["w_proj"], "w.bias": net["b_proj"]}, strict=True)
        head = Linear(input_size=J, n_neurons=V)
        head.load_state_dict({"w.weight": net["w_head"], "w.bias": net["b_head"]}, strict=True)
        joiner = Transducer_joint(joint="sum", nonlinearity=torch.nn.LeakyReLU)
        runs = {}
        for dtype in (torch.float32, torch.float64):
            for mod in (emb, dec, proj, head):
                mod.to(dtype).eval()
            bs = TransducerBeamSearcher(decode_network_lst=[emb, dec, proj], tjoint=joiner, classifier_network=[head], blank_id=0, beam_size=BEAM,
                                        nbest=BW.NBEST, state_beam=2.3, expand_beam=2.3)
            with torch.no_grad():
                _, _, nb, sc = bs(net["enc"].to(dtype))
            runs[dtype] = ([[list(map(int, h)) for h in u] for u in nb], [[float(s) for s in u] for u in sc])
        assert runs[torch.float32][0] == runs[torch.float64][0], f"{name}: the reference's float32 and float64 searches differ - replace the case"
        ours = BW.run_case(name, BEAM)
        ok, peak, n_long, per_frame, mm = BW.beam_case_ok(ours, BW.CASES[name]["T"])
        assert ok, (name, peak, n_long, per_frame, mm)
        assert [r["nbest"] for r in ours] == runs[torch.float64][0], f"{name}: the float64 helper disagrees with the reference"
        worst = max(abs(a - b) for r, u in zip(ours, runs[torch.float64][1]) for a, b in zip(r["scores"], u))
        assert worst <= 1e-9, f"{name}: the float64 helper's scores are {worst:.2e} from the reference's"
        nb, sc = runs[torch.float32]
        B = len(nb)
        lens = np.full((B, BW.NBEST), -1, np.int64)
        scores = np.full((B, BW.NBEST), -np.inf, np.float64)
        hyps = np.zeros((B, BW.NBEST, max(1, max(len(h) for u in nb for h in u))), np.int16)
        for b in range(B):
            for r, h in enumerate(nb[b]):
                lens[b, r], scores[b, r] = len(h), sc[b][r]
                hyps[b, r, : len(h)] = h
        out[f"{name}_hyps"], out[f"{name}_lens"], out[f"{name}_scores"] = hyps, lens, scores
        print(f"beam {name}: best lengths {lens[:, 0].tolist()}, peak {peak}, expansions per frame {per_frame:.2f}, smallest margin {mm:.2e}")
    np.savez_compressed(os.path.join(G.OUT, "c1_beam_wide.npz"), **out)


if __name__ == "__main__":
    main()
