#!/usr/bin/env python3
"""Golden vectors for the wide-vocabulary joint (TEST INFRASTRUCTURE; runs only where the reference is installed).

Imports the reference read-only through oracle/gen_golden.py (import_reference) and runs its own ``Transducer_joint(joint="sum",
nonlinearity=LeakyReLU)`` followed by its ``Linear`` head in float32 on [2, 7, 64] encoder and [2, 5, 64] predictor projections, at
V = 33 and V = 100. Inputs and weights are the seeded tensors of tests/helpers/joint_wide_ref.py ``fixture_inputs`` (every one a det_tensor), so
tests/golden/c1_wide_vocab.npz stores only results: ``logits_v33`` and ``logits_v100`` [2, 7, 5, V] float32.

Greedy search: the reference's own ``TransducerBeamSearcher(beam_size=1)`` over its one-hot ``Embedding``, ``LSTM`` and ``Linear`` modules at
V = 64 and V = 100 (B = 3, T = 40, H = 64, J = 64; the seeded weights and encoder output of ``greedy_net``, the head's blank bias raised by
3 as in oracle/gen_golden_beam.py). Each case is run in float32 and in float64: a case where the two differ for the reference alone is
replaced, not tolerated (the generator stops). A stored case also meets ``greedy_case_ok`` (a quarter blank and a quarter emitting decisions
at least, float64 top-2 logit margin >= 1e-4 at every decision). Stored: ``greedy_<case>_hyps`` int16 [3, longest] and ``_lens``.

Run from the repository root:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_wide_vocab.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "helpers")]
import gen_golden as G  # noqa: E402
import joint_wide_ref as JW  # noqa: E402


def main():
    G.import_reference()
    from speechbrain.nnet.linear import Linear
    from speechbrain.nnet.transducer.transducer_joint import Transducer_joint

    out = {}
    for V in JW.FIXTURE_VOCABS:
        enc, dec, W, b = (torch.from_numpy(x) for x in JW.fixture_inputs(V))
        joiner = Transducer_joint(joint="sum", nonlinearity=torch.nn.LeakyReLU)
        head = Linear(input_size=enc.shape[-1], n_neurons=V)
        head.load_state_dict({"w.weight": W, "w.bias": b}, strict=True)
        with torch.no_grad():
            logits = head(joiner(enc.unsqueeze(2), dec.unsqueeze(1)))
        assert logits.shape == (*JW.FIXTURE_SHAPE[:3], V) and logits.dtype == torch.float32
        out[f"logits_v{V}"] = logits.numpy()
        print(f"V={V}: logits {tuple(logits.shape)}, |max| {float(logits.abs().max()):.3f}")
    from speechbrain.decoders.transducer import TransducerBeamSearcher
    from speechbrain.nnet.embedding import Embedding
    from speechbrain.nnet.RNN import LSTM

    for name in JW.FIXTURE_GREEDY:
        V, E, H, J, _ = JW.GREEDY_CASES[name]
        assert E is None
        net = {k: torch.from_numpy(v) for k, v in JW.greedy_net(name).items()}
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
            bs = TransducerBeamSearcher(decode_network_lst=[emb, dec, proj], tjoint=joiner, classifier_network=[head], blank_id=0, beam_size=1)
            with torch.no_grad():
                runs[dtype] = bs(net["enc"].to(dtype))[0]
        assert runs[torch.float32] == runs[torch.float64], f"{name}: the reference's float32 and float64 searches differ - replace the case"
        ours = JW.greedy(JW.greedy_net(name))
        ok, fb, fe, mm = JW.greedy_case_ok(ours)
        assert ok, (name, fb, fe, mm)
        assert [r["tokens"] for r in ours] == runs[torch.float64], f"{name}: the float64 helper disagrees with the reference"
        hyps = runs[torch.float32]
        lens = np.array([len(h) for h in hyps], np.int64)
        pad = np.zeros((len(hyps), max(1, lens.max())), np.int16)
        for i, h in enumerate(hyps):
            pad[i, : len(h)] = h
        out[f"greedy_{name}_hyps"], out[f"greedy_{name}_lens"] = pad, lens
        print(f"greedy {name}: lengths {lens.tolist()}, blank {fb:.2f} emit {fe:.2f}, smallest margin {mm:.2e}")
    np.savez_compressed(os.path.join(G.OUT, "c1_wide_vocab.npz"), **out)


if __name__ == "__main__":
    main()
