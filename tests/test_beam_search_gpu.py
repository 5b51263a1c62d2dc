"""Beam transducer search on the MI355X (csrc/search.hip: tsasr_beam_search, offline and in streams) against the reference's golden
hypotheses, the CPU oracle and the host loop it replaces; determinism, streams decoded in pieces, overflow, the streaming transcriber and
the recipe's TEST stage."""
import contextlib
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from oracle import tsasr_ref as R  # noqa: E402
from oracle.golden_recipe import CFG1, det_tensor  # noqa: E402
from tests.test_oracle_golden import full_state_dict  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dec = importlib.import_module("ts-asr_amd.decoders")
ops = importlib.import_module("ts-asr_amd.ops")
nnet = importlib.import_module("ts-asr_amd.nnet")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


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


def searcher(m, beam, nbest=1, cap=dec.BEAM_CAP):
    return dec.TransducerBeamSearcher([m.embedding, m.decoder, m.decoder_proj], m.joiner, [m.transducer_head], blank_id=0, beam_size=beam,
                                      nbest=nbest, state_beam=2.3, expand_beam=2.3, cap=cap)


@contextlib.contextmanager
def blank_shift(head, shift):
    """The golden fixtures raise the head's blank bias (oracle/gen_golden_beam.py) so that the reference's loop ends."""
    with torch.no_grad():
        head.w.bias[0] += shift
    try:
        yield
    finally:
        with torch.no_grad():
            head.w.bias[0] -= shift


def second_enc(golden, B=6, Tn=40):
    """A second encoder output: the golden one reversed in time and rolled over the batch, plus seeded noise. (Plain seeded noise of
    the same scale makes blank rare among the best 2-4 symbols, and the reference's expansion loop then does not end in useful time.)"""
    c = golden["c1_chain_cat"]["enc_proj"]
    base = np.concatenate([c[:, ::-1], np.roll(c, 1, axis=0)], 0)[:B, :Tn]
    return T(base + det_tensor("beam.enc_proj.2", base.shape, 0.05))


def tolerance(hyps, scores, ref_hyps, ref_scores):
    """The golden test's rule: equal sequence or equal normalised score (5e-4), all scores within 1e-3, half of them exact."""
    exact = 0
    for b in range(len(ref_hyps)):
        exact += hyps[b] == ref_hyps[b]
        assert hyps[b] == ref_hyps[b] or abs(scores[b] - ref_scores[b]) < 5e-4, b
        assert abs(scores[b] - ref_scores[b]) < 1e-3, b
    assert 2 * exact >= len(ref_hyps), exact
    return exact


@pytest.mark.parametrize("beam", [4, 15])
def test_device_beam_vs_reference_golden(brains, golden, beam):
    """Device route, fp32, against the reference's hypotheses (tests/golden/c1_beam.npz). Measured: 4 of 4 utterances exact at beam 4
    and at beam 15 (printed)."""
    brain, h = brains("fp32")
    g = golden["c1_beam"]
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"]).to(DEV)
    with blank_shift(m.transducer_head, float(g["blank_bias"])), torch.no_grad():
        s = searcher(m, beam)
        assert s._device_beam_ok(enc)
        hyps, _, _, scores = s(enc)
    ref = [g[f"beam{beam}_hyps"][b, : g[f"beam{beam}_lens"][b]].tolist() for b in range(4)]
    exact = tolerance(hyps, [x[0] for x in scores], ref, g[f"beam{beam}_scores"].tolist())
    print(f"beam {beam}: {exact} of 4 utterances exact")


@pytest.mark.parametrize("beam", [2, 4, 15])
def test_device_beam_vs_oracle(brains, golden, beam):
    """Device fp32 against oracle.beam_decode on a second seeded encoder output (golden weights, shifted blank bias)."""
    brain, h = brains("fp32")
    shift = float(golden["c1_beam"]["blank_bias"])
    enc = second_enc(golden)
    sd = full_state_dict(CFG1, "cat")
    sd["transducer_head.w.bias"] = sd["transducer_head.w.bias"].clone()
    sd["transducer_head.w.bias"][0] += shift
    with torch.no_grad():
        ref_hyps, ref_scores = R.beam_decode(enc, sd, CFG1, beam_size=beam)
    m = brain.modules
    with blank_shift(m.transducer_head, shift), torch.no_grad():
        s = searcher(m, beam)
        assert s._device_beam_ok(enc.to(DEV))
        hyps, _, _, scores = s(enc.to(DEV))
    exact = tolerance(hyps, [x[0] for x in scores], ref_hyps, ref_scores)
    print(f"beam {beam}: {exact} of {len(ref_hyps)} exact")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_beam_equals_host_loop(brains, golden, dtype, monkeypatch):
    """Device against the host loop (TSASR_BEAM_KERNEL=0) on the same inputs, whole n-best (nbest 3). fp32: the tolerance rule on every
    rank; bf16 (the loop keeps the predictor output in bf16, the kernel in fp32): at least 3 of 4 utterances identical. The bf16 case
    runs the first 12 frames: over all 40 the hypotheses (~110 symbols) pass enough near-ties that 1 of 4 stayed identical."""
    brain, h = brains(dtype)
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    m = brain.modules
    enc = second_enc(golden, 4, 40 if dtype == "fp32" else 12).to(DEV, dt)
    with blank_shift(m.transducer_head, float(golden["c1_beam"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, nbest=3)
        assert s._device_beam_ok(enc)
        _, _, nb_k, sc_k = s(enc)
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        assert not s._device_beam_ok(enc)
        _, _, nb_h, sc_h = s(enc)
    if dtype == "fp32":
        for r in range(3):
            tolerance([n[r] for n in nb_k], [x[r] for x in sc_k], [n[r] for n in nb_h], [x[r] for x in sc_h])
    else:
        same = sum(a == b for a, b in zip(nb_k, nb_h))
        assert same >= 3, (same, nb_k, nb_h)


def test_device_beam_deterministic(brains, golden):
    brain, h = brains("fp32")
    m = brain.modules
    enc = second_enc(golden).to(DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 15, nbest=5)
        r1 = s(enc)
        r2 = s(enc)
    assert r1[2] == r2[2]
    assert all(np.array(a, np.float64).tobytes() == np.array(b, np.float64).tobytes() for a, b in zip(r1[3], r2[3]))


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_beam_stream_pieces_bit_identical(brains, golden, route, dtype, monkeypatch):
    """beam_stream in chunks of 1, 7, 40 and whole, and with ragged counts (one stream ends early, zero-count chunks) gives the bits of
    one call of the same route over each utterance's valid prefix: hypotheses, lengths and fp64 scores."""
    brain, h = brains(dtype)
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    if route == "host":
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
    m = brain.modules
    B, Tn = (3, 40) if route == "device" else (2, 12)
    enc = second_enc(golden, B, Tn).to(DEV, dt)
    lens = [Tn, Tn * 2 // 3, 5][:B]
    with blank_shift(m.transducer_head, float(golden["c1_beam"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, nbest=3)
        assert s._device_beam_ok(enc) == (route == "device")
        ref = [s(enc[b:b + 1, : lens[b]]) for b in range(B)]
        ref_nb = [r[2][0] for r in ref]
        ref_sc = [r[3][0] for r in ref]
        for chunk in ([1, 7, 40] if route == "device" else [1, 7]) + [Tn]:
            state = None
            for t0 in range(0, Tn, chunk):
                c = min(chunk, Tn - t0)
                nv = torch.tensor([min(max(lens[b] - t0, 0), c) for b in range(B)], dtype=torch.int32)
                best, state = s.beam_stream(enc[:, t0:t0 + c], state, nv, max_frames=Tn)
                if chunk == 7 and t0 == 7:       # a chunk with zero counts everywhere leaves every stream where it was
                    before = (state["nbest"], state["scores"])
                    _, state = s.beam_stream(enc[:, t0:t0 + c], state, torch.zeros(B, dtype=torch.int32), max_frames=Tn)
                    assert (state["nbest"], state["scores"]) == before
            assert state["nbest"] == ref_nb, chunk
            assert [np.array(x, np.float64).tobytes() for x in state["scores"]] == [np.array(x, np.float64).tobytes() for x in ref_sc], chunk
            assert best == [n[0] for n in ref_nb]


def test_beam_overflow_status_and_host_redecode(brains, golden, monkeypatch):
    """A tiny cap stops the utterances that need more hypotheses in a frame (status word, not a fault); the searcher decodes those again
    on the host loop, the others keep the device result; beam_stream raises instead."""
    brain, h = brains("fp32")
    m = brain.modules
    enc = second_enc(golden, 6, 12)
    enc[3:] = 0.0                      # blank wins every frame there: A never holds more than the beam
    enc = enc.to(DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, nbest=2)
        table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)
        run = lambda e, cap: ops.beam_search(e, table, mats, b_ih, b_hh, b_proj, b_head, 0, s.tjoint.nonlinearity.negative_slope, wdt,  # noqa: E731
                                             4, 2, 2.3, 2.3, cap)
        nb_full, sc_full, st_full = run(enc, dec.BEAM_CAP)
        assert st_full.tolist() == [0] * 6
        for cap in range(4, 64):                         # the smallest cap that stops some utterances but not all
            nb, sc, status = run(enc, cap)
            bad = [b for b in range(6) if status[b] != 0]
            if 0 < len(bad) < 6:
                break
        assert 0 < len(bad) < 6, "no cap separates the utterances"
        s.cap = cap
        per_utt = [int(run(enc[b:b + 1], cap)[2][0]) for b in range(6)]
        assert status.tolist() == per_utt                                 # each utterance's status is its own
        assert all(int(status[b]) == 1 for b in bad), status
        assert all(nb[b] == [] for b in bad)
        assert all(nb[b] == nb_full[b] and sc[b] == sc_full[b] for b in range(6) if b not in bad)   # the others are unaffected
        before = dec.BEAM_HOST_REDECODES["utterances"]
        with pytest.warns(RuntimeWarning) if before == 0 else contextlib.nullcontext():
            _, _, nb_d, sc_d = s(enc)
        assert dec.BEAM_HOST_REDECODES["utterances"] == before + len(bad)
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        _, _, nb_h, sc_h = s(enc)
        monkeypatch.delenv("TSASR_BEAM_KERNEL")
        for b in bad:
            assert nb_d[b] == nb_h[b] and sc_d[b] == sc_h[b]
        with pytest.raises(RuntimeError, match="cap"):
            s.beam_stream(enc, None, None, max_frames=12)


def test_streaming_transcriber_beam_equals_offline(golden, monkeypatch):
    """StreamingTranscriber(search="beam") on a causal golden model: finish() and nbest() are the bits of the offline device search over
    encoder_proj of the stream's encoder output; under TSASR_STRICT_HIP no library route is taken."""
    streaming = importlib.import_module("ts-asr_amd.streaming")
    monkeypatch.setattr(ops, "STRICT_HIP", True)
    ops.LIB_FALLBACKS.clear()
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal")
    try:
        s = h["beam_searcher"]
        s.beam_size, s.nbest = 4, 3
        feats = T(golden["c1_features"]["norm"]).to(DEV)
        spk = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)
        with blank_shift(s.classifier_network[0], float(golden["c1_beam"]["blank_bias"])), torch.no_grad():
            st = streaming.StreamingTranscriber(brain, search="beam")
            st.start(feats.shape[0], max_frames=(feats.shape[1] + 3) // 4, speaker_embs=spk, keep_encoder_out=True)
            F = feats.shape[1]
            for f0 in range(0, F, 32):
                best = st.push(feats[:, f0:f0 + 32], last=f0 + 32 >= F)
                assert len(best) == 4 and all(isinstance(x, list) for x in best)
            hyps = st.finish()
            nb, sc = st.nbest()
            enc = brain.modules.encoder_proj(st.encoder_out())
            assert s._device_beam_ok(enc)
            off_best, _, off_nb, off_sc = s(enc)
        assert hyps == off_best and nb == off_nb
        assert [np.array(x, np.float64).tobytes() for x in sc] == [np.array(x, np.float64).tobytes() for x in off_sc]
        assert ops.LIB_FALLBACKS == {}
    finally:
        nnet.set_compute_dtype(torch.bfloat16)


def test_recipe_test_stage_takes_device_route(monkeypatch):
    """A small fp32 recipe run whose TEST stage goes through the device beam search: brain.last_hyps equal a host-loop evaluation of the
    same batches under the tolerance rule (hypotheses; the n-best scores are compared where the route exposes them)."""
    main = importlib.import_module("train_tsasr").main
    argv = [os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml"), "--device", "cuda:0", "--synthetic", "2", "--number_of_epochs",
            "1", "--syn_batch", "4", "--syn_seconds", "2.0", "--syn_enroll_seconds", "1.0", "--syn_tokens", "12", "--hip_graph", "False",
            "--lr", "0.002", "--warmup_steps", "5", "--dropout", "0.0", "--beam_size", "3", "--d_model", "144", "--nhead", "4",
            "--encoder_num_layers", "2", "--speaker_num_layers", "2", "--d_ffn", "576", "--joint_dim", "160", "--decoder_neurons", "128",
            "--compute_dtype", "fp32"]
    taken = []
    orig = dec.TransducerBeamSearcher._beam_on_device

    def spy(self, tn_output):
        out = orig(self, tn_output)
        taken.append((tn_output.detach().clone(), self, out))
        return out
    monkeypatch.setattr(dec.TransducerBeamSearcher, "_beam_on_device", spy)
    ops.LIB_FALLBACKS.clear()
    try:
        brain, result = main(argv)
        assert taken, "the TEST stage did not take the device beam search"
        assert ops.LIB_FALLBACKS == {}, ops.LIB_FALLBACKS
        enc, s, (best, _, nb, sc) = taken[-1]
        assert brain.last_hyps == best
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        with torch.no_grad():
            best_h, _, nb_h, sc_h = s(enc)
        tolerance(best, [x[0] for x in sc], best_h, [x[0] for x in sc_h])
    finally:
        nnet.set_compute_dtype(torch.bfloat16)
