"""Beam transducer search with LM fusion on the MI355X (csrc/search.hip: tsasr_beam_search with lm): the device route against the reference's
own hypotheses (tests/golden/c1_beam_lm.npz), the float64 restatement (tests/helpers/beam_lm_ref.py) and the host loop; LMs the kernel
does not take; lm_weight = 0; streams; overflow; the reference-default LM's width; the launcher's argument checks; the recipe."""
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
import beam_lm_ref as BL  # noqa: E402
from oracle.golden_recipe import det_tensor  # noqa: E402
from tiny_lm import TinyLM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
dec = importlib.import_module("ts-asr_amd.decoders")
ops = importlib.import_module("ts-asr_amd.ops")
nnet = importlib.import_module("ts-asr_amd.nnet")
capi = importlib.import_module("ts-asr_amd._capi")
V = 29


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def bits(scores):
    return [np.array(x, np.float64).tobytes() for x in scores]


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
def lms():
    """The fixture's LMs as nnet.RNNLM on the device, built once."""
    out = {}

    def get(name):
        if name not in out:
            c = BL.LM_CONFIGS[name]
            lm = nnet.RNNLM(V, embedding_dim=c["emb"], dropout=0.0, rnn_layers=c["layers"], rnn_neurons=c["hidden"], return_hidden=True,
                            dnn_blocks=c["blocks"], dnn_neurons=c["dnn"])
            lm.load_state_dict({k: T(v) for k, v in BL.lm_weights(name).items()}, strict=True)
            out[name] = lm.to(DEV).eval()
        return out[name]
    return get


def searcher(m, beam, lm=None, lm_weight=0.0, nbest=BL.NBEST, cap=dec.BEAM_CAP):
    return dec.TransducerBeamSearcher([m.embedding, m.decoder, m.decoder_proj], m.joiner, [m.transducer_head], blank_id=0, beam_size=beam,
                                      nbest=nbest, lm_module=lm, lm_weight=lm_weight, state_beam=2.3, expand_beam=2.3, cap=cap)


@contextlib.contextmanager
def blank_shift(head, shift):
    """The golden fixtures raise the head's blank bias so that the reference's loop ends."""
    with torch.no_grad():
        head.w.bias[0] += shift
    try:
        yield
    finally:
        with torch.no_grad():
            head.w.bias[0] -= shift


def second_enc(golden, B=6, Tn=40):
    """A second encoder output: the golden one reversed in time and rolled over the batch, plus seeded noise (as the plain beam test
    builds it: plain noise of this scale makes blank rare among the best symbols and the expansion loop long)."""
    c = golden["c1_chain_cat"]["enc_proj"]
    base = np.concatenate([c[:, ::-1], np.roll(c, 1, axis=0)], 0)[:B, :Tn]
    return T(base + det_tensor("beam.enc_proj.2", base.shape, 0.05))


def tolerance(hyps, scores, ref_hyps, ref_scores):
    """The project's rule: equal sequence or equal normalised score (5e-4), all scores within 1e-3, half of the sequences exact."""
    exact = 0
    for b in range(len(ref_hyps)):
        exact += hyps[b] == ref_hyps[b]
        assert hyps[b] == ref_hyps[b] or abs(scores[b] - ref_scores[b]) < 5e-4, b
        assert abs(scores[b] - ref_scores[b]) < 1e-3, b
    assert 2 * exact >= len(ref_hyps), exact
    return exact


def tolerance_ranks(nb, sc, ref_nb, ref_sc):
    """The rule on every rank the reference side holds; both sides hold as many."""
    assert [len(n) for n in nb] == [len(n) for n in ref_nb]
    exact = []
    for r in range(max(len(n) for n in ref_nb)):
        rows = [b for b in range(len(ref_nb)) if len(ref_nb[b]) > r]
        exact.append(tolerance([nb[b][r] for b in rows], [sc[b][r] for b in rows], [ref_nb[b][r] for b in rows], [ref_sc[b][r] for b in rows]))
    return exact


@pytest.mark.parametrize("beam", BL.BEAMS)
@pytest.mark.parametrize("name", sorted(BL.LM_CONFIGS))
def test_device_lm_vs_reference_golden(brains, lms, golden, name, beam):
    """Device route, fp32, T = 50, against the reference's TransducerBeamSearcher with its RNNLM: L = 1, 2, 3 layers, 0, 1, 2 dnn blocks,
    Hl = 40 (no multiple of 64), embedding_dim = 72 (past gemv_rows' 64-column side operand). On the parent the constructor raises
    NotImplementedError."""
    brain, h = brains("fp32")
    g = golden["c1_beam_lm"]
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"]).to(DEV)
    with blank_shift(m.transducer_head, float(g["blank_bias"])), torch.no_grad():
        s = searcher(m, beam, lms(name), BL.LM_CONFIGS[name]["weight"])
        assert s._device_beam_ok(enc)
        _, _, nb, sc = s(enc)
    ref = [BL.fixture_case(g, name, 50, beam, b) for b in range(4)]
    exact = tolerance_ranks(nb, sc, [r[0] for r in ref], [r[1] for r in ref])
    print(f"{name} beam {beam}: utterances exact per rank {exact}")


@pytest.mark.parametrize("beam", [4, 15])
@pytest.mark.parametrize("name", ["l2b1e72", "l3b2h40"])
def test_device_lm_vs_float64(brains, lms, golden, name, beam):
    """Device fp32 against the float64 restatement on a second encoder output."""
    brain, h = brains("fp32")
    shift = float(golden["c1_beam_lm"]["blank_bias"])
    enc = second_enc(golden)
    w, lw, weight = BL.predictor_weights(shift), BL.lm_weights(name), BL.LM_CONFIGS[name]["weight"]
    ref = [BL.beam_search_lm(enc[b].numpy(), w, lw, weight, beam) for b in range(enc.shape[0])]
    m = brain.modules
    with blank_shift(m.transducer_head, shift), torch.no_grad():
        s = searcher(m, beam, lms(name), weight)
        assert s._device_beam_ok(enc.to(DEV))
        _, _, nb, sc = s(enc.to(DEV))
    exact = tolerance_ranks(nb, sc, [r[0] for r in ref], [r[1] for r in ref])
    print(f"{name} beam {beam}: utterances exact per rank {exact}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_lm_equals_host_loop(brains, lms, golden, dtype, monkeypatch):
    """Device against the host loop (TSASR_BEAM_KERNEL=0) with the same LM, nbest 3, beam 4. fp32, T = 24: the tolerance rule on every
    rank. bf16 (the loop keeps the predictor's and the LM's activations in bf16, the kernel in fp32), the first 12 frames: at least 3
    of 4 utterances identical, the plain beam test's form."""
    brain, h = brains(dtype)
    dt = torch.float32 if dtype == "fp32" else torch.bfloat16
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:, : 24 if dtype == "fp32" else 12].to(DEV, dt)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, lms("l2b1e72"), 0.3)
        assert s._device_beam_ok(enc)
        _, _, nb_k, sc_k = s(enc)
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        assert not s._device_beam_ok(enc)
        _, _, nb_h, sc_h = s(enc)
    if dtype == "fp32":
        print("utterances exact per rank", tolerance_ranks(nb_k, sc_k, nb_h, sc_h))
    else:
        same = sum(a == b for a, b in zip(nb_k, nb_h))
        print("bf16: utterances identical", same)
        assert same >= 3, (same, nb_k, nb_h)


def test_host_loop_takes_other_lms(brains, golden):
    """A module that is no nnet.RNNLM, with the (tokens, hx) -> (logits, hidden) form: the searcher takes the host route and matches the
    float64 restatement with that module's step; so do RNNLM shapes the kernel refuses (5 layers) and an LM left in train mode."""
    brain, h = brains("fp32")
    shift = float(golden["c1_beam_lm"]["blank_bias"])
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:, :24]
    lm = TinyLM(V).to(DEV).eval()
    w = BL.predictor_weights(shift)
    ref = [BL.beam_search_lm(enc[b].numpy(), w, {}, 0.5, 4, step=lm.numpy_step()) for b in range(4)]
    with blank_shift(m.transducer_head, shift), torch.no_grad():
        s = searcher(m, 4, lm, 0.5)
        assert not s._device_beam_ok(enc.to(DEV))
        _, _, nb, sc = s(enc.to(DEV))
        plain = searcher(m, 4)(enc.to(DEV))
    assert nb != plain[2]
    print("utterances exact per rank", tolerance_ranks(nb, sc, [r[0] for r in ref], [r[1] for r in ref]))
    deep = nnet.RNNLM(V, embedding_dim=16, rnn_layers=5, rnn_neurons=32, dnn_blocks=0, dnn_neurons=32, return_hidden=True).to(DEV).eval()
    assert not searcher(m, 4, deep, 0.5)._device_beam_ok(enc.to(DEV))
    odd = nnet.RNNLM(V, embedding_dim=16, rnn_layers=1, rnn_neurons=30, dnn_blocks=0, dnn_neurons=30, return_hidden=True).to(DEV).eval()
    assert not searcher(m, 4, odd, 0.5)._device_beam_ok(enc.to(DEV))
    ok = nnet.RNNLM(V, embedding_dim=16, rnn_layers=1, rnn_neurons=32, dnn_blocks=0, dnn_neurons=32, return_hidden=True).to(DEV)
    assert not searcher(m, 4, ok, 0.5)._device_beam_ok(enc.to(DEV))          # train mode: dropout would be live in the host loop
    assert searcher(m, 4, ok.eval(), 0.5)._device_beam_ok(enc.to(DEV))


def _entry_points(s, enc, nv):
    """(n-best, score bits, status) of the four LM-free forms (offline / stream, untimed / timed) on enc."""
    out = []
    for frames in (False, True):
        r = s._device_beam_call(enc, ops.beam_search, frames=frames)
        out.append((r[0], bits(r[1]), r[2].tolist()) + tuple(r[3:]))
        ws = torch.zeros(ops.beam_workspace_bytes(enc.shape[0], enc.shape[1], 128, 160, V, s.beam_size, s.cap, times=frames),
                         dtype=torch.uint8, device=enc.device)
        r = s._device_beam_call(enc, ops.beam_search_stream, ws, nv, enc.shape[1], frames=frames)
        out.append((r[0], bits(r[1]), r[2].tolist()) + tuple(r[3:]))
    return out


def test_lm_weight_zero_is_the_plain_search(brains, lms, golden):
    """A searcher given an LM with lm_weight = 0 returns the bits of the searcher without it (hypotheses, scores, status); the four
    LM-free forms return the same bits before and after a fused search ran in the process."""
    brain, h = brains("fp32")
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"]).to(DEV)
    nv = torch.full((4,), 50, dtype=torch.int32, device=DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        plain, zero = searcher(m, 4), searcher(m, 4, lms("l2b1e72"), 0.0)
        assert zero._device_beam_ok(enc)
        before = _entry_points(plain, enc, nv)
        assert _entry_points(zero, enc, nv) == before
        a, b = plain(enc), zero(enc)
        assert a[0] == b[0] and a[2] == b[2] and bits(a[3]) == bits(b[3]) and float(a[1]) == float(b[1])
        fused = searcher(m, 4, lms("l2b1e72"), 0.3)(enc)
        assert fused[2] != a[2]
        assert _entry_points(plain, enc, nv) == before
    # greedy never uses the LM
    with torch.no_grad():
        assert searcher(m, 1, lms("l2b1e72"), 0.3)(enc)[0] == searcher(m, 1)(enc)[0]


@pytest.mark.parametrize("route", ["device", "host"])
def test_lm_stream_pieces_bit_identical(brains, lms, golden, route, monkeypatch):
    """beam_stream with an LM in chunks of 7 frames with ragged counts (one stream ends early, one chunk with a zero count for every
    stream) gives the bits of one call over each stream's valid prefix, timed and untimed, on both routes; the timed search gives the
    untimed hypotheses and score bits, and frames that do not decrease."""
    brain, h = brains("fp32")
    if route == "host":
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
    m = brain.modules
    B, Tn = (3, 24) if route == "device" else (2, 12)
    enc = second_enc(golden, B, Tn).to(DEV)
    lens = [Tn, Tn * 2 // 3, 5][:B]
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, lms("l3b2h40" if route == "device" else "l2b1e72"), 0.3)      # (the host loop's LayerNorm kernel: widths % 8)
        assert s._device_beam_ok(enc) == (route == "device")
        ref = [s.forward_timed(enc[b:b + 1, : lens[b]]) for b in range(B)]
        untimed = [s(enc[b:b + 1, : lens[b]]) for b in range(B)]
        assert [r[2] for r in ref] == [u[2] for u in untimed] and [bits(r[3]) for r in ref] == [bits(u[3]) for u in untimed]
        ref_nb, ref_sc, ref_fr = [r[2][0] for r in ref], [r[3][0] for r in ref], [r[5][0] for r in ref]
        assert all(fr == sorted(fr) and len(fr) == len(hy) for nb, nf in zip(ref_nb, ref_fr) for hy, fr in zip(nb, nf))
        for frames in (False, True):
            state = None
            for t0 in range(0, Tn, 7):
                c = min(7, Tn - t0)
                nv = torch.tensor([min(max(lens[b] - t0, 0), c) for b in range(B)], dtype=torch.int32)
                best, state = s.beam_stream(enc[:, t0:t0 + c], state, nv, max_frames=Tn, return_frames=frames)
                if t0 == 7:
                    before = (state["nbest"], state["scores"])
                    _, state = s.beam_stream(enc[:, t0:t0 + c], state, torch.zeros(B, dtype=torch.int32), max_frames=Tn, return_frames=frames)
                    assert (state["nbest"], state["scores"]) == before
            assert state["nbest"] == ref_nb and bits(state["scores"]) == bits(ref_sc)
            assert best == [n[0] for n in ref_nb]
            assert not frames or state["frames"] == ref_fr


def test_streaming_transcriber_beam_lm_equals_offline(lms, golden, monkeypatch):
    """StreamingTranscriber(search="beam") with an LM-carrying searcher: finish() and nbest() are the bits of the offline fused search
    over encoder_proj of the stream's encoder output; no library route is taken."""
    streaming = importlib.import_module("ts-asr_amd.streaming")
    monkeypatch.setattr(ops, "STRICT_HIP", True)
    ops.LIB_FALLBACKS.clear()
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal")
    try:
        s = h["beam_searcher"]
        s.beam_size, s.nbest = 4, 3
        s.lm, s.lm_weight = lms("l2b1e72"), 0.3
        feats = T(golden["c1_features"]["norm"]).to(DEV)
        spk = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)
        with blank_shift(s.classifier_network[0], float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
            st = streaming.StreamingTranscriber(brain, search="beam")
            st.start(feats.shape[0], max_frames=(feats.shape[1] + 3) // 4, speaker_embs=spk, keep_encoder_out=True)
            F = feats.shape[1]
            for f0 in range(0, F, 32):
                st.push(feats[:, f0:f0 + 32], last=f0 + 32 >= F)
            hyps = st.finish()
            nb, sc = st.nbest()
            enc = brain.modules.encoder_proj(st.encoder_out())
            assert s._device_beam_ok(enc)
            off_best, _, off_nb, off_sc = s(enc)
            s.lm_weight = 0.0
            assert s(enc)[2] != off_nb
        assert hyps == off_best and nb == off_nb and bits(sc) == bits(off_sc)
        assert ops.LIB_FALLBACKS == {}
    finally:
        nnet.set_compute_dtype(torch.bfloat16)


def test_lm_overflow_status_and_host_redecode(brains, lms, golden, monkeypatch):
    """A small cap with an LM: status 1 for the utterances that need more hypotheses in a frame; the searcher decodes those again on
    the host loop, with the LM: the result equals the plain host loop's."""
    brain, h = brains("fp32")
    m = brain.modules
    enc = second_enc(golden, 6, 12)
    enc[3:] = 0.0                      # blank wins every frame there: A never holds more than the beam
    enc = enc.to(DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, lms("l2b1e72"), 0.3, nbest=2)
        full = s._device_beam_call(enc, ops.beam_search)
        assert full[2].tolist() == [0] * 6
        for cap in range(4, 64):                         # the smallest cap that stops some utterances but not all
            s.cap = cap
            nb, sc, status = s._device_beam_call(enc, ops.beam_search)
            bad = [b for b in range(6) if status[b] != 0]
            if 0 < len(bad) < 6:
                break
        assert 0 < len(bad) < 6, "no cap separates the utterances"
        assert all(int(status[b]) == 1 for b in bad), status
        assert all(nb[b] == full[0][b] and sc[b] == full[1][b] for b in range(6) if b not in bad)
        before = dec.BEAM_HOST_REDECODES["utterances"]
        with pytest.warns(RuntimeWarning) if before == 0 else contextlib.nullcontext():
            _, _, nb_d, sc_d = s(enc)
        assert dec.BEAM_HOST_REDECODES["utterances"] == before + len(bad)
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        _, _, nb_h, sc_h = s(enc)
        _, _, nb_plain, _ = searcher(m, 4, nbest=2)(enc)
        monkeypatch.delenv("TSASR_BEAM_KERNEL")
        for b in bad:
            assert nb_d[b] == nb_h[b] and sc_d[b] == sc_h[b]
        assert any(nb_h[b] != nb_plain[b] for b in bad)              # the re-decode used the LM


def test_reference_default_lm_width(brains, golden, monkeypatch):
    """The reference-default LM (2 layers, Hl = 1024, E = 128, D = 512) at B = 2, T = 8, beam 4: the K = 1024 products, the LDS sizing
    and the workspace size function. Device against host loop by the tolerance rule; the bytes behind the workspace stay as they were."""
    brain, h = brains("fp32")
    m = brain.modules
    torch.manual_seed(17)
    lm = nnet.RNNLM(V, return_hidden=True).to(DEV).eval()
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:2, :8].to(DEV)
    need = ops.beam_workspace_bytes(2, 8, 128, 160, V, 4, dec.BEAM_CAP, 2, 1024)
    assert need == capi.lib().tsasr_beam_search_workspace_bytes(2, 8, 128, 160, V, 4, dec.BEAM_CAP, 2, 1024, 0, 0, 0)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, lm, 0.3)
        assert s._device_beam_ok(enc)
        nb, sc, status = s._device_beam_call(enc, ops.beam_search, ws[:need])
        assert status.tolist() == [0, 0]
        assert bool((ws[need:] == 0xA5).all())
        monkeypatch.setenv("TSASR_BEAM_KERNEL", "0")
        _, _, nb_h, sc_h = s(enc)
    print("utterances exact per rank", tolerance_ranks(nb, sc, nb_h, sc_h))


def test_launcher_refuses_bad_lm_arguments(brains, lms, golden):
    """A workspace that is too small, 5 LSTM layers, a hidden size that is no multiple of 4 and an LDS need past 152 KB each come back
    as the launcher's error; nothing is launched (the status words keep their fill)."""
    brain, h = brains("fp32")
    m = brain.modules
    enc = T(golden["c1_chain_cat"]["enc_proj"])[:2, :8].to(DEV).contiguous()
    B, Tn, J, H, E = 2, 8, 160, 128, 28
    with blank_shift(m.transducer_head, float(golden["c1_beam_lm"]["blank_bias"])), torch.no_grad():
        s = searcher(m, 4, lms("l2b1e72"), 0.3)
        table, mats, b_ih, b_hh, b_proj, b_head, wdt = s._device_greedy_args(enc)

        def call(lm_args, cap=dec.BEAM_CAP, ws_bytes=None):
            desc, weight, layers, hidden = ops._beam_lm_desc(lm_args, V, wdt)
            need = ops.beam_workspace_bytes(B, Tn, H, J, V, 4, cap, min(layers, 4), hidden)
            ws = torch.empty(need if ws_bytes is None else need + ws_bytes, dtype=torch.uint8, device=DEV)
            hyps = torch.zeros(B, 3, 32, dtype=torch.int32, device=DEV)
            lens = torch.zeros(B, 3, dtype=torch.int32, device=DEV)
            scores = torch.zeros(B, 3, dtype=torch.float64, device=DEV)
            status = torch.full((B,), 77, dtype=torch.int32, device=DEV)
            rc = ops._beam_launch(enc, ops._beam_ptrs(table, mats, b_ih, b_hh, b_proj, b_head, ws), None,
                                  (capi.ptr(hyps), capi.ptr(lens), capi.ptr(scores), capi.ptr(status)), B, Tn, Tn, J, H, E, V, 0, 4, 3, cap, 32,
                                  2.3, 2.3, 0.01, wdt, None, desc, weight, None, False)
            torch.cuda.synchronize()
            return rc, status.tolist(), capi.lib().tsasr_last_error().decode()

        good = s._device_lm_args(enc)
        rc, status, _ = call(good)
        assert rc == 0 and status == [0, 0]
        rc, status, msg = call(good, ws_bytes=-16)
        assert rc != 0 and status == [77, 77] and "workspace" in msg
        deep = searcher(m, 4, nnet.RNNLM(V, embedding_dim=16, rnn_layers=5, rnn_neurons=32, dnn_blocks=0, dnn_neurons=32).to(DEV).eval(), 0.3)
        rc, status, msg = call(deep._device_lm_args(enc))
        assert rc != 0 and status == [77, 77] and "bad LM shape" in msg
        odd = searcher(m, 4, nnet.RNNLM(V, embedding_dim=16, rnn_layers=1, rnn_neurons=30, dnn_blocks=0, dnn_neurons=30).to(DEV).eval(), 0.3)
        rc, status, msg = call(odd._device_lm_args(enc))
        assert rc != 0 and status == [77, 77] and "bad LM shape" in msg
        rc, status, msg = call(good, cap=4000)                               # 4000 x 40 B of hypothesis arrays: past the LDS bound
        assert rc != 0 and status == [77, 77] and "LDS" in msg


def test_recipe_test_stage_with_lm_takes_device_route(tmp_path, monkeypatch):
    """A small fp32 recipe run with --lm_ckpt / --lm_weight: the TEST stage's searcher carries the loaded LM, goes through the fused
    device search (no library route) and writes its WER file."""
    main = importlib.import_module("train_tsasr").main
    torch.manual_seed(5)
    lm = nnet.RNNLM(V, embedding_dim=24, rnn_layers=2, rnn_neurons=40, dnn_blocks=1, dnn_neurons=36)
    ckpt, wer = tmp_path / "lm.pt", tmp_path / "wer.txt"
    torch.save(lm.state_dict(), str(ckpt))
    argv = [os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml"), "--device", "cuda:0", "--synthetic", "2", "--number_of_epochs",
            "1", "--syn_batch", "4", "--syn_seconds", "2.0", "--syn_enroll_seconds", "1.0", "--syn_tokens", "12", "--hip_graph", "False",
            "--lr", "0.002", "--warmup_steps", "5", "--dropout", "0.0", "--beam_size", "3", "--d_model", "144", "--nhead", "4",
            "--encoder_num_layers", "2", "--speaker_num_layers", "2", "--d_ffn", "576", "--joint_dim", "160", "--decoder_neurons", "128",
            "--compute_dtype", "fp32", "--lm_ckpt", str(ckpt), "--lm_weight", "0.4", "--wer_file", str(wer)]
    taken = []
    orig = ops.beam_search

    def spy(*a, **kw):
        taken.append(kw.get("lm"))
        return orig(*a, **kw)
    monkeypatch.setattr(ops, "beam_search", spy)
    ops.LIB_FALLBACKS.clear()
    try:
        brain, result = main(argv)
        assert taken and all(t is not None and t["weight"] == 0.4 for t in taken), "the TEST stage did not take the fused device search"
        assert ops.LIB_FALLBACKS == {}, ops.LIB_FALLBACKS
        s = brain.hparams.beam_searcher
        assert isinstance(s.lm, nnet.RNNLM) and s.lm.rnn.rnn.num_layers == 2 and s.lm.rnn.rnn.hidden_size == 40 and not s.lm.training
        assert all(torch.equal(v.cpu(), lm.state_dict()[k]) for k, v in s.lm.state_dict().items())
        assert wer.exists() and "%WER" in wer.read_text()
    finally:
        nnet.set_compute_dtype(torch.bfloat16)
