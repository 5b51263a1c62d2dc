"""Causal features on the MI355X (csrc/features_stream.hip, nnet.CausalFeatures, StreamingTranscriber.push_audio, hparams
``causal_features``): raw frames against the offline kernel bit for bit, the running normalisation against the float64 reference
(tests/helpers/stream_feats_ref.py) on the kernel's own raw dB, chunk invariance and ragged streams bit for bit, and the stream and the
recipe end to end."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
from oracle.golden_recipe import golden_inputs  # noqa: E402
from tests.helpers import stream_feats_ref as SR  # noqa: E402
from tests.helpers.stream_feats_audio import GPU_CASES, noise_audio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_REL, TOL_ABS = 2.0 ** -22, 1e-9      # one fp32 rounding + slack for the order of the fp64 operations; set by the issue


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture(scope="module")
def mods():
    return (importlib.import_module("ts-asr_amd.ops"), importlib.import_module("ts-asr_amd.nnet"),
            importlib.import_module("ts-asr_amd.streaming"))


@pytest.fixture(scope="module")
def fbank(mods):
    return mods[1].Fbank(sample_rate=16000, n_fft=512, n_mels=80, win_length=32).to(DEV)


def _raw(ops, fbank, wav):
    """raw dB frames of whole signals through the new entry: [B, 1 + L//160, 80] fp32 on the device."""
    return ops.fbank_frames(torch.nn.functional.pad(wav, (256, 256)), fbank.window, fbank.fbank_matrix, 160, fbank.amin)


def _check_close(y, ref, what):
    y, ref = y.detach().float().cpu().numpy().astype(np.float64), ref.astype(np.float64)
    err = np.abs(y - ref) - (TOL_REL * np.abs(ref) + TOL_ABS)
    print(f"{what}: max |y - ref| = {np.abs(y - ref).max():.3e}, worst excess over the bound = {err.max():.3e}")
    assert np.isfinite(y).all() and err.max() <= 0.0, (what, float(err.max()))


# ---------------------------------------------------------------------------------------------- 1. raw frames
@pytest.mark.parametrize("L", [16000 + 77, 159])
def test_raw_frames_equal_offline_kernel_bits(mods, fbank, L):
    ops = mods[0]
    wav = T(noise_audio(2, L, 48)).to(DEV)
    off = ops.fbank(wav, fbank.window, fbank.fbank_matrix, 512, 160, 512, float("inf"), fbank.amin)
    got = _raw(ops, fbank, wav)
    assert got.shape == off.shape == (2, 1 + L // 160, 80) and got.dtype == torch.float32
    assert torch.equal(got, off)
    # a slice of the padded signal gives the frames that start inside it
    seg = torch.nn.functional.pad(wav, (256, 256))[:, 320:320 + 512 + 160 * min(3, L // 160 - 2)] if L > 1000 else None
    if seg is not None:
        assert torch.equal(ops.fbank_frames(seg, fbank.window, fbank.fbank_matrix, 160, fbank.amin), off[:, 2:2 + seg.shape[1] // 160 - 2])


def test_raw_frames_of_silence_are_minus_100(mods, fbank):
    got = _raw(mods[0], fbank, torch.zeros(2, 1000, device=DEV))
    assert got.shape == (2, 7, 80) and bool((got == -100.0).all())


def test_offline_fbank_unchanged_by_the_origin_parameter(mods, fbank):
    """tsasr_fbank_fwd with its floor: the floor of the raw frames at the utterance maximum, as before (its goldens are in test_blocks_gpu)."""
    ops = mods[0]
    wav = T(noise_audio(2, 16077, 48)).to(DEV)
    raw = _raw(ops, fbank, wav)
    off = ops.fbank(wav, fbank.window, fbank.fbank_matrix, 512, 160, 512, 80.0, fbank.amin)
    assert torch.equal(off, torch.maximum(raw, raw.amax(dim=(1, 2), keepdim=True) - 80.0))


# ---------------------------------------------------------------------------------------------- 2. running_norm vs float64
@pytest.mark.parametrize("case", range(len(GPU_CASES)))
def test_running_norm_vs_float64_reference(mods, fbank, case):
    """Both waves (80 bins); F = 101 (not a multiple of 4, under one tile), F = 4 and F = 1, F = 201 (two tiles); the whole row valid."""
    ops = mods[0]
    B, L, seed = GPU_CASES[case]
    db = _raw(ops, fbank, T(noise_audio(B, L, seed)).to(DEV))
    F = db.shape[1]
    state = ops.running_norm_state(B, 80, DEV)
    nv = torch.full((B,), F, dtype=torch.int32, device=DEV)
    y = ops.running_norm(db, state, nv, 80.0, 1e-10, torch.float32)
    ref, r = SR.causal_features_ref(db.cpu().numpy())
    assert r.min_cond >= 1e-3, r.min_cond          # (inf when no frame has two predecessors)
    _check_close(y, ref, f"running_norm B={B} F={F}")
    y16 = ops.running_norm(db, ops.running_norm_state(B, 80, DEV), nv, 80.0, 1e-10, torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and torch.equal(y16, y.to(torch.bfloat16))
    s = state.cpu().numpy()
    assert np.allclose(s[:, :80], r.s1, rtol=1e-14, atol=0) and np.allclose(s[:, 80:160], r.s2, rtol=1e-14, atol=0) and np.array_equal(s[:, 160], r.n)
    tail = state[:, 161:].contiguous().view(torch.float32).cpu().numpy()
    assert np.array_equal(tail[:, 0], r.rmax)


def test_running_norm_ragged_pushes_vs_float64_reference(mods, fbank):
    """Three pushes (F = 37, 1, 63) with streams that end inside a push, one that never starts (n_valid = 0 from the first push) and
    n_valid = 0 after an end: outputs against the reference, the state of an ended stream bit-unchanged."""
    ops = mods[0]
    B, L, seed = GPU_CASES[3]
    db = _raw(ops, fbank, T(noise_audio(B, L, seed)).to(DEV))[:, :101].contiguous()
    total = [101, 50, 0, 37]
    state = ops.running_norm_state(B, 80, DEV)
    ref = SR.RunningNormRef(B)
    for a, b in ((0, 37), (37, 38), (38, 101)):
        nv = [min(max(t - a, 0), b - a) for t in total]
        before = state.clone()
        y = ops.running_norm(db[:, a:b].contiguous(), state, torch.tensor(nv, dtype=torch.int32, device=DEV), 80.0, 1e-10)
        _check_close(y, ref.push(db[:, a:b].cpu().numpy(), nv), f"frames {a}..{b} n_valid {nv}")
        for s in range(B):
            if nv[s] == 0:
                assert torch.equal(state[s], before[s])
    assert ref.min_cond >= 1e-3, ref.min_cond
    assert bool((state[2] == 0).all())
    assert np.array_equal(state[:, 160].cpu().numpy(), np.array(total, np.float64))


def test_running_norm_refuses_bad_arguments(mods):
    ops = mods[0]
    db = torch.zeros(2, 4, 80, device=DEV)
    nv = torch.full((2,), 4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.running_norm(db, ops.running_norm_state(3, 80, DEV), nv, 80.0, 1e-10)
    with pytest.raises(ValueError):
        ops.running_norm(db.to(torch.bfloat16), ops.running_norm_state(2, 80, DEV), nv, 80.0, 1e-10)
    C = importlib.import_module("ts-asr_amd._capi")
    big = torch.zeros(1, 2, 129, device=DEV)
    with pytest.raises(C.TsasrHipError):
        ops.running_norm(big, ops.running_norm_state(1, 129, DEV), nv[:1].contiguous(), 80.0, 1e-10)


# ---------------------------------------------------------------------------------------------- 3. chunk invariance
def _pushes(cf, wav, sizes, group=4):
    st = cf.init_stream(wav.shape[0], DEV)
    outs, pos, i = [], 0, 0
    L = wav.shape[1]
    while True:
        n = min(sizes[i % len(sizes)], L - pos)
        last = pos + n >= L
        f, nv, st = cf.forward_chunk(wav[:, pos:pos + n], st, last=last, group=group)
        assert f.shape[1] % group == 0 or last
        assert nv.tolist() == [f.shape[1]] * wav.shape[0]
        outs.append(f)
        pos, i = pos + n, i + 1
        if last:
            return torch.cat(outs, 1), st["norm"]


def test_chunk_invariance_bit_for_bit(mods, fbank):
    nn_ = mods[1]
    B, L, seed = GPU_CASES[0]
    wav = T(noise_audio(B, L, seed)).to(DEV)
    cf = nn_.CausalFeatures(fbank)
    whole = cf(wav, torch.ones(B, device=DEV))
    assert whole.shape == (B, 1 + L // 160, 80) and whole.dtype == torch.float32
    ref_state = None
    for sizes in ([L], [160], [641], [100, 1000, 37, 5000, 159, 3, 2500]):
        feats, state = _pushes(cf, wav, sizes)
        assert torch.equal(feats, whole), sizes
        if ref_state is None:
            ref_state = state.clone()
        assert torch.equal(state.view(torch.int64), ref_state.view(torch.int64)), sizes
    feats8, _ = _pushes(cf, wav, [1234], group=32)
    assert torch.equal(feats8, whole)


# ---------------------------------------------------------------------------------------------- 4. ragged streams
def test_ragged_streams_equal_each_stream_alone(mods, fbank):
    nn_ = mods[1]
    B, L, seed = 3, 16000, 83
    wav = T(noise_audio(B, L, seed)).to(DEV)
    ends = [16000, 9000 + 33, 2077]                   # stream 1 ends in push 3, stream 2 in push 1 (pushes of 4000 samples)
    cf = nn_.CausalFeatures(fbank)
    st = cf.init_stream(B, DEV)
    outs, nvs, frozen = [], [], {}
    for p in range(4):
        lens = [min(max(e - 4000 * p, 0), 4000) for e in ends]
        f, nv, st = cf.forward_chunk(wav[:, 4000 * p:4000 * (p + 1)], st, wav_lens=lens, last=p == 3)
        outs.append(f)
        nvs.append(nv)
        for b in frozen:
            assert torch.equal(st["norm"][b], frozen[b]), (p, b)
        for b, e in enumerate(ends):
            if e < 4000 * (p + 1) and b not in frozen and int(st["norm"][b, 160]) == 1 + e // 160:
                frozen[b] = st["norm"][b].clone()
    assert sorted(frozen) == [1, 2]
    feats, n_valid = torch.cat(outs, 1), torch.stack(nvs).sum(0)
    assert feats.shape[1] == 101 and n_valid.tolist() == [1 + e // 160 for e in ends]
    for b, e in enumerate(ends):
        alone, state = _pushes(cf, wav[b:b + 1, :e].contiguous(), [4000])
        assert alone.shape[1] == 1 + e // 160
        assert torch.equal(feats[b, :alone.shape[1]], alone[0]), b
        assert torch.equal(st["norm"][b].view(torch.int64), state[0].view(torch.int64)), b
    assert bool(torch.isfinite(feats).all())


# ---------------------------------------------------------------------------------------------- 5. edge cases
def test_silence_gives_zeros(mods, fbank):
    cf = mods[1].CausalFeatures(fbank)
    y = cf(torch.zeros(2, 4000, device=DEV), torch.ones(2, device=DEV))
    assert y.shape == (2, 26, 80) and bool((y == 0).all())
    f, _ = _pushes(cf, torch.zeros(2, 4000, device=DEV), [700])
    assert bool((f == 0).all())


def test_prior_is_honoured(mods, fbank):
    ops, nn_ = mods[0], mods[1]
    B, L, seed = GPU_CASES[1]
    wav = T(noise_audio(B, L, seed)).to(DEV)
    mu, sd, n0 = np.linspace(-3.0, 3.0, 80), np.linspace(4.0, 6.0, 80), 10.0
    cf = nn_.CausalFeatures(fbank, prior=(mu, sd, n0)).to(DEV)
    y = cf(wav, torch.ones(B, device=DEV))
    db = _raw(ops, fbank, wav)
    ref, r = SR.causal_features_ref(db.cpu().numpy(), prior=(mu, sd, n0))
    assert r.min_cond >= 1e-3, r.min_cond
    _check_close(y, ref, "prior n0 = 10")
    assert not torch.equal(y, nn_.CausalFeatures(fbank)(wav, torch.ones(B, device=DEV)))
    assert torch.equal(nn_.CausalFeatures(fbank, prior=(mu, sd, 0.0)).to(DEV)(wav, torch.ones(B, device=DEV)),
                       nn_.CausalFeatures(fbank)(wav, torch.ones(B, device=DEV)))
    f, _ = _pushes(cf, wav, [77])
    assert torch.equal(f, y)


def test_rejected_push_leaves_the_state_untouched(mods, fbank):
    cf = mods[1].CausalFeatures(fbank)
    wav = T(noise_audio(2, 3000, 7)).to(DEV)
    st = cf.init_stream(2, DEV)
    cf.forward_chunk(wav[:, :1000], st, wav_lens=[1000, 900])          # stream 1 ends at sample 900

    def snap():
        return (st["buf"].clone(), st["norm"].clone(), st["samples"], st["emitted"], list(st["valid"]), st["closed"])

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)) and a[2:] == b[2:]

    before = snap()
    with pytest.raises(ValueError):
        cf.forward_chunk(wav[:, 1000:2000], st, wav_lens=[1000, 5])    # samples after the end
    with pytest.raises(ValueError):
        cf.forward_chunk(wav[:1, 1000:2000], st)                       # wrong B
    with pytest.raises(ValueError):
        cf.forward_chunk(wav[:, 1000:2000], st, wav_lens=[1001, 0])    # more valid samples than the push holds
    assert same(before, snap())
    f, nv, _ = cf.forward_chunk(wav[:, 1000:2000], st, wav_lens=[1000, 0], last=True)
    assert f.shape[1] == 13 - 4 and nv.tolist() == [9, 2]              # frames 4..12; stream 1 has 1 + 900//160 = 6 frames


# ---------------------------------------------------------------------------------------------- 6. the stream end to end
@pytest.mark.parametrize("search", ["greedy", "beam"])
@pytest.mark.parametrize("chunk_size", [0, 8])
def test_push_audio_equals_push_of_the_same_frames(mods, golden, chunk_size, search):
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "bf16", causal_encoder=True, frontend_padding="causal", attention_chunk_size=chunk_size)
    try:
        inp = golden_inputs()
        wav = T(inp["mixed_sig"]).to(DEV)
        B, L = wav.shape
        Tn = 1 + L // 160
        frames = [Tn, 180, 160, 140]
        ends = [L] + [(t - 1) * 160 + 50 for t in frames[1:]]
        wav = wav * (torch.arange(L, device=DEV)[None, :] < torch.tensor(ends, device=DEV)[:, None])
        spk, spk_len = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV), T(inp["enroll_lens"]).to(DEV)
        group = 4 * max(chunk_size, 1)
        head = h["beam_searcher"].classifier_network[0]
        # (beam search on the untrained golden weights: blank is rare among the best symbols and a frame then needs more hypotheses than
        # the searcher's cap; the beam goldens raise the head's blank bias for the same reason - here by 2 more, the features being others)
        shift = float(golden["c1_beam"]["blank_bias"]) + 2.0 if search == "beam" else 0.0
        with torch.no_grad():
            head.w.bias[0] += shift
            h["beam_searcher"].beam_size = 4
            a = streaming.StreamingTranscriber(brain, search=search)
            a.start(B, max_frames=(Tn + 3) // 4, speaker_embs=spk, speaker_embs_length=spk_len, keep_encoder_out=True, timestamps=True, audio=True)
            pushed, inner = [], a.push

            def record(feats, mel_lens=None, enc_lens=None, last=False):
                pushed.append((feats.shape[1], mel_lens.tolist()))
                return inner(feats, mel_lens=mel_lens, enc_lens=enc_lens, last=last)

            a.push = record
            pos, i, sizes = 0, 0, [3000, 100, 7777, 159, 5000, 1, 9000]
            while pos < L:
                n = min(sizes[i % len(sizes)], L - pos)
                a.push_audio(wav[:, pos:pos + n], wav_lens=[min(max(e - pos, 0), n) for e in ends], last=pos + n >= L)
                pos, i = pos + n, i + 1
            assert [f for f, _ in pushed if f][:-1] == [f - f % group for f, _ in pushed if f][:-1] and sum(f for f, _ in pushed) == Tn
            assert [sum(ml[b] for _, ml in pushed) for b in range(B)] == frames
            # the same frames from the offline call, pushed in the same multiples of the group
            cf = nn_.CausalFeatures(brain.modules.feature_extractor)
            feats = cf(wav, torch.tensor([t / Tn for t in frames], device=DEV))
            b = streaming.StreamingTranscriber(brain, search=search)
            b.start(B, max_frames=(Tn + 3) // 4, speaker_embs=spk, speaker_embs_length=spk_len, keep_encoder_out=True, timestamps=True)
            f0 = 0
            for f, ml in pushed:
                if f:
                    b.push(feats[:, f0:f0 + f], mel_lens=torch.tensor(ml, device=DEV), last=f0 + f >= Tn)
                    f0 += f
            assert torch.equal(a.encoder_out(), b.encoder_out())
            assert a.frames() == b.frames()
            ha, hb = a.finish(), b.finish()
        print(f"push_audio chunk_size={chunk_size} {search}: hypothesis lengths {[len(x) for x in ha]}")
        assert ha == hb and any(len(x) for x in ha)
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_push_audio_needs_audio_mode_and_short_pushes_return_nothing(mods, golden):
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "bf16", causal_encoder=True, frontend_padding="causal")
    try:
        spk = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)
        with torch.no_grad():
            st = streaming.StreamingTranscriber(brain)
            st.start(4, 50, speaker_embs=spk)
            with pytest.raises(RuntimeError):
                st.push_audio(torch.zeros(4, 100, device=DEV))
            with pytest.raises(ValueError):
                st.start(4, 50, speaker_embs=spk, feature_prior=(np.zeros(80), np.ones(80), 1.0))
            st.start(4, 50, speaker_embs=spk, audio=True)
            assert st.push_audio(torch.zeros(4, 100, device=DEV)) == [[], [], [], []]      # no frame group complete yet
            assert st.encoder_frames == 0
            st.finish()
            # a push that push() itself refuses (past max_frames) leaves the buffered samples and the running statistics as they were
            st.start(4, 2, speaker_embs=spk, audio=True)
            wav = T(noise_audio(4, 4000, 9)).to(DEV)
            st.push_audio(wav[:, :1000])                                                   # 4 frames = 1 encoder frame
            fs = st.feat_state
            before = (fs["buf"].clone(), fs["norm"].clone(), fs["samples"], fs["emitted"])
            with pytest.raises(ValueError):
                st.push_audio(wav[:, 1000:])                                               # 20 more frames: past 2 encoder frames
            fs = st.feat_state
            assert torch.equal(fs["buf"], before[0]) and torch.equal(fs["norm"].view(torch.int64), before[1].view(torch.int64))
            assert (fs["samples"], fs["emitted"]) == before[2:] and st.encoder_frames == 1
            assert len(st.push_audio(wav[:, 1000:1640])) == 4 and st.encoder_frames == 2   # 4 more frames fit
            st.finish()
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


# ---------------------------------------------------------------------------------------------- 7. the recipe
def _batch(inp):
    bm = importlib.import_module("ts-asr_amd.batch")
    return bm.PaddedBatch({
        "id": ["a", "b", "c", "d"],
        "mixed_sig": bm.PaddedData(T(inp["mixed_sig"]), T(inp["mixed_lens"])),
        "enroll_sig": bm.PaddedData(T(inp["enroll_sig"]), T(inp["enroll_lens"])),
        "tokens_bos": bm.PaddedData(T(inp["tokens_bos"]), T(inp["tokens_bos_lens"])),
        "tokens": bm.PaddedData(T(inp["tokens"]), T(inp["tokens_lens"])),
    })


def test_recipe_causal_features_forward_equals_by_hand(mods):
    """(VALID stage, as tests/test_model_gpu.py evaluates the golden weights: the TEST stage's beam search over untrained weights, where
    blank is rare among the best symbols, does not end in useful time.)"""
    ops, nn_, _ = mods
    core = importlib.import_module("ts-asr_amd.core")
    rnnt = importlib.import_module("ts-asr_amd.rnnt")
    try:
        brain, h = entry._config1_brain(DEV, "fp32", causal_features=True)
        brain._setup_dtype()
        brain.modules.eval()
        batch = _batch(golden_inputs()).to(DEV)
        with torch.no_grad():
            logits, _ = brain.compute_forward(batch, core.Stage.VALID)
            m = brain.modules
            mixed, mixed_lens = batch.mixed_sig
            spk, enroll_lens = brain._speaker_embedding(batch, 0)
            feats = nn_.CausalFeatures(m.feature_extractor)(mixed, mixed_lens)
            enc = m.encoder_proj(m.encoder(m.frontend(feats), mixed_lens, spk, enroll_lens))
            dec = brain._predictor(*batch.tokens_bos)
            tlen = nn_.abs_lengths_round(mixed_lens, enc.shape[1])
            ulen = nn_.abs_lengths_round(batch.tokens.lengths, batch.tokens.data.shape[1])
            hand = rnnt.fused_joint_logits(enc, dec, m.transducer_head.w.weight, m.transducer_head.w.bias, m.joiner.nonlinearity.negative_slope, tlen, ulen)
            assert torch.equal(logits, hand)
            plain, _ = entry._config1_brain(DEV, "fp32")
            plain._setup_dtype()
            plain.modules.eval()
            other, _ = plain.compute_forward(batch, core.Stage.VALID)
            assert other.shape == logits.shape and not torch.equal(other, logits)      # the sentence-level features are other features
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_recipe_causal_features_trains_and_hip_graph_replay_equals_eager(mods):
    """TRAIN-stage steps with causal_features: finite, decreasing loss; the captured step (the feature stage is inside it: the batch's
    waveform is the graph's static input) reproduces the eager losses."""
    losses = {}
    for mode in ("eager", "graph"):
        brain, h = entry._config1_brain(DEV, "bf16", causal_features=True)
        brain.modules.train()
        if mode == "graph":
            brain.enable_hip_graph(warmup_steps=2)
        batch = _batch(golden_inputs()).to(DEV)
        losses[mode] = [float(brain.fit_batch(batch)) for _ in range(6)]
        if mode == "graph":
            assert brain._graph is not None
    assert np.isfinite(losses["eager"]).all() and losses["eager"][0] > losses["eager"][-1]
    print("eager", losses["eager"], "graph", losses["graph"])
    assert losses["graph"] == losses["eager"], losses
