"""Slot sessions fed audio (StreamingTranscriber.admit(..., audio=True) / push_audio in slot mode; csrc/features.hip fbank_slots_kernel,
csrc/features_stream.hip audio_ring_append_kernel) on the MI355X.

Four sessions - the golden utterances (31840 samples, relative lengths 1, 0.9, 0.8, 0.7: a session's audio is its row cut at its length)
with their golden speaker embeddings - enter and leave three slots: s0 enters slot 0 at tick 0, s1 enters slot 2 at tick 1 (with a
feature prior) and is paused at tick 3, s3 enters slot 1 at tick 4, and when s0's audio has ended it is released and s2 is admitted
into slot 0 in the same tick. Every session has its own packet sizes (0, 1, 100 - a first packet that holds no frame yet -, 777, 1600,
2000); max_audio_samples = 2000, so every ring wraps many times; after the first admission has allocated the rings they are filled with
NaN (as the K/V caches are).

1. features_out(slot) of every session equals nnet.CausalFeatures(fbank, prior).forward over the session alone, bit for bit.
2. Replaying the logged audio_steps through push(feats) with each session's solo features gives the same hypotheses, encoder_out bytes,
   emission frames and n-best lists / scores (greedy and beam, fp32 and bf16).
3. A slot that is not active in a call keeps every piece of its state; a refused call leaves every slot as it was."""
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
from tests.test_stream_slots_gpu import T, _golden_beam_searcher, same, speaker, state_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, MAXF, MAX_AUDIO = 3, 64, 2000
SESS = {"s0": dict(row=0, slot=0, sizes=[100, 2000, 0, 777, 2000, 1, 1600, 2000]),
        "s1": dict(row=1, slot=2, sizes=[1600, 2000, 777, 2000, 0, 2000, 1, 2000], prior=True),
        "s2": dict(row=2, slot=0, sizes=[777, 2000, 2000, 1, 1600, 2000, 0, 2000]),
        "s3": dict(row=3, slot=1, sizes=[2000, 1, 2000, 1600, 2000, 0, 777, 2000])}
ADMIT_AT = {0: "s0", 1: "s1", 4: "s3"}          # s2 follows s0 into slot 0
PAUSE_AT = {3: 2}                               # tick 3: slot 2 (s1) is left out of the call


@pytest.fixture(scope="module")
def mods():
    return (importlib.import_module("ts-asr_amd.ops"), importlib.import_module("ts-asr_amd.nnet"),
            importlib.import_module("ts-asr_amd.streaming"))


@pytest.fixture(scope="module")
def audio():
    """{session: its waveform [L] on the device}, and the feature prior of s1."""
    inp = golden_inputs()
    wav = T(inp["mixed_sig"]).to(DEV)
    lens = [int(round(float(r) * wav.shape[1])) for r in inp["mixed_lens"]]
    assert wav.shape[1] == 31840 and lens == [31840, 28656, 25472, 22288]
    g = torch.Generator().manual_seed(3)
    prior = (torch.randn(80, generator=g) * 2 - 60, torch.rand(80, generator=g) * 5 + 5, 25.0)
    return {n: wav[s["row"], :lens[s["row"]]].contiguous() for n, s in SESS.items()}, prior


def build_ticks(lengths):
    """The schedule, on the host: per tick the sessions released and admitted, and per slot whether it is active, how many samples it gets
    and whether its audio ends with the call."""
    owner, pos, turn, over, released, ticks, t = [None] * NS, {n: 0 for n in SESS}, {n: 0 for n in SESS}, set(), set(), [], 0
    while len(released) < len(SESS):
        tick = dict(release=[], admit=[], active=[False] * NS, lens=[0] * NS, end=[False] * NS, paused=t in PAUSE_AT)
        for b, name in enumerate(owner):
            if name in over:
                tick["release"].append(name)
                released.add(name)
                owner[b] = None
                if name == "s0":
                    tick["admit"].append("s2")
        if t in ADMIT_AT:
            tick["admit"].append(ADMIT_AT[t])
        for name in tick["admit"]:
            assert owner[SESS[name]["slot"]] is None
            owner[SESS[name]["slot"]] = name
        for b, name in enumerate(owner):
            if name is None or PAUSE_AT.get(t) == b:
                continue
            n = min(SESS[name]["sizes"][turn[name] % 8], lengths[name] - pos[name])
            tick["active"][b], tick["lens"][b] = True, n
            tick.setdefault("src", {})[b] = (name, pos[name], n)
            pos[name], turn[name] = pos[name] + n, turn[name] + 1
            if pos[name] == lengths[name]:
                tick["end"][b] = True
                over.add(name)
        ticks.append(tick)
        t += 1
        assert t < 200
    return ticks


def audio_state(st, b):
    fs = st.feat_slots
    return [fs["ring"][b].clone(), fs["norm"][b].clone(), torch.tensor([st.a_have[b], st.a_emit[b], int(st.a_end[b]), int(st.audio_slot[b])])]


def all_state(st):
    out = []
    for b in range(NS):
        out += state_of(st, b) + (audio_state(st, b) if st.feat_slots is not None else [])
    return out


def collect(st, b, search, timed):
    r = dict(enc=st.encoder_out(b).clone(), frames=st.frames()[b] if timed else None, n_enc=st.encoder_frames(b))
    r["hyp"] = st.release(b)
    if search == "beam":
        r["nbest"], r["scores"] = (x[b] for x in st.nbest())
        r["nbest_frames"] = st.nbest_frames()[b] if timed else None
    return r


def begin(streaming, brain, search, searcher, **kw):
    st = streaming.StreamingTranscriber(brain, search=search)
    if searcher is not None:
        st.searcher = searcher
    st.start(NS, MAXF, slots=True, keep_encoder_out=True, timestamps=True, **kw)
    for layer in st.enc_state["layers"]:
        layer["k"].fill_(float("nan"))
        layer["v"].fill_(float("nan"))
    return st


def run_audio(streaming, brain, wavs, prior, emb, search="greedy", searcher=None):
    """The schedule through push_audio -> ({session: results + its features}, per tick the steps it ran)."""
    st = begin(streaming, brain, search, searcher, max_audio_samples=MAX_AUDIO, keep_features=True)
    assert st.feat_slots is None and st.audio_steps == []
    with pytest.raises(RuntimeError):
        st.push_audio(torch.zeros(NS, 10, device=DEV))           # no audio session has been admitted yet
    res, steps_of_tick, seen = {}, [], 0
    for n_tick, tick in enumerate(build_ticks({n: w.numel() for n, w in wavs.items()})):
        for name in tick["release"]:
            b = SESS[name]["slot"]
            feats = st.features_out(b).clone()
            res[name] = dict(collect(st, b, search, True), feats=feats)
        for name in tick["admit"]:
            s = SESS[name]
            first = st.feat_slots is None
            st.admit(s["slot"], speaker_embs=emb[s["row"]:s["row"] + 1], audio=True, feature_prior=prior if s.get("prior") else None)
            if first:
                st.feat_slots["ring"].fill_(float("nan"))          # admit() clears no ring; what a session has not sent is never read
            assert st.features_out(s["slot"]).shape == (0, 80) and st.encoder_frames(s["slot"]) == 0
        N = max(tick["lens"])
        wav = torch.full((NS, N), float("nan"), device=DEV)      # samples past a slot's wav_lens are not read either
        for b, (name, p, n) in tick.get("src", {}).items():
            wav[b, :n] = wavs[name][p:p + n]
        idle = [b for b in range(NS) if not tick["active"][b]]
        before = {b: state_of(st, b) + audio_state(st, b) for b in idle} if st.search_state is not None else {}
        hyps_before = [list(h) for h in st.hyps]
        ret = st.push_audio(wav, wav_lens=tick["lens"], active=tick["active"] if tick["paused"] else None, end=tick["end"])
        for b, snap in before.items():
            assert same(snap, state_of(st, b) + audio_state(st, b)), f"tick {n_tick}: state of idle slot {b} moved"
            assert ret[b] == ([] if search == "greedy" else hyps_before[b]) and st.hyps[b] == hyps_before[b], (n_tick, b)
        steps_of_tick.append(st.audio_steps[seen:])
        seen = len(st.audio_steps)
    assert st.occupied == [False] * NS and set(res) == set(SESS)
    assert st.feat_slots["ring"].shape[1] < 8000 < min(w.numel() for w in wavs.values())          # every ring wrapped
    return res, steps_of_tick


def run_replay(streaming, brain, wavs, solo, emb, steps_of_tick, search="greedy", searcher=None):
    """The same admissions, releases and steps through push(feats) with every session's solo features, zeros in the padded rows."""
    st = begin(streaming, brain, search, searcher)
    res, owner, done = {}, [None] * NS, {n: 0 for n in SESS}
    for tick, steps in zip(build_ticks({n: w.numel() for n, w in wavs.items()}), steps_of_tick):
        for name in tick["release"]:
            res[name] = collect(st, SESS[name]["slot"], search, True)
            owner[SESS[name]["slot"]] = None
        for name in tick["admit"]:
            s = SESS[name]
            st.admit(s["slot"], speaker_embs=emb[s["row"]:s["row"] + 1])
            owner[s["slot"]] = name
        for F, on, ml in steps:
            f = torch.zeros(NS, F, 80, device=DEV)
            for b in range(NS):
                if on[b]:
                    name = owner[b]
                    f[b, :ml[b]] = solo[name][done[name]:done[name] + ml[b]]
                    done[name] += ml[b]
            st.push(f, mel_lens=torch.tensor(ml), active=on)
    assert all(done[n] == solo[n].shape[0] for n in SESS)
    return res


def solo_features(nn_, brain, wavs, prior):
    fb = brain.modules.feature_extractor
    return {n: nn_.CausalFeatures(fb, prior if SESS[n].get("prior") else None).to(DEV)(w[None], torch.ones(1, device=DEV))[0] for n, w in wavs.items()}


def brain_of(dtype, chunk):
    kw = dict(attention_chunk_size=chunk) if chunk else {}
    return entry._config1_brain(DEV, dtype, causal_encoder=True, frontend_padding="causal", **kw)


# ------------------------------------------------------------------------------------------------------ 1. the feature bits
@pytest.mark.parametrize("chunk", [0, 8])
def test_slot_audio_features_equal_solo_features_bitwise(mods, golden, audio, chunk):
    ops, nn_, streaming = mods
    wavs, prior = audio
    brain, h = brain_of("fp32", chunk)
    try:
        emb, _ = speaker("cat", golden)
        with torch.no_grad():
            res, steps = run_audio(streaming, brain, wavs, prior, emb)
            solo = solo_features(nn_, brain, wavs, prior)
        g = 4 * max(chunk, 1)
        assert all(F % g == 0 for tick in steps for F, _, _ in tick)
        for name, w in wavs.items():
            got, want = res[name]["feats"], solo[name]
            assert got.shape == want.shape == (1 + w.numel() // 160, 80), (name, got.shape, want.shape)
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), \
                f"chunk {chunk} {name}: {int((got != want).sum())} feature values differ from the session alone"
        print(f"SLOT-AUDIO chunk{chunk}: {sum(len(t) for t in steps)} steps in {len(steps)} ticks, sizes {sorted({F for t in steps for F, _, _ in t})}")
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------ 2. end to end
def end_to_end(mods, golden, audio, dtype, chunk, search):
    ops, nn_, streaming = mods
    wavs, prior = audio
    brain, h = brain_of(dtype, chunk)
    try:
        emb, _ = speaker("cat", golden)
        srch = _golden_beam_searcher(golden)(h) if search == "beam" else None
        with torch.no_grad():
            got, steps = run_audio(streaming, brain, wavs, prior, emb, search, srch)
            solo = solo_features(nn_, brain, wavs, prior)
            want = run_replay(streaming, brain, wavs, solo, emb, steps, search, srch)
        for name in SESS:
            g, w = got[name], want[name]
            assert g["n_enc"] == w["n_enc"] and g["enc"].shape == w["enc"].shape
            assert torch.equal(g["enc"].contiguous().view(torch.uint8), w["enc"].contiguous().view(torch.uint8)), f"{name}: encoder_out bits differ"
            assert g["hyp"] == w["hyp"] and g["frames"] == w["frames"], name
            if search == "beam":
                assert g["nbest"] == w["nbest"] and g["nbest_frames"] == w["nbest_frames"], name
                assert [np.float64(x).tobytes() for x in g["scores"]] == [np.float64(x).tobytes() for x in w["scores"]], name
        print(f"SLOT-AUDIO {dtype}-chunk{chunk}-{search}: tokens per session {[len(got[n]['hyp']) for n in SESS]}")
        assert sum(len(got[n]["hyp"]) for n in SESS) > 0
        return got
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("dtype,chunk", [("fp32", 0), ("bf16", 0), ("bf16", 8)])
def test_slot_audio_greedy_equals_replay_through_push(mods, golden, audio, dtype, chunk):
    end_to_end(mods, golden, audio, dtype, chunk, "greedy")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_slot_audio_beam_equals_replay_through_push(mods, golden, audio, dtype):
    got = end_to_end(mods, golden, audio, dtype, 0, "beam")
    assert all(len(got[n]["nbest"]) > 1 for n in SESS)


def test_slot_audio_strict_hip_stays_silent(mods, golden, audio, monkeypatch):
    ops, nn_, streaming = mods
    monkeypatch.setattr(ops, "STRICT_HIP", True)
    ops.LIB_FALLBACKS.clear()
    wavs, prior = audio
    brain, h = brain_of("bf16", 8)
    try:
        with torch.no_grad():
            run_audio(streaming, brain, wavs, prior, speaker("cat", golden)[0])
        assert ops.LIB_FALLBACKS == {}
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------ 3. state discipline
def test_slot_audio_refusals_leave_every_slot_as_it_was(mods, golden, audio):
    ops, nn_, streaming = mods
    wavs, prior = audio
    brain, h = brain_of("fp32", 0)
    try:
        emb, _ = speaker("cat", golden)
        w = wavs["s0"]
        with torch.no_grad():
            solo = solo_features(nn_, brain, wavs, prior)
            st = streaming.StreamingTranscriber(brain)
            with pytest.raises(ValueError, match="admit"):
                st.start(NS, 12, slots=True, audio=True)
            st.start(NS, 13, slots=True, max_audio_samples=MAX_AUDIO, keep_features=True)
            with pytest.raises(ValueError, match="feature_prior"):
                st.admit(1, speaker_embs=emb[1:2], feature_prior=prior)
            assert st.occupied == [False] * NS
            st.admit(1, speaker_embs=emb[1:2])                                # slot 1: fed features
            with pytest.raises(RuntimeError):
                st.push_audio(torch.zeros(NS, 10, device=DEV))               # no audio session yet
            st.admit(0, speaker_embs=emb[0:1], audio=True)                    # slot 0: fed audio; slot 2 stays free
            f = torch.zeros(NS, 32, 80, device=DEV)
            f[1] = solo["s1"][:32]
            st.push(f)                                                       # default active: the feature-fed session only
            assert (st.encoder_frames(0), st.encoder_frames(1)) == (0, 8)
            pack = lambda p: w[p:p + MAX_AUDIO][None].expand(NS, -1)         # noqa: E731  (row stride 0: no copy is needed)
            for p in range(4):                                               # 8000 samples: 49 frames, 48 pushed = 12 encoder frames
                st.push_audio(pack(p * MAX_AUDIO))
            assert (st.encoder_frames(0), st.encoder_frames(1), st.a_emit[0]) == (12, 8, 48)
            before = all_state(st)
            refused = [
                (dict(wav=pack(8000)), "max_frames"),                                                        # 12 more frames: 12 + 3 > 13 encoder frames
                (dict(wav=torch.zeros(NS, MAX_AUDIO + 1, device=DEV)), "max_audio_samples"),
                (dict(wav=pack(8000), active=[True, False, True]), "free"),
                (dict(wav=pack(8000), active=[True, True, False]), "fed features"),
                (dict(wav=pack(8000), wav_lens=[MAX_AUDIO + 1, 0, 0]), "wav_lens"),
                (dict(wav=pack(8000), wav_lens=[-1, 0, 0]), "wav_lens"),
                (dict(wav=pack(8000), wav_lens=[1, 0]), "wav_lens"),
                (dict(wav=pack(8000), end=[False, True, False]), "end"),
                (dict(wav=w[:100]), "wav must be"),
            ]
            for kw, what in refused:
                with pytest.raises(ValueError, match=what):
                    st.push_audio(**kw)
                assert same(before, all_state(st)), f"a push_audio refused for {what!r} moved state"
            with pytest.raises(ValueError, match="fed audio"):
                st.push(f, active=[True, True, False])                       # push() does not take an audio session
            assert same(before, all_state(st)) and st.encoder_frames(1) == 8
            st.push_audio(pack(8000), wav_lens=[100, 0, 0], end=[True, False, False])     # 8100 samples: 51 frames, 3 remain: the 13th encoder frame
            assert st.a_end[0] and st.a_emit[0] == 51 and st.audio_steps[-1] == (4, [True, False, False], [3, 0, 0])
            before = all_state(st)
            with pytest.raises(ValueError, match="ended"):
                st.push_audio(pack(8100), active=[True, False, False])
            assert same(before, all_state(st))
            assert st.push_audio(pack(8100)) == [[], [], []] and same(before, all_state(st))      # default active: nobody
            got = st.features_out(0)
            want = nn_.CausalFeatures(brain.modules.feature_extractor).to(DEV)(w[None, :8100], torch.ones(1, device=DEV))[0]
            assert got.shape == (51, 80) and torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))
            st.release(0)
            st.finish()
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_steps_behind_a_stopped_one_wait_for_the_next_call(mods, golden, audio):
    """push() raises RuntimeError for a stopped beam stream after the step's state is stored. Here the slot push is made to raise
    after the first of a call's two steps: that step counts, the second does not run, its samples stay in the ring, and the next call -
    carrying no samples at all - drains it; the sessions' features are still those of each session alone."""
    ops, nn_, streaming = mods
    wavs, prior = audio
    brain, h = brain_of("fp32", 0)
    try:
        emb, _ = speaker("cat", golden)
        w0, w1 = wavs["s0"][:6000], wavs["s3"][:3000]
        with torch.no_grad():
            st = streaming.StreamingTranscriber(brain)
            st.start(2, MAXF, slots=True, max_audio_samples=MAX_AUDIO, keep_features=True)
            st.admit(0, speaker_embs=emb[0:1], audio=True)
            st.admit(1, speaker_embs=emb[3:4], audio=True)
            real, calls = st._push_slots, []

            def stopping(*a, **kw):
                out = real(*a, **kw)
                calls.append(a[0].shape[1])
                if len(calls) == 1:
                    raise RuntimeError("beam_stream: slot(s) [1] stopped")
                return out

            st._push_slots = stopping
            wav = torch.zeros(2, MAX_AUDIO, device=DEV)
            wav[0], wav[1, :777] = w0[:2000], w1[:777]
            with pytest.raises(RuntimeError, match="stopped"):
                st.push_audio(wav, wav_lens=[2000, 777])                         # 11 and 4 frames: a step of 4 for both, one of 4 for slot 0
            assert st.audio_steps == [(4, [True, True], [4, 4])] and st.a_emit == [4, 4] and st.a_have == [2000, 777]
            assert st.push_audio(torch.zeros(2, 0, device=DEV)) is not None
            assert st.audio_steps[1:] == [(4, [True, False], [4, 0])] and st.a_emit == [8, 4]
            st.push_audio(torch.stack([w0[2000:4000], w1[777:2777]]))
            wav[0], wav[1, :223] = w0[4000:], w1[2777:]
            st.push_audio(wav, wav_lens=[2000, 223], end=[True, True])
            for b, w in ((0, w0), (1, w1)):
                got = st.features_out(b)
                want = nn_.CausalFeatures(brain.modules.feature_extractor).to(DEV)(w[None], torch.ones(1, device=DEV))[0]
                assert got.shape == want.shape and torch.equal(got.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), b
            st.finish()
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_a_feature_fed_and_an_audio_fed_session_share_a_batch(mods, golden, audio):
    """Slot 0 is fed s1's features, slot 1 s0's audio, tick by tick in one batch: each gets the bits it gets with the other slot free."""
    ops, nn_, streaming = mods
    wavs, prior = audio
    brain, h = brain_of("bf16", 0)
    try:
        emb, _ = speaker("cat", golden)
        w = wavs["s0"][:16000]

        def run(with_feats, with_audio, solo):
            st = streaming.StreamingTranscriber(brain)
            st.start(2, MAXF, slots=True, max_audio_samples=MAX_AUDIO, keep_encoder_out=True, timestamps=True)
            if with_feats:
                st.admit(0, speaker_embs=emb[1:2])
            if with_audio:
                st.admit(1, speaker_embs=emb[0:1], audio=True)
            for p in range(8):
                if with_feats:
                    f = torch.zeros(2, 16, 80, device=DEV)
                    f[0] = solo[16 * p:16 * p + 16]
                    st.push(f)
                if with_audio:
                    st.push_audio(w[p * MAX_AUDIO:(p + 1) * MAX_AUDIO][None].expand(2, -1), end=[False, p == 7])
            out = [(st.encoder_out(b).clone(), st.frames()[b], st.release(b)) if on else None for b, on in enumerate((with_feats, with_audio))]
            st.finish()
            return out

        with torch.no_grad():
            solo = solo_features(nn_, brain, wavs, prior)["s1"]
            mixed, feats_alone, audio_alone = run(True, True, solo), run(True, False, solo), run(False, True, solo)
        for b, alone in ((0, feats_alone), (1, audio_alone)):
            assert mixed[b][0].shape == alone[b][0].shape and mixed[b][0].shape[0] == (32 if b == 0 else 26)      # 101 frames: 25 groups + the tail
            assert torch.equal(mixed[b][0].view(torch.uint8), alone[b][0].view(torch.uint8)) and mixed[b][1:] == alone[b][1:], b
    finally:
        nn_.set_compute_dtype(torch.bfloat16)
