"""Per-chunk cost of streaming transcription (ts-asr_amd/streaming.py) at BASELINE.json configs[1] model size (d_model 256, 12 layers,
4 heads), causal encoder with block-causal attention over chunks of 40 frames, bf16, deterministic weights.

    python tools/stream_bench.py [--B 1 32] [--t0 0 1000 3960] [--reps 20] [--json out.json]
    python tools/stream_bench.py --audio                                  # also: the same push fed 1.6 s of waveform (push_audio)
    python tools/stream_bench.py --slots                                  # slot mode (start(slots=True)) beside the lockstep push
    python tools/stream_bench.py --slots --audio                          # also: every slot a session fed 1.6 s of waveform (admit(audio=True))
    python tools/stream_bench.py --profile-chunks 20 --B 32 --t0 3960     # under rocprofv3 --kernel-trace --stats: 20 chunks and nothing else timed

A chunk is one push of 160 mel frames = 40 encoder frames = 1.6 s of audio. The time of a push is host wall-clock from the call to
the return of its new tokens (the push reads its symbols back, so the device work is included), the median over --reps pushes. For
each offset t0 the stream is moved there by setting its frame counter (the cost of a chunk does not depend on what the cache holds).
Kernel launches per chunk are counted with torch.profiler. Real-time factor = time per chunk / 1.6 s.
--audio: a second stream of the same model started with audio=True is pushed 25600 samples at a time (in the steady state every such
push completes exactly one group of 160 causal feature frames: nnet.CausalFeatures, then the same push()); its median is reported beside
the feature push's, with the median of the feature stage alone (CausalFeatures.forward_chunk on a stream of its own).
--slots: B = 32 and B = 1, every slot occupied, the slots' offsets spread evenly over 0 .. 3960 (B = 1: at 3960) and put back there
before every push; the median of 15 pushes, the second half of which each do one release() + admit() inside the timed region. The
lockstep push at t0 = 1000 and t0 = 3960 is timed in the same run (15 pushes each), with the kernel launches per chunk of all three.
--slots --audio: also B = 32 and B = 1 with every slot an audio session (admit(..., audio=True)) pushed 25600 samples at a time, at the same
spread offsets: ms per push_audio (median, min, max of 15) and of the feature stage alone (one ring append, the per-slot frame kernel and
the running normalisation on a state of their own, with their two small host tables), beside the lockstep --audio figures at the same B.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "ts-asr_amd"
CHUNK_MEL, CHUNK_ENC, AUDIO_MS = 160, 40, 1600.0
CHUNK_SAMPLES = 160 * CHUNK_MEL


def build(device):
    from oracle.golden_recipe import load_det_weights
    hp = importlib.import_module(PKG + ".hparams")
    tsasr = importlib.import_module(PKG + ".recipes.tsasr")
    ov = dict(input_is_feats=True, compute_dtype="bf16", causal_encoder=True, frontend_padding="causal", attention_chunk_size=40, dropout=0.0)
    with open(os.path.join(ROOT, "hparams", "conformer-t_scratch_mi355x.yaml")) as f:
        h = hp.load_hyperpyyaml(f, ov)
    for name, mod in h["modules"].items():
        if isinstance(mod, torch.nn.Module):
            load_det_weights(mod, name + ".")
    brain = tsasr.TSASR(h["modules"], h["opt_class"], h, {"device": device, "compute_dtype": "bf16"})
    brain.modules.eval()
    return brain, h


def make_stream(streaming, brain, B, max_frames, device):
    D = brain.modules.encoder.d_model
    g = torch.Generator(device="cpu").manual_seed(7)
    spk = (torch.randn(B, 1, D, generator=g) * 0.5).to(device)
    st = streaming.StreamingTranscriber(brain)
    st.start(B, max_frames, speaker_embs=spk)
    feats = torch.randn(B, CHUNK_MEL, 80, generator=g).to(device)
    return st, feats


def make_audio_stream(streaming, brain, B, max_frames, device):
    D = brain.modules.encoder.d_model
    g = torch.Generator(device="cpu").manual_seed(7)
    spk = (torch.randn(B, 1, D, generator=g) * 0.5).to(device)
    st = streaming.StreamingTranscriber(brain)
    st.start(B, max_frames, speaker_embs=spk, audio=True)
    wav = (torch.randn(B, CHUNK_SAMPLES, generator=g) * 0.05).to(device)
    return st, wav


def time_audio(st, wav, t0, reps):
    """Median ms of push_audio (features + push) and median, min, max ms of the feature stage alone, at encoder offset t0."""
    both, alone = [], []
    fs = st.features.init_stream(wav.shape[0], wav.device)
    st.features.forward_chunk(wav, fs, group=CHUNK_MEL)
    for _ in range(reps):
        place(st, t0)
        torch.cuda.synchronize()
        s = time.perf_counter()
        st.push_audio(wav)
        both.append((time.perf_counter() - s) * 1e3)
        torch.cuda.synchronize()
        s = time.perf_counter()
        f, _, fs = st.features.forward_chunk(wav, fs, group=CHUNK_MEL)
        torch.cuda.synchronize()
        alone.append((time.perf_counter() - s) * 1e3)
        assert f.shape[1] == CHUNK_MEL
    return statistics.median(both), statistics.median(alone), min(alone), max(alone)


def make_slot_stream(streaming, brain, B, max_frames, device):
    D = brain.modules.encoder.d_model
    g = torch.Generator(device="cpu").manual_seed(7)
    spk = (torch.randn(B, 1, D, generator=g) * 0.5).to(device)
    st = streaming.StreamingTranscriber(brain)
    st.start(B, max_frames, slots=True)
    for b in range(B):
        st.admit(b, speaker_embs=spk[b:b + 1])
    feats = torch.randn(B, CHUNK_MEL, 80, generator=g).to(device)
    offs = [3960] if B == 1 else [round(3960 * b / (B - 1) / CHUNK_ENC) * CHUNK_ENC for b in range(B)]
    return st, feats, spk, offs


def make_slot_audio_stream(streaming, brain, B, max_frames, device):
    D = brain.modules.encoder.d_model
    g = torch.Generator(device="cpu").manual_seed(7)
    spk = (torch.randn(B, 1, D, generator=g) * 0.5).to(device)
    st = streaming.StreamingTranscriber(brain)
    st.start(B, max_frames, slots=True, max_audio_samples=CHUNK_SAMPLES)
    for b in range(B):
        st.admit(b, speaker_embs=spk[b:b + 1], audio=True)
    wav = (torch.randn(B, CHUNK_SAMPLES, generator=g) * 0.05).to(device)
    offs = [3960] if B == 1 else [round(3960 * b / (B - 1) / CHUNK_ENC) * CHUNK_ENC for b in range(B)]
    return st, wav, offs


def time_slot_audio(st, wav, offs, reps):
    """ms of `reps` push_audio calls in slot mode at the spread offsets (every one completes one group of 160 frames per slot), and of the
    feature stage alone on slot state of its own: the append, the frames of every slot from its ring, the running normalisation."""
    both, alone, B = [], [], wav.shape[0]
    cf, cap, dev = st.features, st.feat_slots["ring"].shape[1], wav.device
    fs = cf.init_slots(B, cap, dev)
    have = emitted = 0

    def feature_stage(frames):
        nonlocal have, emitted
        cf.append_slots(fs, wav, torch.tensor([[have % cap] * B, [CHUNK_SAMPLES] * B], dtype=torch.int32, device=dev))
        have += CHUNK_SAMPLES
        if frames:
            f = cf.frames_slots(fs, torch.tensor([[emitted] * B, [frames] * B, [have] * B], dtype=torch.int32, device=dev), frames)
            emitted += frames
            return f

    feature_stage(0)                                 # (the first push completes no group of 160 frames: 16 ms of look-ahead)
    for _ in range(3):
        feature_stage(CHUNK_MEL)
    for _ in range(reps):
        place_slots(st, offs)
        torch.cuda.synchronize()
        s = time.perf_counter()
        st.push_audio(wav)
        both.append((time.perf_counter() - s) * 1e3)
        assert st.audio_steps[-1][0] == CHUNK_MEL and all(st.audio_steps[-1][1])
        torch.cuda.synchronize()
        s = time.perf_counter()
        feature_stage(CHUNK_MEL)
        torch.cuda.synchronize()
        alone.append((time.perf_counter() - s) * 1e3)
    return both, alone


def place_slots(st, offs):
    """Move every slot to its encoder frame (the caches keep whatever they hold)."""
    st.enc_state["t0"] = list(offs)
    t = torch.tensor(offs, dtype=torch.int32, device=st.mel.device)
    st.enc_state["t0s"].copy_(t)
    st.mel.copy_(4 * t.long())


def time_slots(st, feats, spk, offs, reps):
    """ms of `reps` slot pushes at the spread offsets; from the middle on each push also releases and admits one slot."""
    times, B = [], len(offs)
    for n in range(reps):
        place_slots(st, offs)
        torch.cuda.synchronize()
        s = time.perf_counter()
        if n >= reps // 2:
            b = n % B
            st.release(b)
            st.admit(b, speaker_embs=spk[b:b + 1])
        st.push(feats)
        times.append((time.perf_counter() - s) * 1e3)
    return times


def place(st, t0):
    """Move the stream to encoder frame t0 (the caches keep whatever they hold)."""
    st.enc_state["t0"] = t0
    st.mel.fill_(4 * t0)


def count_launches(st, feats, t0):
    from torch.profiler import ProfilerActivity, profile
    place_slots(st, t0) if isinstance(t0, list) else place(st, t0)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        st.push(feats)
        torch.cuda.synchronize()
    kinds = {}
    n = 0
    for e in p.events():
        if getattr(e, "device_type", None) is not None and str(e.device_type).endswith("CUDA") and e.name and "Memcpy" not in e.name \
                and "Memset" not in e.name:
            n += 1
            kinds[e.name] = kinds.get(e.name, 0) + 1
    return n, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--t0", type=int, nargs="+", default=[0, 1000, 3960])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-frames", type=int, default=4000)
    ap.add_argument("--no-split", action="store_true", help="attention without the key split (prices the split)")
    ap.add_argument("--audio", action="store_true", help="also time push_audio of 1.6 s of waveform (causal features + the same push)")
    ap.add_argument("--slots", action="store_true", help="slot mode at spread offsets beside the lockstep push at t0 = 1000 and 3960, 15 pushes each")
    ap.add_argument("--profile-chunks", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    device = "cuda:0"
    streaming = importlib.import_module(PKG + ".streaming")
    ops = importlib.import_module(PKG + ".ops")
    if a.no_split:
        ops.relpos_attn_stream_workspace = lambda *args, **kw: None
    brain, _ = build(device)
    results = []
    if a.slots:
        a.B, a.t0, a.reps = [32, 1], [1000, 3960], 15
    with torch.no_grad():
        for B in a.B:
            if a.slots:
                sts, feats_s, spk, offs = make_slot_stream(streaming, brain, B, a.max_frames, device)
                for _ in range(3):
                    place_slots(sts, offs)
                    sts.push(feats_s)
                times = time_slots(sts, feats_s, spk, offs, a.reps)
                try:
                    n, _ = count_launches(sts, feats_s, offs)
                except Exception as e:
                    n = f"n/a ({type(e).__name__})"
                med = statistics.median(times)
                r = {"B": B, "mode": "slots", "offsets": [offs[0], offs[-1]], "ms_per_chunk_median": round(med, 3), "ms_min": round(min(times), 3),
                     "ms_max": round(max(times), 3), "kernel_launches_per_chunk": n, "rtf": round(med / AUDIO_MS, 5)}
                print(json.dumps(r), flush=True)
                results.append(r)
                del sts
                if a.audio:
                    sta_s, wav_s, offs = make_slot_audio_stream(streaming, brain, B, a.max_frames, device)
                    for _ in range(4):
                        place_slots(sta_s, offs)
                        sta_s.push_audio(wav_s)
                    both, alone = time_slot_audio(sta_s, wav_s, offs, a.reps)
                    med = statistics.median(both)
                    r = {"B": B, "mode": "slots-audio", "offsets": [offs[0], offs[-1]], "ms_per_audio_chunk_median": round(med, 3),
                         "ms_min": round(min(both), 3), "ms_max": round(max(both), 3), "ms_features_median": round(statistics.median(alone), 3),
                         "ms_features_min": round(min(alone), 3), "ms_features_max": round(max(alone), 3), "rtf_audio": round(med / AUDIO_MS, 5)}
                    print(json.dumps(r), flush=True)
                    results.append(r)
                    del sta_s
            st, feats = make_stream(streaming, brain, B, a.max_frames, device)
            for _ in range(0 if a.profile_chunks else 3):     # warm-up: allocations, workspaces, first launches
                st.push(feats)
            if a.profile_chunks:
                for t0 in a.t0:
                    for _ in range(a.profile_chunks):
                        if st.enc_state is not None:
                            place(st, t0)
                        st.push(feats)                          # (the first push allocates the stream and runs at t0 = 0)
                torch.cuda.synchronize()
                print(json.dumps({"profiled_chunks": a.profile_chunks, "B": B, "t0": a.t0}))
                continue
            if a.audio:
                sta, wav = make_audio_stream(streaming, brain, B, a.max_frames, device)
                for _ in range(4):                              # (the first push completes no group of 160 frames: 16 ms of look-ahead)
                    sta.push_audio(wav)
            for t0 in a.t0:
                times = []
                for _ in range(a.reps):
                    place(st, t0)
                    torch.cuda.synchronize()
                    s = time.perf_counter()
                    st.push(feats)
                    times.append((time.perf_counter() - s) * 1e3)
                try:
                    n, _ = count_launches(st, feats, t0)
                except Exception as e:                          # (profiler not usable: report the timing anyway)
                    n = f"n/a ({type(e).__name__})"
                med = statistics.median(times)
                r = {"B": B, "t0": t0, "ms_per_chunk_median": round(med, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                     "kernel_launches_per_chunk": n, "rtf": round(med / AUDIO_MS, 5), "split": not a.no_split}
                if a.audio:
                    med_a, med_f, min_f, max_f = time_audio(sta, wav, t0, a.reps)
                    r.update({"ms_per_audio_chunk_median": round(med_a, 3), "ms_features_median": round(med_f, 3), "ms_features_min": round(min_f, 3),
                              "ms_features_max": round(max_f, 3), "rtf_audio": round(med_a / AUDIO_MS, 5)})
                print(json.dumps(r), flush=True)
                results.append(r)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"workload": "streaming configs[1] causal chunk 40, bf16, 160 mel frames per push", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
