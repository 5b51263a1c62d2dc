"""StreamingTranscriber(start(slots=True)) on the MI355X: four sessions (the golden utterances with their golden speaker embeddings)
enter and leave three slots of a running batch, and each one gets the bits of the lockstep transcriber at batch_size = 3 with the
session in the same slot, the same push sizes and zeros in the other rows.

Schedule (pushes of 32 feature frames = 8 encoder frames): s0 enters slot 0 at tick 0; s1 enters slot 2 at tick 1 and is paused at tick
2; slot 1 stays free for four ticks, then takes s3; s0 ends at tick 2 with a short mel_lens, is released at tick 3, and s2 is admitted
into slot 0 in the same tick with its own embedding. Before the first admission the K/V caches are filled with NaN: admit() does not
clear them, and rows at or past a slot's offset are never read."""
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
from oracle.golden_recipe import CFG1, golden_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, PUSH, MAXF = 3, 32, 48
SESS = {"s0": dict(row=0, slot=0, npush=3, last_mel=20), "s1": dict(row=1, slot=2, npush=4), "s2": dict(row=2, slot=0, npush=3),
        "s3": dict(row=3, slot=1, npush=3)}
TICKS = [dict(admit=["s0"]), dict(admit=["s1"]), dict(pause=[2]), dict(release=["s0"], admit=["s2"]), dict(admit=["s3"]), dict(),
         dict(release=["s1", "s2"])]


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture(scope="module")
def mods():
    return (importlib.import_module("ts-asr_amd.ops"), importlib.import_module("ts-asr_amd.nnet"),
            importlib.import_module("ts-asr_amd.streaming"))


def speaker(mode, golden):
    """-> (embeddings [4,S,D], valid rows of each) of the golden batch."""
    inp = golden_inputs()
    if mode != "cross_attention":
        e = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)
        return e, [e.shape[1]] * 4
    from tests.test_oracle_golden import full_state_dict
    cc = {}
    R.compute_forward({k: T(v) for k, v in inp.items()}, full_state_dict(CFG1, mode), CFG1, mode, True, "causal", collect=cc)
    e = cc["spk_emb"].float().to(DEV)
    return e, [int(round(float(x) * e.shape[1])) for x in inp["enroll_lens"]]


def state_of(st, b):
    """Clones of every piece of state slot b owns."""
    es = st.enc_state
    out = [es["t0s"][b].clone(), torch.tensor(es["t0"][b]), st.mel[b].clone()] + [c[b].clone() for c in st.fe_state]
    for layer in es["layers"]:
        out += [layer["k"][b].clone(), layer["v"][b].clone(), layer["hist"][0][b].clone()]
    ss = st.search_state
    if "max_frames" in ss:                       # device beam search: the slot's block of the workspace
        per = ss["dev"].numel() // ss["B"]
        out.append(ss["dev"][b * per:(b + 1) * per].clone())
    else:
        out.append(ss["dev"][b].clone())
    if isinstance(ss.get("frames_done"), torch.Tensor):
        out.append(ss["frames_done"][b].clone())
    return out


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.uint8) if x.is_floating_point() else x, y.view(torch.uint8) if y.is_floating_point() else y)
                                    for x, y in zip(a, b))


def run_slots(streaming, brain, feats, emb, emb_n, search, timed, searcher=None):
    """The schedule -> {session: dict(hyp, frames, enc, nbest, scores, nbest_frames)}."""
    st = streaming.StreamingTranscriber(brain, search=search)
    if searcher is not None:
        st.searcher = searcher
    res, owner, done = {}, [None] * NS, {n: 0 for n in SESS}
    Sm = emb.shape[1]
    st.start(NS, MAXF, slots=True, max_speaker_frames=Sm, keep_encoder_out=True, timestamps=timed)
    assert st.occupied == [False] * NS
    for layer in st.enc_state["layers"]:
        layer["k"].fill_(float("nan"))
        layer["v"].fill_(float("nan"))
    for n_tick, tick in enumerate(TICKS + [dict(release=["s3"])]):
        for name in tick.get("release", ()):
            b = SESS[name]["slot"]
            assert st.encoder_frames(b) == 8 * SESS[name]["npush"]
            r = dict(enc=st.encoder_out(b).clone(), frames=st.frames()[b] if timed else None)
            r["hyp"] = st.release(b)
            if search == "beam":
                r["nbest"], r["scores"] = (x[b] for x in st.nbest())
                r["nbest_frames"] = st.nbest_frames()[b] if timed else None
            res[name], owner[b] = r, None
        if n_tick == len(TICKS):
            break
        for name in tick.get("admit", ()):
            s = SESS[name]
            n = emb_n[s["row"]]
            st.admit(s["slot"], speaker_embs=emb[s["row"]:s["row"] + 1, :n], speaker_embs_length=torch.ones(1))
            owner[s["slot"]] = name
            assert st.encoder_frames(s["slot"]) == 0
        paused = tick.get("pause", ())
        f = torch.zeros(NS, PUSH, feats.shape[2], device=DEV)
        ml = torch.full((NS,), PUSH, dtype=torch.int64)
        active = [False] * NS
        for b, name in enumerate(owner):
            if name is None or b in paused or done[name] == SESS[name]["npush"]:
                continue
            s = SESS[name]
            f[b] = feats[s["row"], done[name] * PUSH:(done[name] + 1) * PUSH]
            done[name] += 1
            if done[name] == s["npush"] and "last_mel" in s:
                ml[b] = s["last_mel"]
            active[b] = True
        before = {b: state_of(st, b) for b in range(NS) if not active[b] and st.search_state is not None}
        hyps_before = [list(h) for h in st.hyps]
        explicit = active != st.occupied            # a paused or finished-but-occupied slot: name the active ones
        ret = st.push(f, mel_lens=ml, active=active if explicit else None)
        for b, snap in before.items():              # an idle slot (free, paused or ended): nothing of its state moved
            assert same(snap, state_of(st, b)), f"tick {n_tick}: state of idle slot {b} moved"
            assert ret[b] == ([] if search == "greedy" else hyps_before[b]) and st.hyps[b] == hyps_before[b], (n_tick, b)
    assert st.occupied == [False] * NS
    return res


def run_lockstep(streaming, brain, feats, emb, emb_n, search, timed, name, searcher=None):
    s = SESS[name]
    b, Sm = s["slot"], emb.shape[1]
    st = streaming.StreamingTranscriber(brain, search=search)
    if searcher is not None:
        st.searcher = searcher
    spk = torch.zeros(NS, Sm, emb.shape[2], dtype=emb.dtype, device=DEV)
    n = emb_n[s["row"]]
    spk[b, :n] = emb[s["row"], :n]
    lens = torch.ones(NS, dtype=torch.float32, device=DEV)
    lens[b] = n / Sm
    st.start(NS, MAXF, speaker_embs=spk, speaker_embs_length=lens, keep_encoder_out=True, timestamps=timed)
    for p in range(s["npush"]):
        f = torch.zeros(NS, PUSH, feats.shape[2], device=DEV)
        f[b] = feats[s["row"], p * PUSH:(p + 1) * PUSH]
        ml = torch.zeros(NS, dtype=torch.int64)         # the other rows carry no frames
        ml[b] = s["last_mel"] if p == s["npush"] - 1 and "last_mel" in s else PUSH
        st.push(f, mel_lens=ml)
    r = dict(enc=st.encoder_out()[b], frames=st.frames()[b] if timed else None)
    if search == "beam":
        r["nbest"], r["scores"] = (x[b] for x in st.nbest())
        r["nbest_frames"] = st.nbest_frames()[b] if timed else None
    r["hyp"] = st.finish()[b]
    return r


def compare(tag, got, want, search, timed):
    for name in SESS:
        g, w = got[name], want[name]
        assert g["enc"].shape == w["enc"].shape and torch.equal(g["enc"].view(torch.uint8), w["enc"].contiguous().view(torch.uint8)), \
            f"{tag} {name}: encoder_out bits differ from the lockstep run"
        assert g["hyp"] == w["hyp"], (tag, name, g["hyp"], w["hyp"])
        if timed:
            assert g["frames"] == w["frames"], (tag, name)
        if search == "beam":
            assert g["nbest"] == w["nbest"], (tag, name)
            assert [np.float64(x).tobytes() for x in g["scores"]] == [np.float64(x).tobytes() for x in w["scores"]], (tag, name)
            if timed:
                assert g["nbest_frames"] == w["nbest_frames"], (tag, name)
    print(f"STREAM-SLOTS {tag}: tokens per session {[len(got[n]['hyp']) for n in SESS]}")


def both(mods, golden, dtype, mode, chunk, search, timed, searcher=None):
    ops, nn_, streaming = mods
    kw = dict(attention_chunk_size=chunk) if chunk else {}
    brain, h = entry._config1_brain(DEV, dtype, causal_encoder=True, frontend_padding="causal", injection_mode=mode, **kw)
    try:
        feats = T(golden["c1_features"]["norm"]).to(DEV)
        emb, emb_n = speaker(mode, golden)
        srch = searcher(h) if searcher is not None else None
        with torch.no_grad():
            got = run_slots(streaming, brain, feats, emb, emb_n, search, timed, srch)
            want = {n: run_lockstep(streaming, brain, feats, emb, emb_n, search, timed, n, srch) for n in SESS}
        compare(f"{dtype}-{mode}-chunk{chunk}-{search}{'-timed' if timed else ''}", got, want, search, timed)
        return got
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("dtype,mode,chunk", [("fp32", "cat", 0), ("bf16", "cat", 0), ("fp32", "cross_attention", 0), ("bf16", "cross_attention", 0),
                                              ("fp32", "cat", 8), ("bf16", "cat", 8)])
def test_slots_greedy_equals_lockstep(mods, golden, dtype, mode, chunk):
    both(mods, golden, dtype, mode, chunk, "greedy", True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_slots_beam_equals_lockstep(mods, golden, dtype, timed):
    got = both(mods, golden, dtype, "cat", 0, "beam", timed, _golden_beam_searcher(golden))
    assert sum(len(got[n]["hyp"]) for n in SESS) > 0 and all(len(got[n]["nbest"]) > 1 for n in SESS)


def _golden_beam_searcher(golden):
    """The recipe's beam searcher at beam 4 / nbest 3 with the head's blank bias raised as the golden beam fixtures raise it
    (oracle/gen_golden_beam.py: the untrained network would otherwise emit at every frame and the search would not stay within cap)."""
    def make(h):
        s = h["beam_searcher"]
        s.beam_size, s.nbest = 4, 3
        with torch.no_grad():
            s.classifier_network[0].w.bias[0] += float(golden["c1_beam"]["blank_bias"])
        return s
    return make


def _subword_searcher(h):
    """A subword beam searcher (V = 256, learned embedding) on the model's joint dimension; the head's bias leans to blank so that the
    untrained network keeps the search small."""
    nnet, dec, rnnt = (importlib.import_module(f"ts-asr_amd.{m}") for m in ("nnet", "decoders", "rnnt"))
    J, V, Hd = h["modules"]["encoder_proj"].w.out_features, 256, 128
    torch.manual_seed(11)
    emb, lstm, proj, head = nnet.Embedding(V, embedding_dim=64), nnet.LSTM(Hd, input_size=64), nnet.Linear(J, input_size=Hd), nnet.Linear(V, input_size=J)
    with torch.no_grad():
        head.w.weight.mul_(2.0)
        head.w.bias.zero_()
        head.w.bias[0] = 3.0
    mods_ = [m.to(DEV).eval() for m in (emb, lstm, proj, head)]
    s = dec.TransducerBeamSearcher(mods_[:3], rnnt.Transducer_joint(), [mods_[3]], blank_id=0, beam_size=4, nbest=4)
    assert s._beam_is_wide()
    return s


def test_slots_beam_subword_equals_lockstep(mods, golden):
    both(mods, golden, "bf16", "cat", 0, "beam", True, _subword_searcher)


def test_slots_strict_hip_stays_silent(mods, golden, monkeypatch):
    ops = mods[0]
    monkeypatch.setattr(ops, "STRICT_HIP", True)
    ops.LIB_FALLBACKS.clear()
    both(mods, golden, "bf16", "cat", 8, "greedy", True)
    assert ops.LIB_FALLBACKS == {}


def test_slots_error_cases(mods, golden):
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal")
    feats = T(golden["c1_features"]["norm"]).to(DEV)
    emb, _ = speaker("cat", golden)
    inp = golden_inputs()
    st = streaming.StreamingTranscriber(brain)
    try:
        with torch.no_grad():
            with pytest.raises(ValueError):
                st.start(NS, 12, slots=True, audio=True)
            with pytest.raises(ValueError):
                st.start(NS, 12, slots=True, speaker_embs=emb[:NS])
            st.start(NS, 12, slots=True)
            with pytest.raises(ValueError, match="free"):
                st.push(feats[:NS, :32], active=[True, False, False])           # no session in slot 0 yet
            st.admit(0, speaker_embs=emb[0:1])
            st.admit(1, speaker_embs=emb[1:2])
            with pytest.raises(ValueError, match="occupied"):
                st.admit(1, speaker_embs=emb[2:3])
            with pytest.raises(ValueError, match="free"):
                st.push(feats[:NS, :32], active=[True, True, True])
            st.push(feats[:NS, :32], active=[True, False, False])               # slot 0 at 8 frames, slot 1 (paused) at 0
            assert (st.encoder_frames(0), st.encoder_frames(1)) == (8, 0)
            before = [state_of(st, b) for b in range(NS)]
            with pytest.raises(ValueError, match=r"slot 0 .*max_frames"):
                st.push(feats[:NS, 32:64])                                       # 8 + 8 > 12 for slot 0 alone
            assert all(same(a, state_of(st, b)) for b, a in enumerate(before)), "a refused push moved state"
            assert (st.encoder_frames(0), st.encoder_frames(1)) == (8, 0)
            st.push(feats[:NS, 32:48])                                           # 8 + 4 fits
            assert (st.encoder_frames(0), st.encoder_frames(1), int(st.encoder_frames)) == (12, 4, 12)
            with pytest.raises(ValueError, match="free"):
                st.release(2)
            assert isinstance(st.release(0), list) and st.occupied == [False, True, False]
            # admit(enroll=...): one utterance through the recipe's speaker branch, as start(enroll=...) computes it for a batch
            st.admit(2, enroll=(T(inp["enroll_sig"][2:3]).to(DEV), T(inp["enroll_lens"][2:3]).to(DEV)))
            e = float((st.spk[2:3].float().cpu() - emb[2:3].cpu()).norm() / emb[2:3].cpu().norm())
            print(f"speaker embedding through admit(enroll=...) vs reference: {e:.2e}")
            assert e < 1e-3, e
            assert torch.equal(st.spk[1:2], emb[1:2]) and st.occupied == [False, True, True]
            st.finish()
    finally:
        nn_.set_compute_dtype(torch.bfloat16)


def test_encoder_forward_chunk_slot_checks(mods, golden):
    """ConformerEncoder.forward_chunk on a slot state: ValueError, naming the slot and before any state moves, for an active slot whose
    chunk would pass max_frames or whose offset is no multiple of the attention block; idle slots do not advance."""
    ops, nn_, streaming = mods
    brain, h = entry._config1_brain(DEV, "fp32", causal_encoder=True, frontend_padding="causal", attention_chunk_size=8)
    brain._setup_dtype()
    enc = brain.modules.encoder.eval()
    try:
        with torch.no_grad():
            state = enc.init_stream(NS, 20, device=DEV, slots=True)
            x = torch.randn(NS, 8, CFG1["encoder_input_size"], generator=torch.Generator().manual_seed(1)).to(DEV)
            spk = T(golden["c1_chain_cat"]["spk_emb"]).to(DEV)[:NS]
            with pytest.raises(ValueError):
                enc.forward_chunk(x, enc.init_stream(NS, 20, device=DEV), spk, active=[True] * NS)      # `active` needs a slot state
            enc.forward_chunk(x[:, :4], state, spk, active=[True, False, False])                        # a last, short chunk for slot 0
            assert state["t0"] == [4, 0, 0] and state["t0s"].tolist() == [4, 0, 0]
            snap = [t.clone() for layer in state["layers"] for t in (layer["k"], layer["v"], layer["hist"][0])]
            with pytest.raises(ValueError, match="slot 0"):
                enc.forward_chunk(x, state, spk, active=[True, True, False])                            # offset 4 is inside a block of 8
            enc.forward_chunk(x, state, spk, active=[False, True, True])
            enc.forward_chunk(x, state, spk, active=torch.tensor([False, True, False]))
            assert state["t0"] == [4, 16, 8] and state["t0s"].tolist() == [4, 16, 8]
            snap = [t.clone() for layer in state["layers"] for t in (layer["k"], layer["v"], layer["hist"][0])]
            with pytest.raises(ValueError, match=r"slot 1.*max_frames"):
                enc.forward_chunk(x, state, spk, active=[False, True, True])                            # 16 + 8 > 20 for slot 1 alone
            now = [t for layer in state["layers"] for t in (layer["k"], layer["v"], layer["hist"][0])]
            assert state["t0"] == [4, 16, 8] and all(torch.equal(a, b) for a, b in zip(snap, now))
            out = enc.forward_chunk(x, state, spk, active=[False, False, True])
            assert state["t0"] == [4, 16, 16] and bool(torch.isfinite(out).all())
    finally:
        nn_.set_compute_dtype(torch.bfloat16)
