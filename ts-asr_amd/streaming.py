"""Chunk-by-chunk transcription with a causal TS-ASR model (``causal_encoder: True``, ``frontend_padding: causal``).

    st = StreamingTranscriber(brain)
    st.start(batch_size=B, max_frames=4000, enroll=(enroll_sig, enroll_lens))     # or speaker_embs=..., or nothing (variant none)
    with torch.no_grad():
        for feats in chunks:                        # [B, F, 80] normalised fbank frames, F a multiple of 4
            new_tokens = st.push(feats)             # list (per stream) of the symbols emitted for these frames
        # or, after start(..., audio=True): st.push_audio(wav) with wav [B, N] samples, any N
        hyps = st.finish()

StreamingTranscriber(brain, search="beam") decodes with the recipe's beam searcher instead (TransducerBeamSearcher.beam_stream): push()
then returns each stream's best hypothesis so far as a whole token list (its prefix may change), finish() the best hypotheses and
nbest() the n-best lists with their logp / len.

start(..., timestamps=True) also keeps when each token was emitted: frames() returns, per stream, the absolute encoder frame of every
token of the hypothesis finish() would return now (greedy: the accumulated list; beam: the current best hypothesis's), nbest_frames()
goes with nbest(). Seconds are frames x align.frame_seconds(hparams); word spans come from align.word_spans.

Every block of such a model is causal: the front-end pads time on the left only, the depthwise convolution is left-padded, the
attention mask (look-ahead or block-causal on absolute frame indices) never looks past the current chunk, and RelPosEncXL's table is
symmetric, so one half table serves every offset. A push therefore costs the new frames only: the front-end carries the last 2 input
frames of each block, every encoder layer a K/V cache and the K-1 GLU rows of its convolution, the greedy search its predictor state
(ConvolutionFrontEnd.forward_chunk, ConformerEncoder.forward_chunk, TransducerBeamSearcher.greedy_stream). The valid encoder rows
equal those of the offline causal encoder over the whole utterance.

Features reach the stream by one of two routes. push(feats) takes normalised feature frames the caller computed: the recipe's Fbank
clamps each utterance at ``top_db`` below its own maximum and InputNormalization (``norm_type: sentence``) uses the utterance's mean and
deviation - statistics of the whole utterance, which a live signal does not have yet; this route serves recorded utterances (the offline
pair's output) or features normalised with statistics the caller chooses. start(..., audio=True) + push_audio(wav) takes the waveform, any
number of samples per push: nnet.CausalFeatures computes each frame from the samples so far (16 ms of look-ahead), floors it at ``top_db``
below the running maximum and normalises it with the running mean and deviation (optionally started from ``feature_prior``), buffers
samples until a whole group of frames is complete and hands those to push(). Its frames do not depend on how the audio is cut into pushes.
A model trained with the sentence-level features sees different inputs under audio=True: train with ``causal_features: True`` (the
mixture branch then runs the same CausalFeatures) for a match.

With block-causal attention (``attention_chunk_size`` c > 1) a push holds a multiple of 4c feature frames (a frame attends its
whole block, so a push cannot end inside one).

Streams of different lengths share a batch: each one stops at its own valid count, ``ceil(ceil(L/2)/2)`` encoder frames for L valid
mel frames pushed so far (``mel_lens`` per push, default the whole push); ``enc_lens`` overrides that count (absolute encoder frames).
Inference only: eval mode, under torch.no_grad().

Slots (start(..., slots=True)): the B rows of the batch are slots that sessions enter and leave while the batch runs.

    st.start(batch_size=B, max_frames=4000, slots=True, max_speaker_frames=S)      # every slot begins free
    st.admit(2, speaker_embs=emb)               # or enroll=(signal, length): one utterance through the recipe's speaker branch
    new = st.push(feats)                        # feats [B, F, 80]; the occupied slots advance, the others keep every bit of state
    new = st.push(feats, active=[True, False, True])      # an occupied slot left out is paused
    hyp = st.release(2)                         # the session's hypothesis; the slot is free again

Every slot has its own offset (a device int32 array the kernels read, tsasr_relpos_attn_stream_slots_fwd, and a host mirror), mel
count, front-end carry, conv histories and search state; admit() resets them for that slot alone. The K/V cache rows are not cleared:
rows at or past a slot's offset are never read. mel_lens / enc_lens, the emission frames, encoder_out(slot) and encoder_frames(slot) are
absolute in the slot's own session. A session is still bounded by max_frames.

Slot sessions fed audio (admit(slot, ..., audio=True)): every such session has its own sample count, frame position and running
statistics, in one batch with feature-fed sessions if need be.

    st.start(batch_size=B, max_frames=4000, slots=True, max_audio_samples=32000)
    st.admit(0, speaker_embs=emb, audio=True)                   # feature_prior=(mean, std, n0) starts this session's statistics
    new = st.push_audio(wav, wav_lens=[1600, 0, 777])           # wav [B, N]: each active slot's next samples, any number per slot
    new = st.push_audio(wav, end=[True, False, False])          # session 0's audio stops with this call: its last frames go out
    hyp = st.release(0)

The samples live in a ring per slot on the device (tsasr_audio_ring_append: one launch per call appends every slot's packet), the frames
of a step are computed by one launch that reads each slot's frames from its own position in its own ring (tsasr_fbank_frames_slots: the
frame body of the offline kernel), normalised by the running_norm kernel on a state row per slot, and handed to the slot push():
whatever B, no per-session launch, copy or concatenation. Which frames go when is plan_audio_steps' rule; audio_steps logs it. A
session's frames are the bits nnet.CausalFeatures.forward gives for its audio alone. start(slots=True, audio=True) still raises: in
slot mode audio is a property of a session (admit), not of the batch.
"""
import types

import torch

from . import _capi as C

__all__ = ["StreamingTranscriber", "audio_frames_available", "audio_ring_capacity", "plan_audio_steps"]


def audio_frames_available(samples, ended, hop=160, pad=256):
    """Causal feature frames of a session that has received ``samples`` samples: frame k covers samples [k*hop - pad, k*hop + pad), so
    a live session has frames 0 .. (samples - pad)//hop once ``pad`` samples are there; an ended one (zeros follow) all 1 + samples//hop."""
    if ended:
        return 1 + samples // hop
    return (samples - pad) // hop + 1 if samples >= pad else 0


def audio_ring_capacity(max_audio_samples, group, hop=160, pad=256):
    """Samples per slot of the ring that feeds audio sessions. The oldest sample a session with e frames emitted still needs is
    e*hop - pad. After a drain a live session has fewer than ``group`` available frames left, (P - pad)//hop + 1 - e <= group - 1,
    hence P < (e + group - 1)*hop + pad: it needs fewer than (group - 1)*hop + 2*pad samples (a session with P < pad needs P + pad <
    2*pad; an ended one is drained completely). The next push adds at most max_audio_samples."""
    return int(max_audio_samples) + (int(group) - 1) * hop + 2 * pad


def _ring_needed(samples, emitted, hop, pad):
    """Samples of a session the ring must still hold: from the first one its next frame reads to the last one received."""
    return samples - max(emitted * hop - pad, 0)


def plan_audio_steps(samples, emitted, ended, group, hop=160, pad=256):
    """The engine steps that drain the audio sessions of a slot batch. Per slot: ``samples`` received so far (None: the slot takes no
    part), ``emitted`` frames already pushed, ``ended`` whether its audio has stopped. A slot is ready with at least ``group`` frames
    available (audio_frames_available) and not emitted, an ended slot while any frame remains. One step takes the ready slots and
    pushes F = group*k frames, k the smallest count among them (a live slot counts its complete groups, an ended one
    ceil(remaining / group)); an ended slot's mel_lens entry is min(remaining, F), the other ready slots' F, the rest are inactive.
    Steps repeat until no slot is ready. -> (steps = [(F, active [B] bools, mel_lens [B] ints)], emitted after the steps [B])."""
    g, B = int(group), len(samples)
    if g < 1:
        raise ValueError(f"group must be >= 1, got {group}")
    done = list(emitted)
    avail = [0 if samples[b] is None else audio_frames_available(samples[b], ended[b], hop, pad) for b in range(B)]
    steps = []
    while True:
        rem = [0 if samples[b] is None else avail[b] - done[b] for b in range(B)]
        ready = [rem[b] >= g or (bool(ended[b]) and rem[b] > 0) for b in range(B)]
        if not any(ready):
            return steps, done
        F = g * min(-(-rem[b] // g) if ended[b] else rem[b] // g for b in range(B) if ready[b])
        lens = [(min(rem[b], F) if ended[b] else F) if ready[b] else 0 for b in range(B)]
        steps.append((F, ready, lens))
        done = [done[b] + lens[b] for b in range(B)]


class _SlotFrames(int):
    """encoder_frames in slot mode: the largest offset as an int, and called with a slot that slot's frames."""

    def __new__(cls, offsets):
        obj = super().__new__(cls, max(offsets) if offsets else 0)
        obj.offsets = tuple(offsets)
        return obj

    def __call__(self, slot):
        return self.offsets[slot]


def _enc_frames(mel):
    return (mel + 3) // 4 if isinstance(mel, int) else torch.div(torch.div(mel + 1, 2, rounding_mode="floor") + 1, 2, rounding_mode="floor")


class StreamingTranscriber:
    """Streams of one causal model; see the module docstring. Side effect while a stream is open (bf16 compute): from start() to
    finish() every fp32 weight matrix of the front-end, the encoder and encoder_proj that has no bf16 copy carries one (``p._bf16``,
    valid while ``p._version`` is unchanged; the copy the training step's gradient arena keeps, so that a push does not cast its
    weights again). That is one bf16 copy of those matrices in memory; do not change the weights in place (``p.data``) while a stream
    is open. finish() removes the copies."""

    def __init__(self, brain, search="greedy"):
        if search not in ("greedy", "beam"):
            raise ValueError(f"StreamingTranscriber: search must be 'greedy' or 'beam', got {search!r}")
        m = brain.modules
        enc, fe = m["encoder"] if isinstance(m, dict) else m.encoder, m["frontend"] if isinstance(m, dict) else m.frontend
        if not getattr(enc, "causal", False):
            raise ValueError("StreamingTranscriber needs a causal encoder (causal_encoder: True); this model looks at future frames")
        pads = {getattr(fe, f"convblock_{i}").padding for i in range(fe.num_blocks)}
        if pads != {"causal"}:
            raise ValueError(f"StreamingTranscriber needs frontend_padding: causal (the front-end pads with {sorted(pads)})")
        self.brain, self.encoder, self.frontend = brain, enc, fe
        self.encoder_proj = m["encoder_proj"] if isinstance(m, dict) else m.encoder_proj
        hp = brain.hparams
        name = "greedy_searcher" if search == "greedy" else "beam_searcher"
        self.search = search
        self.searcher = hp[name] if isinstance(hp, dict) else getattr(hp, name)
        self._started = False
        self._copies = []

    # ------------------------------------------------------------------------------------------------------------------------------
    def start(self, batch_size, max_frames, enroll=None, speaker_embs=None, speaker_embs_length=None, keep_encoder_out=False, timestamps=False,
              audio=False, feature_prior=None, slots=False, max_speaker_frames=1, max_audio_samples=32000, keep_features=False, bias=None):
        """Begin B streams of at most ``max_frames`` encoder frames (4 mel frames each). The speaker embedding is computed once here:
        ``enroll`` = (enrollment signals or features, relative lengths) through the recipe's own speaker branch, or given directly as
        ``speaker_embs`` (+ ``speaker_embs_length`` for cross-attention); neither = no injection (variant none). keep_encoder_out: keep
        every chunk's encoder output (before encoder_proj) for encoder_out(). timestamps: keep the emission frame of every token
        (frames(), nbest_frames()). audio: the stream is fed waveforms (push_audio) - causal features over the recipe's Fbank tables,
        ``feature_prior`` = (mean [n_mels], std [n_mels], n0) optionally starting their running statistics (nnet.CausalFeatures).
        slots: the B rows are slots, all free to begin with, that sessions enter with admit() and leave with release() (module
        docstring); the speaker embedding then comes per session with admit(), padded to ``max_speaker_frames`` rows. Slot sessions
        admitted with audio=True are fed with push_audio(): ``max_audio_samples`` is the most samples one call may carry per slot (it
        sizes the sample rings, which the first such admit() allocates); keep_features keeps their feature frames for features_out().
        bias (search="beam"; biasing.py): the streams' phrase graphs, one ContextGraph for all or a list of B entries (a graph or
        None). start(slots=True, bias=True) reserves the biased search layout; each session then names its graph with
        admit(slot, ..., bias=graph or None). Greedy search is not biased: ValueError."""
        if torch.is_grad_enabled():
            raise RuntimeError("StreamingTranscriber is inference only: run it under torch.no_grad()")
        if bias is not None and bias is not False and self.search != "beam":
            raise ValueError("start(bias=...): contextual biasing needs StreamingTranscriber(brain, search='beam')")
        if slots and not isinstance(bias, bool) and bias is not None:
            raise ValueError("start(slots=True): bias=True reserves the biased search; the graphs come per session, with admit(slot, bias=...)")
        if not slots and isinstance(bias, bool):
            raise ValueError("start(bias=True/False) goes with slots=True; give the streams' graph(s) otherwise")
        if bias is None or bias is False:
            self.bias_graphs = None
        elif slots:
            self.bias_graphs = [None] * int(batch_size)
        else:
            from .biasing import as_list
            self.searcher._check_bias(bias)
            self.bias_graphs = as_list(bias, int(batch_size))
        if slots and (enroll is not None or speaker_embs is not None):
            raise ValueError("start(slots=True): the speaker embedding comes per session, with admit(slot, enroll=... / speaker_embs=...)")
        if slots and audio:
            raise ValueError("start(slots=True, audio=True): in slot mode a session, not the batch, is fed audio: start(slots=True) and "
                             "admit(slot, ..., audio=True)")
        if hasattr(self.brain, "_setup_dtype"):      # the brain's compute dtype (as fit / evaluate set it)
            self.brain._setup_dtype()
        for mod in (self.frontend, self.encoder, self.encoder_proj, self.searcher):
            mod.eval()
        from .nnet import compute_dtype
        if compute_dtype() == torch.bfloat16:
            # bf16 copies of the matrices, kept beside the weights as the training step's gradient arena keeps them (ops._bf16_weight
            # takes them while the weight's version is unchanged): without them every GEMM of every push casts its weight again.
            # A weight that already has a copy (the arena's view into its flat shadow) is left alone; finish() removes the copies.
            self._drop_copies()
            for mod in (self.frontend, self.encoder, self.encoder_proj):
                for p in mod.parameters():
                    if p.dim() >= 2 and p.is_cuda and p.dtype == torch.float32 and getattr(p, "_bf16", None) is None:
                        p._bf16 = p.detach().to(torch.bfloat16).contiguous()
                        p._bf16_ver = p._version
                        self._copies.append((p, p._bf16))
        if enroll is not None:
            sig, lens = enroll
            batch = types.SimpleNamespace(enroll_sig=(sig, lens))
            for name in ("speaker_frontend", "speaker_encoder", "speaker_proj"):
                mods = self.brain.modules
                if (name in mods) if isinstance(mods, dict) else hasattr(mods, name):
                    (mods[name] if isinstance(mods, dict) else getattr(mods, name)).eval()
            speaker_embs, speaker_embs_length = self.brain._speaker_embedding(batch, 0)
        self.B, self.max_frames = int(batch_size), int(max_frames)
        self.spk, self.spk_len = speaker_embs, speaker_embs_length
        self.enc_state = None                    # allocated by the first push (after its arguments are checked)
        self.fe_state, self.search_state = None, None
        self.mel = None
        self.hyps = [[] for _ in range(self.B)]
        self.timestamps = bool(timestamps)
        self.hyp_frames = [[] for _ in range(self.B)]
        self.closed = False
        self.keep = bool(keep_encoder_out)
        self.enc_chunks = []
        self.features, self.feat_state = None, None
        if audio:
            from .nnet import CausalFeatures
            mods = self.brain.modules
            fbank = mods["feature_extractor"] if isinstance(mods, dict) else mods.feature_extractor
            self.features = CausalFeatures(fbank, prior=feature_prior).to(fbank.window.device)
        elif feature_prior is not None:
            raise ValueError("feature_prior goes with audio=True")
        self.slots = bool(slots)
        if self.slots:
            self.max_speaker_frames = int(max_speaker_frames)
            self.occupied = [False] * self.B
            self.slot_chunks = [[] for _ in range(self.B)]
            if int(max_audio_samples) < 1:
                raise ValueError(f"start(): max_audio_samples must be >= 1, got {max_audio_samples}")
            self.max_audio_samples, self.keep_feats = int(max_audio_samples), bool(keep_features)
            self.feat_slots = None                   # sample rings + normaliser rows: allocated by the first admit(..., audio=True)
            self.audio_slot = [False] * self.B       # per slot: its session is fed audio; samples received; frames pushed; audio ended
            self.a_have, self.a_emit, self.a_end = [0] * self.B, [0] * self.B, [False] * self.B
            self.feat_chunks = [[] for _ in range(self.B)]
            self.audio_steps = []
            dev = self.encoder.norm.norm.weight.device
            self.enc_state = self.encoder.init_stream(self.B, self.max_frames, device=dev, slots=True)
            self.mel = torch.zeros(self.B, dtype=torch.int64, device=dev)
        self._started = True
        return self

    # ---- slots ---------------------------------------------------------------------------------------------------------------------
    def _need_slots(self, what, slot=None):
        if not self._started or not getattr(self, "slots", False):
            raise RuntimeError(f"{what} needs start(..., slots=True)")
        if slot is not None and not 0 <= int(slot) < self.B:
            raise ValueError(f"{what}: slot {slot} is not one of the {self.B} slots")

    def admit(self, slot, enroll=None, speaker_embs=None, speaker_embs_length=None, audio=False, feature_prior=None, bias=None):
        """A new session enters the free ``slot``. Its speaker embedding: ``enroll`` = (one enrollment signal [1, N], its relative
        length [1]) through the recipe's speaker branch, or ``speaker_embs`` [1, S, D] (+ ``speaker_embs_length`` [1] relative, for
        cross-attention), S <= max_speaker_frames; neither = no injection. Reset for this slot only: offset and mel count, the
        front-end carries, both conv histories of every layer, the search state, the hypothesis, its frames and the kept encoder
        output. The K/V cache keeps its bytes: rows at or past a slot's offset are never read. audio: the session is fed waveform
        (push_audio) instead of features; also reset for this slot are then its sample and emitted-frame counts, its ended flag and its
        row of the normaliser's state (zeros, or ``feature_prior`` = (mean [n_mels], std [n_mels], n0) as ops.running_norm_state writes
        it). The sample ring keeps its bytes: samples a session has not received are never read. bias (start(slots=True,
        bias=True)): the session's phrase graph (None: the session is not biased); the graphs of the other slots stay as they are."""
        self._need_slots("admit()", slot)
        if bias is not None:
            if self.bias_graphs is None:
                raise ValueError("admit(bias=...) needs start(..., slots=True, bias=True)")
            self.searcher._check_bias(bias)
            if not hasattr(bias, "step"):
                raise ValueError("admit(bias=...): one session's graph is a biasing.ContextGraph or None")
        if torch.is_grad_enabled():
            raise RuntimeError("StreamingTranscriber is inference only: run it under torch.no_grad()")
        slot = int(slot)
        if self.occupied[slot]:
            raise ValueError(f"admit(): slot {slot} is occupied; release() it first")
        if enroll is not None and speaker_embs is not None:
            raise ValueError("admit(): give enroll or speaker_embs, not both")
        if feature_prior is not None and not audio:
            raise ValueError("admit(): feature_prior goes with audio=True")
        if enroll is not None:
            sig, lens = enroll
            batch = types.SimpleNamespace(enroll_sig=(sig, lens))
            mods = self.brain.modules
            for name in ("speaker_frontend", "speaker_encoder", "speaker_proj"):
                if (name in mods) if isinstance(mods, dict) else hasattr(mods, name):
                    (mods[name] if isinstance(mods, dict) else getattr(mods, name)).eval()
            speaker_embs, speaker_embs_length = self.brain._speaker_embedding(batch, 0)
        if speaker_embs is not None:
            S, Sm = speaker_embs.shape[-2], self.max_speaker_frames
            if speaker_embs.ndim != 3 or speaker_embs.shape[0] != 1 or S > Sm:
                raise ValueError(f"admit(): one session's embedding is [1, S <= {Sm}, D], got {tuple(speaker_embs.shape)}")
            dev = self.mel.device
            if self.spk is None:
                self.spk = torch.zeros(self.B, Sm, speaker_embs.shape[-1], dtype=speaker_embs.dtype, device=dev)
                self.spk_len = torch.ones(self.B, dtype=torch.float32, device=dev)
            n = S if speaker_embs_length is None else int(torch.round(torch.as_tensor(speaker_embs_length).float().reshape(-1)[0] * S))
            self.spk[slot] = 0
            self.spk[slot, :S] = speaker_embs[0].to(device=dev, dtype=self.spk.dtype)
            self.spk_len[slot] = min(max(n, 1), S) / Sm
        elif self.spk is not None:
            self.spk[slot] = 0
            self.spk_len[slot] = 1.0
        es = self.enc_state
        es["t0"][slot] = 0
        es["t0s"][slot] = 0
        self.mel[slot] = 0
        if self.fe_state is not None:
            for carry in self.fe_state:
                carry[slot] = 0
        for layer in es["layers"]:
            for hist in layer["hist"]:
                hist[slot] = 0
        self.searcher.reset_streams(self.search_state, [slot])
        if self.bias_graphs is not None:                 # the search learns the slot's new graph with the next push
            self.bias_graphs[slot] = None if bias is None or bias.empty else bias
        self.hyps[slot], self.hyp_frames[slot], self.slot_chunks[slot] = [], [], []
        if audio:
            if self.features is None:
                from .nnet import CausalFeatures
                mods = self.brain.modules
                fbank = mods["feature_extractor"] if isinstance(mods, dict) else mods.feature_extractor
                self.features = CausalFeatures(fbank).to(fbank.window.device)
                self.audio_group = 4 * max(int(getattr(self.encoder.layers[0], "chunk_size", 0) or 0), 1)
                cap = audio_ring_capacity(self.max_audio_samples, self.audio_group, self.features.hop, self.features.pad)
                self.feat_slots = self.features.init_slots(self.B, cap, fbank.window.device)
            self.features.reset_slot(self.feat_slots, slot, feature_prior)
        self.audio_slot[slot] = bool(audio)
        self.a_have[slot], self.a_emit[slot], self.a_end[slot], self.feat_chunks[slot] = 0, 0, False, []
        self.occupied[slot] = True
        return self

    def release(self, slot):
        """The session in ``slot`` leaves: returns its hypothesis (what finish() would give for that row) and frees the slot. With beam
        search nbest() / nbest_frames() still describe the session until the slot is admitted again."""
        self._need_slots("release()", slot)
        slot = int(slot)
        if not self.occupied[slot]:
            raise ValueError(f"release(): slot {slot} is free")
        self.occupied[slot] = False
        self.audio_slot[slot] = False                # (samples of an audio session that were still pending are dropped)
        return list(self.hyps[slot])

    def _push_slots(self, feats, mel_lens, enc_lens, active, last, from_audio=False):
        B, F = self.B, feats.shape[1]
        if active is None:                               # (with no audio session: the occupied slots)
            act = [o and not a for o, a in zip(self.occupied, self.audio_slot)]
        else:
            act = [bool(a) for a in (active.tolist() if isinstance(active, torch.Tensor) else active)]
        if len(act) != B:
            raise ValueError(f"active must name {B} slots, got {len(act)}")
        free = [b for b in range(B) if act[b] and not self.occupied[b]]
        if free:
            raise ValueError(f"push(): slot(s) {free} are free; admit() a session before pushing to them")
        fed = [b for b in range(B) if act[b] and self.audio_slot[b]]
        if fed and not from_audio:
            raise ValueError(f"push(): the session(s) in slot(s) {fed} are fed audio (admit(..., audio=True)): push_audio() computes their features")
        if F == 0 or not any(act):
            return [list(h) for h in self.hyps] if self.search == "beam" else [[] for _ in range(B)]
        es, Cn = self.enc_state, _enc_frames(F)
        for b in range(B):                               # checked before any state of any slot moves
            if act[b] and es["t0"][b] + Cn > self.max_frames:
                raise ValueError(f"the push would take slot {b} past start()'s max_frames: {es['t0'][b]} + {Cn} > {self.max_frames} encoder frames")
        C.require_gpu(feats)
        dev = feats.device
        act_dev = torch.tensor(act, dtype=torch.bool, device=dev)
        ml = torch.full((B,), F, dtype=torch.int64, device=dev) if mel_lens is None else torch.as_tensor(mel_lens, device=dev).long()
        self.mel = self.mel + ml.clamp(0, F) * act_dev
        valid = _enc_frames(self.mel) if enc_lens is None else torch.as_tensor(enc_lens, device=dev).long()
        t0 = es["t0s"].clone().long()                    # each slot's offset before this push
        x, fe = self.frontend.forward_chunk(feats, self.fe_state)
        keep = act_dev.view(B, 1, 1, 1)                  # an idle slot keeps its carry (zeros before its first push)
        self.fe_state = [torch.where(keep, new, torch.zeros_like(new) if self.fe_state is None else self.fe_state[i]) for i, new in enumerate(fe)]
        e = self.encoder.forward_chunk(x, es, self.spk, self.spk_len, enc_lens=valid.to(torch.int32), active=act)
        if self.keep:
            for b in range(B):
                if act[b]:
                    self.slot_chunks[b].append(e[b])
        e = self.encoder_proj(e)
        n_valid = ((valid - t0).clamp(0, e.shape[1]) * act_dev).to(torch.int32)
        self.closed = bool(last)
        if self.search == "beam":
            best, self.search_state = self.searcher.beam_stream(e, self.search_state, n_valid, max_frames=self.max_frames,
                                                                return_frames=self.timestamps, raise_stopped=False, bias=self.bias_graphs)
            self.hyps = [list(h) for h in best]
            if self.timestamps:
                self.hyp_frames = [list(f[0]) for f in self.search_state["frames"]]
            stopped = {b: why for b, why in self.search_state.get("stopped", {}).items() if self.occupied[b]}
            if stopped:                                  # every slot's state is stored; the others continue with the next push
                raise RuntimeError(f"beam_stream: slot(s) {sorted(stopped)} stopped ({sorted(set(stopped.values()))}) with "
                                   f"cap={self.searcher.cap} hypotheses per frame and max_frames={self.max_frames}; release() and admit() "
                                   f"them to run again (a larger cap or max_frames needs a new start())")
            return best
        if self.timestamps:
            new, new_frames, self.search_state = self.searcher.greedy_stream(e, self.search_state, n_valid, return_frames=True)
            for b, fr in enumerate(new_frames):
                self.hyp_frames[b].extend(fr)
        else:
            new, self.search_state = self.searcher.greedy_stream(e, self.search_state, n_valid)
        for b, toks in enumerate(new):
            self.hyps[b].extend(toks)
        return new

    def _push_audio_slots(self, wav, wav_lens, active, end):
        """push_audio() in slot mode: every check first, then one append for the batch, then the planned steps."""
        B = self.B
        if self.features is None:
            raise RuntimeError("push_audio() needs an audio session: admit(slot, ..., audio=True)")
        if wav.ndim != 2 or wav.shape[0] != B:
            raise ValueError(f"wav must be [B={B}, N], got {tuple(wav.shape)}")
        N = wav.shape[1]
        if N > self.max_audio_samples:
            raise ValueError(f"push_audio(): {N} samples per slot is more than start()'s max_audio_samples={self.max_audio_samples}")
        hop, pad, g = self.features.hop, self.features.pad, self.audio_group
        have, emit, ended = self.a_have, self.a_emit, self.a_end
        left = [audio_frames_available(have[b], ended[b], hop, pad) - emit[b] for b in range(B)]
        flags = lambda x: [bool(v) for v in (x.tolist() if isinstance(x, torch.Tensor) else x)]  # noqa: E731
        if active is None:                               # the audio sessions that go on, and ended ones a stopped call left undrained
            act = [self.occupied[b] and self.audio_slot[b] and (not ended[b] or left[b] > 0) for b in range(B)]
        else:
            act = flags(active)
            if len(act) != B:
                raise ValueError(f"active must name {B} slots, got {len(act)}")
            for b in range(B):
                if act[b] and not self.occupied[b]:
                    raise ValueError(f"push_audio(): slot {b} is free; admit() a session before pushing to it")
                if act[b] and not self.audio_slot[b]:
                    raise ValueError(f"push_audio(): the session in slot {b} is fed features (push()); admit(..., audio=True) for audio")
                if act[b] and ended[b] and left[b] <= 0:
                    raise ValueError(f"push_audio(): the audio of the session in slot {b} has ended; release() it")
        stop = [False] * B if end is None else flags(end)
        if len(stop) != B or any(s and not a for s, a in zip(stop, act)):
            raise ValueError(f"end must name slots among the {B} that are active in this call, got {stop}")
        if wav_lens is None:
            lens = [N if act[b] and not ended[b] else 0 for b in range(B)]
        else:
            lens = [int(v) for v in torch.as_tensor(wav_lens).reshape(-1).tolist()]
            if len(lens) != B or any(v < 0 or v > N for v in lens):
                raise ValueError(f"wav_lens must hold B={B} counts in [0, {N}], got {lens}")
            lens = [v if act[b] else 0 for b, v in enumerate(lens)]
            late = [b for b in range(B) if ended[b] and lens[b]]
            if late:
                raise ValueError(f"push_audio(): the audio of slot(s) {late} has ended: they carry 0 samples")
        cap = self.feat_slots["ring"].shape[1]
        for b in range(B):                               # (audio_ring_capacity: only a call that a stopped beam stream cut short leaves this much)
            if lens[b] and _ring_needed(have[b] + lens[b], emit[b], hop, pad) > cap:
                raise ValueError(f"push_audio(): slot {b} holds {_ring_needed(have[b], emit[b], hop, pad)} samples that are not pushed yet; "
                                 f"{lens[b]} more do not fit its ring of {cap}: drain it with a call that carries 0 samples")
            if have[b] + lens[b] >= 2 ** 31:
                raise ValueError(f"push_audio(): slot {b} would pass 2^31 samples")
        new_have = [have[b] + lens[b] for b in range(B)]
        new_end = [ended[b] or stop[b] for b in range(B)]
        steps, _ = plan_audio_steps([new_have[b] if act[b] else None for b in range(B)], emit, new_end, g, hop, pad)
        t0 = self.enc_state["t0"]
        for b in range(B):
            grow = sum(_enc_frames(F) for F, on, _ in steps if on[b])
            if t0[b] + grow > self.max_frames:
                raise ValueError(f"the push would take slot {b} past start()'s max_frames: {t0[b]} + {grow} > {self.max_frames} encoder frames")
        if any(lens):
            C.require_gpu(wav)
        # ---- checked: from here on the state moves
        dev = self.feat_slots["ring"].device
        if any(lens):
            w = wav.detach()
            if w.dtype != torch.float32:
                w = w.float()
            if N > 1 and w.stride(1) != 1:
                w = w.contiguous()
            self.features.append_slots(self.feat_slots, w, torch.tensor([[h % cap for h in have], lens], dtype=torch.int32, device=dev))
        self.a_have, self.a_end = new_have, new_end
        out = [[] for _ in range(B)]
        best = None
        for F, on, ml in steps:
            tbl = torch.tensor([self.a_emit, ml, new_have], dtype=torch.int32, device=dev)
            feats = self.features.frames_slots(self.feat_slots, tbl, F)
            for b in range(B):
                if on[b] and ml[b] < F:                  # the padded tail of an ended session's last group: zeros
                    feats[b, ml[b]:] = 0
                if on[b] and self.keep_feats:
                    self.feat_chunks[b].append(feats[b, :ml[b]])
            # the step's frames are computed and the normaliser has moved: it counts, even if a beam stream stops in it (RuntimeError
            # after every slot's state is stored; the later steps' samples stay in the rings and the next call drains them)
            self.a_emit = [e + m for e, m in zip(self.a_emit, ml)]
            self.audio_steps.append((F, list(on), list(ml)))
            best = self._push_slots(feats, tbl[1], None, on, False, from_audio=True)
            if self.search != "beam":
                for b, toks in enumerate(best):
                    out[b].extend(toks)
        if self.search == "beam":
            return best if best is not None else [list(h) for h in self.hyps]
        return out

    def features_out(self, slot):
        """start(slots=True, keep_features=True): [frames so far, n_mels], the normalised feature frames the audio session in ``slot``
        has been given (the bits nnet.CausalFeatures.forward computes for its audio alone)."""
        self._need_slots("features_out(slot)", slot)
        if not self.keep_feats:
            raise RuntimeError("features_out() needs start(..., keep_features=True)")
        chunks = self.feat_chunks[int(slot)]
        mods = self.brain.modules
        n_mels = (mods["feature_extractor"] if isinstance(mods, dict) else mods.feature_extractor).n_mels
        return torch.cat(chunks, dim=0) if chunks else torch.empty(0, n_mels, device=self.mel.device)

    def push_audio(self, wav, wav_lens=None, last=False, active=None, end=None):
        """start(..., audio=True): feed the next N samples of every stream, wav [B, N], any N. wav_lens [B]: valid samples of this push per
        stream (default N; fewer ends that stream, whose later pushes carry 0). The frames whose samples have arrived are computed in
        whole groups of 4 (4 x attention_chunk_size with block-causal attention) and pushed; the rest waits for the next push, every
        remaining frame goes with the ``last`` one. Returns what push() returns (for no frames when no group is complete yet). A push that
        raises (bad wav_lens, past max_frames) leaves the stream, its buffered samples and running statistics included, as it was.
        start(slots=True): feeds the sessions admitted with audio=True. wav_lens [B]: this call's samples per slot, 0 .. N <=
        max_audio_samples (default N for the active slots); ``active`` (bool per slot): the sessions this call belongs to, default the
        occupied audio sessions whose audio has not ended - a free slot, a feature-fed session or an ended one raises ValueError; ``end``
        (bool per slot): sessions whose audio stops with this call. The samples are appended to the slots' rings, then the steps
        plan_audio_steps gives are pushed, each through the slot push(); an ended session's last frames go out as a group padded with
        zeros and a short mel_lens. Returns per slot the concatenation of its steps' symbols (greedy) or its best hypothesis (beam).
        Every check runs before anything moves (a plan that would take a slot past max_frames included). A beam stream that stops
        raises RuntimeError as push() does after that step; the later steps wait for the next call."""
        if not self._started:
            raise RuntimeError("push_audio() before start()")
        if getattr(self, "slots", False):
            if self.closed:
                raise RuntimeError("push_audio() after the last push of the stream")
            if torch.is_grad_enabled():
                raise RuntimeError("StreamingTranscriber is inference only: run it under torch.no_grad()")
            if last:
                raise ValueError("push_audio(last=True) belongs to lockstep streams; a slot session's audio stops with end=[...]")
            return self._push_audio_slots(wav, wav_lens, active, end)
        if active is not None or end is not None:
            raise ValueError("push_audio(active=..., end=...) needs start(..., slots=True)")
        if self.features is None:
            raise RuntimeError("push_audio() needs start(..., audio=True)")
        if self.closed:
            raise RuntimeError("push_audio() after the last push of the stream")
        if torch.is_grad_enabled():
            raise RuntimeError("StreamingTranscriber is inference only: run it under torch.no_grad()")
        if wav.ndim != 2 or wav.shape[0] != self.B:
            raise ValueError(f"wav must be [B={self.B}, N], got {tuple(wav.shape)}")
        if self.feat_state is None:
            self.feat_state = self.features.init_stream(self.B, wav.device)
        blk = max(int(getattr(self.encoder.layers[0], "chunk_size", 0) or 0), 1)
        # forward_chunk moves the feature state (in place; the normaliser's sums on the device) before push() has checked its own
        # arguments (max_frames): keep what a refused push must find again
        fs = self.feat_state
        saved = dict(fs, norm=fs["norm"].clone(), valid=list(fs["valid"]))
        feats, n_valid, self.feat_state = self.features.forward_chunk(wav, fs, wav_lens=wav_lens, last=last, group=4 * blk)
        try:
            return self.push(feats, mel_lens=n_valid, last=last)
        except Exception:
            self.feat_state = saved
            raise

    def push(self, feats, mel_lens=None, enc_lens=None, active=None, last=False):
        """Feed the next F feature frames of every stream, feats [B, F, 80]; F must be a multiple of 4 unless ``last`` (no push may
        follow a last one). mel_lens [B]: valid frames of this push per stream (default F); enc_lens [B]: absolute valid encoder frames
        after this push (default ceil(ceil(L/2)/2) of the mel frames pushed so far). Returns the new symbols of each stream.
        start(slots=True): ``active`` (bool per slot, default the occupied slots whose sessions are fed features) names the slots this
        push belongs to; an occupied slot left out is paused, a session fed audio (admit(..., audio=True)) raises ValueError. A slot that is not active keeps every piece of its state bit for bit and returns [] (greedy) or its
        current hypothesis (beam); mel_lens / enc_lens count in each slot's own session. A push that would take a slot past max_frames
        raises ValueError naming the slot before any state moves; a beam stream that stops raises RuntimeError naming the slots after
        every slot's state has been stored."""
        if not self._started:
            raise RuntimeError("push() before start()")
        if self.closed:
            raise RuntimeError("push() after the last push of the stream")
        if torch.is_grad_enabled():
            raise RuntimeError("StreamingTranscriber is inference only: run it under torch.no_grad()")
        if feats.ndim != 3 or feats.shape[0] != self.B:
            raise ValueError(f"feats must be [B={self.B}, F, n_mels], got {tuple(feats.shape)}")
        F = feats.shape[1]
        if F % 4 and not last:
            raise ValueError(f"a push carries a multiple of 4 feature frames (one encoder frame per 4) except the last one: got {F}")
        blk = max(int(getattr(self.encoder.layers[0], "chunk_size", 0) or 0), 1)
        if (F // 4) % blk and not last:
            raise ValueError(f"with block-causal attention over {blk} frames a push carries a multiple of {4 * blk} feature frames "
                             f"except the last one: got {F}")
        if getattr(self, "slots", False):
            return self._push_slots(feats, mel_lens, enc_lens, active, last)
        if active is not None:
            raise ValueError("push(active=...) needs start(..., slots=True)")
        if F == 0:
            return [list(h) for h in self.hyps] if self.search == "beam" else [[] for _ in range(self.B)]
        t_done = 0 if self.enc_state is None else self.enc_state["t0"]
        if t_done + _enc_frames(F) > self.max_frames:      # checked before any state of the stream moves
            raise ValueError(f"the push would take the stream past start()'s max_frames: {t_done} + {_enc_frames(F)} > {self.max_frames} encoder frames")
        C.require_gpu(feats)
        dev = feats.device
        if self.enc_state is None:
            self.enc_state = self.encoder.init_stream(self.B, self.max_frames, device=dev)
            self.mel = torch.zeros(self.B, dtype=torch.int64, device=dev)
        ml = torch.full((self.B,), F, dtype=torch.int64, device=dev) if mel_lens is None else torch.as_tensor(mel_lens, device=dev).long()
        self.mel = self.mel + ml.clamp(0, F)
        valid = _enc_frames(self.mel) if enc_lens is None else torch.as_tensor(enc_lens, device=dev).long()
        t0 = self.enc_state["t0"]
        x, self.fe_state = self.frontend.forward_chunk(feats, self.fe_state)
        e = self.encoder.forward_chunk(x, self.enc_state, self.spk, self.spk_len, enc_lens=valid.to(torch.int32))
        if self.keep:
            self.enc_chunks.append(e)
        e = self.encoder_proj(e)
        n_valid = (valid - t0).clamp(0, e.shape[1]).to(torch.int32)
        if self.search == "beam":                 # the best hypothesis so far (its prefix may change with later frames)
            best, self.search_state = self.searcher.beam_stream(e, self.search_state, n_valid, max_frames=self.max_frames,
                                                                return_frames=self.timestamps, bias=self.bias_graphs)
            self.hyps = [list(h) for h in best]
            if self.timestamps:
                self.hyp_frames = [list(f[0]) for f in self.search_state["frames"]]
            self.closed = bool(last)
            return best
        if self.timestamps:
            new, new_frames, self.search_state = self.searcher.greedy_stream(e, self.search_state, n_valid, return_frames=True)
            for b, fr in enumerate(new_frames):
                self.hyp_frames[b].extend(fr)
        else:
            new, self.search_state = self.searcher.greedy_stream(e, self.search_state, n_valid)
        for b, toks in enumerate(new):
            self.hyps[b].extend(toks)
        self.closed = bool(last)
        return new

    def finish(self):
        """The hypotheses (symbol lists) of every stream; the stream is closed and the weights' bf16 copies made by start() are dropped."""
        self.closed = True
        self._drop_copies()
        return [list(h) for h in self.hyps]

    def nbest(self):
        """search="beam": (n-best symbol lists of every stream, their logp / len), best first, as TransducerBeamSearcher returns them."""
        if self.search != "beam":
            raise RuntimeError("nbest() needs StreamingTranscriber(brain, search='beam')")
        if self.search_state is None:
            return [[[]] for _ in range(self.B)], [[0.0] for _ in range(self.B)]
        return [[list(h) for h in n] for n in self.search_state["nbest"]], [list(s) for s in self.search_state["scores"]]

    def frames(self):
        """start(timestamps=True): per stream, the absolute encoder frame that emitted each token of the hypothesis finish() would return
        now. Seconds: frame x align.frame_seconds(hparams); words: align.word_spans(frames, tokens, pieces, frame_seconds)."""
        if not getattr(self, "timestamps", False):
            raise RuntimeError("frames() needs start(..., timestamps=True)")
        return [list(f) for f in self.hyp_frames]

    def nbest_frames(self):
        """start(timestamps=True), search="beam": the emission frames of nbest()'s symbol lists, in the same order."""
        if self.search != "beam":
            raise RuntimeError("nbest_frames() needs StreamingTranscriber(brain, search='beam')")
        if not getattr(self, "timestamps", False):
            raise RuntimeError("nbest_frames() needs start(..., timestamps=True)")
        if self.search_state is None:
            return [[[]] for _ in range(self.B)]
        return [[list(f) for f in n] for n in self.search_state["frames"]]

    def _drop_copies(self):
        for p, copy in self._copies:
            if getattr(p, "_bf16", None) is copy:          # (not replaced since: e.g. by a gradient arena)
                del p._bf16
                if hasattr(p, "_bf16_ver"):
                    del p._bf16_ver
        self._copies = []

    def encoder_out(self, slot=None):
        """[B, frames so far, d_model]: the encoder output of every push (start(keep_encoder_out=True)). start(slots=True):
        encoder_out(slot) = [frames so far, d_model] of the slot's current session."""
        if getattr(self, "slots", False):
            self._need_slots("encoder_out(slot)", slot if slot is not None else -1)
            chunks = self.slot_chunks[int(slot)]
            return torch.cat(chunks, dim=0) if chunks else torch.empty(0, self.encoder.d_model, device=self.mel.device)
        return torch.cat(self.enc_chunks, dim=1)

    @property
    def encoder_frames(self):
        """Encoder frames pushed so far. start(slots=True): encoder_frames(slot) = those of the slot's current session (read as a plain
        number it is the largest over the slots)."""
        if getattr(self, "slots", False):
            return _SlotFrames(self.enc_state["t0"])
        return 0 if self.enc_state is None else self.enc_state["t0"]
