"""Host-side mirror of the reference modules on the TS-ASR hot path.

Every class keeps the reference's constructor arguments, call signature and ``state_dict`` key names/shapes so
that (i) the three hparams YAMLs work with only the ``!new:`` paths re-pointed and (ii) checkpoints written by
the reference load unchanged. What runs underneath is different: tensors stay on the MI355X, lengths stay on
the device (no ``.item()`` / ``.cpu()`` in the step - it must be hipGraph-capturable), activations are kept in
the *compute dtype* (bf16 by default), and the hot operators go through the C-ABI of libtsasr_hip.so
(``ops.py``). Nothing here runs on the CPU: see ``_capi.require_gpu``.

Reference files mirrored (SB = vendor/speechbrain/speechbrain):
  Linear            SB/nnet/linear.py:15-78            Embedding      SB/nnet/embedding.py:14-114
  LSTM              SB/nnet/RNN.py:170-278             LayerNorm      SB/nnet/normalization.py:172-223
  Fbank             SB/lobes/features.py:22-147        InputNormalization SB/processing/features.py:933-1216
  ConvolutionFrontEnd SB/lobes/models/convolution.py:103-266  (Conv2d: SB/nnet/CNN.py:513-739)
  RelPosEncXL / RelPosMHAXL / PositionalwiseFeedForward  SB/nnet/attention.py:312-359 / 362-639 / 778-836
  ConvolutionModule / ConformerEncoderLayer              SB/lobes/models/transformer/Conformer.py:24-115 / 118-260
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import _capi as C
from . import ops

_COMPUTE_DTYPE = torch.bfloat16


def set_compute_dtype(dtype):
    """torch.bfloat16 (default, BASELINE configs[1]) or torch.float32 (parity runs)."""
    global _COMPUTE_DTYPE
    if dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("compute dtype must be torch.bfloat16 or torch.float32")
    _COMPUTE_DTYPE = dtype


def compute_dtype():
    return _COMPUTE_DTYPE


def _cd(x):
    return x if x.dtype == _COMPUTE_DTYPE else x.to(_COMPUTE_DTYPE)


def abs_lengths_round(rel, dim):
    """(rel * dim).round() kept on the device (models/conformer.py:272, SB/nnet/losses.py:58-59): one HIP launch
    (round half to even like torch.round) instead of mul + round + cast."""
    if rel.is_cuda and rel.shape[0] <= 1024:
        return ops.abs_lengths(rel, dim, 0)
    return (rel * dim).round().to(torch.int32)


# ------------------------------------------------------------------------------------------------------
class Linear(nn.Module):
    def __init__(self, n_neurons, input_shape=None, input_size=None, bias=True, combine_dims=False):
        super().__init__()
        self.combine_dims = combine_dims
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size")
        if input_size is None:
            input_size = input_shape[-1]
            if len(input_shape) == 4 and self.combine_dims:
                input_size = input_shape[2] * input_shape[3]
        self.w = nn.Linear(input_size, n_neurons, bias=bias)

    def forward(self, x):
        C.require_gpu(x)
        if x.ndim == 4 and self.combine_dims:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        return ops.linear(_cd(x), self.w.weight, self.w.bias)


class Embedding(nn.Module):
    def __init__(self, num_embeddings, embedding_dim=128, consider_as_one_hot=False, blank_id=0):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.consider_as_one_hot = consider_as_one_hot
        self.embedding_dim = num_embeddings - 1 if consider_as_one_hot else embedding_dim
        self.blank_id = blank_id
        if consider_as_one_hot:
            self.Embedding = nn.Embedding(num_embeddings, self.embedding_dim, padding_idx=blank_id)
            eye = torch.eye(self.embedding_dim)
            with torch.no_grad():
                self.Embedding.weight.zero_()
                self.Embedding.weight[blank_id + 1:] = eye[blank_id:]
                if blank_id != 0:
                    self.Embedding.weight[:blank_id] = eye[:blank_id]
            self.Embedding.weight.requires_grad = False
        else:
            self.Embedding = nn.Embedding(num_embeddings, self.embedding_dim)

    def forward(self, x):
        C.require_gpu(x)
        return _cd(F.embedding(x.long(), self.Embedding.weight))


class LSTM(nn.Module):
    """Predictor network. cuDNN-style packed sequences are replaced by masking: the recurrence runs over the padded
    batch and outputs beyond each length are zeroed, which equals pad_packed_sequence(pack_padded_sequence(..))
    on every valid and padded position (lengths = floor(rel*T), SB/nnet/RNN.py:35) without a host sync."""

    def __init__(self, hidden_size, input_shape=None, input_size=None, num_layers=1, bias=True, dropout=0.0,
                 re_init=True, bidirectional=False):
        super().__init__()
        self.reshape = False
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = int(torch.prod(torch.tensor(input_shape[2:])).item())
        if bidirectional:
            raise NotImplementedError("the TS-ASR predictor is unidirectional")
        self.rnn = nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, dropout=dropout,
                           bidirectional=False, bias=bias, batch_first=True)
        if re_init:
            for name, p in self.rnn.named_parameters():
                if "weight_hh" in name:
                    nn.init.orthogonal_(p)

    def forward(self, x, hx=None, lengths=None):
        C.require_gpu(x)
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        out, hn = ops.lstm(_cd(x), self.rnn, hx)
        if lengths is not None:     # zero the outputs beyond floor(len * T) (pad_packed_sequence's padding): one masking launch each way
            out = ops.mask_time(out, ops.abs_lengths(lengths, x.shape[1], 1))
        return out, hn

    def forward_tokens(self, tokens, embedding, lengths=None):
        """decoder(embedding(tokens), lengths=lengths) for the recipes' predictor (train_librispeechmix_scratch.py:117-119). With the
        frozen one-hot Embedding of the TS-ASR YAMLs and bf16 compute, the embedding lookup and the LSTM's input projection collapse
        into one launch (ops.lstm_onehot: a token selects a column of W_ih); anything else takes the two modules as they are."""
        if (_COMPUTE_DTYPE == torch.bfloat16 and isinstance(embedding, Embedding) and embedding.consider_as_one_hot
                and not embedding.Embedding.weight.requires_grad
                and ops.lstm_onehot_supported(tokens, self.rnn, embedding.num_embeddings)):
            C.require_gpu(tokens)
            out = ops.lstm_onehot(tokens, self.rnn, embedding.blank_id)
            if lengths is not None:
                out = ops.mask_time(out, ops.abs_lengths(lengths, tokens.shape[1], 1))
            return out, None
        return self.forward(embedding(tokens), lengths=lengths)


class LayerNorm(nn.Module):
    def __init__(self, input_size=None, input_shape=None, eps=1e-05, elementwise_affine=True):
        super().__init__()
        self.eps = eps
        if input_shape is not None:
            input_size = input_shape[2:]
        self.norm = nn.LayerNorm(input_size, eps=eps, elementwise_affine=elementwise_affine)

    def forward(self, x):
        return ops.layer_norm(x, self.norm.weight, self.norm.bias, self.eps)


class RNNLM(nn.Module):
    """Recurrent language model (SB/lobes/models/RNNLM.py:15-122): embedding -> dropout -> ``rnn_layers`` recurrent layers -> ``dnn_blocks``
    blocks of Linear, LayerNorm, activation, dropout -> Linear to the vocabulary. Constructor, call and state_dict keys are the
    reference's (embedding.Embedding.weight, rnn.rnn.*, dnn.linear.w.*, dnn.norm.norm.*, out.w.*; the blocks after the first are named
    linear_0, norm_0, ... as the reference's Sequential names repeated layers), so its LM checkpoints load with strict=True. Inference
    and fine-tuning through the existing operators; the transducer beam search fuses it (decoders.TransducerBeamSearcher(lm_module=))."""

    def __init__(self, output_neurons, embedding_dim=128, activation=nn.LeakyReLU, dropout=0.15, rnn_class=LSTM, rnn_layers=2,
                 rnn_neurons=1024, rnn_re_init=False, return_hidden=False, dnn_blocks=1, dnn_neurons=512):
        super().__init__()
        self.embedding = Embedding(num_embeddings=output_neurons, embedding_dim=embedding_dim)
        self.dropout = nn.Dropout(p=dropout)
        self.rnn = rnn_class(input_size=embedding_dim, hidden_size=rnn_neurons, num_layers=rnn_layers, dropout=dropout, re_init=rnn_re_init)
        self.return_hidden = return_hidden
        self.reshape = False
        self.dnn = nn.ModuleDict()
        width = rnn_neurons
        for _ in range(dnn_blocks):
            for name, layer in (("linear", Linear(n_neurons=dnn_neurons, input_size=width, bias=True)), ("norm", LayerNorm(input_size=dnn_neurons)),
                                ("act", activation()), ("dropout", nn.Dropout(p=dropout))):
                if name in self.dnn:                     # the reference's Sequential.append: name, name_0, name_1, ...
                    index = 0
                    while f"{name}_{index}" in self.dnn:
                        index += 1
                    name = f"{name}_{index}"
                self.dnn[name] = layer
            width = dnn_neurons
        self.out = Linear(input_size=dnn_neurons, n_neurons=output_neurons)

    def dnn_layers(self):
        """[(Linear, LayerNorm, activation, Dropout)] of the dnn blocks, in order."""
        layers = list(self.dnn.values())
        return [tuple(layers[i:i + 4]) for i in range(0, len(layers), 4)]

    def _rnn(self, x, hx):
        """The stacked LSTM through the exact-fp32 recurrence kernel, layer by layer (any depth, with or without an initial state:
        hidden = (h, c), each [layers, B, H], as torch's); other recurrent classes are called as they are."""
        rnn = getattr(self.rnn, "rnn", None)
        if not (isinstance(self.rnn, LSTM) and ops.LSTM_F32_HIP and rnn.hidden_size <= 1024 and x.is_cuda):
            return self.rnn(x, hx=hx)
        hs, cs = [], []
        y = x.float()
        for l in range(rnn.num_layers):
            w_ih, w_hh = getattr(rnn, f"weight_ih_l{l}"), getattr(rnn, f"weight_hh_l{l}")
            b_ih, b_hh = (getattr(rnn, f"bias_ih_l{l}"), getattr(rnn, f"bias_hh_l{l}")) if rnn.bias else (None, None)
            h0, c0 = (None, None) if hx is None else (hx[0][l], hx[1][l])
            y, hn, cn = ops._LstmF32Fn.apply(y, w_ih, w_hh, b_ih, b_hh, h0, c0, torch.is_grad_enabled())
            if self.training and rnn.dropout > 0 and l + 1 < rnn.num_layers:
                y = F.dropout(y, rnn.dropout, True)
            hs.append(hn)
            cs.append(cn)
        return y.to(x.dtype), (torch.stack(hs), torch.stack(cs))

    def forward(self, x, hx=None):
        x = self.dropout(self.embedding(x))
        if x.dim() == 2:                                 # inference: add the time axis (the flag stays set, as in the reference)
            x = x.unsqueeze(1)
            self.reshape = True
        x, hidden = self._rnn(x, hx)
        for linear, norm, act, drop in self.dnn_layers():
            x = linear(x)
            if norm.norm.weight.numel() % 8:             # (the row kernels take widths that are multiples of 8)
                ops.lib_fallback("layer_norm", f"width {norm.norm.weight.numel()} is no multiple of 8")
                x = drop(act(F.layer_norm(x.float(), norm.norm.normalized_shape, norm.norm.weight, norm.norm.bias, norm.eps))).to(x.dtype)
            elif isinstance(act, nn.LeakyReLU):          # LayerNorm and the LeakyReLU behind it: one launch
                x = drop(ops.layer_norm(x, norm.norm.weight, norm.norm.bias, norm.eps, act_slope=act.negative_slope))
            else:
                x = drop(act(norm(x)))
        out = self.out(x)
        if self.reshape:
            out = out.squeeze(1)
        return (out, hidden) if self.return_hidden else out


# ------------------------------------------------------------------------------------------------------
# A1 / A2 features
# ------------------------------------------------------------------------------------------------------
class Fbank(nn.Module):
    def __init__(self, deltas=False, context=False, requires_grad=False, sample_rate=16000, f_min=0, f_max=None,
                 n_fft=400, n_mels=40, filter_shape="triangular", param_change_factor=1.0, param_rand_factor=0.0,
                 left_frames=5, right_frames=5, win_length=25, hop_length=10):
        super().__init__()
        if deltas or context or requires_grad or filter_shape != "triangular" or param_rand_factor != 0.0:
            raise NotImplementedError("ts-asr_amd.Fbank implements the configuration the TS-ASR recipes use "
                                      "(frozen triangular filters, no deltas/context)")
        self.sample_rate, self.n_fft, self.n_mels = sample_rate, n_fft, n_mels
        self.f_min, self.f_max = f_min, sample_rate / 2 if f_max is None else f_max
        self.win_length = int(round(sample_rate / 1000.0 * win_length))
        self.hop_length = int(round(sample_rate / 1000.0 * hop_length))
        self.top_db, self.amin = 80.0, 1e-10
        # fixed tables: built once on the host (the reference rebuilds the filter matrix on every call)
        self.register_buffer("window", torch.hamming_window(self.win_length), persistent=False)
        self.register_buffer("fbank_matrix", _mel_matrix(n_mels, n_fft, sample_rate, self.f_min, self.f_max), persistent=False)

    def forward(self, wav):
        C.require_gpu(wav)
        return ops.fbank(wav.float(), self.window, self.fbank_matrix, self.n_fft, self.hop_length, self.win_length,
                         self.top_db, self.amin)


def _mel_matrix(n_mels, n_fft, sample_rate, f_min, f_max):
    mel_lo = 2595.0 * math.log10(1.0 + f_min / 700.0)
    mel_hi = 2595.0 * math.log10(1.0 + f_max / 700.0)
    hz = 700.0 * (10.0 ** (torch.linspace(mel_lo, mel_hi, n_mels + 2) / 2595.0) - 1.0)
    band, centre = (hz[1:] - hz[:-1])[:-1], hz[1:-1]
    freqs = torch.linspace(0, sample_rate // 2, n_fft // 2 + 1)
    slope = (freqs[None, :] - centre[:, None]) / band[:, None]
    return torch.clamp(torch.minimum(slope + 1.0, 1.0 - slope), min=0.0).t().contiguous()  # [n_fft/2+1, n_mels]


class InputNormalization(nn.Module):
    def __init__(self, mean_norm=True, std_norm=True, norm_type="global", avg_factor=None, requires_grad=False,
                 update_until_epoch=3):
        super().__init__()
        if norm_type != "sentence" or not mean_norm or not std_norm:
            raise NotImplementedError("ts-asr_amd.InputNormalization implements norm_type='sentence' (all TS-ASR YAMLs)")
        self.norm_type, self.eps, self.update_until_epoch = norm_type, 1e-10, update_until_epoch

    def forward(self, x, lengths, spk_ids=None, epoch=0):
        C.require_gpu(x, lengths)
        return ops.sentence_norm(x, abs_lengths_round(lengths, x.shape[1]), self.eps)


class CausalFeatures(nn.Module):
    """Causal log-mel features with a running floor and running normalisation (build extension; the reference has no such mode): what a
    live stream can compute, and what a model meant for one is trained on (hparams ``causal_features: True``). ``fbank``: the recipe's
    Fbank (its window, filters, hop, top_db, amin are used; it is not called). The signal is padded with n_fft/2 zeros on the left
    and, at its end, on the right; frame k covers padded samples [k*hop, k*hop + n_fft) - the offline center=True frame, bit for bit,
    before the floor - and exists once sample k*hop + n_fft/2 - 1 has arrived (16 ms of look-ahead). Frame k is floored at top_db below
    the maximum of frames 0..k and normalised with the per-bin mean / unbiased deviation of the floored frames 0..k (fp64 sums in
    frame order; fewer than 2 frames: deviation 1), so no frame depends on later audio or on how the audio is cut into pushes.
    ``prior`` = (mean [n_mels], std [n_mels], n0): n0 pseudo-frames of those statistics start the sums (Kaldi's online-CMVN prior).

    forward(wav, rel_lens): whole utterances in one call. init_stream / forward_chunk: the same frames push by push."""

    def __init__(self, fbank, prior=None, out_dtype=torch.float32):
        super().__init__()
        if fbank.n_fft != 512 or fbank.win_length != 512:
            raise NotImplementedError("ts-asr_amd.CausalFeatures: n_fft = win_length = 512 samples (as ops.fbank)")
        self.fbank, self.eps, self.out_dtype = fbank, 1e-10, out_dtype
        self.pad, self.hop, self.n_mels = fbank.n_fft // 2, fbank.hop_length, fbank.n_mels
        self.prior_n = 0.0
        if prior is not None:
            mu, sd, n0 = prior
            self.prior_n = float(n0)
            self.register_buffer("prior_mean", torch.as_tensor(mu, dtype=torch.float64).reshape(self.n_mels).clone(), persistent=False)
            self.register_buffer("prior_std", torch.as_tensor(sd, dtype=torch.float64).reshape(self.n_mels).clone(), persistent=False)

    def _norm_state(self, B, device):
        prior = (self.prior_mean, self.prior_std, self.prior_n) if self.prior_n > 0 else None
        return ops.running_norm_state(B, self.n_mels, device, prior)

    def _frames(self, seg):
        return ops.fbank_frames(seg, self.fbank.window, self.fbank.fbank_matrix, self.hop, self.fbank.amin)

    def forward(self, wav, rel_lens):
        """wav [B,L], rel_lens [B] -> [B, 1 + L//hop, n_mels]; row b's statistics stop at abs_lengths_round(rel_lens, T)[b] frames.
        Every call starts from a fresh state (one zero fill; with a prior three more element-wise launches): no host copy, capturable."""
        C.require_gpu(wav, rel_lens)
        db = self._frames(F.pad(wav.detach().float(), (self.pad, self.pad)))
        n_valid = abs_lengths_round(rel_lens, db.shape[1]).to(torch.int32).contiguous()
        return ops.running_norm(db, self._norm_state(wav.shape[0], wav.device), n_valid, self.fbank.top_db, self.eps, self.out_dtype)

    def init_stream(self, B, device):
        """State of B streams that start together: the samples not yet consumed (the left padding to begin with), the normaliser's
        state, and per stream whether and where it ended."""
        return {"buf": torch.zeros(B, self.pad, dtype=torch.float32, device=device), "norm": self._norm_state(B, device),
                "samples": 0, "emitted": 0, "valid": [None] * B, "closed": False}

    def forward_chunk(self, wav_chunk, state, wav_lens=None, last=False, group=4):
        """Next N samples of every stream, wav_chunk [B,N] (any N >= 0) -> (feats [B,F,n_mels], n_valid [B] int32, state). F is the
        largest multiple of ``group`` of frames whose samples have arrived (every remaining frame when ``last``: the right padding is
        appended; no push may follow), possibly 0; it depends on the number of samples pushed to the batch only. wav_lens [B]: valid
        samples of this push per stream (default N); fewer than N ends that stream - the rest of its row is taken as zeros, its later
        pushes must carry 0, and its frames past 1 + (its samples)//hop are not counted in n_valid and leave its statistics alone.
        The state is updated in place; a push that raises leaves it as it was."""
        B = state["buf"].shape[0]
        if wav_chunk.ndim != 2 or wav_chunk.shape[0] != B:
            raise ValueError(f"wav_chunk must be [B={B}, N], got {tuple(wav_chunk.shape)}")
        if state["closed"]:
            raise ValueError("forward_chunk after the last push of the stream")
        if int(group) < 1:
            raise ValueError(f"group must be >= 1, got {group}")
        N = wav_chunk.shape[1]
        lens = [N] * B if wav_lens is None else [int(v) for v in torch.as_tensor(wav_lens).reshape(-1).tolist()]
        if len(lens) != B or any(v < 0 or v > N for v in lens):
            raise ValueError(f"wav_lens must hold B={B} counts in [0, {N}], got {lens}")
        for b, v in enumerate(lens):
            if state["valid"][b] is not None and v != 0:
                raise ValueError(f"stream {b} ended at sample {state['valid'][b]}: its later pushes carry 0 valid samples, got {v}")
        C.require_gpu(wav_chunk)
        # ---- checked: from here on the state moves
        chunk = wav_chunk.detach().float()
        if any(v < N for v in lens):
            keep = torch.arange(N, device=chunk.device)[None, :] < torch.tensor(lens, device=chunk.device)[:, None]
            chunk = chunk * keep
        for b, v in enumerate(lens):
            if state["valid"][b] is None and v < N:
                state["valid"][b] = state["samples"] + v
        state["samples"] += N
        P, e0 = state["samples"], state["emitted"]
        parts = [state["buf"], chunk] + ([chunk.new_zeros(B, self.pad)] if last else [])
        buf = torch.cat(parts, dim=1)
        if last:
            e1 = 1 + P // self.hop
            state["closed"] = True
        else:
            avail = (P - self.pad) // self.hop + 1 if P >= self.pad else 0
            e1 = e0 + max(avail - e0, 0) // int(group) * int(group)
        nf = e1 - e0
        ends = [e1 if a is None else min(max(1 + a // self.hop, e0), e1) for a in state["valid"]]
        n_valid = torch.tensor([e - e0 for e in ends], dtype=torch.int32, device=chunk.device)
        if nf == 0:
            state["buf"] = buf
            return torch.empty(B, 0, self.n_mels, dtype=self.out_dtype, device=chunk.device), n_valid, state
        db = self._frames(buf[:, :(nf - 1) * self.hop + 2 * self.pad])
        feats = ops.running_norm(db, state["norm"], n_valid, self.fbank.top_db, self.eps, self.out_dtype)
        state["buf"] = buf[:, nf * self.hop:].contiguous()
        state["emitted"] = e1
        return feats, n_valid, state

    # ---- slots: every row a session of its own (StreamingTranscriber.admit(..., audio=True)); the caller keeps the counts -----------
    def init_slots(self, B, cap, device):
        """State of B slots: a sample ring [B, cap] on the device (sample s of a slot's session at s % cap; never cleared), the
        normaliser's state (one row per slot) and the filter-band workspace of the frame kernel."""
        if int(cap) < 2 * self.pad:
            raise ValueError(f"init_slots: the ring holds at least one window of {2 * self.pad} samples, got cap={cap}")
        return {"ring": torch.zeros(B, int(cap), dtype=torch.float32, device=device), "norm": ops.running_norm_state(B, self.n_mels, device),
                "ws": torch.empty(C.lib().tsasr_fbank_frames_workspace_bytes(self.n_mels), dtype=torch.uint8, device=device)}

    def reset_slot(self, state, slot, prior=None):
        """A new session in ``slot``: its normaliser row is a fresh stream's (zeros, or ``prior`` = (mean, std, n0) as
        ops.running_norm_state writes it). The ring keeps its bytes: samples a session has not received are never read."""
        state["norm"][slot] = ops.running_norm_state(1, self.n_mels, state["norm"].device, prior)[0]

    def append_slots(self, state, wav, tbl):
        """ring[b][(have[b] + i) % cap] = wav[b][i], i < lens[b]; tbl [2,B] int32 on the device = (have % cap, lens). One launch."""
        ops.audio_ring_append(state["ring"], wav, tbl)

    def frames_slots(self, state, tbl, F):
        """F normalised frames per slot -> [B,F,n_mels]: row i < count[b] of slot b is frame first[b] + i of its session (the bits of
        forward() over the session alone), computed from its ring and advancing its normaliser row; a slot with count 0 keeps its
        state. tbl [3,B] int32 on the device = (first, count, total samples received). Frames (with the tiny filter-band kernel before them) and norm: no copy of the samples, whatever B."""
        db = ops.fbank_frames_slots(state["ring"], tbl, F, self.fbank.window, self.fbank.fbank_matrix, self.hop, self.fbank.amin, ws=state["ws"])
        return ops.running_norm(db, state["norm"], tbl[1], self.fbank.top_db, self.eps, self.out_dtype)

# ------------------------------------------------------------------------------------------------------
# A17 / A18 the two augmenters of compute_forward (TRAIN stage, ``augment: True``; train_librispeechmix_scratch.py:82-94)
# ------------------------------------------------------------------------------------------------------
class SpecAugment(nn.Module):
    """speechbrain.lobes.augment.SpecAugment (SB/lobes/augment.py:32-201), same constructor. Differences: the draws come from a
    device-side counter generator (one tiny kernel) instead of torch's CPU/GPU generators - distribution-identical, no host
    synchronisation, capturable into the step's hipGraph - and the result is a new tensor (the reference warps in place)."""

    def __init__(self, time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True, freq_mask_width=(0, 20),
                 n_freq_mask=2, time_mask=True, time_mask_width=(0, 100), n_time_mask=2, replace_with_zero=True):
        super().__init__()
        assert time_warp or freq_mask or time_mask, "at least one of time_warp, time_mask, or freq_mask should be applied"
        if time_warp and time_warp_mode != "bicubic":
            raise NotImplementedError("ts-asr_amd.SpecAugment implements time_warp_mode='bicubic' (the default and all TS-ASR YAMLs)")
        as_range = lambda w: (0, w) if isinstance(w, int) else tuple(w)  # noqa: E731
        self.apply_time_warp, self.time_warp_window, self.time_warp_mode = time_warp, time_warp_window, time_warp_mode
        self.freq_mask, self.freq_mask_width, self.n_freq_mask = freq_mask, as_range(freq_mask_width), n_freq_mask
        self.time_mask, self.time_mask_width, self.n_time_mask = time_mask, as_range(time_mask_width), n_time_mask
        self.replace_with_zero = replace_with_zero

    def _counts(self):
        return (self.n_freq_mask if self.freq_mask else 0), (self.n_time_mask if self.time_mask else 0)

    def draw(self, x):
        """Device int32 table of this call's random numbers (layout: include/tsasr_hip.h, tsasr_specaug_draw)."""
        B, T, Fq = x.shape[0], x.shape[-2], x.shape[-1]
        nf, nt = self._counts()
        return ops.spec_augment_draw(B, T, Fq, self.time_warp_window if self.apply_time_warp else 0, nf, self.freq_mask_width, nt,
                                     self.time_mask_width, x.device)

    def forward(self, x, params=None):
        C.require_gpu(x)
        shape = x.shape
        if x.dim() == 4:                      # [B,C,T,F]: masks are drawn per (batch x channel) row, as the reference's view does
            x = x.reshape(-1, shape[2], shape[3])
        nf, nt = self._counts()
        y = ops.spec_augment_apply(x, self.draw(x) if params is None else params, nf, nt, self.replace_with_zero)
        return y.view(shape)


class Resample(nn.Module):
    """speechbrain.processing.speech_augmentation.Resample (SB/processing/speech_augmentation.py:504-820): windowed-sinc
    polyphase resampling. The filter bank is built once on the host with the reference's formulas; the resampling itself is one
    HIP launch instead of one conv1d + conv_transpose1d + two pads per phase."""

    def __init__(self, orig_freq=16000, new_freq=16000, lowpass_filter_width=6):
        super().__init__()
        self.orig_freq, self.new_freq, self.lowpass_filter_width = int(orig_freq), int(new_freq), lowpass_filter_width
        base = math.gcd(self.orig_freq, self.new_freq)
        self.conv_stride, self.output_samples = self.orig_freq // base, self.new_freq // base
        self.conv_transpose_stride = self.output_samples
        self._bank = {}

    def _filters(self, device):
        """(weights [P,W] fp32, first [P] int32) on ``device``: Hann-windowed sinc, cutoff 0.99 x the lower Nyquist (:758-820)."""
        if device not in self._bank:
            cutoff = 0.99 * 0.5 * min(self.orig_freq, self.new_freq)
            half = self.lowpass_filter_width / (2.0 * cutoff)
            out_t = torch.arange(0.0, self.output_samples) / self.new_freq
            lo = torch.ceil((out_t - half) * self.orig_freq)
            hi = torch.floor((out_t + half) * self.orig_freq)
            taps = torch.arange(int((hi - lo + 1).max()))
            dt = (lo[:, None] + taps[None, :]) / self.orig_freq - out_t[:, None]
            w = torch.where(dt.abs() < half, 0.5 * (1 + torch.cos(2 * math.pi * cutoff / self.lowpass_filter_width * dt)), torch.zeros_like(dt))
            safe = torch.where(dt == 0, torch.ones_like(dt), dt)
            w = w * torch.where(dt == 0, torch.full_like(dt, 2 * cutoff), torch.sin(2 * math.pi * cutoff * safe) / (math.pi * safe))
            self.first_indices, self.weights = lo, w / self.orig_freq
            self._bank[device] = (self.weights.to(device).contiguous(), lo.to(torch.int32).to(device))
        return self._bank[device]

    def forward(self, waveforms):
        if self.orig_freq == self.new_freq:
            return waveforms
        C.require_gpu(waveforms)
        if waveforms.dim() == 2:
            w, f = self._filters(waveforms.device)
            return ops.resample(waveforms, w, f, self.orig_freq, self.new_freq)
        if waveforms.dim() == 3:              # [B,L,C]: channels are resampled independently
            B, L, Cn = waveforms.shape
            w, f = self._filters(waveforms.device)
            y = ops.resample(waveforms.transpose(1, 2).reshape(B * Cn, L), w, f, self.orig_freq, self.new_freq)
            return y.view(B, Cn, -1).transpose(1, 2)
        raise ValueError("Input must be 2 or 3 dimensions")


class SpeedPerturb(nn.Module):
    """speechbrain.processing.speech_augmentation.SpeedPerturb (:435-501): one of ``speeds`` (percent) is picked per batch with
    the same CPU draws as the reference (torch.rand(1), torch.randint(len(speeds), (1,))) and applied by ``Resample``."""

    def __init__(self, orig_freq, speeds=[90, 100, 110], perturb_prob=1.0):  # noqa: B006  (reference signature)
        super().__init__()
        self.orig_freq, self.speeds, self.perturb_prob = orig_freq, list(speeds), perturb_prob
        self.samp_index = 0
        self.resamplers = [Resample(orig_freq=orig_freq, new_freq=orig_freq * speed // 100) for speed in self.speeds]

    def draw(self):
        """The reference's two CPU draws for the NEXT forward (torch.rand(1) against perturb_prob, torch.randint over the speeds),
        taken ahead of it: the host picks the speed before a hipGraph replay and the Brain keys its graphs by the result - a draw made
        inside a captured forward would be frozen into every replay. Returns (skip, speed index)."""
        skip = bool(torch.rand(1) > self.perturb_prob)
        if not skip:
            self.samp_index = int(torch.randint(len(self.speeds), (1,))[0])
        self._pending = (skip, self.samp_index)
        return self._pending

    def forward(self, waveform):
        skip, idx = self._pending if getattr(self, "_pending", None) is not None else self.draw()
        self._pending = None
        if skip:
            return waveform.clone()
        return self.resamplers[idx](waveform)

# ------------------------------------------------------------------------------------------------------
# A3 convolutional front-end
# ------------------------------------------------------------------------------------------------------
class _Holder(nn.Module):
    """Gives a child the attribute name the reference's state_dict uses (``conv`` / ``norm``)."""

    def __init__(self, name, child):
        super().__init__()
        self.add_module(name, child)


_FUSED_CONVBLOCK = True   # (False: conv kernel + 2 LayerNorm kernels + dropout-add kernel - the path of shapes the fused kernel does not take)


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels, in_freq, kernel_size=3, stride=2, padding="same"):
        super().__init__()
        self.padding, self.stride, self.k = padding, stride, kernel_size
        out_freq = (in_freq + 2 * (kernel_size // 2) - kernel_size) // stride + 1
        self.convs = nn.Module()
        self.convs.add_module("conv_0", _Holder("conv", nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride)))
        self.convs.add_module("norm_0", _Holder("norm", nn.LayerNorm([out_freq, out_channels])))
        self.reduce_conv = nn.Module()
        self.reduce_conv.add_module("conv", _Holder("conv", nn.Conv2d(in_channels, out_channels, 1, stride=stride)))
        self.reduce_conv.add_module("norm", _Holder("norm", nn.LayerNorm([out_freq, out_channels])))
        self.out_freq = out_freq

    def forward(self, x, dropout, training):
        """x [B,T,F,C] (channels-last all the way: this IS the NHWC layout of a conv over (T,F))."""
        c, n = self.convs.conv_0.conv, self.convs.norm_0.norm
        rc, rn = self.reduce_conv.conv.conv, self.reduce_conv.norm.norm
        if _FUSED_CONVBLOCK and ops.frontend_block_supported(x, c.weight.shape[0]):   # the whole block in one kernel per direction
            return ops.frontend_block(x, c.weight, c.bias, rc.weight, rc.bias, n.weight, n.bias, rn.weight, rn.bias, self.padding,
                                      0.01, 1e-5, dropout, training)
        y, r = ops.frontend_convs(x, c.weight, c.bias, rc.weight, rc.bias, self.padding)
        y = ops.layer_norm(y, n.weight, n.bias, 1e-5, act_slope=0.01)               # LN over [F,C] + LeakyReLU, one pass
        r = ops.layer_norm(r, rn.weight, rn.bias, 1e-5)
        return ops.dropout_add(y, None, r, 1.0, dropout, training, outer_p=dropout)   # Dropout(r + Dropout(y)), one pass


class ConvolutionFrontEnd(nn.Module):
    def __init__(self, input_shape, num_blocks=3, num_layers_per_block=5, out_channels=(128, 256, 512),
                 kernel_sizes=(3, 3, 3), strides=(1, 2, 2), dilations=(1, 1, 1), residuals=(True, True, True),
                 conv_module=None, activation=nn.LeakyReLU, norm=None, dropout=0.1, conv_bias=True, padding="same",
                 conv_init=None):
        super().__init__()
        if num_layers_per_block != 1 or not all(residuals[:num_blocks]) or activation is not nn.LeakyReLU \
                or any(s != 2 for s in strides[:num_blocks]) or any(d != 1 for d in dilations[:num_blocks]):
            raise NotImplementedError("ts-asr_amd.ConvolutionFrontEnd implements the TS-ASR YAML configuration: "
                                      "1 layer per block, stride 2, residual blocks, LayerNorm, LeakyReLU")
        self.dropout = dropout
        freq, cin = input_shape[-1], 1
        for i in range(num_blocks):
            blk = ConvBlock(cin, out_channels[i], freq, kernel_sizes[i], strides[i], padding)
            self.add_module(f"convblock_{i}", blk)
            freq, cin = blk.out_freq, out_channels[i]
        self.num_blocks = num_blocks

    def forward(self, x):
        C.require_gpu(x)
        x = _cd(x)
        if x.ndim == 3:
            x = x.unsqueeze(-1)
        for i in range(self.num_blocks):
            x = getattr(self, f"convblock_{i}")(x, self.dropout, self.training)
        return x

    def forward_chunk(self, x, state=None):
        """Streaming forward of a causally padded front-end (eval only): x [B,F,80] the next F feature frames, ``state`` the list of
        the last 2 input frames of each block (None = start of the stream: zeros, the offline causal pad). Each block runs the offline
        kernels on [carry | chunk] and drops its first output row, whose window reaches into the zero pad in front of the carry; row
        r + 1 of that output is row (t0 + r) of the offline output (3x3 stride-2 window on input rows 2t-2 .. 2t). Returns
        (y [B, ceil(ceil(F/2)/2), F', C], new state)."""
        C.require_gpu(x)
        if torch.is_grad_enabled() or self.training:
            raise RuntimeError("ConvolutionFrontEnd.forward_chunk is inference only (eval mode, under torch.no_grad())")
        x = _cd(x)
        if x.ndim == 3:
            x = x.unsqueeze(-1)
        new_state = []
        for i in range(self.num_blocks):
            blk = getattr(self, f"convblock_{i}")
            if blk.padding != "causal":
                raise ValueError("forward_chunk needs a front-end with padding='causal'")
            carry = state[i] if state is not None else torch.zeros(x.shape[0], 2, x.shape[2], x.shape[3], dtype=x.dtype, device=x.device)
            xe = torch.cat([carry, x], dim=1)
            new_state.append(xe[:, -2:].contiguous())
            x = blk(xe, 0.0, False)[:, 1:]
        return x, new_state


# ------------------------------------------------------------------------------------------------------
# A6-A9 Conformer block
# ------------------------------------------------------------------------------------------------------
class RelPosEncXL(nn.Module):
    """Symmetric table of the reference (SB/nnet/attention.py:352: the sin term keeps its sign in the future half):
    pe[i] = PE_abs(|T-1-i|), i = 0..2T-2. Cached per (T, dtype): it depends on nothing else."""

    def __init__(self, emb_dim):
        super().__init__()
        self.emb_dim = emb_dim
        inv_freq = torch.exp(torch.arange(0, emb_dim, 2, dtype=torch.float32) * -(math.log(10000.0) / emb_dim))
        self.register_buffer("inv_freq", inv_freq)
        self._cache = {}

    def forward(self, x):
        T = x.size(1)
        key = (T, x.device)
        if key not in self._cache:
            with torch.no_grad():
                pos = (torch.arange(2 * T - 1, device=x.device, dtype=torch.float32) - (T - 1)).abs().unsqueeze(-1)
                ang = pos * self.inv_freq.to(x.device)
                pe = torch.empty(2 * T - 1, self.emb_dim, device=x.device)
                pe[:, 0::2], pe[:, 1::2] = torch.sin(ang), torch.cos(ang)
                self._cache[key] = pe.unsqueeze(0)
        return self._cache[key]


_POS_CD = {}


def _pos_cd(pos_embs):
    """pos_embs[0] in the compute dtype. The table is a long-lived cached tensor (RelPosEncXL): cast it once, not once per layer
    and step (18 small cast kernels per step otherwise)."""
    if pos_embs.dtype == _COMPUTE_DTYPE:
        return pos_embs[0]
    key = (pos_embs.data_ptr(), tuple(pos_embs.shape), _COMPUTE_DTYPE)
    hit = _POS_CD.get(key)
    if hit is None or hit[0] is not pos_embs:
        _POS_CD[key] = hit = (pos_embs, pos_embs[0].to(_COMPUTE_DTYPE))
    return hit[1]


class RelPosMHAXL(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout=0.0, vbias=False, vdim=None, mask_pos_future=False):
        super().__init__()
        if vbias or (vdim is not None and vdim != embed_dim):
            raise NotImplementedError("vbias / vdim are not used by the TS-ASR recipes")
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.mask_pos_future = mask_pos_future
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        self.linear_pos = nn.Linear(embed_dim, embed_dim, bias=False)
        self.pos_bias_u = nn.Parameter(torch.empty(self.head_dim, num_heads))
        self.pos_bias_v = nn.Parameter(torch.empty(self.head_dim, num_heads))
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.xavier_uniform_(self.pos_bias_u)
        nn.init.xavier_uniform_(self.pos_bias_v)
        self.scale = 1.0 / math.sqrt(embed_dim)  # 1/sqrt(embed_dim), NOT 1/sqrt(head_dim) (attention.py:452)

    def forward(self, query, key, value, pos_embs, key_padding_mask=None, attn_mask=None, return_attn_weights=True,
                key_lens=None, causal=None):
        """Self-attention only (query is key is value, as ConformerEncoderLayer calls it). ``key_lens`` (int32 [B],
        valid keys per utterance) / ``causal`` are the device-side equivalents of key_padding_mask / the look-ahead
        attn_mask; when the reference-style masks are given instead they are converted (prefix masks only)."""
        C.require_gpu(query)
        if not (query is key and key is value):
            raise NotImplementedError("RelPosMHAXL is used as self-attention on this path")
        B, T, D = query.shape
        if key_lens is None and key_padding_mask is not None:
            key_lens = (~key_padding_mask).sum(-1).to(torch.int32)
        if causal is None:
            causal = attn_mask is not None
        o, attn = self._context(_cd(query), pos_embs, key_lens, causal, return_attn_weights)
        out = ops.linear(o, self.out_proj.weight, self.out_proj.bias)
        return (out, attn) if return_attn_weights else out

    def project_pos(self, pos_embs):
        """(pk, deferrable): pk = linear_pos(pos_embs) [2T-1, D] - depends on the weights and the positional table only, so the encoder
        computes it for ALL its layers ahead of the first one (the main stream then does it while it would otherwise wait for the speaker
        branch at the injection, instead of once per layer on the critical path). deferrable: d(pk) has ONE reader - that weight's
        gradient - when pk is the HIP GEMM of a leaf weight over the gradient-free table (ops._RelPosAttnFn.backward)."""
        pos = _pos_cd(pos_embs)
        w = self.linear_pos.weight
        return ops.matmul_nt(pos, w), bool(ops._gemm_ok(pos, w) and w.is_leaf and not pos.requires_grad)

    def _context(self, x, pos_embs, key_lens, causal, need_weights, pk=None):
        qkv = ops.matmul_nt(x, self.in_proj_weight)                          # [B,T,H*3*Dh] per-head interleaved Q|K|V
        pk, deferrable = self.project_pos(pos_embs) if pk is None else pk
        return ops.relpos_attention(qkv, pk, self.pos_bias_u, self.pos_bias_v, key_lens, self.num_heads, self.scale, causal,
                                    self.dropout if self.training else 0.0, need_weights, dpk_deferrable=deferrable)

    def forward_add(self, x, res, pos_embs, key_lens=None, causal=False, need_weights=False):
        """res + out_proj(attention(x)) with the projection bias and the residual add in one epilogue pass."""
        o, attn = self._context(_cd(x), pos_embs, key_lens, causal, need_weights)
        return ops.dropout_add(ops.matmul_nt(o, self.out_proj.weight), self.out_proj.bias, res), attn


class PositionalwiseFeedForward(nn.Module):
    def __init__(self, d_ffn, input_shape=None, input_size=None, dropout=0.0, activation=nn.ReLU):
        super().__init__()
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size")
        if input_size is None:
            input_size = input_shape[-1]
        self.ffn = nn.Sequential(nn.Linear(input_size, d_ffn), activation(), nn.Dropout(dropout), nn.Linear(d_ffn, input_size))


def _act_slope(activation):
    a = activation() if isinstance(activation, type) else activation
    if isinstance(a, nn.LeakyReLU):
        return a.negative_slope
    if isinstance(a, nn.ReLU):
        return 0.0
    raise NotImplementedError("ts-asr_amd kernels fuse LeakyReLU/ReLU (all TS-ASR YAMLs pass torch.nn.LeakyReLU)")


class ConvolutionModule(nn.Module):
    def __init__(self, input_size, kernel_size=31, bias=True, activation=nn.LeakyReLU, dropout=0.0, causal=False, dilation=1):
        super().__init__()
        if dilation != 1 or not bias:
            raise NotImplementedError("dilation/bias-free conv module is not used by the TS-ASR recipes")
        self.causal, self.kernel_size, self.dropout = causal, kernel_size, dropout
        self.padding = (kernel_size - 1) if causal else (kernel_size - 1) // 2
        self.slope = _act_slope(activation)
        self.layer_norm = nn.LayerNorm(input_size)
        self.bottleneck = nn.Sequential(nn.Conv1d(input_size, 2 * input_size, kernel_size=1), nn.GLU(dim=1))
        self.conv = nn.Conv1d(input_size, input_size, kernel_size, padding=self.padding, groups=input_size)
        self.after_conv = nn.Sequential(nn.LayerNorm(input_size), activation(), nn.Linear(input_size, input_size), nn.Dropout(dropout))

    def forward(self, x, mask=None, valid_lens=None):
        """``valid_lens`` int32 [B] replaces the boolean pad mask ([B,T,1], True = padded) of the reference."""
        if valid_lens is None and mask is not None:
            valid_lens = (~mask.squeeze(-1)).sum(-1).to(torch.int32)
        return self.forward_add(x, None, valid_lens)

    def core(self, y, last=True):
        """Everything between the module's LayerNorm and its last bias/dropout: y = LN(x) -> [.., D] (bias of after_conv[2] not added);
        last=False stops in front of the last point-wise convolution (the caller fuses it with what follows)."""
        y = ops.matmul_nt(y, self.bottleneck[0].weight)     # 1x1 conv D->2D: the [2D, D, 1] Parameter itself (bias below)
        y = ops.convmod_core(y, self.bottleneck[0].bias, self.conv.weight, self.conv.bias, self.after_conv[0].weight,
                             self.after_conv[0].bias, self.causal, 1e-5, self.slope)                # bias+GLU+depthwise+LN+act
        return ops.matmul_nt(y, self.after_conv[2].weight) if last else y

    def forward_add(self, x, res, valid_lens=None):
        """res + module(x) with dropout, pad masking and the residual add fused into the last pass."""
        y = self.core(ops.layer_norm(x, self.layer_norm.weight, self.layer_norm.bias, 1e-5))
        return ops.dropout_add(y, self.after_conv[2].bias, res, 1.0, self.dropout, self.training, valid_lens)


class ConformerEncoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, nhead, kernel_size=31, kdim=None, vdim=None, activation=nn.LeakyReLU, bias=True,
                 dropout=0.0, causal=False, attention_type="RelPosMHAXL", chunk_size=0):
        super().__init__()
        # chunk_size (BUILD EXTENSION, not in the reference: BASELINE.json configs[4] "chunk=40 frames"): with causal=True and chunk_size > 1
        # the look-ahead mask becomes block-causal - a frame attends its whole chunk and everything before it; the convolution module and
        # the front-end stay strictly causal. 0 / 1 = the reference's look-ahead mask.
        self.chunk_size = int(chunk_size or 0)
        if attention_type != "RelPosMHAXL":
            raise NotImplementedError("the TS-ASR encoder always uses RelPosMHAXL (models/conformer.py:131-132)")
        self.mha_layer = RelPosMHAXL(num_heads=nhead, embed_dim=d_model, dropout=dropout, mask_pos_future=causal)
        self.convolution_module = ConvolutionModule(d_model, kernel_size, bias, activation, dropout, causal=causal)
        self.ffn_module1 = nn.Sequential(nn.LayerNorm(d_model), PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout, activation=activation), nn.Dropout(dropout))
        self.ffn_module2 = nn.Sequential(nn.LayerNorm(d_model), PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout, activation=activation), nn.Dropout(dropout))
        self.norm1 = LayerNorm(d_model)
        self.norm2 = LayerNorm(d_model)
        self.drop = nn.Dropout(dropout)
        self.causal, self.dropout, self.slope = causal, dropout, _act_slope(activation)

    def _ffn_add(self, x, mod):
        """x + 0.5 * Dropout(PFF(LN(x)))  - macaron half-step (Conformer.py:243,258)."""
        ln, pff = mod[0], mod[1].ffn
        y = ops.layer_norm(x, ln.weight, ln.bias, 1e-5)
        y = ops.ffn_core(y, pff[0].weight, pff[0].bias, pff[3].weight, self.slope, self.dropout, self.training)   # two GEMMs, fused epilogues
        return ops.dropout_add(y, pff[3].bias, x, 0.5, self.dropout, self.training)

    def forward(self, x, src_mask=None, src_key_padding_mask=None, pos_embs=None, valid_lens=None, need_attn=True, prenorm=None,
                next_ln=None, pk=None):
        """Returns (x, attention weights [B,H,T,T] or None). The reference always materialises the weights
        (Conformer.py:247-254); the encoder passes need_attn=False unless return_attn is requested.
        Every ``residual + branch`` of Conformer.py:243-259 is fused with the LayerNorm that reads it (ops.add_layer_norm).
        The seam between two LAYERS is two LayerNorms in a row (this layer's norm2, then the next layer's first macaron LayerNorm or the
        encoder's final norm): the encoder may pass that next ``nn.LayerNorm`` as ``next_ln`` - a third value, next_ln(x), is then
        returned (same launch as norm2, same bits) - and hand it to the next layer as ``prenorm``."""
        if valid_lens is None and src_key_padding_mask is not None:
            valid_lens = (~src_key_padding_mask).sum(-1).to(torch.int32)
        tr, p, conv, mha = self.training, self.dropout, self.convolution_module, self.mha_layer
        ln1, pff1 = self.ffn_module1[0], self.ffn_module1[1].ffn
        ln2, pff2 = self.ffn_module2[0], self.ffn_module2[1].ffn
        x = _cd(x)
        if prenorm is None:
            y, x = ops.layer_norm_res(x, ln1.weight, ln1.bias, 1e-5)     # x is read twice (here and as the residual): one backward kernel sums both gradients
        else:
            y = prenorm                                                  # ln1(x), computed by the previous layer's last launch
        h = ops.ffn_core(y, pff1[0].weight, pff1[0].bias, pff1[3].weight, self.slope, p, tr)
        x, y = ops.add_layer_norm(h, pff1[3].bias, x, self.norm1.norm, 0.5, p, tr)                  # x + .5*drop(ffn1) ; norm1
        causal = self.causal or src_mask is not None
        o, attn = mha._context(y, pos_embs, valid_lens, (max(self.chunk_size, 1) if causal else 0), need_attn, pk=pk)   # pk: mha.project_pos(pos_embs), made ahead by the encoder
        # the two seams whose GEMM has K = d_model: projection, residual tail and LayerNorm in one launch (csrc/linear_ln.hip)
        x, y = ops.linear_add_layer_norm(o, mha.out_proj.weight, mha.out_proj.bias, x, conv.layer_norm)               # + skip ; conv LN
        c = conv.core(y, last=False)
        x, y = ops.linear_add_layer_norm(c, conv.after_conv[2].weight, conv.after_conv[2].bias, x, ln2, 1.0, conv.dropout, tr, valid_lens)   # + conv ; ffn2 LN
        h = ops.ffn_core(y, pff2[0].weight, pff2[0].bias, pff2[3].weight, self.slope, p, tr)
        if next_ln is not None and ops.add_layer_norm2_supported(h):
            x, z = ops.add_layer_norm2(h, pff2[3].bias, x, self.norm2.norm, next_ln, 0.5, p, tr, eps2=next_ln.eps)
            return x, attn, z
        _, x = ops.add_layer_norm(h, pff2[3].bias, x, self.norm2.norm, 0.5, p, tr)                  # norm2(x + .5*drop(ffn2))
        return (x, attn) if next_ln is None else (x, attn, None)

    def init_stream(self, B, max_frames, dtype, device):
        """Per-layer streaming state: K/V cache [B,H,max_frames,Dh] each, two fp32 conv histories [B,K-1,D] (swapped per chunk)."""
        mha, conv = self.mha_layer, self.convolution_module
        H, Dh, D, K = mha.num_heads, mha.head_dim, mha.embed_dim, conv.kernel_size
        kv = torch.zeros(2, B, H, max_frames, Dh, dtype=dtype, device=device)
        hist = torch.zeros(2, B, K - 1, D, dtype=torch.float32, device=device)
        return {"k": kv[0], "v": kv[1], "hist": [hist[0], hist[1]], "pk": None, "ws": {}}

    def forward_chunk(self, x, layer_state, t0, key_lens, active=None):
        """One chunk [B,C,D] of this (causal) layer at absolute frame offset ``t0``; ``key_lens`` int32 [B] = valid frames of each
        stream so far (None: all). The FFNs, norms and projections are the offline ops; the attention reads and extends the layer's
        K/V cache (ops.relpos_attention_stream), the convolution core carries its K-1 GLU rows (ops.convmod_stream). Eval only.
        Slots: ``t0`` an int32 device tensor [B] of per-row offsets (a negative entry = an idle row) and / or ``active`` bool [B]
        (default all): an idle row's K/V cache and conv history keep their bits, its attention and convolution outputs are zeros."""
        if not self.causal:
            raise ValueError("forward_chunk needs a causal layer")
        if torch.is_grad_enabled() or self.training:
            raise RuntimeError("ConformerEncoderLayer.forward_chunk is inference only (eval mode, under torch.no_grad())")
        conv, mha = self.convolution_module, self.mha_layer
        ln1, pff1 = self.ffn_module1[0], self.ffn_module1[1].ffn
        ln2, pff2 = self.ffn_module2[0], self.ffn_module2[1].ffn
        x = _cd(x)
        t0s = None
        if isinstance(t0, torch.Tensor) or active is not None:      # slot mode: one device array of offsets, idle rows negative
            t0s = t0 if isinstance(t0, torch.Tensor) else torch.full((x.shape[0],), int(t0), dtype=torch.int32, device=x.device)
            if active is not None:
                t0s = torch.where(torch.as_tensor(active, device=x.device).bool(), t0s, torch.full_like(t0s, -1))
            t0 = t0s = t0s.contiguous()
        y = ops.layer_norm(x, ln1.weight, ln1.bias, 1e-5)
        h = ops.ffn_core(y, pff1[0].weight, pff1[0].bias, pff1[3].weight, self.slope, 0.0, False)
        x, y = ops.add_layer_norm(h, pff1[3].bias, x, self.norm1.norm, 0.5)                          # x + .5*ffn1 ; norm1
        qkv = ops.matmul_nt(y, mha.in_proj_weight)
        B, Cn = qkv.shape[0], qkv.shape[1]
        ws = layer_state["ws"]
        if Cn not in ws:
            ws[Cn] = ops.relpos_attn_stream_workspace(B, Cn, mha.num_heads, mha.head_dim, layer_state["k"].shape[2], qkv.device)
        o = ops.relpos_attention_stream(qkv, layer_state["k"], layer_state["v"], layer_state["pk"], mha.pos_bias_u, mha.pos_bias_v, key_lens,
                                        mha.num_heads, mha.scale, max(self.chunk_size, 1), t0, ws[Cn])
        x, y = ops.linear_add_layer_norm(o, mha.out_proj.weight, mha.out_proj.bias, x, conv.layer_norm)               # + attention ; conv LN
        y2 = ops.matmul_nt(y, conv.bottleneck[0].weight)
        hin, hout = layer_state["hist"]
        c = ops.convmod_stream(y2, conv.bottleneck[0].bias, conv.conv.weight, conv.conv.bias, conv.after_conv[0].weight, conv.after_conv[0].bias,
                               hin, hout, 1e-5, conv.slope, t0s)
        layer_state["hist"] = [hout, hin]
        x, y = ops.linear_add_layer_norm(c, conv.after_conv[2].weight, conv.after_conv[2].bias, x, ln2)              # + conv ; ffn2 LN
        h = ops.ffn_core(y, pff2[0].weight, pff2[0].bias, pff2[3].weight, self.slope, 0.0, False)
        _, x = ops.add_layer_norm(h, pff2[3].bias, x, self.norm2.norm, 0.5)                          # norm2(x + .5*ffn2)
        return x
