"""Host mirror of the reference's joiner + head + transducer loss on top of the fused HIP kernels.

Reference interface kept (names, argument meaning, error behaviour):
  * ``Transducer_joint(joint="sum", nonlinearity=LeakyReLU)``  speechbrain/nnet/transducer/transducer_joint.py:14-95
  * ``transducer_loss(logits, targets, input_lens, target_lens, blank_index, reduction, use_torchaudio)``
    speechbrain/nnet/losses.py:29-87
Extra (MI355X-native) entry: ``fused_joint_logits`` = joiner + transducer_head without the [B,T,U,J] tensor.
"""
import torch

from . import _capi as C
from . import prof

_LDL = 32  # logits rows are padded to 32 floats (128 B) so that every row access is a 16-byte multiple
WIDE_VMAX, WIDE_JMAX = 1024, 1024   # csrc/joint_wide.hip: 32 < V <= 1024 (rows padded to the next multiple of 32 floats), J % 32 == 0, J <= 1024
JOINT_F32_EXACT = True   # fp32 activations: joint + head in exact fp32 arithmetic (csrc/joint_f32.hip). False: the MFMA kernels with fp32
                         # storage and bf16-rounded operands (tests that cover that instantiation switch it off)


def _exact(enc, J, V):
    return JOINT_F32_EXACT and enc.dtype == torch.float32 and J <= 768 and V <= 32


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class _JointLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, dec, weight, bias, slope, tlen, ulen):
        C.require_gpu(enc, dec, weight, bias)
        if enc.dtype != dec.dtype:
            raise ValueError("Arg 1 and 2 must have the same dtype")
        enc, dec = enc.contiguous(), dec.contiguous()
        w32, b32 = weight.float().contiguous(), bias.float().contiguous()
        B, T, J = enc.shape
        U1 = dec.shape[1]
        V = w32.shape[0]
        ctx.wide = V > _LDL
        if ctx.wide and (V > WIDE_VMAX or J % 32 or J > WIDE_JMAX):
            raise ValueError(f"fused joint: vocabulary {V} / joint dimension {J} outside the wide kernels' range "
                             f"(V <= {WIDE_VMAX}, J a multiple of 32 <= {WIDE_JMAX})")
        ldl = (V + 31) // 32 * 32 if ctx.wide else _LDL
        buf = torch.empty(B, T, U1, ldl, dtype=torch.float32, device=enc.device)
        ctx.exact = _exact(enc, J, V)
        with prof.region("joint_fwd"):
            if ctx.wide:     # subword vocabularies: vocabulary tiles inside the kernel; fp32 activations keep fp32 storage, operands rounded to bf16
                C.check(C.lib().tsasr_joint_wide_fwd(C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(b32), C.ptr(buf), B, T, U1, J, V, ldl,
                                                     C.io_dtype(enc), float(slope), C.stream_ptr()), "tsasr_joint_wide_fwd")
            elif ctx.exact:
                C.check(C.lib().tsasr_joint_f32_fwd(C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(b32), C.ptr(buf), B, T, U1, J, V, _LDL,
                                                    float(slope), C.stream_ptr()), "tsasr_joint_f32_fwd")
            else:
                C.check(C.lib().tsasr_joint_fwd(C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(b32), C.ptr(buf), B, T, U1, J, V, _LDL,
                                                C.io_dtype(enc), float(slope), C.stream_ptr()), "tsasr_joint_fwd")
        ctx.save_for_backward(enc, dec, w32, tlen, ulen)
        ctx.slope, ctx.V = float(slope), V
        ctx.params = (weight, bias)
        return buf[..., :V]

    @staticmethod
    def backward(ctx, dlogits):
        enc, dec, w32, tlen, ulen = ctx.saved_tensors
        B, T, J = enc.shape
        U1, V = dec.shape[1], ctx.V
        dl = _as_padded_rows(dlogits, V)
        denc, ddec = torch.empty_like(enc), torch.empty_like(dec)
        dW = torch.empty(V, J, dtype=torch.float32, device=enc.device)
        db = torch.empty(V, dtype=torch.float32, device=enc.device)
        if ctx.wide:
            nws = C.lib().tsasr_joint_wide_bwd_workspace_bytes(B, T, U1, J, V)
        else:
            nws = C.lib().tsasr_joint_f32_bwd_workspace_bytes(B, U1, J) if ctx.exact else C.lib().tsasr_joint_bwd_workspace_bytes(B, T, U1, J)
        ws = _ws(nws, enc.device)
        with prof.region("joint_bwd"):
            if ctx.wide:
                C.check(C.lib().tsasr_joint_wide_bwd(C.ptr(dl), C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(denc), C.ptr(ddec), C.ptr(dW), C.ptr(db),
                                                     C.ptr(tlen), C.ptr(ulen), B, T, U1, J, V, dl.stride(-2), C.io_dtype(enc), ctx.slope,
                                                     C.ptr(ws), ws.numel(), C.stream_ptr()), "tsasr_joint_wide_bwd")
            elif ctx.exact:
                C.check(C.lib().tsasr_joint_f32_bwd(C.ptr(dl), C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(denc), C.ptr(ddec), C.ptr(dW), C.ptr(db),
                                                    C.ptr(tlen), C.ptr(ulen), B, T, U1, J, V, dl.stride(-2), ctx.slope,
                                                    C.ptr(ws), ws.numel(), C.stream_ptr()), "tsasr_joint_f32_bwd")
            else:
              C.check(C.lib().tsasr_joint_bwd(C.ptr(dl), C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(denc), C.ptr(ddec), C.ptr(dW), C.ptr(db),
                                            C.ptr(tlen), C.ptr(ulen), B, T, U1, J, V, dl.stride(-2), C.io_dtype(enc), ctx.slope,
                                            C.ptr(ws), ws.numel(), C.stream_ptr()), "tsasr_joint_bwd")
        from .ops import _keep, _pgrad
        _keep(dW, db, ws)     # while reductions are deferred the two are filled from the slabs in `ws` by the batched launch at the end of backward
        return denc, ddec, _pgrad(ctx.params[0], dW), _pgrad(ctx.params[1], db), None, None, None


def _as_padded_rows(x, V):
    """A float32 [B,T,U1,V] tensor whose rows are 16-byte aligned multiples of 4 floats (copying only if needed)."""
    ldl = x.stride(-2) if x.dim() == 4 else 0
    ok = (x.dtype == torch.float32 and x.dim() == 4 and x.stride(-1) == 1 and ldl % 4 == 0 and ldl >= V
          and (ldl <= 32 or V > 32) and x.stride(1) == x.shape[2] * ldl and x.stride(0) == x.shape[1] * x.stride(1)
          and x.data_ptr() % 16 == 0)
    if ok:
        return x
    buf = torch.zeros(*x.shape[:3], _LDL if V <= _LDL else (V + 3) // 4 * 4, dtype=torch.float32, device=x.device)
    buf[..., :V] = x
    return buf[..., :V]


class JointLogits:
    """The joint logits as a recipe: what ``fused_joint_logits(..., materialize=False)`` returns. Nothing is launched and no [B,T,U1,V]
    tensor exists; ``rnnt_costs`` / ``transducer_loss`` / ``rnnt_align`` / ``transducer_align`` take the handle and, for 32 < V <= 1024, run
    the fused joint + loss kernels (csrc/joint_wide.hip) on its operands. ``.materialize()`` is the eager call."""

    def __init__(self, enc, dec, weight, bias, slope=0.01, enc_abs_lens=None, tok_abs_lens=None):
        if enc.dim() != 3 or dec.dim() != 3 or enc.shape[0] != dec.shape[0] or enc.shape[2] != dec.shape[2]:
            raise ValueError(f"joint operands must be [B,T,J] and [B,U1,J], got {tuple(enc.shape)} and {tuple(dec.shape)}")
        if weight.dim() != 2 or weight.shape[1] != enc.shape[2] or bias.shape != weight.shape[:1]:
            raise ValueError(f"head must be [V,J] with bias [V], got {tuple(weight.shape)} and {tuple(bias.shape)}")
        self.enc, self.dec, self.weight, self.bias, self.slope = enc, dec, weight, bias, float(slope)
        self.enc_abs_lens, self.tok_abs_lens = enc_abs_lens, tok_abs_lens

    shape = property(lambda self: torch.Size((self.enc.shape[0], self.enc.shape[1], self.dec.shape[1], self.weight.shape[0])))
    dtype = property(lambda self: torch.float32)
    device = property(lambda self: self.enc.device)
    wide = property(lambda self: self.weight.shape[0] > _LDL)

    def dim(self):
        return 4

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def materialize(self):
        """The [B,T,U1,V] logits tensor, exactly what the eager ``fused_joint_logits`` call returns (with its autograd graph)."""
        return _JointLogitsFn.apply(self.enc, self.dec, self.weight, self.bias, self.slope, self.enc_abs_lens, self.tok_abs_lens)

    def detach(self):
        return JointLogits(self.enc.detach(), self.dec.detach(), self.weight.detach(), self.bias.detach(), self.slope,
                           self.enc_abs_lens, self.tok_abs_lens)

    def _not_a_tensor(self, *a, **k):
        raise TypeError("JointLogits is a lazy handle, not a tensor: hand it to transducer_loss / rnnt_costs / rnnt_align, or call "
                        ".materialize() for the [B,T,U1,V] logits")

    __getitem__ = __setitem__ = __iter__ = __len__ = __array__ = __float__ = _not_a_tensor
    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __truediv__ = __rtruediv__ = __matmul__ = __rmatmul__ = _not_a_tensor
    __neg__ = __pow__ = __abs__ = __lt__ = __le__ = __gt__ = __ge__ = _not_a_tensor

    def __repr__(self):
        return f"JointLogits(shape={tuple(self.shape)}, io={self.enc.dtype}, device={self.device})"


def fused_joint_logits(enc_proj, dec_proj, head_weight, head_bias, slope=0.01, enc_abs_lens=None, tok_abs_lens=None, materialize=True):
    """logits[b,t,u,:] = head(LeakyReLU(enc_proj[b,t] + dec_proj[b,u]))  as a [B,T,U1,V] view of rows padded to 32 floats (V <= 32: 128-byte
    rows, csrc/rnnt.hip or the exact-fp32 csrc/joint_f32.hip; 32 < V <= 1024: csrc/joint_wide.hip, bf16-rounded operands in either dtype).
    ``materialize=False`` launches nothing and returns a ``JointLogits`` handle for the loss / alignment entries below."""
    if not materialize:
        return JointLogits(enc_proj, dec_proj, head_weight, head_bias, slope, enc_abs_lens, tok_abs_lens)
    return _JointLogitsFn.apply(enc_proj, dec_proj, head_weight, head_bias, slope, enc_abs_lens, tok_abs_lens)


def _check_wide(V, J):
    if V > WIDE_VMAX or J % 32 or J > WIDE_JMAX:
        raise ValueError(f"fused joint: vocabulary {V} / joint dimension {J} outside the wide kernels' range "
                         f"(V <= {WIDE_VMAX}, J a multiple of 32 <= {WIDE_JMAX})")


def _check_targets(tg, B, U1):
    if tg.dim() != 2 or tg.shape[0] != B or tg.shape[1] < U1 - 1:
        raise ValueError(f"targets must be [B, >= U1-1] = [{B}, >= {U1 - 1}], got {tuple(tg.shape)}")


class _JointLossFn(torch.autograd.Function):
    """Joint + head + RNN-T costs in one node, 32 < V <= 1024, without the logits / dlogits tensors (tsasr_joint_wide_loss_*)."""

    @staticmethod
    def forward(ctx, enc, dec, weight, bias, slope, targets, tlen, ulen, blank):
        C.require_gpu(enc, dec, weight, bias, targets, tlen, ulen)
        if enc.dtype != dec.dtype:
            raise ValueError("Arg 1 and 2 must have the same dtype")
        enc, dec = enc.contiguous(), dec.contiguous()
        w32, b32 = weight.float().contiguous(), bias.float().contiguous()
        B, T, J = enc.shape
        U1, V = dec.shape[1], w32.shape[0]
        _check_wide(V, J)
        tg = targets.to(torch.int32).contiguous()
        _check_targets(tg, B, U1)
        tlen, ulen = tlen.to(torch.int32).contiguous(), ulen.to(torch.int32).contiguous()
        costs = torch.empty(B, dtype=torch.float32, device=enc.device)
        ws = _ws(C.lib().tsasr_joint_wide_loss_workspace_bytes(B, T, U1, J, V), enc.device)
        with prof.region("joint_loss_fwd"):
            C.check(C.lib().tsasr_joint_wide_loss_fwd(C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(b32), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen),
                                                      C.ptr(costs), B, T, U1, J, V, int(blank), C.io_dtype(enc), float(slope), C.ptr(ws), ws.numel(),
                                                      C.stream_ptr()), "tsasr_joint_wide_loss_fwd")
        off = int(C.lib().tsasr_joint_wide_loss_error_word_offset(B, T, U1, J, V))
        if off >= 0:        # a lattice split over workgroups: keep its time-out word for Brain.flush_nonfinite, as _RnntLossFn does
            _LATTICE_ERR.append(ws[off:off + 4])
            del _LATTICE_ERR[:-4]
        ctx.save_for_backward(enc, dec, w32, b32, tg, tlen, ulen, ws)
        ctx.slope, ctx.blank = float(slope), int(blank)
        ctx.params = (weight, bias)
        return costs

    @staticmethod
    def backward(ctx, gcosts):
        enc, dec, w32, b32, tg, tlen, ulen, ws = ctx.saved_tensors
        B, T, J = enc.shape
        U1, V = dec.shape[1], w32.shape[0]
        gs = gcosts.float().contiguous()
        denc, ddec = torch.empty_like(enc), torch.empty_like(dec)
        dW = torch.empty(V, J, dtype=torch.float32, device=enc.device)
        db = torch.empty(V, dtype=torch.float32, device=enc.device)
        with prof.region("joint_loss_bwd"):
            C.check(C.lib().tsasr_joint_wide_loss_bwd(C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(b32), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen),
                                                      C.ptr(gs), C.ptr(denc), C.ptr(ddec), C.ptr(dW), C.ptr(db), B, T, U1, J, V, ctx.blank,
                                                      C.io_dtype(enc), ctx.slope, C.ptr(ws), ws.numel(), C.stream_ptr()), "tsasr_joint_wide_loss_bwd")
        from .ops import _keep, _pgrad
        _keep(dW, db, ws)     # while reductions are deferred the two are filled from the slabs in `ws` by the batched launch at the end of backward
        return denc, ddec, _pgrad(ctx.params[0], dW), _pgrad(ctx.params[1], db), None, None, None, None, None


_LATTICE_ERR = []    # time-out words of the most recent split-lattice launches (csrc/rnnt.hip AB_SPIN_LIMIT)


def lattice_timeouts():
    """Number of kept split-lattice launches whose inter-workgroup wait ran out (a host read): their costs came out NaN."""
    return sum(int(w.view(torch.int32)[0].item() == 1) for w in _LATTICE_ERR)


class _RnntLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, tlen, ulen, blank):
        C.require_gpu(logits, targets, tlen, ulen)
        B, T, U1, V = logits.shape
        lg = _as_padded_rows(logits.float() if logits.dtype != torch.float32 else logits, V)
        tg = targets.to(torch.int32).contiguous()
        tlen, ulen = tlen.to(torch.int32).contiguous(), ulen.to(torch.int32).contiguous()
        if tg.dim() != 2 or tg.shape[0] != B or tg.shape[1] < U1 - 1:
            raise ValueError(f"targets must be [B, >= U1-1] = [{B}, >= {U1 - 1}], got {tuple(tg.shape)}")
        costs = torch.empty(B, dtype=torch.float32, device=lg.device)
        ws = _ws(C.lib().tsasr_rnnt_loss_workspace_bytes(B, T, U1), lg.device)
        with prof.region("rnnt_loss_fwd"):
            C.check(C.lib().tsasr_rnnt_loss_fwd(C.ptr(lg), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen), C.ptr(costs),
                                                B, T, U1, V, lg.stride(-2), int(blank), C.ptr(ws), ws.numel(), C.stream_ptr()),
                    "tsasr_rnnt_loss_fwd")
        off = int(C.lib().tsasr_rnnt_loss_error_word_offset(B, T, U1))
        if off >= 0:        # a lattice split over workgroups (long targets in small batches): keep its time-out word for Brain.flush_nonfinite
            _LATTICE_ERR.append(ws[off:off + 4])
            del _LATTICE_ERR[:-4]
        ctx.save_for_backward(lg, tg, tlen, ulen, ws)
        ctx.blank, ctx.in_dtype = int(blank), logits.dtype
        return costs

    @staticmethod
    def backward(ctx, gcosts):
        lg, tg, tlen, ulen, ws = ctx.saved_tensors
        B, T, U1, V = lg.shape
        ldl = lg.stride(-2)
        gs = gcosts.float().contiguous()
        buf = torch.empty(B, T, U1, ldl, dtype=torch.float32, device=lg.device)
        with prof.region("rnnt_loss_bwd"):
            C.check(C.lib().tsasr_rnnt_loss_bwd(C.ptr(lg), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen), C.ptr(gs), C.ptr(buf),
                                                B, T, U1, V, ldl, ctx.blank, C.ptr(ws), ws.numel(), C.stream_ptr()),
                    "tsasr_rnnt_loss_bwd")
        g = buf[..., :V]
        return (g if ctx.in_dtype == torch.float32 else g.to(ctx.in_dtype)), None, None, None, None


def rnnt_costs(logits, targets, abs_input_lens, abs_target_lens, blank=0):
    """Per-utterance -log P(y|x) with gradient w.r.t. logits (torchaudio.functional.rnnt_loss, reduction="none"). A ``JointLogits`` handle
    with 32 < V <= 1024 runs the fused joint + loss kernels (gradients for enc, dec, head weight and bias; the lengths given HERE are the
    ones used); a narrower one is materialised and takes the route below."""
    if isinstance(logits, JointLogits):
        if logits.wide:
            return _JointLossFn.apply(logits.enc, logits.dec, logits.weight, logits.bias, logits.slope, targets, abs_input_lens, abs_target_lens,
                                      blank)
        logits = logits.materialize()
    return _RnntLossFn.apply(logits, targets, abs_input_lens, abs_target_lens, blank)


def transducer_loss(logits, targets, input_lens, target_lens, blank_index, reduction="mean", use_torchaudio=True):
    """Drop-in for speechbrain.nnet.losses.transducer_loss (losses.py:29-87).

    ``input_lens`` / ``target_lens`` are RELATIVE lengths; absolute = (rel * dim).round().int() exactly as
    losses.py:58-59. ``use_torchaudio`` selects the reference's two conventions: True (the recipes' default)
    = torchaudio semantics (no division by T); False = the Numba kernel's convention cost/T
    (speechbrain/nnet/loss/transducer_loss.py:104-106). Both run on the same HIP kernels.
    """
    from .nnet import abs_lengths_round
    tl = abs_lengths_round(input_lens, logits.shape[1])
    ul = abs_lengths_round(target_lens, targets.shape[1])
    costs = rnnt_costs(logits, targets, tl, ul, blank_index)
    if not use_torchaudio:
        costs = costs / tl.to(costs.dtype)
    if reduction == "mean":
        return costs.mean()
    if reduction == "sum":
        return costs.sum()
    if reduction == "none":
        return costs
    raise Exception("Unexpected reduction {}".format(reduction))


def rnnt_align(logits, targets, abs_input_lens, abs_target_lens, blank=0):
    """Forced alignment of `targets` on the loss lattice (csrc/rnnt.hip rnnt_viterbi_kernel; no autograd).

    Returns ``(frames int32 [B, U], scores float32 [B])`` with U = U1 - 1: ``frames[b, u]`` is the frame at which label u is emitted on
    the most probable path (-1 for u >= the utterance's target length), ``scores[b]`` that path's log-probability. Among equally
    probable paths the one that emits every label as early as possible is returned. Accepts what ``rnnt_costs`` accepts."""
    if isinstance(logits, JointLogits):
        if logits.wide:
            return _joint_align(logits, targets, abs_input_lens, abs_target_lens, blank)
        logits = logits.materialize()
    C.require_gpu(logits, targets, abs_input_lens, abs_target_lens)
    B, T, U1, V = logits.shape
    lg = logits.detach()
    lg = _as_padded_rows(lg.float() if lg.dtype != torch.float32 else lg, V)
    tg = targets.to(torch.int32).contiguous()
    tlen, ulen = abs_input_lens.to(torch.int32).contiguous(), abs_target_lens.to(torch.int32).contiguous()
    if tg.dim() != 2 or tg.shape[0] != B or tg.shape[1] < U1 - 1:
        raise ValueError(f"targets must be [B, >= U1-1] = [{B}, >= {U1 - 1}], got {tuple(tg.shape)}")
    frames = torch.empty(B, max(U1 - 1, 1), dtype=torch.int32, device=lg.device)
    scores = torch.empty(B, dtype=torch.float32, device=lg.device)
    ws = _ws(C.lib().tsasr_rnnt_align_workspace_bytes(B, T, U1), lg.device)
    with prof.region("rnnt_align"):
        C.check(C.lib().tsasr_rnnt_align(C.ptr(lg), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen), C.ptr(frames), frames.stride(0),
                                         C.ptr(scores), B, T, U1, V, lg.stride(-2), int(blank), C.ptr(ws), ws.numel(), C.stream_ptr()),
                "tsasr_rnnt_align")
    return frames[:, :U1 - 1], scores


def _joint_align(handle, targets, abs_input_lens, abs_target_lens, blank):
    """rnnt_align for a wide handle: tsasr_joint_wide_align fills the lattice planes from the joint's operands (no logits tensor)."""
    enc, dec = handle.enc.detach().contiguous(), handle.dec.detach().contiguous()
    w32, b32 = handle.weight.detach().float().contiguous(), handle.bias.detach().float().contiguous()
    C.require_gpu(enc, dec, w32, b32, targets, abs_input_lens, abs_target_lens)
    if enc.dtype != dec.dtype:
        raise ValueError("Arg 1 and 2 must have the same dtype")
    B, T, J = enc.shape
    U1, V = dec.shape[1], w32.shape[0]
    _check_wide(V, J)
    tg = targets.to(torch.int32).contiguous()
    _check_targets(tg, B, U1)
    tlen, ulen = abs_input_lens.to(torch.int32).contiguous(), abs_target_lens.to(torch.int32).contiguous()
    frames = torch.empty(B, max(U1 - 1, 1), dtype=torch.int32, device=enc.device)
    scores = torch.empty(B, dtype=torch.float32, device=enc.device)
    ws = _ws(C.lib().tsasr_joint_wide_align_workspace_bytes(B, T, U1, J, V), enc.device)
    with prof.region("joint_align"):
        C.check(C.lib().tsasr_joint_wide_align(C.ptr(enc), C.ptr(dec), C.ptr(w32), C.ptr(b32), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen),
                                               C.ptr(frames), frames.stride(0), C.ptr(scores), B, T, U1, J, V, int(blank), C.io_dtype(enc),
                                               handle.slope, C.ptr(ws), ws.numel(), C.stream_ptr()), "tsasr_joint_wide_align")
    return frames[:, :U1 - 1], scores


def transducer_align(logits, targets, input_lens, target_lens, blank_index):
    """``rnnt_align`` with RELATIVE lengths, rounded exactly as ``transducer_loss`` rounds them."""
    from .nnet import abs_lengths_round
    tl = abs_lengths_round(input_lens, logits.shape[1])
    ul = abs_lengths_round(target_lens, targets.shape[1])
    return rnnt_align(logits, targets, tl, ul, blank_index)


class Transducer_joint(torch.nn.Module):
    """Same constructor/forward as the reference joiner (transducer_joint.py:14-95) for joint="sum".

    ``forward(input_TN [B,T,1,J], input_PN [B,1,U,J])`` returns a lazy handle when the recipe immediately feeds
    the head (see ``FusedJointHead``); called stand-alone (e.g. by the searchers, one step at a time on
    [B,1,1,J]) it materialises nonlinearity(TN + PN) with ordinary device ops.
    """

    def __init__(self, joint_network=None, joint="sum", nonlinearity=torch.nn.LeakyReLU):
        super().__init__()
        if joint != "sum":
            raise NotImplementedError("ts-asr_amd implements joint='sum' (the only mode the TS-ASR recipes use)")
        self.joint_network = joint_network
        self.joint = joint
        self.nonlinearity = nonlinearity()

    def forward(self, input_TN, input_PN):
        if len(input_TN.shape) != len(input_PN.shape):
            raise ValueError("Arg 1 and 2 must be have same size")
        return self.nonlinearity(input_TN + input_PN)
