"""Host mirror of the reference's auxiliary CTC branch on top of csrc/ctc.hip.

Reference interface kept (names, argument meaning):
  * ``ctc_loss(log_probs, targets, input_lens, target_lens, blank_index, reduction)``   speechbrain/nnet/losses.py:247-296
  * ``ctc_greedy_decode(probabilities, seq_lens, blank_id)``                             speechbrain/decoders/ctc.py:334-376
  * ``Softmax(apply_log)``                                                               speechbrain/nnet/activations.py (the YAML's `log_softmax`)
The kernels take the RAW scores of ``proj_ctc`` and normalise each row themselves, so no log-prob tensor is written; a row that is
already normalised is left unchanged by that (log-softmax is idempotent): log-probs and raw scores give the same loss.
"""
import torch

from . import _capi as C
from . import prof

VMAX, UMAX = 1024, 2047     # csrc/ctc.hip: one workgroup of at most 1024 threads owns a lattice, four states per thread


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _check_ranges(B, T, U, V, blank):
    if B < 1 or T < 1:
        raise ValueError(f"ctc: empty batch (B={B}, T={T})")
    if not 1 <= V <= VMAX:
        raise ValueError(f"ctc: vocabulary {V} outside the kernels' range [1, {VMAX}]")
    if not 0 <= U <= UMAX:
        raise ValueError(f"ctc: {U} target columns outside the kernels' range [0, {UMAX}] (2 U + 1 <= 4095 lattice states)")
    if not 0 <= int(blank) < V:
        raise ValueError(f"ctc: blank {blank} outside [0, {V})")


def _padded_rows(x):
    """[B,T,V] scores in fp32 or bf16 whose rows start 16-byte aligned every ``ld`` elements, ld % 8 == 0 (copying only if needed)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    B, T, V = x.shape
    ld = x.stride(1)
    if (x.stride(2) == 1 and ld % 8 == 0 and ld >= V and x.stride(0) == T * ld and x.data_ptr() % 16 == 0):
        return x
    buf = torch.zeros(B, T, (V + 7) // 8 * 8, dtype=x.dtype, device=x.device)
    buf[..., :V] = x
    return buf[..., :V]


class _CtcLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, tlen, ulen, blank):
        C.require_gpu(logits, targets, tlen, ulen)
        if logits.dim() != 3:
            raise ValueError(f"ctc: scores must be [B,T,V], got {tuple(logits.shape)}")
        B, T, V = logits.shape
        if targets.dim() != 2 or targets.shape[0] != B:
            raise ValueError(f"ctc: targets must be [B,U] = [{B},U], got {tuple(targets.shape)}")
        U = targets.shape[1]
        _check_ranges(B, T, U, V, blank)
        lg = _padded_rows(logits)
        tg = targets.to(torch.int32).contiguous()
        if U == 0:      # (a pointer for the kernels' argument check; no column of it is read)
            tg = torch.zeros(B, 1, dtype=torch.int32, device=lg.device)
        tlen, ulen = tlen.to(torch.int32).contiguous(), ulen.to(torch.int32).contiguous()
        costs = torch.empty(B, dtype=torch.float32, device=lg.device)
        ws = _ws(C.lib().tsasr_ctc_loss_workspace_bytes(B, T, U, V), lg.device)
        with prof.region("ctc_loss_fwd"):
            C.check(C.lib().tsasr_ctc_loss_fwd(C.ptr(lg), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen), C.ptr(costs), B, T, U, V,
                                               lg.stride(1), int(blank), C.io_dtype(lg), C.ptr(ws), ws.numel(), C.stream_ptr()),
                    "tsasr_ctc_loss_fwd")
        ctx.save_for_backward(lg, tg, tlen, ulen, ws)
        ctx.blank, ctx.U, ctx.in_dtype = int(blank), U, logits.dtype
        return costs

    @staticmethod
    def backward(ctx, gcosts):
        lg, tg, tlen, ulen, ws = ctx.saved_tensors
        B, T, V = lg.shape
        ldl = lg.stride(1)
        gs = gcosts.float().contiguous()
        buf = torch.empty(B, T, ldl, dtype=lg.dtype, device=lg.device)
        with prof.region("ctc_loss_bwd"):
            C.check(C.lib().tsasr_ctc_loss_bwd(C.ptr(lg), C.ptr(tg), tg.stride(0), C.ptr(tlen), C.ptr(ulen), C.ptr(gs), C.ptr(buf), B, T, ctx.U, V,
                                               ldl, ctx.blank, C.io_dtype(lg), C.ptr(ws), ws.numel(), C.stream_ptr()),
                    "tsasr_ctc_loss_bwd")
        g = buf[..., :V]
        if ctx.in_dtype == lg.dtype:
            if len(_PADDED_GRADS) > 8:
                _PADDED_GRADS.clear()
            _PADDED_GRADS[buf.data_ptr()] = ldl
        return (g if ctx.in_dtype == lg.dtype else g.to(ctx.in_dtype)), None, None, None, None


def ctc_costs(logits, targets, abs_input_lens, abs_target_lens, blank=0):
    """Per-utterance -log P(y|x) of the CTC lattice with gradient w.r.t. ``logits`` [B,T,V] (fp32 or bf16, raw scores or log-probs: rows are
    normalised inside). ``targets`` [B,U] without blanks, lengths ABSOLUTE (clamped to [1,T] / [0,U]). An utterance with no valid path
    costs 0 and has a zero gradient (torch's zero_infinity=True). V <= 1024, U <= 2047, else ValueError before any launch."""
    return _CtcLossFn.apply(logits, targets, abs_input_lens, abs_target_lens, blank)


def ctc_loss(log_probs, targets, input_lens, target_lens, blank_index, reduction="mean"):
    """Drop-in for speechbrain.nnet.losses.ctc_loss (losses.py:247-296): RELATIVE lengths, absolute = (rel * dim).round().int() as
    losses.py:270-271; reductions as there: "mean" (torch's: each cost / max(U_b, 1), then the batch mean), "sum", "none", "batchmean"
    (sum / batch size) and "batch" (each cost / U_b).

    ``log_probs`` [B,T,V] may be log-probs (what the reference passes) or the raw scores of ``proj_ctc``: the kernels normalise every
    row themselves and log-softmax is idempotent, so both give the same value - feed the raw scores and skip the log-softmax tensor."""
    from .nnet import abs_lengths_round
    tl = abs_lengths_round(input_lens, log_probs.shape[1])
    ul = abs_lengths_round(target_lens, targets.shape[1])
    costs = ctc_costs(log_probs, targets, tl, ul, blank_index)
    if reduction == "mean":
        return (costs / ul.clamp(min=1).to(costs.dtype)).mean()
    if reduction == "sum":
        return costs.sum()
    if reduction == "none":
        return costs
    if reduction == "batchmean":
        return costs.sum() / targets.shape[0]
    if reduction == "batch":
        return costs / ul.to(costs.dtype)
    raise ValueError(f"Unexpected reduction {reduction}")


def ctc_greedy_tokens(logits, abs_input_lens, blank=0):
    """``(tokens int32 [B,T], ntok int32 [B])`` on the device: per-frame argmax (lowest index among equal scores) over the first
    clamp(len, 0, T) frames, repeats merged, blanks dropped; ``tokens[b, ntok[b]:]`` is -1. One launch, no host read."""
    C.require_gpu(logits, abs_input_lens)
    if logits.dim() != 3:
        raise ValueError(f"ctc: scores must be [B,T,V], got {tuple(logits.shape)}")
    B, T, V = logits.shape
    _check_ranges(B, T, 0, V, blank)
    lg = _padded_rows(logits.detach())
    tlen = abs_input_lens.to(torch.int32).contiguous()
    tokens = torch.empty(B, T, dtype=torch.int32, device=lg.device)
    ntok = torch.empty(B, dtype=torch.int32, device=lg.device)
    with prof.region("ctc_greedy"):
        C.check(C.lib().tsasr_ctc_greedy(C.ptr(lg), C.ptr(tlen), C.ptr(tokens), T, C.ptr(ntok), B, T, V, lg.stride(1), int(blank),
                                         C.io_dtype(lg), C.stream_ptr()), "tsasr_ctc_greedy")
    return tokens, ntok


def ctc_greedy_decode(probabilities, seq_lens, blank_id=-1, return_tensors=False):
    """Drop-in for speechbrain.decoders.ctc.ctc_greedy_decode (decoders/ctc.py:334-376): ``probabilities`` [B,T,V] (scores, probabilities or
    log-probs: only the per-frame argmax matters), RELATIVE ``seq_lens``, a negative ``blank_id`` counts from the last index. Returns a
    list of token lists (one host read of the compacted result); ``return_tensors=True`` returns ``ctc_greedy_tokens``' pair instead and
    stays on the device."""
    from .nnet import abs_lengths_round
    if isinstance(blank_id, int) and blank_id < 0:
        blank_id = probabilities.shape[-1] + blank_id
    tokens, ntok = ctc_greedy_tokens(probabilities, abs_lengths_round(seq_lens, probabilities.shape[1]), blank_id)
    if return_tensors:
        return tokens, ntok
    tokens, ntok = tokens.cpu(), ntok.cpu().tolist()
    return [tokens[b, :n].tolist() for b, n in enumerate(ntok)]


_PADDED_GRADS = {}     # data_ptr -> row length of dlogits buffers just written by tsasr_ctc_loss_bwd (every row whole, pad columns zero)


def _padded_head(weight, VP):
    """The zero-padded bf16 copy [VP,K] of a head's weight and fp32 copy [VP] of its bias, kept with the Parameter: allocated and
    zeroed on first use (an eager step, before any capture), rows [:V] rewritten by every forward."""
    buf = getattr(weight, "_ctc_padded", None)
    if buf is None or buf[0].shape[0] != VP or buf[0].device != weight.device:
        buf = (torch.zeros(VP, weight.shape[1], dtype=torch.bfloat16, device=weight.device),
               torch.zeros(VP, dtype=torch.float32, device=weight.device))
        weight._ctc_padded = buf
    return buf


class _ProjPaddedFn(torch.autograd.Function):
    """scores = x . W^T + b for a bf16 x and a head whose row count V is no multiple of 8 (the character vocabulary's 29): the bf16 MFMA GEMM
    takes matrices of 8-row multiples, so W (its bf16 shadow) and b are padded with zero rows to VP = 8 * ceil(V / 8) per call. The scores
    come out with rows of VP elements - the layout tsasr_ctc_loss_* read in place - and the gradients are the padded GEMMs' first V rows."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from . import ops
        V, K = weight.shape
        VP = (V + 7) // 8 * 8
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        M = x2.shape[0]
        wp, bp = _padded_head(weight, VP)          # zero rows written once; the live rows are refreshed per call (two copies)
        wp[:V].copy_(ops._bf16_weight(weight))
        if bias is not None:
            bp[:V].copy_(bias.detach())
        y = ops.gemm_bf16_fused(x2, wp, M, VP, K, K, K, 0, 0, 1, bias=bp)
        ctx.save_for_backward(x2)
        ctx.wp = wp      # (kept with the Parameter and rewritten by the next forward, after this one's backward)
        ctx.weight, ctx.bias, ctx.xshape = weight, bias, x.shape
        return y.view(*x.shape[:-1], VP)[..., :V]

    @staticmethod
    def backward(ctx, dy):
        from . import ops
        (x2,), wp = ctx.saved_tensors, ctx.wp
        weight, bias = ctx.weight, ctx.bias
        V, K = weight.shape
        VP, M = wp.shape[0], x2.shape[0]
        if (_PADDED_GRADS.pop(dy.data_ptr(), None) == VP and dy.dtype == torch.bfloat16 and dy.shape[-1] == V and dy.stride(-1) == 1
                and all(dy.stride(d) == dy.stride(d + 1) * (VP if d == dy.dim() - 2 else dy.shape[d + 1]) for d in range(dy.dim() - 1))):
            dyp = torch.as_strided(dy, (M, VP), (VP, 1))       # tsasr_ctc_loss_bwd's own buffer: its pad columns are zero already
        else:
            dyp = torch.zeros(M, VP, dtype=torch.bfloat16, device=dy.device)
            dyp[:, :V] = dy.reshape(M, V)
        dx = ops.gemm_bf16(dyp, wp, M, K, VP, VP, K, 0, 1).view(ctx.xshape) if ctx.needs_input_grad[0] else None        # dy . W
        dw = db = None
        if ctx.needs_input_grad[1]:
            dwp = ops.gemm_bf16(dyp, x2, VP, K, M, VP, K, 1, 1, out_dtype=torch.float32)                                # dy^T . x
            dw = ops._pgrad(weight, dwp[:V])
        if bias is not None and ctx.needs_input_grad[2]:
            db = ops._pgrad(bias, ops.colsum(dyp)[:V])
        return dx, dw, db


def project(linear, x):
    """``proj_ctc(x)`` for the CTC branch: the nnet.Linear's own forward where its kernels take the shape (fp32 activations, or a bf16 head
    with a multiple of 8 rows), the padded GEMM above otherwise. Either way hand-written kernels only."""
    w = linear.w
    if x.dtype == torch.bfloat16 and w.weight.shape[0] % 8 and w.weight.shape[1] % 8 == 0:
        C.require_gpu(x)
        return _ProjPaddedFn.apply(x, w.weight, w.bias)
    return linear(x)


class Softmax(torch.nn.Module):
    """speechbrain.nnet.activations.Softmax(apply_log, dim): the reference YAML's `log_softmax` key. The CTC branch here never calls it
    (``ctc_loss`` takes the raw scores); called all the same it is the plain softmax / log-softmax over ``dim`` on the tensor's device."""

    def __init__(self, apply_log=False, dim=-1, reshape=True, dtype=torch.float32):
        super().__init__()
        self.apply_log, self.dim, self.dtype = apply_log, dim, dtype

    def forward(self, x):
        fn = torch.nn.functional.log_softmax if self.apply_log else torch.nn.functional.softmax
        return fn(x, dim=self.dim, dtype=self.dtype)
