"""float64 references, the step checker and the fp32 emulation for the bf16 LSTM recurrence kernels (csrc/lstm.hip). Test infrastructure
only, CPU only; tests/test_lstm_paths_gpu.py applies it to every kernel path, tests/test_lstm_ref_cpu.py proves that it can fail.

STEP CHECK. The recurrence carries a last-bit flip of h_t along, so a free-running comparison cannot tell a flip from a defect. Here every
step is checked GIVEN THE KERNEL'S OWN previous state: forward from its stored h[b, t-1] / c[b, t-1], backward from its stored dgates[b, t+1]
(the dc carry, which is no output, is recomputed in float64 from the kernel's stored gates and c). Every element then has a tight bound, and
a wrong element is reported at the step where it first went wrong:
  forward   pre = gates0 + h_{t-1} . W_hh^T ; i, f, o = sigmoid, g = tanh ; c_t = f c_{t-1} + i g ; h_t = o tanh(c_t)
            activated gates and c_t (fp32): |got - ref| <= delta_fwd ; h_t (bf16): |got - ref| <= 1/2 ulp_bf16(ref) + delta_fwd
  backward  dh_t = dout_t + dgates[t+1] . W_hh ; dc_t = dh_t o (1 - tanh^2 c_t) + dc_{t+1} f_{t+1} ; gate gradients as lstm_cell_bwd_kernel
            |got - ref| <= 1/2 ulp_bf16(ref) + delta_bwd A, A = the same recursion over absolute values (|dout| + sum |dg| |w| ..., every
            difference 1 - x taken as 1 + |x|: _cell_mag)
fp32 io (the step and cell kernels): the operand is rounded to bf16 as the kernels do, and the 1/2 ulp terms drop.
Layouts as in csrc/lstm.hip: gates [B, U, H, 4] gate-minor (i, f, g, o), W_hh [4H, H] and dgates [B, U, 4H] gate-major.

EMULATION. recurrence_fwd / recurrence_bwd / model run free in a chosen dtype: float64 with the kernels' rounding points is the model the
ops-level test compares with, float64 without them equals torch.nn.LSTM, float32 with the kernels' formulas (sigm, tanh_fast of
csrc/lstm.hip:16-17) is the emulation the bounds in TOL are derived from (`python tests/helpers/lstm_ref.py` prints the derivation)."""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GATES = "ifgo"
ROW_FLOOR = 0.1          # per-row relative errors: a row is judged against max(|ref row|, ROW_FLOOR x the RMS row norm) (as attn_ref)


class Mismatch(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------------------------ the case matrix
def matrix():
    """(path, io, B, U, H) of every recurrence case of tests/test_lstm_paths_gpu.py: the smallest shapes at which each dispatch rule, group
    size, ragged group, loader ring (seq1 runs four steps ahead) and K chunk (H = 640: a second 8-step chunk per wave) can fail."""
    m = [("seq1", "bf16", 1, U, 512) for U in (1, 2, 3, 4, 5, 9, 97)]
    m += [("group8", "bf16", 1, U, 512) for U in (1, 2, 3, 4, 5, 9, 97)]                  # the same U with TSASR_LSTM_SEQ1=0
    m += [("group8", "bf16", B, U, 512) for B in (2, 7, 8) for U in (1, 2, 33)]
    m += [("group8", "bf16", B, U, 256) for B in (1, 5, 8) for U in (1, 2, 33)]
    for H in (256, 512):
        m += [("group16", "bf16", B, U, H) for B in (9, 16, 17, 31, 32, 33, 40) for U in (2, 33)]
        m += [("group16", "bf16", 17, 1, H), ("group16", "bf16", 256, 3, H)]
    m += [("step", "bf16", B, U, H) for H in (16, 48, 128, 640) for B in (1, 31, 32, 33, 65) for U in (1, 2, 7)]
    m += [("step", "bf16", 257, 3, 512), ("step_direct", "bf16", 33, 4, 256)]
    m += [("step", "f32", 33, 5, H) for H in (48, 512)]
    m += [("cell", "bf16", 33, 3, 48), ("cell", "f32", 33, 3, 48)]
    return m


OPS_SHAPES = [(1, 9, 28, 512), (7, 5, 28, 256), (33, 6, 28, 512), (33, 4, 12, 48)]      # (B, U, I, H) of the ops-level test


def case_seed(B, U, H):
    return 1000003 * B + 1009 * U + H


def case_inputs(B, U, H, seed=None):
    """gates0 = 0.5 randn fp32 [B, U, H, 4], W_hh = 0.04 randn bf16 [4H, H], dout = randn bf16 [B, U, H] (the scales of the existing tests)."""
    g = torch.Generator().manual_seed(case_seed(B, U, H) if seed is None else seed)
    gates0 = torch.randn(B, U, H, 4, generator=g) * 0.5
    whh = (torch.randn(4 * H, H, generator=g) * 0.04).to(BF16)
    dout = torch.randn(B, U, H, generator=g).to(BF16)
    return gates0, whh, dout


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def bf(x):
    """round to bf16 (nearest-even), keep the dtype"""
    return x.to(BF16).to(x.dtype)


def half_ulp_bf16(ref):
    """half a unit in the last place of bf16 at |ref|: 2^(floor(log2 |ref|) - 8); 0 at 0"""
    r = ref.abs().to(F64)
    _, e = torch.frexp(r)                                       # |ref| = m 2^e, m in [0.5, 1)
    return torch.where(r > 0, torch.ldexp(torch.ones_like(r), e - 9), torch.zeros_like(r))


def _sig(x, fast):
    return 1.0 / (1.0 + torch.exp(-x)) if fast else torch.sigmoid(x)


def _tanh(x, fast):
    if not fast:
        return torch.tanh(x)
    e = torch.exp(-2.0 * x.abs())
    t = (1.0 - e) / (1.0 + e)
    return torch.where(x < 0, -t, t)


def _minor(rec, H):
    """[..., 4H] gate-major -> [..., H, 4]"""
    return rec.reshape(*rec.shape[:-1], 4, H).transpose(-1, -2)


def _cell_bwd(act, cn, cp, dh, dc_in, fast=False):
    """lstm_cell_bwd_kernel's formulas: -> (dgates [..., 4, H] gate-major, dc carry out = dc f)"""
    gi, gf, gg, go = act.unbind(-1)
    tc = _tanh(cn, fast)
    dc = dh * go * (1.0 - tc * tc) + dc_in
    dg = torch.stack([dc * gg * gi * (1.0 - gi), dc * cp * gf * (1.0 - gf), dc * gi * (1.0 - gg * gg), dh * tc * go * (1.0 - go)], dim=-2)
    return dg, dc * gf


def _cell_mag(act, cn, cp, adh, adc_in):
    """The magnitude companion of _cell_bwd: every term by absolute value and every difference 1 - x as 1 + |x| - the size of the numbers the
    kernel adds, which is what its fp32 rounding is relative to. tanh_fast(c) = (1 - e) / (1 + e) is such a difference too: its error is
    absolute (2^-24 of 1), not relative to a tanh(c) near zero, so its companion is 1."""
    gi, gf, gg, go = act.abs().unbind(-1)
    tc2 = torch.tanh(cn) ** 2
    adc = adh * go * (1.0 + tc2) + adc_in
    A = torch.stack([adc * gg * gi * (1.0 + gi), adc * cp.abs() * gf * (1.0 + gf), adc * gi * (1.0 + gg * gg), adh * go * (1.0 + go)], dim=-2)
    return A, adc * gf


# ------------------------------------------------------------------------------------------------------------------ free-running recurrence
def recurrence_fwd(gates0, whh, io="bf16", dtype=F64, fast=False):
    """Free-running forward in `dtype`. io: "bf16" (h stored and fed back in bf16), "f32" (h stored whole, the operand rounded to bf16: the
    step kernels' fp32 io), "exact" (no rounding). whh None: the pre-activations are given whole (the cell kernels).
    -> act [B, U, H, 4], c [B, U, H], h [B, U, H] in `dtype`."""
    B, U, H, _ = gates0.shape
    g0 = gates0.to(dtype)
    wT = None if whh is None else whh.to(dtype).t()
    act, c, h = torch.empty_like(g0), g0.new_empty(B, U, H), g0.new_empty(B, U, H)
    hp, cp = g0.new_zeros(B, H), g0.new_zeros(B, H)
    for t in range(U):
        pre = g0[:, t] if (wT is None or t == 0) else g0[:, t] + _minor(hp @ wT, H)
        gi, gf, go = _sig(pre[..., 0], fast), _sig(pre[..., 1], fast), _sig(pre[..., 3], fast)
        gg = _tanh(pre[..., 2], fast)
        cp = gf * cp + gi * gg
        ht = go * _tanh(cp, fast)
        act[:, t], c[:, t] = torch.stack([gi, gf, gg, go], dim=-1), cp
        h[:, t] = bf(ht) if io == "bf16" else ht
        hp = h[:, t] if io == "exact" else bf(h[:, t])
    return act, c, h


def recurrence_bwd(act, c, dout, whh, io="bf16", dtype=F64, fast=False, dh_rec=None):
    """Free-running backward in `dtype` -> dgates [B, U, 4H] gate-major (rounded to bf16 when io == "bf16"). dh_rec [B, U, H]: the recurrent
    term given by the caller instead of dgates[t+1] . W_hh (the cell kernels)."""
    B, U, H, _ = act.shape
    a, cc, do = act.to(dtype), c.to(dtype), dout.to(dtype)
    w = None if whh is None else whh.to(dtype)
    dg = a.new_empty(B, U, 4 * H)
    dcar = a.new_zeros(B, H)
    for t in range(U - 1, -1, -1):
        dh = do[:, t]
        if t < U - 1:
            nxt = dg[:, t + 1] if io == "exact" else bf(dg[:, t + 1])
            dh = dh + (dh_rec[:, t].to(dtype) if dh_rec is not None else nxt @ w)
        cp = cc[:, t - 1] if t > 0 else torch.zeros_like(cc[:, 0])
        d4, dcar = _cell_bwd(a[:, t], cc[:, t], cp, dh, dcar, fast)
        d4 = d4.reshape(B, 4 * H)
        dg[:, t] = bf(d4) if io == "bf16" else d4
    return dg


# ------------------------------------------------------------------------------------------------------------------ step references
def step_fwd_ref(gates0, whh, h_k, c_k, io="bf16"):
    """float64 step reference of every (b, t) from the kernel's own previous state -> act [B, U, H, 4], c, h [B, U, H]"""
    B, U, H, _ = gates0.shape
    pre = gates0.to(F64).clone()
    if whh is not None and U > 1:
        hp = h_k[:, :-1].to(F64) if io == "bf16" else bf(h_k[:, :-1].to(F32)).to(F64)
        pre[:, 1:] += _minor(hp @ whh.to(F64).t(), H)
    cp = torch.zeros(B, U, H, dtype=F64)
    cp[:, 1:] = c_k[:, :-1].to(F64)
    gi, gf, go, gg = torch.sigmoid(pre[..., 0]), torch.sigmoid(pre[..., 1]), torch.sigmoid(pre[..., 3]), torch.tanh(pre[..., 2])
    c = gf * cp + gi * gg
    return torch.stack([gi, gf, gg, go], dim=-1), c, go * torch.tanh(c)


def step_bwd_ref(act_k, c_k, dout, whh, dg_k, io="bf16", dh_rec=None):
    """float64 step reference of dgates from the kernel's own stored gates, c and dgates[t+1] -> (ref [B, U, 4H], A [B, U, 4H]): A is the
    magnitude companion - the same recursion over absolute values, what an error relative to the operands is measured in."""
    B, U, H, _ = act_k.shape
    a, cc, do = act_k.to(F64), c_k.to(F64), dout.to(F64)
    dh, adh = do.clone(), do.abs()
    if U > 1:
        if dh_rec is not None:
            dh[:, :-1] += dh_rec[:, :-1].to(F64)
            adh[:, :-1] += dh_rec[:, :-1].to(F64).abs()
        else:
            nxt = dg_k[:, 1:].to(F64) if io == "bf16" else bf(dg_k[:, 1:].to(F32)).to(F64)
            w = whh.to(F64)
            dh[:, :-1] += nxt @ w
            adh[:, :-1] += nxt.abs() @ w.abs()
    cp = torch.zeros_like(cc)
    cp[:, 1:] = cc[:, :-1]
    ref, A = torch.empty(B, U, 4, H, dtype=F64), torch.empty(B, U, 4, H, dtype=F64)
    dcar, acar = torch.zeros(B, H, dtype=F64), torch.zeros(B, H, dtype=F64)
    for t in range(U - 1, -1, -1):
        ref[:, t], dcar = _cell_bwd(a[:, t], cc[:, t], cp[:, t], dh[:, t], dcar)
        A[:, t], acar = _cell_mag(a[:, t], cc[:, t], cp[:, t], adh[:, t], acar)
    return ref.reshape(B, U, 4 * H), A.reshape(B, U, 4 * H)


# ------------------------------------------------------------------------------------------------------------------ the checker
def _where(b, t, unit, BR, wg_units):
    return f"exchange group {b // BR} row {b % BR}, workgroup {unit // wg_units} (units {unit // wg_units * wg_units}..+{wg_units - 1})"


def suspect_pieces(resid, whh_rows, H):
    """Which 8-unit pieces of the operand h_{t-1} explain a residual of pre-activations? resid [n] over the rows `whh_rows` [n, H] of W_hh:
    least squares for the operand error dh, pieces holding more than a quarter of its largest entry. Under-determined (n < H): None."""
    if whh_rows.shape[0] < H:
        return None
    dh = torch.linalg.lstsq(whh_rows, resid[:, None]).solution[:, 0].abs()
    piece = dh.reshape(H // 8, 8).max(dim=1).values
    return [int(p) for p in torch.nonzero(piece > 0.25 * piece.max())[:, 0]]


def _report(what, name, bad, diff, bound, got, ref, order_desc, BR, wg_units, gate_of, extra=""):
    """bad [B, U, ...]: the first (in the recurrence's order: t ascending forward, descending backward) and the worst element"""
    idx = torch.nonzero(bad)
    tkey = -idx[:, 1] if order_desc else idx[:, 1]
    first = idx[torch.argsort(tkey * (1 << 40) + idx[:, 0] * (1 << 20) + idx[:, 2] * 8 + (idx[:, 3] if idx.shape[1] > 3 else 0), stable=True)[0]]
    excess = torch.where(bad, diff - bound, torch.full_like(diff, -1.0))
    worst = torch.nonzero(excess == excess.max())[0]

    def show(ix):
        b, t = int(ix[0]), int(ix[1])
        unit, gate = gate_of(ix)
        key = tuple(int(v) for v in ix)
        g = f", gate={GATES[gate]}" if gate is not None else ""
        return (f"(b={b}, t={t}, unit={unit}{g}) = {_where(b, t, unit, BR, wg_units)}: got {float(got[key])!r}, want {float(ref[key])!r}, "
                f"|diff| {float(diff[key]):.3e} > bound {float(bound[key]):.3e}")
    return f"{what} {name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {show(first)}; worst at {show(worst)}{extra}"


def check_fwd(gates0, whh, act_k, c_k, h_k, delta, io="bf16", BR=16, wg_units=32, what=""):
    """Step check of a forward result (all CPU tensors). Raises Mismatch naming the first and the worst element and the structure they
    belong to. -> {"act", "c": worst |diff|, "h": worst excess over 1/2 ulp, "h_flips": share of h not the nearest bf16 of the reference}."""
    B, U, H, _ = gates0.shape
    act_r, c_r, h_r = step_fwd_ref(gates0, whh, h_k, c_k, io)
    stats = {}
    for name, got, ref in (("gates", act_k, act_r), ("c", c_k, c_r), ("h", h_k, h_r)):
        got = got.to(F64)
        diff = (got - ref).abs()
        diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
        slack = half_ulp_bf16(ref) if (name == "h" and io == "bf16") else torch.zeros_like(ref)
        bound = slack + delta
        stats["act" if name == "gates" else name] = float((diff - slack).clamp_min(0).max())
        bad = diff > bound
        if bad.any():
            gate_of = (lambda ix: (int(ix[2]), int(ix[3]))) if name == "gates" else (lambda ix: (int(ix[2]), None))
            extra = ""
            if name == "gates" and whh is not None:
                # the operand error behind the first failing row: pre-activations back from the activated gates, over the failing units
                idx = torch.nonzero(bad)
                t0 = int(idx[:, 1].min())
                b0 = int(idx[idx[:, 1] == t0][:, 0].min())
                if t0 > 0:
                    units = torch.unique(idx[(idx[:, 1] == t0) & (idx[:, 0] == b0)][:, 2])
                    g, r = got[b0, t0, units].clamp(-1 + 1e-15, 1 - 1e-15), ref[b0, t0, units]
                    inv = lambda a: torch.stack([torch.logit(a[:, 0]), torch.logit(a[:, 1]), torch.atanh(a[:, 2]), torch.logit(a[:, 3])], 1)  # noqa: E731
                    resid = (inv(g) - inv(r)).t().reshape(-1)                       # [4 x units], gate-major
                    rows = (torch.arange(4)[:, None] * H + units[None, :]).reshape(-1)
                    pieces = suspect_pieces(torch.nan_to_num(resid), whh.to(F64)[rows], H)
                    extra = (f"; operand h[b={b0}, t={t0 - 1}]: " + ("not identifiable from these units" if pieces is None else
                             f"suspect 8-unit piece(s) {pieces} (units {[8 * p for p in pieces]}..+7)"))
            raise Mismatch(_report(what, name, bad, diff, bound, got, ref, False, BR, wg_units, gate_of, extra))
    if io == "bf16":
        stats["h_flips"] = float((h_k.to(BF16).view(torch.int16) != h_r.to(F32).to(BF16).view(torch.int16)).double().mean())
    return stats


def check_bwd(act_k, c_k, dout, whh, dg_k, delta, io="bf16", BR=16, wg_units=32, what="", dh_rec=None):
    """Step check of a backward result. -> {"dgates": worst (|diff| - 1/2 ulp) / A, "dg_flips": share not the nearest bf16 of the reference}"""
    B, U, H, _ = act_k.shape
    ref, A = step_bwd_ref(act_k, c_k, dout, whh, dg_k, io, dh_rec)
    got = dg_k.to(F64)
    diff = (got - ref).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    slack = half_ulp_bf16(ref) if io == "bf16" else torch.zeros_like(ref)
    bound = slack + delta * A
    stats = {"dgates": float(((diff - slack).clamp_min(0) / A.clamp_min(1e-300)).max())}
    bad = diff > bound
    if bad.any():
        raise Mismatch(_report(what, "dgates", bad, diff, bound, got, ref, True, BR, wg_units, lambda ix: (int(ix[2]) % H, int(ix[2]) // H)))
    if io == "bf16":
        stats["dg_flips"] = float((dg_k.to(BF16).view(torch.int16) != ref.to(F32).to(BF16).view(torch.int16)).double().mean())
    return stats


# ------------------------------------------------------------------------------------------------------------------ ops._LstmFn, free-running
def onehot_rows(tokens, I, blank):
    """The one-hot rows of ops.lstm_onehot: token k -> column k - 1 above `blank`, k below it; the blank and negative ids -> no column."""
    col = torch.where(tokens > blank, tokens - 1, tokens)
    col = torch.where((tokens == blank) | (tokens < 0), torch.full_like(col, -1), col)
    return (col[..., None] == torch.arange(I)).to(F64)


def model(x, w_ih, w_hh, b_ih, b_hh, dout, dtype=F64, rounding=True, fast=False, tokens=None, blank=0):
    """ops._LstmFn run free in `dtype`, forward and backward. rounding: its rounding points - x and W_ih in bf16, the bias as a bf16 high +
    low part (the padding columns of the input GEMM), W_hh in bf16, h_t in bf16, dout and dgates in bf16, the weight-gradient GEMMs and dx
    over the bf16 dgates, dx stored in bf16. tokens [B, U] (ops.lstm_onehot): the input projection is a column of the fp32 W_ih plus the
    fp32 biases, not rounded; no dx. Without rounding this is torch.nn.LSTM."""
    r = bf if rounding else (lambda v: v)
    H = w_hh.shape[1]
    wi, wh, bias = w_ih.to(dtype), r(w_hh.to(dtype)), (b_ih.to(dtype) + b_hh.to(dtype))
    if tokens is not None:
        xin = onehot_rows(tokens, w_ih.shape[1], blank).to(dtype)
        g0 = xin @ wi.t() + bias
    else:
        xin, wi = r(x.to(dtype)), r(wi)
        hi = r(bias)
        g0 = xin @ wi.t() + (hi + r(bias - hi))
    B, U, I = xin.shape
    io = "bf16" if rounding else "exact"
    act, c, h = recurrence_fwd(_minor(g0, H), wh, io, dtype, fast)
    do = r(dout.to(dtype))
    dg = recurrence_bwd(act, c, do, wh, io, dtype, fast)
    hp = torch.zeros_like(h)
    hp[:, 1:] = h[:, :-1]
    dg2 = dg.reshape(B * U, 4 * H)
    db = dg2.sum(0)
    out = {"out": h, "hn": h[:, -1], "cn": c[:, -1], "dW_hh": dg2.t() @ hp.reshape(B * U, H), "dW_ih": dg2.t() @ xin.reshape(B * U, I),
           "db_ih": db, "db_hh": db}
    if tokens is None:
        out["dx"] = r(dg2 @ wi).reshape(B, U, I)
    return {k: v.to(F64) for k, v in out.items()}


def row_view(name, t):
    """out / dx: one row per (b, t); dW_hh / dW_ih / db_*: one row per gate row of the 4H"""
    return t.reshape(-1, 1) if name.startswith("db") else t.reshape(-1, t.shape[-1])


def row_errors(name, got, ref):
    """per-row relative L2 of `got` against `ref` (float64), rows judged against max(|ref row|, ROW_FLOOR x the RMS row norm)"""
    g, r = row_view(name, got.to(F64)), row_view(name, ref.to(F64))
    rn = r.norm(dim=1)
    floor = ROW_FLOOR * float(rn.pow(2).mean().sqrt())
    return (g - r).norm(dim=1) / rn.clamp_min(max(floor, 1e-300))


def check_rows(name, got, ref, bound, what=""):
    e = row_errors(name, got, ref)
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    if float(e.max()) > bound:
        w = int(e.argmax())
        raise Mismatch(f"{what} {name}: {int((e > bound).sum())} of {e.numel()} rows above {bound:.3e}; first row {int(torch.nonzero(e > bound)[0])}, "
                       f"worst row {w}: {float(e[w]):.3e}")
    return float(e.max())


# ------------------------------------------------------------------------------------------------------------------ the bounds
# delta_fwd / delta_bwd = 16 x the worst step-check distance of the fp32 emulation (run free, then checked like a kernel) over matrix():
# the device's v_exp_f32 / v_rcp_f32 are 1-ulp approximations and the MFMA sums in another order, neither of which the CPU emulation shares.
# ops rows = 4 x the worst per-row distance between the fp32 emulation run free and the float64 model over OPS_SHAPES; "model" is the
# model's own worst per-row distance to pure-float64 torch.nn.LSTM, which every bound must stay below a quarter of.
# Each entry: bound, then the CPU measurement it came from; the worst values measured on the MI355X per path are in GPU_MEASURED.
TOL = {
    "delta_fwd": (3.2e-6, 1.99e-7),      # absolute, on the activated gates, c and (over 1/2 ulp) h
    "delta_bwd": (3.4e-6, 2.11e-7),      # relative to A, on dgates (over 1/2 ulp)
    "flips": 0.01,                       # share of h / dgates elements that are not the nearest bf16 of the reference, per case (the
                                         # emulation: at most 9.7e-4 of h, 4.9e-4 of dgates)
    # quantity: (bound, emulation vs model, model vs pure float64). NO bound is below a quarter of the third figure, and with these shapes
    # none can be: one bf16 flip in a row of 48 h values, or in a sum over B U = 9 samples, is already 6e-4 .. 1.5e-3 of the row, a quarter
    # or more of what rounding EVERY element (the model's distance to float64) amounts to. The bounds still see what the whole-tensor norms
    # (1e-2 / 3e-2) could not: one wrong row, step or gate row.
    "ops": {"out": (2.4e-3, 5.91e-4, 1.90e-3), "dx": (1.23e-2, 3.06e-3, 3.70e-3), "dW_hh": (5.0e-3, 1.25e-3, 5.08e-3),
            "dW_ih": (6.3e-3, 1.57e-3, 3.26e-3), "db_ih": (2.8e-2, 6.91e-3, 4.41e-2), "db_hh": (2.8e-2, 6.91e-3, 4.41e-2)},
}
# worst values measured on the MI355X over each path's cases (act / c / h over 1/2 ulp: absolute; dgates over 1/2 ulp: relative to A)
GPU_MEASURED = {
    "seq1 bf16": {"act": 1.48e-7, "c": 1.48e-7, "h": 1.01e-8, "dgates": 4.52e-9, "h_flips": 6.0e-5, "dg_flips": 9.8e-5},
    "group8 bf16": {"act": 1.80e-7, "c": 1.68e-7, "h": 5.93e-8, "dgates": 1.58e-8, "h_flips": 4.9e-4, "dg_flips": 2.0e-4},
    "group16 bf16": {"act": 1.95e-7, "c": 2.04e-7, "h": 4.59e-8, "dgates": 6.54e-8, "h_flips": 4.3e-4, "dg_flips": 1.1e-4},
    "step bf16": {"act": 1.44e-7, "c": 1.58e-7, "h": 3.74e-8, "dgates": 9.38e-8, "h_flips": 9.6e-4, "dg_flips": 2.9e-4},
    "step_direct bf16": {"act": 1.34e-7, "c": 1.22e-7, "h": 2.67e-9, "dgates": 2.78e-9, "h_flips": 3.0e-5, "dg_flips": 3.7e-5},
    "step f32": {"act": 1.46e-7, "c": 1.40e-7, "h": 1.11e-7, "dgates": 1.97e-7},
    "cell bf16": {"act": 1.13e-7, "c": 1.04e-7, "h": 1.62e-8, "dgates": 0.0, "h_flips": 2.1e-4, "dg_flips": 0.0},
    "cell f32": {"act": 1.13e-7, "c": 1.04e-7, "h": 1.07e-7, "dgates": 1.44e-7},
    # ops level, worst per-row relative L2 over the five cases (the one-hot case has no dx)
    "ops": {"out": 9.67e-4, "dx": 1.14e-3, "dW_hh": 1.25e-3, "dW_ih": 1.57e-3, "db_ih": 3.09e-3, "db_hh": 3.09e-3},
}


def derive(verbose=True):
    """The CPU measurements behind TOL (minutes of CPU)."""
    worst = {"fwd": 0.0, "bwd": 0.0, "h_flips": 0.0, "dg_flips": 0.0}
    for path, io, B, U, H in matrix():
        gates0, whh, dout = case_inputs(B, U, H)
        w = None if path == "cell" else whh
        g = torch.Generator().manual_seed(7)
        dh_rec = torch.randn(B, U, H, generator=g) * 0.3 if path == "cell" else None
        do = dout if io == "bf16" else dout.float()
        act, c, h = recurrence_fwd(gates0, w, io, F32, fast=True)
        dg = recurrence_bwd(act, c, do, w, io, F32, fast=True, dh_rec=dh_rec)
        sf = check_fwd(gates0, w, act, c, h, float("inf"), io)
        sb = check_bwd(act, c, do, w, dg, float("inf"), io, dh_rec=dh_rec)
        worst["fwd"] = max(worst["fwd"], sf["act"], sf["c"], sf["h"])
        worst["bwd"] = max(worst["bwd"], sb["dgates"])
        worst["h_flips"] = max(worst["h_flips"], sf.get("h_flips", 0.0))
        worst["dg_flips"] = max(worst["dg_flips"], sb.get("dg_flips", 0.0))
        if verbose:
            print(f"{path:12s} {io} B={B:3d} U={U:2d} H={H:3d} fwd {max(sf['act'], sf['c'], sf['h']):.2e} bwd {sb['dgates']:.2e} "
                  f"flips {sf.get('h_flips', 0):.1e} {sb.get('dg_flips', 0):.1e}", flush=True)
    ops = {}
    for B, U, I, H in OPS_SHAPES:
        for onehot in ((False, True) if (B, U) == (33, 6) else (False,)):
            args, kw = ops_inputs(B, U, I, H, onehot)
            ref, emu, pure = model(*args, **kw), model(*args, dtype=F32, fast=True, **kw), model(*args, rounding=False, **kw)
            for k in ref:
                if k in ("hn", "cn"):
                    continue
                e, p = ops.setdefault(k, [0.0, float("inf")])
                ops[k] = [max(e, float(row_errors(k, emu[k], ref[k]).max())), min(p, float(row_errors(k, ref[k], pure[k]).max()))]
    if verbose:
        print("worst over the matrix:", worst)
        print(f"delta_fwd = {16 * worst['fwd']:.3e}, delta_bwd = {16 * worst['bwd']:.3e}")
        for k, (e, p) in ops.items():
            print(f"ops {k}: emulation vs model {e:.3e} -> bound {4 * e:.3e}; model vs pure float64 {p:.3e} (quarter {p / 4:.3e}) "
                  f"{'ok' if 4 * e < p / 4 else 'NOT below a quarter'}")
    return worst, ops


def ops_inputs(B, U, I, H, onehot=False):
    """(x, w_ih, w_hh, b_ih, b_hh, dout), kwargs of model() for an ops-level case: torch.nn.LSTM's own initialisation, dense random bf16 x
    (or token ids over V = I + 1 with blank 0, including the blank, V - 1 and a negative id)."""
    g = torch.Generator().manual_seed(case_seed(B, U, H) + I)
    k = 1.0 / math.sqrt(H)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    w_ih, w_hh, b_ih, b_hh = u(4 * H, I), u(4 * H, H), u(4 * H), u(4 * H)
    x = torch.randn(B, U, I, generator=g).to(BF16)
    dout = torch.randn(B, U, H, generator=g).to(BF16)
    kw = {}
    if onehot:
        tok = torch.randint(0, I + 1, (B, U), generator=g)
        tok[0, 0], tok[0, 1], tok[1, 0], tok[1, 1] = 0, I, -1, 1
        kw = {"tokens": tok, "blank": 0}
    return (x, w_ih, w_hh, b_ih, b_hh, dout), kw


if __name__ == "__main__":
    derive()
