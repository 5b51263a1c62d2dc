"""The bf16 LSTM recurrence kernels (csrc/lstm.hip), path by path through the C-ABI, step by step against float64 (tests/helpers/lstm_ref.py).

    seq1     lstm_seq1_{fwd,bwd}_kernel<512>           bf16, B = 1, H = 512, TSASR_LSTM_SEQ1 not 0
    group8   lstm_seq_{fwd,bwd}_kernel<H, 8>            bf16, H in {256, 512}, B <= 8
    group16  lstm_seq_{fwd,bwd}_kernel<H, 16>           bf16, H in {256, 512}, 9 <= B <= 256, ceil(B / 16) H / 32 <= the device's CUs
    step     lstm_step_{fwd,bwd}_kernel<T>, per step    any other H % 16 == 0, B > 256, fp32 io
    cell     lstm_cell_{fwd,bwd}_kernel<T>              (exported; pre-activations given whole)

Every case: inputs seeded per case (gates0 = 0.5 randn, W_hh = 0.04 randn bf16, dout = randn bf16), the dispatch rule mirrored by
expected_path() and asserted against tsasr_lstm_seq_persistent; h, c, gates and dgates carry two guard rows of a sentinel behind row B - 1
and start as NaN; the workspace is filled with 0xFF before each launch and the error words (odd words of its first 256 bytes) must be 0
afterwards on the persistent paths (the per-step kernels never touch that block); forward, step check, backward on the forward's outputs,
step check. Each step is judged from the kernel's own previous state, so the bounds (lstm_ref.TOL: 16 x the fp32 emulation's own distance
to float64) are a few fp32 epsilons plus half a bf16 ulp, and a failure names the first wrong (b, t, unit, gate) with its exchange group,
workgroup and - where it can be told - the 8-unit piece of h_{t-1} it came from. The share of h / dgates elements that are not the nearest
bf16 of the reference stays below 1 % per case.

Ops level (ops.lstm / ops.lstm_onehot with requires_grad on x, so that the bf16 dx GEMM of _LstmFn.backward runs): per-row relative L2
against the free-running float64 model with the kernels' rounding points."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SENT = -7.0                               # guard rows (representable in bf16; no output reaches it: |h| < 1, gates in (-1, 1))
NAN = float("nan")
D_FWD, D_BWD, FLIPS = LR.TOL["delta_fwd"][0], LR.TOL["delta_bwd"][0], LR.TOL["flips"]


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------ the host's dispatch rule (csrc/lstm.hip)
def expected_path(B, H, io, cus, seq1_env):
    """seq_persistent_ok + lq_seq1 + lq_br"""
    BR = 8 if B <= 8 else 16
    G = cdiv(B, BR)
    if not (io == "bf16" and H in (256, 512) and G <= 16 and G * (H // 32) <= cus):
        return "step"
    if B == 1 and H == 512 and seq1_env != "0":
        return "seq1"
    return "group8" if BR == 8 else "group16"


STRUCTURE = {"seq1": (1, 8), "group8": (8, 32), "group16": (16, 32), "step": (32, 16), "step_direct": (32, 16), "cell": (32, 16)}   # (BR, units per workgroup)


def require_path(C, path, B, H, io, cus, monkeypatch):
    """Set the per-call switch, assert what the ABI shows of the dispatch, and skip (never pass on another path) when this device has too
    few CUs for the case to reach its path."""
    env = "0" if (path == "group8" and B == 1 and H == 512) else "1"
    monkeypatch.setenv("TSASR_LSTM_SEQ1", env)
    want = expected_path(B, H, io, cus, env)
    assert C.lib().tsasr_lstm_seq_persistent(B, H, C.BF16 if io == "bf16" else C.F32) == (0 if want == "step" else 1), (path, B, H, io, cus)
    if want != path:
        full = expected_path(B, H, io, 256, env)
        assert full == path, f"the matrix expects {path} for B={B} H={H} {io}, the rule gives {full} on a full device"
        pytest.skip(f"{path} needs {cdiv(B, 8 if B <= 8 else 16) * (H // 32)} CUs for B={B} H={H}, this device exposes {cus}")


# ------------------------------------------------------------------------------------------------------ one case
class Case:
    def __init__(self, C, path, io, B, U, H):
        self.C, self.lib, self.path, self.io, self.B, self.U, self.H = C, C.lib(), path, io, B, U, H
        self.iod, self.dt = (C.BF16, BF16) if io == "bf16" else (C.F32, F32)
        self.gates0, self.whh, dout = LR.case_inputs(B, U, H)
        self.dout = dout.to(self.dt)
        self.what = f"{path} {io} B={B} U={U} H={H}"
        self.BR, self.wg = STRUCTURE[path]
        self.whh_d, self.whhT_d, self.dout_d = self.whh.to(DEV), self.whh.t().contiguous().to(DEV), self.dout.to(DEV)
        self.gates, self.c = self.guarded((H, 4), F32, self.gates0), self.guarded((H,), F32, NAN)
        self.h, self.dgates = self.guarded((H,), self.dt, NAN), self.guarded((4 * H,), self.dt, NAN)
        self.nb = self.lib.tsasr_lstm_seq_workspace_bytes(B, U, H)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=DEV)

    def guarded(self, tail, dtype, fill):
        t = torch.full((self.B + 2, self.U, *tail), SENT, dtype=dtype, device=DEV)
        t[:self.B] = fill.to(DEV) if isinstance(fill, torch.Tensor) else fill
        return t

    def launched(self, name, call, outputs):
        """one launch over a workspace of 0xFF; afterwards: no error word, guard rows intact, no NaN left in what it writes"""
        self.ws.fill_(0xFF)
        call()
        torch.cuda.synchronize()
        if self.path in ("seq1", "group8", "group16"):
            err = self.ws[:256].view(torch.int32)[1::2].cpu()
            assert int((err != 0).sum()) == 0, f"{self.what} {name}: error words raised: {err.tolist()}"
        for k in ("gates", "c", "h", "dgates"):
            t = getattr(self, k)
            assert bool((t[self.B:] == SENT).all()), f"{self.what} {name}: guard rows of {k} were written"
        for k in outputs:
            n = int(torch.isnan(getattr(self, k)[:self.B].float()).sum())
            assert n == 0, f"{self.what} {name}: {n} NaN left in {k}"

    def seq_fwd(self):
        C, p = self.C, self.C.ptr
        C.check(self.lib.tsasr_lstm_seq_fwd(p(self.gates), p(self.c), p(self.h), p(self.whh_d), self.B, self.U, self.H, self.iod, p(self.ws), self.nb,
                                            C.stream_ptr()), "tsasr_lstm_seq_fwd")

    def seq_bwd(self):
        C, p = self.C, self.C.ptr
        C.check(self.lib.tsasr_lstm_seq_bwd(p(self.gates), p(self.c), p(self.dout_d), p(self.dgates), p(self.whhT_d), self.B, self.U, self.H, self.iod,
                                            p(self.ws), self.nb, C.stream_ptr()), "tsasr_lstm_seq_bwd")

    def step_fwd(self):
        C, p = self.C, self.C.ptr
        for t in range(self.U):
            C.check(self.lib.tsasr_lstm_step_fwd(p(self.gates), p(self.c), p(self.h), p(self.whh_d), self.B, self.U, self.H, t, self.iod, C.stream_ptr()),
                    "tsasr_lstm_step_fwd")

    def step_bwd(self):
        C, p = self.C, self.C.ptr
        dc_io = torch.full((self.B, self.H), NAN, dtype=F32, device=DEV)          # step U - 1 must not read it
        for t in range(self.U - 1, -1, -1):
            C.check(self.lib.tsasr_lstm_step_bwd(p(self.gates), p(self.c), p(self.dout_d), p(self.dgates), p(self.whhT_d), p(dc_io), self.B, self.U,
                                                 self.H, t, self.iod, C.stream_ptr()), "tsasr_lstm_step_bwd")

    def cell_fwd(self):
        C, p = self.C, self.C.ptr
        for t in range(self.U):
            C.check(self.lib.tsasr_lstm_cell_fwd(p(self.gates), p(self.c), p(self.h), self.B, self.U, self.H, t, self.iod, C.stream_ptr()),
                    "tsasr_lstm_cell_fwd")

    def cell_bwd(self):
        C, p = self.C, self.C.ptr
        dc_io = torch.full((self.B, self.H), NAN, dtype=F32, device=DEV)
        rec = self.dh_rec.transpose(0, 1).contiguous().to(DEV)                    # [U, B, H]: one [B, H] plane per step
        rec[self.U - 1] = NAN                                                     # the last step has no recurrent term
        for t in range(self.U - 1, -1, -1):
            C.check(self.lib.tsasr_lstm_cell_bwd(p(self.gates), p(self.c), p(self.dout_d), p(rec[t]), p(dc_io), p(self.dgates), self.B, self.U, self.H,
                                                 t, self.iod, C.stream_ptr()), "tsasr_lstm_cell_bwd")

    def run(self):
        """forward, step check, backward on the forward's outputs, step check -> the kernel's outputs on the CPU"""
        B = self.B
        fwd, bwd = {"step_direct": (self.step_fwd, self.step_bwd), "cell": (self.cell_fwd, self.cell_bwd)}.get(self.path, (self.seq_fwd, self.seq_bwd))
        cell = self.path == "cell"
        self.dh_rec = torch.randn(B, self.U, self.H, generator=torch.Generator().manual_seed(7)) * 0.3 if cell else None
        w = None if cell else self.whh
        self.launched("fwd", fwd, ("gates", "c", "h"))
        act, c, h = self.gates[:B].cpu(), self.c[:B].cpu(), self.h[:B].cpu()
        sf = LR.check_fwd(self.gates0, w, act, c, h, D_FWD, self.io, self.BR, self.wg, self.what + " fwd")
        kept = [t.clone() for t in (self.gates, self.c, self.h)]
        self.launched("bwd", bwd, ("dgates",))
        assert all(torch.equal(a.view(torch.int32) if a.dtype == F32 else a.view(torch.int16), b.view(torch.int32) if b.dtype == F32 else b.view(torch.int16))
                   for a, b in zip(kept, (self.gates, self.c, self.h))), f"{self.what}: the backward changed a forward output"
        dg = self.dgates[:B].cpu()
        sb = LR.check_bwd(act, c, self.dout, w, dg, D_BWD, self.io, self.BR, self.wg, self.what + " bwd", dh_rec=self.dh_rec)
        print(f"\nLSTMSTAT {self.path} {self.io} {B} {self.U} {self.H} act {sf['act']:.3e} c {sf['c']:.3e} h {sf['h']:.3e} dgates {sb['dgates']:.3e} "
              f"h_flips {sf.get('h_flips', 0):.3e} dg_flips {sb.get('dg_flips', 0):.3e}")
        if self.io == "bf16":
            assert sf["h_flips"] <= FLIPS, f"{self.what}: {sf['h_flips']:.3%} of h is not the nearest bf16 of the reference"
            assert sb["dg_flips"] <= FLIPS, f"{self.what}: {sb['dg_flips']:.3%} of dgates is not the nearest bf16 of the reference"
        return act, c, h, dg


def cases(path, io="bf16"):
    return [pytest.param(B, U, H, id=f"B{B}-U{U}-H{H}") for p, i, B, U, H in LR.matrix() if p == path and i == io]


# ------------------------------------------------------------------------------------------------------ the recurrence paths
@pytest.mark.parametrize("U", [1, 2, 3, 4, 5, 9, 97])
def test_seq1_and_its_exchange_group_route(C, cus, monkeypatch, U):
    """B = 1, H = 512: the wave-autonomous kernels (a loader ring four steps ahead: U <= 5 ends inside its prologue; arrival by the 0xFFFF
    fill of the outputs, which the launch lays over the caller's NaN itself) and the same U through group8 (TSASR_LSTM_SEQ1=0, read per
    call), BOTH against the reference; the forward of the two still bit for bit equal."""
    assert ("seq1", "bf16", 1, U, 512) in LR.matrix() and ("group8", "bf16", 1, U, 512) in LR.matrix()
    outs = {}
    for path in ("group8", "seq1"):
        require_path(C, path, 1, 512, "bf16", cus, monkeypatch)
        outs[path] = Case(C, path, "bf16", 1, U, 512).run()
    for a, b, name in zip(outs["seq1"], outs["group8"], ("gates", "c", "h")):
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a.view(torch.int16), b.view(torch.int32) if b.dtype == F32 else b.view(torch.int16)), name


@pytest.mark.parametrize("B,U,H", [p for p in cases("group8") if p.values[0] > 1 or p.values[2] == 256])
def test_group8(C, cus, monkeypatch, B, U, H):
    """exchange groups of 8 rows: full (8), ragged (2, 5, 7) and one row at H = 256; U = 1 (no exchange at all), 2, 33"""
    require_path(C, "group8", B, H, "bf16", cus, monkeypatch)
    Case(C, "group8", "bf16", B, U, H).run()


@pytest.mark.parametrize("B,U,H", cases("group16"))
def test_group16(C, cus, monkeypatch, B, U, H):
    """exchange groups of 16 rows: one group ragged (9) and full (16), two groups with 1, 15, 16 rows in the last, three with 1 and 8;
    B = 256 is sixteen groups - at H = 512 one workgroup on every CU of the full device, the documented limit"""
    require_path(C, "group16", B, H, "bf16", cus, monkeypatch)
    Case(C, "group16", "bf16", B, U, H).run()


@pytest.mark.parametrize("B,U,H", cases("step"))
def test_step_kernels_bf16(C, cus, monkeypatch, B, U, H):
    """one launch per step: H = 16 (three of four waves without a K slice), 48, 128, 640 (a second 8-step chunk per wave, the clamped
    s = min(sb + q, s_end - 1) loads); row blocks of 32 full, ragged and three; H = 512 with B = 257 is past the persistent grid"""
    require_path(C, "step", B, H, "bf16", cus, monkeypatch)
    Case(C, "step", "bf16", B, U, H).run()


@pytest.mark.parametrize("B,U,H", cases("step", "f32"))
def test_step_kernels_f32_io(C, cus, monkeypatch, B, U, H):
    """fp32 h, dout and dgates; the operand is rounded to bf16 inside the kernel (never persistent, also at H = 512)"""
    require_path(C, "step", B, H, "f32", cus, monkeypatch)
    Case(C, "step", "f32", B, U, H).run()


def test_step_kernels_called_directly_at_a_persistent_size(C):
    """tsasr_lstm_step_fwd / bwd at H = 256, B = 33: tsasr_lstm_seq_* never reach them at this size"""
    (B, U, H), = [p.values for p in cases("step_direct")]
    Case(C, "step_direct", "bf16", B, U, H).run()


@pytest.mark.parametrize("io", ["bf16", "f32"])
def test_cell_kernels(C, io):
    """tsasr_lstm_cell_fwd / bwd: pre-activations given whole, dh_rec given per step, dc carried in dc_io (NaN at the last step, which must
    not read either)"""
    (B, U, H), = [p.values for p in cases("cell", io)]
    Case(C, "cell", io, B, U, H).run()


# ------------------------------------------------------------------------------------------------------ the one-hot input projection
@pytest.mark.parametrize("B,U,H,I,blank", [(5, 7, 128, 28, 3), (2, 3, 16, 6, 0), (1, 1, 512, 28, 28)])
def test_onehot_gates_bit_exact(C, B, U, H, I, blank):
    """tsasr_lstm_onehot_gates: gates == (b_ih + b_hh) + W_ih[:, col] evaluated in fp32 in that order, gate-minor, BIT FOR BIT; xp = the
    one-hot column plus ones in columns I and I + 1; tokens include the blank, 0, V - 1 and a negative id; and again with xp = NULL"""
    V, Ip = I + 1, (I + 2 + 7) // 8 * 8
    g = torch.Generator().manual_seed(LR.case_seed(B, U, H))
    w_ih, b_ih, b_hh = torch.randn(4 * H, I, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1
    tok = torch.randint(0, V, (B * U,), generator=g)
    special = torch.tensor([blank, 0, V - 1, -1])[:B * U]
    tok[:special.numel()] = special
    tok = tok.view(B, U)
    col = torch.where(tok > blank, tok - 1, tok)
    col = torch.where((tok == blank) | (tok < 0), torch.full_like(col, -1), col)
    picked = torch.where((col >= 0)[..., None], w_ih.t()[col.clamp_min(0)], torch.zeros(()))        # [B, U, 4H]
    want = ((b_ih + b_hh) + picked).view(B, U, 4, H).transpose(-1, -2).contiguous()
    j = torch.arange(Ip)
    want_xp = ((j == col.view(-1, 1)) | (j == I) | (j == I + 1)).to(BF16)
    lib, p = C.lib(), C.ptr
    dev = [t.to(DEV) for t in (tok, w_ih, b_ih, b_hh)]
    for with_xp in (True, False):
        gates = torch.full((B + 2, U, H, 4), SENT, dtype=F32, device=DEV)
        gates[:B] = NAN
        xp = torch.full((B * U + 2, Ip), SENT, dtype=BF16, device=DEV)
        xp[:B * U] = NAN
        C.check(lib.tsasr_lstm_onehot_gates(p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(gates), p(xp) if with_xp else None, B, U, H, I, Ip, blank,
                                            C.stream_ptr()), "tsasr_lstm_onehot_gates")
        torch.cuda.synchronize()
        assert bool((gates[B:] == SENT).all()) and bool((xp[B * U:] == SENT).all())
        got = gates[:B].cpu()
        bad = got.view(torch.int32) != want.view(torch.int32)
        assert not bad.any(), f"{int(bad.sum())} gate values differ, first at (b, u, unit, gate) = {torch.nonzero(bad)[0].tolist()}"
        if with_xp:
            assert torch.equal(xp[:B * U].cpu().view(torch.int16), want_xp.view(torch.int16))
        else:
            assert bool(torch.isnan(xp[:B * U].float()).all())


# ------------------------------------------------------------------------------------------------------ ops level
@pytest.mark.parametrize("B,U,I,H,onehot", [(*s, False) for s in LR.OPS_SHAPES] + [(33, 6, 28, 512, True)])
def test_ops_lstm_rows_vs_free_running_model(C, B, U, I, H, onehot):
    """ops.lstm with requires_grad on x (the bf16 dx GEMM of _LstmFn.backward, which no test computed before) and ops.lstm_onehot with token
    ids: out and dx per (b, t), dW_hh / dW_ih / db_ih / db_hh per gate row of the 4H, relative L2 against the free-running float64 model
    with the kernels' rounding points (lstm_ref.model; bounds: lstm_ref.TOL["ops"]); db_ih == db_hh bit for bit."""
    ops = importlib.import_module("ts-asr_amd.ops")
    (x, w_ih, w_hh, b_ih, b_hh, dout), kw = LR.ops_inputs(B, U, I, H, onehot)
    rnn = torch.nn.LSTM(I, H, batch_first=True).to(DEV)
    with torch.no_grad():
        for prm, v in zip((rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            prm.copy_(v)
    ref = LR.model(x, w_ih, w_hh, b_ih, b_hh, dout, **kw)
    if onehot:
        assert ops.lstm_onehot_supported(kw["tokens"].to(DEV), rnn, I + 1)
        xg = None
        out = ops.lstm_onehot(kw["tokens"].to(DEV), rnn, kw["blank"])
    else:
        xg = x.to(DEV).requires_grad_()
        out, _ = ops.lstm(xg, rnn)
    assert out.dtype == BF16 and "_LstmFn" in type(out.grad_fn).__name__
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    assert ops.lstm_timeouts() == 0
    got = {"out": out.detach(), "dW_hh": rnn.weight_hh_l0.grad, "dW_ih": rnn.weight_ih_l0.grad, "db_ih": rnn.bias_ih_l0.grad, "db_hh": rnn.bias_hh_l0.grad}
    if not onehot:
        assert xg.grad is not None and xg.grad.dtype == BF16 and xg.grad.shape == x.shape
        got["dx"] = xg.grad
    assert torch.equal(got["db_ih"].view(torch.int32), got["db_hh"].view(torch.int32))
    what = f"ops B={B} U={U} I={I} H={H} onehot={onehot}"
    worst = {k: float(LR.row_errors(k, v.float().cpu(), ref[k]).max()) for k, v in got.items()}
    print("\nLSTMSTAT", what, " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in got.items():
        LR.check_rows(k, v.float().cpu(), ref[k], LR.TOL["ops"][k][0], what)
