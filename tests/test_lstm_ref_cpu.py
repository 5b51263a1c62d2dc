"""The LSTM step checker and models of tests/helpers/lstm_ref.py bite: the free-running model without its rounding points is torch.nn.LSTM,
the fp32 emulation passes the step check with the final delta, and a float64 "kernel" with ONE defect each is rejected with the place of
the defect named - while the first three defects pass the criteria the suite had before (whole-tensor `rel L2 < 1e-2` on out, `3e-2` on the
parameter gradients)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lstm_ref as LR  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
B, H, U, BR, I = 19, 64, 6, 16, 28            # two exchange groups of 16, the last with 3 live rows; four 16-unit blocks; eight 8-unit pieces
D_FWD, D_BWD = LR.TOL["delta_fwd"][0], LR.TOL["delta_bwd"][0]


@pytest.fixture(scope="module")
def case():
    gates0, whh, dout = LR.case_inputs(B, U, H, seed=5)
    x = torch.randn(B, U, I, generator=torch.Generator().manual_seed(6)).to(F64)
    return gates0, whh, dout, x


# ------------------------------------------------------------------------------------------------------------------ a float64 kernel with defects
def kernel(case, defect=None):
    """bf16-io recurrence in float64, forward then backward on the forward's outputs, with at most one planted defect.
    -> act, c, h, dgates (h and dgates hold bf16 values)."""
    gates0, whh, dout, _ = case
    w = whh.to(F64)
    g0, do = gates0.to(F64), dout.to(F64)
    act, c, h = torch.zeros(B, U, H, 4, dtype=F64), torch.zeros(B, U, H, dtype=F64), torch.zeros(B, U, H, dtype=F64)
    for t in range(U):
        hp = h[:, t - 1].clone() if t > 0 else torch.zeros(B, H, dtype=F64)
        cp = c[:, t - 1].clone() if t > 0 else torch.zeros(B, H, dtype=F64)
        if defect == "stale_piece" and t == 3:
            hp[17, 40:48] = h[17, t - 2, 40:48]                       # piece 5 of row 17 = group 1 row 1 still holds step t - 2
        rec = hp @ w.t()
        if defect == "clamped_row" and t == 1:                        # in workgroup 1 (units 32..63) a live row of the ragged group gets
            rows = (torch.arange(4)[:, None] * H + torch.arange(32, 64)[None, :]).reshape(-1)
            rec[17, rows] = rec[B - 1, rows]                          # the operand of the row its padding rows are clamped to
        if defect == "k_quarter" and t == 4:
            hq = hp.clone()
            hq[:, 16:32] = 0                                          # wave 1's quarter of K ...
            u = torch.arange(32, 48)
            rows = (torch.arange(4)[:, None] * H + u[None, :]).reshape(-1)
            rec[:, rows] = (hq @ w.t())[:, rows]                      # ... never reaches the 16-unit block 2
        if defect == "c_neighbour" and t == 3:
            cp[5] = c[6, t - 1]
        pre = g0[:, t] + LR._minor(rec, H)
        gi, gf, gg, go = torch.sigmoid(pre[..., 0]), torch.sigmoid(pre[..., 1]), torch.tanh(pre[..., 2]), torch.sigmoid(pre[..., 3])
        c[:, t] = gf * cp + gi * gg
        ht = go * torch.tanh(c[:, t])
        h[:, t] = LR.bf(ht)
        if defect == "h_ulp" and t == 2:
            r, ulp = ht[4, 9], 2 * LR.half_ulp_bf16(ht[4, 9])
            h[4, t, 9] = LR.bf(r) + (ulp if LR.bf(r) > r else -ulp)   # one ulp further AWAY from the exact value
            assert LR.bf(h[4, t, 9]) == h[4, t, 9]
        act[:, t] = torch.stack([gi, gf, gg, go], dim=-1)
        if defect == "swap_fg":
            act[:, t, 21, 1], act[:, t, 21, 2] = gg[:, 21], gf[:, 21]
    dg = torch.zeros(B, U, 4 * H, dtype=F64)
    dcar = torch.zeros(B, H, dtype=F64)
    stale = torch.randn(B, 4 * H, generator=torch.Generator().manual_seed(8), dtype=F64) * 0.1
    for t in range(U - 1, -1, -1):
        dh = do[:, t].clone()
        if t < U - 1:
            dh += dg[:, t + 1] @ w
        elif defect == "rec_at_last":
            dh += LR.bf(stale) @ w                                    # whatever the buffer held: `last` not honoured
        if defect == "dc_dropped" and t == 2:
            dcar = torch.zeros_like(dcar)
        cp = c[:, t - 1] if t > 0 else torch.zeros(B, H, dtype=F64)
        d4, dcar = LR._cell_bwd(act[:, t], c[:, t], cp, dh, dcar)
        dg[:, t] = LR.bf(d4.reshape(B, 4 * H))
        if defect == "gate_minor" and t == 1:
            dg[18, t] = LR.bf(d4[18].t().reshape(4 * H))
    return act, c, h, dg


def checked(case, out):
    gates0, whh, dout, _ = case
    act, c, h, dg = out
    sf = LR.check_fwd(gates0, whh, act, c, h, D_FWD, BR=BR, what="mutant fwd")
    sb = LR.check_bwd(act, c, dout, whh, dg, D_BWD, BR=BR, what="mutant bwd")
    return sf, sb


def rejected(case, defect):
    with pytest.raises(LR.Mismatch) as e:
        checked(case, kernel(case, defect))
    return str(e.value)


def old_criteria_pass(case, out):
    """what tests/test_blocks_gpu.py::test_lstm_hip_path_vs_oracle asks: rel L2 of out < 1e-2, of the four parameter gradients < 3e-2"""
    x = case[3]

    def quantities(o):
        act, c, h, dg = o
        hp = torch.zeros_like(h)
        hp[:, 1:] = h[:, :-1]
        d2 = dg.reshape(B * U, 4 * H)
        return h, d2.t() @ x.reshape(B * U, I), d2.t() @ hp.reshape(B * U, H), d2.sum(0)
    rel = [float((a - b).norm() / b.norm()) for a, b in zip(quantities(out), quantities(kernel(case)))]
    return rel[0] < 1e-2 and all(r < 3e-2 for r in rel[1:]), rel


# ------------------------------------------------------------------------------------------------------------------ the checker accepts the truth
def test_correct_kernel_passes(case):
    sf, sb = checked(case, kernel(case))
    # (torch rounds float64 to bf16 through float32: a value within 2^-25 of a tie may land on the other neighbour, 1/2 ulp + 3e-8 away)
    assert max(sf["act"], sf["c"]) < 1e-12 and sf["h"] < 1e-7 and sb["dgates"] < 1e-7 and sf["h_flips"] == 0 and sb["dg_flips"] == 0


@pytest.mark.parametrize("io", ["bf16", "f32"])
def test_fp32_emulation_passes_with_the_final_delta(case, io):
    """the kernels' formulas in float32 (sigm, tanh_fast), run free: at most 1/16 of the deltas by construction of TOL"""
    gates0, whh, dout, _ = case
    do = dout if io == "bf16" else dout.float()
    act, c, h = LR.recurrence_fwd(gates0, whh, io, F32, fast=True)
    dg = LR.recurrence_bwd(act, c, do, whh, io, F32, fast=True)
    sf = LR.check_fwd(gates0, whh, act, c, h, D_FWD, io, BR=BR)
    sb = LR.check_bwd(act, c, do, whh, dg, D_BWD, io, BR=BR)
    assert max(sf["act"], sf["c"], sf["h"]) <= LR.TOL["delta_fwd"][1] and sb["dgates"] <= LR.TOL["delta_bwd"][1]
    if io == "bf16":
        assert sf["h_flips"] <= LR.TOL["flips"] and sb["dg_flips"] <= LR.TOL["flips"]


def test_deltas_are_sixteen_times_the_emulation():
    for k in ("delta_fwd", "delta_bwd"):
        bound, cpu = LR.TOL[k]
        assert cpu * 15.9 <= bound <= cpu * 16.2
    for k, (bound, emu, _) in LR.TOL["ops"].items():
        assert emu * 3.95 <= bound <= emu * 4.1, k


@pytest.mark.parametrize("shape", [(3, 5, 7, 16), (2, 4, 28, 48)])
def test_model_without_rounding_is_torch_lstm(shape):
    """outputs, final state and every gradient to 1e-12 relative, dense input; the one-hot route against the same module fed one-hot rows"""
    Bq, Uq, Iq, Hq = shape
    (x, w_ih, w_hh, b_ih, b_hh, dout), _ = LR.ops_inputs(Bq, Uq, Iq, Hq)
    rnn = torch.nn.LSTM(Iq, Hq, batch_first=True).double()
    with torch.no_grad():
        for p, v in zip((rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(v.double())
    _, kw = LR.ops_inputs(Bq, Uq, Iq, Hq, onehot=True)
    for tokens in (None, kw["tokens"]):
        xin = (x.double() if tokens is None else LR.onehot_rows(tokens, Iq, 0)).requires_grad_()
        rnn.zero_grad()
        out, (hn, cn) = rnn(xin)
        out.backward(dout.double())
        got = LR.model(x, w_ih, w_hh, b_ih, b_hh, dout, rounding=False, tokens=tokens)
        want = {"out": out, "hn": hn[0], "cn": cn[0], "dW_ih": rnn.weight_ih_l0.grad, "dW_hh": rnn.weight_hh_l0.grad,
                "db_ih": rnn.bias_ih_l0.grad, "db_hh": rnn.bias_hh_l0.grad}
        if tokens is None:
            want["dx"] = xin.grad
        assert set(got) == set(want)
        for k, r in want.items():
            assert float((got[k] - r.detach()).norm() / r.detach().norm()) < 1e-12, k


def test_onehot_rows_follow_the_embedding():
    tok = torch.tensor([[3, 0, 5, -1, 4]])
    rows = LR.onehot_rows(tok, 5, 3)                                   # blank 3: ids above it shift down, the blank and -1 select nothing
    assert rows[0].argmax(1).tolist()[1:3] == [0, 4] and rows[0, 4].argmax() == 3
    assert rows[0, 0].sum() == 0 and rows[0, 3].sum() == 0 and rows.sum() == 3


# ------------------------------------------------------------------------------------------------------------------ one defect each
def test_stale_exchange_piece(case):
    msg = rejected(case, "stale_piece")
    assert "mutant fwd gates" in msg and "first at (b=17, t=3, unit=0, gate=i)" in msg and "exchange group 1 row 1" in msg
    assert "operand h[b=17, t=2]: suspect 8-unit piece(s) [5] (units [40]..+7)" in msg


def test_clamped_row_leaks_into_a_live_row(case):
    msg = rejected(case, "clamped_row")
    assert "first at (b=17, t=1, unit=32, gate=i)" in msg and "exchange group 1 row 1, workgroup 1 (units 32..+31)" in msg
    assert "operand h[b=17, t=0]: suspect 8-unit piece(s) [0, 1, 2, 3, 4, 5, 6, 7]" in msg


def test_skipped_k_quarter(case):
    msg = rejected(case, "k_quarter")
    assert "first at (b=0, t=4, unit=32, gate=i)" in msg and "exchange group 0 row 0, workgroup 1 (units 32..+31)" in msg
    assert "operand h[b=0, t=3]: suspect 8-unit piece(s) [2, 3] (units [16, 24]..+7)" in msg


def test_first_three_defects_pass_the_old_norm_criteria(case):
    """the gap this checker closes: one wrong row or block moves the whole-tensor norms by far less than 1e-2 / 3e-2"""
    for d in ("stale_piece", "clamped_row", "k_quarter"):
        ok, rel = old_criteria_pass(case, kernel(case, d))
        assert ok and max(rel) > 0, (d, rel)


def test_c_from_the_neighbouring_row(case):
    msg = rejected(case, "c_neighbour")
    assert "mutant fwd c:" in msg and f"{H} of" in msg and "first at (b=5, t=3, unit=0)" in msg and "exchange group 0 row 5" in msg


def test_gates_f_and_g_swapped(case):
    msg = rejected(case, "swap_fg")
    assert "mutant fwd gates" in msg and f"{2 * B * U} of" in msg and "first at (b=0, t=0, unit=21, gate=f)" in msg


def test_dc_carry_dropped(case):
    msg = rejected(case, "dc_dropped")
    assert "mutant bwd dgates" in msg and "first at (b=0, t=2, unit=0, gate=i)" in msg
    assert ", t=1," not in msg and ", t=3," not in msg                     # only the step that lost it


def test_recurrent_term_at_the_last_step(case):
    msg = rejected(case, "rec_at_last")
    assert "mutant bwd dgates" in msg and f"first at (b=0, t={U - 1}, unit=0, gate=i)" in msg


def test_dgates_row_stored_gate_minor(case):
    msg = rejected(case, "gate_minor")
    assert "mutant bwd dgates" in msg and "first at (b=18, t=1, unit=" in msg and "exchange group 1 row 2" in msg
    assert ", t=0," not in msg.split("worst at")[0]


def test_h_one_ulp_the_wrong_way(case):
    msg = rejected(case, "h_ulp")
    assert "mutant fwd h: 1 of" in msg and "first at (b=4, t=2, unit=9)" in msg and "workgroup 0" in msg


def test_seq1_names_its_eight_unit_workgroups(case):
    gates0, whh, dout, _ = case
    act, c, h, dg = kernel(case, "h_ulp")
    with pytest.raises(LR.Mismatch) as e:
        LR.check_fwd(gates0, whh, act, c, h, D_FWD, BR=1, wg_units=8, what="seq1")
    assert "exchange group 4 row 0, workgroup 1 (units 8..+7)" in str(e.value)


def test_nan_and_half_ulp(case):
    gates0, whh, dout, _ = case
    act, c, h, dg = kernel(case)
    h2 = h.clone()
    h2[2, 1, 3] = float("nan")
    with pytest.raises(LR.Mismatch):
        LR.check_fwd(gates0, whh, act, c, h2, D_FWD, BR=BR)
    r = torch.tensor([1.0, 1.5, 0.75, -3.0, 0.0, 2.0 ** -20], dtype=F64)
    assert LR.half_ulp_bf16(r).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -9, 2.0 ** -7, 0.0, 2.0 ** -28]


def test_matrix_covers_what_the_issue_lists():
    m = LR.matrix()
    assert len(m) == len(set(m))
    assert {U for p, _, _, U, _ in m if p == "seq1"} == {1, 2, 3, 4, 5, 9, 97}
    assert {B for p, _, B, _, _ in m if p == "group16"} == {9, 16, 17, 31, 32, 33, 40, 256}
    assert {H for p, io, _, _, H in m if p == "step" and io == "bf16"} == {16, 48, 128, 640, 512}
