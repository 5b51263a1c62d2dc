"""tests/helpers/rowkern_ref.py on the CPU: the float64 model against float64 autograd, the fp32 emulation within TOL on every case of the
matrix, the dispatch mirror at every boundary, the workspace and LDS formulas against hand-computed values, the dropout-mask port's
statistics, and the judge failing on planted errors. No GPU."""
import collections
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rowkern_ref as R  # noqa: E402

F64, F32 = torch.float64, torch.float32


def find(prefix):
    return next(c for c in R.matrix() if c["key"].startswith(prefix))


# ------------------------------------------------------------------------------------------------------ the model is the operation
def autograd(c, inp):
    """float64 autograd through F.layer_norm / F.leaky_relu and an explicit masked dropout-add chain"""
    fam, M, D = c["fam"], c["M"], c["D"]
    leaf = lambda t: None if t is None else t.to(F64).clone().requires_grad_()  # noqa: E731
    con = lambda t: None if t is None else t.to(F64)  # noqa: E731
    x = leaf(inp["x"])
    if fam == "colsum":
        return {"out": inp["x"].to(F64).sum(0) + (inp["out0"].to(F64) if c["acc"] else 0)}
    if fam == "ln":
        g, b = leaf(inp["gamma"]), leaf(inp["beta"])
        y = Fn.layer_norm(x, (D,), g, b, c["eps"])
        if c["slope"] >= 0:
            y = Fn.leaky_relu(y, c["slope"])
        loss = (y * con(inp["dy"])).sum() + (0 if inp["dadd"] is None else (x * con(inp["dadd"])).sum())
        loss.backward()
        return {"y": y.detach(), "dx": x.grad, "dgamma": g.grad, "dbeta": b.grad}
    bias = leaf(inp["bias"])
    t = x if bias is None else x + bias
    keep = torch.ones(M, D, dtype=F64) if inp["keep"] is None else inp["keep"].to(F64)
    if fam == "bad":
        if c["slope"] >= 0:
            t = Fn.leaky_relu(t, c["slope"])
        y = t * keep * inp["ks"]
        (y * con(inp["dy"])).sum().backward()
        return {"y": y.detach(), "dx": x.grad, "dbias": None if bias is None else bias.grad}
    res = leaf(inp["res"])
    s = res + c["alpha"] * inp["live"].to(F64)[:, None] * (t * keep * inp["ks"])
    if fam in ("da", "da2"):
        out = s if inp.get("keep2") is None else s * inp["keep2"].to(F64) * inp["ks2"]
        (out * con(inp["dy"])).sum().backward()
        o = {"out": out.detach(), "dx": x.grad, "dbias": None if bias is None else bias.grad}
        if inp.get("keep2") is not None:
            o["dres"] = res.grad
        return o
    g, b = leaf(inp["gamma"]), leaf(inp["beta"])
    y = Fn.layer_norm(s, (D,), g, b, c["eps"])
    loss = (0 if inp["dy"] is None else (y * con(inp["dy"])).sum()) + (0 if inp["dout"] is None else (s * con(inp["dout"])).sum())
    o = {}
    if fam == "aln2":
        g2, b2 = leaf(inp["gamma2"]), leaf(inp["beta2"])
        z = Fn.layer_norm(y, (D,), g2, b2, c["eps2"])
        loss = loss + (z * con(inp["dz"])).sum()
    loss.backward()
    o.update(s=s.detach(), y=y.detach(), dx=x.grad, dres=res.grad, dgamma=g.grad, dbeta=b.grad, dbias=None if bias is None else bias.grad)
    if fam == "aln2":
        o.update(z=z.detach(), dgamma2=g2.grad, dbeta2=b2.grad)
    return o


SMALL = [c for c in R.matrix() if (c["M"] <= 39 and c["D"] <= 520) or (c["fam"] == "colsum" and c["M"] <= 777)]


@pytest.mark.parametrize("fam", ["ln", "aln", "aln2", "bad", "da", "da2", "colsum"])
def test_model_is_float64_autograd(fam):
    n = 0
    for c in SMALL:
        if c["fam"] != fam:
            continue
        inp, _ = R.case_inputs(c)
        got, want = R.model(c, inp, rounding=False), autograd(c, inp)
        for k, w in want.items():
            if w is None:
                continue
            scale = float(w.abs().max()) + 1e-300
            assert float((got[k] - w).abs().max()) <= 1e-12 * scale, (c["key"], k)
            n += 1
    assert n >= 6


# ------------------------------------------------------------------------------------------------------ the emulation within the bounds
@pytest.fixture(scope="module")
def emulated():
    out = {}
    for c in R.matrix():
        inp, n = R.case_inputs(c, search=True)
        out[c["key"]] = (c, inp, n, R.emulate(c, inp))
    return out


def test_emulation_within_tol_and_flips_within_quarter_cap(emulated):
    worst = {io: collections.defaultdict(float) for io in R.IOS}
    for key, (c, inp, n, e) in emulated.items():
        assert n == R.SEEDS.get(key, 0), key
        st = R.check_case(c, inp, e, R.deltas(c["io"]))
        for k, v in st.items():
            if k.endswith("_flips"):
                assert v <= R.TOL["flips"] / 4, (key, k, v)
            elif k != "min_abs_pre":
                worst[c["io"]][k] = max(worst[c["io"]][k], v)
    for io in R.IOS:                              # the recorded measurements are the ones this run makes (row outputs: the larger io's)
        for k, (bound, meas) in R.TOL[io].items():
            m = max(worst[i][k] for i in R.IOS) if k in R.ROW_OUTPUTS else worst[io][k]
            assert m <= meas * 1.01 + 1e-12 and bound == pytest.approx(4 * max(meas, R.FLOOR), rel=0.01), (io, k, m, meas, bound)


def test_kink_clearance_and_margin(emulated):
    assert R.KINK_MARGIN >= 100 * R.EMU_PRE_ERR
    worst, n = 0.0, 0
    for key, (c, inp, _, e) in emulated.items():
        if c["fam"] == "ln" and c["slope"] >= 0:
            y = R.pre_activation(inp["x"], inp["gamma"], inp["beta"], c["eps"])
            assert float(y.abs().min()) >= R.KINK_MARGIN, key
            assert torch.equal(R.bf(inp["x"]), inp["x"]), key                  # still whole bf16 values
            worst = max(worst, float((e["pre"].to(F64) - y).abs().max()))
            n += 1
    assert n >= 20 and worst <= R.EMU_PRE_ERR * 1.01


# ------------------------------------------------------------------------------------------------------ the dispatch mirror
def test_matrix_reaches_every_instantiation():
    seen = collections.defaultdict(set)
    for c in R.matrix():
        for entry, path in R.case_paths(c).items():
            seen[(entry, c["io"])].add(path)
    for entry, per_io in R.INSTANTIATIONS.items():
        for io, paths in per_io.items():
            assert set(paths) <= seen[(entry, io)], (entry, io, sorted(set(paths) - seen[(entry, io)]))
    assert R.INSTANTIATIONS["layernorm_fwd"]["bf16"] == [
        "layernorm_fwd_kernel<bf16,32,1>", "layernorm_fwd_kernel<bf16,64,1>", "layernorm_fwd_kernel<bf16,64,2>", "layernorm_fwd_kernel<bf16,64,4>",
        "layernorm_fwd_wide_kernel<bf16,2>", "layernorm_fwd_wide_kernel<bf16,3>", "layernorm_fwd_wide_kernel<bf16,4>", "layernorm_fwd_wide_kernel<bf16,6>",
        "layernorm_fwd_wide_kernel<bf16,8>"]
    assert R.INSTANTIATIONS["add_layernorm_bwd"]["f32"] == [f"add_layernorm_bwd_kernel<float,{i},false>" for i in (1, 2, 4, 8)]
    assert R.INSTANTIATIONS["add_layernorm2_bwd"]["bf16"] == ["add_layernorm2_bwd_kernel<bf16,1,true>", "add_layernorm2_bwd_kernel<bf16,1,false>",
                                                              "add_layernorm2_bwd_kernel<bf16,2,false>"]
    assert sum(len(v) for d in R.INSTANTIATIONS.values() for v in d.values()) == 2 * 18 + 8 + 2 * 8 + 2 * 6
    for fam in ("bad", "da", "da2"):              # both thread layouts of the slab kernels: several row slots through LDS, and one slot
        for io in R.IOS:
            lds = {R.slot_lds(io, c["D"]) > 0 for c in R.matrix() if c["fam"] == fam and c["io"] == io}
            assert lds == {True, False}, (fam, io)


LN_BOUNDS = {"bf16": [(8, "32,1"), (256, "32,1"), (264, "64,1"), (512, "64,1"), (520, "64,2"), (1024, "64,2"), (1032, "64,4"), (2048, "64,4"), (2056, "w2"),
                      (4096, "w2"), (4104, "w3"), (6144, "w3"), (6152, "w4"), (8192, "w4"), (8200, "w6"), (12288, "w6"), (12296, "w8"), (16384, "w8"),
                      (16392, None), (260, None)],
             "f32": [(8, "32,1"), (128, "32,1"), (136, "64,1"), (256, "64,1"), (264, "64,2"), (512, "64,2"), (520, "64,4"), (1024, "64,4"), (1032, "w2"),
                     (2048, "w2"), (2056, "w3"), (3072, "w3"), (3080, "w4"), (4096, "w4"), (4104, "w6"), (6144, "w6"), (6152, "w8"), (8192, "w8"), (8200, None),
                     (132, None)]}


def test_expected_path_at_every_boundary():
    for io, t in (("bf16", "bf16"), ("f32", "float")):
        for D, tag in LN_BOUNDS[io]:
            for kind in ("fwd", "bwd"):
                want = R.REJECTED if tag is None else (f"layernorm_{kind}_wide_kernel<{t},{tag[1:]}>" if tag[0] == "w" else f"layernorm_{kind}_kernel<{t},{tag}>")
                assert R.expected_path(f"layernorm_{kind}", io, D) == want, (io, D, kind)
            want = R.REJECTED if (tag is None or tag[0] == "w") else f"layernorm_bwd_kernel<{t},{tag}>"
            assert R.expected_path("layernorm_bwd_add", io, D) == want, (io, D)
    aln = {"bf16": [(8, "1,true"), (256, "1,true"), (264, "1,false"), (512, "1,false"), (520, "2,false"), (1024, "2,false"), (1032, "4,false"),
                    (2048, "4,false"), (2056, None), (12, None)],
           "f32": [(8, "1,false"), (256, "1,false"), (264, "2,false"), (512, "2,false"), (520, "4,false"), (1024, "4,false"), (1032, "8,false"),
                   (2048, "8,false"), (2056, None), (12, None)]}
    for io, t in (("bf16", "bf16"), ("f32", "float")):
        for D, tag in aln[io]:
            for d in ("fwd", "bwd"):
                assert R.expected_path(f"add_layernorm_{d}", io, D) == (R.REJECTED if tag is None else f"add_layernorm_{d}_kernel<{t},{tag}>"), (io, D)
                two = None if D > 1024 else tag
                assert R.expected_path(f"add_layernorm2_{d}", io, D) == (R.REJECTED if two is None else f"add_layernorm2_{d}_kernel<{t},{two}>"), (io, D)
    assert R.slot_layout("bf16", 8) == (1, 256) and R.slot_layout("bf16", 64) == (8, 32) and R.slot_layout("bf16", 2048) == (256, 1)
    assert R.slot_layout("bf16", 2056) == (256, 1) and R.slot_layout("f32", 8) == (2, 128) and R.slot_layout("f32", 2056) == (256, 1)
    assert R.slot_layout("bf16", 72) == (9, 28)                                     # 256 / 9: four threads idle
    assert R.slot_lds("bf16", 64) == 32 * 64 * 4 and R.slot_lds("bf16", 2048) == 0 and R.slot_lds("f32", 64, part=False) == 0
    assert R.expected_path("colsum", "bf16", 2056) == R.REJECTED and "slots=2 " in R.expected_path("colsum", "f32", 512)


def test_rows_workgroups_and_workspace_bytes_by_hand():
    assert [R.rows_per_wg(M) for M in (1, 37, 16384, 16385, 17408, 17409, 70001)] == [16, 16, 16, 17, 17, 18, 69]
    assert R.n_workgroups("ln", "bf16", 16401, 64) == 965 and 16401 - 964 * 17 == 13          # an odd rows_per_wg, a last workgroup of 13 rows
    assert R.n_workgroups("aln", "bf16", 37, 144) == 3 and 37 - 2 * 16 == 5
    assert R.ln_bwd_rows_per_wg("bf16", 20000, 2048) == 20 and R.ln_bwd_rows_per_wg("bf16", 20000, 2056) == 40      # wide: ceil(M / 512)
    assert R.ln_bwd_rows_per_wg("f32", 20000, 1024) == 20 and R.ln_bwd_rows_per_wg("f32", 20000, 1032) == 40
    assert R.n_workgroups("ln", "bf16", 20000, 2056) == 500
    assert R.workspace_bytes("ln", 37, 144) == 3584            # 3 x 2 x 144 x 4 = 3456 -> 256-aligned
    assert R.workspace_bytes("aln", 37, 144) == 5376           # 3 x 3 x 144 x 4 = 5184
    assert R.workspace_bytes("aln2", 37, 144) == 8704          # 3 x 5 x 144 x 4 = 8640
    assert R.workspace_bytes("ln", 16401, 64) == 965 * 2 * 64 * 4 == 494080
    assert R.workspace_bytes("bad", 37, 8) == 256 and R.workspace_bytes("da", 16401, 64) == 965 * 64 * 4
    assert R.workspace_bytes("colsum", 70001, 128) == 1015 * 128 * 4 and R.n_workgroups("colsum", "f32", 70001, 128) == 1015     # rpw = 69
    assert R.workspace_bytes("colsum", 777, 256) == 13 * 256 * 4


def test_lds_table():
    """static + dynamic LDS per launch; the three launches over 64 KB stay under the 160 KB a workgroup of gfx950 may use"""
    assert R.lds_bytes("layernorm_bwd", "bf16", 2048) == 65536 + 16 and R.lds_bytes("layernorm_bwd", "f32", 1024) == 32768 + 16
    assert R.lds_bytes("layernorm_bwd", "bf16", 256) == 8 * 2 * 256 * 4 + 16 and R.lds_bytes("layernorm_bwd", "bf16", 2056) == 64
    assert R.lds_bytes("add_layernorm_bwd", "bf16", 2048) == 96 * 1024 and R.lds_bytes("add_layernorm_bwd", "f32", 1368) == 65664
    assert R.lds_bytes("add_layernorm_bwd", "f32", 1360) == 65280 and R.lds_bytes("add_layernorm_bwd", "bf16", 256) == 24 * 1024
    assert R.lds_bytes("add_layernorm2_bwd", "bf16", 1024) == 80 * 1024 and R.lds_bytes("add_layernorm2_bwd", "f32", 824) == 65920
    assert R.lds_bytes("add_layernorm2_bwd", "f32", 816) == 65280 and R.lds_bytes("add_layernorm2_bwd", "bf16", 256) == 40 * 1024
    worst = max(R.lds_bytes(e, io, D) for e in ("layernorm_fwd", "layernorm_bwd", "add_layernorm_bwd", "add_layernorm2_bwd", "colsum", "bias_act_dropout_bwd",
                                                "dropout_add_bwd") for io in R.IOS for D in range(8, 16392, 8))
    assert worst == 96 * 1024 <= R.LDS_LIMIT
    assert max(R.lds_bytes(e, io, D) for e in ("colsum", "bias_act_dropout_bwd", "dropout_add_bwd") for io in R.IOS for D in range(8, 2049, 8)) <= 8192


# ------------------------------------------------------------------------------------------------------ the mask port
def test_mask_port_statistics():
    assert R.drop_thr16(0.1) == 6554 and R.drop_thr16(0.0) == 0 and R.drop_thr16(0.999999) == 65535 and R.drop_thr16(0.5) == 32768
    assert R.drop_scale16(6554) == float(np.float32(65536.0) / np.float32(58982.0)) and R.drop_scale16(0) == 1.0
    n = 1 << 20
    for seed, dev in ((0x1234567, 0), (R.BIG_SEED, 0), (R.BIG_SEED, R.DEV_SEED)):
        k = R.keep_mask(n, seed, 0.1, dev).double()
        q = 1 - 6554 / 65536
        sigma = (q * (1 - q) / n) ** 0.5
        assert abs(float(k.mean()) - q) <= 5 * sigma, (seed, float(k.mean()))
        lo, hi = k[0::2], k[1::2]                                                # the two halves of a hash word
        cov = float(((lo - q) * (hi - q)).mean())
        assert abs(cov) <= 5 * q * (1 - q) / (n / 2) ** 0.5, (seed, cov)
        for lag in (2, 8, 144):                                                  # neighbouring words, the next access, the next row
            cov = float(((k[:-lag] - q) * (k[lag:] - q)).mean())
            assert abs(cov) <= 5 * q * (1 - q) / (n - lag) ** 0.5, (seed, lag, cov)
    a, b = R.keep_mask(4096, 5, 0.1), R.keep_mask(4096, 6, 0.1)
    assert 0.7 < float((a == b).double().mean()) < 0.9                           # another seed, another mask (agreement q^2 + (1 - q)^2 = 0.82)
    assert torch.equal(R.keep_mask(4096, 2 ** 64 - 1, 0.1, 6), R.keep_mask(4096, 5, 0.1))       # host + device seed wraps as uint64
    assert torch.equal(R.keep_mask(100, 5, 0.1, start=1000), R.keep_mask(1100, 5, 0.1)[1000:])  # a pure function of the element index
    hi32 = R.keep_mask(64, 5, 0.1, start=1 << 33)                                # the counter's high word enters the hash
    assert not torch.equal(hi32, R.keep_mask(64, 5, 0.1))


# ------------------------------------------------------------------------------------------------------ the judge can fail
def planted(c, inp, e, stage, name):
    with pytest.raises(R.Mismatch) as ei:
        R.check_case(c, inp, e, R.deltas(c["io"]))
    assert ei.value.stage == stage and name in ei.value.name, str(ei.value)
    return ei.value


def ln_terms(c, inp, e):
    return R.ln_backward(inp["dy"].float(), inp["x"].float(), e["mean"], e["rstd"], inp["gamma"], inp["beta"], c["slope"], None)


def test_judge_fails_on_planted_errors():
    c = find("ln-f32-M37-D72-s0.01")
    inp, _ = R.case_inputs(c)
    base = R.emulate(c, inp)
    R.check_case(c, inp, base, R.deltas("f32"))
    e = dict(base, dx=base["dx"].clone())
    e["dx"][21] *= 1 + 4 * R.deltas("f32")["dx"]                                  # one row's dx scaled by 1 + 4 delta
    m = planted(c, inp, e, "rows", "dx")
    assert m.first[0] == 21 and "row=21" in str(m) and "lane=" in str(m) and "iteration=" in str(m) and "layernorm_bwd_kernel<float,32,1>" in str(m)
    t = ln_terms(c, inp, base)
    e = dict(base, dgamma=base["dgamma"].clone())
    e["dgamma"][40] -= t["tg"][32:37, 40].sum()                                   # the last workgroup's partial-slab column 40 dropped
    assert planted(c, inp, e, "columns", "dgamma").first == (40,)
    e = dict(base, dbeta=base["dbeta"] + t["tb"][16])                             # row 16 counted twice
    planted(c, inp, e, "columns", "dbeta")
    c = find("bad-bf16-M37-D64")
    inp, _ = R.case_inputs(c)
    base = R.emulate(c, inp)
    R.check_case(c, inp, base, R.deltas("bf16"))
    r, col = [int(v) for v in torch.nonzero(inp["keep"] & (base["y"] != 0))[5]]
    e = dict(base, y=base["y"].clone())
    e["y"][r, col] = 0                                                            # one mask bit flipped: kept -> dropped
    assert planted(c, inp, e, "forward", "y").first == (r, col)
    r, col = [int(v) for v in torch.nonzero(~inp["keep"])[3]]
    e = dict(base, dx=base["dx"].clone())
    e["dx"][r, col] = inp["dy"][r, col] * inp["ks"]                               # the backward uses another bit than the forward
    assert planted(c, inp, e, "backward", "dx").first == (r, col)
    c = find("aln-bf16-M39-D144-p0.1")
    inp, _ = R.case_inputs(c)
    base = R.emulate(c, inp)
    R.check_case(c, inp, base, R.deltas("bf16"))
    row = 13 + 8                                                                  # utterance 1 keeps 6 of its 13 frames: a masked row
    assert not bool(inp["live"][row])
    wrong, _ = R.tail(inp["x"][row:row + 1], inp["bias"], inp["res"][row:row + 1], inp["keep"][row:row + 1], inp["ks"], c["alpha"], torch.ones(1, dtype=torch.bool), F32)
    e = dict(base, s=base["s"].clone())
    e["s"][row] = wrong[0].to(torch.bfloat16)                                     # alpha applied to the unmasked branch: the time mask came too late
    assert planted(c, inp, e, "tail", "s").first[0] == row
    e = R.emulate(c, inp, plant="mean_unrounded")                                 # statistics of the unrounded s
    planted(c, inp, e, "stats", "mean")
    c = find("aln2-bf16-M37-D144")
    inp, _ = R.case_inputs(c)
    base = R.emulate(c, inp)
    R.check_case(c, inp, base, R.deltas("bf16"))
    e = dict(base, dgamma2=base["dgamma2"].clone())
    e["dgamma2"][7] *= 1 + 1e-4
    planted(c, inp, e, "columns", "dgamma2")
    e = dict(base, dres=(base["dres"].float() * (1 + 2.0 ** -6)).to(torch.bfloat16))      # two bf16 ulps off everywhere
    planted(c, inp, e, "rows", "dres")
    e = dict(base, dx=base["dx"].clone())
    e["dx"][:, 0] = (base["dx"][:, 0].float() * (1 + 2.0 ** -8)).to(torch.bfloat16)        # one ulp off in one column: too many to be flips
    planted(c, inp, e, "rows", "dx")
    c = find("colsum-f32-M777-D256-acc1")
    inp, _ = R.case_inputs(c)
    e = R.emulate(c, inp)
    R.check_case(c, inp, e, R.deltas("f32"))
    e = {"out": e["out"] - inp["out0"]}                                           # accumulate ignored
    planted(c, inp, e, "columns", "out")
