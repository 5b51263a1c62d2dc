"""The convolution-core model and stage checks of tests/helpers/convmod_ref.py are right, and the checks bite: the model without its rounding
points is float64 autograd through F.conv1d(groups=D) / F.layer_norm / F.leaky_relu and the oracle's conv_module; the fp32 emulation passes
every check at the final deltas on the whole matrix, with its flip shares within a quarter of the cap and every case's recorded seed clear of
the LeakyReLU kink; and a "kernel" (the emulation) with ONE defect each is rejected by the named check at the named place."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import convmod_ref as CR  # noqa: E402
from oracle import tsasr_ref as R  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DELTA = {io: {k: v[0] for k, v in CR.TOL[io].items()} for io in ("f32", "bf16")}
QUARTER = CR.TOL["flips"] / 4


def small_inputs(K, causal, bias, slope, B=2, T=37, D=16, seed=3):
    inp = CR.draw(B, T, D, K, bias, seed)
    inp.update(K=K, causal=causal, slope=slope)
    return inp


# ------------------------------------------------------------------------------------------------------------------ the model is the operation
@pytest.mark.parametrize("slope", [0.01, 0.0, -1.0])
@pytest.mark.parametrize("bias", [1, 0])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("K", CR.KS)
def test_pure_model_is_float64_autograd(K, causal, bias, slope):
    inp = small_inputs(K, causal, bias, slope)
    got, ref = CR.model(inp, rounding=False), CR.autograd_reference(inp)
    assert ("db2" in ref) == bool(bias)
    for k, r in ref.items():
        err = float((got[k] - r).abs().max() / r.abs().max().clamp_min(1.0))
        assert err <= 1e-12, (k, err)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("K", [31, 7])
def test_pure_model_is_the_oracles_conv_module(K, causal):
    """oracle.tsasr_ref.conv_module = LayerNorm + bottleneck GEMM, the core, the output linear: with the two GEMMs done here in float64 the
    core must be the pure model (the oracle's slope is its LRELU_SLOPE, its bias always present)."""
    D, B, T = 16, 2, 29
    g = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    sd = {"c.layer_norm.weight": rn(D) * 0.1 + 1, "c.layer_norm.bias": rn(D) * 0.1, "c.bottleneck.0.weight": rn(2 * D, D, 1) / 4, "c.bottleneck.0.bias": rn(2 * D) * 0.1,
          "c.conv.weight": rn(D, 1, K) / K ** 0.5, "c.conv.bias": rn(D) * 0.1, "c.after_conv.0.weight": rn(D) * 0.1 + 1, "c.after_conv.0.bias": rn(D) * 0.1,
          "c.after_conv.2.weight": rn(D, D) / 4, "c.after_conv.2.bias": rn(D) * 0.1}
    x = rn(B, T, D)
    want = R.conv_module(x, sd, "c.", None, causal)
    y2 = torch.nn.functional.layer_norm(x, (D,), sd["c.layer_norm.weight"], sd["c.layer_norm.bias"], 1e-5) @ sd["c.bottleneck.0.weight"].squeeze(-1).t()
    inp = {"y2": y2, "b2": sd["c.bottleneck.0.bias"], "cw": sd["c.conv.weight"].view(D, K), "cb": sd["c.conv.bias"], "gamma": sd["c.after_conv.0.weight"],
           "beta": sd["c.after_conv.0.bias"], "dz": None, "K": K, "causal": int(causal), "slope": R.LRELU_SLOPE}
    z = CR.model(inp, rounding=False)["z"]
    got = z @ sd["c.after_conv.2.weight"].t() + sd["c.after_conv.2.bias"]
    assert float((got - want).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ the emulation passes
def run_checks(inp, io, out, tile=64, what=""):
    """the three stage checks in the order the GPU test applies them"""
    d = DELTA[io]
    st = CR.check_conv(inp, io, out["c"], d, tile, what)
    st.update(CR.check_ln(inp, io, out["c"], out["mean"], out["rstd"], out["z"], d, tile, what))
    par = {k: out[k] for k in CR.PARAMS if k in out and (inp["b2"] is not None or k != "db2")}
    st.update(CR.check_bwd(inp, io, out["c"], out["mean"], out["rstd"], out["dy2"], par, d, tile, what))
    return st


@pytest.mark.parametrize("group", ["kpb", "time", "chan", "act"])
def test_emulation_passes_every_check_on_the_matrix(group):
    """every case of the group at its recorded seed: the search from seed 0 ends on it, no pre-activation within KINK_MARGIN of the kink, the
    emulation inside every bound, its flip shares (and the share of dy2 that needs the flip allowance) within a quarter of the cap"""
    done = set()
    for grp, path, B, T, D, K, causal, bias, slope in CR.matrix():
        io = CR.io_of(path)
        key = CR.case_key(B, T, D, K, causal, bias, slope)
        if grp != group or (key, io) in done:
            continue
        done.add((key, io))
        inp, n = CR.case_inputs(B, T, D, K, causal, bias, slope, search=True)
        assert n == CR.SEEDS.get(key, 0), (key, n)
        if slope >= 0:
            assert CR.min_abs_y(inp) >= CR.KINK_MARGIN, key
        st = run_checks(inp, io, CR.emulate(inp, io), CR.TILE[path.split()[0]], f"{key} {io}")
        if io == "bf16":
            for k in ("c_flips", "z_flips", "dy2_flips", "dy2_over"):
                assert st[k] <= QUARTER, (key, k, st[k])
    assert done


def test_ops_case_seeds_are_recorded():
    for B, T, D, K, causal, bias, slope in CR.all_case_keys():
        key = CR.case_key(B, T, D, K, causal, bias, slope)
        assert CR.case_inputs(B, T, D, K, causal, bias, slope, search=True)[1] == CR.SEEDS.get(key, 0), key
    assert set(CR.SEEDS) <= {CR.case_key(*k) for k in CR.all_case_keys()}


@pytest.mark.parametrize("io", ["f32", "bf16"])
def test_stream_emulation_passes(io):
    for K, D, chunks, slope in [(*v, 0.01) for v in CR.STREAM] + CR.STREAM_ACT:
        inp = CR.stream_inputs(K, D, slope=slope)
        zs, hs, _ = CR.emulate_stream(inp, io, chunks)
        st = CR.check_stream(inp, io, chunks, zs, hs, DELTA[io], f"stream K={K} D={D} {chunks} slope={slope} {io}")
        assert st["z_over"] <= QUARTER, (K, D, chunks, slope, st)


def test_bounds_are_sixteen_times_their_measurement():
    for io in ("f32", "bf16"):
        for k, (bound, measured) in CR.TOL[io].items():
            assert abs(bound / (16 * measured) - 1) < 0.01, (io, k)
    for path, d in CR.TOL["ops"].items():
        for k, (bound, emu, _) in d.items():
            assert abs(bound / (4 * emu) - 1) < 0.01, (path, k)
    assert max(CR.TOL["emu_flips"].values()) <= QUARTER


# ------------------------------------------------------------------------------------------------------------------ the checks bite
B, T, D, K = 3, 100, 72, 31


@pytest.fixture(scope="module")
def base():
    """the bf16 emulation of B3-T100-D72-K31-same-b2 and the fp32 pieces the defects are built from"""
    inp, _ = CR.case_inputs(B, T, D, K, 0, 1, 0.01)
    e = CR.emulate(inp, "bf16")
    a, sg, g, _ = CR.glu_parts(inp["y2"], inp["b2"], F32, True)
    c32, _ = CR.conv_fwd(g, inp["cw"], inp["cb"], 15)
    run_checks(inp, "bf16", e)                               # the undamaged emulation passes
    return inp, e, {"a": a, "sg": sg, "g": g, "c32": c32}


def rejected(inp, io, out, stage, name, tile=64):
    with pytest.raises(CR.Mismatch) as ei:
        run_checks(inp, io, out, tile)
    assert (ei.value.stage, ei.value.name) == (stage, name), str(ei.value)
    return ei.value


@pytest.mark.parametrize("tile,b,t", [(64, 1, 64), (32, 0, 32), (32, 2, 96)])
def test_dropped_halo_tap_at_a_tile_edge(base, tile, b, t):
    """the first frame of a time tile misses the tap that reads the last frame of the tile before"""
    inp, e, p = base
    out = dict(e)
    k = 15 - 1                                               # reads g[t + k - pad_l] = g[t - 1]
    out["c"] = e["c"].clone()
    out["c"][b, t] = (p["c32"][b, t] - inp["cw"][:, k] * p["g"][b, t - 1]).to(BF16)
    err = rejected(inp, "bf16", out, "conv", "c_save", tile)
    assert err.first[:2] == (b, t)
    assert f"time tile {t // tile} position 0 of {tile}" in str(err) and "within K-1 of a tile edge (start" in str(err)


def test_pad_left_off_by_one(base):
    inp, e, _ = base
    err = rejected(inp, "bf16", CR.emulate(inp, "bf16", pad_l=16), "conv", "c_save")
    assert err.first[:2] == (0, 0) and "within K-1 of the utterance's start" in str(err)


@pytest.mark.parametrize("causal", [0, 1])
def test_causal_and_centred_padding_swapped_for_k3(causal):
    inp, _ = CR.case_inputs(3, 100, 72, 3, causal, 1, 0.01)
    run_checks(inp, "bf16", CR.emulate(inp, "bf16"))
    rejected(inp, "bf16", CR.emulate(inp, "bf16", pad_l=CR.pad_left(3, not causal)), "conv", "c_save")


def test_halo_read_from_the_next_utterance(base):
    """the frames behind the end of utterance 0 read the first rows of utterance 1 (a clamp or a zero fill forgotten)"""
    inp, e, p = base
    ext = torch.cat([p["g"][0:1], p["g"][1:2, :K - 1]], 1)
    leak, _ = CR.conv_fwd(ext, inp["cw"], inp["cb"], 15)
    out = dict(e)
    out["c"] = e["c"].clone()
    out["c"][0] = leak[0, :T].to(BF16)
    err = rejected(inp, "bf16", out, "conv", "c_save")
    assert err.first[:2] == (0, T - 15) and "within K-1 of the utterance's end" in str(err)


def _ln_pieces(inp, e):
    """d = LeakyReLU'(dz) and h of the emulation's own state, float64"""
    c, mu, rs = e["c"].to(F64), e["mean"].to(F64)[..., None], e["rstd"].to(F64)[..., None]
    h = (c - mu) * rs
    y = h * inp["gamma"].to(F64) + inp["beta"].to(F64)
    dz = inp["dz"].to(F64)
    return torch.where(y <= 0, dz * inp["slope"], dz), h, y


@pytest.mark.parametrize("name", ["dgamma", "dbeta"])
def test_layernorm_gradient_includes_a_tiles_halo_rows(base, name):
    """the one-launch backward recomputes the LayerNorm backward of its halo rows; they belong to dc only"""
    inp, e, _ = base
    d, h, _ = _ln_pieces(inp, e)
    halo = list(range(32 - 15, 32)) + list(range(64, 64 + 15))          # tile 1 of utterance 0 at 32 frames
    out = dict(e)
    extra = (d * h if name == "dgamma" else d)[0, halo].sum(0)
    out[name] = (e[name].to(F64) + extra).float()
    rejected(inp, "bf16", out, "bwd", name, 32)


@pytest.mark.parametrize("name", ["dconv_w", "dconv_b", "db2"])
def test_a_time_tiles_slab_row_is_missing(base, name):
    """tile 1 (frames 64..99) of utterance 0 never reaches the reduction"""
    inp, e, p = base
    dc = e["dc"].to(F64).clone()
    rest = dc.clone()
    rest[0, 64:] = 0
    part, _ = CR.conv_bwd(rest, rest.abs(), p["a"].to(F64), p["sg"].to(F64), p["g"].to(F64), inp["cw"], 15)
    out = dict(e)
    if name == "db2":                                        # db2 sums dy2's halves over the tile's own frames
        full, _ = CR.conv_bwd(dc, dc.abs(), p["a"].to(F64), p["sg"].to(F64), p["g"].to(F64), inp["cw"], 15)
        dy = full["dy2"].clone()
        dy[0, 64:] = 0
        out[name] = dy.sum((0, 1)).float()
    else:
        out[name] = part[name].float()
    err = rejected(inp, "bf16", out, "bwd", name)
    assert err.first is not None and ("tap=" in str(err)) == (name == "dconv_w")


def test_db2_halves_swapped(base):
    inp, e, _ = base
    out = dict(e)
    out["db2"] = torch.cat([e["db2"][D:], e["db2"][:D]])
    err = rejected(inp, "bf16", out, "bwd", "db2")
    assert "value half" in str(err)


@pytest.mark.parametrize("name", ["dgamma", "dbeta"])
def test_mask_taken_with_less_than_zero(base, name):
    """slope 0 and gamma = beta = 0 in channel 5: its pre-activation is exactly 0 in every row, where the kernels' `<= 0` gives no gradient
    and `< 0` would pass dz on"""
    inp, _, _ = base
    inp = dict(inp, slope=0.0, gamma=inp["gamma"].clone(), beta=inp["beta"].clone())
    inp["gamma"][5], inp["beta"][5] = 0.0, 0.0
    e = CR.emulate(inp, "bf16")
    run_checks(inp, "bf16", e)
    _, h, y = _ln_pieces(inp, e)
    assert bool((y[..., 5] == 0).all())
    dz = inp["dz"].to(F64)
    out = dict(e)
    out[name] = e[name].clone()
    out[name][5] = float((dz * h if name == "dgamma" else dz)[..., 5].sum())
    err = rejected(inp, "bf16", out, "bwd", name)
    assert err.first == (5,)


def test_dc_left_unrounded(base):
    """dy2 computed from the fp32 dc instead of the bf16 value the pair stores: every element stays inside the flip allowance, far too
    many need it"""
    inp, e, p = base
    dc, _, _, A_dc, _, _, _ = CR.ln_bwd(inp["dz"].float(), e["c"].float(), e["mean"], e["rstd"], inp["gamma"], inp["beta"], inp["slope"])
    o, _ = CR.conv_bwd(dc, A_dc, p["a"], p["sg"], p["g"], inp["cw"], 15)
    out = dict(e)
    out["dy2"] = o["dy2"].to(BF16)
    err = rejected(inp, "bf16", out, "bwd", "dy2")
    assert "over the tight bound" in str(err) or "outside the bound" in str(err)


@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("chunks", [(7,), (40,), (1,)])
def test_stream_history_one_row_late(io, chunks):
    inp = CR.stream_inputs(31, 144)
    zs, hs, _ = CR.emulate_stream(inp, io, chunks)
    CR.check_stream(inp, io, chunks, zs, hs, DELTA[io])
    zs, hs, _ = CR.emulate_stream(inp, io, chunks, late=1)
    with pytest.raises(CR.Mismatch) as ei:
        CR.check_stream(inp, io, chunks, zs, hs, DELTA[io])
    assert (ei.value.stage, ei.value.name) == ("stream", "hist"), str(ei.value)
    assert "chunk 0" in str(ei.value)


def test_a_dropped_tap_is_invisible_to_a_whole_tensor_norm(base):
    """the dropped halo tap that check_conv names above moves z by far less than the 2e-2 whole-tensor relative L2 the gradients were held to"""
    inp, e, p = base
    c = p["c32"].clone()
    c[1, 64] = c[1, 64] - inp["cw"][:, 14] * p["g"][1, 63]
    _, _, _, z = CR.ln_fwd(c.to(BF16).float(), inp["gamma"], inp["beta"], inp["slope"], True)
    ref = CR.model(inp, rounding=False)["z"]
    rel = float((z.double() - ref).norm() / ref.norm())
    assert rel < 2e-2, rel
