"""float64 model, stage checks and fp32 emulation for the Conformer convolution core (csrc/convmod.hip, convmod_stream_kernel of
csrc/stream.hip). Test infrastructure only, CPU only; tests/test_convmod_paths_gpu.py applies it to every kernel path,
tests/test_convmod_ref_cpu.py proves that it can fail.

    z = LeakyReLU(LN(dwconv(GLU(y2 + b2)) + conv_b)), channels-last: y2 [B, T, 2D] -> z [B, T, D]; conv_w [D, K], pad_l = K - 1 (causal) or
    (K - 1) / 2; slope < 0 means no activation.

MODEL. model() runs the chain free in a chosen dtype. float64 with the kernels' rounding points (c where c_save is stored, dc where the pair
stores it and the one-launch kernel converts it, z and dy2 on store; the GLU tile and every sum unrounded) is the model; rounding=False is the
pure float64 operation (= autograd through F.conv1d / F.layer_norm / F.leaky_relu); dtype=float32, fast=True is the emulation of the kernels'
arithmetic (taps summed in the kernels' order, bias first; sigmoid as 1 / (1 + exp(-x))) that the bounds in TOL are derived from
(`python tests/helpers/convmod_ref.py` prints the derivation).

STAGE CHECKS. Every stage is judged from the KERNEL'S OWN state, so that one bf16 flip in c is not charged to the LayerNorm:
  check_conv    c_save against the float64 convolution of the float64 GLU
  check_ln      mean, rstd, z against float64 LayerNorm + activation of the kernel's own c_save
  check_bwd     dy2 and the five parameter gradients against the float64 backward from the kernel's own c_save, mean and rstd
  check_stream  z of every chunk and the history after every chunk against the model run over the whole causal sequence
Element-wise: |got - ref| <= delta A for fp32 outputs, delta A + 1/2 ulp_bf16(ref) for bf16 outputs, A = the sum of the absolute values of
the terms that make the element (and, where an unreturned intermediate feeds it, of that intermediate's own A). bf16 dy2 also sees one-ulp
flips of the internal dc: an element over the tight bound is accepted only within sum_k |w_k| ulp_bf16(dc_ref[t - k + pad_l]) of the
reference, and the share of such elements per case stays under TOL["flips"]. (The streamed z sees flips of the unreturned c the same way:
accepted within rstd |gamma| (ulp(c_ref) + 2 max_j ulp(c_ref_j) (1 + |h_i h_j|) / D) - its own flip and two more in its row through the
row statistics - under the same cap.) The fp32 parameter gradients of the bf16 paths sum those flips too; their delta is derived from an
emulation that has them, so it is wider than the fp32 paths' (TOL is per io dtype).
A failure names the first wrong (b, t, channel) - (channel, tap) for dconv_w - with its time tile and position (64 frames for the pair, 32
for the one-launch kernels), its 64-channel tile, and whether the frame lies within K - 1 of a tile edge or of the utterance's ends.

THE KINK. The backward multiplies dz by slope where h gamma + beta <= 0; an element within fp32 noise of zero may take either branch.
Nothing is excluded: case_inputs() moves to the next seed until no pre-activation of the case has |y| < KINK_MARGIN, in the bf16 and in the
fp32 model alike (both io dtypes run the same inputs: y2 and dz hold bf16 values). SEEDS records the seed offset each case ends on."""
import functools
import math

import torch
import torch.nn.functional as Fn

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS = 1e-5
KS = (31, 15, 7, 3)
ROW_FLOOR = 0.1
PARAMS = ("dgamma", "dbeta", "dconv_b", "db2", "dconv_w")
TILE = {"pair": 64, "fused": 32, "stream": 1}


class Mismatch(AssertionError):
    def __init__(self, msg, stage=None, name=None, first=None):
        super().__init__(msg)
        self.stage, self.name, self.first = stage, name, first


# ------------------------------------------------------------------------------------------------------------------ the case matrix
PATHS = ("pair f32", "pair bf16", "fused bf16")


def matrix():
    """(group, path, B, T, D, K, causal, bias, slope) of every training case of tests/test_convmod_paths_gpu.py."""
    m = []
    for K in KS:                                             # K x padding x bias on every path; T = 100 = 64 + 36 = 3 x 32 + 4
        for causal in (0, 1):
            for bias in (1, 0):
                m += [("kpb", p, 3, 100, D, K, causal, bias, 0.01) for p, D in (("fused bf16", 256), ("pair bf16", 256), ("pair f32", 72), ("pair bf16", 72))]
    for K in (31, 3):                                        # time edges
        for causal in (0, 1):
            for T in sorted({1, 2, K // 2, K - 1, K, 31, 32, 33, 63, 64, 65, 129}):
                m += [("time", p, 2, T, D, K, causal, 1, 0.01) for p, D in (("pair f32", 72), ("pair bf16", 72), ("fused bf16", 256))]
    for K, causal in ((31, 0), (7, 1)):                      # channel edges: the partial 64-channel tile, every LayerNorm dispatch step
        for D in (8, 72, 144, 256, 264, 520, 1032, 2048):
            m += [("chan", p, 2, 70, D, K, causal, 1, 0.01) for p in ("pair f32", "pair bf16")]
    for slope in (0.01, 0.0, -1.0):                          # activation
        m += [("act", p, 2, 70, D, 15, 0, 1, slope) for p, D in (("pair f32", 72), ("pair bf16", 72), ("fused bf16", 256))]
    return m


STREAM_T = 50
STREAM = [(31, 144, (1,)), (31, 144, (7,)), (31, 256, (30,)), (31, 256, (40,)), (3, 72, (1,)), (3, 72, (5,)), (7, 2048, (6,)), (15, 8, (14,)),
          (31, 144, (5, 1, 17))]                             # (K, D, chunk list), B = 2, T = 50, both dtypes
STREAM_ACT = [(7, 72, (5,), 0.0), (7, 72, (5,), -1.0)]      # (K, D, chunk list, slope): ReLU and no activation; STREAM runs slope 0.01
OPS = [("pair f32", 3, 100, 72, 31, 0), ("pair bf16", 3, 100, 72, 15, 1), ("fused bf16", 3, 100, 256, 31, 0)]      # (path, B, T, D, K, causal), b2 = None


def io_of(path):
    return "f32" if path.endswith("f32") else "bf16"


def case_key(B, T, D, K, causal, bias, slope):
    return f"B{B}-T{T}-D{D}-K{K}-{'causal' if causal else 'same'}-{'b2' if bias else 'nob2'}-s{slope:g}"


def case_seed(B, T, D, K, causal, bias):
    return ((((B * 1009 + T) * 4099 + D) * 37 + K) * 2 + int(causal)) * 2 + int(bias)


def pad_left(K, causal):
    return K - 1 if causal else (K - 1) // 2


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def bf(x):
    return x.to(BF16).to(x.dtype)


def rnd(x, io):
    """round to the io dtype, keep the dtype"""
    return x.to(BF16 if io == "bf16" else F32).to(x.dtype)


def ulp_bf16(ref):
    """one unit in the last place of bf16 at |ref|: 2^(floor(log2 |ref|) - 7); 0 at 0"""
    r = ref.abs().to(F64)
    _, e = torch.frexp(r)
    return torch.where(r > 0, torch.ldexp(torch.ones_like(r), e - 8), torch.zeros_like(r))


def _sig(x, fast):
    return 1.0 / (1.0 + torch.exp(-x)) if fast else torch.sigmoid(x)


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32)


def glu_parts(y2, b2, dt=F64, fast=False):
    """-> a (value half + bias), sg (sigmoid of the gate half + bias), g = a sg, A_g (the magnitude of g's terms)"""
    D = y2.shape[-1] // 2
    a, gt = y2[..., :D].to(dt), y2[..., D:].to(dt)
    A = a.abs()
    if b2 is not None:
        a, gt, A = a + b2[:D].to(dt), gt + b2[D:].to(dt), A + b2[:D].to(dt).abs()
    sg = _sig(gt, fast)
    return a, sg, a * sg, A * sg


def conv_fwd(g, cw, cb, pad_l):
    """bias first, then the taps k = 0 .. K - 1 (the kernels' order) -> c, A_c; g [B, T, D], zero outside [0, T)"""
    B, T, D = g.shape
    K = cw.shape[1]
    gp = Fn.pad(g, (0, 0, pad_l, K - 1 - pad_l))
    w = cw.to(g.dtype)
    acc = cb.to(g.dtype).expand(B, T, D).clone()
    A = acc.abs()
    for k in range(K):
        term = w[:, k] * gp[:, k:k + T]
        acc, A = acc + term, A + term.abs()
    return acc, A


def ln_fwd(c, gamma, beta, slope, fast=False):
    D = c.shape[-1]
    mu = c.sum(-1) / D
    q = ((c - mu[..., None]) ** 2).sum(-1) / D
    rs = torch.rsqrt(q + EPS) if fast else 1.0 / torch.sqrt(q + EPS)
    y = (c - mu[..., None]) * rs[..., None] * gamma.to(c.dtype) + beta.to(c.dtype)
    return mu, rs, y, (y if slope < 0 else torch.where(y > 0, y, y * slope))


def ln_bwd(dz, c, mu, rs, gamma, beta, slope):
    """layernorm_bwd_kernel's formulas -> dc (unrounded), dgamma, dbeta, and their magnitudes A_dc, A_dgamma, A_dbeta, and y"""
    D = c.shape[-1]
    ga, rs1 = gamma.to(c.dtype), rs[..., None]
    h = (c - mu[..., None]) * rs1
    y = h * ga + beta.to(c.dtype)
    d = dz if slope < 0 else torch.where(y <= 0, dz * slope, dz)
    gd = d * ga
    m1, m2 = gd.sum(-1, keepdim=True) / D, (gd * h).sum(-1, keepdim=True) / D
    dc = rs1 * (gd - m1 - h * m2)
    A_dc = rs1 * (gd.abs() + gd.abs().sum(-1, keepdim=True) / D + h.abs() * (gd * h).abs().sum(-1, keepdim=True) / D)
    return dc, (d * h).sum((0, 1)), d.sum((0, 1)), A_dc, (d * h).abs().sum((0, 1)), d.abs().sum((0, 1)), y


def conv_bwd(dc, A_dc, a, sg, g, cw, pad_l):
    """glu_dwconv_bwd_kernel's formulas: dg[t] = sum_k w[k] dc[t - k + pad_l], taps k = 0 .. K - 1 in order -> values and magnitudes"""
    B, T, D = dc.shape
    K = cw.shape[1]
    w = cw.to(dc.dtype)
    dcp, Ap = Fn.pad(dc, (0, 0, K - 1 - pad_l, pad_l)), Fn.pad(A_dc, (0, 0, K - 1 - pad_l, pad_l))
    gp = Fn.pad(g, (0, 0, pad_l, K - 1 - pad_l))
    dg, A_dg = torch.zeros_like(dc), torch.zeros_like(dc)
    dw, A_dw = dc.new_empty(D, K), dc.new_empty(D, K)
    for k in range(K):
        dg = dg + w[:, k] * dcp[:, K - 1 - k:K - 1 - k + T]
        A_dg = A_dg + w[:, k].abs() * Ap[:, K - 1 - k:K - 1 - k + T]
        dw[:, k] = (dc * gp[:, k:k + T]).sum((0, 1))
        A_dw[:, k] = (A_dc * gp[:, k:k + T].abs()).sum((0, 1))
    da, db = dg * sg, dg * a * sg * (1.0 - sg)
    A_da, A_db = A_dg * sg, A_dg * a.abs() * sg * (1.0 + sg)           # the difference 1 - sg taken as 1 + sg: its fp32 error is 2^-24 of 1
    out = {"dy2": torch.cat([da, db], -1), "dconv_b": dc.sum((0, 1)), "db2": torch.cat([da.sum((0, 1)), db.sum((0, 1))]), "dconv_w": dw}
    A = {"dy2": torch.cat([A_da, A_db], -1), "dconv_b": A_dc.sum((0, 1)), "db2": torch.cat([A_da.sum((0, 1)), A_db.sum((0, 1))]), "dconv_w": A_dw}
    return out, A


# ------------------------------------------------------------------------------------------------------------------ the free-running chain
def model(inp, io="bf16", dtype=F64, fast=False, rounding=True, pad_l=None):
    """Forward and backward, run free in `dtype`. inp: dict(y2, b2, cw, cb, gamma, beta, dz, K, causal, slope). -> dict of c (as c_save), mean,
    rstd, y (pre-activation), z, dc, dy2, dgamma, dbeta, dconv_b, db2, dconv_w, g."""
    r = (lambda v: rnd(v, io)) if rounding else (lambda v: v)
    pl = pad_left(inp["K"], inp["causal"]) if pad_l is None else pad_l
    a, sg, g, _ = glu_parts(inp["y2"], inp["b2"], dtype, fast)
    c, _ = conv_fwd(g, inp["cw"], inp["cb"], pl)
    c = r(c)
    mu, rs, y, z = ln_fwd(c, inp["gamma"], inp["beta"], inp["slope"], fast)
    out = {"g": g, "c": c, "mean": mu, "rstd": rs, "y": y, "z": r(z)}
    if inp.get("dz") is not None:
        dc, dgam, dbet, A_dc, _, _, _ = ln_bwd(inp["dz"].to(dtype), c, mu, rs, inp["gamma"], inp["beta"], inp["slope"])
        dc = r(dc)
        o, _ = conv_bwd(dc, A_dc, a, sg, g, inp["cw"], pl)
        out.update(o, dc=dc, dgamma=dgam, dbeta=dbet)
        out["dy2"] = r(out["dy2"])
    return out


def emulate(inp, io, **kw):
    """the fp32 emulation in the kernels' storage dtypes: c, z, dy2 in the io dtype, mean / rstd and the parameter gradients fp32"""
    e = model(inp, io, F32, fast=True, **kw)
    st = BF16 if io == "bf16" else F32
    for k in ("c", "z", "dy2"):
        if k in e:
            e[k] = e[k].to(st)
    return e


def autograd_reference(inp):
    """float64 autograd through F.conv1d(groups=D) / F.layer_norm / F.leaky_relu on the transposed layout: what rounding=False must equal"""
    K, D = inp["K"], inp["cw"].shape[0]
    names = ("y2", "b2", "cw", "cb", "gamma", "beta")
    p = {k: (None if inp[k] is None else inp[k].to(F64).clone().requires_grad_()) for k in names}
    h = p["y2"] if p["b2"] is None else p["y2"] + p["b2"]
    gl = (h[..., :D] * torch.sigmoid(h[..., D:])).transpose(1, 2)
    gl = Fn.pad(gl, (K - 1, 0)) if inp["causal"] else Fn.pad(gl, ((K - 1) // 2, (K - 1) // 2))
    c = Fn.conv1d(gl, p["cw"].view(D, 1, K), p["cb"], groups=D).transpose(1, 2)
    z = Fn.layer_norm(c, (D,), p["gamma"], p["beta"], EPS)
    if inp["slope"] >= 0:
        z = Fn.leaky_relu(z, inp["slope"])
    z.backward(inp["dz"].to(F64))
    out = {"c": c.detach(), "z": z.detach(), "dy2": p["y2"].grad, "dconv_w": p["cw"].grad, "dconv_b": p["cb"].grad, "dgamma": p["gamma"].grad,
           "dbeta": p["beta"].grad}
    if p["b2"] is not None:
        out["db2"] = p["b2"].grad
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs
def draw(B, T, D, K, bias, seed):
    """The scales of the existing tests: y2, dz = randn (bf16 values, which both io dtypes run), b2, conv_b, beta = 0.1 randn, conv_w = randn /
    sqrt(K), gamma = +-(1 + 0.1 randn) with both signs. Ragged data: utterance b > 0 has y2 = dz = 0 from frame T - b max(1, T / 5) on, so
    that a row read across the batch boundary is a different row."""
    g = torch.Generator().manual_seed(seed)
    y2 = torch.randn(B, T, 2 * D, generator=g)
    b2 = torch.randn(2 * D, generator=g) * 0.1
    cw, cb = torch.randn(D, K, generator=g) / math.sqrt(K), torch.randn(D, generator=g) * 0.1
    gamma, beta = torch.randn(D, generator=g) * 0.1 + 1, torch.randn(D, generator=g) * 0.1
    gamma = gamma * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)
    dz = torch.randn(B, T, D, generator=g)
    for b in range(1, B):
        n = max(1, T - b * max(1, T // 5))
        y2[b, n:], dz[b, n:] = 0, 0
    return {"y2": bf(y2), "b2": b2 if bias else None, "cw": cw, "cb": cb, "gamma": gamma, "beta": beta, "dz": bf(dz)}


def min_abs_y(inp):
    """the smallest |pre-activation| of the bf16 and of the fp32 model"""
    return min(float(model({**inp, "dz": None}, io)["y"].abs().min()) for io in ("bf16", "f32"))


@functools.lru_cache(maxsize=None)
def _case(B, T, D, K, causal, bias, slope, start):
    base, n = case_seed(B, T, D, K, causal, bias), start
    while True:
        inp = draw(B, T, D, K, bias, base + 7919 * n)
        inp.update(K=K, causal=int(causal), slope=float(slope))
        if (slope < 0 or min_abs_y(inp) >= KINK_MARGIN) and max(emu_flip_shares(inp).values()) <= TOL["flips"] / 4:
            return inp, n
        n += 1


def emu_flip_shares(inp):
    """the shares of c_save, z and dy2 of the bf16 emulation that are not the nearest bf16 of the stage reference"""
    e, inf = emulate(inp, "bf16"), {k: float("inf") for k in ("c", "mean", "rstd", "z", "dy2") + PARAMS}
    st = check_conv(inp, "bf16", e["c"], inf)
    st.update(check_ln(inp, "bf16", e["c"], e["mean"], e["rstd"], e["z"], inf))
    st.update(check_bwd(inp, "bf16", e["c"], e["mean"], e["rstd"], e["dy2"], {}, inf, flip_cap=1.0))
    return {k: v for k, v in st.items() if k.endswith("_flips")}


def case_inputs(B, T, D, K, causal, bias, slope, search=False):
    """-> (inputs, seed offset). The draw moves to the next seed until no pre-activation lies within KINK_MARGIN of the kink (slope < 0: no
    kink) and the bf16 emulation's flip shares are within a quarter of the cap (a case of 144 elements cannot afford one flip). By default
    the search starts at the offset recorded in SEEDS (search=True: at 0, which must end on the same one)."""
    start = 0 if search else SEEDS.get(case_key(B, T, D, K, causal, bias, slope), 0)
    inp, n = _case(B, T, D, K, int(causal), int(bias), float(slope), start)
    return dict(inp), n


def all_case_keys():
    ks = {(B, T, D, K, causal, bias, slope) for _, _, B, T, D, K, causal, bias, slope in matrix()}
    ks |= {(B, T, D, K, causal, bias, 0.01) for _, B, T, D, K, causal in OPS for bias in (0, 1)}
    return sorted(ks)


def stream_inputs(K, D, B=2, T=STREAM_T, slope=0.01):
    inp = draw(B, T, D, K, True, 424243 + 131 * K + D)
    inp.update(K=K, causal=1, slope=slope, dz=None)
    return inp


# ------------------------------------------------------------------------------------------------------------------ the checker
def where(b, t, d, T, K, tile):
    """the structure an element belongs to"""
    pos = t % tile
    s = f"time tile {t // tile} position {pos} of {tile}, channel tile {d // 64} channel {d % 64}"
    notes = []
    if tile > 1 and (pos < K - 1 or tile - 1 - pos < K - 1):
        notes.append("within K-1 of a tile edge (" + " and ".join(n for n, c in (("start", pos < K - 1), ("end", tile - 1 - pos < K - 1)) if c) + ")")
    if t < K - 1:
        notes.append("within K-1 of the utterance's start")
    if T - 1 - t < K - 1:
        notes.append("within K-1 of the utterance's end")
    return s + (": " + ", ".join(notes) if notes else ": interior")


def _fail(stage, name, bad, diff, bound, got, ref, what, describe):
    idx = torch.nonzero(bad)
    first = tuple(int(v) for v in idx[0])
    excess = torch.where(bad, diff - bound, torch.full_like(diff, -1.0))
    worst = tuple(int(v) for v in torch.nonzero(excess == excess.max())[0])

    def show(ix):
        return f"{describe(ix)}: got {float(got[ix])!r}, want {float(ref[ix])!r}, |diff| {float(diff[ix]):.3e} > bound {float(bound[ix]):.3e}"
    raise Mismatch(f"{what} {stage} {name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {show(first)}; worst at {show(worst)}",
                   stage, name, first)


def _judge(stage, name, got, ref, A, delta, half_ulp, what, describe, flip_allow=None, flip_cap=None):
    """-> (worst (|diff| - 1/2 ulp) / A over the elements inside the tight bound, share of elements over it). Raises Mismatch."""
    got, ref = got.to(F64), ref.to(F64)
    diff = (got - ref).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    slack = 0.5 * ulp_bf16(ref) if half_ulp else torch.zeros_like(ref)
    bound = slack + delta * A
    over = diff > bound
    share = 0.0
    if flip_allow is not None and over.any():
        bad = over & (diff > bound + flip_allow)
        if bad.any():
            _fail(stage, name, bad, diff, bound + flip_allow, got, ref, what, describe)
        share = float(over.double().mean())
        if share > flip_cap:
            first = tuple(int(v) for v in torch.nonzero(over)[0])
            raise Mismatch(f"{what} {stage} {name}: {share:.3%} of the elements are over the tight bound (cap {flip_cap:.1%}: they lie within the "
                           f"flip allowance, but so many are no flips); first at {describe(first)}", stage, name, first)
    elif over.any():
        _fail(stage, name, over, diff, bound, got, ref, what, describe)
    live = (A > 0) & ~over if flip_allow is not None else A > 0          # the figure of a flip-affected element is no arithmetic error
    worst = float(((diff - slack).clamp_min(0)[live] / A[live]).max()) if live.any() else 0.0
    return worst, share


def _flips(got, ref, io):
    """share of a bf16 output that is not the nearest bf16 of the reference"""
    if io != "bf16":
        return 0.0
    return float((_bits(got.to(BF16)) != _bits(ref.to(F32).to(BF16))).double().mean())


def _desc3(T, K, tile, half=None):
    def f(ix):
        b, t, d = ix
        dd, part = (d, "") if half is None else (d % half, f" ({'value' if d < half else 'gate'} half)")
        return f"(b={b}, t={t}, channel={dd}){part} = {where(b, t, dd, T, K, tile)}"
    return f


def check_conv(inp, io, c_k, delta, tile=64, what=""):
    """c_save against the float64 convolution of the float64 GLU -> {"c": worst relative to A, "c_flips"}"""
    K, T = inp["K"], c_k.shape[1]
    _, _, g, A_g = glu_parts(inp["y2"], inp["b2"])
    ref, _ = conv_fwd(g, inp["cw"], inp["cb"], pad_left(K, inp["causal"]))
    _, A = conv_fwd(A_g, inp["cw"].abs(), inp["cb"].abs(), pad_left(K, inp["causal"]))
    w, _ = _judge("conv", "c_save", c_k, ref, A, delta["c"], io == "bf16", what, _desc3(T, K, tile))
    return {"c": w, "c_flips": _flips(c_k, ref, io)}


def check_ln(inp, io, c_k, mean_k, rstd_k, z_k, delta, tile=64, what=""):
    """mean, rstd and z against float64 LayerNorm + activation of the kernel's own c_save"""
    K, (B, T, D) = inp["K"], c_k.shape
    c = c_k.to(F64)
    mu, rs, y, z = ln_fwd(c, inp["gamma"], inp["beta"], inp["slope"])
    row = lambda ix: f"(b={ix[0]}, t={ix[1]}) = time tile {ix[1] // tile} position {ix[1] % tile} of {tile}"  # noqa: E731
    st = {}
    st["mean"], _ = _judge("ln", "mean", mean_k.view(B, T), mu, c.abs().sum(-1) / D, delta["mean"], False, what, row)
    st["rstd"], _ = _judge("ln", "rstd", rstd_k.view(B, T), rs, rs, delta["rstd"], False, what, row)
    cabs = c.abs() + c.abs().sum(-1, keepdim=True) / D
    A = cabs * rs[..., None] * inp["gamma"].to(F64).abs() + inp["beta"].to(F64).abs()
    if inp["slope"] >= 0:
        A = torch.where(y > -KINK_MARGIN, A, A * inp["slope"])
    st["z"], _ = _judge("ln", "z", z_k, z, A, delta["z"], io == "bf16", what, _desc3(T, K, tile))
    st["z_flips"] = _flips(z_k, z, io)
    return st


def split_dparams(dpar, D, K):
    """the packed fp32 [dgamma D | dbeta D | dconv_b D | db2 2D | dconv_w D K] of tsasr_convmod_bwd"""
    return {"dgamma": dpar[:D], "dbeta": dpar[D:2 * D], "dconv_b": dpar[2 * D:3 * D], "db2": dpar[3 * D:5 * D], "dconv_w": dpar[5 * D:5 * D + D * K].view(D, K)}


def bwd_reference(inp, io, c_k, mean_k, rstd_k, dc_own=None):
    """float64 backward from the kernel's own c_save, mean, rstd -> (ref, A, y): dc rounded to the io dtype (dc_own: the emulation's own dc
    instead, for the derivation of the tight dy2 bound), dy2 unrounded"""
    B, T, D = c_k.shape
    a, sg, g, _ = glu_parts(inp["y2"], inp["b2"])
    dc, dgam, dbet, A_dc, A_dgam, A_dbet, y = ln_bwd(inp["dz"].to(F64), c_k.to(F64), mean_k.view(B, T).to(F64), rstd_k.view(B, T).to(F64),
                                                     inp["gamma"], inp["beta"], inp["slope"])
    dc = rnd(dc, io) if dc_own is None else dc_own.to(F64)
    ref, A = conv_bwd(dc, A_dc, a, sg, g, inp["cw"], pad_left(inp["K"], inp["causal"]))
    ref.update(dgamma=dgam, dbeta=dbet, dc=dc)
    A.update(dgamma=A_dgam, dbeta=A_dbet)
    return ref, A, y


def check_bwd(inp, io, c_k, mean_k, rstd_k, dy2_k, dpar_k, delta, tile=64, what="", flip_cap=None, dc_own=None):
    """dy2 and the five parameter gradients (dpar_k: the packed dparams, or a dict of them; db2 is skipped when the case has no b2 and the dict
    has none) -> worst relative to A per quantity, "dy2_over" (share over the tight bound), "dy2_flips", "min_abs_y" """
    K, (B, T, D) = inp["K"], c_k.shape
    pl = pad_left(K, inp["causal"])
    ref, A, y = bwd_reference(inp, io, c_k, mean_k, rstd_k, dc_own)
    st = {"min_abs_y": float(y.abs().min()) if inp["slope"] >= 0 else float("inf")}
    allow = None
    if io == "bf16":                                         # one-ulp flips of the internal dc: sum_k |w_k| ulp(dc_ref[t - k + pad_l])
        up = Fn.pad(ulp_bf16(ref["dc"]), (0, 0, K - 1 - pl, pl))
        allow = torch.zeros_like(ref["dc"])
        for k in range(K):
            allow = allow + inp["cw"][:, k].to(F64).abs() * up[:, K - 1 - k:K - 1 - k + T]
        allow = torch.cat([allow, allow], -1)
    st["dy2"], st["dy2_over"] = _judge("bwd", "dy2", dy2_k, ref["dy2"], A["dy2"], delta["dy2"], io == "bf16", what, _desc3(T, K, tile, D), allow,
                                       TOL["flips"] if flip_cap is None else flip_cap)
    st["dy2_flips"] = _flips(dy2_k, ref["dy2"], io)
    got = dpar_k if isinstance(dpar_k, dict) else split_dparams(dpar_k, D, K)
    for name in PARAMS:
        if name not in got:
            continue
        if name == "dconv_w":
            desc = lambda ix: f"(channel={ix[0]}, tap={ix[1]}) = channel tile {ix[0] // 64} channel {ix[0] % 64}"  # noqa: E731
        elif name == "db2":
            desc = lambda ix: f"(channel={ix[0] % D}, {'value' if ix[0] < D else 'gate'} half) = channel tile {ix[0] % D // 64}"  # noqa: E731
        else:
            desc = lambda ix: f"(channel={ix[0]}) = channel tile {ix[0] // 64} channel {ix[0] % 64}"  # noqa: E731
        st[name], _ = _judge("bwd", name, got[name], ref[name], A[name], delta[name], False, what, desc)
    return st


# ------------------------------------------------------------------------------------------------------------------ streaming
def stream_chunks(T, chunks):
    out, t0, i = [], 0, 0
    while t0 < T:
        c = min(chunks[i % len(chunks)], T - t0)
        out.append((t0, c))
        t0, i = t0 + c, i + 1
    return out


def emulate_stream(inp, io, chunks, late=0):
    """convmod_stream_kernel chunk by chunk in fp32 (history carried as fp32 GLU rows) -> [z per chunk], [history after each chunk].
    late: the history written `late` rows late (a planted defect for the CPU test)."""
    B, T, D2 = inp["y2"].shape
    D, K = D2 // 2, inp["K"]
    hist = torch.zeros(B, K - 1, D)
    zs, hs, cs = [], [], []
    for t0, c in stream_chunks(T, chunks):
        _, _, g, _ = glu_parts(inp["y2"][:, t0:t0 + c], inp["b2"], F32, True)
        ext = torch.cat([hist, g], 1)
        cc, _ = conv_fwd(ext, inp["cw"], inp["cb"], 0)
        cc = rnd(cc[:, :c], io)
        cs.append(cc)
        _, _, _, z = ln_fwd(cc, inp["gamma"], inp["beta"], inp["slope"], True)
        zs.append(z.to(BF16 if io == "bf16" else F32))
        hist = ext[:, c - late:c - late + K - 1].clone() if late else ext[:, c:c + K - 1].clone()
        hs.append(hist)
    return zs, hs, torch.cat(cs, 1)


def check_stream(inp, io, chunks, zs, hists, delta, what="", c_own=None):
    """z of every chunk and the history after every chunk against the float64 model over the whole causal sequence; history rows that a
    chunk shorter than K - 1 carries over must be the previous buffer's rows bit for bit."""
    B, T, D2 = inp["y2"].shape
    D, K = D2 // 2, inp["K"]
    _, _, g, A_g = glu_parts(inp["y2"], inp["b2"])
    c, _ = conv_fwd(g, inp["cw"], inp["cb"], K - 1)
    _, A_c = conv_fwd(A_g, inp["cw"].abs(), inp["cb"].abs(), K - 1)
    c = rnd(c, io) if c_own is None else c_own.to(F64)        # c_own: the emulation's own c, for the derivation of the tight bound
    mu, rs, y, z = ln_fwd(c, inp["gamma"], inp["beta"], inp["slope"])
    h, rs1, ga = (c - mu[..., None]) * rs[..., None], rs[..., None], inp["gamma"].to(F64).abs()
    # the conv error (delta A_c, unreturned) reaches z through its own element and the row statistics
    A = rs1 * ga * (A_c + A_c.sum(-1, keepdim=True) / D + h.abs() * (A_c * h.abs()).sum(-1, keepdim=True) / D) + inp["beta"].to(F64).abs()
    neg = inp["slope"] if inp["slope"] >= 0 else 1.0
    A = torch.where(y > -KINK_MARGIN, A, A * neg)
    allow = None
    if io == "bf16":
        u = ulp_bf16(c)
        allow = rs1 * ga * (u + 2 * (u.max(-1, keepdim=True).values + (u * h.abs()).max(-1, keepdim=True).values * h.abs()) / D)
        allow = torch.where(y > -KINK_MARGIN, allow, allow * neg)
    gp = Fn.pad(g, (0, 0, K - 1, 0))                          # ext row e of the whole sequence = frame e - (K - 1)
    Agp = Fn.pad(A_g, (0, 0, K - 1, 0))
    st = {"z": 0.0, "hist": 0.0, "z_over": 0.0}
    over_n, total = 0, 0
    prev = torch.zeros(B, K - 1, D)
    for i, (t0, cn) in enumerate(stream_chunks(T, chunks)):
        w = f"{what} chunk {i} (frames {t0}..{t0 + cn - 1})"
        desc = lambda ix: f"(b={ix[0]}, t={t0 + ix[1]}, channel={ix[2]}) = row {ix[1]} of the chunk"  # noqa: E731
        worst, share = _judge("stream", "z", zs[i], z[:, t0:t0 + cn], A[:, t0:t0 + cn], delta["stream_z"], io == "bf16", w, desc,
                              None if allow is None else allow[:, t0:t0 + cn], 1.0)
        over_n, total = over_n + share * zs[i].numel(), total + zs[i].numel()
        st["z"] = max(st["z"], worst)
        hdesc = lambda ix: f"(b={ix[0]}, history row={ix[1]}, channel={ix[2]}) = frame {t0 + cn - (K - 1) + ix[1]}"  # noqa: E731
        worst, _ = _judge("stream", "hist", hists[i], gp[:, t0 + cn:t0 + cn + K - 1], Agp[:, t0 + cn:t0 + cn + K - 1], delta["hist"], False, w, hdesc)
        st["hist"] = max(st["hist"], worst)
        keep = K - 1 - cn
        if keep > 0 and not torch.equal(_bits(hists[i][:, :keep].float().contiguous()), _bits(prev[:, cn:].float().contiguous())):
            bad = torch.nonzero(_bits(hists[i][:, :keep].float().contiguous()) != _bits(prev[:, cn:].float().contiguous()))[0]
            raise Mismatch(f"{w} stream hist: carried row differs from the previous buffer, first at {hdesc(tuple(int(v) for v in bad))}", "stream", "hist",
                           tuple(int(v) for v in bad))
        prev = hists[i].float()
    st["z_over"] = over_n / max(total, 1)
    if st["z_over"] > TOL["flips"]:
        raise Mismatch(f"{what} stream z: {st['z_over']:.3%} of the elements are over the tight bound (cap {TOL['flips']:.1%})", "stream", "z", None)
    return st


# ------------------------------------------------------------------------------------------------------------------ ops level
def row_errors(name, got, ref):
    """relative L2 per (b, t) row of dy2 / z, per channel of dconv_w, per element of the vectors; "dconv_w/tap": per tap over the channels.
    Rows are judged against max(|ref row|, ROW_FLOOR x the RMS row norm)."""
    g, r = got.to(F64), ref.to(F64)
    if name == "dconv_w/tap":
        g, r = g.t(), r.t()
    elif g.dim() == 1:
        g, r = g[:, None], r[:, None]
    g, r = g.reshape(-1, g.shape[-1]), r.reshape(-1, r.shape[-1])
    rn = r.norm(dim=1)
    floor = ROW_FLOOR * float(rn.pow(2).mean().sqrt())
    e = (g - r).norm(dim=1) / rn.clamp_min(max(floor, 1e-300))
    return torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)


def check_rows(name, got, ref, bound, what=""):
    e = row_errors(name, got, ref)
    if float(e.max()) > bound:
        raise Mismatch(f"{what} {name}: {int((e > bound).sum())} of {e.numel()} rows above {bound:.3e}; first row {int(torch.nonzero(e > bound)[0])}, "
                       f"worst row {int(e.argmax())}: {float(e.max()):.3e}", "ops", name, (int(torch.nonzero(e > bound)[0]),))
    return float(e.max())


OPS_NAMES = ("z", "dy2", "dgamma", "dbeta", "dconv_b", "db2", "dconv_w", "dconv_w/tap")


# ------------------------------------------------------------------------------------------------------------------ the bounds
# delta = 16 x the worst stage-check distance of the fp32 emulation (run free, then checked like a kernel) over matrix() / STREAM, per io
# dtype: the device's v_exp_f32 / v_rcp_f32 / v_rsq_f32 are 1-ulp approximations, FMA contraction and the kernels' row and tile sums run in
# another order, none of which the CPU emulation shares. Each entry: (bound, the CPU measurement it came from), relative to A.
#   bf16 dy2 and the streamed bf16 z are measured against the emulation's OWN dc / c (the flips of that unreturned intermediate are what the
#   flip allowance and the cap are for); the bf16 parameter gradients are measured free-running, flips of dc included, because the kernels'
#   sums include them too - with B T = 2 .. 4 terms (the T = 1, 2 cases) one flipped term is up to 2^-8 of the sum, which is why those
#   three deltas are three orders wider than the fp32 paths'.
# KINK_MARGIN = 64 x the emulation's worst absolute error on a pre-activation y with |y| < KINK_NEAR (derive(): 1.46e-7). The error of y is
# relative to its terms (|c| + |mean|) rstd |gamma| + |beta|; the worst over ALL elements (1.5e-6, at |y| = 6.5) says nothing about the
# neighbourhood of zero, where the mask is decided.
KINK_NEAR = 0.05
KINK_MARGIN = 1e-5
TOL = {
    "flips": 0.01,          # share of a bf16 output that may be other than the nearest bf16 of the reference (dy2, streamed z: that may lie
                            # over the tight bound), per case; the emulation's worst shares over the matrix are in "emu_flips"
    "f32": {"c": (8.00e-06, 5.00e-07), "mean": (2.22e-06, 1.39e-07), "rstd": (2.89e-06, 1.80e-07), "z": (3.68e-06, 2.30e-07),
            "dy2": (4.01e-06, 2.51e-07), "dgamma": (2.59e-06, 1.62e-07), "dbeta": (1.91e-06, 1.19e-07), "dconv_b": (1.30e-06, 8.13e-08),
            "db2": (1.87e-06, 1.17e-07), "dconv_w": (2.64e-06, 1.65e-07), "stream_z": (1.88e-06, 1.18e-07), "hist": (4.22e-06, 2.63e-07)},
    "bf16": {"c": (2.04e-06, 1.27e-07), "mean": (5.54e-07, 3.46e-08), "rstd": (2.99e-06, 1.87e-07), "z": (1.27e-06, 7.92e-08),
             "dy2": (7.04e-07, 4.40e-08), "dgamma": (3.58e-06, 2.24e-07), "dbeta": (2.30e-06, 1.44e-07), "dconv_b": (2.43e-03, 1.52e-04),
             "db2": (1.07e-03, 6.67e-05), "dconv_w": (8.37e-03, 5.23e-04), "stream_z": (3.11e-07, 1.95e-08), "hist": (4.22e-06, 2.63e-07)},
    "emu_flips": {"c_flips": 2.44e-04, "z_flips": 6.51e-04, "dy2_over": 7.00e-04, "dy2_flips": 1.95e-03, "stream_z_over": 8.79e-05},
    # ops level, per path and quantity: (bound = 4 x the emulation's worst row distance to the model over OPS_DRAWS draws of the shape, that
    # distance, the model's own distance to the pure float64 operation). The bound is to stay below a quarter of the third figure. It does
    # for the parameter gradients and dy2 of the bf16 paths, except: z on both bf16 paths and dy2 on the pair (one flipped c in a row of 72
    # or 256 values is already 1.4e-3 of the row, while rounding EVERY element is 3e-3); dbeta on the pair's shapes (a sum of masked dz: no rounding
    # point reaches it unless it turns a mask, the third figure is 0); and nothing on the fp32 path, where the model IS the pure operation to 2^-24 and the
    # emulation's fp32 sums are further from it than that. These bounds still see what a whole-tensor norm could not: one wrong row, channel
    # or tap, and a slice of dparams that reaches the wrong parameter.
    "ops": {
        "pair f32": {"z": (1.27e-06, 3.18e-07, 5.20e-08), "dy2": (9.90e-07, 2.47e-07, 4.55e-08), "dgamma": (1.87e-05, 4.66e-06, 1.57e-07),
                  "dbeta": (7.37e-06, 1.84e-06, 0.00e+00), "dconv_b": (2.25e-05, 5.63e-06, 2.00e-07), "db2": (1.97e-05, 4.93e-06, 2.85e-07),
                  "dconv_w": (1.10e-06, 2.75e-07, 3.83e-08), "dconv_w/tap": (8.74e-07, 2.18e-07, 3.19e-08)},
        "pair bf16": {"z": (5.88e-03, 1.47e-03, 3.37e-03), "dy2": (2.92e-03, 7.31e-04, 3.38e-03), "dgamma": (8.01e-04, 2.00e-04, 1.24e-02),
                   "dbeta": (8.58e-06, 2.15e-06, 0.00e+00), "dconv_b": (8.81e-04, 2.20e-04, 2.28e-02), "db2": (3.82e-04, 9.56e-05, 2.55e-02),
                   "dconv_w": (3.48e-04, 8.71e-05, 2.91e-03), "dconv_w/tap": (7.96e-05, 1.99e-05, 1.96e-03)},
        "fused bf16": {"z": (5.61e-03, 1.40e-03, 2.89e-03), "dy2": (2.69e-03, 6.73e-04, 2.89e-02), "dgamma": (3.12e-03, 7.79e-04, 2.06e-02),
                    "dbeta": (1.10e-05, 2.74e-06, 9.40e-02), "dconv_b": (8.82e-03, 2.21e-03, 8.98e-02), "db2": (1.77e-03, 4.41e-04, 6.07e-02),
                    "dconv_w": (3.03e-03, 7.57e-04, 2.67e-02), "dconv_w/tap": (6.37e-04, 1.59e-04, 6.73e-03)},
    },
}
# seed offset each case's draw ends on (absent: 0), found by case_inputs(search=True)
SEEDS = {
    'B3-T100-D256-K31-same-b2-s0.01': 2, 'B3-T100-D256-K31-same-nob2-s0.01': 2, 'B3-T100-D72-K31-same-nob2-s0.01': 1,
    'B3-T100-D72-K31-causal-nob2-s0.01': 1, 'B3-T100-D256-K15-same-b2-s0.01': 6, 'B3-T100-D256-K15-same-nob2-s0.01': 3,
    'B3-T100-D72-K15-same-nob2-s0.01': 1, 'B3-T100-D256-K15-causal-b2-s0.01': 1, 'B3-T100-D256-K15-causal-nob2-s0.01': 5,
    'B3-T100-D72-K15-causal-nob2-s0.01': 1, 'B3-T100-D256-K7-same-nob2-s0.01': 3, 'B3-T100-D72-K7-same-nob2-s0.01': 2,
    'B3-T100-D256-K7-causal-b2-s0.01': 8, 'B3-T100-D256-K7-causal-nob2-s0.01': 1, 'B3-T100-D256-K3-same-b2-s0.01': 1,
    'B3-T100-D256-K3-same-nob2-s0.01': 1, 'B3-T100-D256-K3-causal-b2-s0.01': 10, 'B3-T100-D72-K3-causal-b2-s0.01': 1,
    'B3-T100-D256-K3-causal-nob2-s0.01': 5, 'B2-T1-D72-K31-same-b2-s0.01': 1, 'B2-T15-D256-K31-same-b2-s0.01': 1, 'B2-T64-D256-K31-same-b2-s0.01': 2,
    'B2-T65-D256-K31-same-b2-s0.01': 1, 'B2-T30-D256-K31-causal-b2-s0.01': 1, 'B2-T33-D256-K31-causal-b2-s0.01': 1, 'B2-T63-D256-K31-causal-b2-s0.01':
    1, 'B2-T65-D256-K31-causal-b2-s0.01': 2, 'B2-T32-D256-K3-same-b2-s0.01': 2, 'B2-T63-D256-K3-same-b2-s0.01': 2, 'B2-T64-D256-K3-same-b2-s0.01': 2,
    'B2-T129-D256-K3-same-b2-s0.01': 1, 'B2-T3-D256-K3-causal-b2-s0.01': 1, 'B2-T31-D256-K3-causal-b2-s0.01': 3, 'B2-T33-D256-K3-causal-b2-s0.01': 1,
    'B2-T64-D72-K3-causal-b2-s0.01': 1, 'B2-T64-D256-K3-causal-b2-s0.01': 1, 'B2-T65-D72-K3-causal-b2-s0.01': 1, 'B2-T129-D72-K3-causal-b2-s0.01': 2,
    'B2-T129-D256-K3-causal-b2-s0.01': 7, 'B2-T70-D144-K31-same-b2-s0.01': 1, 'B2-T70-D256-K31-same-b2-s0.01': 2, 'B2-T70-D264-K31-same-b2-s0.01': 4,
    'B2-T70-D520-K31-same-b2-s0.01': 1, 'B2-T70-D1032-K31-same-b2-s0.01': 9, 'B2-T70-D2048-K31-same-b2-s0.01': 34, 'B2-T70-D8-K7-causal-b2-s0.01': 1,
    'B2-T70-D264-K7-causal-b2-s0.01': 1, 'B2-T70-D520-K7-causal-b2-s0.01': 6, 'B2-T70-D1032-K7-causal-b2-s0.01': 24,
    'B2-T70-D2048-K7-causal-b2-s0.01': 224, 'B2-T70-D72-K15-same-b2-s0.01': 1, 'B2-T70-D72-K15-same-b2-s0': 1
}
# worst values measured on the MI355X over each path's cases: the stage figures relative to A (over 1/2 ulp for bf16 outputs; dy2 and the
# streamed bf16 z over the elements inside the tight bound - where flips of the unreturned dc / c occur that figure is close to the bound
# by construction, the share over it is the one to read), the shares, the smallest |pre-activation| of the kernels' own state
GPU_MEASURED = {
    "pair f32": {"c": 4.28e-07, "mean": 7.77e-08, "rstd": 1.42e-07, "z": 2.15e-07, "dy2": 2.87e-07, "dgamma": 1.46e-07, "dbeta": 1.09e-07,
                 "dconv_b": 1.55e-07, "db2": 1.17e-07, "dconv_w": 1.45e-07, "min_abs_y": 1.01e-05},
    "pair bf16": {"c": 7.46e-08, "mean": 3.46e-08, "rstd": 1.44e-07, "z": 5.55e-08, "dy2": 6.73e-07, "dgamma": 1.51e-07, "dbeta": 1.09e-07,
                  "dconv_b": 3.26e-05, "db2": 1.55e-05, "dconv_w": 1.34e-04, "c_flips": 8.93e-04, "z_flips": 4.63e-04, "dy2_flips": 6.94e-04,
                  "dy2_over": 6.94e-04, "min_abs_y": 1.04e-05},
    "fused bf16": {"c": 1.18e-07, "mean": 1.13e-08, "rstd": 1.42e-07, "z": 5.55e-08, "dy2": 5.90e-07, "dgamma": 1.59e-07, "dbeta": 1.27e-07,
                   "dconv_b": 1.52e-04, "db2": 6.67e-05, "dconv_w": 4.69e-04, "c_flips": 2.14e-04, "z_flips": 6.51e-04, "dy2_flips": 1.95e-03,
                   "dy2_over": 1.56e-04, "min_abs_y": 1.16e-05},
    "stream f32": {"stream_z": 1.11e-07, "hist": 3.73e-07},
    "stream bf16": {"stream_z": 2.93e-07, "hist": 3.73e-07, "z_over": 7.81e-05},
    # ops level, worst per-row relative L2 over the two cases of each path
    "ops pair f32": {"z": 2.23e-07, "dy2": 2.34e-07, "dgamma": 3.42e-06, "dbeta": 1.00e-06, "dconv_b": 2.10e-06, "db2": 2.91e-06, "dconv_w": 2.08e-07,
                     "dconv_w/tap": 1.91e-07},
    "ops pair bf16": {"z": 2.57e-06, "dy2": 5.44e-06, "dgamma": 2.02e-05, "dbeta": 1.32e-06, "dconv_b": 2.42e-05, "db2": 4.36e-05, "dconv_w": 3.91e-06,
                      "dconv_w/tap": 1.96e-06},
    "ops fused bf16": {"z": 7.84e-04, "dy2": 3.56e-04, "dgamma": 9.59e-04, "dbeta": 2.11e-06, "dconv_b": 4.04e-03, "db2": 1.90e-04, "dconv_w": 2.86e-04,
                       "dconv_w/tap": 5.48e-05},
}
OPS_DRAWS = 8               # the ops-level bounds take the emulation's worst row over this many draws of each shape


def _emu_y_error(inp, io, e):
    """|y computed in fp32 from the emulation's own c, mean, rstd - the float64 y of the emulation's c|, over all and over |y| < KINK_NEAR"""
    _, _, y64, _ = ln_fwd(e["c"].to(F64), inp["gamma"], inp["beta"], inp["slope"])
    err, near = (e["y"].to(F64) - y64).abs(), y64.abs() < KINK_NEAR
    return float(err.max()), (float(err[near].max()) if near.any() else 0.0)


def ops_inputs(path, B, T, D, K, causal, bias, draw_no=0):
    """the inputs of an ops-level case: the draw_no-th qualifying draw of the shape"""
    n = -1
    for _ in range(draw_no + 1):
        inp, n = _case(B, T, D, K, int(causal), int(bias), 0.01, n + 1)
    return dict(inp)


def ops_keys(ref):
    return [k for k in OPS_NAMES if k.split("/")[0] in ref]


def derive(verbose=True):
    """The CPU measurements behind TOL, KINK_MARGIN and SEEDS (a few minutes of CPU)."""
    inf = {k: float("inf") for k in ("c", "mean", "rstd", "z", "dy2", "stream_z", "hist") + PARAMS}
    worst = {"f32": {}, "bf16": {}}
    flips = {}
    yerr, ynear, seeds, done = 0.0, 0.0, {}, set()
    for _, path, B, T, D, K, causal, bias, slope in matrix():
        io = io_of(path)
        key = case_key(B, T, D, K, causal, bias, slope)
        if (key, io) in done:
            continue
        done.add((key, io))
        inp, n = case_inputs(B, T, D, K, causal, bias, slope, search=True)
        if n:
            seeds[key] = n
        e = emulate(inp, io)
        ya, yn = _emu_y_error(inp, io, e)
        yerr, ynear = max(yerr, ya), max(ynear, yn)
        par = {k: e[k] for k in PARAMS if bias or k != "db2"}
        st = check_conv(inp, io, e["c"], inf)
        st.update(check_ln(inp, io, e["c"], e["mean"], e["rstd"], e["z"], inf))
        st.update(check_bwd(inp, io, e["c"], e["mean"], e["rstd"], e["dy2"], par, inf, flip_cap=1.0))
        if io == "bf16":
            st["dy2"] = check_bwd(inp, io, e["c"], e["mean"], e["rstd"], e["dy2"], {}, inf, flip_cap=1.0, dc_own=e["dc"])["dy2"]
            if "dy2" in TOL["bf16"]:                          # with the bound in force: the share that needs the flip allowance
                d = {k: v[0] for k, v in TOL["bf16"].items()}
                st["dy2_over"] = check_bwd(inp, io, e["c"], e["mean"], e["rstd"], e["dy2"], {}, d, flip_cap=1.0)["dy2_over"]
        for k, v in st.items():
            if k.endswith("_flips") or k == "dy2_over":
                flips[k] = max(flips.get(k, 0.0), v)
            elif k != "min_abs_y":
                worst[io][k] = max(worst[io].get(k, 0.0), v)
        if verbose:
            print(f"{key:44s} {io:4s} seed+{n} " + " ".join(f"{k} {v:.2e}" for k, v in st.items()), flush=True)
    for B, T, D, K, causal, bias, slope in all_case_keys():
        n = case_inputs(B, T, D, K, causal, bias, slope, search=True)[1]
        if n:
            seeds[case_key(B, T, D, K, causal, bias, slope)] = n
    for K, D, chunks in STREAM:
        inp = stream_inputs(K, D)
        for io in ("f32", "bf16"):
            zs, hs, cs = emulate_stream(inp, io, chunks)
            st = check_stream(inp, io, chunks, zs, hs, inf, c_own=cs if io == "bf16" else None)
            worst[io]["stream_z"] = max(worst[io].get("stream_z", 0.0), st["z"])
            worst[io]["hist"] = max(worst[io].get("hist", 0.0), st["hist"])
            if io == "bf16" and "stream_z" in TOL["bf16"]:
                st["z_over"] = check_stream(inp, io, chunks, zs, hs, {k: v[0] for k, v in TOL["bf16"].items()})["z_over"]
                flips["stream_z_over"] = max(flips.get("stream_z_over", 0.0), st["z_over"])
            if verbose:
                print(f"stream K={K} D={D} chunks={chunks} {io} " + " ".join(f"{k} {v:.2e}" for k, v in st.items()), flush=True)
    ops = {}
    for path, B, T, D, K, causal in OPS:
        io = io_of(path)
        for bias in (1, 0):
            for n in range(OPS_DRAWS):
                inp = ops_inputs(path, B, T, D, K, causal, bias, n)
                ref, emu, pure = model(inp, io), model(inp, io, F32, fast=True), model(inp, io, rounding=False)
                for k in ops_keys({kk: v for kk, v in ref.items() if bias or kk != "db2"}):
                    q = k.split("/")[0]
                    e0, p0 = ops.setdefault(path, {}).get(k, (0.0, float("inf")))
                    ops[path][k] = (max(e0, float(row_errors(k, emu[q], ref[q]).max())), min(p0, float(row_errors(k, ref[q], pure[q]).max())))
    if verbose:
        print(f"worst |y error| of the emulation {yerr:.3e}; where |y| < {KINK_NEAR}: {ynear:.3e} -> KINK_MARGIN = {64 * ynear:.3e}")
        for io in ("f32", "bf16"):
            print(f'    "{io}": {{' + ", ".join(f'"{k}": ({16 * v:.2e}, {v:.2e})' for k, v in worst[io].items()) + "},")
        print('    "emu_flips": {' + ", ".join(f'"{k}": {v:.2e}' for k, v in flips.items()) + "},")
        for path, d in ops.items():
            print(f'        "{path}": {{' + ", ".join(f'"{k}": ({4 * e:.2e}, {e:.2e}, {p:.2e})' for k, (e, p) in d.items()) + "},")
            for k, (e, p) in d.items():
                if not 4 * e < p / 4:
                    print(f"        # {path} {k}: bound {4 * e:.2e} NOT below a quarter of the model's distance to pure float64 {p:.2e}")
        print("SEEDS =", seeds)
    return worst, flips, (yerr, ynear), seeds, ops


if __name__ == "__main__":
    derive()
