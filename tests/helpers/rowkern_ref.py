"""Dispatch mirror, case matrix, float64 model, fp32 emulation, dropout-mask port and judge for the row kernels of csrc/elementwise.hip:
LayerNorm fwd / bwd (narrow and wide), add_layernorm, add_layernorm2, bias_act_dropout, dropout_add, dropout_add2, colsum. Test
infrastructure only, CPU only: tests/test_rowkern_paths_gpu.py applies it to every template instantiation through the C-ABI,
tests/test_rowkern_ref_cpu.py proves that it can fail. `python tests/helpers/rowkern_ref.py` prints the derivation of TOL and KINK_MARGIN.

THE OPERATIONS (from the kernels' comments and include/tsasr_hip.h)
    LN        y = act(gamma (x - mean) rstd + beta), act = LeakyReLU(slope) when slope >= 0
              dx = rstd (g - mean(g) - h mean(g h)) [+ dadd], g = gamma act'(y) dy, h = (x - mean) rstd; dgamma = sum_rows act' dy h, dbeta = sum_rows act' dy
    tail      s = res + alpha timemask(dropout_p(x + bias)); rows [B, Trows] flattened, timemask zeroes rows t >= valid_lens[b] of the x branch
    add_ln    y = LN(s); backward d_s = LN_bwd(dy) + dout = dres, dx = alpha timemask dropmask / (1 - p) d_s, dbias = sum_rows dx
    add_ln2   z = LN2(y), statistics of the STORED y; backward dy_total = LN2_bwd(dz) + dy rounded to the io type, then add_ln's backward
    bad       y = dropout_p(act(x + bias)); dx = dy keep / (1 - p) act'(y), dbias = sum_rows dx
    da2       out = dropout_p2(round_io(tail)); dres = round_io(dropout_p2'(dout)), dx = alpha timemask dropout_p'(dres)
    colsum    out[c] (+)= sum_rows x[r][c]

MODEL AND EMULATION. Every function below runs in a chosen dtype. float64 with the kernels' rounding points (bf16 inputs; s rounded to the io
type before the statistics; y rounded before the second LayerNorm's statistics; dy_total rounded to the io type; outputs rounded to the io
type) is the model; the same functions in float32 with fast=True (rsqrt, column sums per workgroup and then over the partial rows in the
kernels' 16-slice order) are the emulation that TOL is derived from. Beside each value the model returns its magnitude A, the sum of the
absolute values of its terms: every bound is relative to A, not to a possibly cancelled result.

STAGE CHECKS judge a kernel from its OWN upstream state (mean / rstd from its stored s or x, y from that row with the float64 statistics, z
from its stored y, the gradients from its saved mean / rstd), so that one bf16 flip upstream is not charged downstream. fp32 outputs:
|got - ref| <= delta A. bf16 outputs: the nearest bf16 of the reference, or within delta A + one bf16 ulp of it and of the reference; the
share of such non-nearest elements per case stays under TOL["flips"]. The bf16 add_layernorm2 backward rounds the unreturned dy_total: dres
and dx get a flip allowance for it (one ulp of dy_total through the first LayerNorm's backward) and the fp32 parameter gradients of the
first LayerNorm allow 1 + 1 % of a column's rows to hold one such flip (_param).

THE MASK. keep_mask() ports drop_key / drop_hash / drop_thr16 / drop_scale16 of csrc/common.h and the pairing of two elements per hash word
(element i takes the low half of word i >> 1 when i is even, the high half when odd). It has no CPU ground truth but the header's text; the
GPU test confirms it first against tsasr_bias_act_dropout_fwd of all ones.

THE KINK. LN backward multiplies dy by slope where h gamma + beta <= 0. clear_kink() moves every x whose float64 pre-activation lies within
KINK_MARGIN of 0 by whole bf16 ulps (x holds bf16 values on both io types) until none does; no element is excluded from any comparison."""
import functools
import math

import numpy as np
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
IOS = ("bf16", "f32")
VEC = {"bf16": 8, "f32": 4}
TNAME = {"bf16": "bf16", "f32": "float"}
REJECTED = "rejected"
EPS = 1e-5
LDS_LIMIT = 160 * 1024          # per workgroup on gfx950; launches above 64 KB need the kernel's dynamic-LDS limit raised first


class Mismatch(AssertionError):
    def __init__(self, msg, stage=None, name=None, first=None):
        super().__init__(msg)
        self.stage, self.name, self.first = stage, name, first


# ------------------------------------------------------------------------------------------------------------------ the dispatch mirror
def cdiv(a, b):
    return -(-a // b)


def align256(n):
    return cdiv(n, 256) * 256


def rows_per_wg(M, min_rows=16):
    """pick_rows_per_wg: about 1024 workgroups, at least min_rows rows each"""
    return max(cdiv(M, 1024), min_rows)


def ln_is_wide(io, D):
    return D > 4 * 64 * VEC[io]


def ln_bwd_rows_per_wg(io, M, D):
    """layernorm_bwd_impl: the wide kernel walks max(rpw, ceil(M / 512)) rows per workgroup"""
    r = rows_per_wg(M)
    return max(r, cdiv(M, 512)) if ln_is_wide(io, D) else r


def _ln_path(kind, io, D, dadd=False):
    n, t = VEC[io], TNAME[io]
    pw, pg = 64 * n, 256 * n
    if D <= 0 or D % 8 or (dadd and D > 4 * pw):
        return REJECTED
    for lim, tpr, it in ((pw // 2, 32, 1), (pw, 64, 1), (2 * pw, 64, 2), (4 * pw, 64, 4)):
        if D <= lim:
            return f"layernorm_{kind}_kernel<{t},{tpr},{it}>"
    for it in (2, 3, 4, 6, 8):
        if D <= it * pg:
            return f"layernorm_{kind}_wide_kernel<{t},{it}>"
    return REJECTED


def _aln_path(name, io, D, limit):
    t = TNAME[io]
    if D <= 0 or D % 8 or D > limit:
        return REJECTED
    if io == "bf16":
        if D <= 256:
            return f"{name}_kernel<{t},1,true>"
        it = 1 if D <= 512 else 2 if D <= 1024 else 4
    else:
        it = 1 if D <= 256 else 2 if D <= 512 else 4 if D <= 1024 else 8
    return f"{name}_kernel<{t},{it},false>"


def slot_layout(io, N):
    """the (tpr, slots) thread layout of colsum_rows / bias_act_dropout_bwd / dropout_add_bwd: tpr column chunks x slots row slots"""
    chunks = N // VEC[io]
    tpr = min(chunks, 256)
    return tpr, 256 // tpr


def slot_lds(io, N, part=True):
    tpr, slots = slot_layout(io, N)
    return slots * N * 4 if (part and slots > 1) else 0


def expected_path(entry, io, D):
    """The kernel template and parameters that `entry` launches for rows of D elements of `io`, or REJECTED."""
    if entry == "layernorm_fwd":
        return _ln_path("fwd", io, D)
    if entry == "layernorm_bwd":
        return _ln_path("bwd", io, D)
    if entry == "layernorm_bwd_add":
        return _ln_path("bwd", io, D, dadd=True)
    if entry in ("add_layernorm_fwd", "add_layernorm_bwd"):
        return _aln_path(entry, io, D, 2048)
    if entry in ("add_layernorm2_fwd", "add_layernorm2_bwd"):
        return _aln_path(entry, io, D, 1024)
    if entry == "colsum":
        if D <= 0 or D % 8 or D > 2048:
            return REJECTED
        tpr, slots = slot_layout(io, D)
        return f"colsum_rows_kernel<{TNAME[io]}> tpr={tpr} slots={slots} lds={slots * D * 4}"
    if entry in ("bias_act_dropout_bwd", "dropout_add_bwd"):
        if D <= 0 or D % 8:
            return REJECTED
        tpr, slots = slot_layout(io, D)
        return f"{entry}_kernel<{TNAME[io]}> tpr={tpr} slots={slots} lds={slot_lds(io, D)}"
    if entry in ("bias_act_dropout_fwd", "dropout_add_fwd"):
        return REJECTED if (D <= 0 or D % 8) else f"{entry}_kernel<{TNAME[io]}>"
    raise KeyError(entry)


# every instantiation the dispatch can reach, per entry point and io type: matrix() must launch each (test_rowkern_ref_cpu.py)
def _inst(kind):
    return {io: [f"layernorm_{kind}_kernel<{TNAME[io]},{a},{b}>" for a, b in ((32, 1), (64, 1), (64, 2), (64, 4))]
            + [f"layernorm_{kind}_wide_kernel<{TNAME[io]},{i}>" for i in (2, 3, 4, 6, 8)] for io in IOS}


def _inst_aln(name, two):
    return {"bf16": [f"{name}_kernel<bf16,1,true>"] + [f"{name}_kernel<bf16,{i},false>" for i in ((1, 2) if two else (1, 2, 4))],
            "f32": [f"{name}_kernel<float,{i},false>" for i in ((1, 2, 4) if two else (1, 2, 4, 8))]}


INSTANTIATIONS = {
    "layernorm_fwd": _inst("fwd"), "layernorm_bwd": _inst("bwd"),
    "layernorm_bwd_add": {io: v[:4] for io, v in _inst("bwd").items()},
    "add_layernorm_fwd": _inst_aln("add_layernorm_fwd", False), "add_layernorm_bwd": _inst_aln("add_layernorm_bwd", False),
    "add_layernorm2_fwd": _inst_aln("add_layernorm2_fwd", True), "add_layernorm2_bwd": _inst_aln("add_layernorm2_bwd", True),
}
PART_K = {"ln": 2, "aln": 3, "aln2": 5}      # partial-slab rows per workgroup: k x D floats


def workspace_bytes(fam, M, D):
    """tsasr_{layernorm,add_layernorm,add_layernorm2}_bwd_workspace_bytes / tsasr_colpart_workspace_bytes (k = 1) / tsasr_colsum_workspace_bytes"""
    if fam == "colsum":
        return align256(cdiv(M, max(64, cdiv(M, 1024))) * D * 4)
    k = PART_K.get(fam, 1)
    return align256(cdiv(M, rows_per_wg(M)) * k * D * 4)


def n_workgroups(fam, io, M, D):
    if fam == "colsum":
        return cdiv(M, max(64, cdiv(M, 1024)))
    return cdiv(M, ln_bwd_rows_per_wg(io, M, D) if fam == "ln" else rows_per_wg(M))


def lds_bytes(entry, io, D):
    """static + dynamic LDS of the launch `entry` makes for rows of D (the LDS table of the header)"""
    path = expected_path(entry, io, D)
    if path == REJECTED:
        return 0
    if entry in ("layernorm_fwd",):
        return 64 if "wide" in path else 16
    if entry in ("layernorm_bwd", "layernorm_bwd_add"):
        if "wide" in path:
            return 64
        tpr = int(path.split(",")[1])
        return 16 + (256 // tpr) * 2 * D * 4
    if entry == "add_layernorm_bwd":
        return (24 if "true" in path else 12) * D * 4
    if entry == "add_layernorm2_bwd":
        return (8 if "true" in path else 4) * 5 * D * 4
    if entry == "colsum":
        return slot_layout(io, D)[1] * D * 4
    if entry in ("bias_act_dropout_bwd", "dropout_add_bwd"):
        return slot_lds(io, D)
    return 0


def lanes_of(path):
    """(lanes per row, elements per lane access) of a LN-family path"""
    n = 8 if "bf16" in path else 4
    if "wide" in path:
        return 256, n
    if path.startswith("layernorm_"):
        return int(path.split(",")[1]), n
    return (32 if "true" in path else 64), n


def where(path, row, col):
    lpr, n = lanes_of(path)
    chunk = col // n
    return f"(row={row}, column={col}, lane={chunk % lpr}, iteration={chunk // lpr})"


# ------------------------------------------------------------------------------------------------------------------ the dropout mask
M64, M32 = (1 << 64) - 1, np.uint64(0xFFFFFFFF)


def drop_key(seed):
    z = (seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z & 0xFFFFFFFF, z >> 32


def drop_hash(ctr, key):
    """ctr: uint64 array of hash-word counters -> uint64 array holding the 32-bit words"""
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    x = ((ctr & M32) + k0) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x + (k1 ^ (ctr >> np.uint64(32)))) & M32
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def drop_thr16(p):
    return min(65535, int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))) if p > 0 else 0


def drop_scale16(thr):
    """65536 / (65536 - thr) in fp32, as a Python float"""
    return float(np.float32(65536.0) / np.float32(65536 - thr))


def keep_mask(n, seed, p, seed_dev=0, start=0):
    """keep bits of the elements start .. start + n - 1 (flattened row * D + column) -> bool tensor [n]; p = 0 keeps all"""
    if p <= 0:
        return torch.ones(n, dtype=torch.bool)
    idx = np.arange(start, start + n, dtype=np.uint64)
    h = drop_hash(idx >> np.uint64(1), drop_key((seed + seed_dev) & M64))
    u = np.where((idx & np.uint64(1)) == 1, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return torch.from_numpy(u >= np.uint64(drop_thr16(p)))


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def bf(x):
    return x.to(BF16).to(x.dtype)


def rnd(x, io):
    return x.to(BF16).to(x.dtype) if io == "bf16" else x.to(F32).to(x.dtype)


def store(x, io):
    return x.to(BF16 if io == "bf16" else F32)


def ulp_bf16(ref):
    r = ref.abs().to(F64)
    _, e = torch.frexp(r)
    return torch.where(r > 0, torch.ldexp(torch.ones_like(r), e - 8), torch.zeros_like(r))


def ambiguous(v, A, delta):
    """where the bf16 rounding of the float64 value v may go either way under an error of delta A: v lies that close to the midpoint of
    its two bf16 neighbours"""
    v = v.to(F64)
    return ((v - bf(v.to(F32)).to(F64)).abs() - ulp_bf16(v) / 2).abs() <= delta * A


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF16 else t.contiguous().view(torch.int32)


def colsum_like_kernels(terms, nwg, rpw, fast):
    """[M, D] per-row terms -> [D]. fast: one partial row per workgroup of rpw rows, then the partial rows in colsum_kernel's order (16
    slices, each summing its rows in sequence, the slices in sequence); otherwise the plain sum."""
    if not fast:
        return terms.sum(0)
    M, D = terms.shape
    pad = torch.zeros(nwg * rpw - M, D, dtype=terms.dtype)
    part = torch.cat([terms, pad]).view(nwg, rpw, D).sum(1)
    n16 = cdiv(nwg, 16) * 16
    part = torch.cat([part, torch.zeros(n16 - nwg, D, dtype=terms.dtype)]).view(n16 // 16, 16, D)
    sl = part.cumsum(0)[-1]
    return sl.cumsum(0)[-1]


def ln_stats(x, D, eps, fast=False):
    mu = x.sum(-1) / D
    q = ((x - mu[:, None]) ** 2).sum(-1) / D
    return mu, (torch.rsqrt(q + eps) if fast else 1.0 / torch.sqrt(q + eps))


def ln_apply(x, mu, rs, gamma, beta, slope):
    """-> pre-activation y, output z, A_z"""
    g, b = gamma.to(x.dtype), beta.to(x.dtype)
    y = (x - mu[:, None]) * rs[:, None] * g + b
    A = (x.abs() + x.abs().sum(-1, keepdim=True) / x.shape[-1]) * rs[:, None] * g.abs() + b.abs()      # the mean's own terms, not |mean|
    if slope >= 0:
        return y, torch.where(y > 0, y, y * slope), torch.where(y > 0, A, A * slope)
    return y, y, A


def ln_backward(dy, x, mu, rs, gamma, beta, slope, dadd=None):
    """-> dict(dx, tg (per-row dgamma terms), tb (dbeta terms), A_dx, y); beta None: no activation (add_layernorm)"""
    D = x.shape[-1]
    g, rs1 = gamma.to(x.dtype), rs[:, None]
    h = (x - mu[:, None]) * rs1
    y = h * g + beta.to(x.dtype) if beta is not None else None
    d = dy if (slope < 0 or beta is None) else torch.where(y <= 0, dy * slope, dy)
    gd = d * g
    m1, m2 = gd.sum(-1, keepdim=True) / D, (gd * h).sum(-1, keepdim=True) / D
    dx = rs1 * (gd - m1 - h * m2)
    A = rs1 * (gd.abs() + gd.abs().sum(-1, keepdim=True) / D + h.abs() * (gd * h).abs().sum(-1, keepdim=True) / D)
    if dadd is not None:
        dx, A = dx + dadd, A + dadd.abs()
    return {"dx": dx, "tg": d * h, "tb": d, "A_dx": A, "y": y, "h": h, "g": g}


def live_rows(M, vl):
    """vl: None or (B, [valid lens]) with Trows = M / B -> bool [M]"""
    if vl is None:
        return torch.ones(M, dtype=torch.bool)
    B, lens = vl
    T = M // B
    return (torch.arange(M) % T) < torch.tensor(lens)[torch.arange(M) // T]


def tail(x, bias, res, keep, ks, alpha, live, dt):
    """s = res + alpha timemask(dropout(x + bias)), unrounded, and A_s"""
    t = x.to(dt)
    A = t.abs()
    if bias is not None:
        t, A = t + bias.to(dt), A + bias.to(dt).abs()
    if keep is not None:
        zero = torch.zeros((), dtype=dt)
        t, A = torch.where(keep, t * ks, zero), torch.where(keep, A * ks, zero)
    lv = live[:, None].to(dt)
    t, A = t * alpha * lv, A * abs(alpha) * lv
    if res is not None:
        t, A = t + res.to(dt), A + res.to(dt).abs()
    return t, A


def tail_grad(d, keep, ks, alpha, live):
    """dx = alpha timemask dropmask ks d (the kernels multiply by alpha first, then by ks)"""
    g = d * alpha * live[:, None].to(d.dtype)
    return g * ks * keep.to(d.dtype) if keep is not None else g


# ------------------------------------------------------------------------------------------------------------------ the cases
def _case(fam, io, M, D, **o):
    c = dict(fam=fam, io=io, M=M, D=D, slope=-1.0, dadd=0, bias=1, dout=1, dy=1, nulls=(), vl=0, p=0.1, alpha=0.5, seed=0x1234567, seed_dev=0,
             eps=EPS, eps2=1e-6, p2=0.0, acc=0)
    c.update(o)
    if fam == "ln":
        c.update(p=0.0, alpha=1.0)
    c["key"] = case_key(c)
    return c


def case_key(c):
    s = f"{c['fam']}-{c['io']}-M{c['M']}-D{c['D']}"
    if c["fam"] == "ln":
        return s + f"-s{c['slope']:g}" + ("-dadd" if c["dadd"] else "")
    if c["fam"] == "colsum":
        return s + f"-acc{c['acc']}"
    s += f"-p{c['p']:g}-a{c['alpha']:g}-{'b' if c['bias'] else 'nob'}-{'vl' if c['vl'] else 'novl'}-seed{c['seed']:x}+{c['seed_dev']:x}"
    if c["fam"] in ("aln", "aln2"):
        s += ("-dout" if c["dout"] else "-nodout") + ("" if c["fam"] == "aln" or c["dy"] else "-nody") + ("-null:" + ".".join(c["nulls"]) if c["nulls"] else "")
    if c["fam"] == "bad":
        s += f"-s{c['slope']:g}"
    if c["fam"] == "da2":
        s += f"-p2{c['p2']:g}"
    return s


LN_D = {"bf16": (144, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4104, 6152, 8200, 12296, 16384), "f32": (72, 128, 136, 256, 264, 512, 520, 1024, 1032,
        2048, 2056, 3080, 4104, 6152, 8192)}
LN_REJ = {"bf16": 16392, "f32": 8200}
ALN_D = {"bf16": (144, 256, 264, 512, 520, 1024, 1032, 2048), "f32": (72, 256, 264, 512, 520, 1024, 1032, 2048)}
ALN2_D = {"bf16": (144, 256, 264, 512, 520, 1024), "f32": (72, 256, 264, 512, 520, 1024)}
ALN_REJ, ALN2_REJ = 2056, 1032
NARROW = {"bf16": 144, "f32": 72}            # the narrow D on which rows and options are crossed
BIG_SEED, DEV_SEED = 0x1_2345_6789_ABCD, 0xFFFF_FFFF_0000_1234     # host seed above 2^32; host + device seed wraps past 2^64
VL_B = 3


def valid_lens(M):
    T = M // VL_B
    return (VL_B, [T, max(1, T // 2), 1])


@functools.lru_cache(maxsize=None)
def matrix():
    m = []
    for io in IOS:
        # ---- LayerNorm: every instantiation (M = 37: workgroups of 16, 16, 5), slope sampled on both kinds
        for i, D in enumerate(LN_D[io]):
            m.append(_case("ln", io, 37, D, slope=0.01 if i % 2 == 0 else -1.0))
        m.append(_case("ln", io, 37, LN_D[io][9], slope=-1.0))                         # a wide path without activation ...
        m.append(_case("ln", io, 37, LN_D[io][10], slope=0.01))                        # ... and its neighbour with
        for D in LN_D[io][:8:2] + (LN_D[io][7],):                                       # the pass-through sum on each one-wave kernel, and at its limit
            m.append(_case("ln", io, 37, D, slope=0.01, dadd=1))
        for M in (1, 7, 37):                                                            # rows x slope x dadd on the narrow D
            for slope in (-1.0, 0.01):
                for dadd in (0, 1):
                    m.append(_case("ln", io, M, NARROW[io], slope=slope, dadd=dadd))
        m.append(_case("ln", io, 16401, 64, slope=0.01))                                # rows_per_wg = 17, the half-wave kernel on both io
        m.append(_case("ln", io, 16401, 64, slope=-1.0, dadd=1))
        # ---- add_layernorm / add_layernorm2: every instantiation, options sampled; rows and options crossed on the narrow D
        for fam, Ds in (("aln", ALN_D[io]), ("aln2", ALN2_D[io])):
            for i, D in enumerate(Ds):
                m.append(_case(fam, io, 37, D, bias=i % 2, dout=(i + 1) % 2 or fam == "aln2", dy=i % 2, p=0.1 if i % 3 else 0.0, alpha=(1.0, 0.5)[i % 2],
                               seed=BIG_SEED if i % 2 else 0x1234567))
            for M in (1, 7, 37):
                m.append(_case(fam, io, M, NARROW[io]))
            D = NARROW[io]
            m.append(_case(fam, io, 39, D, vl=1, seed=BIG_SEED, seed_dev=DEV_SEED))      # time mask, B = 3, T = 13, lens 13, 6, 1
            m.append(_case(fam, io, 39, D, vl=1, p=0.0, alpha=1.0, bias=0, dout=0))
            m.append(_case(fam, io, 37, D, alpha=1.0, bias=0, dout=0, dy=0, nulls=("dgamma", "dbias")))
            m.append(_case(fam, io, 37, D, p=0.0, seed_dev=DEV_SEED, nulls=("dbeta",)))
            m.append(_case(fam, io, 37, 256, vl=0, seed=BIG_SEED, seed_dev=DEV_SEED, nulls=("dgamma2",) if fam == "aln2" else ()))
            m.append(_case(fam, io, 16401, 64, vl=1, seed=BIG_SEED))                     # rows_per_wg = 17, last workgroup of 13 rows
        # ---- element-wise kernels with a bias-gradient slab
        for fam in ("bad", "da", "da2"):
            for i, N in enumerate((8, 64, 2048, 2056)):
                for M in (1, 37):
                    m.append(_case(fam, io, M, N, slope=0.01 if (i + M) % 2 else -1.0, bias=(i + M) % 2, p=0.1, alpha=(1.0, 0.5)[i % 2],
                                   seed=BIG_SEED if i % 2 else 0x1234567, seed_dev=DEV_SEED if i == 2 else 0, p2=0.2 if fam == "da2" else 0.0))
            m.append(_case(fam, io, 16401, 64, slope=0.01, vl=0 if fam == "bad" else 1, p2=0.2 if fam == "da2" else 0.0))
            m.append(_case(fam, io, 39, 64, slope=-1.0, p=0.0, vl=0 if fam == "bad" else 1, bias=0, p2=0.0, nulls=("dbias",)))
        for M, N in ((5, 2048), (777, 256), (65, 8), (70001, 128)):
            for acc in (0, 1):
                m.append(_case("colsum", io, M, N, acc=acc))
    seen = set()
    return tuple(c for c in m if not (c["key"] in seen or seen.add(c["key"])))


def case_paths(c):
    """{entry: expected path} of the launches a case makes"""
    fam, io, D = c["fam"], c["io"], c["D"]
    if fam == "ln":
        return {"layernorm_fwd": expected_path("layernorm_fwd", io, D),
                ("layernorm_bwd_add" if c["dadd"] else "layernorm_bwd"): expected_path("layernorm_bwd_add" if c["dadd"] else "layernorm_bwd", io, D)}
    if fam in ("aln", "aln2"):
        n = "add_layernorm" if fam == "aln" else "add_layernorm2"
        return {n + "_fwd": expected_path(n + "_fwd", io, D), n + "_bwd": expected_path(n + "_bwd", io, D)}
    if fam == "colsum":
        return {"colsum": expected_path("colsum", io, D)}
    n = "bias_act_dropout" if fam == "bad" else "dropout_add"
    return {n + "_fwd": expected_path(n + "_fwd", io, D), n + "_bwd": expected_path(n + "_bwd", io, D)}


def _seed_of(key):
    h = 1469598103934665603
    for ch in key.encode():
        h = ((h ^ ch) * 1099511628211) & M64
    return h % (2 ** 31)


def pre_activation(x, gamma, beta, eps):
    x = x.to(F64)
    mu, rs = ln_stats(x, x.shape[-1], eps)
    return ln_apply(x, mu, rs, gamma.to(F64), beta.to(F64), -1.0)[0]


def clear_kink(x, gamma, beta, eps, margin=None):
    """move every x whose float64 pre-activation lies within the margin of 0 by whole bf16 ulps until none does -> (x, elements moved)"""
    margin = KINK_MARGIN if margin is None else margin
    moved = 0
    for k in range(1, 64):
        near = pre_activation(x, gamma, beta, eps).abs() < margin
        if not near.any():
            return x, moved
        moved += int(near.sum())
        step = ulp_bf16(x).to(F32).clamp_min(2.0 ** -9) * k
        x = torch.where(near, bf(x + step * torch.sign(gamma)[None, :]), x)
    raise AssertionError("clear_kink did not converge")


@functools.lru_cache(maxsize=None)
def _inputs(key, attempt):
    c = {k["key"]: k for k in matrix()}[key]
    g = torch.Generator().manual_seed(_seed_of(key) + 7919 * attempt)
    M, D, fam = c["M"], c["D"], c["fam"]
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    i = {"x": bf(rn(M, D))}
    if fam == "colsum":
        i["out0"] = rn(D)
        return i
    i["bias"] = rn(D) * 0.1 if c["bias"] else None
    if fam in ("ln", "aln", "aln2"):
        i["gamma"] = (rn(D) * 0.1 + 1) * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)
        i["beta"] = rn(D) * 0.1
        i["dy"] = bf(rn(M, D))
    if fam == "ln":
        i["x"] = bf(i["x"] * 1.5 + 0.3)
        i["dadd"] = bf(rn(M, D)) if c["dadd"] else None
        if c["slope"] >= 0:
            i["x"], i["moved"] = clear_kink(i["x"], i["gamma"], i["beta"], c["eps"])
    else:
        i["res"] = bf(rn(M, D))
    if fam in ("aln", "aln2"):
        i["dout"] = bf(rn(M, D)) if c["dout"] else None
    if fam == "aln2":
        i["gamma2"] = (rn(D) * 0.1 + 1) * (torch.randint(0, 2, (D,), generator=g) * 2 - 1)
        i["beta2"] = rn(D) * 0.1
        i["dz"] = bf(rn(M, D))
        if not c["dy"]:
            i["dy"] = None
    if fam in ("bad", "da", "da2"):
        i["dy"] = bf(rn(M, D))
    if fam != "ln":
        i["keep"] = keep_mask(M * D, c["seed"], c["p"], c["seed_dev"]).view(M, D) if c["p"] > 0 else None
        i["ks"] = drop_scale16(drop_thr16(c["p"]))
        i["live"] = live_rows(M, valid_lens(M) if c["vl"] else None)
    if fam == "da2":
        i["keep2"] = keep_mask(M * D, (c["seed"] + 77) & M64, c["p2"], c["seed_dev"]).view(M, D) if c["p2"] > 0 else None
        i["ks2"] = drop_scale16(drop_thr16(c["p2"]))
    return i


def case_inputs(c, search=False):
    """-> (inputs, attempt). The draw moves to the next attempt until the bf16 emulation's share of non-nearest outputs is at most a quarter
    of the cap; SEEDS records where each case ends (absent: 0)."""
    n = 0 if search else SEEDS.get(c["key"], 0)
    while True:
        inp = _inputs(c["key"], n)
        if c["io"] != "bf16" or c["fam"] == "colsum" or max(emu_flip_shares(c, inp).values(), default=0.0) <= TOL["flips"] / 4:
            return dict(inp), n
        n += 1


# ------------------------------------------------------------------------------------------------------------------ the free-running chains
def model(c, inp, dt=F64, fast=False, plant=None, rounding=True):
    """Forward and backward of a case, run free in `dt` with the kernels' rounding points (rounding=False: none, the pure operation, which
    must equal float64 autograd). fast: the fp32 emulation's associations. plant: a defect for the CPU test ("mean_unrounded": statistics of
    the unrounded s)."""
    fam, io, M, D = c["fam"], c["io"], c["M"], c["D"]
    r = (lambda v: rnd(v, io)) if rounding else (lambda v: v)  # noqa: E731
    x = inp["x"].to(dt)
    o = {}
    if fam == "colsum":
        rpw = max(64, cdiv(M, 1024))
        o["out"] = colsum_like_kernels(x, cdiv(M, rpw), rpw, fast) + (inp["out0"].to(dt) if c["acc"] else 0)
        return o
    if fam == "ln":
        rpw = ln_bwd_rows_per_wg(io, M, D)
        nwg = cdiv(M, rpw)
        mu, rs = ln_stats(x, D, c["eps"], fast)
        y, z, _ = ln_apply(x, mu, rs, inp["gamma"], inp["beta"], c["slope"])
        b = ln_backward(inp["dy"].to(dt), x, mu, rs, inp["gamma"], inp["beta"], c["slope"], None if inp["dadd"] is None else inp["dadd"].to(dt))
        o.update(mean=mu, rstd=rs, y=r(z), pre=y, dx=r(b["dx"]), dgamma=colsum_like_kernels(b["tg"], nwg, rpw, fast),
                 dbeta=colsum_like_kernels(b["tb"], nwg, rpw, fast))
        return o
    rpw = rows_per_wg(M)
    nwg = cdiv(M, rpw)
    if fam == "bad":
        t, _ = tail(x, inp["bias"], None, None, 1.0, 1.0, torch.ones(M, dtype=torch.bool), dt)
        if c["slope"] >= 0:
            t = torch.where(t > 0, t, t * c["slope"])
        if inp["keep"] is not None:
            t = torch.where(inp["keep"], t * inp["ks"], torch.zeros((), dtype=dt))
        o["y"] = r(t)
        g = inp["dy"].to(dt)
        if inp["keep"] is not None:
            g = torch.where(inp["keep"], g * inp["ks"], torch.zeros((), dtype=dt))
        if c["slope"] >= 0:
            g = torch.where(o["y"] < 0, g * c["slope"], g)
        o.update(dx=r(g), dbias=colsum_like_kernels(g, nwg, rpw, fast))
        return o
    s, _ = tail(x, inp["bias"], inp["res"], inp["keep"], inp["ks"], c["alpha"], inp["live"], dt)
    if fam in ("da", "da2"):
        d = inp["dy"].to(dt)
        if fam == "da2" and inp["keep2"] is not None:
            zero = torch.zeros((), dtype=dt)
            s = torch.where(inp["keep2"], r(s) * inp["ks2"], zero)
            d = r(torch.where(inp["keep2"], d * inp["ks2"], zero))
            o["dres"] = d
        g = tail_grad(d, inp["keep"], inp["ks"], c["alpha"], inp["live"])
        o.update(out=r(s), dx=r(g), dbias=colsum_like_kernels(g, nwg, rpw, fast))
        return o
    s_st = s if plant == "mean_unrounded" else r(s)
    mu, rs = ln_stats(s_st, D, c["eps"], fast)
    s = r(s)
    y = ln_apply(s, mu, rs, inp["gamma"], inp["beta"], -1.0)[0]
    o.update(s=s, mean=mu, rstd=rs, y=r(y))
    dy = None if inp["dy"] is None else inp["dy"].to(dt)
    if fam == "aln2":
        yr = o["y"]
        mu2, rs2 = ln_stats(yr, D, c["eps2"], fast)
        o.update(mean2=mu2, rstd2=rs2, z=r(ln_apply(yr, mu2, rs2, inp["gamma2"], inp["beta2"], -1.0)[0]))
        b2 = ln_backward(inp["dz"].to(dt), yr, mu2, rs2, inp["gamma2"], None, -1.0, dy)
        dy = r(b2["dx"])
        o.update(dy_total=dy, dyt_raw=b2["dx"], dgamma2=colsum_like_kernels(b2["tg"], nwg, rpw, fast), dbeta2=colsum_like_kernels(b2["tb"], nwg, rpw, fast))
    b = ln_backward(dy, s, mu, rs, inp["gamma"], None, -1.0, None if inp["dout"] is None else inp["dout"].to(dt))
    g = tail_grad(b["dx"], inp["keep"], inp["ks"], c["alpha"], inp["live"])
    o.update(dres=r(b["dx"]), dx=r(g), dgamma=colsum_like_kernels(b["tg"], nwg, rpw, fast), dbeta=colsum_like_kernels(b["tb"], nwg, rpw, fast),
             dbias=colsum_like_kernels(g, nwg, rpw, fast))
    return o


IO_OUTPUTS = ("y", "z", "s", "dx", "dres", "out")


def emulate(c, inp, **kw):
    """the fp32 emulation in the kernels' storage types"""
    e = model(c, inp, F32, fast=True, **kw)
    if c["fam"] == "colsum":
        return e
    return {k: (store(v, c["io"]) if k in IO_OUTPUTS else v) for k, v in e.items()}


# ------------------------------------------------------------------------------------------------------------------ the judge
def _fail(what, stage, name, bad, diff, bound, got, ref, describe):
    idx = torch.nonzero(bad)
    first = tuple(int(v) for v in idx[0])
    excess = torch.where(bad, diff - bound, torch.full_like(diff, -1.0))
    worst = tuple(int(v) for v in torch.nonzero(excess == excess.max())[0])

    def show(ix):
        return f"{describe(ix)}: got {float(got[ix])!r}, want {float(ref[ix])!r}, |diff| {float(diff[ix]):.3e} > bound {float(bound[ix]):.3e}"
    raise Mismatch(f"{what} | stage {stage} {name}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {show(first)}; worst at {show(worst)}",
                   stage, name, first)


_CAP = None            # check_case(flip_cap=...) lifts the cap while the emulation itself is being measured


def judge(what, stage, name, got, ref, A, delta, io_out, describe, allow=None, flip_cap=None):
    """-> (worst |diff| / A (bf16 outputs: of the elements that are not the nearest bf16, over one ulp), share of non-nearest elements).
    io_out: "f32" (an fp32 tensor: |got - ref| <= delta A) or "bf16" (nearest, or one ulp from it and within delta A + one ulp)."""
    g, ref, A = got.to(F64), ref.to(F64), A.to(F64)
    diff = (g - ref).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    extra = torch.zeros_like(ref) if allow is None else allow.to(F64)
    if io_out != "bf16":
        bound = delta * A + extra
        bad = diff > bound
        if bad.any():
            _fail(what, stage, name, bad, diff, bound, g, ref, describe)
        live = A > 0
        return (float(((diff - extra).clamp_min(0)[live] / A[live]).max()) if live.any() else 0.0), 0.0
    near = ref.to(F32).to(BF16)
    non = (got.to(BF16) != near) | torch.isnan(g)
    u = torch.maximum(ulp_bf16(ref), ulp_bf16(near))
    bound = delta * A + u + extra
    bad = non & (((g - near.to(F64)).abs() > bound) | (diff > bound))       # a cancelled result may lie delta A, many of ITS ulps, away
    bad = bad | torch.isnan(g)
    if bad.any():
        _fail(what, stage, name, bad, diff, bound, g, ref, describe)
    share = float(non.double().mean())
    cap = flip_cap if flip_cap is not None else (TOL["flips"] if _CAP is None else _CAP)
    if share > cap:
        first = tuple(int(v) for v in torch.nonzero(non)[0])
        raise Mismatch(f"{what} | stage {stage} {name}: {share:.3%} of the elements are not the nearest bf16 of the reference (cap {cap:.1%}); first at "
                       f"{describe(first)}: got {float(g[first])!r}, want {float(ref[first])!r}", stage, name, first)
    live = non & (A > 0)
    return (float(((diff - u - extra).clamp_min(0)[live] / A[live]).max()) if live.any() else 0.0), share


def _d2(path):
    return lambda ix: where(path, ix[0], ix[1])


def _d1(ix):
    return f"(row={ix[0]})"


def _dcol(ix):
    return f"(column={ix[0]})"


def exact(what, stage, name, got, want, describe):
    """bit for bit (+0 and -0 alike)"""
    bad = (got.to(F64) != want.to(F64)) | torch.isnan(got.to(F64))
    if bad.any():
        first = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise Mismatch(f"{what} | stage {stage} {name}: {int(bad.sum())} of {bad.numel()} elements differ from the exact value; first at {describe(first)}: "
                       f"got {float(got[first])!r}, want {float(want[first])!r}", stage, name, first)


def check_ln_fwd(c, inp, k, delta, what="", path=None, x_key="x", pre="", gamma="gamma", beta="beta", eps=None, slope=None):
    """mean, rstd against the float64 statistics of the row the kernel read (its own stored s / y when there is one), the output against the
    float64 LayerNorm of that row. k: the kernel's outputs. -> statistics"""
    io, D = c["io"], c["D"]
    path = path or "layernorm_fwd_kernel<%s,64,1>" % TNAME[io]
    x = (k[x_key] if x_key in k else inp[x_key]).to(F64)
    eps = c["eps"] if eps is None else eps
    slope = c["slope"] if slope is None else slope
    mu, rs = ln_stats(x, D, eps)
    y, z, A = ln_apply(x, mu, rs, inp[gamma].to(F64), inp[beta].to(F64), slope)
    mname, rname, oname = ("mean2", "rstd2", "z") if pre else ("mean", "rstd", "y")
    st = {}
    st[pre + "mean"], _ = judge(what, "stats", mname, k[mname], mu, x.abs().sum(-1) / D, delta[pre + "mean"], "f32", _d1)
    st[pre + "rstd"], _ = judge(what, "stats", rname, k[rname], rs, rs, delta[pre + "rstd"], "f32", _d1)
    st[pre + "y"], st[pre + "y_flips"] = judge(what, "normalise", oname, k[oname], z, A, delta[pre + "y"], io, _d2(path))
    if slope >= 0:
        st["min_abs_pre"] = float(y.abs().min())
    return st


def check_tail_fwd(c, inp, s_k, delta, what="", path=None, name="s"):
    """the stored s (or out of dropout_add) against the float64 tail; dropped / time-masked elements must be res exactly"""
    io = c["io"]
    path = path or "add_layernorm_fwd_kernel<%s,1,false>" % TNAME[io]
    s, A = tail(inp["x"], inp["bias"], inp["res"], inp["keep"], inp["ks"], c["alpha"], inp["live"], F64)
    dead = ~inp["live"][:, None].expand_as(s) if inp["keep"] is None else (~inp["keep"] | ~inp["live"][:, None])
    if dead.any():
        exact(what, "tail", name + " where the x branch is dropped or masked", torch.where(dead, s_k.to(F64), 0.0), torch.where(dead, inp["res"].to(F64), 0.0),
              _d2(path))
    w, f = judge(what, "tail", name, s_k, s, A, delta["s"], io, _d2(path))
    return {"s": w, "s_flips": f}


def _param(what, st, name, got, terms, delta, key=None, flip_terms=None, A_terms=None):
    """a parameter gradient against the float64 column sum of the float64 per-row terms. flip_terms: what a one-ulp flip of an unreturned
    bf16 intermediate moves each term by, zero where its rounding is not ambiguous."""
    if got is None:
        return
    ref, A = terms.sum(0), (terms.abs() if A_terms is None else A_terms).sum(0)     # A_terms: the terms are themselves cancelled sums
    allow = None if flip_terms is None else flip_terms.sum(0)
    st[key or name], _ = judge(what, "columns", name, got, ref, A, delta[key or name], "f32", _dcol, allow)


def check_ln_bwd(c, inp, k, delta, what="", path=None):
    """dx, dgamma, dbeta of the LayerNorm backward from x and the kernel's saved mean / rstd"""
    io = c["io"]
    path = path or "layernorm_bwd_kernel<%s,64,1>" % TNAME[io]
    dadd = None if inp.get("dadd") is None else inp["dadd"].to(F64)
    b = ln_backward(inp["dy"].to(F64), inp["x"].to(F64), k["mean"].to(F64), k["rstd"].to(F64), inp["gamma"].to(F64), inp["beta"].to(F64), c["slope"], dadd)
    st = {}
    st["dx"], st["dx_flips"] = judge(what, "rows", "dx", k["dx"], b["dx"], b["A_dx"], delta["dx"], io, _d2(path))
    _param(what, st, "dgamma", k.get("dgamma"), b["tg"], delta)
    _param(what, st, "dbeta", k.get("dbeta"), b["tb"], delta)
    if c["slope"] >= 0:
        st["min_abs_pre"] = float(b["y"].abs().min())
    return st


def check_aln_bwd(c, inp, k, delta, what="", path=None):
    """dres, dx and the parameter gradients of add_layernorm(2)_bwd from the kernel's own s, y and saved statistics"""
    io, fam, D = c["io"], c["fam"], c["D"]
    path = path or "add_layernorm_bwd_kernel<%s,1,false>" % TNAME[io]
    s = k["s"].to(F64)
    st, pre = {}, "aln2." if fam == "aln2" else ""
    dy = None if inp["dy"] is None else inp["dy"].to(F64)
    allow = None
    if fam == "aln2":
        b2 = ln_backward(inp["dz"].to(F64), k["y"].to(F64), k["mean2"].to(F64), k["rstd2"].to(F64), inp["gamma2"].to(F64), None, -1.0, dy)
        A2 = b2["A_dx"]
        _param(what, st, "dgamma2", k.get("dgamma2"), b2["tg"], delta)
        _param(what, st, "dbeta2", k.get("dbeta2"), b2["tb"], delta)
        if "dyt_raw" in k:                       # the emulation's own unrounded dy_total: the measurement behind delta["dyt"]
            st["dyt"], _ = judge(what, "rows", "dy_total before rounding", k["dyt_raw"], b2["dx"], b2["A_dx"], delta["dyt"], "f32", _d2(path))
        dy = rnd(b2["dx"], io)
        if io == "bf16":                         # one-ulp flips of the unreturned dy_total, where its rounding is ambiguous under delta["dyt"]
            ud = torch.where(ambiguous(b2["dx"], b2["A_dx"], delta["dyt"]), ulp_bf16(dy), torch.zeros_like(dy))
            u = ud * inp["gamma"].to(F64).abs()
    b = ln_backward(dy, s, k["mean"].to(F64), k["rstd"].to(F64), inp["gamma"].to(F64), None, -1.0, None if inp["dout"] is None else inp["dout"].to(F64))
    if fam == "aln2" and io == "bf16":
        h = b["h"].abs()
        allow = k["rstd"].to(F64)[:, None] * (u + (u.sum(-1, keepdim=True) + h * (u * h).sum(-1, keepdim=True)) / D)
    st[pre + "dres"], st["dres_flips"] = judge(what, "rows", "dres", k["dres"], b["dx"], b["A_dx"], delta[pre + "dres"], io, _d2(path), allow)
    g = tail_grad(b["dx"], inp["keep"], inp["ks"], c["alpha"], inp["live"])
    A_g = tail_grad(b["A_dx"], inp["keep"], inp["ks"], abs(c["alpha"]), inp["live"])
    dead = ~inp["live"][:, None].expand_as(g) if inp["keep"] is None else (~inp["keep"] | ~inp["live"][:, None])
    if dead.any():
        exact(what, "rows", "dx where the x branch is dropped or masked", torch.where(dead, k["dx"].to(F64), 0.0), torch.zeros_like(g), _d2(path))
    al = None if allow is None else tail_grad(allow, inp["keep"], inp["ks"], abs(c["alpha"]), inp["live"])
    st[pre + "dx"], st["dx_flips"] = judge(what, "rows", "dx", k["dx"], g, A_g, delta[pre + "dx"], io, _d2(path), al)
    ft = allow is not None
    two = fam == "aln2"                          # dy_total is itself a cancelled sum: its terms' magnitudes, not its own
    _param(what, st, "dgamma", k.get("dgamma"), b["tg"], delta, pre + "dgamma", ud * b["h"].abs() if ft else None, A2 * b["h"].abs() if two else None)
    _param(what, st, "dbeta", k.get("dbeta"), b["tb"], delta, pre + "dbeta", ud if ft else None, A2 if two else None)
    _param(what, st, "dbias", k.get("dbias"), g, delta, pre + "dbias", al if ft else None, A_g)
    return st


def check_eltwise(c, inp, k, delta, what=""):
    """bias_act_dropout / dropout_add / dropout_add2, forward and backward. The products of the backward (and the whole bias_act_dropout
    forward) contain no sum after the first, so they are fp32-exact: compared bit for bit with the fp32 emulation."""
    fam, io, M, D = c["fam"], c["io"], c["M"], c["D"]
    p = f"{'bias_act_dropout' if fam == 'bad' else 'dropout_add'}_kernel<{TNAME[io]}>"
    d2 = lambda ix: f"(row={ix[0]}, column={ix[1]}, element index {ix[0] * D + ix[1]})"  # noqa: E731
    e = emulate(c, inp)
    st = {}
    zero = torch.zeros(M, D, dtype=F64)
    if fam == "bad":
        exact(what, "forward", "y (dropped: 0; kept: act(x + bias) 65536 / (65536 - thr) in fp32)", k["y"], e["y"], d2)
        g = inp["dy"].to(F32)
        if inp["keep"] is not None:
            g = torch.where(inp["keep"], g * np.float32(inp["ks"]), torch.zeros((), dtype=F32))
        if c["slope"] >= 0:
            g = torch.where(k["y"].to(F32) < 0, g * np.float32(c["slope"]), g)
        exact(what, "backward", "dx (the forward's mask bits)", k["dx"], store(g, io), d2)
        _param(what, st, "dbias", k.get("dbias"), g.to(F64), delta)
        return st
    s, A = tail(inp["x"], inp["bias"], inp["res"], inp["keep"], inp["ks"], c["alpha"], inp["live"], F64)
    d = inp["dy"].to(F32)
    if fam == "da2" and inp["keep2"] is not None:
        exact(what, "forward", "out where the outer dropout drops", torch.where(inp["keep2"], zero, k["out"].to(F64)), zero, d2)
        # a flip of the rounded intermediate, where its rounding is ambiguous under delta["s"], moves out by ks2 ulp
        allow = torch.where(inp["keep2"] & ambiguous(s, A, delta["s"]), ulp_bf16(s) * inp["ks2"], zero) if io == "bf16" else None
        s, A = rnd(s, io) * inp["ks2"], A * inp["ks2"]
        s, A = torch.where(inp["keep2"], s, zero), torch.where(inp["keep2"], A, zero)
        d = rnd(torch.where(inp["keep2"], d * np.float32(inp["ks2"]), torch.zeros((), dtype=F32)), io)
        exact(what, "backward", "dres (the outer mask bits)", k["dres"], store(d, io), d2)
    else:
        allow = None
        dead = ~inp["live"][:, None].expand_as(s) if inp["keep"] is None else (~inp["keep"] | ~inp["live"][:, None])
        if dead.any():
            exact(what, "forward", "out where the x branch is dropped or masked", torch.where(dead, k["out"].to(F64), zero), torch.where(dead, inp["res"].to(F64), zero), d2)
    st["s"], st["s_flips"] = judge(what, "forward", "out", k["out"], s, A, delta["s"], io, d2, allow)
    g = d * np.float32(c["alpha"]) * inp["live"][:, None].to(F32)
    if inp["keep"] is not None:
        g = torch.where(inp["keep"], g * np.float32(inp["ks"]), torch.zeros((), dtype=F32))
    exact(what, "backward", "dx (the forward's mask bits)", k["dx"], store(g, io), d2)
    _param(what, st, "dbias", k.get("dbias"), g.to(F64), delta)
    return st


def check_colsum(c, inp, out_k, delta, what=""):
    x = inp["x"].to(F64)
    ref, A = x.sum(0), x.abs().sum(0)
    if c["acc"]:
        ref, A = ref + inp["out0"].to(F64), A + inp["out0"].to(F64).abs()
    w, _ = judge(what, "columns", "out", out_k, ref, A, delta["colsum"], "f32", _dcol)
    return {"colsum": w}


def check_case(c, inp, k, delta, what=None, flip_cap=None):
    """every stage check of a case on the outputs k (a kernel's or the emulation's) -> statistics. Raises Mismatch."""
    fam = c["fam"]
    what = what or c["key"]
    paths = case_paths(c)
    global _CAP
    old, _CAP = _CAP, flip_cap
    try:
        if fam == "colsum":
            return check_colsum(c, inp, k["out"], delta, what)
        if fam in ("bad", "da", "da2"):
            return check_eltwise(c, inp, k, delta, what)
        if fam == "ln":
            st = check_ln_fwd(c, inp, k, delta, f"tsasr_layernorm_fwd {paths['layernorm_fwd']} {what}", paths["layernorm_fwd"])
            e = "layernorm_bwd_add" if c["dadd"] else "layernorm_bwd"
            b = check_ln_bwd(c, inp, k, delta, f"tsasr_{e} {paths[e]} {what}", paths[e])
            st["min_abs_pre"] = min(st.get("min_abs_pre", math.inf), b.pop("min_abs_pre", math.inf))
            st.update(b)
            return st
        n = "add_layernorm" if fam == "aln" else "add_layernorm2"
        wf, wb = f"tsasr_{n}_fwd {paths[n + '_fwd']} {what}", f"tsasr_{n}_bwd {paths[n + '_bwd']} {what}"
        st = check_tail_fwd(c, inp, k["s"], delta, wf, paths[n + "_fwd"])
        st.update(check_ln_fwd(c, inp, k, delta, wf, paths[n + "_fwd"], x_key="s", slope=-1.0))
        if fam == "aln2":
            st.update(check_ln_fwd(c, inp, k, delta, wf, paths[n + "_fwd"], x_key="y", pre="2", gamma="gamma2", beta="beta2", eps=c["eps2"], slope=-1.0))
        st.update(check_aln_bwd(c, inp, k, delta, wb, paths[n + "_bwd"]))
        return st
    finally:
        _CAP = old


DELTA_KEYS = ("dyt", "mean", "rstd", "y", "2mean", "2rstd", "2y", "s", "dx", "dres", "dgamma", "dbeta", "dbias", "dgamma2", "dbeta2", "aln2.dx", "aln2.dres",
              "aln2.dgamma", "aln2.dbeta", "aln2.dbias", "colsum")
INF = {k: float("inf") for k in DELTA_KEYS}


def emu_flip_shares(c, inp):
    st = check_case(c, inp, emulate(c, inp), INF, flip_cap=1.0)
    return {k: v for k, v in st.items() if k.endswith("_flips")}


def deltas(io):
    return {k: v[0] for k, v in TOL[io].items()}


# ------------------------------------------------------------------------------------------------------------------ the bounds
# delta = 4 x the worst stage-check distance of the fp32 emulation (run free, then checked like a kernel) over matrix(), per io type and
# quantity, relative to A: (bound, the CPU measurement it came from). The factor covers the kernels summing rows by DPP tree and columns by
# workgroup in another association than the emulation's, which is bounded by a small multiple of the same eps A. Measured against the model
# and the emulation only, never against kernel output. The "aln2." entries are the first LayerNorm's quantities in add_layernorm2_bwd, whose
# input dy_total is an unreturned tensor rounded to the io type: on bf16 its one-ulp flips are part of the measurement of the fp32 sums
# (hence the wider deltas) and are allowed for, not measured, in dres / dx.
# Each delta is 4 x max(measurement, FLOOR). The row outputs (y, s, dx, dres, ...) take the larger of the two io types' measurements: the same
# fp32 arithmetic writes both, and a bf16 case only measures its non-nearest elements.
# KINK_MARGIN = at least 100 x the emulation's worst |pre-activation - float64 pre-activation| over the slope >= 0 cases (EMU_PRE_ERR).
EMU_PRE_ERR = 9.196e-07      # derive(), with KINK_MARGIN = 1e-4 in force; x 100 = 9.2e-05
KINK_MARGIN = 1e-4
FLOOR = 2.0 ** -24           # half an fp32 ulp: no figure below it is a measurement of arithmetic (sums of a few bf16 values are exact on the CPU)
TOL = {
    "flips": 0.01,           # share of a bf16 output that may be other than the nearest bf16 of its reference, per case: the project's cap, a condition
    "bf16": {"mean": (2.38e-07, 4.83e-08), "rstd": (6.72e-07, 1.68e-07), "y": (1.03e-06, 2.57e-07), "dx": (6.61e-07, 1.65e-07), "dgamma": (8.25e-07,
             2.06e-07), "dbeta": (6.32e-07, 1.58e-07), "s": (6.67e-07, 1.67e-07), "dres": (5.37e-07, 1.34e-07), "dbias": (3.91e-07, 9.78e-08), "2mean":
             (2.38e-07, 2.31e-08), "2rstd": (6.98e-07, 1.74e-07), "2y": (8.94e-07, 2.24e-07), "dgamma2": (4.79e-07, 1.20e-07), "dbeta2": (2.38e-07,
             9.56e-09), "dyt": (5.38e-07, 1.35e-07), "aln2.dres": (1.14e-06, 2.86e-07), "aln2.dx": (9.05e-07, 2.26e-07), "aln2.dgamma": (4.24e-07,
             1.06e-07), "aln2.dbeta": (2.38e-07, 3.43e-09), "aln2.dbias": (2.52e-07, 6.30e-08), "colsum": (2.38e-07, 5.72e-08)},
    "f32": {"mean": (2.95e-07, 7.37e-08), "rstd": (6.66e-07, 1.67e-07), "y": (1.03e-06, 2.57e-07), "dx": (6.61e-07, 1.65e-07), "dgamma": (7.55e-07,
            1.89e-07), "dbeta": (5.99e-07, 1.50e-07), "s": (6.67e-07, 1.67e-07), "dres": (5.37e-07, 1.34e-07), "dbias": (4.65e-07, 1.16e-07), "2mean":
            (2.78e-07, 6.94e-08), "2rstd": (7.37e-07, 1.84e-07), "2y": (8.94e-07, 2.24e-07), "dgamma2": (4.85e-07, 1.21e-07), "dbeta2": (2.38e-07,
            9.18e-09), "dyt": (5.38e-07, 1.35e-07), "aln2.dres": (1.14e-06, 2.86e-07), "aln2.dx": (9.05e-07, 2.26e-07), "aln2.dgamma": (3.22e-07,
            8.04e-08), "aln2.dbeta": (2.43e-07, 6.08e-08), "aln2.dbias": (3.45e-07, 8.64e-08), "colsum": (2.38e-07, 5.80e-08)},
    # the emulation's own worst shares over the matrix (every case at most TOL["flips"] / 4; no case needed a second draw)
    "emu_flips": {"y_flips": 1.78e-04, "dx_flips": 9.38e-04, "s_flips": 2.05e-04, "dres_flips": 9.38e-04, "2y_flips": 1.88e-04},
}
SEEDS = {}                   # draw each case ends on, found by case_inputs(search=True); absent: 0


def derive(verbose=True):
    """The CPU measurements behind TOL, EMU_PRE_ERR and SEEDS. Two passes: "s" and "dyt" decide where the rounding of an unreturned bf16
    intermediate is ambiguous, so they are measured first (nothing they are measured on depends on an allowance) and then held at 4 x."""
    first = {io: dict(INF) for io in IOS}
    for rnd_no in (0, 1):
        worst, flips, seeds, pre_err = {io: {} for io in IOS}, {}, {}, 0.0
        for c in matrix():
            inp, n = case_inputs(c, search=True)
            if n:
                seeds[c["key"]] = n
            e = emulate(c, inp)
            if c["fam"] == "ln" and c["slope"] >= 0:
                pre_err = max(pre_err, float((e["pre"].to(F64) - pre_activation(inp["x"], inp["gamma"], inp["beta"], c["eps"])).abs().max()))
            st = check_case(c, inp, e, first[c["io"]], flip_cap=1.0)
            for k, v in st.items():
                if k.endswith("_flips"):
                    flips[k] = max(flips.get(k, 0.0), v)
                elif k != "min_abs_pre":
                    worst[c["io"]][k] = max(worst[c["io"]].get(k, 0.0), v)
            if verbose and rnd_no:
                print(f"{c['key']:70s} +{n} " + " ".join(f"{k} {v:.2e}" for k, v in st.items()), flush=True)
        for io in IOS:
            for k in ("s", "dyt"):
                first[io][k] = 4 * max(FLOOR, max(worst[i][k] for i in IOS))
    for k in ROW_OUTPUTS:                        # the same fp32 arithmetic writes both io types: a bf16 output's delta is the larger figure
        worst["bf16"][k] = max(worst[io].get(k, 0.0) for io in IOS)
    if verbose:
        print(f"EMU_PRE_ERR = {pre_err:.3e}    # x 100 = {100 * pre_err:.3e}")
        for io in IOS:
            print(f'TOL["{io}"] = {{' + ", ".join(f'"{k}": ({4 * max(v, FLOOR):.2e}, {v:.2e})' for k, v in worst[io].items()) + "}")
        print('TOL["emu_flips"] = {' + ", ".join(f'"{k}": {v:.2e}' for k, v in flips.items()) + "}")
        print("SEEDS =", seeds)
    return worst, flips, pre_err, seeds


ROW_OUTPUTS = ("y", "2y", "s", "dx", "dres", "dyt", "aln2.dx", "aln2.dres")


if __name__ == "__main__":
    derive()
