"""float64 references, host-plan mirrors and the case matrix for the gradient tail: grouped weight gradients (csrc/wgrad.hip), batched
reductions (csrc/reduce.hip), the deferred-gradient add and the weight transposes (csrc/optim.hip), the non-finite counter (csrc/misc.hip),
global-norm clipping + AdamW (csrc/optim.hip) and the arena that ties them together (dp.GradArena). Test infrastructure only.

Two regimes, as in gemm_ref.py:

  exact     small-integer operands / gradients: every fp32 partial sum is an integer below 2^24, so EVERY summation order gives the float64
            result bit for bit (gemm_ref.assert_exact_regime proves the precondition, gemm_ref.check_exact compares with tolerance 0).
  rounding  Gaussian data: adamw_step64 is the yardstick, adamw_step32 (an fp32 numpy restatement of the kernel's operation order) measures
            what fp32 arithmetic alone costs, and TOL = 4 x that measurement is what a kernel gets (-ffp-contract=fast may fuse differently).

adamw_step64 takes the scalars the kernel receives as `float` (beta1, beta2, eps, weight decay, max_norm) and the three device floats of
`hyper` ROUNDED TO fp32 first, then computes in float64: hyper-parameter rounding is not charged to the kernel."""
import math

import numpy as np
import torch

F32_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24           # unit roundoff of fp32 (round to nearest)
OPT_PARTS, OPT_MAX_WGS = 1024, 2048
WG_TILE, WG_BK = 256, 32
ACC_SPLIT = 16
RD_WIDE_TILE, RD_TALL_COLS = 1024, 64
PAD = 64                 # dp._PAD


def r32(x):
    """a Python float rounded to fp32, as a float64"""
    return float(np.float32(x))


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ clip + AdamW
def hyper3(lr, beta1, beta2, t):
    """the device array optim._clip_adamw / FusedClipAdamW.prepare ship: fp32 {lr, 1 - beta1^t, 1 - beta2^t} (computed in double, stored fp32)"""
    return np.array([lr, 1.0 - beta1 ** t, 1.0 - beta2 ** t], dtype=np.float32)


def clip_coef64(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max=1) - NaN stays NaN, Inf gives 0; max_norm <= 0: no clipping"""
    if not max_norm > 0:
        return 1.0
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(norm) + r32(1e-6))
    return float(c) if c != c else float(min(1.0, c))


def adamw_step64(p, g, m, v, hyper, beta1, beta2, eps, wd, max_norm, skip=False, round_scalars=True):
    """One tsasr_clip_adamw_step in float64: clip_grad_norm_(max_norm) + torch.optim.AdamW (decoupled decay p *= 1 - lr wd, then
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)). hyper = {lr, 1 - beta1^t, 1 - beta2^t}. skip: a counter is passed - a non-finite norm
    leaves everything alone. Returns a dict: p, m, v (float64 arrays), norm, clip, skipped (0 / 1).
    round_scalars False: take every scalar as the double it is (the comparison with torch.optim.AdamW in float64)."""
    rs = r32 if round_scalars else float
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, bc1, bc2 = (float(h) for h in np.asarray(hyper, dtype=np.float32 if round_scalars else np.float64))
    b1, b2, eps, wd, max_norm = rs(beta1), rs(beta2), rs(eps), rs(wd), rs(max_norm)
    with np.errstate(all="ignore"):
        norm = float(np.sqrt((g * g).sum()))
        if skip and not math.isfinite(norm):
            return {"p": p.copy(), "m": m.copy(), "v": v.copy(), "norm": norm, "clip": float("nan"), "skipped": 1,
                    "scale": {"p": np.abs(p), "m": np.abs(m), "v": np.abs(v)}}
        clip = clip_coef64(norm, max_norm)
        gk = g * clip
        m2 = b1 * m + (1.0 - b1) * gk
        v2 = b2 * v + (1.0 - b2) * gk * gk
        denom = np.sqrt(v2) / math.sqrt(bc2) + eps
        p2 = p * (1.0 - lr * wd) - (lr / bc1) * m2 / denom
        # what an fp32 error of each output is measured against: the largest term that went into it. m: beta1 m and (1 - beta1) g clip (they
        # may cancel); v: its two positive terms; p: the old and new value and the step formed from m's LARGEST term - where m's terms
        # cancel, one rounding of the larger one is many ulps of m, and the step inherits it
        ms = np.maximum(np.maximum(np.abs(b1 * m), np.abs((1.0 - b1) * gk)), np.abs(m2))
        vs = np.maximum(np.maximum(b2 * v, (1.0 - b2) * gk * gk), v2)
        ps = np.maximum(np.maximum(np.abs(p), np.abs(p2)), np.abs(lr / bc1) * ms / denom)
    return {"p": p2, "m": m2, "v": v2, "norm": norm, "clip": clip, "skipped": 0, "scale": {"p": ps, "m": ms, "v": vs}}


def sumsq_per(n):
    """elements per part of sumsq_partials_kernel: n / 1024 rounded up, then up to a multiple of 4 (every part starts 16-byte aligned)"""
    return (cdiv(n, OPT_PARTS) + 3) & ~3


def sumsq_parts(n):
    """[(lo, hi)] of the 1024 parts"""
    per = sumsq_per(n)
    return [(min(n, b * per), min(n, min(n, b * per) + per)) for b in range(OPT_PARTS)]


def sumsq_paths(n):
    """which pieces of sumsq_partials_kernel run at this n: {"unrolled1" (thread 0 only), "unrolled_all" (every thread at least one round),
    "unrolled2" (a second round), "single" (the one-load loop), "tail" (the scalar tail of a part), "empty" (a part with no elements)}"""
    out = set()
    for lo, hi in sumsq_parts(n):
        if hi == lo:
            out.add("empty")
            continue
        hi4 = lo + ((hi - lo) & ~3)
        if hi4 < hi:
            out.add("tail")
        for tid in (0, 255):
            i, rounds = lo + tid * 4, 0
            while i + 3 * 1024 + 4 <= hi4:
                i, rounds = i + 4096, rounds + 1
            if rounds >= 1:
                out.add("unrolled1" if tid == 0 else "unrolled_all")
            if rounds >= 2:
                out.add("unrolled2")
            if i + 4 <= hi4:
                out.add("single")
    return out


def opt_wgs(n):
    """workgroups of clip_adamw_kernel: one thread per 4 elements (a last partial group counts), capped at 2048 - then the grid strides"""
    return min(OPT_MAX_WGS, cdiv(cdiv(n, 4), 256))


def opt_paths(n):
    out = {"vec4"} if n >= 4 else set()
    if n % 4:
        out.add("scalar_tail")
    if n > OPT_MAX_WGS * 1024:
        out.add("grid_stride")
    return out


def _tree(x):
    """pairwise sum over the last axis (a power of two): the pairing of wave_sum's quad / mirror steps"""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def sumsq32(g):
    """fp32 restatement of sumsq_partials_kernel + the re-reduction in clip_adamw_kernel. Per part: round r of 1024 elements is one 16-byte
    load per thread, ((x^2 + y^2) + z^2) + w^2, added to accumulator r % 4 while four whole rounds remain and to accumulator 0 afterwards
    (exact for thread 0, off by one round for the threads behind the part's end); the scalar tail goes to thread 0; (s0 + s1) + (s2 + s3);
    wave tree; four waves in order. Then 1024 partials: 4 per thread in order, wave tree, four waves in order."""
    g = np.asarray(g, dtype=np.float32)
    n, per = g.size, sumsq_per(g.size)
    rounds = cdiv(per, 1024)
    buf = np.zeros(OPT_PARTS * rounds * 1024, dtype=np.float32).reshape(OPT_PARTS, rounds * 1024)
    flat = np.zeros(OPT_PARTS * per, dtype=np.float32)
    flat[:n] = g
    buf[:, :per] = flat.reshape(OPT_PARTS, per)
    x = buf.reshape(OPT_PARTS, rounds, 256, 4)
    sq = x * x
    load = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]            # [parts, rounds, 256]
    acc = np.zeros((4, OPT_PARTS, 256), dtype=np.float32)
    unrolled = 4 * ((per - 3076) // 4096 + 1) if per >= 3076 else 0       # rounds thread 0 takes four at a time
    for r in range(rounds):
        a = r % 4 if r < unrolled else 0
        acc[a] = acc[a] + load[:, r]
    s = (acc[0] + acc[1]) + (acc[2] + acc[3])                               # [parts, 256]
    w = _tree(s.reshape(OPT_PARTS, 4, 64))
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]                        # [parts]
    t = part.reshape(4, 256)
    s = ((t[0] + t[1]) + t[2]) + t[3]
    w = _tree(s.reshape(4, 64))
    return np.float32(((w[0] + w[1]) + w[2]) + w[3])


def adamw_step32(p, g, m, v, hyper, beta1, beta2, eps, wd, max_norm):
    """fp32 numpy restatement of clip_adamw_kernel's operation order (no fused multiply-adds). Same returns as adamw_step64, fp32."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    h = np.asarray(hyper, dtype=f)
    b1, b2, eps, wd, max_norm = f(beta1), f(beta2), f(eps), f(wd), f(max_norm)
    with np.errstate(all="ignore"):
        norm = np.sqrt(sumsq32(g))
        clip = f(1)
        if max_norm > 0:
            c = max_norm / (norm + f(1e-6))
            clip = c if c != c else min(f(1), c)
        lr, bc1, bc2s = h[0], h[1], np.sqrt(h[2])
        step, decay = lr / bc1, f(1) - lr * wd
        gk = g * clip
        m2 = b1 * m + (f(1) - b1) * gk
        v2 = b2 * v + (f(1) - b2) * gk * gk
        p2 = p * decay - step * m2 / (np.sqrt(v2) / bc2s + eps)
    return {"p": p2, "m": m2, "v": v2, "norm": float(norm), "clip": float(clip), "skipped": 0}


def ulp32(x):
    """fp32 unit in the last place at |x| (float64 array), 2^-149 at 0"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    return np.maximum(2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 23), 2.0 ** -149)


def update_errors(got, ref, prev):
    """{"p", "m", "v"}: worst |got - ref| in fp32 ulps of ref["scale"] (max(|result|, |largest term|), see adamw_step64); "norm": |got - ref| /
    (2^-24 ref). ref: adamw_step64 from the state `prev` the code under test started from."""
    sc = ref["scale"]
    out = {k: float((np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]) / ulp32(sc[k])).max()) for k in ("p", "m", "v")}
    out["norm"] = abs(float(got["norm"]) - ref["norm"]) / (U * max(ref["norm"], 1e-300))
    return out


def norm_depth(n):
    """longest chain of fp32 roundings on the way from one g^2 to the sum: the product, 3 adds inside a load, one accumulate per round of the
    part (a thread's accumulators take ceil(per / 1024) loads between them, at most that many in one chain), 2 to join the four
    accumulators, 6 wave steps, 3 for the four waves; then the second level: 3 (four partials per thread), 6, 3."""
    return 1 + 3 + cdiv(sumsq_per(n), 1024) + 2 + 6 + 3 + 3 + 6 + 3


def norm_bound(n, sumsq):
    """|norm - sqrt(sumsq)| allowed for a Gaussian gradient: every term is positive, so |fl(sum) - sum| <= depth 2^-24 sum (first order, 1.01
    for the rest); the square root halves a relative error and adds half an ulp of its own (<= 2^-24 relative)."""
    return (0.5 * 1.01 * norm_depth(n) + 1.0) * U * math.sqrt(sumsq)


# measured by tests/test_gradtail_ref_cpu.py::test_fp32_emulation_sets_the_tolerances (python -m pytest -s tests/test_gradtail_ref_cpu.py -k
# sets_the_tolerances prints the table): adamw_step32 against adamw_step64, n = 200 003 and 1 000 003, three steps in each of the four clip
# regimes, worst value of update_errors per output; "gpu" = 4 x measured (the kernel may contract a * b + c where numpy does not).
# Units: fp32 ulps of max(|result|, |largest term|) (adamw_step64's "scale"). m and v are mostly the clip coefficient's own rounding.
TOL = {
    "measured": {"p": 4.17, "m": 3.17, "v": 5.38},
    "gpu": {"p": 16.68, "m": 12.68, "v": 21.52},
}

ADAM = dict(beta1=0.9, beta2=0.98, eps=1e-8, wd=0.01)
REGIMES = {"clipped": 5.0, "unclipped": 1e9, "off": 0.0, "zero_grad": 5.0}     # name -> max_norm (zero_grad: g = 0)


def gaussian_case(n, seed, regime="clipped"):
    """deterministic p, g[3 steps], m0 = v0 = 0 (fp32 arrays) for the Gaussian update checks"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = [(rng.standard_normal(n) * (0.0 if regime == "zero_grad" else 3.0 * (k + 1))).astype(np.float32) for k in range(3)]
    return p, g


STEP_LR = (1e-3, 7e-4, 2.5e-3)       # lr of steps t = 1, 2, 3 (the Noam schedule changes it through the device array)

OPT_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4099, 3_149_824, 5_000_003, 8_392_709)


def exact_gradient(n, seed):
    """int8-valued fp32 gradient in {-2 .. 2} whose sum of squares stays below 2^24 (the density of non-zeros falls with n), and that sum"""
    rng = np.random.default_rng(seed)
    g = rng.integers(-2, 3, size=n).astype(np.float32)
    keep = min(1.0, 4.0e6 / n)          # E[g^2] = 2 -> expected sum 2 n keep <= 8e6 < 2^24
    if keep < 1.0:
        g *= rng.random(n) < keep
    ss = int((g.astype(np.int64) ** 2).sum())
    assert ss < (1 << 24), ss
    return g, ss


def single_positions(n):
    """element 0, element n - 1, and the first and last element of a middle part that is not empty"""
    parts = [(lo, hi) for lo, hi in sumsq_parts(n) if hi > lo]
    lo, hi = parts[len(parts) // 2]
    return sorted({0, n - 1, lo, hi - 1})


# ------------------------------------------------------------------------------------------------------------------ grouped weight gradients
def wgrad_tiles(M, N):
    return cdiv(M, WG_TILE) * cdiv(N, WG_TILE)


def wgrad_plan(jobs):
    """jobs: [(M, N, K)] in queue order -> (order: indices sorted by K descending, stable; tile0 per sorted job; total tiles)"""
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][2])
    tile0, t = [], 0
    for i in order:
        tile0.append(t)
        t += wgrad_tiles(jobs[i][0], jobs[i][1])
    return order, tile0, t


def xcd_id(bid, total):
    """workgroup -> tile: the 8 XCDs take workgroups round-robin; XCD x gets a contiguous run of tiles (the first total & 7 runs one longer)"""
    xcd, q, rem = bid & 7, total >> 3, total & 7
    return (xcd * (q + 1) if xcd < rem else rem * (q + 1) + (xcd - rem) * q) + (bid >> 3)


def search64(tile0, tid):
    """the 64-ary search of wgrad_group_kernel / reduce_many_kernel: (index of the last job whose first tile <= tid, levels probed)"""
    lo, n, levels = 0, len(tile0), 0
    while n > 1:
        step = (n + 63) >> 6
        seg = sum(1 for lane in range(64) if lane * step < n and tile0[lo + lane * step] <= tid) - 1
        lo += seg * step
        n = min(step, n - seg * step)
        levels += 1
    return lo, levels


def wgrad_ktiles(K):
    """(k-tiles of 32 rows, rows of the last one when it is ragged else 0)"""
    return cdiv(K, WG_BK), K % WG_BK


WG_K = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 200)
WG_MN = ((8, 8), (264, 256), (256, 264), (136, 520), (512, 512))
WG_MANY = (1, 2, 63, 64, 65, 200)


def many_jobs(count):
    """`count` small jobs of 8x8 .. 24x40 with distinct K (queue order is NOT K order), one 520 x 264 job in the middle"""
    jobs = []
    for i in range(count):
        jobs.append((8 * (1 + i % 3), 8 * (1 + (i * 7) % 5), 1 + (i * 37) % 211 if count <= 211 else 1 + i))
    ks = [j[2] for j in jobs]
    assert len(set(ks)) == len(ks)
    if count >= 2:
        jobs.insert(count // 2, (520, 264, 77))
    return jobs


def wg_variants(tiles):
    """(name, slots, wgs) of every launch variant for a flush of `tiles` tiles"""
    out = [("default", 0, 0), ("slots2", 2, 0)]
    for w in sorted({1, 3, tiles - 1, tiles, tiles + 5}):
        if w >= 1:
            out.append((f"wgs{w}", 0, w))
    out.append(("slots2_wgs3", 2, 3))
    return out


# ------------------------------------------------------------------------------------------------------------------ transposes
def transpose_jobs(mats, src_offsets=None, pad=PAD):
    """as dp.GradArena.refresh_shadow: mats [(rows, cols)] -> ([(src off, dst off, rows, cols, first tile)], tiles, dst elements). Sources sit
    at multiples of `pad` elements (or at src_offsets), transposed copies at multiples of `pad` (pad = 1: packed back to back)."""
    jobs, s_off, t_off, tiles = [], 0, 0, 0
    for k, (r, c) in enumerate(mats):
        so = s_off if src_offsets is None else src_offsets[k]
        jobs.append((so, t_off, r, c, tiles))
        s_off = so + cdiv(r * c, PAD) * PAD
        t_off += cdiv(r * c, pad) * pad
        tiles += cdiv(r, 64) * cdiv(c, 64)
    return jobs, tiles, t_off


def transpose_fast(job, lt):
    """does local tile `lt` of a job take the vectorised whole-tile path?"""
    so, do, rows, cols, _ = job
    tcn = cdiv(cols, 64)
    r0, c0 = (lt // tcn) * 64, (lt % tcn) * 64
    return r0 + 64 <= rows and c0 + 64 <= cols and cols % 8 == 0 and rows % 8 == 0 and (so | do) % 8 == 0


def transpose_paths(jobs):
    out = set()
    for j in jobs:
        for lt in range(cdiv(j[2], 64) * cdiv(j[3], 64)):
            out.add("fast" if transpose_fast(j, lt) else "general")
    return out


TR_MATS = ((64, 64), (256, 2048), (2048, 256), (72, 200), (29, 640), (17, 241), (16, 4096), (128, 128))


def distinct_bits(n, start=1):
    """n 16-bit patterns, distinct while n <= 65535, as an int16 tensor (viewed as bf16 by the caller)"""
    return torch.from_numpy(((np.arange(n, dtype=np.int64) * 40503 + start) % 65536).astype(np.uint16).view(np.int16).copy())


# ------------------------------------------------------------------------------------------------------------------ reductions
def reduce_wide(nparts, width):
    return nparts < 32 and width >= 4096


def reduce_tiles(nparts, width):
    return cdiv(width, RD_WIDE_TILE) if reduce_wide(nparts, width) else cdiv(width, RD_TALL_COLS)


def colsum_parts(M):
    """partial rows tsasr_colsum leaves for [M, N]: rows per workgroup = max(64, ceil(M / 1024))"""
    rpw = max(64, cdiv(M, 1024))
    return cdiv(M, rpw)


def gemm_splits(M, N, K):
    """split-K factor of an fp32-output tsasr_gemm_bf16 (mirror of plan() in csrc/gemm.hip): (splits, slab bytes of the workspace)"""
    t0, t1, t2 = cdiv(M, 128) * cdiv(N, 128), cdiv(M, 128) * cdiv(N, 64), cdiv(M, 64) * cdiv(N, 64)
    tiles = t0 if t0 >= 512 else (t1 if t1 >= 192 else t2)
    s = 1
    if tiles < 256 and K >= 384:
        s = max(1, min(cdiv(768, tiles), max(1, K // 128), 32))
    kchunk = cdiv(cdiv(K, s), 64) * 64
    s = cdiv(K, kchunk)
    return s, (cdiv(s * M * N * 4, 256) * 256 if s > 1 else 0)


RD_COUNTS = (1, 2, 64, 65, 300)
RD_WIDTHS = (8, 64, 72, 520)
RD_GEMM = ((64, 64, 512), (32, 136, 384), (128, 64, 1024))       # (M, N, K): width M N >= 4096, a handful of slabs -> wide jobs


def reduce_jobs(count):
    """`count` jobs, round-robin: colsum [M, width] (accumulate on every other one) with a wide split-K GEMM every 16th job"""
    jobs = []
    for i in range(count):
        if i % 16 == 5 or (count == 1 and False):
            jobs.append(("gemm",) + RD_GEMM[(i // 16) % len(RD_GEMM)])
        else:
            jobs.append(("colsum", (65, 200, 1100, 64, 3000)[i % 5], RD_WIDTHS[i % 4], i % 2))
    return jobs


# ------------------------------------------------------------------------------------------------------------------ accumulate_many
ACC_COUNTS = (1, 3, 70)
ACC_LENS = (0, 1, 255, 256, 257, 4095, 4096, 4097, 100_003)


def acc_lengths(count):
    return [ACC_LENS[(i * 4 + count) % len(ACC_LENS)] for i in range(count)] if count < len(ACC_LENS) else [ACC_LENS[i % len(ACC_LENS)] for i in range(count)]


def acc_paths(n):
    """pieces of accumulate_many_kernel a vector of n elements reaches"""
    out = {"empty"} if n == 0 else set()
    if 0 < n:
        out.add("one_piece" if n <= 256 else "many_wgs")
    if n > 256 * ACC_SPLIT:
        out.add("second_round")
    if n % 256:
        out.add("ragged_piece")
    return out


# ------------------------------------------------------------------------------------------------------------------ the matrix
def matrix():
    """every case of tests/test_gradtail_paths_gpu.py with the paths the mirrors say it reaches: [{"key", "fam", "paths", ...}]"""
    cs = []
    for n in OPT_SIZES:
        cs.append({"key": f"adamw_n{n}", "fam": "adamw", "n": n,
                   "paths": {"sumsq:" + s for s in sumsq_paths(n)} | {"adamw:" + s for s in opt_paths(n)}})
    for name in REGIMES:
        cs.append({"key": f"adamw_regime_{name}", "fam": "adamw_regime", "regime": name, "paths": {"clip:" + name}})
    for n in (1, 63, 64, 65, 1000):
        cs.append({"key": f"nonfinite_n{n}", "fam": "nonfinite", "n": n, "paths": {"nonfinite:" + ("one_round" if n <= 64 else "strided")}})
    for count in ACC_COUNTS:
        ls = acc_lengths(count)
        cs.append({"key": f"acc_{count}", "fam": "acc", "lengths": ls, "paths": set().union(*({"acc:" + s for s in acc_paths(n)} for n in ls))})
    for njobs in (1, 2, 33):
        mats = tr_mats(njobs)
        for pad in (PAD, 1):
            jobs, tiles, _ = transpose_jobs(mats, pad=pad)
            paths = {"tr:" + s for s in transpose_paths(jobs)}
            if pad == 1 and any(not transpose_fast(j, 0) for j in jobs if (j[2], j[3]) == (128, 128)):
                paths.add("tr:general_by_offset")
            if njobs > 2:
                paths.add("tr:search")
            cs.append({"key": f"tr_{njobs}_pad{pad}", "fam": "tr", "mats": mats, "pad": pad, "paths": paths})
    for (M, N) in WG_MN:
        for K in WG_K:
            nk, tail = wgrad_ktiles(K)
            paths = {f"wg:ktiles{nk}", "wg:tail" if tail else "wg:notail"}
            if nk > 4:
                paths.add("wg:ring4_wrap")
            if nk > 2:
                paths.add("wg:ring2_wrap")
            if M % WG_TILE or N % WG_TILE:
                paths.add("wg:edge_tile")
            cs.append({"key": f"wg_{M}x{N}_k{K}", "fam": "wg", "M": M, "N": N, "K": K, "paths": paths})
    for count in WG_MANY:
        jobs = many_jobs(count)
        order, tile0, total = wgrad_plan(jobs)
        levels = max(search64(tile0, t)[1] for t in range(total))
        paths = {f"wg:search_levels{levels}", f"wg:xcd_rem{total & 7}"}
        if order != list(range(len(jobs))):
            paths.add("wg:sort_reorders")
        cs.append({"key": f"wg_many{count}", "fam": "wg_many", "jobs": jobs, "tiles": total, "paths": paths})
    for t in range(1, 18):
        cs.append({"key": f"wg_tiles{t}", "fam": "wg_tiles", "jobs": tiles_jobs(t), "tiles": t, "paths": {f"wg:total_tiles{t}", f"wg:xcd_rem{t & 7}"}})
    for count in RD_COUNTS:
        jobs = reduce_jobs(count)
        tile0, t, paths = [], 0, set()
        for j in jobs:
            tile0.append(t)
            nparts, width = (colsum_parts(j[1]), j[2]) if j[0] == "colsum" else (gemm_splits(*j[1:])[0], j[1] * j[2])
            paths.add("rd:wide" if reduce_wide(nparts, width) else "rd:tall")
            if j[0] == "colsum" and j[3]:
                paths.add("rd:tall_accumulate")
            if j[0] == "colsum" and nparts > 12:
                paths.add("rd:tall_unrolled")
            t += reduce_tiles(nparts, width)
        paths.add(f"rd:search_levels{max(search64(tile0, x)[1] for x in range(t))}")
        cs.append({"key": f"rd_{count}", "fam": "rd", "jobs": jobs, "paths": paths})
    cs.append({"key": "rd_streams", "fam": "rd_streams", "paths": {"rd:flush_stream"}})
    cs.append({"key": "arena", "fam": "arena", "paths": {"arena:odd_matrix", "arena:relayout", "arena:dgrad"}})
    return cs


def tr_mats(njobs):
    if njobs == 1:
        return [TR_MATS[0]]
    if njobs == 2:
        return [(17, 241), (128, 128)]
    small = [(64, 64), (72, 200), (29, 640), (17, 241), (128, 128), (16, 4096)]
    return list(TR_MATS) + [small[i % len(small)] for i in range(njobs - len(TR_MATS))]


def tiles_jobs(t):
    """jobs whose tile counts add up to t: 512 x 512 (4 tiles), 264 x 256 (2), 8 x 8 (1), K distinct"""
    jobs, k = [], 40
    while t >= 4:
        jobs.append((512, 512, k)); t -= 4; k += 3
    if t >= 2:
        jobs.append((264, 256, k)); t -= 2; k += 3
    if t:
        jobs.append((8, 8, k))
    return jobs


REQUIRED_PATHS = (
    ["sumsq:" + s for s in ("unrolled1", "unrolled_all", "unrolled2", "single", "tail", "empty")]
    + ["adamw:" + s for s in ("vec4", "scalar_tail", "grid_stride")] + ["clip:" + s for s in REGIMES]
    + ["nonfinite:one_round", "nonfinite:strided"]
    + ["acc:" + s for s in ("empty", "one_piece", "many_wgs", "second_round", "ragged_piece")]
    + ["tr:fast", "tr:general", "tr:general_by_offset", "tr:search"]
    + [f"wg:ktiles{k}" for k in range(1, 8)] + ["wg:tail", "wg:notail", "wg:ring4_wrap", "wg:ring2_wrap", "wg:edge_tile", "wg:search_levels1",
                                                 "wg:search_levels2", "wg:sort_reorders", "wg:xcd_rem0", "wg:xcd_rem1", "wg:xcd_rem7"]
    + [f"wg:total_tiles{t}" for t in range(1, 18)]
    + ["rd:wide", "rd:tall", "rd:tall_accumulate", "rd:tall_unrolled", "rd:search_levels1", "rd:search_levels2", "rd:flush_stream"]
    + ["arena:odd_matrix", "arena:relayout", "arena:dgrad"]
)
