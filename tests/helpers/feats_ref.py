"""float64 references, fp32 restatements, tolerance models and the case matrices for the feature and augmentation kernels: log-mel
filterbank and sentence normalisation (csrc/features.hip), SpecAugment and polyphase resampling (csrc/augment.hip), the speaker
mean-pool, the length rounding and the speaker injection (csrc/misc.hip). Test infrastructure only.

Layout as in gradtail_ref.py: the float64 function is the yardstick; an fp32 numpy restatement of the kernel's operation order
measures what fp32 arithmetic alone costs; the kernel gets 4 x that measurement (-ffp-contract=fast may fuse differently). Every
measured constant stands next to the case list it was measured on; tests/test_feats_ref_cpu.py re-measures them (`measure_*`) and
fails when 4 x the measurement exceeds the constant written here. Every restatement takes a ``fault`` name: the planted faults of
tests/test_feats_ref_cpu.py, which the case matrix and the tolerances must reject.

Scalars the kernels receive as `float` (amin, eps, top_db) are rounded to fp32 first: their rounding is not charged to the kernel."""
import math

import numpy as np

U = 2.0 ** -24            # unit roundoff of fp32
N_FFT = 512
SN_NT = 1024              # threads of sentence_norm_kernel


def r32(x):
    return float(np.float32(x))


def bf16_round(x):
    """fp32 array -> nearest-even bf16, returned as fp32 (finite values)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32)


def bf16_ulp(x):
    """spacing of bf16 at |x| (8 significand bits); the smallest normal's below it"""
    a = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def _rng(seed):
    return np.random.RandomState(seed)


# ====================================================================================================================== fbank
#: measured by measure_fbank() over fbank_cases() (fp32 radix-2 restatement against float64): a = 10.21 (the banded mel sum of the
#: rounded float64 power spectrum alone), c = 4.64 (what the window product, the FFT and |.|^2 need on top, worst element of the
#: matrix); x 4, rounded up:
FB_A, FB_C = 41.0, 19.0
#: elements with c u rho > FB_RHO_CUT are not resolved by fp32 and left out, at most FB_EXCL_CAP of a case
FB_RHO_CUT, FB_EXCL_CAP = 0.25, 0.01


def hamming512():
    """the periodic Hamming window as torch.hamming_window(512) holds it (fp32 table)"""
    import torch
    return torch.hamming_window(N_FFT).numpy()


def mel_matrix(n_mels):
    from oracle import tsasr_ref as R
    return R.mel_filterbank(n_mels).numpy()


def frame_signal(wav, hop, origin=N_FFT // 2):
    """[B,L] -> [B, 1 + L // hop, 512]: frame t covers samples [t * hop - origin, +512), zeros outside the signal"""
    wav = np.asarray(wav)
    B, L = wav.shape
    T = 1 + L // hop
    idx = np.arange(T)[:, None] * hop - origin + np.arange(N_FFT)[None, :]
    ok = (idx >= 0) & (idx < L)
    return np.where(ok[None], wav[:, np.clip(idx, 0, L - 1)], wav.dtype.type(0))


def _db64(s, amin):
    return 10.0 * np.log10(np.maximum(s, r32(amin)))


def fbank64(wav, window_f32, melmat_f32, hop, top_db=80.0, amin=1e-10):
    """Log-mel filterbank in float64 from the fp32 tables: frames of 512 samples with origin -256 (zero padded), window, DFT, power,
    mel product, 10 log10(max(s, amin)), per-utterance (max - top_db) floor. Returns a dict: out, raw (dB before the floor), s,
    rho = ||x_windowed||_2 sqrt(sum_k w_km / s) per element (0 where s = 0 because the column or the frame is all zero), and the
    pieces the tolerance needs (xn = ||x_windowed||_2 per frame, wsum per mel column, umax per utterance, floor)."""
    xw = frame_signal(np.asarray(wav, np.float32).astype(np.float64), hop) * np.asarray(window_f32, np.float64)
    spec = np.fft.rfft(xw, axis=-1)
    power = spec.real ** 2 + spec.imag ** 2
    mel = np.asarray(melmat_f32, np.float64)
    s = power @ mel
    raw = _db64(s, amin)
    umax = raw.max(axis=(1, 2))
    floor = umax - r32(top_db)
    out = np.maximum(raw, floor[:, None, None])
    xn = np.sqrt((xw * xw).sum(-1))
    wsum = mel.sum(0)
    with np.errstate(all="ignore"):
        rho = xn[..., None] * np.sqrt(wsum[None, None, :] / s)
    rho = np.where(s > 0, rho, np.where((wsum[None, None, :] == 0) | (xn[..., None] == 0), 0.0, np.inf))
    return {"out": out, "raw": raw, "s": s, "rho": rho, "xn": xn, "wsum": wsum, "umax": umax, "floor": floor, "amin": r32(amin)}


def fbank_ds(ref, a=FB_A, c=FB_C):
    """|ds| <= a u s + 2 e sqrt(W s) + e^2 W with e = c u ||x_windowed||: the error model |ds|/s <= a u + 2 c u rho + (c u rho)^2
    in absolute form (it stays finite where s = 0)"""
    e = c * U * ref["xn"][..., None]
    W = ref["wsum"][None, None, :]
    return a * U * ref["s"] + 2.0 * e * np.sqrt(W * ref["s"]) + e * e * W


def fbank_tol(ref, a=FB_A, c=FB_C):
    """(tol [B,T,M] in dB, excluded [B,T,M]). tol_elem carries ds through 10 log10(max(s +- ds, amin)) and adds 2 u |dB| for the fp32
    logarithm and product. max() is continuous, so an output may be off by max(tol_elem, tol_floor_b), tol_floor_b = the tolerance of
    the utterance's maximum; an element whose reference lies under the floor by more than both is held to tol_floor_b alone. Elements
    with c u rho > 0.25 whose s + ds reaches amin are excluded (below amin they are -100 whatever the FFT gives, and stay in)."""
    ds = fbank_ds(ref, a, c)
    s, raw, amin = ref["s"], ref["raw"], ref["amin"]
    hi = _db64(s + ds, amin) - raw
    lo = raw - _db64(np.maximum(s - ds, 0.0), amin)
    tol_elem = np.maximum(hi, lo) + 2.0 * U * np.abs(raw)
    excl = (c * U * ref["rho"] > FB_RHO_CUT) & (s + ds > amin)
    B = raw.shape[0]
    flat = raw.reshape(B, -1).argmax(1)
    fl = np.where(np.isfinite(ref["floor"]), ref["floor"], 0.0)                 # top_db = inf: no floor, nothing to add
    tol_floor = tol_elem.reshape(B, -1)[np.arange(B), flat][:, None, None] + 2.0 * U * np.abs(fl)[:, None, None]
    both = np.maximum(tol_elem, tol_floor)
    under = ref["floor"][:, None, None] - raw > both
    return np.where(under, tol_floor, both), excl


def _twiddles32():
    i = np.arange(N_FFT // 2)
    ang = -2.0 * i / N_FFT * np.pi
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _bitrev9(i):
    r = np.zeros_like(i)
    for b in range(9):
        r |= ((i >> b) & 1) << (8 - b)
    return r


def _int_max_plain(v):
    """maximum of fp32 values by a plain signed-integer compare of their bits (negatives come out in reversed order)"""
    bits = np.ascontiguousarray(v, np.float32).view(np.int32)
    return bits.reshape(bits.shape[0], -1).max(1).view(np.float32)


def fbank32(wav, window_f32, melmat_f32, hop, top_db=80.0, amin=1e-10, fault=None, power64=None):
    """fbank_kernel restated in fp32 numpy: wav * window, bit-reversed load, 9 radix-2 stages with the 256-entry twiddle table, power,
    the mel sum over k ascending (adding a zero weight's product changes nothing, so the dense loop IS the banded one), log10 in double,
    floor. Returns (out fp32, s fp32). power64: take this power spectrum (rounded to fp32) instead of the FFT's - isolates the mel sum."""
    wav = np.asarray(wav, np.float32)
    window = np.asarray(window_f32, np.float32)
    mel = np.array(melmat_f32, np.float32)
    if fault == "window_shift":
        window = np.roll(window, 1)
    if fault == "band_end":
        for m in range(mel.shape[1]):
            nz = np.nonzero(mel[:, m])[0]
            if len(nz):
                mel[nz[-1], m] = 0
    x = frame_signal(wav, hop, 255 if fault == "origin" else 256) * window      # fp32 product, as the kernel rounds it
    B, T, _ = x.shape
    if power64 is None:
        re = np.zeros((B * T, N_FFT), np.float32)
        im = np.zeros_like(re)
        re[:, _bitrev9(np.arange(N_FFT))] = x.reshape(B * T, N_FFT)
        twc, tws = _twiddles32()
        k = np.arange(N_FFT // 2)
        for st in range(9):
            half = 1 << st
            j = k & (half - 1)
            i0 = ((k >> st) << (st + 1)) + j
            i1 = i0 + half
            wx, wy = twc[j << (8 - st)], tws[j << (8 - st)]
            ax, ay, cx, cy = re[:, i0], im[:, i0], re[:, i1], im[:, i1]
            tx, ty = cx * wx - cy * wy, cx * wy + cy * wx
            re[:, i0], im[:, i0], re[:, i1], im[:, i1] = ax + tx, ay + ty, ax - tx, ay - ty
        pw = (re * re + im * im)[:, :N_FFT // 2 + 1]
    else:
        pw = np.asarray(power64, np.float64).astype(np.float32).reshape(B * T, -1)
    s = np.zeros((B * T, mel.shape[1]), np.float32)
    for kk in range(N_FFT // 2 + 1):
        s += pw[:, kk:kk + 1] * mel[kk][None, :]
    s = s.reshape(B, T, -1)
    raw = (np.float32(10) * np.log10(np.maximum(s, np.float32(amin)).astype(np.float64)).astype(np.float32)).astype(np.float32)
    if fault == "max_T_minus_1":
        umax = raw[:, :T - 1].reshape(B, -1).max(1) if T > 1 else np.full(B, -np.inf, np.float32)
    elif fault == "int_compare":
        umax = _int_max_plain(raw)
    elif fault == "batch_max":
        umax = np.full(B, raw[0].max(), np.float32)
    else:
        umax = raw.reshape(B, -1).max(1)
    out = np.maximum(raw, (umax - np.float32(top_db)).astype(np.float32)[:, None, None])
    return out.astype(np.float32), s


def _noise(seed, B, L, amp=0.1):
    return (_rng(seed).randn(B, L) * amp).astype(np.float32)


def _old_test_wav():
    """the input of test_blocks_gpu.test_fbank_and_sentence_norm_known_answers"""
    import torch
    g = torch.Generator().manual_seed(4)
    wav = torch.randn(3, 16000 + 77, generator=g) * 0.1
    wav[1, 9000:] = 0
    return wav.numpy()


def _levels_wav():
    """three levels in one batch, L = 15999 (the last 63 samples are seen by the last frame alone): loud noise; 1e-6 noise with a 1e-3
    burst in those last samples - its maximum (about -50 dB) is negative, lies in the LAST frame, and with top_db = 40 the floor is
    active on the rest of the row; zeros (exactly -100 dB)"""
    L = 15999
    r = _rng(31)
    w = np.zeros((3, L), np.float32)
    w[0] = r.randn(L) * 0.3
    w[1] = r.randn(L) * 1e-6
    w[1, 15940:] = r.randn(L - 15940) * 1e-3
    return w


def _tone_wav():
    n = np.arange(4000)
    r = _rng(32)
    w = np.stack([0.5 * np.sin(2 * np.pi * 1000.0 * n / 16000.0), 0.5 * np.sin(2 * np.pi * 1000.0 * n / 16000.0 + 1.0)])
    return (w + 1e-4 * r.randn(2, 4000)).astype(np.float32)


def custom_mel(kind):
    """[257,16] fp32, non-negative. "dense": every entry random. "special": random bands of 5..40 rows, with column 3 all zero, column 5
    with zeros inside its band, column 7 non-zero at row 0 only, column 9 non-zero at row 256 only."""
    r = _rng(33)
    if kind == "dense":
        return (r.rand(257, 16) + 0.01).astype(np.float32)
    m = np.zeros((257, 16), np.float32)
    for c in range(16):
        lo, n = r.randint(0, 200), r.randint(5, 41)
        m[lo:lo + n, c] = r.rand(n) + 0.01
    m[:, 3] = 0
    m[:, 5] = 0
    m[40:60, 5] = r.rand(20) + 0.01
    m[45:52, 5] = 0
    m[55, 5] = 0
    m[:, 7] = 0
    m[0, 7] = 0.7
    m[:, 9] = 0
    m[256, 9] = 0.9
    return m


def _fb(wav, n_mels=80, hop=160, top_db=80.0, mel=None):
    return {"wav": wav, "n_mels": n_mels, "hop": hop, "top_db": top_db, "mel": mel}


def fbank_cases():
    """name -> dict(wav [B,L] fp32, n_mels, hop, top_db, mel = custom matrix or None). Noise 0.1 unless said.
    Exclusion share (elements with c u rho > 0.25): 0 in every case, "tone" included - its 1e-4 noise keeps every band's s above
    1e-9 of the frame's energy (the fp32 torch.stft oracle stays inside the model there too, at 0.13 of the tolerance).
    Largest tolerance on "old" (the existing test's input, which allows 3e-3 dB there): 5.1e-4 dB; elsewhere at most 2.7e-4 dB
    except "tone", whose leakage bins reach 2.5e-2 dB."""
    c = {"old": _fb(_old_test_wav()), "base": _fb(_noise(40, 3, 16077))}
    for L in (100, 159, 160, 255, 257, 511, 512, 513, 1125):
        c[f"len{L}"] = _fb(_noise(41 + L, 2, L))
    for n in (1, 23, 40, 64, 65, 128):
        c[f"mels{n}"] = _fb(_noise(42 + n, 2, 1125), n_mels=n)
    for h in (80, 128, 512, 700):
        c[f"hop{h}"] = _fb(_noise(43 + h, 2, 2000), hop=h)
    c["levels"] = _fb(_levels_wav(), top_db=40.0)
    c["topdb_inf"] = _fb(_noise(44, 2, 1125), top_db=float("inf"))
    c["topdb_0"] = _fb(_noise(45, 2, 1125), top_db=0.0)
    c["loud"] = _fb(_noise(46, 2, 1125, 3000.0))
    c["quiet"] = _fb(_noise(47, 2, 1125, 1e-7))
    c["tone"] = _fb(_tone_wav())
    c["mel_dense"] = _fb(_noise(48, 2, 1125), n_mels=16, mel=custom_mel("dense"))
    c["mel_special"] = _fb(_noise(49, 2, 1125), n_mels=16, mel=custom_mel("special"))
    return c


def fbank_case_mel(case):
    return case["mel"] if case["mel"] is not None else mel_matrix(case["n_mels"])


def fbank_check(got, ref, a=FB_A, c=FB_C):
    """(worst |got - out| / tol over the elements kept, share of elements excluded)"""
    tol, excl = fbank_tol(ref, a, c)
    err = np.abs(np.asarray(got, np.float64) - ref["out"])
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / tol)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(np.where(excl, 0.0, ratio).max()), float(excl.mean())


def measure_fbank():
    """(a, c) the fp32 restatement needs over fbank_cases(), unscaled: a from the mel sum of the rounded float64 power spectrum alone,
    c = the e / (u ||x||) that closes the rest of |s32 - s64| in fbank_ds."""
    win = hamming512()
    a_m = c_m = 0.0
    for case in fbank_cases().values():
        mel = fbank_case_mel(case)
        ref = fbank64(case["wav"], win, mel, case["hop"], case["top_db"])
        xw = frame_signal(case["wav"].astype(np.float64), case["hop"]) * win.astype(np.float64)
        sp = np.fft.rfft(xw, axis=-1)
        _, s_a = fbank32(case["wav"], win, mel, case["hop"], power64=sp.real ** 2 + sp.imag ** 2)
        _, s32 = fbank32(case["wav"], win, mel, case["hop"])
        s = ref["s"]
        pos = s > 0
        if pos.any():
            a_m = max(a_m, float((np.abs(s_a - s)[pos] / (U * s[pos])).max()))
        assert np.all(s32[~pos] == 0)
    for case in fbank_cases().values():
        mel = fbank_case_mel(case)
        ref = fbank64(case["wav"], win, mel, case["hop"], case["top_db"])
        _, s32 = fbank32(case["wav"], win, mel, case["hop"])
        s, W, xn = ref["s"], ref["wsum"][None, None, :] + 0 * ref["s"], ref["xn"][..., None] + 0 * ref["s"]
        R = np.maximum(np.abs(s32 - s) - a_m * U * s, 0.0)
        ok = (W > 0) & (xn > 0)
        e = (np.sqrt(W[ok] * s[ok] + W[ok] * R[ok]) - np.sqrt(W[ok] * s[ok])) / W[ok]
        c_m = max(c_m, float((e / (U * xn[ok])).max()))
    return a_m, c_m


# ============================================================================================================= sentence norm
#: measured by measure_norm() over norm_cases() (fp32 restatement: four accumulators per thread row, two passes): k = 1.81; x 4, rounded up:
SN_K = 8.0


def sentence_norm64(x, lens, eps=1e-10):
    """y = (x - mean) / max(std, eps) in float64: n = min(max(lens, 1), T), mean and unbiased std over the first n frames, applied to
    all T frames; n <= 1 gives a NaN row (0 / 0 in the variance, which max() hands on). Returns (y, scale): the tolerance is
    SN_K u scale (+ half a bf16 ulp of |y| for bf16 output), scale = (|x| + max_t |x[:, f]|) / sd + |y| (1 + SN_K u (max_t |x| / sd)^2)
    with sd = max(std, eps): the error of the mean and of x - mean against the deviation, the relative error of the deviation, and
    the second-order share of the mean's error in the sum of squares."""
    x = np.asarray(x, np.float64)
    B, T, F = x.shape
    y = np.empty_like(x)
    scale = np.empty_like(x)
    eps = r32(eps)
    for b in range(B):
        n = min(max(int(lens[b]), 1), T)
        if n <= 1:
            y[b] = np.nan
            scale[b] = np.nan
            continue
        mu = x[b, :n].mean(0)
        sd = np.maximum(x[b, :n].std(0, ddof=1), eps)
        y[b] = (x[b] - mu) / sd
        xmax = np.abs(x[b, :n]).max(0)
        scale[b] = (np.abs(x[b]) + xmax) / sd + np.abs(y[b]) * (1.0 + SN_K * U * (xmax / sd) ** 2)
    return y, scale


def sentence_norm32(x, lens, eps=1e-10, fault=None):
    """sentence_norm_kernel restated in fp32 numpy: rows = 1024 // F thread rows; row r sums frames r, r + rows, ... into four accumulators
    (a 4 x rows unrolled sweep, then a tail into the first), ((s0 + s1) + (s2 + s3)); the rows are added in order; two passes."""
    x = np.asarray(x, np.float32)
    B, T, F = x.shape
    rows = SN_NT // F
    y = np.empty_like(x)
    f0 = np.float32(0)

    def colsum(xb, n, mu):
        tot = np.zeros(F, np.float32)
        for r in range(rows - 1 if fault == "drop_last_row" else rows):
            s = [np.zeros(F, np.float32) for _ in range(4)]
            t = r
            while t + 3 * rows < n:
                for q in range(4):
                    v = xb[t + q * rows]
                    s[q] = s[q] + (v if mu is None else (v - mu) * (v - mu))
                t += 4 * rows
            while t < n:
                v = xb[t]
                s[0] = s[0] + (v if mu is None else (v - mu) * (v - mu))
                t += rows
            tot = tot + ((s[0] + s[1]) + (s[2] + s[3]))
        return tot

    for b in range(B):
        n = min(max(int(lens[b]), 1), T)
        ns = T if fault == "all_frames" else n
        nm = ns - 1 if fault == "mean_n_minus_1" else ns
        mu = colsum(x[b], nm, None) / np.float32(nm) if nm > 0 else np.full(F, np.nan, np.float32)
        with np.errstate(all="ignore"):
            var = colsum(x[b], ns, mu) / np.float32(ns if fault == "biased" else ns - 1)
            sd = np.sqrt(var)
            sd = np.where(sd < np.float32(eps), np.float32(eps), sd)        # NaN compares false and stays
            y[b] = (x[b] - mu) * (np.float32(1) / sd)
    return y + f0


def _sn(x, lens):
    return {"x": x.astype(np.float32), "lens": np.asarray(lens, np.int32)}


def norm_cases():
    """name -> dict(x [B,T,F] fp32, lens [B]); x = -60 + 10 randn (dB-like) unless said, padded frames hold data. F = 80 has rows = 12,
    F = 144 rows = 7 (1024 % 144 != 0: a partial thread row exists and must stay idle). n at 2, 3 and around rows, 4 rows (the unroll
    boundary) and 8 rows + 3, with T = n and T = n + 5; T < rows; lens > T; F = 1, 7, 255, 256; mean 1e4 with std 1."""
    r = _rng(50)
    c = {}

    def db(B, T, F):
        return -60.0 + 10.0 * r.randn(B, T, F)

    for F in (80, 144):
        rows = SN_NT // F
        ns = [2, 3, rows - 1, rows, rows + 1, 4 * rows - 1, 4 * rows, 4 * rows + 1, 8 * rows + 3]
        for pad in (0, 5):
            T = max(ns) + pad
            # one batch per padding: T is shared, so only the longest row has exactly `pad` padded frames; the T = n + pad pairs proper
            # follow as batches of one
            c[f"F{F}_pad{pad}"] = _sn(db(len(ns), T, F), ns)
            for n in ns:
                c[f"F{F}_n{n}_T{n + pad}"] = _sn(db(1, n + pad, F), [n])
    for F in (1, 7, 255, 256):
        c[f"F{F}"] = _sn(db(3, 40, F), [40, 17, 2])
    c["T_lt_rows"] = _sn(db(2, 5, 80), [5, 3])
    c["lens_gt_T"] = _sn(db(2, 30, 80), [45, 31])
    c["mean1e4"] = _sn(1e4 + r.randn(2, 60, 80), [60, 33])
    return c


def norm_check(got, y, scale, k=SN_K, bf16_out=False):
    tol = k * U * scale + (0.5 * bf16_ulp(y) if bf16_out else 0.0)
    err = np.abs(np.asarray(got, np.float64) - y)
    ok = ~np.isnan(y)
    assert np.array_equal(np.isnan(np.asarray(got, np.float64)), ~ok), "NaN rows differ from the reference's"
    with np.errstate(all="ignore"):
        ratio = np.where(err[ok] == 0, 0.0, err[ok] / tol[ok])
    return float(ratio.max()) if ratio.size else 0.0


def measure_norm():
    k = 0.0
    for c in norm_cases().values():
        y, scale = sentence_norm64(c["x"], c["lens"])
        k = max(k, norm_check(sentence_norm32(c["x"], c["lens"]), y, scale, k=1.0))
    return k


# ======================================================================================================= mean pool, lengths
#: measured by measure_pool() over pool_cases() (four time slices added sequentially, ((r0 + r1) + (r2 + r3)) / n): k = 2.44; x 4, rounded up:
MP_K = 10.0


def pool_n(rel, T):
    """frames pooled: max(1, min(ceil(rel * T), T)), the product formed in fp32 as the kernel and torch form it"""
    v = np.asarray(rel, np.float32) * np.float32(T)
    return np.maximum(1, np.minimum(np.ceil(v), T)).astype(np.int64)


def mean_pool64(x, rel, fault=None):
    """(out [B,1,D], scale [B,1,D], n [B]): out = sum_{t < n} x / n in float64, tolerance MP_K u scale with scale = sum |x| / n
    (+ half a bf16 ulp of |out| for bf16 output)."""
    x = np.asarray(x, np.float64)
    B, T, D = x.shape
    n = pool_n(rel, T)
    if fault == "floor":
        n = np.maximum(1, np.minimum(np.floor(np.asarray(rel, np.float32) * np.float32(T)), T)).astype(np.int64)
    out = np.stack([x[b, :n[b]].sum(0) / (T if fault == "div_T" else n[b]) for b in range(B)])[:, None]
    scale = np.stack([np.abs(x[b, :n[b]]).sum(0) / n[b] for b in range(B)])[:, None]
    return out, scale, n


def mean_pool_grad64(dout, rel, T):
    """dx [B,T,D] = dout / n on the pooled frames, exactly 0 after them"""
    dout = np.asarray(dout, np.float64)
    n = pool_n(rel, T)
    live = np.arange(T)[None, :, None] < n[:, None, None]
    return np.where(live, dout / n[:, None, None], 0.0)


def mean_pool32(x, rel, fault=None):
    x = np.asarray(x, np.float32)
    B, T, D = x.shape
    _, _, n = mean_pool64(x, rel, fault)
    out = np.zeros((B, 1, D), np.float32)
    for b in range(B):
        red = []
        for sl in range(4):
            s = np.zeros(D, np.float32)
            for t in range(sl, n[b], 4):
                s = s + x[b, t]
            red.append(s)
        out[b, 0] = ((red[0] + red[1]) + (red[2] + red[3])) / np.float32(T if fault == "div_T" else n[b])
    return out


def pool_cases():
    """name -> dict(x [B,T,D] fp32 (randn + 0.5), rel [B] fp32). rel per row: rel T exactly an integer (k / T for a power-of-two T, else
    the fp32 nearest whose product rounds back to k), one fp32 ulp above it, 1.0, 1.5 (clamped to T), 1e-6 (n = 1).
    T in {1, 3, 4, 5, 37, 260} (one trip or fewer per time slice, ragged against the 4 slices, many trips) x D in {1, 63, 64, 65, 144, 256}
    (D = 64 / 65: one / two channel blocks)."""
    r = _rng(60)
    c = {}
    for T, D in ((T, D) for T in (1, 3, 4, 5, 37, 260) for D in (1, 63, 64, 65, 144, 256)):
        k = max(1, T // 2)
        exact = np.float32(k) / np.float32(T)
        while np.float32(exact * np.float32(T)) > k:
            exact = np.nextafter(exact, np.float32(0))
        while np.float32(exact * np.float32(T)) < k:
            exact = np.nextafter(exact, np.float32(2))
        assert np.float32(exact * np.float32(T)) == k
        above = exact
        while np.float32(above * np.float32(T)) <= k:
            above = np.nextafter(above, np.float32(2))
        rel = np.array([exact, above, 1.0, 1.5, 1e-6], np.float32)
        c[f"T{T}_D{D}"] = {"x": (r.randn(5, T, D) + 0.5).astype(np.float32), "rel": rel, "k": k}
    return c


def measure_pool():
    k = 0.0
    for c in pool_cases().values():
        out, scale, _ = mean_pool64(c["x"], c["rel"])
        k = max(k, float((np.abs(mean_pool32(c["x"], c["rel"]) - out) / (U * scale)).max()))
    return k


def abs_lengths_ref(rel, dim, mode, fault=None):
    """int32 lengths: the product formed in fp32 (as the kernel and torch form it), then mode 0 = rint (half to even), 1 = floor,
    2 = ceil clamped to dim. Integer equality, no tolerance."""
    v = np.asarray(rel, np.float32) * np.float32(dim)
    if mode == 0:
        if fault == "half_away":
            return (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int32)
        return np.rint(v).astype(np.int32)
    if mode == 1:
        return np.floor(v).astype(np.int32)
    return np.minimum(np.ceil(v), dim).astype(np.int32)


def tie_grid(dim, B):
    """B relative lengths on the grid k / (2 dim), kept where the fp32 product rel * dim gives k / 2 back exactly (so that rint meets
    a true tie): first a tie that rounds down to an even integer and one that rounds up to one, then 0 and 1, then random grid points"""
    k = np.arange(2 * dim + 1)
    rel = (k.astype(np.float64) / (2.0 * dim)).astype(np.float32)
    k = k[rel * np.float32(dim) == (k / 2.0).astype(np.float32)]
    ties = k[k % 2 == 1]
    down, up = ties[(ties // 2) % 2 == 0], ties[(ties // 2) % 2 == 1]
    assert len(down) and len(up), dim
    r = _rng(61 + dim + B)
    ks = np.concatenate([[down[len(down) // 2], up[len(up) // 2], 0, 2 * dim], r.choice(k, size=B)])[:B]
    return (ks.astype(np.float64) / (2.0 * dim)).astype(np.float32)


# ================================================================================================================= injection
#: measured by measure_inject() over inject_cases(): dspk's slice sums (64 time slices for fp32, 128 for bf16, added in order): k = 2.73; x 4, rounded up:
INJ_K = 11.0


def inject64(src, spk, dout, mode):
    """Speaker injection out = src (+ | *) spk [B,1,D] and its gradients in float64. a + b and a * b of fp32 values are exact in float64,
    so out and dsrc are compared as fp32(float64 result) bit for bit (bf16 I/O: bf16(fp32(.))). dspk = sum_t term, term = dout (sum) or
    dout * src (prod); its tolerance is INJ_K u sum_t |term| (+ half a bf16 ulp of |dspk| for bf16). Returns out, dsrc, dspk, dspk_scale."""
    src, spk, dout = (np.asarray(a, np.float64) for a in (src, spk, dout))
    if mode == "prod":
        out, dsrc, term = src * spk, dout * spk, dout * src
    else:
        out, dsrc, term = src + spk, dout.copy(), dout
    return out, dsrc, term.sum(1, keepdims=True), np.abs(term).sum(1, keepdims=True)


def inject_dspk32(src, dout, mode, nsl):
    src, dout = np.asarray(src, np.float32), np.asarray(dout, np.float32)
    term = dout * src if mode == "prod" else dout
    B, T, D = term.shape
    tot = np.zeros((B, 1, D), np.float32)
    for sl in range(nsl):
        acc = np.zeros((B, D), np.float32)
        for t in range(sl, T, nsl):
            acc = acc + term[:, t]
        tot[:, 0] = tot[:, 0] + acc
    return tot


INJECT_T = (1, 64, 65, 128, 129, 300)      # one trip per slice or none, the second trip's first frame (fp32 64 / bf16 128 slices), several
INJECT_D = (8, 64, 72, 136)                # one 16-byte piece, one full channel block, blocks with a ragged last one


def inject_case(T, D, seed=70):
    r = _rng(seed + T * 1000 + D)
    return (r.randn(2, T, D).astype(np.float32), r.randn(2, 1, D).astype(np.float32), r.randn(2, T, D).astype(np.float32))


def measure_inject():
    k = 0.0
    for T in INJECT_T:
        for D in INJECT_D:
            src, spk, dout = inject_case(T, D)
            for mode in ("sum", "prod"):
                for nsl, rnd in ((64, lambda a: a), (128, bf16_round)):
                    s, _, d = rnd(src), rnd(spk), rnd(dout)
                    _, _, dspk, scale = inject64(s, spk, d, mode)
                    k = max(k, float((np.abs(inject_dspk32(s, d, mode, nsl) - dspk) / (U * scale)).max()))
    return k


# =============================================================================================================== SpecAugment
#: measured by measure_specaug() over specaug_cases() and specaug_cases(big=True): warped elements k = 11.31 against
#: sum_i (|w_i| + 1) |x_i| (see spec_augment64), fills k = 6.32 against mean |x| (fp32 sums of up to 1.3 M elements, combined in
#: double); x 4, rounded up:
SA_K_WARP, SA_K_FILL = 46.0, 26.0


def sa_table(c, w, flen, fpos, tlen, tpos):
    """int32 draw table in the layout of tsasr_specaug_draw: c, w, flen [B*nf], fpos, tlen [B*nt], tpos"""
    parts = [np.array([c, w])] + [np.asarray(a).reshape(-1) for a in (flen, fpos, tlen, tpos)]
    return np.concatenate(parts).astype(np.int32)


def _sa_split(table, B, nf, nt):
    c, w = int(table[0]), int(table[1])
    o = 2
    out = []
    for n in (nf, nf, nt, nt):
        out.append(np.asarray(table[o:o + B * n]).reshape(B, n))
        o += B * n
    return (c, w, *out)


def _cubic64(t):
    A = -0.75
    t = np.asarray(t, np.float64)
    u = 1.0 - t
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A      # noqa: E731
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1           # noqa: E731
    return far(t + 1), near(t), near(u), far(u + 1)


def _cubic32(t):
    A, one = np.float32(-0.75), np.float32(1)
    t = np.asarray(t, np.float32)
    u = one - t
    far = lambda x: ((A * x - np.float32(5) * A) * x + np.float32(8) * A) * x - np.float32(4) * A      # noqa: E731
    near = lambda x: ((A + np.float32(2)) * x - (A + np.float32(3))) * x * x + one                     # noqa: E731
    return far(t + one), near(t), near(u), far(u + one)


def _warp_plan(T, c, w, whole=False):
    """per output row: the four source rows and the tap parameter t (fp32). The source position src = fp32(fp32(ratio) * d) and t = src - i0
    are part of the operation's definition (the reference forms them in fp32). whole: the planted fault - taps clamped to [0, T)."""
    t_idx = np.arange(T)
    left = t_idx < w
    base = np.where(left, 0, c)
    in_len = np.where(left, c, T - c)
    out_len = np.where(left, w, T - w)
    d = np.where(left, t_idx, t_idx - w)
    with np.errstate(all="ignore"):
        scale = np.where(out_len > 1, (in_len - 1).astype(np.float64) / np.maximum(out_len - 1, 1), 0.0).astype(np.float32)
    src = scale * d.astype(np.float32)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_len - 1)
    tp = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1))
    if whole:
        rows = [np.clip(base + i0 + k, 0, T - 1) for k in (-1, 0, 1, 2)]
    else:
        rows = [base + np.clip(i0 + k, 0, in_len - 1) for k in (-1, 0, 1, 2)]
    return rows, tp


def _mask1d(lens, pos, D, inclusive=False):
    """[B, D] bool: element i masked when some pos <= i < pos + len (inclusive: the planted fault i <= pos + len); and [B, D] int counts"""
    ar = np.arange(D)[None, None, :]
    hit = (pos[:, :, None] <= ar) & ((ar <= (pos + lens)[:, :, None]) if inclusive else (ar < (pos + lens)[:, :, None]))
    return hit.any(1), hit.sum(1)


def spec_augment64(x, table, nf, nt, zero, dtype="fp32"):
    """SpecAugment with the draws of `table`: time warp (two halves resized with align_corners, cubic taps A = -0.75 clamped to their
    half), frequency masks filled with the mean of the warped tensor, time masks filled with the mean of the frequency-masked tensor.
    Taps, the four-term sum, both means and the fills in float64. dtype "bf16" restates the kernel's order of roundings: the warped
    value is stored as bf16, the means are over stored values, fill1 is rounded to bf16 before it enters the second mean.
    Returns dict: y, kind (0 = copied input, 1 = warped, 2 = fill1, 3 = fill2), scale, fill1, fill2. scale of a fill: mean |x|. scale of
    a warped element: sum_i (|w_i| + 1) |x_i|, not sum_i |w_i x_i| alone: the kernel (and the reference) evaluate the tap polynomials
    in fp32, whose intermediate terms reach 6 whatever the tap's own size, so a tap near 0 carries an ABSOLUTE error of a few u. Against
    sum |w_i x_i| the fp32 restatement needs k = 3631 (an element whose heavy tap meets a small x and whose light tap a large one);
    against this scale it needs 11.3, which holds every element tighter than 4 x 3631 would."""
    x = np.asarray(x, np.float64)
    B, T, F = x.shape
    c, w, flen, fpos, tlen, tpos = _sa_split(np.asarray(table), B, nf, nt)
    kind = np.zeros((B, T, F), np.int8)
    if c > 0:
        rows, tp = _warp_plan(T, c, w)
        taps = _cubic64(tp)
        y = sum(taps[k][None, :, None] * x[:, rows[k]] for k in range(4))
        scale = sum((np.abs(taps[k]) + 1.0)[None, :, None] * np.abs(x[:, rows[k]]) for k in range(4))
        kind[:] = 1
        if dtype == "bf16":
            y = bf16_round(y.astype(np.float32)).astype(np.float64)
    else:
        y, scale = x.copy(), np.abs(x)
    mabs = float(np.abs(y).mean())
    fill1 = 0.0 if zero else float(y.mean())
    if dtype == "bf16":
        fill1 = float(bf16_round(np.float32(fill1)).reshape(-1)[0])
    fill2 = fill1
    if nf > 0:
        fm, _ = _mask1d(flen, fpos, F)
        fm = np.broadcast_to(fm[:, None, :], y.shape)
        y = np.where(fm, fill1, y)
        kind[fm] = 2
        scale = np.where(fm, mabs, scale)
        fill2 = 0.0 if zero else float(y.mean())
    if nt > 0:
        tm, _ = _mask1d(tlen, tpos, T)
        tm = np.broadcast_to(tm[:, :, None], y.shape)
        y = np.where(tm, fill2, y)
        kind[tm] = 3
        scale = np.where(tm, mabs, scale)
    return {"y": y, "kind": kind, "scale": scale, "fill1": fill1, "fill2": fill2}


def spec_augment32(x, table, nf, nt, zero, fault=None):
    """the two SpecAugment kernels restated in fp32 numpy: ((w0 x0 + w1 x1) + w2 x2) + w3 x3 with fp32 taps; S, S_masked and n_masked as
    fp32 sums, fill1 = S / N, fill2 = (S - S_masked + n_masked fill1) / N in double as the mask kernel combines them."""
    x = np.asarray(x, np.float32)
    B, T, F = x.shape
    c, w, flen, fpos, tlen, tpos = _sa_split(np.asarray(table), B, nf, nt)
    if c > 0:
        rows, tp = _warp_plan(T, c, w, whole=fault == "clamp_whole")
        k = _cubic32(tp)
        y = ((k[0][None, :, None] * x[:, rows[0]] + k[1][None, :, None] * x[:, rows[1]]) + k[2][None, :, None] * x[:, rows[2]]) \
            + k[3][None, :, None] * x[:, rows[3]]
    else:
        y = x.copy()
    N = float(B * T * F)
    S = float(y.sum(dtype=np.float32))
    fill1 = 0.0 if zero else float(np.float32(S / N))
    fill2 = fill1
    incl = fault == "end_inclusive"
    if nf > 0:
        fm, cnt = _mask1d(flen, fpos, F, incl)
        wgt = cnt if fault == "overlap_twice" else fm
        wgt = np.broadcast_to(wgt[:, None, :].astype(np.float32), y.shape)
        s_fm = float((y * wgt).sum(dtype=np.float32))
        n_fm = float(wgt.sum())
        fill2 = 0.0 if zero else float(np.float32((S - s_fm + n_fm * fill1) / N))
        y = np.where(np.broadcast_to(fm[:, None, :], y.shape), np.float32(fill1), y)
    if fault == "fill2_is_fill1":
        fill2 = fill1
    if nt > 0:
        tm, _ = _mask1d(tlen, tpos, T, incl)
        y = np.where(np.broadcast_to(tm[:, :, None], y.shape), np.float32(fill2), y)
    return y.astype(np.float32)


def specaug_tol(ref, dtype="fp32"):
    """per-element tolerance: copied elements 0 (bit-equal to the input); warped SA_K_WARP u scale, fills SA_K_FILL u mean |x|;
    bf16 adds one bf16 ulp of the reference to both (the fp32 term stays: a warped value that cancels to almost nothing still carries
    the fp32 error of its four products)"""
    kind, scale = ref["kind"], ref["scale"]
    tol = np.where(kind == 1, SA_K_WARP * U * scale, np.where(kind >= 2, SA_K_FILL * U * scale, 0.0))
    if dtype == "bf16":
        tol = np.where(kind >= 1, tol + bf16_ulp(ref["y"]), 0.0)
    return tol


def _draw(B, n, vals):
    return np.array(vals, np.int64).reshape(B, n)


def specaug_cases(big=False):
    """name -> dict(x [B,T,F] fp32 (randn + 0.5, so the fills are well away from 0), table, nf, nt, zero). window = 5.
    F = 80 takes the 4-wide kernels, F = 81 and F = 3 the 1-wide ones. Warps: none; c = window, w = 1 (left half: ONE output row);
    w = c + window with c = T - window - 1 (right half: one output row); w = c (both scales 1). Masks: width 0; ending exactly at F
    and at T; two overlapping; nf = 0 with nt = 2 and the reverse; none at all with a warp (the mask kernel is not launched);
    8 + 8; replace_with_zero. big: the two shapes whose B T F / V exceeds 262144 (the grid-stride loops' second trip)."""
    r = _rng(80)
    c = {}

    def add(name, B, T, F, cw, nf, nt, fl=None, fp=None, tl=None, tp=None, zero=False):
        fl = _draw(B, nf, fl if fl is not None else r.randint(0, min(F, 30), B * nf))
        tl = _draw(B, nt, tl if tl is not None else r.randint(0, min(T // 2, 20), B * nt))
        fp = _draw(B, nf, fp if fp is not None else r.randint(0, max(1, F - int(fl.max(initial=0))), B * nf))
        tp = _draw(B, nt, tp if tp is not None else r.randint(0, max(1, T - int(tl.max(initial=0))), B * nt))
        assert np.all(fp + fl <= F) and np.all(tp + tl <= T) and (cw[0] == 0 or (0 < cw[0] < T and 0 < cw[1] < T))
        c[name] = {"x": (r.randn(B, T, F) + 0.5).astype(np.float32), "table": sa_table(cw[0], cw[1], fl, fp, tl, tp), "nf": nf, "nt": nt,
                   "zero": zero}

    if big:
        add("big_F80", 16, 1000, 80, (400, 403), 2, 2)
        add("big_F81", 4, 900, 81, (300, 297), 2, 2)
        return c
    for F in (80, 81, 3):
        T = 40
        fw = min(F, 30)
        add(f"F{F}_nowarp", 2, T, F, (0, 0), 2, 2)
        add(f"F{F}_left1", 2, T, F, (5, 1), 2, 2)
        add(f"F{F}_right1", 2, T, F, (T - 6, T - 1), 2, 2)
        add(f"F{F}_identity", 2, T, F, (17, 17), 2, 2)
        add(f"F{F}_warp_only", 2, T, F, (20, 23), 0, 0)
        add(f"F{F}_width0", 2, T, F, (20, 18), 2, 2, fl=[0, 0, 0, 2], tl=[0, 3, 0, 0])
        add(f"F{F}_at_end", 2, T, F, (20, 22), 2, 2, fl=[2, 1, 1, 2], fp=[F - 2, 0, F - 1, 0], tl=[7, 2, 3, 4], tp=[T - 7, 3, 1, T - 4])
        add(f"F{F}_overlap", 2, T, F, (0, 0), 2, 2, fl=[2, 2, 1, 2] if F == 3 else [fw - 10, fw - 12, 9, 9], fp=[0, 1, 1, 0] if F == 3 else [5, 9, 30, 34],
            tl=[10, 10, 6, 8], tp=[4, 9, 20, 22])
        add(f"F{F}_time_only", 2, T, F, (20, 19), 0, 2)
        add(f"F{F}_freq_only", 2, T, F, (0, 0), 2, 0)
        add(f"F{F}_eight", 2, T, F, (20, 24), 8, 8, fl=r.randint(0, 3 if F == 3 else 6, 16), tl=r.randint(0, 4, 16))
        add(f"F{F}_zero", 2, T, F, (20, 21), 2, 2, zero=True)
    return c


def specaug_check(got, ref, dtype="fp32"):
    tol = specaug_tol(ref, dtype)
    err = np.abs(np.asarray(got, np.float64) - ref["y"])
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / tol)          # err > 0 against tol 0 (a copied element) gives inf
    return float(ratio.max())


def measure_specaug():
    kw = kf = 0.0
    cases = dict(specaug_cases())
    cases.update(specaug_cases(big=True))
    for c in cases.values():
        ref = spec_augment64(c["x"], c["table"], c["nf"], c["nt"], c["zero"])
        got = spec_augment32(c["x"], c["table"], c["nf"], c["nt"], c["zero"]).astype(np.float64)
        err = np.abs(got - ref["y"])
        for kind in (1, 2, 3):
            sel = (ref["kind"] == kind) & (ref["scale"] > 0)
            if sel.any():
                v = float((err[sel] / (U * ref["scale"][sel])).max())
                if kind == 1:
                    kw = max(kw, v)
                else:
                    kf = max(kf, v)
    return kw, kf


# ================================================================================================================= resample
#: measured by measure_resample() over resample_cases() (taps added left to right in fp32): k = 4.97; x 4, rounded up:
RS_K = 20.0
RESAMPLE_FREQS = (8000, 32000, 15200, 16800, 11025)     # P = 1 (stride 2); upsampling; the recipe's 95 / 105 %; P = 441 phases
RESAMPLE_LENS = (1, 5, 24, 25, 26, 1000, 1003)          # shorter than, equal to and just past the 16 kHz filters' 25 taps; ragged against P


def resample_plan(orig, new):
    base = math.gcd(orig, new)
    return new // base, orig // base      # P, stride


def resample64(x, weights_f32, first, orig, new, n_out):
    """Polyphase resampling with the fp32 filter bank in float64: output n = q P + i is sum_j weights[i][j] x[first[i] + q stride + j],
    zeros outside [0, L). Returns (y, scale = sum_j |w_j x_j|); tolerance RS_K u scale."""
    x = np.asarray(x, np.float64)
    wts = np.asarray(weights_f32, np.float64)
    first = np.asarray(first).astype(np.int64)
    P, stride = resample_plan(orig, new)
    B, L = x.shape
    n = np.arange(n_out)
    pos = (first[n % P] + (n // P) * stride)[:, None] + np.arange(wts.shape[1])[None, :]
    ok = (pos >= 0) & (pos < L)
    terms = np.where(ok[None], x[:, np.clip(pos, 0, L - 1)], 0.0) * wts[n % P][None]
    return terms.sum(-1), np.abs(terms).sum(-1)


def resample32(x, weights_f32, first, orig, new, n_out, fault=None):
    x = np.asarray(x, np.float32)
    wts = np.asarray(weights_f32, np.float32)
    first = np.asarray(first).astype(np.int64) + (1 if fault == "first_plus_1" else 0)
    P, stride = resample_plan(orig, new)
    B, L = x.shape
    n = np.arange(n_out)
    start = first[n % P] + (n // P) * stride
    y = np.zeros((B, n_out), np.float32)
    for j in range(wts.shape[1]):
        pos = start + j
        ok = ((pos >= 0) & (pos < L)) | (fault == "no_zeroing")
        y = y + np.where(ok[None, :], x[:, np.clip(pos, 0, L - 1)] * wts[n % P, j][None, :], np.float32(0))
    return y


def resample_bank(orig, new):
    """(weights [P,W] fp32, first [P] int64) as oracle.resample_filters builds them"""
    from oracle import tsasr_ref as R
    first, wts = R.resample_filters(orig, new)
    return wts.numpy().astype(np.float32), first.numpy().astype(np.int64)


def resample_cases():
    """(new_freq, L) -> x [3, L] fp32 noise 0.1"""
    return {(f, L): _noise(90 + L + f % 97, 3, L) for f in RESAMPLE_FREQS for L in RESAMPLE_LENS}


def measure_resample():
    from oracle import tsasr_ref as R
    k = 0.0
    for (f, L), x in resample_cases().items():
        wts, first = resample_bank(16000, f)
        n_out = R.resample_out_len(L, 16000, f)
        y, scale = resample64(x, wts, first, 16000, f, n_out)
        sel = scale > 0
        k = max(k, float((np.abs(resample32(x, wts, first, 16000, f, n_out) - y)[sel] / (U * scale[sel])).max()))
    return k
