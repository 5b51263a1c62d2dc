"""The feature and augmentation kernels against float64, path by path: log-mel filterbank and sentence normalisation (csrc/features.hip),
SpecAugment and resampling (csrc/augment.hip), mean-pool, length rounding and speaker injection (csrc/misc.hip). References, tolerance
models and case matrices: tests/helpers/feats_ref.py (checked on the CPU by test_feats_ref_cpu.py, planted faults included). Every test
prints its worst error as a fraction of the tolerance; the module prints the worst per family at its end."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from oracle import tsasr_ref as R
from tests.helpers import feats_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst error / tolerance per family:", {k: round(v, 3) for k, v in sorted(WORST.items())})


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    return ratio


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("ts-asr_amd.ops")


@pytest.fixture(scope="module")
def nn_():
    return importlib.import_module("ts-asr_amd.nnet")


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    t = t.detach().contiguous().cpu()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


# =========================================================================================================================== fbank
WIN = FR.hamming512()
FB_CASES = FR.fbank_cases()
_fb_ref = {}


def fb_ref(name):
    if name not in _fb_ref:
        c = FB_CASES[name]
        _fb_ref[name] = FR.fbank64(c["wav"], WIN, FR.fbank_case_mel(c), c["hop"], c["top_db"])
    return _fb_ref[name]


def run_fbank(ops, c, out_dtype=torch.float32):
    return ops.fbank(dev(c["wav"]), dev(WIN), dev(FR.fbank_case_mel(c)), 512, c["hop"], 512, c["top_db"], 1e-10, out_dtype=out_dtype)


@pytest.mark.parametrize("name", list(FB_CASES))
def test_fbank_vs_float64(ops, name):
    c, ref = FB_CASES[name], fb_ref(name)
    got = host(run_fbank(ops, c))
    assert got.shape == ref["out"].shape
    worst, excl = FR.fbank_check(got, ref)
    print(f"fbank {name}: {worst:.3f} of the tolerance, {100 * excl:.3f} % excluded")
    note("fbank", worst)
    assert worst <= 1.0 and excl <= FR.FB_EXCL_CAP
    if name == "levels":
        assert np.all(got[2] == -100.0)                                  # the zero row, untouched by its neighbours' floors
        assert got[1].max() < 0 and np.mean(got[1] == got[1].min()) > 0.5     # negative maximum with its floor active
        assert abs(float(got[1].min()) - (float(got[1].max()) - 40.0)) <= 1e-5
    if name == "quiet":
        assert np.all(got == -100.0)
    if name == "topdb_0":
        assert all(np.all(got[b] == got[b].max()) for b in range(got.shape[0]))
    if name == "loud":
        assert got.max() > 100.0


def test_fbank_rejects_129_filters(ops, C):
    with pytest.raises(C.TsasrHipError):
        ops.fbank(dev(FR._noise(1, 1, 1125)), dev(WIN), torch.rand(257, 129, device=DEV), 512, 160, 512, 80.0, 1e-10)


def test_fbank_bf16_batch_position_and_repeat_give_the_same_bits(ops):
    c = FB_CASES["levels"]
    f32 = run_fbank(ops, c)
    assert np.array_equal(bits(run_fbank(ops, c, torch.bfloat16)), bits(f32.to(torch.bfloat16)))
    assert np.array_equal(bits(run_fbank(ops, c)), bits(f32))
    for row in range(3):
        alone = run_fbank(ops, dict(c, wav=c["wav"][row:row + 1]))
        batch = np.stack([FR._noise(5, 1, c["wav"].shape[1])[0] * 2.0, c["wav"][0], c["wav"][row], c["wav"][2], c["wav"][1]])
        assert np.array_equal(bits(run_fbank(ops, dict(c, wav=batch))[2]), bits(alone[0])), row


def test_fbank_c_abi_dirty_workspace_guards_and_short_workspace(ops, C):
    lib = C.lib()
    c = FB_CASES["mels23"]
    wav, mel, win = dev(c["wav"]), dev(FR.fbank_case_mel(c)), dev(WIN)
    B, L = c["wav"].shape
    T, M = 1 + L // 160, 23
    nbytes = lib.tsasr_fbank_workspace_bytes(B, T, M)
    pieces = [B * T * M * 4, B * 4, 2 * M * 4]
    assert nbytes == sum((p + 255) // 256 * 256 for p in pieces)
    ws = torch.full((nbytes + 256,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((B * T * M + 64,), float("nan"), device=DEV)
    guard_bits = bits(out[B * T * M:]).copy()

    def call(n):
        return lib.tsasr_fbank_fwd(C.ptr(wav), C.ptr(win), C.ptr(mel), C.ptr(out), B, L, T, M, 160, 80.0, 1e-10, C.io_dtype(out), C.ptr(ws), n,
                                   C.stream_ptr())

    C.check(call(nbytes), "tsasr_fbank_fwd")
    torch.cuda.synchronize()
    assert np.array_equal(bits(out[:B * T * M].view(B, T, M)), bits(run_fbank(ops, c)))          # stale workspace contents change nothing
    assert np.array_equal(bits(out[B * T * M:]), guard_bits)
    w, o = ws.cpu().numpy(), 0
    for p in pieces:
        end = o + (p + 255) // 256 * 256
        assert p < end - o and np.all(w[o + p:end] == 0xFF), p                                    # the words after each piece
        o = end
    assert np.all(w[nbytes:] == 0xFF)
    with pytest.raises(C.TsasrHipError):
        C.check(call(nbytes - 1), "tsasr_fbank_fwd")


# =================================================================================================================== sentence norm
SN_CASES = FR.norm_cases()


@pytest.mark.parametrize("name", list(SN_CASES))
def test_sentence_norm_vs_float64(ops, name):
    c = SN_CASES[name]
    y, scale = FR.sentence_norm64(c["x"], c["lens"])
    got = host(ops.sentence_norm(dev(c["x"]), dev(c["lens"]), 1e-10))
    worst = note("sentence_norm", FR.norm_check(got, y, scale))
    print(f"sentence_norm {name}: {worst:.3f} of the tolerance")
    assert worst <= 1.0


def test_sentence_norm_rejects_257_bins_and_silence_is_zero(ops, C):
    with pytest.raises(C.TsasrHipError):
        ops.sentence_norm(torch.zeros(1, 4, 257, device=DEV), torch.tensor([4], dtype=torch.int32, device=DEV), 1e-10)
    got = host(ops.sentence_norm(torch.full((2, 30, 80), -100.0, device=DEV), torch.tensor([30, 11], dtype=torch.int32, device=DEV), 1e-10))
    assert np.all(got == 0.0)                                            # no NaN, no Inf: 0 / eps


@pytest.mark.parametrize("tin,tout", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16),
                                      (torch.bfloat16, torch.float32)])
def test_sentence_norm_dtype_pairs(ops, tin, tout):
    c = SN_CASES["F80_pad5"]
    x = FR.bf16_round(c["x"]) if tin == torch.bfloat16 else c["x"]              # the reference reads what the kernel reads
    y, scale = FR.sentence_norm64(x, c["lens"])
    got = ops.sentence_norm(dev(x, tin), dev(c["lens"]), 1e-10, out_dtype=tout)
    assert got.dtype == tout
    worst = note("sentence_norm" + (" bf16 out" if tout == torch.bfloat16 else ""), FR.norm_check(host(got), y, scale, bf16_out=tout == torch.bfloat16))
    print(f"sentence_norm {tin} -> {tout}: {worst:.3f} of the tolerance")
    assert worst <= 1.0


def test_sentence_norm_one_frame_gives_a_nan_row(ops):
    """lens <= 1: the unbiased deviation of one frame is 0 / 0; the reference's max(std, eps) hands the NaN on, and so must the kernel.
    The other rows of the batch are unaffected."""
    x = SN_CASES["F80_pad5"]["x"][:4]
    lens = np.array([1, 9, 0, 30], np.int32)
    y, scale = FR.sentence_norm64(x, lens)
    got = host(ops.sentence_norm(dev(x), dev(lens), 1e-10))
    assert np.isnan(y[0]).all() and np.isnan(y[2]).all()
    assert np.isnan(got[0]).all() and np.isnan(got[2]).all(), (got[0, :2, :4], got[2, :2, :4])
    assert note("sentence_norm", FR.norm_check(got, y, scale)) <= 1.0


def test_input_normalization_rounds_half_to_even(nn_):
    norm = nn_.InputNormalization(norm_type="sentence")
    r = FR._rng(55)
    for T, n in ((5, 2), (7, 4)):                                          # 0.5 * 5 = 2.5 -> 2, 0.5 * 7 = 3.5 -> 4
        x = (-60.0 + 10.0 * r.randn(2, T, 80)).astype(np.float32)
        rel = np.array([0.5, 1.0], np.float32)
        assert FR.abs_lengths_ref(rel, T, 0).tolist() == [n, T]
        y, scale = FR.sentence_norm64(x, [n, T])
        assert note("sentence_norm", FR.norm_check(host(norm(dev(x), dev(rel))), y, scale)) <= 1.0


# ======================================================================================================================= mean pool
MP_CASES = FR.pool_cases()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(MP_CASES))
def test_mean_pool_vs_float64(ops, name, dtype):
    c = MP_CASES[name]
    bf = dtype == torch.bfloat16
    x = FR.bf16_round(c["x"]) if bf else c["x"]
    B, T, D = x.shape
    dout = FR._rng(66).randn(B, 1, D).astype(np.float32)
    dout = FR.bf16_round(dout) if bf else dout
    out, scale, n = FR.mean_pool64(x, c["rel"])
    xd = dev(x, dtype).requires_grad_()
    got = ops.mean_pool(xd, dev(c["rel"]))
    got.backward(dev(dout, dtype))
    tol = FR.MP_K * FR.U * scale + (0.5 * FR.bf16_ulp(out) if bf else 0.0)
    fam = "mean_pool bf16" if bf else "mean_pool"
    worst = note(fam, (np.abs(host(got) - out) / tol).max())
    print(f"mean_pool {name} {dtype}: {worst:.3f} of the tolerance, n = {n.tolist()}")
    assert got.shape == (B, 1, D) and worst <= 1.0
    dx, ref = host(xd.grad), FR.mean_pool_grad64(dout, c["rel"], T)
    for b in range(B):
        assert np.all(bits(xd.grad[b, n[b]:]) == 0), b                  # exactly +0 after the pooled frames
    # dout / n: one correctly rounded fp32 division (exact in float64 up to its own rounding); an ulp is allowed for the device's divide.
    # bf16: the stored value is that quotient rounded once more
    gtol = 2.0 * FR.U * np.abs(ref) + (0.5 * FR.bf16_ulp(ref) if bf else 0.0)
    assert np.all(np.abs(dx - ref) <= gtol)
    note(fam + " grad", (np.abs(dx - ref)[ref != 0] / gtol[ref != 0]).max())


# ========================================================================================================================= lengths
def _len_jobs(B):
    r = FR._rng(67 + B)
    dims = [7, 50, 1000, 8, 333, 50, 1000, 64]
    modes = [0, 1, 2, 0, 2, 0, 1, 0]
    rels = [FR.tie_grid(d, B) for d in dims]
    rels[2] = np.concatenate([rels[2][:B // 2], (r.rand(B - B // 2) * 1.2).astype(np.float32)])      # mode 2: values past 1 are clamped
    return dims, modes, rels


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1024])
def test_abs_lengths_eight_jobs_in_one_launch(C, B):
    dims, modes, rels = _len_jobs(B)
    rel_d = [dev(r) for r in rels]
    out_d = [torch.full((B + 8,), -7, dtype=torch.int32, device=DEV) for _ in range(8)]
    pr, po = (ctypes.c_void_p * 8)(*[t.data_ptr() for t in rel_d]), (ctypes.c_void_p * 8)(*[t.data_ptr() for t in out_d])
    pd, pm = (ctypes.c_int * 8)(*dims), (ctypes.c_int * 8)(*modes)
    C.check(C.lib().tsasr_abs_lengths(pr, po, pd, pm, 8, B, C.stream_ptr()), "tsasr_abs_lengths")
    torch.cuda.synchronize()
    for k in range(8):
        got = out_d[k].cpu().numpy()
        assert np.array_equal(got[:B], FR.abs_lengths_ref(rels[k], dims[k], modes[k])), (k, dims[k], modes[k])
        assert np.all(got[B:] == -7)
    if B >= 2:
        v = rels[0] * np.float32(dims[0])
        assert set(np.floor(v[v - np.floor(v) == 0.5]) % 2) == {0.0, 1.0}                             # ties to even and to odd were there


def test_abs_lengths_limits_and_cache_key(ops, C):
    rel = torch.rand(1025, device=DEV)
    out = torch.zeros(1025, dtype=torch.int32, device=DEV)
    pr, po = (ctypes.c_void_p * 9)(*[rel.data_ptr()] * 9), (ctypes.c_void_p * 9)(*[out.data_ptr()] * 9)
    pd, pm = (ctypes.c_int * 9)(*[10] * 9), (ctypes.c_int * 9)(*[0] * 9)
    with pytest.raises(C.TsasrHipError):
        C.check(C.lib().tsasr_abs_lengths(pr, po, pd, pm, 1, 1025, C.stream_ptr()), "tsasr_abs_lengths")
    with pytest.raises(C.TsasrHipError):
        C.check(C.lib().tsasr_abs_lengths(pr, po, pd, pm, 9, 4, C.stream_ptr()), "tsasr_abs_lengths")
    r = dev(np.array([0.25, 0.5, 1.0], np.float32))
    assert ops.abs_lengths(r, 10).tolist() == [2, 5, 10]
    r.mul_(0.5)                                                                    # same storage, new version
    assert ops.abs_lengths(r, 10).tolist() == [1, 2, 5]


# ======================================================================================================================= injection
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", ["sum", "prod"])
def test_inject_vs_float64_element_wise(ops, mode, dtype):
    bf = dtype == torch.bfloat16
    rnd = FR.bf16_round if bf else (lambda a: a)
    for T in FR.INJECT_T:
        for D in FR.INJECT_D:
            src, spk, dout = (rnd(a) for a in FR.inject_case(T, D))
            out, dsrc, dspk, scale = FR.inject64(src, spk, dout, mode)
            s, k = dev(src, dtype).requires_grad_(), dev(spk, dtype).requires_grad_()
            assert ops.inject_ok(s, k)
            o = ops.inject(s, k, mode)
            o.backward(dev(dout, dtype))
            assert np.array_equal(host(o), rnd(out.astype(np.float32))), (T, D)              # bit for bit
            assert np.array_equal(host(s.grad), rnd(dsrc.astype(np.float32))), (T, D)
            tol = FR.INJ_K * FR.U * scale + (0.5 * FR.bf16_ulp(dspk) if bf else 0.0)
            worst = note("inject dspk bf16" if bf else "inject dspk", (np.abs(host(k.grad) - dspk) / tol).max())
            assert k.grad.shape == (2, 1, D) and worst <= 1.0, (T, D, worst)
    print(f"inject {mode} {dtype}: dspk at most {WORST['inject dspk bf16' if bf else 'inject dspk']:.3f} of the tolerance so far")


# ===================================================================================================================== SpecAugment
SA_CASES = FR.specaug_cases()


def run_specaug(ops, c, dtype):
    bf = dtype == torch.bfloat16
    x = FR.bf16_round(c["x"]) if bf else c["x"]
    ref = FR.spec_augment64(x, c["table"], c["nf"], c["nt"], c["zero"], dtype="bf16" if bf else "fp32")
    xd = dev(x, dtype)
    y = ops.spec_augment_apply(xd, dev(c["table"]), c["nf"], c["nt"], c["zero"])
    assert y.dtype == dtype and np.array_equal(host(xd), x)                           # the input is left untouched
    got = host(y)
    same = ref["kind"] == 0
    assert np.array_equal(got[same], x[same])                                             # neither warped nor masked: the input's bits
    return FR.specaug_check(got, ref, "bf16" if bf else "fp32"), ref


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(SA_CASES))
def test_spec_augment_vs_float64(ops, name, dtype):
    worst, ref = run_specaug(ops, SA_CASES[name], dtype)
    print(f"spec_augment {name} {dtype}: {worst:.3f} of the tolerance, kinds {np.bincount(ref['kind'].reshape(-1), minlength=4).tolist()}")
    note("spec_augment bf16" if dtype == torch.bfloat16 else "spec_augment", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["big_F80", "big_F81"])
def test_spec_augment_grid_stride_second_trip(ops, name, dtype):
    c = FR.specaug_cases(big=True)[name]
    B, T, F = c["x"].shape
    assert B * T * (F // (4 if F % 4 == 0 else 1)) > 262144
    worst, _ = run_specaug(ops, c, dtype)
    print(f"spec_augment {name} {dtype}: {worst:.3f} of the tolerance")
    note("spec_augment bf16" if dtype == torch.bfloat16 else "spec_augment", worst)
    assert worst <= 1.0


# ======================================================================================================================== resample
@pytest.mark.parametrize("new", FR.RESAMPLE_FREQS)
def test_resample_vs_float64(ops, nn_, new):
    rs = nn_.Resample(16000, new)
    cases = FR.resample_cases()
    for L in FR.RESAMPLE_LENS:
        x = cases[(new, L)]
        got = rs(dev(x))
        n_out = R.resample_out_len(L, 16000, new)
        assert got.shape == (3, n_out) and ops.resample_out_len(L, 16000, new) == n_out
        y, scale = FR.resample64(x, rs.weights.numpy(), rs.first_indices.numpy(), 16000, new, n_out)
        err = np.abs(host(got) - y)
        assert np.all(err[scale == 0] == 0)
        worst = note("resample", (err[scale > 0] / (FR.RS_K * FR.U * scale[scale > 0])).max()) if (scale > 0).any() else 0.0
        assert worst <= 1.0, (new, L, worst)
    print(f"resample 16000 -> {new}: at most {WORST['resample']:.3f} of the tolerance so far")
