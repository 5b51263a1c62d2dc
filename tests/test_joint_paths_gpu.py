"""Every path of the narrow-vocabulary joint kernels (csrc/rnnt.hip: joint_fwd_kernel<T>, joint_fwd_regw_kernel<40, S01>,
joint_bwd_x_kernel<T>, denc_sum_kernel, joint_bwd_reduce_kernel) and of the exact-fp32 joint (csrc/joint_f32.hip) against float64, cell by
cell, through the C-ABI with `ldl` chosen here. Outputs and workspace are NaN before every call; afterwards every element is finite and
within its own tolerance of the reference that rounds what that kernel rounds. Cases, rounding points and the tolerance model:
tests/helpers/joint_ref.py (whose constants tests/test_joint_ref_cpu.py regenerates and whose planted faults it rejects)."""
import collections
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import joint_ref as JR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRACTIONS = collections.defaultdict(dict)      # path -> output -> worst fraction of its tolerance
PATHS = {}                                     # case -> what the launcher chose for it
SWEEP = {}                                     # scale exponent -> figures of the F16 form
FWD = JR.forward_cases()
BWD = JR.backward_cases()


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module("ts-asr_amd.ops")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(a, io=JR.F32):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(torch.bfloat16) if io == JR.BF16 else t


def nan(shape, io=JR.F32):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.bfloat16 if io == JR.BF16 else torch.float32)


def host(t):
    return t.float().cpu().numpy()


def note(path, out, frac):
    FRACTIONS[path][out] = max(FRACTIONS[path].get(out, 0.0), frac)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_fwd(C, exact, io, enc, dec, W, bias, V, ldl, slope):
    B, T, J = enc.shape
    U1 = dec.shape[1]
    logits = nan((B, T, U1, ldl))
    keep = (dev(enc, io), dev(dec, io), dev(W), dev(bias))
    a = [C.ptr(t) for t in keep] + [C.ptr(logits), B, T, U1, J, V, ldl]
    if exact:
        C.check(C.lib().tsasr_joint_f32_fwd(*a, float(slope), C.stream_ptr()), "tsasr_joint_f32_fwd")
    else:
        C.check(C.lib().tsasr_joint_fwd(*a, io, float(slope), C.stream_ptr()), "tsasr_joint_fwd")
    torch.cuda.synchronize()
    return host(logits)


def check_fwd(name, got, ref, S, rel, V, path):
    assert np.all(np.isfinite(got)), f"{name}: {np.count_nonzero(~np.isfinite(got))} elements of logits[..., :ldl] were not written"
    assert np.all(got[..., V:] == 0), f"{name}: pad columns [V, ldl) must be exactly 0"
    frac = JR.fraction(got, ref, JR.tolerance(ref, S, rel))
    note(path, "logits", frac)
    print(f"fwd {name} [{path}]: logits={frac:.3f} of its tolerance")
    assert frac <= 1.0, f"{name}: logits at {frac:.3g} of the tolerance"


@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_forward(C, case):
    name, io, B, T, U1, J, V, ldl, slope, flavor = case
    kernel, split, lds = JR.fwd_path(io, B, T, U1, J, slope)
    PATHS["fwd/" + name] = f"{kernel} split={split} lds={lds}"
    enc, dec, W, bias = JR.make_inputs("f." + name, io, B, T, U1, J, V, flavor)
    got = run_fwd(C, False, io, enc, dec, W, bias, V, ldl, slope)
    ref, S = JR.forward(JR.forward_kernel_path(case), "rounded", enc, dec, W, bias, slope, V, ldl)
    check_fwd(name, got, ref, S, JR.TOL["fwd/" + name]["logits"], V, kernel)
    if flavor != "big":          # the whole-tensor figures of tests/test_rnnt_gpu.py against the un-rounded joint
        plain, _ = JR.forward("generic", "plain", enc, dec, W, bias, slope, V, ldl)
        assert np.all(np.abs(got - plain) <= 6e-2 + 2e-2 * np.abs(plain)), name


EXACT_FWD = [c for c in FWD if c[1] == JR.F32 and JR.exact_ok(c[5])]


@pytest.mark.parametrize("case", EXACT_FWD, ids=[c[0] for c in EXACT_FWD])
def test_exact_forward(C, case):
    name, io, B, T, U1, J, V, ldl, slope, flavor = case
    enc, dec, W, bias = JR.make_inputs("f." + name, io, B, T, U1, J, V, flavor)
    got = run_fwd(C, True, io, enc, dec, W, bias, V, ldl, slope)
    ref, S = JR.forward("exact", "plain", enc, dec, W, bias, slope, V, ldl)
    check_fwd(name, got, ref, S, JR.TOL["fwd-exact/" + name]["logits"], V, "joint_f32_fwd")


def run_bwd(C, ops, exact, io, dl, enc, dec, W, V, slope, tlen, ulen, deferred):
    lib = C.lib()
    B, T, J = enc.shape
    U1, ldl = dec.shape[1], dl.shape[-1]
    nbytes = int(lib.tsasr_joint_f32_bwd_workspace_bytes(B, U1, J) if exact else lib.tsasr_joint_bwd_workspace_bytes(B, T, U1, J))
    ws = nan(((nbytes + 3) // 4,))
    out = {"denc": nan((B, T, J), io), "ddec": nan((B, U1, J), io), "dW": nan((V, J)), "dbias": nan((V,))}
    i32 = lambda a: None if a is None else torch.tensor(list(a), dtype=torch.int32, device=DEV)  # noqa: E731
    tl, ul = i32(tlen), i32(ulen)
    keep = (dev(dl), dev(enc, io), dev(dec, io), dev(W))
    a = [C.ptr(t) for t in keep] + [C.ptr(out[k]) for k in ("denc", "ddec", "dW", "dbias")] + [C.ptr(tl), C.ptr(ul), B, T, U1, J, V, ldl]
    try:
        if deferred:
            ops.reduce_defer_prepare(torch.device(DEV))
            C.check(lib.tsasr_reduce_defer(1), "tsasr_reduce_defer")
        if exact:
            C.check(lib.tsasr_joint_f32_bwd(*a, float(slope), C.ptr(ws), nbytes, C.stream_ptr()), "tsasr_joint_f32_bwd")
        else:
            C.check(lib.tsasr_joint_bwd(*a, io, float(slope), C.ptr(ws), nbytes, C.stream_ptr()), "tsasr_joint_bwd")
        if deferred:
            torch.cuda.synchronize()
            assert lib.tsasr_reduce_pending() == 2 and torch.isnan(out["dW"]).all(), "the head gradients were reduced before the flush"
            ops._reduce_flush("tsasr_reduce_flush")
            torch.cuda.synchronize()
            C.check(lib.tsasr_reduce_defer(0), "tsasr_reduce_defer")
        torch.cuda.synchronize()
    finally:
        if deferred:
            ops.discard_queues()
    return {k: host(v) for k, v in out.items()}


def check_bwd(name, got, ref, S, flip, rel, store, path, asserted=True):
    fr = {}
    for k in ("denc", "ddec", "dW", "dbias"):
        assert np.all(np.isfinite(got[k])), f"{name}: {np.count_nonzero(~np.isfinite(got[k]))} elements of {k} were not written"
        fr[k] = JR.fraction(got[k], ref[k], JR.tolerance(ref[k], S[k], rel[k], flip.get(k), store and k in ("denc", "ddec")))
        if asserted:
            note(path, k, fr[k])
    print(f"bwd {name} [{path}]: " + " ".join(f"{k}={v:.3f}" for k, v in fr.items()) + ("" if asserted else "  (recorded, not asserted)"))
    if asserted:
        assert max(fr.values()) <= 1.0, f"{name}: " + " ".join(f"{k} at {v:.3g} of its tolerance" for k, v in fr.items() if v > 1.0)
    return fr


def l2(a, b):
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a))


BWD_IO = [(c, io) for c in BWD for io in (JR.F32, JR.BF16)]


@pytest.mark.parametrize("case,io", BWD_IO, ids=[f"{c[0]}-{'f32' if io == JR.F32 else 'bf16'}" for c, io in BWD_IO])
def test_backward(C, ops, case, io):
    name, B, T, U1, J, V, ldl, slope, tlen, ulen, flavor, scale = case
    TS, ksplit, empty = JR.bwd_path(B, T, U1, J, cus())
    path, ios = ("bwd32", "f32") if io == JR.F32 else ("bwd16", "bf16")
    form = "joint_bwd_x_kernel<float>" if io == JR.F32 else "joint_bwd_x_kernel<bf16>"
    PATHS[f"bwd/{name}/{ios}"] = f"{form} TS={TS} ksplit={ksplit} empty-slots={empty} ldl={'32 pipelined' if ldl == 32 else f'{ldl} plain'}"
    enc, dec, W, dl = JR.backward_inputs(case, io)
    ref, S, flip = JR.backward(path, "rounded", dl, enc, dec, W, slope, V, tlen, ulen)
    rel = JR.TOL[f"bwd/{name}/{ios}"]
    e = int(round(-np.log2(scale)))
    asserted = scale == 1.0 or e in JR.SCALES_ASSERTED
    first = run_bwd(C, ops, False, io, dl, enc, dec, W, V, slope, tlen, ulen, deferred=False)
    fr = check_bwd(name + "/joint_bwd_reduce_kernel", first, ref, S, flip, rel, io == JR.BF16, form, asserted)
    again = run_bwd(C, ops, False, io, dl, enc, dec, W, V, slope, tlen, ulen, deferred=False)
    for k in first:
        assert np.array_equal(bits(first[k]), bits(again[k])), f"{name}: two runs differ in {k}"
    queued = run_bwd(C, ops, False, io, dl, enc, dec, W, V, slope, tlen, ulen, deferred=True)
    check_bwd(name + "/tsasr_reduce_flush", queued, ref, S, flip, rel, io == JR.BF16, form, asserted)
    for k in ("denc", "ddec"):
        assert np.array_equal(bits(first[k]), bits(queued[k])), f"{name}: {k} depends on the reduction route"
    plain, _, _ = JR.backward(path, "plain", dl, enc, dec, W, slope, V, tlen, ulen)
    if scale == 1.0:             # the whole-tensor figures of tests/test_rnnt_gpu.py against the un-rounded joint
        for k in ("denc", "ddec", "dW"):
            assert l2(first[k], plain[k]) < (6e-3 if io == JR.F32 else 1.2e-2), (name, k, l2(first[k], plain[k]))
    if name.startswith("scale-") and io == JR.BF16:
        SWEEP[e] = {"kernel": {k: l2(first[k], plain[k]) for k in ("denc", "ddec", "dW")},
                    "model": {k: l2(JR.bf16(ref[k].astype(np.float32)) if k != "dW" else ref[k], plain[k]) for k in ("denc", "ddec", "dW")},
                    "fraction": max(fr.values())}


EXACT_BWD = [c for c in BWD if JR.exact_ok(c[4])]


@pytest.mark.parametrize("case", EXACT_BWD, ids=[c[0] for c in EXACT_BWD])
def test_exact_backward(C, ops, case):
    name, B, T, U1, J, V, ldl, slope, tlen, ulen, flavor, scale = case
    enc, dec, W, dl = JR.backward_inputs(case, JR.F32)
    ref, S, _ = JR.backward("exact", "plain", dl, enc, dec, W, slope, V, tlen, ulen)
    first = run_bwd(C, ops, True, JR.F32, dl, enc, dec, W, V, slope, tlen, ulen, deferred=False)
    check_bwd(name, first, ref, S, {}, JR.TOL["bwd-exact/" + name], False, "joint_f32_bwd")
    again = run_bwd(C, ops, True, JR.F32, dl, enc, dec, W, V, slope, tlen, ulen, deferred=False)
    for k in first:
        assert np.array_equal(bits(first[k]), bits(again[k])), f"{name}: two runs differ in {k}"


def test_tables_reach_every_path():
    """By the mirror of the launchers at this device's compute-unit count: a table that no longer reaches a path fails here."""
    f = [JR.fwd_path(c[1], c[2], c[3], c[4], c[5], c[8]) for c in FWD]
    assert {p[0] for p in f} == {"joint_fwd_kernel<float>", "joint_fwd_kernel<bf16>", "regw<40,true>", "regw<40,false>"}
    assert {p[1] for p in f} >= {1, 2, 4}
    for k in ("joint_fwd_kernel<float>", "joint_fwd_kernel<bf16>"):
        assert {p[2] > 65536 for p in f if p[0] == k} == {True, False}
    b = [JR.bwd_path(c[1], c[2], c[3], c[4], cus()) for c in BWD]
    assert {p[0] for p in b} == {1, 2, 3, 4}, f"frame splits reached with {cus()} compute units: {sorted({p[0] for p in b})}"
    assert {p[1] for p in b} == {1, 2} and any(p[2] > 0 for p in b if p[1] == 2)
    assert {c[6] == 32 for c in BWD} == {True, False}


def test_zz_fractions_of_tolerance():
    """Prints the path table, the worst fraction of its tolerance per path and output, and the gradient-scale sweep of the F16 form
    (profiles/joint_paths_notes.md quotes them). Every fraction was asserted where it was measured; nothing is asserted here."""
    for k, v in PATHS.items():
        print(f"path[{k}]: {v}")
    for path, fr in FRACTIONS.items():
        print(f"fractions[{path}]: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(fr.items())))
    for e, d in sorted(SWEEP.items()):
        print(f"sweep[2^-{e}]: fraction of tolerance against rounded {d['fraction']:.3f}; relative L2 against plain, kernel / CPU model: "
              + " ".join(f"{k} {d['kernel'][k]:.2e} / {d['model'][k]:.2e}" for k in ("denc", "ddec", "dW")))
