"""The Conformer convolution core (csrc/convmod.hip, convmod_stream_kernel of csrc/stream.hip), path by path through the C-ABI, stage by stage
against float64 (tests/helpers/convmod_ref.py).

    pair f32     glu_dwconv_{fwd,bwd}_kernel<float, K> + tsasr_layernorm_{fwd,bwd}     io fp32, any D
    pair bf16    glu_dwconv_{fwd,bwd}_kernel<bf16, K> + tsasr_layernorm_{fwd,bwd}      io bf16 with D != 256, or D = 256 under TSASR_CONVMOD_FUSED=0
    fused bf16   convmod_{fwd,bwd}_fused_kernel<K>                                      io bf16, D = 256
    stream       convmod_stream_kernel<T>, forward only                                 tsasr_convmod_stream_fwd

Every training case: inputs seeded per case and clear of the LeakyReLU kink (convmod_ref.case_inputs), B >= 2 with utterances of different
data lengths; the dispatch rule mirrored by expected_path() and asserted against what the backward left in its workspace (the one-launch
kernel fills exactly B ceil(T / 32) D (K + 5) floats from the start; the pair fills its B ceil(T / 64) D (K + 3) slab and stores dc behind
it); z, c_save, dy2, mean, rstd start as NaN and carry two guard rows of a sentinel; the workspace is exactly
tsasr_convmod_bwd_workspace_bytes long with a sentinel block behind it, and it and dparams are 0xFF before the launch, so a slab column that no
workgroup writes surfaces as NaN in a parameter gradient; the backward must leave the forward's outputs bit for bit. Then check_conv,
check_ln, check_bwd: every stage from the kernel's own state, element-wise, deltas from convmod_ref.TOL, at most 1 % of any bf16 output other
than the nearest bf16 of its reference."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import convmod_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SENT, NAN, GUARD = -7.0, float("nan"), 0xA5
FLIPS = CR.TOL["flips"]
DELTA = {io: {k: v[0] for k, v in CR.TOL[io].items()} for io in ("f32", "bf16")}


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


def cdiv(a, b):
    return -(-a // b)


def align256(n):
    return cdiv(n, 256) * 256


# ------------------------------------------------------------------------------------------------------ the host's dispatch rule (csrc/convmod.hip)
def expected_path(io, D, env):
    """convmod_fused(): the one-launch kernels for bf16 rows of 256 channels unless TSASR_CONVMOD_FUSED starts with '0' (read per call)"""
    if (env is None or env[:1] != "0") and io == "bf16" and D == 256:
        return "fused bf16"
    return f"pair {io}"


def require_path(path, D, monkeypatch):
    io = CR.io_of(path)
    env = "0" if (path == "pair bf16" and D == 256) else None
    if env is None:
        monkeypatch.delenv("TSASR_CONVMOD_FUSED", raising=False)
    else:
        monkeypatch.setenv("TSASR_CONVMOD_FUSED", env)
    assert expected_path(io, D, env) == path, (path, D)
    return io


def observed_path(ws, io, B, T, D, K):
    """what the backward wrote into a workspace of 0xFF (no fp32 or bf16 pair that a kernel stores is all ones: that is a NaN)"""
    w = (ws.view(torch.int32) != -1).cpu()
    nF = B * cdiv(T, 32) * D * (K + 5)
    if bool(w[:nF].all()) and not bool(w[nF:].any()):
        return "fused bf16"
    nS = B * cdiv(T, 64) * D * (K + 3)
    off = align256(nS * 4) // 4
    ndc = B * T * D * (2 if io == "bf16" else 4) // 4
    if bool(w[:nS].all()) and not bool(w[nS:off].any()) and bool(w[off:off + ndc].all()):
        return f"pair {io}"
    return "neither"


# ------------------------------------------------------------------------------------------------------ one case
def guarded(rows, tail, dtype, fill=NAN):
    t = torch.full((rows + 2, *tail), SENT, dtype=dtype, device=DEV)
    t[:rows] = fill
    return t


def same_bits(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == BF16 else a.view(torch.int32), b.view(torch.int16) if b.dtype == BF16 else b.view(torch.int32))


class Case:
    def __init__(self, C, path, io, inp, B, T, D):
        self.C, self.lib, self.path, self.io, self.inp, self.B, self.T, self.D, self.K = C, C.lib(), path, io, inp, B, T, D, inp["K"]
        self.iod, self.dt = (C.BF16, BF16) if io == "bf16" else (C.F32, F32)
        dev = lambda t, dt=F32: None if t is None else t.to(dt).contiguous().to(DEV)  # noqa: E731
        self.y2, self.dz = dev(inp["y2"], self.dt), dev(inp["dz"], self.dt)
        self.b2, self.cw, self.cb, self.gamma, self.beta = (dev(inp[k]) for k in ("b2", "cw", "cb", "gamma", "beta"))
        M, K = B * T, self.K
        self.z, self.c_save, self.dy2 = guarded(M, (D,), self.dt), guarded(M, (D,), self.dt), guarded(M, (2 * D,), self.dt)
        self.mean, self.rstd = guarded(M, (), F32), guarded(M, (), F32)
        self.npar = D * (K + 5)
        self.dpar = torch.full((self.npar + 8,), SENT, dtype=F32, device=DEV)
        self.nb = int(self.lib.tsasr_convmod_bwd_workspace_bytes(B, T, D, K))
        self.ws = torch.empty(self.nb + 256, dtype=torch.uint8, device=DEV)
        self.what = f"{path} {CR.case_key(B, T, D, K, inp['causal'], inp['b2'] is not None, inp['slope'])}"

    def fwd(self, K=None, D=None):
        p, i = self.C.ptr, self.inp
        return self.lib.tsasr_convmod_fwd(p(self.y2), p(self.b2), p(self.cw), p(self.cb), p(self.gamma), p(self.beta), p(self.z), p(self.c_save), p(self.mean),
                                          p(self.rstd), self.B, self.T, self.D if D is None else D, self.K if K is None else K, int(i["causal"]), CR.EPS,
                                          float(i["slope"]), self.iod, self.C.stream_ptr())

    def bwd(self, K=None, D=None, nbytes=None):
        p, i = self.C.ptr, self.inp
        self.ws[:self.nb] = 0xFF
        self.ws[self.nb:] = GUARD
        self.dpar[:self.npar].view(torch.uint8).fill_(0xFF)
        return self.lib.tsasr_convmod_bwd(p(self.dz), p(self.y2), p(self.b2), p(self.cw), p(self.gamma), p(self.beta), p(self.c_save), p(self.mean), p(self.rstd),
                                          p(self.dy2), p(self.dpar), self.B, self.T, self.D if D is None else D, self.K if K is None else K, int(i["causal"]),
                                          float(i["slope"]), self.iod, p(self.ws), self.nb if nbytes is None else nbytes, self.C.stream_ptr())

    def guards(self, name):
        M = self.B * self.T
        for k in ("z", "c_save", "dy2", "mean", "rstd"):
            assert bool((getattr(self, k)[M:] == SENT).all()), f"{self.what} {name}: guard rows of {k} were written"
        assert bool((self.dpar[self.npar:] == SENT).all()), f"{self.what} {name}: the words behind dparams were written"

    def written(self, name, keys):
        M = self.B * self.T
        for k in keys:
            t = self.dpar[:self.npar] if k == "dparams" else getattr(self, k)[:M]
            n = int(torch.isnan(t.float()).sum())
            assert n == 0, f"{self.what} {name}: {n} NaN left in {k}"

    def untouched(self, name, keys):
        M = self.B * self.T
        for k in keys:
            if k == "dparams":
                assert bool((self.dpar[:self.npar].view(torch.int32) == -1).all()), f"{self.what} {name}: dparams were written"
            elif k == "workspace":
                assert bool((self.ws[:self.nb] == 0xFF).all()), f"{self.what} {name}: the workspace was written"
            else:
                assert bool(torch.isnan(getattr(self, k)[:M].float()).all()), f"{self.what} {name}: {k} was written"

    def run(self):
        """forward, stage checks, backward on the forward's outputs, stage check -> statistics"""
        C, M, tile = self.C, self.B * self.T, CR.TILE[self.path.split()[0]]
        C.check(self.fwd(), "tsasr_convmod_fwd")
        torch.cuda.synchronize()
        self.guards("fwd")
        self.written("fwd", ("z", "c_save", "mean", "rstd"))
        self.untouched("fwd", ("dy2",))
        sh = (self.B, self.T, self.D)
        c_k, z_k, mean_k, rstd_k = self.c_save[:M].cpu().view(sh), self.z[:M].cpu().view(sh), self.mean[:M].cpu(), self.rstd[:M].cpu()
        d = DELTA[self.io]
        st = CR.check_conv(self.inp, self.io, c_k, d, tile, self.what + " fwd")
        st.update(CR.check_ln(self.inp, self.io, c_k, mean_k, rstd_k, z_k, d, tile, self.what + " fwd"))
        kept = [t.clone() for t in (self.z, self.c_save, self.mean, self.rstd)]
        C.check(self.bwd(), "tsasr_convmod_bwd")
        torch.cuda.synchronize()
        self.guards("bwd")
        assert bool((self.ws[self.nb:] == GUARD).all()), f"{self.what} bwd: bytes behind the workspace's {self.nb} were written"
        self.written("bwd", ("dy2", "dparams"))
        assert all(same_bits(a, b) for a, b in zip(kept, (self.z, self.c_save, self.mean, self.rstd))), f"{self.what}: the backward changed a forward output"
        ran = observed_path(self.ws[:self.nb], self.io, self.B, self.T, self.D, self.K)
        assert ran == self.path, f"{self.what}: the workspace shows {ran}"
        st.update(CR.check_bwd(self.inp, self.io, c_k, mean_k, rstd_k, self.dy2[:M].cpu().view(self.B, self.T, 2 * self.D), self.dpar[:self.npar].cpu(), d, tile,
                               self.what + " bwd"))
        print(f"\nCONVSTAT {self.path} | " + " ".join(f"{k} {v:.3e}" for k, v in st.items()) + f" | {self.what}")
        if self.io == "bf16":
            for k in ("c_flips", "z_flips", "dy2_flips", "dy2_over"):
                assert st[k] <= FLIPS, f"{self.what}: {st[k]:.3%} of {k.split('_')[0]} is not the nearest bf16 of the reference"
        if self.inp["slope"] >= 0:
            assert st["min_abs_y"] >= CR.KINK_MARGIN / 2, f"{self.what}: a pre-activation of the kernel's own state lies {st['min_abs_y']:.2e} from the kink"
        return st


def make_case(C, monkeypatch, path, B, T, D, K, causal, bias, slope):
    io = require_path(path, D, monkeypatch)
    inp, n = CR.case_inputs(B, T, D, K, causal, bias, slope)
    assert n >= CR.SEEDS.get(CR.case_key(B, T, D, K, causal, bias, slope), 0)
    if slope >= 0:
        assert CR.min_abs_y(inp) >= CR.KINK_MARGIN
    return Case(C, path, io, inp, B, T, D)


def cases(group):
    return [pytest.param(*c[1:], id=f"{c[1].replace(' ', '-')}-{CR.case_key(*c[2:])}") for c in CR.matrix() if c[0] == group]


# ------------------------------------------------------------------------------------------------------ the training paths
@pytest.mark.parametrize("path,B,T,D,K,causal,bias,slope", cases("kpb"))
def test_kernel_size_padding_bias(C, monkeypatch, path, B, T, D, K, causal, bias, slope):
    """K in {31, 15, 7, 3} x centred / causal x b2 given / NULL on every path; T = 100 = 64 + 36 = 3 x 32 + 4 (a ragged last tile at both tile
    sizes), three utterances"""
    make_case(C, monkeypatch, path, B, T, D, K, causal, bias, slope).run()


@pytest.mark.parametrize("path,B,T,D,K,causal,bias,slope", cases("time"))
def test_time_edges(C, monkeypatch, path, B, T, D, K, causal, bias, slope):
    """T in {1, 2, K / 2, K - 1, K, 31, 32, 33, 63, 64, 65, 129}: shorter than the padding, than the filter, one frame either side of both
    tile sizes, a third 64-frame tile of one frame"""
    make_case(C, monkeypatch, path, B, T, D, K, causal, bias, slope).run()


@pytest.mark.parametrize("path,B,T,D,K,causal,bias,slope", cases("chan"))
def test_channel_edges(C, monkeypatch, path, B, T, D, K, causal, bias, slope):
    """D in {8, 72, 144, 256 (pair, under the switch for bf16), 264, 520, 1032, 2048}: one clamped 8-channel chunk, 64 + 8, the ABI's limit;
    every step of the LayerNorm dispatch underneath (fp32: 128 / 256 / 512 / 1024 and the wide kernels at 2048; bf16: 256 / 512 / 1024)"""
    make_case(C, monkeypatch, path, B, T, D, K, causal, bias, slope).run()


@pytest.mark.parametrize("path,B,T,D,K,causal,bias,slope", cases("act"))
def test_activation(C, monkeypatch, path, B, T, D, K, causal, bias, slope):
    """slope 0.01, 0 (ReLU: the mask is the whole gradient) and -1 (no activation, in both directions); gamma has both signs in every case"""
    c = make_case(C, monkeypatch, path, B, T, D, K, causal, bias, slope)
    assert bool((c.inp["gamma"] > 0).any()) and bool((c.inp["gamma"] < 0).any())
    c.run()


# ------------------------------------------------------------------------------------------------------ rejections
@pytest.mark.parametrize("path,D", [("pair f32", 72), ("fused bf16", 256)])
def test_rejections_write_nothing(C, monkeypatch, path, D):
    """K = 5, D = 12, D = 2056 and a workspace one byte short return the error and leave every output as it was"""
    B, T, K = 2, 33, 7
    c = make_case(C, monkeypatch, path, B, T, D, K, 0, 1, 0.01)
    outs = ("z", "c_save", "mean", "rstd", "dy2")
    for kw in ({"K": 5}, {"D": 12}, {"D": 2056}):
        assert c.fwd(**kw) != 0, kw
        torch.cuda.synchronize()
        c.untouched(f"fwd {kw}", outs)
    C.check(c.fwd(), "tsasr_convmod_fwd")
    torch.cuda.synchronize()
    for kw in ({"K": 5}, {"D": 12}, {"D": 2056}, {"nbytes": c.nb - 1}):
        assert c.bwd(**kw) != 0, kw
        torch.cuda.synchronize()
        c.untouched(f"bwd {kw}", ("dy2", "dparams", "workspace"))
        c.guards(f"bwd {kw}")
    assert b"workspace too small" in c.lib.tsasr_last_error()


# ------------------------------------------------------------------------------------------------------ streaming
def stream_id(v):
    return f"K{v[0]}-D{v[1]}-chunks{'.'.join(map(str, v[2]))}"


STREAM_CASES = [(*v, 0.01) for v in CR.STREAM] + CR.STREAM_ACT


@pytest.mark.parametrize("io", ["f32", "bf16"])
@pytest.mark.parametrize("K,D,chunks,slope", STREAM_CASES, ids=[stream_id(v) + f"-s{v[3]:g}" for v in STREAM_CASES])
def test_stream(C, io, K, D, chunks, slope):
    """tsasr_convmod_stream_fwd over T = 50 frames from a zero history, the two history buffers swapped per chunk as nnet.py does: chunks of
    1 (every history row but one carried), below, at (30) and above K - 1, a small K under a long chunk, D = 8 and 2048, a mixed chunk list;
    slope 0.01, and once each 0 and -1 (no activation, as in tsasr_convmod_fwd). The output history starts as NaN before every launch and
    both buffers carry guard rows."""
    B, T = 2, CR.STREAM_T
    iod, dt = (C.BF16, BF16) if io == "bf16" else (C.F32, F32)
    inp = CR.stream_inputs(K, D, B, T, slope)
    lib, p = C.lib(), C.ptr
    par = [None if inp[k] is None else inp[k].to(DEV) for k in ("b2", "cw", "cb", "gamma", "beta")]
    y2 = inp["y2"].to(dt).to(DEV)
    hist = [guarded(B * (K - 1), (D,), F32, 0.0), guarded(B * (K - 1), (D,), F32)]
    zs, hs = [], []
    for t0, cn in CR.stream_chunks(T, chunks):
        chunk = y2[:, t0:t0 + cn].contiguous()
        z = guarded(B * cn, (D,), dt)
        hist[1][:B * (K - 1)] = NAN
        C.check(lib.tsasr_convmod_stream_fwd(p(chunk), *(p(t) for t in par), p(hist[0]), p(hist[1]), p(z), B, cn, D, K, CR.EPS, float(slope), iod, C.stream_ptr()),
                "tsasr_convmod_stream_fwd")
        torch.cuda.synchronize()
        assert bool((z[B * cn:] == SENT).all()) and all(bool((h[B * (K - 1):] == SENT).all()) for h in hist), f"guard rows written at frame {t0}"
        assert not bool(torch.isnan(z[:B * cn].float()).any()) and not bool(torch.isnan(hist[1][:B * (K - 1)]).any()), f"NaN left at frame {t0}"
        zs.append(z[:B * cn].cpu().view(B, cn, D))
        hs.append(hist[1][:B * (K - 1)].cpu().view(B, K - 1, D))
        hist = hist[::-1]
    st = CR.check_stream(inp, io, chunks, zs, hs, DELTA[io], f"stream {io} K={K} D={D} chunks={chunks}")
    print(f"\nCONVSTAT stream {io} | " + " ".join(f"{k} {v:.3e}" for k, v in st.items()) + f" | K={K} D={D} chunks={chunks} slope={slope:g}")


def test_stream_rejects_one_history_buffer(C):
    B, cn, D, K = 2, 5, 72, 7
    inp = CR.stream_inputs(K, D, B, cn)
    lib, p = C.lib(), C.ptr
    par = [inp[k].to(DEV) for k in ("b2", "cw", "cb", "gamma", "beta")]
    y2, z, hist = inp["y2"].to(DEV), guarded(B * cn, (D,), F32), guarded(B * (K - 1), (D,), F32)
    assert lib.tsasr_convmod_stream_fwd(p(y2), *(p(t) for t in par), p(hist), p(hist), p(z), B, cn, D, K, CR.EPS, 0.01, C.F32, C.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(z[:B * cn]).all()) and bool(torch.isnan(hist[:B * (K - 1)]).all())
    assert bool((z[B * cn:] == SENT).all()) and bool((hist[B * (K - 1):] == SENT).all())


# ------------------------------------------------------------------------------------------------------ ops level
@pytest.mark.parametrize("bias", [1, 0], ids=["b2", "nob2"])
@pytest.mark.parametrize("path,B,T,D,K,causal", CR.OPS, ids=[o[0].replace(" ", "-") for o in CR.OPS])
def test_ops_convmod_core_rows_vs_model(C, monkeypatch, path, B, T, D, K, causal, bias):
    """ops.convmod_core with a non-contiguous y2, with b2 and with b2 = None: z and dy2 per (b, t) row, the parameter gradients per channel
    (dconv_w per channel and per tap) by relative L2 against the free-running float64 model with the kernels' rounding points (bounds:
    convmod_ref.TOL["ops"]) - the slices of the packed dparams reach the right parameters, three of which have the same length D."""
    ops = importlib.import_module("ts-asr_amd.ops")
    io = require_path(path, D, monkeypatch)
    dt = BF16 if io == "bf16" else F32
    inp = CR.ops_inputs(path, B, T, D, K, causal, bias)
    ref = CR.model(inp, io)
    wide = torch.zeros(B, T, 2 * D + 8, dtype=dt, device=DEV)
    wide[..., :2 * D] = inp["y2"].to(dt).to(DEV)
    y2 = wide[..., :2 * D].detach().requires_grad_()
    assert not y2.is_contiguous()
    leaf = lambda t: None if t is None else t.to(DEV).requires_grad_()  # noqa: E731
    b2, cw, cb, gamma, beta = leaf(inp["b2"]), leaf(inp["cw"].view(D, 1, K)), leaf(inp["cb"]), leaf(inp["gamma"]), leaf(inp["beta"])
    z = ops.convmod_core(y2, b2, cw, cb, gamma, beta, bool(causal), CR.EPS, 0.01)
    assert z.dtype == dt and "_ConvModCoreFn" in type(z.grad_fn).__name__
    z.backward(inp["dz"].to(dt).to(DEV))
    torch.cuda.synchronize()
    got = {"z": z.detach(), "dy2": y2.grad, "dgamma": gamma.grad, "dbeta": beta.grad, "dconv_b": cb.grad, "dconv_w": cw.grad.view(D, K)}
    if bias:
        got["db2"] = b2.grad
    assert all(v is not None for v in got.values())
    what = f"ops {path} {CR.case_key(B, T, D, K, causal, bias, 0.01)}"
    worst = {k: float(CR.row_errors(k, got[k.split("/")[0]].float().cpu(), ref[k.split("/")[0]]).max()) for k in CR.ops_keys(got)}
    print(f"\nCONVSTAT ops {path} | " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f" | {what}")
    for k in CR.ops_keys(got):
        CR.check_rows(k, got[k.split("/")[0]].float().cpu(), ref[k.split("/")[0]], CR.TOL["ops"][path][k][0], what)
