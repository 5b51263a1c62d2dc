"""The row kernels of csrc/elementwise.hip, template instantiation by instantiation through the C-ABI, stage by stage against float64
(tests/helpers/rowkern_ref.py):

    ln      tsasr_layernorm_fwd + tsasr_layernorm_bwd / tsasr_layernorm_bwd_add     layernorm_{fwd,bwd}_kernel<T, 32|64, 1|2|4>, _wide_kernel<T, 2|3|4|6|8>
    aln     tsasr_add_layernorm_{fwd,bwd}                                            add_layernorm_{fwd,bwd}_kernel<T, ITERS, half-wave>
    aln2    tsasr_add_layernorm2_{fwd,bwd}                                           add_layernorm2_{fwd,bwd}_kernel<T, ITERS, half-wave>
    bad     tsasr_bias_act_dropout_{fwd,bwd}         da / da2    tsasr_dropout_add{,2}_{fwd,bwd}         colsum    tsasr_colsum

One test per path (rowkern_ref.matrix() groups the cases by the kernel the mirror of the dispatch expects). Every case: outputs and saved
statistics start as NaN and carry two guard rows of a sentinel; the workspace is exactly *_workspace_bytes() long, 0xFF, with a sentinel block
behind it; parameter gradients are 0xFF before the launch; the backward must leave the forward's outputs and every input bit for bit; exactly
nwg k D floats of the workspace are written (k = 2, 3, 5 for the LN family, nwg N for the bias-gradient producers), which checks rows_per_wg
and the wide kernel's widened rows per workgroup against the mirror. Then rowkern_ref.check_case: every stage from the kernel's own state,
deltas from rowkern_ref.TOL, at most 1 % of any bf16 output other than the nearest bf16 of its reference, dropped and time-masked elements
exact. The numpy port of the dropout mask is confirmed first against tsasr_bias_act_dropout_fwd of all ones."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rowkern_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
SENT, NAN, GUARD = -7.0, float("nan"), 0xA5
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


def guarded(rows, tail, dtype, fill=NAN):
    t = torch.full((rows + 2, *tail), SENT, dtype=dtype, device=DEV)
    t[:rows] = fill
    return t


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32) if t.dtype in (F32, torch.int32) else t.view(torch.int64)


# ------------------------------------------------------------------------------------------------------ the mask port, confirmed first
MASK_SEEDS = [(0x1234567, 0, 0.1), (R.BIG_SEED, 0, 0.1), (R.BIG_SEED, R.DEV_SEED, 0.1), ((0x1234567 + 77) & M64, 0, 0.2), ((R.BIG_SEED + 77) & M64, 0, 0.2),
              ((0x1234567 + 77) & M64, R.DEV_SEED, 0.2)]


@pytest.fixture(scope="module")
def mask_port(C):
    """tsasr_bias_act_dropout_fwd of all ones (fp32, no bias, no activation) IS keep x 65536 / (65536 - thr): the only ground truth the
    port has. 16401 x 64 elements: every element index the matrix uses."""
    lib, p = C.lib(), C.ptr
    M, N = 16401, 64
    x = torch.ones(M, N, dtype=F32, device=DEV)
    for seed, dev, prob in MASK_SEEDS:
        y = torch.full((M, N), NAN, dtype=F32, device=DEV)
        sd = torch.tensor([dev - (1 << 64) if dev >= (1 << 63) else dev], dtype=torch.int64, device=DEV) if dev else None
        C.check(lib.tsasr_bias_act_dropout_fwd(p(x), None, p(y), M, N, -1.0, prob, seed, p(sd), C.F32, C.stream_ptr()), "tsasr_bias_act_dropout_fwd")
        torch.cuda.synchronize()
        want = R.keep_mask(M * N, seed, prob, dev).view(M, N).float() * R.drop_scale16(R.drop_thr16(prob))
        bad = torch.nonzero(y.cpu() != want)
        assert len(bad) == 0, (f"THE NUMPY PORT of the dropout mask (rowkern_ref.keep_mask), not a kernel, is in question: seed {seed:#x} + device seed {dev:#x}, "
                               f"p = {prob}: {len(bad)} of {M * N} elements of dropout(ones) differ, first at element {int(bad[0][0]) * N + int(bad[0][1])}: kernel "
                               f"{float(y[tuple(bad[0])])!r}, port {float(want[tuple(bad[0])])!r}")
    return True


# ------------------------------------------------------------------------------------------------------ one case
class Run:
    def __init__(self, C, c):
        self.C, self.lib, self.c = C, C.lib(), c
        self.inp, n = R.case_inputs(c)
        assert n == R.SEEDS.get(c["key"], 0)
        self.io, self.M, self.D, self.fam = c["io"], c["M"], c["D"], c["fam"]
        self.iod, self.dt = (C.BF16, BF16) if self.io == "bf16" else (C.F32, F32)
        self.paths = R.case_paths(c)
        self.what = c["key"]
        self.dev = {}
        for k, v in self.inp.items():
            if isinstance(v, torch.Tensor) and k not in ("keep", "keep2", "live", "out0"):
                self.dev[k] = v.to(F32 if k in ("gamma", "beta", "gamma2", "beta2", "bias") else self.dt).contiguous().to(DEV)
        self.vl = torch.tensor(R.valid_lens(self.M)[1], dtype=torch.int32, device=DEV) if c["vl"] else None
        self.trows = self.M // R.VL_B if c["vl"] else 0
        sd = c["seed_dev"]
        self.seed_dev = torch.tensor([sd - (1 << 64) if sd >= (1 << 63) else sd], dtype=torch.int64, device=DEV) if sd else None
        self.out, self.par = {}, {}
        self.kind = {"ln": "ln", "aln": "aln", "aln2": "aln2", "colsum": "colsum"}.get(self.fam, "bad")
        self.nb = R.workspace_bytes(self.kind, self.M, self.D)
        self.ws = torch.empty(self.nb + 256, dtype=torch.uint8, device=DEV)

    # -- buffers
    def d(self, k):
        return self.C.ptr(self.dev.get(k))

    def new_out(self, *names, scalar=False):
        for k in names:
            self.out[k] = guarded(self.M, () if scalar else (self.D,), F32 if scalar else self.dt)

    def new_par(self, *names):
        for k in names:
            t = torch.full((self.D + 8,), SENT, dtype=F32, device=DEV)
            t[:self.D].view(torch.uint8).fill_(0xFF)
            self.par[k] = None if k in self.c["nulls"] else t

    def o(self, k):
        return self.C.ptr(self.out.get(k))

    def g(self, k):
        return self.C.ptr(self.par.get(k))

    def arm_workspace(self):
        self.ws[:self.nb] = 0xFF
        self.ws[self.nb:] = GUARD

    def snapshot(self, outs=()):
        return {k: v.clone() for k, v in list(self.dev.items()) + [(o, self.out[o]) for o in outs] + ([("valid_lens", self.vl)] if self.vl is not None else [])
                + ([("seed_dev", self.seed_dev)] if self.seed_dev is not None else [])}

    def unchanged(self, snap, stage):
        cur = dict(self.dev, **self.out, valid_lens=self.vl, seed_dev=self.seed_dev)
        for k, v in snap.items():
            assert torch.equal(bits(v), bits(cur[k])), f"{self.what} {stage}: {k} was changed"

    def guards(self, stage):
        for k, v in self.out.items():
            assert bool((v[self.M:] == SENT).all()), f"{self.what} {stage}: guard rows of {k} were written"
        for k, v in self.par.items():
            assert v is None or bool((v[self.D:] == SENT).all()), f"{self.what} {stage}: the words behind {k} were written"
        assert bool((self.ws[self.nb:] == GUARD).all()), f"{self.what} {stage}: bytes behind the workspace's {self.nb} were written"

    def written(self, stage, names):
        for k in names:
            t = self.out[k][:self.M] if k in self.out else self.par[k][:self.D]
            n = int(torch.isnan(t.float()).sum())
            assert n == 0, f"{self.what} {stage}: {n} NaN left in {k}"

    def untouched(self, stage, names=None):
        for k in (names or list(self.out) + list(self.par) + ["workspace"]):
            if k == "workspace":
                assert bool((self.ws[:self.nb] == 0xFF).all()), f"{self.what} {stage}: the workspace was written"
            elif k in self.out:
                assert bool(torch.isnan(self.out[k][:self.M].float()).all()), f"{self.what} {stage}: {k} was written"
            elif self.par.get(k) is not None:
                assert bool((self.par[k][:self.D].view(torch.int32) == -1).all()), f"{self.what} {stage}: {k} was written"

    def slab(self, k, n=None):
        """exactly nwg k D floats of the 0xFF workspace were written, from the start (no fp32 a kernel stores is all ones: that is a NaN)"""
        nwg = R.n_workgroups(self.kind, self.io, self.M, self.D)
        n = nwg * k * self.D if n is None else n
        w = (self.ws[:self.nb].view(torch.int32) != -1).cpu()
        first_hole = int(torch.nonzero(~w[:n])[0]) if not bool(w[:n].all()) else None
        assert first_hole is None, (f"{self.what}: float {first_hole} of the partial slab (workgroup {first_hole // (k * self.D)}, slab row {first_hole // self.D % k}, "
                                    f"column {first_hole % self.D}) was not written; the mirror expects {nwg} workgroups x {k} x {self.D}")
        assert not bool(w[n:].any()), (f"{self.what}: the workspace was written at float {n + int(torch.nonzero(w[n:])[0])}, behind the {nwg} x {k} x {self.D} floats "
                                       f"the mirror expects")

    def host(self):
        k = {n: v[:self.M].cpu() for n, v in self.out.items()}
        k.update({n: (None if v is None else v[:self.D].cpu()) for n, v in self.par.items()})
        return k

    # -- the launches
    def tail_args(self):
        c = self.c
        return [c["alpha"], c["p"], c["seed"], self.C.ptr(self.seed_dev), self.C.ptr(self.vl), self.trows]

    def fwd(self, D=None, M=None):
        c, lib, D, M, st = self.c, self.lib, self.D if D is None else D, self.M if M is None else M, self.C.stream_ptr()
        if self.fam == "ln":
            return lib.tsasr_layernorm_fwd(self.d("x"), self.d("gamma"), self.d("beta"), self.o("y"), self.o("mean"), self.o("rstd"), M, D, c["eps"], c["slope"],
                                           self.iod, st)
        if self.fam == "aln":
            return lib.tsasr_add_layernorm_fwd(self.d("x"), self.d("bias"), self.d("res"), self.o("s"), self.o("y"), self.o("mean"), self.o("rstd"), self.d("gamma"),
                                               self.d("beta"), M, D, *self.tail_args(), c["eps"], self.iod, st)
        if self.fam == "aln2":
            return lib.tsasr_add_layernorm2_fwd(self.d("x"), self.d("bias"), self.d("res"), self.o("s"), self.o("y"), self.o("z"), self.o("mean"), self.o("rstd"),
                                                self.o("mean2"), self.o("rstd2"), self.d("gamma"), self.d("beta"), self.d("gamma2"), self.d("beta2"), M, D,
                                                *self.tail_args(), c["eps"], c["eps2"], self.iod, st)
        if self.fam == "bad":
            return lib.tsasr_bias_act_dropout_fwd(self.d("x"), self.d("bias"), self.o("y"), M, D, c["slope"], c["p"], c["seed"], self.C.ptr(self.seed_dev), self.iod, st)
        if self.fam == "da":
            return lib.tsasr_dropout_add_fwd(self.d("x"), self.d("bias"), self.d("res"), self.o("out"), M, D, *self.tail_args(), self.iod, st)
        return lib.tsasr_dropout_add2_fwd(self.d("x"), self.d("bias"), self.d("res"), self.o("out"), M, D, c["alpha"], c["p"], c["seed"], c["p2"],
                                          (c["seed"] + 77) & M64, self.C.ptr(self.seed_dev), self.C.ptr(self.vl), self.trows, self.iod, st)

    def bwd(self, D=None, M=None, nbytes=None, dres=True, force_dadd=False):
        c, lib, D, M, st = self.c, self.lib, self.D if D is None else D, self.M if M is None else M, self.C.stream_ptr()
        self.arm_workspace()
        ws = [self.C.ptr(self.ws), self.nb if nbytes is None else nbytes, st]
        if self.fam == "ln":
            a = [self.d("x"), self.d("gamma"), self.d("beta"), self.o("mean"), self.o("rstd"), self.o("dx"), self.g("dgamma"), self.g("dbeta"), M, D, c["slope"], self.iod]
            if c["dadd"] or force_dadd:
                return lib.tsasr_layernorm_bwd_add(self.d("dy"), self.d("dadd") if c["dadd"] else self.d("dy"), *a, *ws)
            return lib.tsasr_layernorm_bwd(self.d("dy"), *a, *ws)
        if self.fam == "aln":
            return lib.tsasr_add_layernorm_bwd(self.d("dy"), self.d("dout"), self.o("s"), self.d("gamma"), self.o("mean"), self.o("rstd"), self.o("dres"), self.o("dx"),
                                               self.g("dgamma"), self.g("dbeta"), self.g("dbias"), M, D, *self.tail_args(), self.iod, *ws)
        if self.fam == "aln2":
            return lib.tsasr_add_layernorm2_bwd(self.d("dz"), self.d("dy"), self.d("dout"), self.o("s"), self.d("gamma"), self.d("beta"), self.d("gamma2"),
                                                self.o("mean"), self.o("rstd"), self.o("mean2"), self.o("rstd2"), self.o("dres"), self.o("dx"), self.g("dgamma"),
                                                self.g("dbeta"), self.g("dbias"), self.g("dgamma2"), self.g("dbeta2"), M, D, *self.tail_args(), self.iod, *ws)
        if self.fam == "bad":
            return lib.tsasr_bias_act_dropout_bwd(self.d("dy"), self.o("y"), self.o("dx"), self.g("dbias"), M, D, c["slope"], c["p"], c["seed"],
                                                  self.C.ptr(self.seed_dev), self.iod, *ws)
        if self.fam == "da":
            return lib.tsasr_dropout_add_bwd(self.d("dy"), self.o("dx"), self.g("dbias"), M, D, *self.tail_args(), self.iod, *ws)
        return lib.tsasr_dropout_add2_bwd(self.d("dy"), self.o("dx"), self.o("dres") if dres else None, self.g("dbias"), M, D, c["alpha"], c["p"], c["seed"], c["p2"],
                                          (c["seed"] + 77) & M64, self.C.ptr(self.seed_dev), self.C.ptr(self.vl), self.trows, self.iod, *ws)

    FWD_OUT = {"ln": ("y",), "aln": ("s", "y"), "aln2": ("s", "y", "z"), "bad": ("y",), "da": ("out",), "da2": ("out",)}
    FWD_STAT = {"ln": ("mean", "rstd"), "aln": ("mean", "rstd"), "aln2": ("mean", "rstd", "mean2", "rstd2")}
    BWD_OUT = {"ln": ("dx",), "aln": ("dres", "dx"), "aln2": ("dres", "dx"), "bad": ("dx",), "da": ("dx",), "da2": ("dx", "dres")}
    PARAMS = {"ln": ("dgamma", "dbeta"), "aln": ("dgamma", "dbeta", "dbias"), "aln2": ("dgamma", "dbeta", "dbias", "dgamma2", "dbeta2"), "bad": ("dbias",),
              "da": ("dbias",), "da2": ("dbias",)}

    def alloc(self):
        f = self.fam
        self.new_out(*self.FWD_OUT[f], *self.BWD_OUT[f])
        self.new_out(*self.FWD_STAT.get(f, ()), scalar=True)
        self.new_par(*self.PARAMS[f])
        if not self.c["bias"] and "dbias" in self.par:
            self.par["dbias"] = None if f in ("bad", "da", "da2") else self.par["dbias"]      # no bias: the slab kernels run without a partial slab
        self.arm_workspace()

    def run(self):
        f, fo, bo = self.fam, self.FWD_OUT[self.fam] + self.FWD_STAT.get(self.fam, ()), self.BWD_OUT[self.fam]
        if f == "da2" and self.c["p2"] <= 0:
            bo = ("dx",)
        self.alloc()
        snap = self.snapshot()
        self.C.check(self.fwd(), "forward of " + self.what)
        torch.cuda.synchronize()
        self.guards("fwd")
        self.written("fwd", fo)
        self.untouched("fwd", [k for k in list(self.out) + list(self.par) + ["workspace"] if k not in fo])
        self.unchanged(snap, "fwd")
        snap = self.snapshot(fo)
        self.C.check(self.bwd(), "backward of " + self.what)
        torch.cuda.synchronize()
        self.guards("bwd")
        self.written("bwd", bo + tuple(k for k, v in self.par.items() if v is not None))
        self.unchanged(snap, "bwd")
        if f in ("ln", "aln", "aln2"):
            self.slab(R.PART_K[f])
        else:
            self.slab(1, None if self.par["dbias"] is not None else 0)
        k = self.host()
        if f == "da2" and self.c["p2"] <= 0:
            assert bool(torch.isnan(k.pop("dres").float()).all()), f"{self.what}: dres written without an outer dropout"
        st = R.check_case(self.c, self.inp, k, R.deltas(self.io))
        print(f"\nROWSTAT {' + '.join(self.paths.values())} | " + " ".join(f"{n} {v:.3e}" for n, v in st.items()) + f" | {self.what}")
        if f == "ln" and self.c["slope"] >= 0:
            assert st["min_abs_pre"] >= R.KINK_MARGIN / 2, f"{self.what}: a pre-activation of the kernel's own state lies {st['min_abs_pre']:.2e} from the kink"
        return st


def run_colsum(C, c):
    lib, p = C.lib(), C.ptr
    inp, _ = R.case_inputs(c)
    M, N, io = c["M"], c["D"], c["io"]
    iod, dt = (C.BF16, BF16) if io == "bf16" else (C.F32, F32)
    x = inp["x"].to(dt).to(DEV)
    keep = x.clone()
    out = torch.full((N + 8,), SENT, dtype=F32, device=DEV)
    if c["acc"]:
        out[:N] = inp["out0"].to(DEV)
    else:
        out[:N].view(torch.uint8).fill_(0xFF)
    nb = R.workspace_bytes("colsum", M, N)
    assert nb == int(lib.tsasr_colsum_workspace_bytes(M, N))
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    ws[:nb], ws[nb:] = 0xFF, GUARD
    C.check(lib.tsasr_colsum(p(x), p(out), M, N, c["acc"], iod, p(ws), nb, C.stream_ptr()), "tsasr_colsum " + c["key"])
    torch.cuda.synchronize()
    assert bool((out[N:] == SENT).all()) and bool((ws[nb:] == GUARD).all()) and torch.equal(bits(x), bits(keep)), c["key"]
    w = (ws[:nb].view(torch.int32) != -1).cpu()
    n = R.n_workgroups("colsum", io, M, N) * N
    assert bool(w[:n].all()) and not bool(w[n:].any()), f"{c['key']}: the partial slab is not the {n // N} x {N} floats the mirror expects"
    st = R.check_case(c, inp, {"out": out[:N].cpu()}, R.deltas(io))
    print(f"\nROWSTAT {R.expected_path('colsum', io, N)} | colsum {st['colsum']:.3e} | {c['key']}")


# ------------------------------------------------------------------------------------------------------ the paths
def groups(fams):
    g = {}
    for c in R.matrix():
        if c["fam"] in fams:
            g.setdefault(f"{c['fam']}-{c['io']}-{next(iter(R.case_paths(c).values()))}", []).append(c)
    return g


LN, ALN, ELT = groups(("ln",)), groups(("aln", "aln2")), groups(("bad", "da", "da2"))


def test_workspace_formulas_match_the_library(C):
    lib = C.lib()
    for M in (1, 37, 16384, 16385, 16401, 17409, 70001):
        for D in (8, 64, 144, 2048, 16384):
            assert int(lib.tsasr_layernorm_bwd_workspace_bytes(M, D)) == R.workspace_bytes("ln", M, D)
            assert int(lib.tsasr_add_layernorm_bwd_workspace_bytes(M, D)) == R.workspace_bytes("aln", M, D)
            assert int(lib.tsasr_add_layernorm2_bwd_workspace_bytes(M, D)) == R.workspace_bytes("aln2", M, D)
            assert int(lib.tsasr_colpart_workspace_bytes(M, D)) == R.workspace_bytes("bad", M, D)
            assert int(lib.tsasr_colsum_workspace_bytes(M, D)) == R.workspace_bytes("colsum", M, D)


@pytest.mark.parametrize("group", list(LN), ids=list(LN))
def test_layernorm_path(C, group):
    """every layernorm_{fwd,bwd}_kernel and _wide_kernel instantiation of both io types: D just over the previous boundary (masked lanes in
    the last iteration) and at the boundary; M = 1, 7, 37 (workgroups of 16, 16, 5), 16401 (17 rows per workgroup, a last one of 13: the
    half-wave loops); slope off / 0.01; tsasr_layernorm_bwd_add on every one-wave kernel"""
    for c in LN[group]:
        Run(C, c).run()


@pytest.mark.parametrize("group", list(ALN), ids=list(ALN))
def test_add_layernorm_path(C, mask_port, group):
    """every add_layernorm{,2}_{fwd,bwd}_kernel instantiation: bias / dout / dy present and absent, p 0 / 0.1, alpha 1 / 0.5, the time mask
    with lengths T, T / 2, 1, seeds above 2^32, host + device seed, NULL parameter gradients, eps != eps2; the three launches over 64 KB of
    LDS (D = 2048 and 1024) among them"""
    for c in ALN[group]:
        Run(C, c).run()


@pytest.mark.parametrize("group", list(ELT), ids=list(ELT))
def test_dropout_path(C, mask_port, group):
    """bias_act_dropout, dropout_add, dropout_add2 (p2 > 0 with dres): N = 8, 64 (row slots through LDS), 2048, 2056 (one slot, a second
    column pass); M = 1, 37, 16401; dropped elements exactly 0, kept ones exactly scaled, the backward on the forward's bits"""
    for c in ELT[group]:
        Run(C, c).run()


@pytest.mark.parametrize("io", R.IOS)
def test_colsum(C, io):
    for c in R.matrix():
        if c["fam"] == "colsum" and c["io"] == io:
            run_colsum(C, c)


# ------------------------------------------------------------------------------------------------------ rejections
def find(prefix):
    return next(c for c in R.matrix() if c["key"].startswith(prefix))


@pytest.mark.parametrize("io", R.IOS)
def test_rejections_write_nothing(C, io):
    """D % 8 != 0, D over each entry's limit, a workspace one byte short, dadd on a wide D, p2 > 0 without dres, M not a multiple of Trows
    with valid_lens: a non-zero return, every output as it was"""
    D0 = R.NARROW[io]
    for fam, limit in (("ln", R.LN_REJ[io]), ("aln", R.ALN_REJ), ("aln2", R.ALN2_REJ)):
        r = Run(C, find(f"{fam}-{io}-M37-D{D0}"))
        r.alloc()
        for kw in ({"D": 12}, {"D": limit}):
            assert R.expected_path(next(iter(r.paths)), io, kw["D"]) == R.REJECTED
            assert r.fwd(**kw) != 0, (fam, kw)
            torch.cuda.synchronize()
            r.untouched(f"fwd {kw}")
        C.check(r.fwd(), "forward")
        torch.cuda.synchronize()
        done = r.FWD_OUT[fam] + r.FWD_STAT[fam]
        rest = [k for k in list(r.out) + list(r.par) + ["workspace"] if k not in done]
        for kw in ({"D": 12}, {"D": limit}, {"nbytes": r.nb - 1}):
            assert r.bwd(**kw) != 0, (fam, kw)
            torch.cuda.synchronize()
            r.untouched(f"bwd {kw}", rest)
            r.guards(f"bwd {kw}")
        assert b"workspace too small" in r.lib.tsasr_last_error()
    wide = R.LN_D[io][8]
    assert R.ln_is_wide(io, wide) and R.expected_path("layernorm_bwd_add", io, wide) == R.REJECTED
    r = Run(C, find(f"ln-{io}-M37-D{wide}"))
    r.alloc()
    C.check(r.fwd(), "forward")
    torch.cuda.synchronize()
    assert r.bwd(force_dadd=True) != 0
    torch.cuda.synchronize()
    r.untouched("bwd_add on a wide row", ["dx", "dgamma", "dbeta", "workspace"])
    r = Run(C, find(f"da2-{io}-M37-D64"))
    r.alloc()
    assert r.c["p2"] > 0 and r.bwd(dres=False) != 0
    torch.cuda.synchronize()
    r.untouched("dropout_add2_bwd without dres")
    for fam in ("aln", "aln2", "da"):
        r = Run(C, find(f"{fam}-{io}-M39-D"))
        assert r.c["vl"]
        r.alloc()
        r.trows = 14                                                            # 39 rows are no multiple of 14
        assert r.fwd() != 0, fam
        torch.cuda.synchronize()
        r.untouched(f"{fam} forward with M % Trows != 0")
