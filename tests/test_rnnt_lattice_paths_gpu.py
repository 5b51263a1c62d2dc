"""Every path of the RNN-T loss lattice (csrc/rnnt.hip: rnnt_lp_kernel -> rnnt_alphabeta_kernel -> rnnt_grad_kernel) against float64, cell by
cell: all 33 instantiations of the lattice kernel, the unguarded steady state of every form, six value regimes, every lane of rnnt_lp's
V <= 32 path, padded rows of the general path and the documented clamps. The planes are read out of a workspace the test owns, through
tsasr_rnnt_loss_workspace_layout; what is compared with what, and the tolerance model: tests/helpers/rnnt_lattice_ref.py."""
import collections
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests.helpers import rnnt_lattice_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRACTIONS = collections.defaultdict(dict)        # family -> check -> worst fraction of its tolerance (printed by the last test)


@pytest.fixture(scope="module")
def C():
    return importlib.import_module("ts-asr_amd._capi")


def layout(C, B, T, U1):
    out = (ctypes.c_longlong * 17)()
    assert C.lib().tsasr_rnnt_loss_workspace_layout(B, T, U1, ctypes.cast(out, ctypes.c_void_p), 17) == 17
    names = ("plane", "R", "U1P", "sh", "K", "KT", "NW", "NC", "skew", "lpb", "lpe_in", "lpe_out", "alpha", "beta", "lse", "xch", "logp")
    return dict(zip(names, (int(v) for v in out)))


def run_loss(C, lg, tg, tlen, ulen, blank, V, gs, ldl, plan, fill, ldt=None):
    """One tsasr_rnnt_loss_fwd + _bwd on a workspace filled with `fill` bytes; logits rows padded to ldl floats with NaN beyond V.
    Returns the planes [B, T, U1] as the kernels left them, logp, costs, dlogits [B, T, U1, ldl] and the layout."""
    lib = C.lib()
    B, T, U1 = lg.shape[:3]
    ldt = max(U1 - 1, 1) if ldt is None else ldt
    x = np.full((B, T, U1, ldl), np.nan, np.float32)
    x[..., :V] = lg[..., :V]
    t_host = np.zeros((B, ldt), np.int32)
    n = min(ldt, tg.shape[1])
    t_host[:, :n] = tg[:, :n]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)  # noqa: E731
    xd, td, tl, ul = torch.from_numpy(x).to(DEV), i32(t_host), i32(tlen), i32(ulen)
    gsd = torch.from_numpy(np.ascontiguousarray(gs, np.float32)).to(DEV)
    try:
        lib.tsasr_rnnt_lattice_plan(*plan)
        lay = layout(C, B, T, U1)
        nbytes = int(lib.tsasr_rnnt_loss_workspace_bytes(B, T, U1))
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        costs = torch.full((B,), float("nan"), device=DEV)
        dl = torch.full((B, T, U1, ldl), float("nan"), device=DEV)
        C.check(lib.tsasr_rnnt_loss_fwd(C.ptr(xd), C.ptr(td), ldt, C.ptr(tl), C.ptr(ul), C.ptr(costs), B, T, U1, V, ldl, blank, C.ptr(ws), nbytes,
                                        C.stream_ptr()), "tsasr_rnnt_loss_fwd")
        C.check(lib.tsasr_rnnt_loss_bwd(C.ptr(xd), C.ptr(td), ldt, C.ptr(tl), C.ptr(ul), C.ptr(gsd), C.ptr(dl), B, T, U1, V, ldl, blank, C.ptr(ws),
                                        nbytes, C.stream_ptr()), "tsasr_rnnt_loss_bwd")
        torch.cuda.synchronize()
        off = int(lib.tsasr_rnnt_loss_error_word_offset(B, T, U1))
    finally:
        lib.tsasr_rnnt_lattice_plan(-1, -1, -1)
    raw = ws.cpu().numpy()
    assert (off >= 0) == (lay["NC"] > 1)
    if off >= 0:
        assert raw[off:off + 4].view(np.uint32)[0] != 1, "the split lattice timed out waiting for a neighbour block"
    wsf = raw[: nbytes // 4 * 4].view(np.float32)
    b, t, u = np.arange(B)[:, None, None], np.arange(T)[None, :, None], np.arange(U1)[None, None, :]
    idx = (b * lay["R"] + t + (u >> lay["sh"])) * lay["U1P"] + u
    assert idx.max() < lay["plane"]
    out = {p: wsf[lay[p] + idx] for p in LR.PLANES}
    out["logp"] = wsf[lay["logp"]: lay["logp"] + B].copy()
    out["costs"] = costs.cpu().numpy()
    out["dlogits"] = dl.cpu().numpy()
    out["layout"] = lay
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(a, b, ref, what):
    live = ref["live"]
    assert np.array_equal(bits(a["costs"]), bits(b["costs"])), f"{what}: costs differ"
    assert np.array_equal(bits(a["dlogits"]), bits(b["dlogits"])), f"{what}: dlogits differ"
    u = np.arange(live.shape[2])[None, None, :]
    masks = {"lpe_out": live & (u < ref["Ub"][:, None, None]), "lpe_in": live & (u > 0)}
    for p in LR.PLANES:
        m = masks.get(p, live)
        assert np.array_equal(bits(a[p])[m], bits(b[p])[m]), f"{what}: live cells of {p} differ"
    assert np.array_equal(bits(a["logp"]), bits(b["logp"])), f"{what}: logp differs"


def check_case(C, family, inputs, ref, tol, ldl, plan, want_inst=None, ldt=None):
    """The general rules of every case: 0xFF- and 0x00-filled workspaces give the same bits, exact zeros outside the lattice and in the
    padding, and the whole check matrix on the kernels' planes."""
    lg, tg, tlen, ulen, blank, V, gs = inputs
    B, T, U1 = lg.shape[:3]
    a = run_loss(C, lg, tg, tlen, ulen, blank, V, gs, ldl, plan, 0xFF, ldt)
    b = run_loss(C, lg, tg, tlen, ulen, blank, V, gs, ldl, plan, 0x00, ldt)
    lay = a["layout"]
    inst = (lay["KT"], lay["NW"], lay["NC"], lay["skew"])
    assert inst == LR.instantiation(B, U1, plan), "the Python mirror of rnnt_plan disagrees with the library"
    if want_inst is not None:
        assert inst == tuple(want_inst)
    assert_same_bits(a, b, ref, f"{family} plan {plan}: workspace fill 0xFF against 0x00")
    dl = a["dlogits"]
    assert np.all(dl[..., V:] == 0), f"dlogits in the padding columns v >= V must be exactly 0 (bit patterns {np.unique(bits(dl[..., V:]))})"      # (+0 or -0: 0 * gscale)
    assert np.all(dl[~ref["live"]] == 0), "dlogits outside the lattice (t >= Tb or u > Ub) must be exactly 0"
    fails, frac = LR.judge(a, ref, tol, inst)
    for k, v in frac.items():
        FRACTIONS[family][k] = max(FRACTIONS[family].get(k, 0.0), v)
    print(f"{family} B,T,U1,V={B},{T},{U1},{V} ldl={ldl} plan={plan} inst={inst}: " + " ".join(f"{k}={v:.3f}" for k, v in frac.items()))
    assert not fails, "\n".join(fails)
    return a


# ---------------------------------------------------------------------------------------------------------------------------------
RAMP = LR.ramp_cases()


@pytest.mark.parametrize("B,U1,plan,inst", RAMP, ids=[f"U{c[1]}-kt{c[3][0]}nw{c[3][1]}nc{c[3][2]}s{c[3][3]}" for c in RAMP])
def test_every_instantiation_ramp_only(C, B, U1, plan, inst):
    """All 33 instantiations at both ends of their K range, T = 11 (ramp-up and ramp-down only), ragged frames [11, 4, 1] and target
    lengths on the thread, wave and column-block boundaries of the instantiation."""
    tlen = LR.RAMP_TLEN[:B]
    ulen = LR.ramp_ulens(U1, inst, B)
    inputs, ref, tol = LR.case("normal", B, LR.RAMP_T, U1, 4, tlen, ulen, seed=U1)
    check_case(C, "ramp", inputs, ref, tol, 4, plan, want_inst=inst)


STEADY = LR.steady_cases()


@pytest.mark.parametrize("group", sorted({c[0] for c in STEADY}, key=lambda g: int(g[2:])))
def test_steady_state_of_every_form(C, group):
    """T = 64 NW + 29: the first utterance runs unguarded chunks between its ramps, the second (64 NW - 3 frames) never does. Frame-major
    and skewed planes (and, on the one-wave lattice, the three split forms) return the same costs and gradients bit for bit."""
    first = None
    for g, B, T, U1, tlen, plan in STEADY:
        if g != group:
            continue
        inputs, ref, tol = LR.case("normal", B, T, U1, 4, tlen, (U1 - 1, U1 - 30), seed=7)
        out = check_case(C, "steady", inputs, ref, tol, 4, plan)
        G = 64 * out["layout"]["NW"]
        assert any(LR.is_steady(s, tlen[0], G) for s in range(tlen[0] + G)) and not any(LR.is_steady(s, tlen[1], G) for s in range(tlen[1] + G))
        if first is None:
            first = (plan, out)
        else:
            assert np.array_equal(bits(out["costs"]), bits(first[1]["costs"])), (first[0], plan)
            assert np.array_equal(bits(out["dlogits"]), bits(first[1]["dlogits"])), (first[0], plan)


@pytest.mark.parametrize("B,T,U1,plan", [(2, 40, 21, (-1, -1, -1)), (2, 90, 130, (0, 1, 0)), (1, 541, 513, (1, 8, 0))],
                         ids=["default", "one-wave", "eight-waves"])
@pytest.mark.parametrize("regime", LR.REGIMES)
def test_regimes(C, regime, B, T, U1, plan):
    tlen = (T, T - 7)[:B]
    ulen = (U1 - 1, U1 - 6)[:B]
    inputs, ref, tol = LR.case(regime, B, T, U1, 4, tlen, ulen, seed=11, allowed=(1, 2))
    out = check_case(C, regime, inputs, ref, tol, 4, plan)
    if regime == "flat":
        for b in range(B):
            want = LR.flat_cost(int(ref["Tb"][b]), int(ref["Ub"][b]), 4)
            assert abs(out["costs"][b] - want) <= tol["cost"][b] + 1e-9 * want


SMALL_SHAPES = [(1, 3, 5), (2, 9, 8), (2, 5, 1)]       # 15 rows (fewer than 32), 144 rows (no multiple of 128), U1 = 1


def label_sets(V, blank):
    first, last = range(0, min(4, V)), range(4 * ((V - 1) // 4), V)
    return list(dict.fromkeys([tuple(first), tuple(last), (V - 1,)]))


@pytest.mark.parametrize("ldl32", [False, True], ids=["ldl=V4", "ldl=32"])
@pytest.mark.parametrize("V", [1, 2, 3, 4, 5, 8, 28, 29, 31, 32])
def test_lp_narrow_vocabulary(C, V, ldl32):
    """rnnt_lp's one-round-trip path (V <= 32): rows of ldl < 32 floats, blank first and last, labels from the first lane, the last lane
    and V - 1 alone."""
    ldl = 32 if ldl32 else (V + 3) // 4 * 4
    for blank in sorted({0, V - 1}):
        for allowed in label_sets(V, blank):
            for i, (B, T, U1) in enumerate(SMALL_SHAPES):
                tlen, ulen = (T, max(T - 2, 1))[:B], (U1 - 1, max(U1 - 3, 0))[:B]
                inputs, ref, tol = LR.case("normal", B, T, U1, V, tlen, ulen, blank=blank, seed=V * 8 + i, allowed=allowed)
                check_case(C, "lp_narrow", inputs, ref, tol, ldl, (-1, -1, -1))


@pytest.mark.parametrize("blank", range(29))
def test_lp_every_blank_lane(C, blank):
    inputs, ref, tol = LR.case("normal", 2, 9, 8, 29, (9, 6), (7, 4), blank=blank, seed=blank)
    check_case(C, "lp_narrow", inputs, ref, tol, 32, (-1, -1, -1))


@pytest.mark.parametrize("pad", [0, 28])
@pytest.mark.parametrize("V", [33, 36, 64, 100])
def test_lp_wide_vocabulary(C, V, pad):
    """The general path of rnnt_lp and rnnt_grad with ldl > V and NaN in the padding, blank in the last column."""
    ldl = (V + 3) // 4 * 4 + pad
    for i, (B, T, U1) in enumerate(SMALL_SHAPES):
        tlen, ulen = (T, max(T - 2, 1))[:B], (U1 - 1, max(U1 - 3, 0))[:B]
        inputs, ref, tol = LR.case("normal", B, T, U1, V, tlen, ulen, blank=V - 1, seed=V + i)
        check_case(C, "lp_wide", inputs, ref, tol, ldl, (-1, -1, -1))


@pytest.mark.parametrize("tl", [0, -3, 14])
@pytest.mark.parametrize("ul", [-1, 10])
def test_documented_clamps(C, tl, ul):
    """tlen in {0, -3, T + 5}, ulen in {-1, U1 + 4}, labels -1 and V + 3, ldt = U1 + 6: the same bits as the call with the arguments
    clamped by hand (and the whole matrix on that call)."""
    B, T, U1, V = 2, 9, 6, 5
    tlen, ulen = (T, tl), (ul, U1 - 2)
    tg = np.array([[1, -1, 2, V + 3, 3], [V + 3, 4, -1, 1, 2]], np.int32)
    tgc, Tb, Ub = LR.clamp_args(tg, tlen, ulen, T, U1, V)
    lg = LR.make_logits("normal", B, T, U1, V, tg, tlen, ulen, 0, 5)
    gs = np.array([0.75, -1.25], np.float32)
    ref = LR.planes64(lg, tg, tlen, ulen, 0, V, gs)
    assert np.array_equal(ref["Tb"], Tb) and np.array_equal(ref["Ub"], Ub)
    tol = LR.tolerances((lg, tg, np.asarray(tlen), np.asarray(ulen), 0, V, gs), ref)
    raw = check_case(C, "clamps", (lg, tg, np.asarray(tlen), np.asarray(ulen), 0, V, gs), ref, tol, 8, (-1, -1, -1), ldt=U1 + 6)
    by_hand = run_loss(C, lg, tgc, Tb, Ub, 0, V, gs, 8, (-1, -1, -1), 0xFF)
    assert_same_bits(raw, by_hand, ref, "raw arguments against arguments clamped by hand")


def test_zz_fractions_of_tolerance():
    """Prints the worst fraction of its tolerance each check used, per family of cases (DESIGN.md quotes them). Every fraction has been
    asserted <= 1 where it was measured; nothing is asserted here."""
    for family, fr in FRACTIONS.items():
        print(f"fractions[{family}]: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(fr.items())))
