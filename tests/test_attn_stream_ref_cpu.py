"""The reference, the push-by-push emulation and the checker of the streaming attention path matrix (tests/helpers/attn_stream_ref.py,
used by tests/test_attn_stream_paths_gpu.py): the reference equals the offline float64 reference and the fp32 oracle, the emulation of
the kernels' tile walk, key splits and merge equals the reference to 1e-12 from a NaN cache, the checker rejects every planted defect at
the loosest bounds the GPU tests allow - and the defects that move one row or one element slip under the relative L2 of 8e-3 over the
whole output that tests/test_streaming_gpu.py checks. CPU only."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import attn_ref as AR  # noqa: E402
import attn_stream_ref as SR  # noqa: E402
from oracle import tsasr_ref as R  # noqa: E402

MIX = (7, 40, 1, 16, 64, 33, 17, 65, 15, 31, 100)
M8 = (8, 40, 16, 64, 24)
OLD_GLOBAL = {"out": (8e-3, None)}      # tests/test_streaming_gpu.py: rel_l2 < 8e-3 for bf16


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("causal", [0, 1, 8])
def test_reference_equals_offline_reference_and_oracle(causal):
    B, T, H, Dh, lens = 3, 50, 2, 12, (50, 33, 9)
    qkv, pkh, u, v, scale = SR.inputs(B, T, H, Dh, T)
    pushes = SR.schedule(M8 if causal else (T,), T)      # without a mask a push sees no later push: one push is the offline call
    allowed = SR.allowed(pushes, lens, causal, B)
    ref = SR.reference(qkv, pkh, u, v, H, scale, allowed)
    pk = pkh[(torch.arange(2 * T - 1) - (T - 1)).abs()]                 # pk[j - i + T - 1] = pkh[|i - j|]
    off = AR.reference(qkv, pk, u, v, torch.zeros(B, T, H * Dh), H, scale, AR.allowed_mask(T, lens, causal))["out"]
    assert float((ref - off).abs().max()) < 1e-12
    kpm = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
    orc, _ = R.relpos_core(qkv, pk, u, v, H, scale, kpm, causal)
    assert rel(orc, ref) < 1e-5


@pytest.mark.parametrize("causal,sizes", [(0, (170,)), (1, MIX), (1, (40,)), (8, M8), (8, (8,)), (40, (40,)), (40, (80, 40))])
def test_allowed_equals_offline_mask_for_aligned_pushes(causal, sizes):
    T, lens = 170, (170, 129, 64, 0, 1)
    got = SR.allowed(SR.schedule(sizes, T), lens, causal, len(lens))
    assert torch.equal(got, AR.allowed_mask(T, lens, causal))
    assert torch.equal(SR.allowed(SR.schedule(sizes, T), None, causal, 2), AR.allowed_mask(T, (T, T), causal))


def test_allowed_without_a_mask_ends_at_the_push():
    """causal = 0: every key pushed so far, the query's own push included, and none of a later push."""
    T = 64
    got = SR.allowed(SR.schedule(MIX, T), (T, 50), 0, 2)
    end = torch.tensor([7] * 7 + [47] * 40 + [48] + [64] * 16)
    j = torch.arange(T)
    assert torch.equal(got[0], j[None, :] < end[:, None])
    assert torch.equal(got[1], j[None, :] < end.clamp(max=50)[:, None])


def test_allowed_unaligned_block_causal_differs_in_the_expected_cells():
    """Pushes (7, 40, ...) under blocks of 8: a query of a block that the push cuts cannot see the block's frames not pushed yet."""
    T, c = 64, 8
    pushes = SR.schedule(MIX, T)                                        # (0,7) (7,40) (47,1) (48,16)
    assert pushes == ((0, 7), (7, 40), (47, 1), (48, 16))
    got, off = SR.allowed(pushes, None, c, 1)[0], AR.allowed_mask(T, (T,), c)[0]
    want = torch.zeros(T, T, dtype=torch.bool)
    want[0:7, 7] = True                                                 # block 0 ends at 7, pushed to 6
    want[40:47, 47] = True                                              # block 5 (40..47) pushed to 46
    assert torch.equal(off & ~got, want)
    assert not (got & ~off).any()


# ---------------------------------------------------------------------------------------------- the emulation
EMU = {  # name: (B, T, H, Dh, Tmax, lens, causal, sizes, nsplit, tps)
    "mix_unsplit": (4, 170, 2, 16, 200, (170, 129, 64, 0), 1, MIX, 1, 4),
    "mix_split": (3, 300, 2, 16, 330, (300, 193, 1), 1, MIX, 3, 2),
    "unaligned_block": (2, 170, 2, 16, 200, None, 8, MIX, 1, 4),
}


@pytest.fixture(scope="module")
def emu():
    out = {}
    for name, (B, T, H, Dh, Tmax, lens, causal, sizes, ns, tps) in EMU.items():
        args = SR.inputs(B, T, H, Dh, Tmax)
        pushes = SR.schedule(sizes, T)
        allowed = SR.allowed(pushes, lens, causal, B)
        out[name] = (args, pushes, allowed, SR.reference(*args[:4], H, args[4], allowed))
    return out


def run(emu, name, defect=None, dtype=torch.float64):
    B, T, H, Dh, Tmax, lens, causal, sizes, ns, tps = EMU[name]
    args, pushes, allowed, ref = emu[name]
    return SR.emulate(*args[:4], H, args[4], pushes, lens, causal, Tmax, ns, tps, dtype, defect)


@pytest.mark.parametrize("name", list(EMU))
def test_emulation_equals_reference_from_a_nan_cache(emu, name):
    """Tile walk, online softmax, key splits (some without a key) and the merge reproduce the reference; the cache starts as NaN, so a
    single read of a row not yet written would show."""
    B, T, H, Dh, Tmax, lens, causal, sizes, ns, tps = EMU[name]
    if ns > 1:
        assert SR.stream_split(B, 40, H, Tmax) == (ns, tps)
    got, ref = run(emu, name), emu[name][3]
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max()) < 1e-12
    errs, bad = SR.measure(got, ref, emu[name][2], B, T, H, Dh)
    assert not SR.failures(errs, bad, {"out": (1e-12, 1e-12)})


def test_emulation_in_float32_is_within_the_fp32_ceiling(emu):
    B, T, H, Dh = EMU["mix_split"][:4]
    errs, bad = SR.measure(run(emu, "mix_split", dtype=torch.float32), emu["mix_split"][3], emu["mix_split"][2], B, T, H, Dh)
    assert not SR.failures(errs, bad, {"out": SR.CEIL["f32"]}), errs


# ---------------------------------------------------------------------------------------------- the checker can fail
def verdict(emu, name, defect, kind=None):
    """(failures of the full checker at the loosest GPU bounds, failures of the older tests' global bound alone)."""
    B, T, H, Dh = EMU[name][:4]
    errs, bad = SR.measure(run(emu, name, defect), emu[name][3], emu[name][2], B, T, H, Dh)
    return SR.failures(errs, bad, SR.loosest(kind)), SR.failures(errs, bad, OLD_GLOBAL, global_only=True), errs


def fired(full):
    return {"structural" if "non-finite" in f or "exactly zero" in f else "per-row" if "per-row" in f else "global" for f in full}


def test_bounds_are_within_the_ceilings():
    """Every bound is within the ceiling of its kernel family but the per-row bounds of SR.OVER_CEILING (the matrix-core kernels on the
    peaked draw: the bf16 rounding of q + u / q + v against dominated rows, see the comment at SR.TOL)."""
    for (path, kind), t in SR.TOL.items():
        (g, r), (cg, cr) = t["out"], SR.CEIL[path.split("_")[0]]
        assert g <= cg, (path, kind)
        assert r <= cr or (path, kind) in SR.OVER_CEILING, (path, kind)
    assert SR.loosest("o1")["out"][1] <= 0.015 and SR.loosest()["out"][0] <= 8e-3
    assert all(k == "peaked" and p.startswith("mfma") for p, k in SR.OVER_CEILING)


def test_causal_limit_one_frame_late_for_the_first_query_of_one_push(emu):
    """Query 64 (the first of the push (64, 64)) also sees key 65, in every utterance that long and every head: those rows move by 7 %,
    the whole output by 1.3e-3, a sixth of the old bound. One row: per-row only."""
    assert emu["mix_unsplit"][1][4] == (64, 64)
    full, glob, errs = verdict(emu, "mix_unsplit", ("causal_late", 4))
    assert fired(full) == {"per-row"}, (full, errs)
    assert not glob, errs


def test_causal_limit_one_frame_late_in_every_push(emu):
    full, glob, errs = verdict(emu, "mix_unsplit", "causal_late")
    assert "per-row" in fired(full), (full, errs)


def test_positional_distance_one_short_for_cached_keys(emu):
    full, glob, errs = verdict(emu, "mix_unsplit", "cache_dist")
    assert {"per-row", "global"} <= fired(full), (full, errs)
    assert glob


def test_last_non_empty_split_dropped_in_the_merge(emu):
    full, glob, errs = verdict(emu, "mix_split", "drop_split")
    assert {"per-row", "global"} <= fired(full), (full, errs)
    assert glob


def test_newest_cache_row_read_as_zeros(emu):
    """Key t0 - 1 with K = V = 0: its score loses the content term and its value is gone, in every row of every push."""
    full, glob, errs = verdict(emu, "mix_unsplit", "stale_cache")
    assert "per-row" in fired(full), (full, errs)


def test_key_lens_ignored_for_keys_of_the_chunk(emu):
    """Rows past an utterance's length attend their own chunk's keys; the rows of utterance 3 (no key at all) come out nonzero."""
    full, glob, errs = verdict(emu, "mix_unsplit", "chunk_lens")
    assert {"per-row", "structural"} <= fired(full), (full, errs)


def test_dead_row_left_as_nan(emu):
    full, glob, errs = verdict(emu, "mix_unsplit", "dead_nan")
    assert fired(full) == {"structural"}, (full, errs)
    full, glob, errs = verdict(emu, "mix_split", "dead_nan")           # utterance 2 (one key): no dead row, nothing to leave
    assert not full, (full, errs)


def test_one_element_of_one_row_off_by_two_percent_of_the_row_norm(emu):
    """Judged at the loosest bound of the o1 draws, the draw it is planted in (per-row 0.0091): the per-row bounds of SR.OVER_CEILING
    (0.022 - 0.033, the matrix-core kernels on the peaked draw) stand for an error of the bf16 operands that is itself as large as this
    defect, and would let it pass on those four entries."""
    full, glob, errs = verdict(emu, "mix_unsplit", "one_element", "o1")
    assert fired(full) == {"per-row"}, (full, errs)
    assert not glob, errs
    assert errs["out"][0] < 8e-3 / 10                                   # an order of magnitude below the old bound


# ---------------------------------------------------------------------------------------------- the host's split rule
@pytest.mark.parametrize("shape,want", [((1, 40, 4, 4000), (32, 2)), ((2, 40, 2, 330), (3, 2)), ((4, 8, 4, 256), (1, 4)),
                                        ((64, 40, 4, 4000), (1, 63)), ((1, 40, 1, 1000), (8, 2)), ((16, 40, 4, 1000), (4, 4)),
                                        ((30, 40, 4, 1000), (3, 6))])
def test_stream_split_hand_evaluated(shape, want):
    assert SR.stream_split(*shape) == want
