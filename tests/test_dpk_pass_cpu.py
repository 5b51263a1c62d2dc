"""The one-pass d(pk) body's tile walk (csrc/dpk_pass.h), proved on a Python mirror of it (tests/helpers/dpk_walk.py): every (query, key)
pair with i < T', j < key_lens[b] and inside the look-ahead limit is accumulated exactly once into the band row r = j - i + T' - 1 of its
utterance group's partial plane, nothing else is, every row of dS is requested once, and the rows of the partial planes the walk writes
are exactly the bytes the size function promises."""
import importlib

import numpy as np
import pytest

from tests.helpers import dpk_walk
from tests.helpers.attn_ref import allowed_mask

SHAPES = [2, 63, 64, 65, 125, 128, 250, 256]


def lens_for(T, B):
    return [T, 1, max(1, T // 2), max(1, T - 1), min(T, 65)][:B]


@pytest.mark.parametrize("causal", [0, 1, 16])
@pytest.mark.parametrize("T", SHAPES)
def test_walk_accumulates_every_allowed_pair_once(T, causal):
    B = 5
    lens = lens_for(T, B)
    count, written, loads = dpk_walk.walk(B, T, lens, causal)
    want = allowed_mask(T, lens, causal).numpy().astype(np.int64)      # [B, i, j]
    assert np.array_equal(count[0], want) and np.array_equal(count[1], want)
    assert np.all(written == 1)                                        # every row of every plane stored once, per head-dim half
    assert np.all(loads == 1)                                          # every row of dS and q + v requested once
    assert dpk_walk.skipped_fragments_are_empty(B, T, lens, causal)


@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("T", SHAPES)
def test_partial_planes_match_the_size_function(pkg, T, B):
    H = 4
    _, written, _ = dpk_walk.walk(B, T, [T] * B, 0)
    stored = int(written.sum()) * 32 * 4 * H                           # rows x head-dim halves x 32 floats x heads
    assert stored == dpk_walk.part_bytes(B, T, H)
    capi = importlib.import_module("ts-asr_amd._capi")
    assert capi.lab().tsasr_lab_dpk_part_bytes(B, T, H) == dpk_walk.part_bytes(B, T, H)
    # the product's workspace holds at least these planes next to its other regions
    assert capi.lib().tsasr_relpos_attn_bwd_workspace_bytes(B, T, H) >= dpk_walk.part_bytes(B, T, H)


def test_groups_are_the_old_bodys():
    # 256 / (4 x blocks of 64 band rows) utterance groups at most: the partial planes of the benchmark's two shapes stay 8 and 16 per layer
    assert (dpk_walk.bgroup(32, 250), dpk_walk.bgroup(32, 125)) == (4, 2)
