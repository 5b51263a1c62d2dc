"""The checker of the attention path matrix (tests/helpers/attn_ref.py, used by tests/test_attention_paths_gpu.py) can fail: each test
builds the float64 reference of a call at the training shape (B = 32, H = 4, T' = 250, block-causal C = 40, dropout 0.1, ragged keys)
and a float64 reference of a subtly WRONG kernel, and asserts that the checker rejects the wrong one at the loosest bounds the GPU tests
allow. Each test also pins whether the older bf16 tests' check - one relative-L2 bound over each whole tensor, 1e-2 on the output and
2.5e-2 on the gradients - would have caught the mutation alone: three of the six slip under it. CPU only."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn_ref as AR  # noqa: E402

B, T, H, Dh, C, P = 32, 250, 4, 64, 40, 0.1
LENS = (250, 161, 97) + tuple(250 - 7 * b for b in range(1, 30))
SEED = 77


@pytest.fixture(scope="module")
def base():
    D = H * Dh
    g = torch.Generator().manual_seed(2024)
    qkv = torch.randn(B, T, 3 * D, generator=g).to(torch.bfloat16)
    pk = torch.randn(2 * T - 1, D, generator=g).to(torch.bfloat16)
    u, v = torch.randn(D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    dout = torch.randn(B, T, D, generator=g).to(torch.bfloat16)
    args = (qkv, pk, u, v, dout, H, 1.0 / D ** 0.5)
    allowed, keep = AR.allowed_mask(T, LENS, C), AR.keep_mask(B, H, T, P, SEED)
    return args, allowed, keep, AR.reference(*args, allowed, keep, P)


# the whole-tensor bounds of the older bf16 tests (test_blocks_gpu.py: 1e-2 on the output, 2.5e-2 on every gradient)
OLD_GLOBAL = {"out": (1e-2, None), **{k: (2.5e-2, None) for k in ("dQ", "dK", "dV", "dpk", "du", "dv")}}


def verdict(mutant, base):
    """(failures of the full checker at the loosest GPU bounds, failures of the older tests' global bounds alone)."""
    _, allowed, _, ref = base
    errs, bad = AR.measure(mutant, ref, allowed, B, T, H, Dh)
    return AR.failures(errs, bad, AR.loosest()), AR.failures(errs, bad, OLD_GLOBAL, global_only=True)


def test_reference_passes_its_own_check(base):
    full, _ = verdict(dict(base[3]), base)
    assert not full, full


def test_block_causal_limit_one_key_late_for_a_whole_chunk(base):
    """The 40 queries of the third chunk also see the first key of the next chunk (a `<=` for a `<` at the chunk end), in every utterance
    and head: 1 / 6 of the rows move, enough for the global bound too."""
    args, _, keep, _ = base
    lim = AR.causal_limit(T, C).clone()
    lim[80:120] += 1
    full, glob = verdict(AR.reference(*args, AR.allowed_mask(T, LENS, limit=lim), keep, P), base)
    assert full
    assert glob


def test_block_causal_limit_one_key_late_at_a_chunk_boundary(base):
    """Only the last query of the third chunk (i = 119, the row on the boundary) sees key 120 - in every utterance and head. Its output
    rows move by tens of percent; the whole-tensor norm by half a percent: per-row only."""
    args, _, keep, _ = base
    lim = AR.causal_limit(T, C).clone()
    lim[119] += 1
    full, glob = verdict(AR.reference(*args, AR.allowed_mask(T, LENS, limit=lim), keep, P), base)
    assert full
    assert not glob


def test_last_valid_key_of_one_utterance_dropped(base):
    """Utterance 1 (161 keys) loses its last key (a length read as len - 1). Per-row: that key's dK / dV rows are zero in the mutant
    while the reference's are not; every output row of the utterance moves a little. The global bound misses it."""
    args, _, keep, _ = base
    full, glob = verdict(AR.reference(*args, AR.allowed_mask(T, (250, 160) + LENS[2:], C), keep, P), base)
    assert full
    assert not glob


def test_dropout_mask_of_one_row_shifted_by_one_key(base):
    """One query row of one head draws its keep bits one key off (a word index off by one in the stream). Only that row's output and
    the gradients it feeds move: invisible globally, plain per row."""
    args, allowed, keep, _ = base
    k2 = keep.clone()
    k2[1, 0, 57] = torch.roll(keep[1, 0, 57], 1)
    full, glob = verdict(AR.reference(*args, allowed, k2, P), base)
    assert full
    assert not glob


def test_dpk_shifted_by_one_band_row(base):
    """d(pk) written one relative row off (r <- r - 1). Neighbouring band rows are uncorrelated sums: the global bound catches it too."""
    ref = base[3]
    full, glob = verdict({**ref, "dpk": torch.roll(ref["dpk"], 1, dims=0)}, base)
    assert full
    assert glob


def test_one_query_block_of_one_head_zeroed(base):
    """One 32-query block of one head left unwritten (zero) in the output: 32 of 1500 rows; the global bound catches it as well."""
    ref = base[3]
    out = ref["out"].clone().view(B, T, H, Dh)
    out[0, 96:128, 1] = 0
    full, glob = verdict({**ref, "out": out.view(B, T, H * Dh)}, base)
    assert full
    assert glob


def test_structural_zero_rows_are_enforced(base):
    """A kernel that leaves a small value (well inside every bound) in the dK row of a key beyond its utterance's length, or in a d(pk)
    row beyond the block-causal band (T - 1 + C - 1), fails the structural check."""
    ref = base[3]
    dq = ref["dqkv"].clone().view(B, T, H, 3, Dh)
    dq[2, 200, 0, 1, 5] = 1e-6                       # key 200 of utterance 2 (97 keys)
    full, glob = verdict({**ref, "dqkv": dq.view(B, T, 3 * H * Dh)}, base)
    assert any("dK" in f and "exactly zero" in f for f in full) and not glob
    dpk = ref["dpk"].clone()
    dpk[T - 1 + C] = 1e-6
    full, glob = verdict({**ref, "dpk": dpk}, base)
    assert any("dpk" in f and "exactly zero" in f for f in full) and not glob
