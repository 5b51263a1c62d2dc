"""Python mirror of the one-pass d(pk) body (csrc/dpk_pass.h, dpk_once_body): which workgroup stages which (utterance, query block),
which 32-row x 16-query fragments each wave multiplies, which it skips, what the staged rows hold, and which rows of the partial planes it
writes. tests/test_dpk_pass_cpu.py proves from it that every allowed (query, key) pair is accumulated exactly once and nothing else is."""
import numpy as np

TH, PAD, LD = 512, 48, 48 + 256 + 48 + 8      # DPO_TH, DPO_PAD, DPO_LD


def cdiv(a, b):
    return (a + b - 1) // b


def bgroup(B, T):                # dpk_bgroup
    want = max(1, 256 // (4 * cdiv(2 * T - 1, 64)))
    return max(1, cdiv(B, min(B, want)))


def part_bytes(B, T, H):         # tsasr_lab_dpk_part_bytes; csrc/attention.hip's attn_part_bytes is this rounded up to 256 (isplit = 1 at T <= 256)
    return cdiv(B, bgroup(B, T)) * (2 * T - 1) * H * 64 * 4


def causal_limit(i, causal):
    return i if causal <= 1 else (i // causal + 1) * causal - 1


def stage(T, Tp, i0, length, causal):
    """bool [64, LD]: the elements of the staged rows that hold a value of dS (everything else is zero), as the masked stores leave them."""
    lds = np.zeros((64, LD), dtype=bool)
    for tid in range(TH):
        sil, sj = tid >> 5, (tid & 31) * 8
        if sj >= Tp:
            continue
        for it in range(4):
            il = sil + 16 * it
            i = i0 + il
            lim = (min(length - 1, causal_limit(i, causal)) if causal else length - 1) if i < T else -1
            nv = min(max(lim + 1 - sj, 0), 8)
            lds[il, PAD + sj:PAD + sj + nv] = True
    return lds


def walk(B, T, lens, causal):
    """-> (count int [2, B, T, T]: how often the pair (b, i, j) is added into its band row, per head-dim half;
           written int [G, 2T-1, 2]: how often a row of a partial plane is stored, per head-dim half;
           loads int [B, T]: how often a row of dS (and of q + v) is requested from memory with i < T (clamped repeats not counted)).
    Asserts on the way that no LDS read leaves the staged rows and that a fragment feeds the band row r = j - i + T - 1 of its own group."""
    Tp, R, nib = cdiv(T, 64) * 64, 2 * T - 1, cdiv(T, 64)
    bg = bgroup(B, T)
    G = cdiv(B, bg)
    count = np.zeros((2, B, T, T), dtype=np.int64)
    written = np.zeros((G, R, 2), dtype=np.int64)
    loads = np.zeros((B, T), dtype=np.int64)
    rl, k = np.meshgrid(np.arange(32), np.arange(16), indexing="ij")
    for grp in range(G):
        b0 = grp * bg
        nb = min(B, b0 + bg) - b0
        for p in range(nb * nib):
            b, i0 = b0 + p // nib, (p % nib) * 64
            length = min(max(int(lens[b]), 1), T)
            lds = stage(T, Tp, i0, length, causal)
            loads[b, i0:min(i0 + 64, T)] += 1
            for wave in range(8):
                cls, dblk = wave & 3, wave >> 2
                for s in range(4):
                    for a in range(4):
                        rb = cls + 4 * a
                        jlo = rb * 32 + i0 - (T - 1) + 16 * s
                        if rb * 32 >= R or jlo + 46 < 0 or jlo >= length or (causal and rb * 32 - (T - 1) > max(causal, 1) - 1):
                            continue
                        il = 16 * s + k
                        col = PAD + (jlo - 16 * s) + rl + il
                        assert col.min() >= 0 and col.max() < LD, (T, i0, rb, s, col.min(), col.max())
                        hit = lds[il, col]
                        ii, jj, rr = (i0 + il)[hit], (col - PAD)[hit], (rb * 32 + rl)[hit]
                        assert np.all(rr == jj - ii + T - 1) and np.all(rr < R)
                        np.add.at(count, (dblk, b, ii, jj), 1)
        for wave in range(8):
            cls, dblk = wave & 3, wave >> 2
            for a in range(4):
                for row in range(32):
                    rg = 32 * (cls + 4 * a) + row
                    if rg < R:
                        written[grp, rg, dblk] += 1
    return count, written, loads


def skipped_fragments_are_empty(B, T, lens, causal):
    """Every fragment the walk skips holds no allowed pair (checked from the mask itself, not from the staged rows)."""
    R, nib = 2 * T - 1, cdiv(T, 64)
    for b in range(B):
        length = min(max(int(lens[b]), 1), T)
        for i0 in range(0, nib * 64, 64):
            for rb in range(16):
                for s in range(4):
                    jlo = rb * 32 + i0 - (T - 1) + 16 * s
                    skip = rb * 32 >= R or jlo + 46 < 0 or jlo >= length or (causal and rb * 32 - (T - 1) > max(causal, 1) - 1)
                    if not skip:
                        continue
                    for r in range(rb * 32, rb * 32 + 32):
                        for i in range(i0 + 16 * s, i0 + 16 * s + 16):
                            j = r + i - (T - 1)
                            ok = i < T and 0 <= j < length and (not causal or j <= causal_limit(i, causal))
                            if ok:
                                return False
    return True
