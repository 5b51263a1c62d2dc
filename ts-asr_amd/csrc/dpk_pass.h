// The d(pk) pass of the relative-position attention backward: the bodies that csrc/attention.hip's stand-alone and grouped launches share,
// in a header of their own so that the lab library (csrc/lab/lab.hip, tsasr_lab_dpk) can run either of them on caller-supplied tensors.
#pragma once
#include <algorithm>

#include "attn_common.h"

// The same 8 elements WITHOUT the zeroing of the dims at and beyond Dh (the address is clamped into the row; the caller masks when it
// consumes the values): load8_clamped's mask overwrites the load's destination, i.e. waits for the load on the spot - a sequence of
// calls was a sequence of round trips (20 of them at the head of relpos_attn_bwd_q). FAST as a compile-time flag: no branch per call.
template <typename T, bool FAST>
__device__ __forceinline__ void load8_raw(const T *__restrict__ row, int d0, int Dh, float (&v)[8]) {
    if constexpr (FAST) ld8(row + min(d0, Dh - 8), v);
    else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ld1(row + min(d0 + j, Dh - 1));
    }
}

// d(pk)[r][h*Dh + d] = sum_b sum_i dS[b][h][i][j = r + i - (T-1)] * (q + v)[b][i][h][d]  - the gradient of the projected positional
// table, straight from the materialised dS (the first version shifted dS back onto an (r, i) grid in HBM - 32 MB - and ran a library
// batched GEMM over it whose K dimension was half zeros: 20 + 31 + 5 us per layer). workgroup = (64 band rows, head, group of
// utterances); per utterance and block of 64 queries that can reach those rows: the 64 x 136 rectangle of dS goes to LDS as
// 16-byte pieces, the skew happens on the way into the A tile (A[rl][i] = dS[i][r0 + rl + i - (T-1)], 2-byte LDS reads, 16-byte
// writes), (q+v) rows are the B tile (k-major: transposing fragment reads), 4 MFMAs per wave; blocks of queries that cannot reach
// the rows are skipped (half of them). Partial sums per utterance group, summed by dpk_reduce_kernel in a fixed order.
#define SH_LD 136
#define DPK_LD 72
template <typename T>
__device__ __forceinline__ void dpk_body(const T *__restrict__ ds, const T *__restrict__ qv /*[H][B*T][Dh]*/,
                                         const int32_t *__restrict__ key_lens, float *__restrict__ part /*[G][R][H*64]*/,
                                         int Bn, int Tn, int Tp, int H, int Dh, int causal, int bgroup, int isplit, int i_span,
                                         int bx, int by, int bz) {
    // (bx, by, bz) = the block index of the one-job launch; isplit > 1 (long sequences, few utterances): bz = utterance group * isplit +
    // query range; a workgroup walks the query blocks of [ipart * i_span, (ipart + 1) * i_span) only - the band rows around r = T-1 are
    // reached by every query block
    __shared__ __attribute__((aligned(16))) T raw[64 * SH_LD];
    __shared__ __attribute__((aligned(16))) bf16_t a_tile[64 * DPK_LD], b_tile[64 * DPK_LD];
    const int r0 = bx * 64, h = by, grp = bz / isplit, ipart = bz % isplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int rblk = wave & 1, dblk = wave >> 1;
    const int R = 2 * Tn - 1;
    const int grp4 = lane >> 4, mhalf = grp4 & 1, q4 = (lane & 15) >> 2, p4 = lane & 3;
    constexpr int VE = 16 / (int)sizeof(T), NG = SH_LD / VE;
    f32x16 acc = {0};
    const int b_end = min(Bn, (grp + 1) * bgroup);
    const int i_lo = ipart * i_span, i_hi = min(Tn, i_lo + i_span);
    // band rows whose every (query, key) pair lies beyond the causal limit (j - i = r - (T-1) > chunk - 1) only ever see zeros
    const bool dead = causal && r0 - (Tn - 1) > max(causal, 1) - 1;
    // (a version that requested the next pair's global loads before building this pair's tiles - LDS-only barriers in between -
    // measured 5 % slower than this plain loop: two to four workgroups share a CU and cover each other's round trips)
    for (int b = grp * bgroup; b < b_end && !dead; ++b) {
        const int len = key_lens ? min(max(key_lens[b], 1), Tn) : Tn;
        const T *src = ds + (((long long)b * H + h) * Tn) * Tp;
        const T *qrow = qv + ((long long)h * Bn + b) * Tn * Dh;
        for (int i0 = i_lo; i0 < i_hi; i0 += 64) {
            const int jlo = r0 + i0 - (Tn - 1);                  // key of (rl = 0, il = 0); keys jlo .. jlo + 126 are touched
            if (jlo + 126 < 0 || jlo >= len) continue;           // no query of this block reaches these band rows (workgroup-uniform)
            const int jal = (jlo >= 0 ? jlo : jlo - 7) / 8 * 8, off = jlo - jal;
            __syncthreads();                                     // previous tiles consumed
            for (int e = tid; e < 64 * NG; e += 256) {           // always-issued clamped loads; validity decided below
                const int il = e / NG, gq = e % NG, j = jal + gq * VE;
                *reinterpret_cast<uint4 *>(raw + il * SH_LD + gq * VE) =
                    *reinterpret_cast<const uint4 *>(src + (long long)min(i0 + il, Tn - 1) * Tp + min(max(j, 0), Tp - VE));
            }
#pragma unroll
            for (int it = 0; it < 2; ++it) {                     // (q + v) rows i0 .. i0+63: 64 x 8 pieces of 8 dims
                const int e = tid + 256 * it, il = e >> 3, c = (e & 7) * 8;
                float v8[8];
                if ((Dh % 8) == 0) load8_raw<T, true>(qrow + (long long)min(i0 + il, Tn - 1) * Dh, c, Dh, v8);     // (both pieces of the
                else load8_raw<T, false>(qrow + (long long)min(i0 + il, Tn - 1) * Dh, c, Dh, v8);                  //  thread in flight together)
#pragma unroll
                for (int q = 0; q < 8; ++q) v8[q] = (c + q < Dh) ? v8[q] : 0.f;
                if (i0 + il >= Tn) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) v8[q] = 0.f;
                }
                st8(b_tile + il * DPK_LD + c, v8);
            }
            __syncthreads();
            {   // A tile: thread = (band row rl, 16 consecutive queries)
                // All 16 reads are issued together and masked afterwards by a bit mask: written as `valid ? raw[..] : 0` with the four-term
                // validity test, each read sat in its own exec-masked block behind ~50 instructions of branches and was waited for on the
                // spot - 16 serialized LDS round trips per tile for 4 MFMAs. Without a look-ahead mask the valid elements of a thread are a
                // contiguous range of q (j = jlo + rl + il0 + q in [0, len), i0 + il0 + q < Tn).
                const int rl = tid >> 2, il0 = (tid & 3) * 16;
                float v16[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v16[q] = (float)raw[(il0 + q) * SH_LD + off + rl + il0 + q];     // always inside the 64 x 136 rectangle
                pin_all(v16);
                const int jq0 = jlo + rl + il0;                                                   // key of q = 0
                const int q_lo = min(max(-jq0, 0), 16), q_hi = min(max(min(len - jq0, Tn - i0 - il0), 0), 16);
                unsigned vm = q_hi > q_lo ? (0xffffu >> (16 - q_hi)) & (0xffffu << q_lo) : 0u;
                if (causal) {       // workgroup-uniform
#pragma unroll
                    for (int q = 0; q < 16; ++q) vm &= ~((jq0 + q > causal_limit(i0 + il0 + q, causal) ? 1u : 0u) << q);
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) v16[q] = __uint_as_float(__float_as_uint(v16[q]) & (unsigned)((int)(vm << (31 - q)) >> 31));
                st8(a_tile + rl * DPK_LD + il0, *reinterpret_cast<float(*)[8]>(&v16[0]));
                st8(a_tile + rl * DPK_LD + il0 + 8, *reinterpret_cast<float(*)[8]>(&v16[8]));
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bf16x8 af = *reinterpret_cast<const bf16x8 *>(a_tile + (32 * rblk + r) * DPK_LD + 16 * s + 8 * hh);
                const bf16_t *bp = b_tile + (16 * s + 8 * hh + q4) * DPK_LD + 32 * dblk + 16 * mhalf + 4 * p4;
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(bp));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(bp + 4 * DPK_LD));
                bf16x8 bfr;
                bfr[0] = lo[0]; bfr[1] = lo[1]; bfr[2] = lo[2]; bfr[3] = lo[3]; bfr[4] = hi[0]; bfr[5] = hi[1]; bfr[6] = hi[2]; bfr[7] = hi[3];
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc, 0, 0, 0);
            }
        }
    }
    // accumulator: rows = band rows 32*rblk + (g&3) + 8(g>>2) + 4hh, column = head dim 32*dblk + r
    float *pw = part + ((long long)bz * R) * (H * 64) + h * 64 + 32 * dblk + r;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int rg = r0 + 32 * rblk + (g & 3) + 8 * (g >> 2) + 4 * hh;
        if (rg < R) pw[(long long)rg * (H * 64)] = acc[g];
    }
}

// dpk[r][h*Dh + d] = sum over the utterance groups of part[g][r][h*64 + d], written in the io dtype (blocks `blk` of `nblk` of one job)
template <typename T>
__device__ __forceinline__ void dpk_reduce_body(const float *__restrict__ part, T *__restrict__ dpk, int R, int H, int Dh, int G, int blk, int nblk) {
    const long long n = (long long)R * H * 64;
    for (long long e = blk * 256LL + threadIdx.x; e < n; e += (long long)nblk * 256) {
        const int c = (int)(e % (H * 64)), d = c & 63, hq = c >> 6;
        const long long rr = e / (H * 64);
        if (d >= Dh) continue;
        float sum = 0.f;
        for (int g = 0; g < G; ++g) sum += part[(long long)g * n + e];
        st1(dpk + rr * (H * Dh) + hq * Dh + d, sum);
    }
}

// ---- one-pass form for the short path (bf16, Dh = 64, 2 <= T <= 256): every element of dS and every row of q+v is fetched ONCE ------
// workgroup = (head, utterance group), 8 waves; it owns EVERY band row (2T-1 <= 511 rows x 64 dims fp32 = 64 accumulator registers per
// lane): the sixteen 32-row blocks are dealt round-robin, wave = (block mod 4, head-dim half), because a block of 64 queries reaches only
// T + 63 consecutive band rows and contiguous ranges would leave most waves idle. Per (utterance, block of 64 queries) - utterances
// ascending, blocks ascending, as dpk_body walks them - the 64 x Tp rows of dS go to LDS once, already masked (key >= key_lens[b],
// query >= T, beyond the look-ahead limit: zero) between two zero margins of DPO_PAD columns, and the 64 rows of q+v next to them.
// A wave then builds, for each of its 32-row blocks and each 16 queries, the A fragment of dpk_body's skewed tile straight from those
// rows (A[rl][il] = dS[il][rb*32 + rl + i0 + il - (T-1)], 2-byte LDS reads) and issues the same v_mfma_f32_32x32x16_bf16 on the same
// operands in the same order per accumulator as dpk_body does; fragments that are zero throughout (no key in [0, len)) are skipped,
// which leaves the fp32 sums as they are (x + 0 = x; an accumulator that starts at +0 never holds -0). Same utterance groups, same
// partial planes: d(pk) and every partial plane are bit-identical to dpk_body's. The next pair's global loads are requested before this
// pair's MFMAs and parked in registers (two workgroups per CU cover the rest); no workgroup waits for another.
#define DPO_TH 512
#define DPO_PAD 48                      // >= 46: a 32-row x 16-query fragment that touches a key in [0, len) starts at key >= -46, ends <= len + 45
#define DPO_LD (DPO_PAD + 256 + DPO_PAD + 8)
__device__ __forceinline__ void dpk_once_body(const bf16_t *__restrict__ ds, const bf16_t *__restrict__ qv /*[H][B*T][64]*/,
                                              const int32_t *__restrict__ key_lens, float *__restrict__ part /*[G][R][H*64]*/,
                                              int Bn, int Tn, int Tp, int H, int causal, int bgroup, int h, int grp) {
    __shared__ __attribute__((aligned(16))) bf16_t raw[64 * DPO_LD];
    __shared__ __attribute__((aligned(16))) bf16_t b_tile[64 * DPK_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int cls = wave & 3, dblk = wave >> 2;
    const int grp4 = lane >> 4, mhalf = grp4 & 1, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int R = 2 * Tn - 1, nib = (Tn + 63) / 64;
    const int b0 = grp * bgroup, nb = min(Bn, b0 + bgroup) - b0, npairs = nb * nib;
    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = (f32x16){0};
    for (int e = tid; e < 64 * DPO_LD / 8; e += DPO_TH) reinterpret_cast<uint4 *>(raw)[e] = make_uint4(0u, 0u, 0u, 0u);     // the margins stay zero
    // this thread's pieces of a pair: four 16-byte pieces of dS (rows sil + 16 it, keys sj .. sj + 7; the lanes with sj >= Tp repeat a
    // neighbour's load and store nothing), one of q+v
    const int sil = tid >> 5, sj = (tid & 31) * 8;
    const int qil = tid >> 3, qc = (tid & 7) * 8;
    uint4 pre[4], preq;
    int len = 0, i0 = 0;
    auto request = [&](int p) {       // always-issued clamped loads, masked when they are stored
        const int b = b0 + p / nib, pi0 = (p % nib) * 64;
        const int plen = key_lens ? min(max(key_lens[b], 1), Tn) : Tn;
        const bf16_t *src = ds + (((long long)b * H + h) * Tn) * Tp;
        const int jmax = ((plen - 1) >> 3) << 3;
#pragma unroll
        for (int it = 0; it < 4; ++it)
            pre[it] = *reinterpret_cast<const uint4 *>(src + (long long)min(pi0 + sil + 16 * it, Tn - 1) * Tp + min(sj, jmax));
        preq = *reinterpret_cast<const uint4 *>(qv + (((long long)h * Bn + b) * Tn + min(pi0 + qil, Tn - 1)) * 64 + qc);
    };
    if (npairs > 0) request(0);
    for (int p = 0; p < npairs; ++p) {
        const int b = b0 + p / nib;
        i0 = (p % nib) * 64;
        len = key_lens ? min(max(key_lens[b], 1), Tn) : Tn;
        __syncthreads();                                         // previous pair consumed (first pair: the margins are cleared)
#pragma unroll
        for (int it = 0; it < 4; ++it)
            if (sj < Tp) {
                const int i = i0 + sil + 16 * it;
                const int lim = i < Tn ? (causal ? min(len - 1, causal_limit(i, causal)) : len - 1) : -1;      // last valid key of the row
                const int nv = min(max(lim + 1 - sj, 0), 8);
                unsigned w[4] = {pre[it].x, pre[it].y, pre[it].z, pre[it].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] &= nv >= 2 * q + 2 ? 0xffffffffu : (nv == 2 * q + 1 ? 0x0000ffffu : 0u);
                *reinterpret_cast<uint4 *>(raw + (sil + 16 * it) * DPO_LD + DPO_PAD + sj) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        *reinterpret_cast<uint4 *>(b_tile + qil * DPK_LD + qc) = i0 + qil < Tn ? preq : make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        if (p + 1 < npairs) request(p + 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) {          // (s outside, blocks inside: per accumulator the fragments still come in ascending s)
            const bf16_t *bp = b_tile + (16 * s + 8 * hh + q4) * DPK_LD + 32 * dblk + 16 * mhalf + 4 * p4;
            const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(bp));
            const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(bp + 4 * DPK_LD));
            bf16x8 bfr;
            bfr[0] = lo[0]; bfr[1] = lo[1]; bfr[2] = lo[2]; bfr[3] = lo[3]; bfr[4] = hi[0]; bfr[5] = hi[1]; bfr[6] = hi[2]; bfr[7] = hi[3];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int rb = cls + 4 * a;
                const int jlo = rb * 32 + i0 - (Tn - 1) + 16 * s;        // key of (rl = 0, il = 16 s); keys jlo .. jlo + 46 are touched
                // (wave-uniform) rows beyond the table; no key in [0, len); every pair of these band rows beyond the look-ahead limit
                if (rb * 32 >= R || jlo + 46 < 0 || jlo >= len || (causal && rb * 32 - (Tn - 1) > max(causal, 1) - 1)) continue;
                const bf16_t *ap = raw + (16 * s + 8 * hh) * (DPO_LD + 1) + DPO_PAD + (jlo - 16 * s) + r;
                bf16x8 af;
#pragma unroll
                for (int e = 0; e < 8; ++e) af[e] = ap[e * (DPO_LD + 1)];
                acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[a], 0, 0, 0);
            }
        }
    }
    // accumulator a: rows = band rows 32 (cls + 4a) + (g&3) + 8(g>>2) + 4hh, column = head dim 32*dblk + r; every row < R is written
    float *pw = part + ((long long)grp * R) * (H * 64) + h * 64 + 32 * dblk + r;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int rg = 32 * (cls + 4 * a) + (g & 3) + 8 * (g >> 2) + 4 * hh;
            if (rg < R) pw[(long long)rg * (H * 64)] = acc[a][g];
        }
}

// utterances per d(pk) workgroup (both bodies): see attn_bgroup in csrc/attention.hip
static inline int dpk_bgroup(int B, int T) {
    const int dpk_wgs = 256;
    const int want = std::max(1, dpk_wgs / (4 * cdiv(2 * T - 1, 64)));
    return std::max(1, cdiv(B, std::min(B, want)));
}
// the one-pass body's gate (io dtype and head size are the caller's to check: bf16, Dh = 64)
static inline bool dpk_once_shape(int T) { return T >= 2 && T <= 256; }
