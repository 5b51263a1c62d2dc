// Chunk-by-chunk inference of the causal encoder (gfx950): the two kernels whose offline versions look at the whole utterance.
//
// (1) attn_stream_kernel: relative-position attention of a chunk of C query frames at absolute offset t0 against a per-layer key/value
//     cache. Same score as csrc/attention_f32.hip / csrc/attention.hip (SB/nnet/attention.py:586-633 with the rel_shift closed form):
//       s(i, j) = scale * ((q_i + u).k_j + (q_i + v).pk_half[|i - j|]),   i = t0 + r
//     RelPosEncXL's table is symmetric (nnet.RelPosEncXL), so the positional row of the offline table, pk[j - i + T - 1], equals the
//     row |i - j| of the half table linear_pos(PE(d)), d = 0 .. Tmax - 1: one table serves every chunk at every offset. Masks: keys
//     j >= key_lens[b], and keys past the causal (causal = 1) or block-causal (causal = c > 1, chunks of c absolute frames) limit of i.
//     Cache layout: separate K and V planes [B, H, Tmax, Dh] in the io dtype (Q is never cached; a head's keys are contiguous rows).
//     The workgroup (query block 0, split 0) of each (b, h) appends the chunk's K, V rows at t0; every workgroup of the launch reads
//     those rows from qkv, and only rows < t0 from the cache, so nothing is read that this launch writes.
//     bf16 with Dh = 32 / 64: attn_stream_mfma_kernel (matrix cores, all <= 64 queries of a (b, h) in one workgroup; see below).
//     fp32 (and other bf16 head sizes): attn_stream_kernel, flash-style in exact fp32 arithmetic: a workgroup owns 16 query rows of one
//     (b, h), walks its keys in tiles of 64 through LDS (K, V and the 79 rows of the positional band a tile can touch), online softmax
//     per row in a wave. Long caches in small batches are split along the keys across workgroups (partials m, l, o in the workspace,
//     merged by a second launch); the split depends on (B, C, H, Tmax) only, never on t0.
// (2) convmod_stream_kernel: tsasr_convmod_fwd with causal = 1 on a chunk - bias + GLU + depthwise conv (K taps) + LayerNorm + LeakyReLU
//     - reading the K - 1 GLU rows before the chunk from a history buffer instead of the zero pad, and writing the next chunk's history
//     to a second buffer (the caller swaps the two per chunk). A zeroed history is the offline causal zero pad.
// Slots (tsasr_relpos_attn_stream_slots_fwd, tsasr_convmod_stream_slots_fwd): the same kernel bodies with a device array t0s [B] in place
//     of the scalar t0 (a null t0s selects the scalar), for batches whose rows are sessions that join and leave: row b runs at its own
//     offset t0s[b] >= 0, or is idle (t0s[b] < 0, or a chunk that would pass Tmax): its workgroups leave at once, its cache and history
//     keep their bits (hist_out = hist_in), its output rows are exact zeros. The offset is uniform per workgroup and read once.
#include "common.h"

namespace {

constexpr int SQB = 16;      // query rows per workgroup (4 per wave)
constexpr int SKT = 64;      // keys per tile = lanes
constexpr int SDMAX = 64;    // head dim <= 64 (lane = d)
constexpr int SLDD = SDMAX + 1;
constexpr int SPB = SKT + SQB - 1;   // positional rows a (query block, key tile) pair touches

struct StreamAttnArgs {
    const void *qkv;             // [B, C, H, 3*Dh]
    void *kc, *vc;               // [B, H, Tmax, Dh]
    const void *pkh;             // [Tmax, H*Dh]
    const float *bu, *bv;        // [H*Dh]
    const int *key_lens;         // [B] or NULL
    void *out;                   // [B, C, H*Dh]
    float *part;                 // [B, H, C, nsplit, Dh + 2] when nsplit > 1
    int B, C, H, Dh, Tmax, t0, causal, nsplit, tps;
    float scale;
    const int *t0s;              // [B] per-slot offsets (tsasr_relpos_attn_stream_slots_fwd) or NULL: every row at t0
};

// the offset of batch row b, read once per workgroup (uniform); slot launches: < 0 = an idle slot, and a slot whose chunk would pass
// the cache is treated as idle, so no row past Tmax can be written
__device__ __forceinline__ int s_offset(const StreamAttnArgs &a, int b) {
    if (!a.t0s) return a.t0;
    const int t = a.t0s[b];
    return (t < 0 || (long long)t + a.C > a.Tmax) ? -1 : t;
}

__device__ __forceinline__ int s_causal_limit(int i, int causal) { return causal <= 1 ? i : (i / causal + 1) * causal - 1; }

template <typename T>
__global__ __launch_bounds__(256) void attn_stream_kernel(const StreamAttnArgs a) {
    __shared__ float Ks[SKT][SLDD], Vs[SKT][SLDD], Ps[SPB][SLDD], Qu[SQB][SLDD], Qv[SQB][SLDD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * SQB, h = blockIdx.y, b = blockIdx.z / a.nsplit, sp = blockIdx.z % a.nsplit;
    const int Dh = a.Dh, C = a.C, t0 = s_offset(a, b), D = a.H * Dh;
    const long long ld = 3LL * D;
    if (t0 < 0) {                                   // idle slot: cache untouched, out rows exact zeros (split: the merge writes them)
        if (a.nsplit == 1)
            for (int e = threadIdx.x; e < SQB * Dh; e += 256) {
                const int ic = i0 + e / Dh;
                if (ic < C) st1((T *)a.out + ((long long)b * C + ic) * D + h * Dh + e % Dh, 0.f);
            }
        return;
    }
    const T *qkv = (const T *)a.qkv + (long long)b * C * ld + (long long)h * 3 * Dh;
    T *kc = (T *)a.kc + ((long long)b * a.H + h) * a.Tmax * Dh;
    T *vc = (T *)a.vc + ((long long)b * a.H + h) * a.Tmax * Dh;
    const T *pkh = (const T *)a.pkh + (long long)h * Dh;
    if (blockIdx.x == 0 && sp == 0) {               // append the chunk's keys / values (rows t0 .. t0 + C - 1 < Tmax, checked on the host)
        for (int e = threadIdx.x; e < C * Dh; e += 256) {
            const int r = e / Dh, d = e % Dh;
            kc[(long long)(t0 + r) * Dh + d] = qkv[r * ld + Dh + d];
            vc[(long long)(t0 + r) * Dh + d] = qkv[r * ld + 2 * Dh + d];
        }
    }
    for (int e = threadIdx.x; e < SQB * SDMAX; e += 256) {
        const int r = e / SDMAX, d = e % SDMAX;
        const float q = (d < Dh && i0 + r < C) ? ld1(qkv + (i0 + r) * ld + d) : 0.f;
        Qu[r][d] = q + (d < Dh ? a.bu[h * Dh + d] : 0.f);
        Qv[r][d] = q + (d < Dh ? a.bv[h * Dh + d] : 0.f);
    }
    const int kend = t0 + C;                         // keys that exist after this chunk
    const int klen = max(0, a.key_lens ? min(a.key_lens[b], kend) : kend);
    const int ilast = t0 + min(i0 + SQB, C) - 1;     // last query row of this block (absolute)
    const int jend = a.causal ? min(klen, min(kend, s_causal_limit(ilast, a.causal) + 1)) : klen;
    const int ntiles = (jend + SKT - 1) / SKT;
    const int tb = sp * a.tps, te = min(ntiles, tb + a.tps);
    float m[4], l[4], o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; o[r] = 0.f; }
    for (int jt = tb; jt < te; ++jt) {
        const int j0 = jt * SKT;
        __syncthreads();
        for (int e = threadIdx.x; e < SKT * SDMAX; e += 256) {
            const int r = e / SDMAX, d = e % SDMAX, j = j0 + r;
            float kv = 0.f, vv = 0.f;
            if (d < Dh && j < jend) {
                if (j < t0) { kv = ld1(kc + (long long)j * Dh + d); vv = ld1(vc + (long long)j * Dh + d); }
                else { kv = ld1(qkv + (j - t0) * ld + Dh + d); vv = ld1(qkv + (j - t0) * ld + 2 * Dh + d); }
            }
            Ks[r][d] = kv;
            Vs[r][d] = vv;
        }
        const int dlo = (t0 + i0) - (j0 + SKT - 1);  // i - j of positional row 0 of the band
        for (int e = threadIdx.x; e < SPB * SDMAX; e += 256) {
            const int r = e / SDMAX, d = e % SDMAX;
            const int dist = abs(dlo + r);
            Ps[r][d] = (d < Dh && dist < a.Tmax) ? ld1(pkh + (long long)dist * D + d) : 0.f;
        }
        __syncthreads();
        const int j = j0 + lane;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ii = wave * 4 + r, i = t0 + i0 + ii;
            if (i0 + ii >= C) continue;                       // wave-uniform
            const bool masked = j >= jend || (a.causal && j > s_causal_limit(i, a.causal));
            float s = 0.f;
            for (int d = 0; d < Dh; ++d) {
                s += Qu[ii][d] * Ks[lane][d];
                s += Qv[ii][d] * Ps[ii - lane + SKT - 1][d];
            }
            s = masked ? -INFINITY : s * a.scale;
            const float mn = fmaxf(m[r], wave_max(s));
            if (mn == -INFINITY) continue;                    // every key so far is masked
            const float alpha = m[r] == -INFINITY ? 0.f : expf(m[r] - mn);
            const float p = masked ? 0.f : expf(s - mn);
            l[r] = l[r] * alpha + wave_sum(p);
            m[r] = mn;
            float acc = o[r] * alpha;
            for (int jj = 0; jj < SKT; ++jj) acc += lane_bcast(p, jj) * Vs[jj][lane];
            o[r] = acc;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ic = i0 + wave * 4 + r;
        if (ic >= C) continue;
        if (a.nsplit == 1) {
            if (lane < Dh) st1((T *)a.out + ((long long)b * C + ic) * D + h * Dh + lane, l[r] > 0.f ? o[r] / l[r] : 0.f);
        } else {
            float *pp = a.part + ((((long long)b * a.H + h) * C + ic) * a.nsplit + sp) * (Dh + 2);
            if (lane < Dh) pp[lane] = o[r];
            if (lane == 0) { pp[Dh] = m[r]; pp[Dh + 1] = l[r]; }
        }
    }
}

// out[b, i, h, :] = sum_s o_s e^(m_s - M) / sum_s l_s e^(m_s - M) over the key splits (fixed order); one wave per (i, h, b), lane = d
template <typename T>
__global__ __launch_bounds__(64) void attn_stream_merge_kernel(const StreamAttnArgs a) {
    const int lane = threadIdx.x, i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, Dh = a.Dh;
    const float *pp = a.part + (((long long)b * a.H + h) * a.C + i) * a.nsplit * (Dh + 2);
    if (s_offset(a, b) < 0) {                       // idle slot: no partials were written for it
        if (lane < Dh) st1((T *)a.out + ((long long)b * a.C + i) * a.H * Dh + h * Dh + lane, 0.f);
        return;
    }
    float M = -INFINITY;
    for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, pp[s * (Dh + 2) + Dh]);
    float L = 0.f, O = 0.f;
    if (M != -INFINITY) {
        for (int s = 0; s < a.nsplit; ++s) {
            const float ms = pp[s * (Dh + 2) + Dh];
            if (ms == -INFINITY) continue;
            const float w = expf(ms - M);
            L += pp[s * (Dh + 2) + Dh + 1] * w;
            if (lane < Dh) O += pp[s * (Dh + 2) + lane] * w;
        }
    }
    if (lane < Dh) st1((T *)a.out + ((long long)b * a.C + i) * a.H * Dh + h * Dh + lane, L > 0.f ? O / L : 0.f);
}

// ---- bf16 on the matrix cores -----------------------------------------------------------------------------------------------
// workgroup = (b, h, 64 queries, key split), 4 waves = (query block qb of 32) x (key part kp): wave kp takes the 32-key sub-blocks
// kp, kp + 2, ... of the workgroup's keys, so the K / V rows a (b, h) needs are fetched once for all its (<= 64) chunk queries (the two
// query-block waves of a key part read the same rows in step, from L2). v_mfma_f32_32x32x16_bf16 with a lane owning ONE query:
//   AC^T [32 keys][32 queries] = K . (Q+u)^T      (A = K rows, B = (Q+u)^T; 16-byte operand loads straight from the cache / qkv)
//   G    [64 band rows][32 queries] = Pband . (Q+v)^T, band row k = pk_half[|i0 - jb - 31 + k|]; BD(key jr, query c) = G[c - jr + 31][c]
//        (through the wave's LDS: the skew crosses lanes)
//   O^T  [Dh][32 queries] += V^T . P^T             (P rounded to bf16 as csrc/attention.hip does; the contraction runs over the keys in
//        the accumulator's row order, so the B operand is the lane's own 8 probabilities and V^T is read from the wave's LDS copy of
//        the sub-block in that order)
// Accumulator element g of lane (r = lane & 31, hh = lane >> 5) is row (g & 3) + 8 (g >> 2) + 4 hh, column r. Online softmax per
// query in fp32 (the two lanes of a query combine their 16 keys by one exchange); the two key parts merge through LDS at the end.
constexpr int MQB = 64;      // queries per workgroup

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int DH>
__global__ __launch_bounds__(256) void attn_stream_mfma_kernel(const StreamAttnArgs a) {
    constexpr int NS = DH / 16, NDB = DH / 32, VLD = DH + 8;
    __shared__ float Gs[4][64][33];                   // per wave: band products; reused for the key-part merge
    __shared__ __attribute__((aligned(16))) bf16_t Vs[4][32][VLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, hh = lane >> 5, qb = wave & 1, kp = wave >> 1;
    const int i0 = blockIdx.x * MQB, h = blockIdx.y, b = blockIdx.z / a.nsplit, sp = blockIdx.z % a.nsplit;
    const int C = a.C, t0 = s_offset(a, b), D = a.H * DH;
    const long long ld = 3LL * D;
    if (t0 < 0) {                                     // idle slot (as attn_stream_kernel)
        if (a.nsplit == 1)
            for (int e = threadIdx.x; e < MQB * DH; e += 256) {
                const int ic = i0 + e / DH;
                if (ic < C) st1((bf16_t *)a.out + ((long long)b * C + ic) * D + h * DH + e % DH, 0.f);
            }
        return;
    }
    const bf16_t *qkv = (const bf16_t *)a.qkv + (long long)b * C * ld + (long long)h * 3 * DH;
    bf16_t *kc = (bf16_t *)a.kc + ((long long)b * a.H + h) * a.Tmax * DH;
    bf16_t *vc = (bf16_t *)a.vc + ((long long)b * a.H + h) * a.Tmax * DH;
    const bf16_t *pkh = (const bf16_t *)a.pkh + (long long)h * DH;
    if (blockIdx.x == 0 && sp == 0) {                 // append the chunk's keys / values (as attn_stream_kernel)
        for (int e = threadIdx.x; e < C * DH; e += 256) {
            const int rr = e / DH, d = e % DH;
            kc[(long long)(t0 + rr) * DH + d] = qkv[rr * ld + DH + d];
            vc[(long long)(t0 + rr) * DH + d] = qkv[rr * ld + 2 * DH + d];
        }
    }
    const int ic = i0 + 32 * qb + r, i = t0 + ic;     // this lane's query (chunk row / absolute frame)
    const bool qvalid = ic < C;
    bf16x8 qu[NS], qv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = 16 * s + 8 * hh + e;
            const float q = qvalid ? ld1(qkv + (long long)ic * ld + d) : 0.f;
            qu[s][e] = (bf16_t)(qvalid ? q + a.bu[h * DH + d] : 0.f);
            qv[s][e] = (bf16_t)(qvalid ? q + a.bv[h * DH + d] : 0.f);
        }
    const int kend = t0 + C;
    const int klen = max(0, a.key_lens ? min(a.key_lens[b], kend) : kend);
    const int ilast = t0 + min(i0 + MQB, C) - 1;
    const int jend = a.causal ? min(klen, min(kend, s_causal_limit(ilast, a.causal) + 1)) : klen;
    const int lim = a.causal ? s_causal_limit(i, a.causal) : 0x3fffffff;
    const int kbeg = sp * a.tps * SKT, kfin = min(jend, (sp + 1) * a.tps * SKT);
    const int nsb = kfin > kbeg ? (kfin - kbeg + 31) / 32 : 0;
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o_acc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g = 0; g < 16; ++g) o_acc[db][g] = 0.f;
    float(*G)[33] = Gs[wave];
    bf16_t(*V)[VLD] = Vs[wave];
    for (int sb = kp; sb < nsb; sb += 2) {
        const int jb = kbeg + 32 * sb;
        wave_lds_sync();                               // the previous sub-block's reads of G / V are done
        // V rows jb .. jb+31 -> the wave's LDS (zeros past jend)
        for (int pc = lane; pc < 32 * (DH / 8); pc += 64) {
            const int rr = pc / (DH / 8), c8 = (pc % (DH / 8)) * 8, j = jb + rr;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (j < jend) v = *reinterpret_cast<const uint4 *>(j < t0 ? vc + (long long)j * DH + c8 : qkv + (long long)(j - t0) * ld + 2 * DH + c8);
            *reinterpret_cast<uint4 *>(&V[rr][c8]) = v;
        }
        f32x16 s_acc, g_acc0, g_acc1;
#pragma unroll
        for (int g = 0; g < 16; ++g) { s_acc[g] = 0.f; g_acc0[g] = 0.f; g_acc1[g] = 0.f; }
        const int jk = jb + r;                         // key row this lane feeds into AC
        const int dd0 = (t0 + i0 + 32 * qb) - jb - 31; // i - j of band row 0 (absolute frames)
        const int dist0 = abs(dd0 + r), dist1 = abs(dd0 + 32 + r);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int d = 16 * s + 8 * hh;
            bf16x8 ka = {}, p0 = {}, p1 = {};
            if (jk < jend) ka = *reinterpret_cast<const bf16x8 *>(jk < t0 ? kc + (long long)jk * DH + d : qkv + (long long)(jk - t0) * ld + DH + d);
            if (dist0 < a.Tmax) p0 = *reinterpret_cast<const bf16x8 *>(pkh + (long long)dist0 * D + d);
            if (dist1 < a.Tmax) p1 = *reinterpret_cast<const bf16x8 *>(pkh + (long long)dist1 * D + d);
            s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qu[s], s_acc, 0, 0, 0);
            g_acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p0, qv[s], g_acc0, 0, 0, 0);
            g_acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p1, qv[s], g_acc1, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int k = (g & 3) + 8 * (g >> 2) + 4 * hh;
            G[k][r] = g_acc0[g];
            G[32 + k][r] = g_acc1[g];
        }
        wave_lds_sync();
        float sc[16], mloc = -INFINITY;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int jr = (g & 3) + 8 * (g >> 2) + 4 * hh, j = jb + jr;
            const bool masked = !qvalid || j >= jend || j > lim;
            sc[g] = masked ? -INFINITY : (s_acc[g] + G[r - jr + 31][r]) * a.scale;
            mloc = fmaxf(mloc, sc[g]);
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = (m_run == -INFINITY) ? (m_new == -INFINITY ? 1.f : 0.f) : expf(m_run - m_new);
        float psum = 0.f;
        bf16x8 pb[2];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const float p = sc[g] == -INFINITY ? 0.f : expf(sc[g] - m_new);
            psum += p;
            pb[g >> 3][g & 7] = (bf16_t)p;
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
#pragma unroll
            for (int g = 0; g < 16; ++g) o_acc[db][g] *= alpha;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 va;
#pragma unroll
                for (int e = 0; e < 8; ++e) va[e] = V[(e & 3) + 8 * (2 * ks + (e >> 2)) + 4 * hh][32 * db + r];
                o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pb[ks], o_acc[db], 0, 0, 0);
            }
        }
    }
    l_run += __shfl_xor(l_run, 32);
    // merge the two key parts of each query block: part 1 leaves (O, m, l) in LDS, part 0 combines and writes
    __syncthreads();
    float *Om = &Gs[0][0][0];                          // [2 qb][32 queries][DH + 1]
    float *Mm = Om + 2 * 32 * (DH + 1), *Lm = Mm + 64;
    if (kp == 1) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 16; ++g) Om[(qb * 32 + r) * (DH + 1) + 32 * db + (g & 3) + 8 * (g >> 2) + 4 * hh] = o_acc[db][g];
        if (hh == 0) { Mm[qb * 32 + r] = m_run; Lm[qb * 32 + r] = l_run; }
    }
    __syncthreads();
    if (kp == 1 || !qvalid) return;
    const float m1 = Mm[qb * 32 + r], l1 = Lm[qb * 32 + r], M = fmaxf(m_run, m1);
    const float w0 = m_run == -INFINITY ? 0.f : expf(m_run - M), w1 = m1 == -INFINITY ? 0.f : expf(m1 - M);
    const float L = l_run * w0 + l1 * w1;
    float *pp = a.nsplit > 1 ? a.part + ((((long long)b * a.H + h) * C + ic) * a.nsplit + sp) * (DH + 2) : nullptr;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int d = 32 * db + (g & 3) + 8 * (g >> 2) + 4 * hh;
            const float o = o_acc[db][g] * w0 + Om[(qb * 32 + r) * (DH + 1) + d] * w1;
            if (pp) pp[d] = o;
            else st1((bf16_t *)a.out + ((long long)b * C + ic) * D + h * DH + d, L > 0.f ? o / L : 0.f);
        }
    if (pp && hh == 0) { pp[DH] = M; pp[DH + 1] = L; }
}

// key splits of one launch: only small grids are split, into pieces of >= 2 key tiles; a function of (B, C, H, Tmax) alone
void stream_split(int B, int C, int H, int Tmax, int *nsplit, int *tps) {
    const int base = B * H * cdiv(C, MQB), maxt = cdiv(Tmax, SKT);
    int n = 1;
    if (base < 256 && maxt > 4) n = min(cdiv(256, base), cdiv(maxt, 2));
    const int t = cdiv(maxt, n);
    *tps = t;
    *nsplit = cdiv(maxt, t);
}

// ---- convolution module core with carried history ----------------------------------------------------------------------------
struct ConvStreamArgs {
    const void *y2;              // [B, C, 2D]
    const float *b2, *w, *cb, *g, *be;
    const float *hin;            // [B, K-1, D] fp32: GLU rows t0-K+1 .. t0-1
    float *hout;                 // [B, K-1, D] fp32: GLU rows t0+C-K+1 .. t0+C-1
    void *z;                     // [B, C, D]
    int B, C, D, K;
    float eps, slope;
    const int *t0s;              // [B] slot offsets (tsasr_convmod_stream_slots_fwd; < 0 = idle slot) or NULL
};

__device__ __forceinline__ float sig_f(float x) { return 1.f / (1.f + __expf(-x)); }

// GLU row e of the extended sequence [history (K-1 rows) | chunk (C rows)], channel d
template <typename T>
__device__ __forceinline__ float ext_glu(const ConvStreamArgs &a, const T *y2, const float *hin, int e, int d) {
    const int hk = a.K - 1;
    if (e < hk) return hin[(long long)e * a.D + d];
    const T *row = y2 + (long long)(e - hk) * 2 * a.D;
    const float x = ld1(row + d) + (a.b2 ? a.b2[d] : 0.f), gt = ld1(row + a.D + d) + (a.b2 ? a.b2[a.D + d] : 0.f);
    return x * sig_f(gt);
}

// one workgroup per output row (r, b): depthwise taps, then LayerNorm over D and the activation; rows r < K-1 also write history rows
template <typename T>
__global__ __launch_bounds__(256) void convmod_stream_kernel(const ConvStreamArgs a) {
    extern __shared__ float crow[];                   // [D] conv output of this row
    __shared__ float red[4];
    const int r = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, K = a.K, hk = K - 1;
    const T *y2 = (const T *)a.y2 + (long long)b * a.C * 2 * D;
    const float *hin = a.hin + (long long)b * hk * D;
    float *hout = a.hout + (long long)b * hk * D;
    if (a.t0s && a.t0s[b] < 0) {                      // idle slot: zero rows, the history carried over bit for bit
        T *zr = (T *)a.z + ((long long)b * a.C + r) * D;
        for (int d = tid; d < D; d += 256) st1(zr + d, 0.f);
        for (int mrow = r; mrow < hk; mrow += a.C)
            for (int d = tid; d < D; d += 256) hout[(long long)mrow * D + d] = hin[(long long)mrow * D + d];
        return;
    }
    float s1 = 0.f;
    for (int d = tid; d < D; d += 256) {
        float acc = a.cb ? a.cb[d] : 0.f;
        for (int k = 0; k < K; ++k) acc += a.w[(long long)d * K + k] * ext_glu<T>(a, y2, hin, r + k, d);   // output r reads ext rows r .. r+K-1
        const float c = (float)(T)acc;      // the conv output in the io dtype, as tsasr_convmod_fwd saves it
        crow[d] = c;
        s1 += c;
    }
    s1 = wave_sum(s1);
    if (lane == 0) red[wave] = s1;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / D;
    __syncthreads();
    float s2 = 0.f;
    for (int d = tid; d < D; d += 256) { const float t = crow[d] - mean; s2 += t * t; }
    s2 = wave_sum(s2);
    if (lane == 0) red[wave] = s2;
    __syncthreads();
    const float rs = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / D + a.eps);
    T *z = (T *)a.z + ((long long)b * a.C + r) * D;
    for (int d = tid; d < D; d += 256) {
        const float y = (crow[d] - mean) * rs * a.g[d] + a.be[d];
        st1(z + d, (a.slope < 0.f || y > 0.f) ? y : y * a.slope);   // slope < 0: no activation, as tsasr_convmod_fwd
    }
    for (int mrow = r; mrow < hk; mrow += a.C)        // next history row mrow = ext row C + mrow
        for (int d = tid; d < D; d += 256) hout[(long long)mrow * D + d] = ext_glu<T>(a, y2, hin, a.C + mrow, d);
}

}  // namespace

extern "C" {

size_t tsasr_relpos_attn_stream_workspace_bytes(int B, int C, int H, int Dh, int Tmax) {
    if (B <= 0 || C <= 0 || H <= 0 || Dh <= 0 || Tmax <= 0) return 0;
    int ns, tps;
    stream_split(B, C, H, Tmax, &ns, &tps);
    return ns > 1 ? (size_t)B * H * C * ns * (Dh + 2) * sizeof(float) : 0;
}

// one launcher for both entry points: t0s == NULL runs every row at the scalar t0
static int attn_stream_launch(const char *name, const void *qkv, void *k_cache, void *v_cache, const void *pk_half, const float *bias_u,
                              const float *bias_v, const int32_t *key_lens, void *out, int B, int C, int H, int Dh, int Tmax, int t0,
                              const int32_t *t0s, int causal, float scale, int io_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(qkv && k_cache && v_cache && pk_half && bias_u && bias_v && out, "%s: null pointer", name);
    TSASR_CHECK_ARG(B > 0 && C > 0 && H > 0 && Dh > 0 && Dh <= SDMAX && t0 >= 0 && causal >= 0 && (long long)t0 + C <= Tmax,
                    "%s: bad shape (B=%d C=%d H=%d Dh=%d Tmax=%d t0=%d causal=%d)", name, B, C, H, Dh, Tmax, t0, causal);
    TSASR_CHECK_ARG(io_dtype == TSASR_F32 || io_dtype == TSASR_BF16, "%s: bad dtype", name);
    int ns, tps;
    stream_split(B, C, H, Tmax, &ns, &tps);
    const size_t need = tsasr_relpos_attn_stream_workspace_bytes(B, C, H, Dh, Tmax);
    if (!workspace || workspace_bytes < need) { ns = 1; tps = cdiv(Tmax, SKT); }   // no workspace: one pass over the keys
    StreamAttnArgs a{qkv, k_cache, v_cache, pk_half, bias_u, bias_v, key_lens, out, (float *)workspace, B, C, H, Dh, Tmax, t0, causal, ns, tps,
                     scale, t0s};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cdiv(C, SQB), H, B * ns), mgrid(C, H, B), qgrid(cdiv(C, MQB), H, B * ns);
    if (io_dtype == TSASR_F32) {                     // exact fp32 arithmetic: the parity mode
        attn_stream_kernel<float><<<grid, 256, 0, st>>>(a);
        if (ns > 1) attn_stream_merge_kernel<float><<<mgrid, 64, 0, st>>>(a);
    } else {
        if (Dh == 64) attn_stream_mfma_kernel<64><<<qgrid, 256, 0, st>>>(a);
        else if (Dh == 32) attn_stream_mfma_kernel<32><<<qgrid, 256, 0, st>>>(a);
        else attn_stream_kernel<bf16_t><<<grid, 256, 0, st>>>(a);    // other head sizes: fp32 arithmetic on bf16 storage
        if (ns > 1) attn_stream_merge_kernel<bf16_t><<<mgrid, 64, 0, st>>>(a);
    }
    TSASR_CHECK_LAUNCH(name);
    return 0;
}

int tsasr_relpos_attn_stream_fwd(const void *qkv, void *k_cache, void *v_cache, const void *pk_half, const float *bias_u, const float *bias_v,
                                 const int32_t *key_lens, void *out, int B, int C, int H, int Dh, int Tmax, int t0, int causal, float scale,
                                 int io_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    return attn_stream_launch("tsasr_relpos_attn_stream_fwd", qkv, k_cache, v_cache, pk_half, bias_u, bias_v, key_lens, out, B, C, H, Dh, Tmax, t0,
                              nullptr, causal, scale, io_dtype, workspace, workspace_bytes, stream);
}

int tsasr_relpos_attn_stream_slots_fwd(const void *qkv, void *k_cache, void *v_cache, const void *pk_half, const float *bias_u,
                                       const float *bias_v, const int32_t *key_lens, void *out, int B, int C, int H, int Dh, int Tmax,
                                       const int32_t *t0s, int causal, float scale, int io_dtype, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    TSASR_CHECK_ARG(t0s, "tsasr_relpos_attn_stream_slots_fwd: null t0s");
    return attn_stream_launch("tsasr_relpos_attn_stream_slots_fwd", qkv, k_cache, v_cache, pk_half, bias_u, bias_v, key_lens, out, B, C, H, Dh,
                              Tmax, 0, t0s, causal, scale, io_dtype, workspace, workspace_bytes, stream);
}

static int convmod_stream_launch(const char *name, const void *y2, const float *b2, const float *conv_w, const float *conv_b, const float *gamma,
                                 const float *beta, const float *hist_in, float *hist_out, void *z, int B, int C, int D, int K, float eps,
                                 float slope, const int32_t *t0s, int io_dtype, void *stream) {
    TSASR_CHECK_ARG(y2 && conv_w && gamma && beta && hist_in && hist_out && z && hist_in != hist_out, "%s: null or aliased pointer", name);
    TSASR_CHECK_ARG(B > 0 && C > 0 && D > 0 && D <= 8192 && K >= 2 && K <= 64, "%s: bad shape (B=%d C=%d D=%d K=%d)", name, B, C, D, K);
    TSASR_CHECK_ARG(io_dtype == TSASR_F32 || io_dtype == TSASR_BF16, "%s: bad dtype", name);
    ConvStreamArgs a{y2, b2, conv_w, conv_b, gamma, beta, hist_in, hist_out, z, B, C, D, K, eps, slope, t0s};
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)D * sizeof(float);
    if (io_dtype == TSASR_F32) convmod_stream_kernel<float><<<dim3(C, B), 256, lds, st>>>(a);
    else convmod_stream_kernel<bf16_t><<<dim3(C, B), 256, lds, st>>>(a);
    TSASR_CHECK_LAUNCH(name);
    return 0;
}

int tsasr_convmod_stream_fwd(const void *y2, const float *b2, const float *conv_w, const float *conv_b, const float *gamma, const float *beta,
                             const float *hist_in, float *hist_out, void *z, int B, int C, int D, int K, float eps, float slope, int io_dtype,
                             void *stream) {
    return convmod_stream_launch("tsasr_convmod_stream_fwd", y2, b2, conv_w, conv_b, gamma, beta, hist_in, hist_out, z, B, C, D, K, eps, slope,
                                 nullptr, io_dtype, stream);
}

int tsasr_convmod_stream_slots_fwd(const void *y2, const float *b2, const float *conv_w, const float *conv_b, const float *gamma,
                                   const float *beta, const float *hist_in, float *hist_out, void *z, int B, int C, int D, int K, float eps,
                                   float slope, int io_dtype, const int32_t *t0s, void *stream) {
    TSASR_CHECK_ARG(t0s, "tsasr_convmod_stream_slots_fwd: null t0s");
    return convmod_stream_launch("tsasr_convmod_stream_slots_fwd", y2, b2, conv_w, conv_b, gamma, beta, hist_in, hist_out, z, B, C, D, K, eps,
                                 slope, t0s, io_dtype, stream);
}

}  // extern "C"
