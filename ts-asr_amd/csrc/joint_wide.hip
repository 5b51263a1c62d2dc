// RNN-T joint + head for subword vocabularies, 32 < V <= 1024, on gfx950 (MI355X).
//
// The same function as csrc/rnnt.hip's joint kernels,
//   logits[b,t,u,v] = bias[v] + sum_k W[v,k] * lrelu(enc[b,t,k] + dec[b,u,k]),
// with a vocabulary TILE LOOP inside every kernel: the head matrix (up to 1024 x 1024) no longer fits LDS or registers, so it is
// streamed from the fp32 masters 32 vocabulary rows at a time (for one launch it is L2-resident) and rounded to bf16 on the way into
// v_mfma_f32_32x32x16_bf16. The [B,T,U1,J] joint tensor is never written: h = lrelu(enc + dec) is formed once per lattice cell, kept in
// LDS as bf16 and reused by every vocabulary tile.
//
// Rounding (what tests/helpers/joint_wide_ref.py follows): forward h and W to bf16; backward dlogits, W and h to bf16; every sum in fp32.
//
//   fwd : workgroup = (b, 32 lattice columns u, TG frames). h tiles [TG][32][J] bf16 in LDS; wave w owns vocabulary tiles w, w+4, ...:
//         A = W tile (rows = vocabulary), B = h^T (columns = u), so a lane ends with 16 vocabulary entries of ONE cell -> 16-byte stores.
//   bwd : three kernels, no float atomics, no waiting on another workgroup, fixed summation orders => two runs give the same bits.
//     X : workgroup = (b, 32 columns u, a range of frames) walks its frames. The frame's dlogits tile [32][V] goes to LDS as bf16 once;
//         wave w owns the 32-wide slices w, w+4, ... of J and accumulates dh = lrelu' * (dlogits . W) over the vocabulary in fp32
//         (A = dlogits, B = W). A lane then holds 16 cells u of ONE joint column: their sum is this tile's share of denc (one partial
//         row per u tile), ddec accumulates in registers across the frames (one partial per frame range). The staging pass also sums
//         dlogits over the tile's rows in fp32 for dbias (one slab row per workgroup).
//     W : dW = dlogits^T . h is a real GEMM with the lattice cells as its inner dimension. Per-workgroup slabs of kernel X would be
//         B * cdiv(U1, 32) * TS copies of [V, J] (1.3 GB at the benchmark batch and V = 1024), so it is a kernel of its own: workgroup =
//         (128 vocabulary rows, 128 joint columns, one of S <= 64 ranges of frames), h recomputed, S slabs of [V, J] joined by the batched
//         reduction (tsasr_reduce_submit) like every other parameter gradient.
//     sum: the denc / ddec partials are added in fixed order and written in the io dtype.
//   tlen / ulen only skip cells whose dlogits the loss left zero; a skipped cell and a processed zero cell add the same +0.
//   fused joint + loss (second half of the file): the same products with the log-softmax reduction (forward) and the loss gradient's formula
//         (backward) fed by the vocabulary tile loop instead of a [B,T,U1,V] tensor in memory: tsasr_joint_wide_loss_* / tsasr_joint_wide_align.
#include <algorithm>

#include "common.h"
#include "rnnt_ws.h"

namespace {

__device__ __forceinline__ int mfma_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }   // row of accumulator register g (32x32 tile)

__device__ __forceinline__ bf16x8 to_bf16x8(const float (&v)[8]) {
    return bf16x8_of(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
}

// ============================================================================================
// forward
// ============================================================================================
template <typename T, int TG>
__global__ __launch_bounds__(256) void joint_wide_fwd_kernel(const T *__restrict__ enc, const T *__restrict__ dec, const float *__restrict__ W,
                                                             const float *__restrict__ bias, float *__restrict__ logits, int Tn, int U1, int J,
                                                             int V, int ldl, float slope) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t *h_lds = reinterpret_cast<bf16_t *>(smem);       // [TG][32][S]
    const int S = J + 8;                                    // +16 B per row: consecutive rows start in different 16-byte slots
    const int b = blockIdx.z, t0 = blockIdx.y * TG, u0 = blockIdx.x * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nc = J / 8;
    for (int i = tid; i < TG * 32 * nc; i += 256) {         // rows past T / U1 repeat the last valid one (never stored)
        const int c = (i % nc) * 8, row = (i / nc) & 31, f = i / (nc * 32);
        const int t = min(t0 + f, Tn - 1), u = min(u0 + row, U1 - 1);
        float e8[8], d8[8], h8[8];
        ld8(enc + ((size_t)b * Tn + t) * J + c, e8);
        ld8(dec + ((size_t)b * U1 + u) * J + c, d8);
#pragma unroll
        for (int j = 0; j < 8; ++j) h8[j] = lrelu(e8[j] + d8[j], slope);
        st8(h_lds + (size_t)(f * 32 + row) * S + c, h8);
    }
    __syncthreads();
    const int nvt = ldl / 32, nks = J / 16;
    for (int vt = wave; vt < nvt; vt += 4) {
        const int v0 = vt * 32;
        const bool wok = v0 + r < V;
        const float *wrow = W + (size_t)min(v0 + r, V - 1) * J + 8 * h;
        const bf16_t *hrow = h_lds + (size_t)r * S + 8 * h;
        f32x16 acc[TG];
#pragma unroll
        for (int f = 0; f < TG; ++f) acc[f] = (f32x16){0};
#pragma unroll 2
        for (int s = 0; s < nks; ++s) {
            float w8[8];
            ld8(wrow + 16 * s, w8);
            if (!wok) {
#pragma unroll
                for (int j = 0; j < 8; ++j) w8[j] = 0.f;
            }
            const bf16x8 wa = to_bf16x8(w8);
#pragma unroll
            for (int f = 0; f < TG; ++f) {
                const bf16x8 hb = *reinterpret_cast<const bf16x8 *>(hrow + (size_t)f * 32 * S + 16 * s);
                acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, hb, acc[f], 0, 0, 0);
            }
        }
        float bv[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int v = v0 + mfma_row(g, h);
            bv[g] = v < V ? bias[v] : 0.f;
        }
        if (u0 + r < U1) {
#pragma unroll
            for (int f = 0; f < TG; ++f) {
                if (t0 + f >= Tn) break;
                float *orow = logits + (((size_t)b * Tn + t0 + f) * U1 + u0 + r) * ldl + v0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {               // vocabulary rows 8q+4h .. 8q+4h+3 of the tile -> one 16-byte store
                    const int vq = 8 * q + 4 * h;
                    float4 o;
                    o.x = (v0 + vq + 0 < V) ? acc[f][4 * q + 0] + bv[4 * q + 0] : 0.f;
                    o.y = (v0 + vq + 1 < V) ? acc[f][4 * q + 1] + bv[4 * q + 1] : 0.f;
                    o.z = (v0 + vq + 2 < V) ? acc[f][4 * q + 2] + bv[4 * q + 2] : 0.f;
                    o.w = (v0 + vq + 3 < V) ? acc[f][4 * q + 3] + bv[4 * q + 3] : 0.f;
                    *reinterpret_cast<float4 *>(orow + vq) = o;
                }
            }
        }
    }
}

// ============================================================================================
// backward X: ddec / denc partial sums, dbias slabs
// ============================================================================================
// NKT: 32-wide slices of J per wave (J <= 128 * NKT * JS)
template <typename T, int NKT>
__global__ __launch_bounds__(256, 1) void joint_wide_bwd_x_kernel(const float *__restrict__ dl, const T *__restrict__ enc, const T *__restrict__ dec,
                                                                  const float *__restrict__ W, float *__restrict__ part_enc,
                                                                  float *__restrict__ part_dec, float *__restrict__ slab_b,
                                                                  const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen, int Tn,
                                                                  int U1, int J, int V, int ldl, float slope, int TS) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t *g_lds = reinterpret_cast<bf16_t *>(smem);       // [32][SV] this frame's dlogits tile
    const int Vp = (V + 15) / 16 * 16, SV = Vp + 8, nq = Vp / 4;
    const int JS = gridDim.y / TS;                          // J > 640 is split over two workgroups (each stages the dlogits tile)
    const int B = gridDim.z, b = blockIdx.z, ts = blockIdx.y / JS, js = blockIdx.y % JS, ut = blockIdx.x, u0 = ut * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tl = tlen ? min(tlen[b], Tn) : Tn, ul = ulen ? min(ulen[b], U1 - 1) : U1 - 1;     // cells t < tl, u <= ul carry gradient
    const int tchunk = (Tn + TS - 1) / TS, t_begin = ts * tchunk, t_end = min(Tn, t_begin + tchunk);
    const int kchunk = (J / 32 + JS - 1) / JS, kt_lo = js * kchunk, nkt = min(J / 32, kt_lo + kchunk);
    // staging role: thread (rg, cq) moves the four columns 4cq .. 4cq+3 of rows rg, rg + RG, ... and keeps their fp32 sums for dbias
    const int RG = 256 / nq > 32 ? 32 : 256 / nq, rg = tid / nq, cq = tid % nq;
    float4 db = make_float4(0.f, 0.f, 0.f, 0.f);
    f32x16 dd[NKT];
#pragma unroll
    for (int i = 0; i < NKT; ++i) dd[i] = (f32x16){0};

    for (int t = t_begin; t < t_end; ++t) {
        const bool active = t < tl && u0 <= ul;             // the same for the whole workgroup
        if (!active) {
            if (h == 0)
                for (int kt = kt_lo + wave; kt < nkt; kt += 4) part_enc[(((size_t)ut * B + b) * Tn + t) * J + kt * 32 + r] = 0.f;
            continue;
        }
        __syncthreads();                                    // the previous frame's MFMA reads of g_lds are done
        if (rg < RG) {
            for (int row = rg; row < 32; row += RG) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                const int c = 4 * cq;
                if (u0 + row <= ul && c < ldl) {
                    v = *reinterpret_cast<const float4 *>(dl + (((size_t)b * Tn + t) * U1 + u0 + row) * ldl + c);
                    if (c + 1 >= V) v.y = 0.f;
                    if (c + 2 >= V) v.z = 0.f;
                    if (c + 3 >= V) v.w = 0.f;
                    if (c >= V) v.x = 0.f;
                }
                db.x += v.x; db.y += v.y; db.z += v.z; db.w += v.w;     // (kept by the js == 0 workgroup)
                *reinterpret_cast<uint2 *>(g_lds + (size_t)row * SV + c) = make_uint2(pk_bf16(v.x, v.y), pk_bf16(v.z, v.w));
            }
        }
        __syncthreads();
        const T *erow = enc + ((size_t)b * Tn + t) * J;
        // vocabulary steps outside, the wave's slices of J inside: one dlogits fragment from LDS feeds NKT MFMAs, and the 8 * NKT weight loads of
        // a step are in flight together (slice by slice every step is a dependent L2 round trip; profiles/wide_vocab_notes.md has the times).
        // A slice past the wave's share repeats its last one: loaded and multiplied, never used.
        f32x16 acc[NKT];
        int jcs[NKT];
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            acc[i] = (f32x16){0};
            jcs[i] = min(kt_lo + wave + 4 * i, nkt - 1) * 32 + r;
        }
        const bf16_t *grow = g_lds + (size_t)r * SV + 8 * h;
        for (int s = 0; s < Vp / 16; ++s) {
            const bf16x8 ga = *reinterpret_cast<const bf16x8 *>(grow + 16 * s);
            float w8[NKT][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float *wrow = W + (size_t)min(16 * s + 8 * h + j, V - 1) * J;     // rows >= V meet zero dlogits
#pragma unroll
                for (int i = 0; i < NKT; ++i) w8[i][j] = wrow[jcs[i]];
            }
#pragma unroll
            for (int i = 0; i < NKT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, to_bf16x8(w8[i]), acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            const int kt = kt_lo + wave + 4 * i;
            if (kt >= nkt) break;
            const int jc = kt * 32 + r;
            const float e = ld1(erow + jc);
            float colsum = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int u = min(u0 + mfma_row(g, h), U1 - 1);
                const float x = e + ld1(dec + ((size_t)b * U1 + u) * J + jc);
                const float dh = acc[i][g] * (x > 0.f ? 1.f : slope);
                dd[i][g] += dh;
                colsum += dh;
            }
            colsum += other_half(colsum);
            if (h == 0) part_enc[(((size_t)ut * B + b) * Tn + t) * J + jc] = colsum;
        }
    }
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
        const int kt = kt_lo + wave + 4 * i;
        if (kt >= nkt) break;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int u = u0 + mfma_row(g, h);
            if (u < U1) part_dec[(((size_t)ts * B + b) * U1 + u) * J + kt * 32 + r] = dd[i][g];
        }
    }
    // dbias: the row groups' sums meet in LDS and are added in row-group order
    if (js != 0) return;
    __syncthreads();
    float *s_lds = reinterpret_cast<float *>(smem);         // [RG][Vp]
    if (rg < RG) *reinterpret_cast<float4 *>(s_lds + (size_t)rg * Vp + 4 * cq) = db;
    __syncthreads();
    float *srow = slab_b + (((size_t)b * TS + ts) * gridDim.x + ut) * Vp;
    for (int v = tid; v < Vp; v += 256) {
        float s = 0.f;
        for (int g = 0; g < RG; ++g) s += s_lds[(size_t)g * Vp + v];
        srow[v] = s;
    }
}

// ============================================================================================
// backward W: dW slabs
// ============================================================================================
template <typename T>
__global__ __launch_bounds__(256) void joint_wide_bwd_w_kernel(const float *__restrict__ dl, const T *__restrict__ enc, const T *__restrict__ dec,
                                                               float *__restrict__ slab_w, const int32_t *__restrict__ tlen,
                                                               const int32_t *__restrict__ ulen, int B, int Tn, int U1, int J, int V, int ldl,
                                                               float slope) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int v0 = blockIdx.y * 128 + (wave >> 1) * 64, j0 = blockIdx.x * 128 + (wave & 1) * 64;
    const int S = gridDim.z, sp = blockIdx.z;
    const long long nfr = (long long)B * Tn, fchunk = (nfr + S - 1) / S;
    const long long f_begin = sp * fchunk, f_end = std::min(nfr, f_begin + fchunk);
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[a][c] = (f32x16){0};
    const bool live = v0 < V && j0 < J;                     // a wave whose tile lies outside [V, J] only writes nothing
    for (long long fr = f_begin; live && fr < f_end; ++fr) {
        const int b = (int)(fr / Tn), t = (int)(fr % Tn);
        const int tl = tlen ? min(tlen[b], Tn) : Tn, ul = ulen ? min(ulen[b], U1 - 1) : U1 - 1;
        if (t >= tl) continue;
        const float *drow = dl + ((size_t)b * Tn + t) * U1 * ldl;
        float e[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) e[c] = ld1(enc + ((size_t)b * Tn + t) * J + min(j0 + 32 * c + r, J - 1));
        for (int uc = 0; uc <= ul; uc += 16) {              // 16 lattice cells of this frame = one k-step
            bf16x8 ga[2], hb[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int v = v0 + 32 * a + r;
                float g8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int u = uc + 8 * h + j;
                    const float x = drow[(size_t)min(u, U1 - 1) * ldl + min(v, V - 1)];
                    g8[j] = (u <= ul && v < V) ? x : 0.f;
                }
                ga[a] = to_bf16x8(g8);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int jc = min(j0 + 32 * c + r, J - 1);
                float h8[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int u = min(uc + 8 * h + j, U1 - 1);
                    h8[j] = lrelu(e[c] + ld1(dec + ((size_t)b * U1 + u) * J + jc), slope);
                }
                hb[c] = to_bf16x8(h8);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga[a], hb[c], acc[a][c], 0, 0, 0);
        }
    }
    if (!live) return;
    float *slab = slab_w + (size_t)sp * V * J;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int jc = j0 + 32 * c + r;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int v = v0 + 32 * a + mfma_row(g, h);
                if (v < V && jc < J) slab[(size_t)v * J + jc] = acc[a][c][g];
            }
        }
}

// out[e] = sum over the partials part[p][e] (fixed order), four elements per thread, written in the io dtype
template <typename T>
__global__ __launch_bounds__(256) void joint_wide_sum_kernel(const float *__restrict__ part, T *__restrict__ out, long long n, int nparts) {
    for (long long e = (blockIdx.x * 256LL + threadIdx.x) * 4; e < n; e += (long long)gridDim.x * 256 * 4) {
        float4 s = *reinterpret_cast<const float4 *>(part + e);
        for (int p = 1; p < nparts; ++p) {
            const float4 v = *reinterpret_cast<const float4 *>(part + (long long)p * n + e);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        st1(out + e, s.x); st1(out + e + 1, s.y); st1(out + e + 2, s.z); st1(out + e + 3, s.w);
    }
}

// ---- host plans: functions of the shape alone, so that the workspace layout and the summation orders never depend on the device ----
// frames per workgroup = h tiles [32][J + 8] bf16 that fit 160 KiB of LDS: 4 up to J = 632, 3 up to J = 832 (the recipe's J = 640), 2 up to J = 1024
int fwd_tg(int J) {
    for (int tg = 4; tg > 2; --tg)
        if ((size_t)tg * 32 * (J + 8) * sizeof(bf16_t) <= 160 * 1024) return tg;
    return 2;
}

int bwd_tsplit(int B, int T, int U1) {          // frame ranges of kernel X: about 512 workgroups, at least 16 frames per range
    int ts = 1;
    while (ts < 8 && (long long)B * cdiv(U1, 32) * ts < 512 && T / (ts * 2) >= 16) ts *= 2;
    return ts;
}

// frame ranges of kernel W: about 1024 workgroups (three fit a CU, and a workgroup is a chain of dependent loads: measured at the benchmark
// batch, V = 256, 160 workgroups took 26 ms), at most 64 slabs and 128 MiB of them
int bwd_wsplit(int B, int T, int J, int V) {
    const long long tiles = (long long)cdiv(J, 128) * cdiv(V, 128);
    long long s = std::min<long long>(64, std::max<long long>(1, 1024 / tiles));
    s = std::min<long long>(s, std::max<long long>(1, (128ll << 20) / ((long long)V * J * (long long)sizeof(float))));
    return (int)std::min<long long>(s, (long long)B * T);
}

struct WideWs {
    float *part_enc, *part_dec, *slab_b, *slab_w;
    size_t bytes;
};
WideWs carve(void *ws, int B, int T, int U1, int J, int V) {
    const int nut = cdiv(U1, 32), TS = bwd_tsplit(B, T, U1), S = bwd_wsplit(B, T, J, V), Vp = (V + 15) / 16 * 16;
    char *p = (char *)ws;
    WideWs w;
    w.part_enc = (float *)p; p += align_up((size_t)nut * B * T * J * sizeof(float), 256);        // denc share of every u tile
    w.part_dec = (float *)p; p += align_up((size_t)TS * B * U1 * J * sizeof(float), 256);        // ddec share of every frame range
    w.slab_b = (float *)p;   p += align_up((size_t)B * TS * nut * Vp * sizeof(float), 256);      // dbias row of every workgroup of kernel X
    w.slab_w = (float *)p;   p += align_up((size_t)S * V * J * sizeof(float), 256);              // dW slab of every frame range of kernel W
    w.bytes = (size_t)(p - (char *)ws);
    return w;
}

template <typename T, int TG>
void launch_fwd(const void *enc, const void *dec, const float *W, const float *bias, float *logits, int B, int Tn, int U1, int J, int V, int ldl,
                float slope, hipStream_t st) {
    const size_t lds = (size_t)TG * 32 * (J + 8) * sizeof(bf16_t);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)joint_wide_fwd_kernel<T, TG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    joint_wide_fwd_kernel<T, TG><<<dim3(cdiv(U1, 32), cdiv(Tn, TG), B), 256, lds, st>>>((const T *)enc, (const T *)dec, W, bias, logits, Tn, U1, J, V,
                                                                                       ldl, slope);
}

template <typename T, int NKT>
void launch_x(const float *dl, const void *enc, const void *dec, const float *W, const WideWs &w, const int32_t *tlen, const int32_t *ulen, int B, int Tn,
              int U1, int J, int V, int ldl, float slope, int TS, hipStream_t st) {
    const int Vp = (V + 15) / 16 * 16;
    const size_t lds_tile = (size_t)32 * (Vp + 8) * sizeof(bf16_t);                              // the frame's dlogits tile
    const size_t lds_sum = (size_t)std::min(32, 256 / (Vp / 4)) * Vp * sizeof(float);            // the row groups' dbias sums (at the end)
    const size_t need = std::max(lds_tile, lds_sum);
    if (need > 64 * 1024) (void)hipFuncSetAttribute((const void *)joint_wide_bwd_x_kernel<T, NKT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    joint_wide_bwd_x_kernel<T, NKT><<<dim3(cdiv(U1, 32), TS * (J > 640 ? 2 : 1), B), 256, need, st>>>(dl, (const T *)enc, (const T *)dec, W, w.part_enc, w.part_dec, w.slab_b,
                                                                                 tlen, ulen, Tn, U1, J, V, ldl, slope, TS);
}

template <typename T>
void launch_bwd(const float *dl, const void *enc, const void *dec, const float *W, void *denc, void *ddec, const WideWs &w, const int32_t *tlen,
                const int32_t *ulen, int B, int Tn, int U1, int J, int V, int ldl, float slope, hipStream_t st) {
    const int nut = cdiv(U1, 32), TS = bwd_tsplit(B, Tn, U1), S = bwd_wsplit(B, Tn, J, V), nkt = cdiv(cdiv(J / 32, J > 640 ? 2 : 1), 4);
    if (nkt <= 1) launch_x<T, 1>(dl, enc, dec, W, w, tlen, ulen, B, Tn, U1, J, V, ldl, slope, TS, st);
    else if (nkt <= 2) launch_x<T, 2>(dl, enc, dec, W, w, tlen, ulen, B, Tn, U1, J, V, ldl, slope, TS, st);
    else launch_x<T, 5>(dl, enc, dec, W, w, tlen, ulen, B, Tn, U1, J, V, ldl, slope, TS, st);      // J <= 640, or half of J <= 1024
    joint_wide_bwd_w_kernel<T><<<dim3(cdiv(J, 128), cdiv(V, 128), S), 256, 0, st>>>(dl, (const T *)enc, (const T *)dec, w.slab_w, tlen, ulen, B, Tn, U1, J,
                                                                                   V, ldl, slope);
    const long long n_enc = (long long)B * Tn * J, n_dec = (long long)B * U1 * J;
    joint_wide_sum_kernel<T><<<(unsigned)std::min<long long>(4096, (n_enc / 4 + 255) / 256), 256, 0, st>>>(w.part_enc, (T *)denc, n_enc, nut);
    joint_wide_sum_kernel<T><<<(unsigned)std::min<long long>(4096, (n_dec / 4 + 255) / 256), 256, 0, st>>>(w.part_dec, (T *)ddec, n_dec, TS);
}

// ============================================================================================
// fused joint + loss ("lazy logits"): the [B,T,U1,V] logits and dlogits tensors are never written
// ============================================================================================
// forward : joint_wide_fwd_kernel's tiling; a tile's logits stay in the accumulators and are folded into a running (maximum, sum of exp)
//           per lattice cell, the blank and the label logit are picked out as their tiles go by, and the cell's lse / lp(blank) / lp(label)
//           go straight into the lattice planes (csrc/rnnt_ws.h) that rnnt_alphabeta_kernel / rnnt_viterbi_kernel walk.
//           Reduction order: a lane folds the 16 entries of a tile in register order and its tiles in tile order; then the two lane halves
//           (rows 4h .. of every tile), then the four waves (tiles w, w + 4, ...) are merged in that fixed order.
// cells   : c0 = alpha + beta - logp - lse, gblank, gemit per live cell (rnnt_grad_kernel's three scalars) in three dense [B,T,U1] planes.
// backward: dlogits = gs * (exp(c0 + logit) - [v == blank] gblank - [v == label] gemit) is a function of a cell's logits row and those
//           scalars, so both products recompute their dlogits operand tile by tile (W tile . h + bias, the forward's operand rounding):
//     X : joint_wide_bwd_x_kernel with the staging pass replaced by a producer: the frame's h tile [32][J] goes to LDS, wave w forms the
//         vocabulary tiles w, w + 4, ... of the frame's dlogits tile on the matrix cores and writes them to LDS as bf16; the dh product,
//         the denc / ddec partial sums and their orders are the materialised kernel's.
//     W : workgroup = (one vocabulary tile of 32 rows, ALL of J, one of S ranges of frames): the W tile stays in LDS as bf16; per 32 lattice
//         cells the h tile goes to LDS, the logits tile [32 v][32 u] is a split-k product over the four waves (partials joined through LDS
//         in wave order), the dlogits formula runs on it (fp32 sums over the cells = this range's dbias row), and dW[32][J] accumulates in
//         registers (J / 128 accumulator tiles per wave). Covering all of J per workgroup is what makes one logits product per cell
//         enough; S slabs of [V, J] are joined by tsasr_reduce_submit as in the materialised route.
// No float atomics, nothing waits on another workgroup, fixed summation orders => two runs give the same bits.
constexpr float kNegInf = -INFINITY;

// (maximum, sum of exp) of two disjoint parts of a row; a part without entries is (-inf, 0)
__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float a = m > kNegInf ? s * __expf(m - mn) : 0.f;
    const float c = m2 > kNegInf ? s2 * __expf(m2 - mn) : 0.f;
    m = mn;
    s = a + c;
}

template <typename T, int TG>
__global__ __launch_bounds__(256) void joint_wide_lp_kernel(const T *__restrict__ enc, const T *__restrict__ dec, const float *__restrict__ W,
                                                            const float *__restrict__ bias, const int32_t *__restrict__ targets, int ldt,
                                                            const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen, RnntWs w, int Tn,
                                                            int U1, int J, int V, int blank, float slope) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t *h_lds = reinterpret_cast<bf16_t *>(smem);       // [TG][32][S]
    const int S = J + 8;
    const int b = blockIdx.z, t0 = blockIdx.y * TG, u0 = blockIdx.x * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nc = J / 8;
    const int Tb = min(max(tlen[b], 1), Tn), Ub = min(max(ulen[b], 0), U1 - 1);
    if (t0 >= Tb || u0 > Ub) return;                        // no live cell in this tile (the same for the whole workgroup)
    for (int i = tid; i < TG * 32 * nc; i += 256) {         // rows past T / U1 repeat the last valid one (never stored)
        const int c = (i % nc) * 8, row = (i / nc) & 31, f = i / (nc * 32);
        const int t = min(t0 + f, Tn - 1), u = min(u0 + row, U1 - 1);
        float e8[8], d8[8], h8[8];
        ld8(enc + ((size_t)b * Tn + t) * J + c, e8);
        ld8(dec + ((size_t)b * U1 + u) * J + c, d8);
#pragma unroll
        for (int j = 0; j < 8; ++j) h8[j] = lrelu(e8[j] + d8[j], slope);
        st8(h_lds + (size_t)(f * 32 + row) * S + c, h8);
    }
    const int lab = (u0 + r < Ub) ? min(max(targets[(size_t)b * ldt + u0 + r], 0), V - 1) : -1;       // label of this lane's cell column
    __syncthreads();
    float mx[TG], sm[TG], vb[TG], vl[TG];
#pragma unroll
    for (int f = 0; f < TG; ++f) { mx[f] = kNegInf; sm[f] = 0.f; vb[f] = 0.f; vl[f] = 0.f; }
    const int nvt = (V + 31) / 32, nks = J / 16;
    for (int vt = wave; vt < nvt; vt += 4) {
        const int v0 = vt * 32;
        const bool wok = v0 + r < V;
        const float *wrow = W + (size_t)min(v0 + r, V - 1) * J + 8 * h;
        const bf16_t *hrow = h_lds + (size_t)r * S + 8 * h;
        f32x16 acc[TG];
#pragma unroll
        for (int f = 0; f < TG; ++f) acc[f] = (f32x16){0};
#pragma unroll 2
        for (int s = 0; s < nks; ++s) {
            float w8[8];
            ld8(wrow + 16 * s, w8);
            if (!wok) {
#pragma unroll
                for (int j = 0; j < 8; ++j) w8[j] = 0.f;
            }
            const bf16x8 wa = to_bf16x8(w8);
#pragma unroll
            for (int f = 0; f < TG; ++f) {
                const bf16x8 hb = *reinterpret_cast<const bf16x8 *>(hrow + (size_t)f * 32 * S + 16 * s);
                acc[f] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, hb, acc[f], 0, 0, 0);
            }
        }
        float bv[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) bv[g] = bias[min(v0 + mfma_row(g, h), V - 1)];
#pragma unroll
        for (int f = 0; f < TG; ++f) {
            float x[16], tm = kNegInf;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int v = v0 + mfma_row(g, h);
                x[g] = v < V ? acc[f][g] + bv[g] : kNegInf;
                tm = fmaxf(tm, x[g]);
                vb[f] += v == blank ? x[g] : 0.f;
                vl[f] += v == lab ? x[g] : 0.f;
            }
            if (tm > kNegInf) {                             // (a half tile entirely past V adds nothing)
                const float mn = fmaxf(mx[f], tm);
                float part = 0.f;
#pragma unroll
                for (int g = 0; g < 16; ++g) part += __expf(x[g] - mn);
                sm[f] = sm[f] * __expf(mx[f] - mn) + part;
                mx[f] = mn;
            }
        }
    }
    __syncthreads();                                        // every wave is done with the h tiles: the area is reused for the merge
    float4 *red = reinterpret_cast<float4 *>(smem);         // [4 waves][TG][32 cells]: (max, sum, blank logit, label logit)
#pragma unroll
    for (int f = 0; f < TG; ++f) {
        const float om = other_half(mx[f]), os = other_half(sm[f]);
        float m0 = h == 0 ? mx[f] : om, s0 = h == 0 ? sm[f] : os;
        lse_merge(m0, s0, h == 0 ? om : mx[f], h == 0 ? os : sm[f]);
        const float b2 = vb[f] + other_half(vb[f]), l2 = vl[f] + other_half(vl[f]);
        if (h == 0) red[(wave * TG + f) * 32 + r] = make_float4(m0, s0, b2, l2);
    }
    __syncthreads();
    if (tid < TG * 32) {
        const int f = tid >> 5, c = tid & 31, t = t0 + f, u = u0 + c;
        float4 a = red[f * 32 + c];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            const float4 o = red[(wv * TG + f) * 32 + c];
            lse_merge(a.x, a.y, o.x, o.y);
            a.z += o.z;
            a.w += o.w;
        }
        if (t < Tb && u <= Ub) {
            const float lse = a.x + __logf(a.y);
            const size_t o = ws_at(w, b, t, u);
            w.lse[o] = lse;
            w.lpb[o] = a.z - lse;
            if (u < Ub) {
                const float e = a.w - lse;
                w.lpe_out[o] = e;
                w.lpe_in[ws_at(w, b, t, u + 1)] = e;
            }
        }
    }
}

// the three per-cell scalars of rnnt_grad_kernel, in dense planes cell[0 / n / 2n + (b * T + t) * U1 + u] (zeros outside the lattice)
__global__ __launch_bounds__(256) void joint_wide_cell_kernel(RnntWs w, const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen,
                                                              float *__restrict__ cell, long long n, int Tn, int U1) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const int u = row % U1, t = (row / U1) % Tn, b = row / ((long long)U1 * Tn);
    const int Tb = min(max(tlen[b], 1), Tn), Ub = min(max(ulen[b], 0), U1 - 1);
    float c0 = 0.f, gblank = 0.f, gemit = 0.f;
    if (t < Tb && u <= Ub) {
        const size_t o = ws_at(w, b, t, u);
        const float logp = w.logp[b], a = w.alpha[o], be = w.beta[o], lse = w.lse[o], lpb = w.lpb[o];
        c0 = a + be - logp - lse;
        if (t < Tb - 1) gblank = __expf(a + lpb + w.beta[o + w.U1P] - logp);
        else gblank = (u == Ub) ? __expf(a + lpb - logp) : 0.f;
        if (u < Ub) gemit = __expf(a + w.lpe_out[o] + w.beta[ws_at(w, b, t, u + 1)] - logp);
    }
    cell[row] = c0;
    cell[n + row] = gblank;
    cell[2 * n + row] = gemit;
}

// rnnt_grad_kernel's formula for one entry (live cell, v < V)
__device__ __forceinline__ float lazy_dlogit(float logit, int v, float c0, float gblank, float gemit, float gs, int blank, int lab) {
    float val = __expf(c0 + logit);
    if (v == blank) val -= gblank;
    if (v == lab) val -= gemit;
    return val * gs;
}

template <typename T, int NKT>
__global__ __launch_bounds__(256, 1) void joint_wide_lazy_x_kernel(const T *__restrict__ enc, const T *__restrict__ dec, const float *__restrict__ W,
                                                                   const float *__restrict__ bias, const int32_t *__restrict__ targets, int ldt,
                                                                   const float *__restrict__ gscale, const float *__restrict__ cell, long long ncell,
                                                                   float *__restrict__ part_enc, float *__restrict__ part_dec,
                                                                   const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen, int Tn, int U1,
                                                                   int J, int V, int blank, float slope, int TS) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Vp = (V + 15) / 16 * 16, SV = Vp + 8, S = J + 8;
    bf16_t *g_lds = reinterpret_cast<bf16_t *>(smem);       // [32][SV] this frame's dlogits tile
    bf16_t *h_lds = g_lds + (size_t)32 * SV;                // [32][S]  this frame's h tile
    const int JS = gridDim.y / TS;
    const int B = gridDim.z, b = blockIdx.z, ts = blockIdx.y / JS, js = blockIdx.y % JS, ut = blockIdx.x, u0 = ut * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int tl = min(max(tlen[b], 1), Tn), ul = min(max(ulen[b], 0), U1 - 1);                  // the loss's clamps: cells t < tl, u <= ul are live
    const int tchunk = (Tn + TS - 1) / TS, t_begin = ts * tchunk, t_end = min(Tn, t_begin + tchunk);
    const int kchunk = (J / 32 + JS - 1) / JS, kt_lo = js * kchunk, nkt = min(J / 32, kt_lo + kchunk);
    const int nc = J / 8, nvt = (V + 31) / 32, nks = J / 16;
    const int ucell = min(u0 + r, U1 - 1);
    const bool live = u0 + r <= ul;
    const int lab = (u0 + r < ul) ? min(max(targets[(size_t)b * ldt + u0 + r], 0), V - 1) : -1;
    const float gs = gscale[b];
    f32x16 dd[NKT];
#pragma unroll
    for (int i = 0; i < NKT; ++i) dd[i] = (f32x16){0};

    for (int t = t_begin; t < t_end; ++t) {
        const bool active = t < tl && u0 <= ul;             // the same for the whole workgroup
        if (!active) {
            if (h == 0)
                for (int kt = kt_lo + wave; kt < nkt; kt += 4) part_enc[(((size_t)ut * B + b) * Tn + t) * J + kt * 32 + r] = 0.f;
            continue;
        }
        __syncthreads();                                    // the previous frame's MFMA reads of g_lds / h_lds are done
        for (int i = tid; i < 32 * nc; i += 256) {
            const int c = (i % nc) * 8, row = i / nc;
            float e8[8], d8[8], h8[8];
            ld8(enc + ((size_t)b * Tn + t) * J + c, e8);
            ld8(dec + ((size_t)b * U1 + min(u0 + row, U1 - 1)) * J + c, d8);
#pragma unroll
            for (int j = 0; j < 8; ++j) h8[j] = lrelu(e8[j] + d8[j], slope);
            st8(h_lds + (size_t)row * S + c, h8);
        }
        const long long ci = ((long long)b * Tn + t) * U1 + ucell;
        const float c0 = cell[ci], gblank = cell[ncell + ci], gemit = cell[2 * ncell + ci];
        __syncthreads();
        // producer: the frame's dlogits tile, vocabulary tile by vocabulary tile (joint_wide_lp_kernel's product)
        for (int vt = wave; vt < nvt; vt += 4) {
            const int v0 = vt * 32;
            const bool wok = v0 + r < V;
            const float *wrow = W + (size_t)min(v0 + r, V - 1) * J + 8 * h;
            const bf16_t *hrow = h_lds + (size_t)r * S + 8 * h;
            f32x16 lg = {0};
#pragma unroll 2
            for (int s = 0; s < nks; ++s) {
                float w8[8];
                ld8(wrow + 16 * s, w8);
                if (!wok) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) w8[j] = 0.f;
                }
                lg = __builtin_amdgcn_mfma_f32_32x32x16_bf16(to_bf16x8(w8), *reinterpret_cast<const bf16x8 *>(hrow + 16 * s), lg, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int vq = v0 + 8 * q + 4 * h;
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = vq + j;
                    o[j] = (live && v < V) ? lazy_dlogit(lg[4 * q + j] + bias[min(v, V - 1)], v, c0, gblank, gemit, gs, blank, lab) : 0.f;
                }
                if (vq < Vp) *reinterpret_cast<uint2 *>(g_lds + (size_t)r * SV + vq) = make_uint2(pk_bf16(o[0], o[1]), pk_bf16(o[2], o[3]));
            }
        }
        __syncthreads();
        const T *erow = enc + ((size_t)b * Tn + t) * J;
        f32x16 acc[NKT];
        int jcs[NKT];
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            acc[i] = (f32x16){0};
            jcs[i] = min(kt_lo + wave + 4 * i, nkt - 1) * 32 + r;
        }
        const bf16_t *grow = g_lds + (size_t)r * SV + 8 * h;
        for (int s = 0; s < Vp / 16; ++s) {
            const bf16x8 ga = *reinterpret_cast<const bf16x8 *>(grow + 16 * s);
            float w8[NKT][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float *wrow = W + (size_t)min(16 * s + 8 * h + j, V - 1) * J;     // rows >= V meet zero dlogits
#pragma unroll
                for (int i = 0; i < NKT; ++i) w8[i][j] = wrow[jcs[i]];
            }
#pragma unroll
            for (int i = 0; i < NKT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, to_bf16x8(w8[i]), acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            const int kt = kt_lo + wave + 4 * i;
            if (kt >= nkt) break;
            const int jc = kt * 32 + r;
            const float e = ld1(erow + jc);
            float colsum = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int u = min(u0 + mfma_row(g, h), U1 - 1);
                const float x = e + ld1(dec + ((size_t)b * U1 + u) * J + jc);
                const float dh = acc[i][g] * (x > 0.f ? 1.f : slope);
                dd[i][g] += dh;
                colsum += dh;
            }
            colsum += other_half(colsum);
            if (h == 0) part_enc[(((size_t)ut * B + b) * Tn + t) * J + jc] = colsum;
        }
    }
#pragma unroll
    for (int i = 0; i < NKT; ++i) {
        const int kt = kt_lo + wave + 4 * i;
        if (kt >= nkt) break;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int u = u0 + mfma_row(g, h);
            if (u < U1) part_dec[(((size_t)ts * B + b) * U1 + u) * J + kt * 32 + r] = dd[i][g];
        }
    }
}

// NJT: 32-wide slices of J per wave (J <= 128 * NJT)
template <typename T, int NJT>
__global__ __launch_bounds__(256, 1) void joint_wide_lazy_w_kernel(const T *__restrict__ enc, const T *__restrict__ dec, const float *__restrict__ W,
                                                                   const float *__restrict__ bias, const int32_t *__restrict__ targets, int ldt,
                                                                   const float *__restrict__ gscale, const float *__restrict__ cell, long long ncell,
                                                                   float *__restrict__ slab_w, float *__restrict__ slab_b,
                                                                   const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen, int B, int Tn,
                                                                   int U1, int J, int V, int blank, float slope) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = J + 8;
    constexpr int SD = 40;                                  // dlogits tile row: 32 cells + 16 bytes
    bf16_t *w_lds = reinterpret_cast<bf16_t *>(smem);       // [32][S]  this workgroup's vocabulary tile of W
    bf16_t *h_lds = w_lds + (size_t)32 * S;                 // [32][S]  h of the 32 cells at hand
    float *red = reinterpret_cast<float *>(h_lds + (size_t)32 * S);       // [4][32 v][32 u] the waves' shares of the logits tile
    bf16_t *d_lds = reinterpret_cast<bf16_t *>(red + 4 * 1024);           // [32 v][SD]  dlogits, cells contiguous
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nvt = gridDim.x, v0 = blockIdx.x * 32, Sn = gridDim.y, sp = blockIdx.y;
    const int nc = J / 8, nks = J / 16, nkt = J / 32;
    const long long nfr = (long long)B * Tn, fchunk = (nfr + Sn - 1) / Sn;
    const long long f_begin = sp * fchunk, f_end = std::min(nfr, f_begin + fchunk);
    for (int i = tid; i < 32 * nc; i += 256) {
        const int c = (i % nc) * 8, row = i / nc;
        float w8[8];
        ld8(W + (size_t)min(v0 + row, V - 1) * J + c, w8);
        if (v0 + row >= V) {
#pragma unroll
            for (int j = 0; j < 8; ++j) w8[j] = 0.f;
        }
        st8(w_lds + (size_t)row * S + c, w8);
    }
    f32x16 acc[NJT];
#pragma unroll
    for (int i = 0; i < NJT; ++i) acc[i] = (f32x16){0};
    // formula role: thread (vr, cq) owns vocabulary row v0 + vr and the four cells 4cq .. 4cq+3 of the tile, and keeps their fp32 sum for dbias
    const int vr = tid >> 3, cq = tid & 7, vmine = v0 + vr;
    const float bmine = bias[min(vmine, V - 1)];
    float db = 0.f;
    for (long long fr = f_begin; fr < f_end; ++fr) {
        const int b = (int)(fr / Tn), t = (int)(fr % Tn);
        const int tl = min(max(tlen[b], 1), Tn), ul = min(max(ulen[b], 0), U1 - 1);
        if (t >= tl) continue;
        const float gs = gscale[b];
        for (int uc = 0; uc <= ul; uc += 32) {              // 32 lattice cells of this frame
            __syncthreads();                                // the previous cells' reads of h_lds / d_lds are done (first pass: w_lds is staged)
            for (int i = tid; i < 32 * nc; i += 256) {
                const int c = (i % nc) * 8, row = i / nc;
                float e8[8], d8[8], h8[8];
                ld8(enc + ((size_t)b * Tn + t) * J + c, e8);
                ld8(dec + ((size_t)b * U1 + min(uc + row, U1 - 1)) * J + c, d8);
#pragma unroll
                for (int j = 0; j < 8; ++j) h8[j] = lrelu(e8[j] + d8[j], slope);
                st8(h_lds + (size_t)row * S + c, h8);
            }
            __syncthreads();
            f32x16 p = {0};                                 // this wave's k-steps of logits[v][u] = W tile . h^T
            for (int s = wave; s < nks; s += 4)
                p = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(w_lds + (size_t)r * S + 8 * h + 16 * s),
                                                            *reinterpret_cast<const bf16x8 *>(h_lds + (size_t)r * S + 8 * h + 16 * s), p, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 16; ++g) red[wave * 1024 + mfma_row(g, h) * 32 + r] = p[g];
            __syncthreads();
            {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int uu = 4 * cq + j, u = uc + uu, e = vr * 32 + uu;
                    const float logit = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e] + bmine;
                    const long long ci = ((long long)b * Tn + t) * U1 + min(u, U1 - 1);
                    const float c0 = cell[ci], gblank = cell[ncell + ci], gemit = cell[2 * ncell + ci];
                    const int lab = u < ul ? min(max(targets[(size_t)b * ldt + u], 0), V - 1) : -1;
                    o[j] = (u <= ul && vmine < V) ? lazy_dlogit(logit, vmine, c0, gblank, gemit, gs, blank, lab) : 0.f;
                    db += o[j];
                }
                *reinterpret_cast<uint2 *>(d_lds + vr * SD + 4 * cq) = make_uint2(pk_bf16(o[0], o[1]), pk_bf16(o[2], o[3]));
            }
            __syncthreads();
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {                // 16 cells = one k-step of dW[v][j] += dlogits[u][v] h[u][j]
                const bf16x8 ga = *reinterpret_cast<const bf16x8 *>(d_lds + r * SD + 16 * s2 + 8 * h);
#pragma unroll
                for (int i = 0; i < NJT; ++i) {
                    const int kt = wave + 4 * i;
                    if (kt >= nkt) break;
                    bf16x8 hb;
#pragma unroll
                    for (int j = 0; j < 8; ++j) hb[j] = h_lds[(size_t)(16 * s2 + 8 * h + j) * S + kt * 32 + r];
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ga, hb, acc[i], 0, 0, 0);
                }
            }
        }
    }
    float *slab = slab_w + (size_t)sp * V * J;
#pragma unroll
    for (int i = 0; i < NJT; ++i) {
        const int kt = wave + 4 * i;
        if (kt >= nkt) break;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int v = v0 + mfma_row(g, h);
            if (v < V) slab[(size_t)v * J + kt * 32 + r] = acc[i][g];
        }
    }
    db += __shfl_xor(db, 1, 64);                            // the eight cell groups of a vocabulary row, in a fixed order
    db += __shfl_xor(db, 2, 64);
    db += __shfl_xor(db, 4, 64);
    if (cq == 0) slab_b[((size_t)sp * nvt) * 32 + vmine] = db;
}

// frame ranges of the lazy kernel W: about 1024 workgroups over the vocabulary tiles, at most 64 slabs and 128 MiB of them
int lazy_wsplit(int B, int T, int J, int V) {
    long long s = std::min<long long>(64, std::max<long long>(1, 1024 / cdiv(V, 32)));
    s = std::min<long long>(s, std::max<long long>(1, (128ll << 20) / ((long long)V * J * (long long)sizeof(float))));
    return (int)std::min<long long>(s, (long long)B * T);
}

// Workspace of the fused loss: the lattice workspace of tsasr_rnnt_loss_* first (so the split lattice's time-out word sits at the same
// offset), the three cell planes, then the backward's partial sums and slabs.
struct LossWs {
    RnntWs r;
    float *cell, *part_enc, *part_dec, *slab_b, *slab_w;
    long long ncell;
    size_t bytes;
};
LossWs loss_carve(void *ws, int B, int T, int U1, int J, int V) {
    const int nut = cdiv(U1, 32), TS = bwd_tsplit(B, T, U1), S = lazy_wsplit(B, T, J, V), nvt = cdiv(V, 32);
    LossWs w;
    w.r = rnnt_carve(ws, B, T, U1);
    w.ncell = (long long)B * T * U1;
    char *p = (char *)ws + align_up(tsasr_rnnt_loss_workspace_bytes(B, T, U1), 256);
    w.cell = (float *)p;     p += align_up((size_t)3 * w.ncell * sizeof(float), 256);
    w.part_enc = (float *)p; p += align_up((size_t)nut * B * T * J * sizeof(float), 256);
    w.part_dec = (float *)p; p += align_up((size_t)TS * B * U1 * J * sizeof(float), 256);
    w.slab_b = (float *)p;   p += align_up((size_t)S * nvt * 32 * sizeof(float), 256);
    w.slab_w = (float *)p;   p += align_up((size_t)S * V * J * sizeof(float), 256);
    w.bytes = (size_t)(p - (char *)ws);
    return w;
}

size_t lp_lds(int J, int tg) { return std::max((size_t)tg * 32 * (J + 8) * sizeof(bf16_t), (size_t)4 * tg * 32 * sizeof(float4)); }

template <typename T, int TG>
void launch_lp(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt, const int32_t *tlen,
               const int32_t *ulen, const RnntWs &w, int B, int Tn, int U1, int J, int V, int blank, float slope, hipStream_t st) {
    const size_t lds = lp_lds(J, TG);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void *)joint_wide_lp_kernel<T, TG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    joint_wide_lp_kernel<T, TG><<<dim3(cdiv(U1, 32), cdiv(Tn, TG), B), 256, lds, st>>>((const T *)enc, (const T *)dec, W, bias, targets, ldt, tlen, ulen,
                                                                                      w, Tn, U1, J, V, blank, slope);
}
template <typename T>
void launch_lp_any(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt, const int32_t *tlen,
                   const int32_t *ulen, const RnntWs &w, int B, int Tn, int U1, int J, int V, int blank, float slope, hipStream_t st) {
    const int tg = fwd_tg(J);
    if (tg == 4) launch_lp<T, 4>(enc, dec, W, bias, targets, ldt, tlen, ulen, w, B, Tn, U1, J, V, blank, slope, st);
    else if (tg == 3) launch_lp<T, 3>(enc, dec, W, bias, targets, ldt, tlen, ulen, w, B, Tn, U1, J, V, blank, slope, st);
    else launch_lp<T, 2>(enc, dec, W, bias, targets, ldt, tlen, ulen, w, B, Tn, U1, J, V, blank, slope, st);
}

template <typename T, int NKT>
void launch_lazy_x(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt, const float *gscale,
                   const LossWs &w, const int32_t *tlen, const int32_t *ulen, int B, int Tn, int U1, int J, int V, int blank, float slope, int TS,
                   hipStream_t st) {
    const int Vp = (V + 15) / 16 * 16;
    const size_t need = ((size_t)32 * (Vp + 8) + (size_t)32 * (J + 8)) * sizeof(bf16_t);         // the frame's dlogits tile and its h tile
    if (need > 64 * 1024) (void)hipFuncSetAttribute((const void *)joint_wide_lazy_x_kernel<T, NKT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    joint_wide_lazy_x_kernel<T, NKT><<<dim3(cdiv(U1, 32), TS * (J > 640 ? 2 : 1), B), 256, need, st>>>(
        (const T *)enc, (const T *)dec, W, bias, targets, ldt, gscale, w.cell, w.ncell, w.part_enc, w.part_dec, tlen, ulen, Tn, U1, J, V, blank, slope, TS);
}
template <typename T, int NJT>
void launch_lazy_w(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt, const float *gscale,
                   const LossWs &w, const int32_t *tlen, const int32_t *ulen, int B, int Tn, int U1, int J, int V, int blank, float slope, int S,
                   hipStream_t st) {
    const size_t need = (size_t)2 * 32 * (J + 8) * sizeof(bf16_t) + 4 * 1024 * sizeof(float) + 32 * 40 * sizeof(bf16_t);
    if (need > 64 * 1024) (void)hipFuncSetAttribute((const void *)joint_wide_lazy_w_kernel<T, NJT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    joint_wide_lazy_w_kernel<T, NJT><<<dim3(cdiv(V, 32), S), 256, need, st>>>((const T *)enc, (const T *)dec, W, bias, targets, ldt, gscale, w.cell, w.ncell,
                                                                             w.slab_w, w.slab_b, tlen, ulen, B, Tn, U1, J, V, blank, slope);
}

template <typename T>
void launch_lazy_bwd(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt, const float *gscale,
                     void *denc, void *ddec, const LossWs &w, const int32_t *tlen, const int32_t *ulen, int B, int Tn, int U1, int J, int V,
                     int blank, float slope, hipStream_t st) {
    const int nut = cdiv(U1, 32), TS = bwd_tsplit(B, Tn, U1), S = lazy_wsplit(B, Tn, J, V), nkt = cdiv(cdiv(J / 32, J > 640 ? 2 : 1), 4);
    joint_wide_cell_kernel<<<(unsigned)((w.ncell + 255) / 256), 256, 0, st>>>(w.r, tlen, ulen, w.cell, w.ncell, Tn, U1);
#define LAZY_X(N_) launch_lazy_x<T, N_>(enc, dec, W, bias, targets, ldt, gscale, w, tlen, ulen, B, Tn, U1, J, V, blank, slope, TS, st)
    if (nkt <= 1) LAZY_X(1);
    else if (nkt <= 2) LAZY_X(2);
    else LAZY_X(5);
#undef LAZY_X
#define LAZY_W(N_) launch_lazy_w<T, N_>(enc, dec, W, bias, targets, ldt, gscale, w, tlen, ulen, B, Tn, U1, J, V, blank, slope, S, st)
    if (J <= 128) LAZY_W(1);
    else if (J <= 256) LAZY_W(2);
    else if (J <= 640) LAZY_W(5);
    else LAZY_W(8);
#undef LAZY_W
    const long long n_enc = (long long)B * Tn * J, n_dec = (long long)B * U1 * J;
    joint_wide_sum_kernel<T><<<(unsigned)std::min<long long>(4096, (n_enc / 4 + 255) / 256), 256, 0, st>>>(w.part_enc, (T *)denc, n_enc, nut);
    joint_wide_sum_kernel<T><<<(unsigned)std::min<long long>(4096, (n_dec / 4 + 255) / 256), 256, 0, st>>>(w.part_dec, (T *)ddec, n_dec, TS);
}

// argument checks shared by the three fused entry points; 0 = fine
int check_loss_shape(const char *who, int B, int T, int U1, int J, int V, int ldt, int blank, int io_dtype) {
    TSASR_CHECK_ARG(B > 0 && T > 0 && U1 > 0, "%s: empty batch (B=%d T=%d U1=%d)", who, B, T, U1);
    TSASR_CHECK_ARG(B <= 65535 && cdiv(T, 2) <= 65535, "%s: B=%d T=%d beyond the launch grid", who, B, T);
    TSASR_CHECK_ARG(J > 0 && J % 32 == 0 && J <= 1024, "%s: J=%d must be a multiple of 32, at most 1024", who, J);
    TSASR_CHECK_ARG(V > 32 && V <= 1024, "%s: V=%d not supported (33..1024; narrower vocabularies: tsasr_joint_fwd + tsasr_rnnt_loss_fwd)", who, V);
    TSASR_CHECK_ARG(blank >= 0 && blank < V, "%s: blank=%d outside [0,%d)", who, blank, V);
    TSASR_CHECK_ARG(U1 <= 64 * 32, "%s: U1=%d > 2048 lattice columns not supported", who, U1);
    TSASR_CHECK_ARG(ldt >= std::max(U1 - 1, 1), "%s: targets rows of %d labels, U1 - 1 = %d needed", who, ldt, U1 - 1);
    TSASR_CHECK_ARG(io_dtype == TSASR_F32 || io_dtype == TSASR_BF16, "%s: bad io_dtype %d", who, io_dtype);
    return 0;
}

}  // namespace

extern "C" {

int tsasr_joint_wide_fwd(const void *enc, const void *dec, const float *W, const float *bias, float *logits, int B, int T, int U1, int J, int V,
                         int ldl, int io_dtype, float slope, void *stream) {
    TSASR_CHECK_ARG(enc && dec && W && bias && logits, "tsasr_joint_wide_fwd: null pointer");
    TSASR_CHECK_ARG(B > 0 && T > 0 && U1 > 0, "tsasr_joint_wide_fwd: empty batch (B=%d T=%d U1=%d)", B, T, U1);
    TSASR_CHECK_ARG(B <= 65535 && cdiv(T, 2) <= 65535, "tsasr_joint_wide_fwd: B=%d T=%d beyond the launch grid", B, T);
    TSASR_CHECK_ARG(J > 0 && J % 32 == 0 && J <= 1024, "tsasr_joint_wide_fwd: J=%d must be a multiple of 32, at most 1024", J);
    TSASR_CHECK_ARG(V > 32 && V <= 1024, "tsasr_joint_wide_fwd: V=%d not supported (33..1024; narrower vocabularies: tsasr_joint_fwd)", V);
    TSASR_CHECK_ARG(ldl >= V && ldl % 32 == 0, "tsasr_joint_wide_fwd: ldl=%d must be a multiple of 32, at least V=%d", ldl, V);
    TSASR_CHECK_ARG(io_dtype == TSASR_F32 || io_dtype == TSASR_BF16, "tsasr_joint_wide_fwd: bad io_dtype %d", io_dtype);
    hipStream_t st = (hipStream_t)stream;
    const int tg = fwd_tg(J);
    if (io_dtype == TSASR_F32) {
        if (tg == 4) launch_fwd<float, 4>(enc, dec, W, bias, logits, B, T, U1, J, V, ldl, slope, st);
        else if (tg == 3) launch_fwd<float, 3>(enc, dec, W, bias, logits, B, T, U1, J, V, ldl, slope, st);
        else launch_fwd<float, 2>(enc, dec, W, bias, logits, B, T, U1, J, V, ldl, slope, st);
    } else {
        if (tg == 4) launch_fwd<bf16_t, 4>(enc, dec, W, bias, logits, B, T, U1, J, V, ldl, slope, st);
        else if (tg == 3) launch_fwd<bf16_t, 3>(enc, dec, W, bias, logits, B, T, U1, J, V, ldl, slope, st);
        else launch_fwd<bf16_t, 2>(enc, dec, W, bias, logits, B, T, U1, J, V, ldl, slope, st);
    }
    TSASR_CHECK_LAUNCH("tsasr_joint_wide_fwd");
    return 0;
}

/* Workspace of the wide backward: the denc shares of the cdiv(U1, 32) u tiles, the ddec shares of at most 8 frame ranges, one dbias row per
 * workgroup of the dh kernel and at most 64 dW slabs of [V, J], 128 MiB of them at most (csrc/joint_wide.hip carve). */
size_t tsasr_joint_wide_bwd_workspace_bytes(int B, int T, int U1, int J, int V) {
    if (B <= 0 || T <= 0 || U1 <= 0 || J <= 0 || V <= 0) return 0;
    return carve(nullptr, B, T, U1, J, V).bytes;
}

int tsasr_joint_wide_bwd(const float *dlogits, const void *enc, const void *dec, const float *W, void *denc, void *ddec, float *dW, float *dbias,
                         const int32_t *tlen, const int32_t *ulen, int B, int T, int U1, int J, int V, int ldl, int io_dtype, float slope,
                         void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(dlogits && enc && dec && W && denc && ddec && dW && dbias && workspace, "tsasr_joint_wide_bwd: null pointer");
    TSASR_CHECK_ARG(B > 0 && T > 0 && U1 > 0, "tsasr_joint_wide_bwd: empty batch");
    TSASR_CHECK_ARG(B <= 65535, "tsasr_joint_wide_bwd: B=%d beyond the launch grid", B);
    TSASR_CHECK_ARG(J > 0 && J % 32 == 0 && J <= 1024, "tsasr_joint_wide_bwd: J=%d must be a multiple of 32, at most 1024", J);
    TSASR_CHECK_ARG(V > 32 && V <= 1024, "tsasr_joint_wide_bwd: V=%d not supported (33..1024; narrower vocabularies: tsasr_joint_bwd)", V);
    TSASR_CHECK_ARG(ldl >= V && ldl % 4 == 0, "tsasr_joint_wide_bwd: ldl=%d must be a multiple of 4, at least V=%d", ldl, V);
    TSASR_CHECK_ARG(io_dtype == TSASR_F32 || io_dtype == TSASR_BF16, "tsasr_joint_wide_bwd: bad io_dtype %d", io_dtype);
    TSASR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "tsasr_joint_wide_bwd: workspace must be 16-byte aligned");
    TSASR_CHECK_ARG(workspace_bytes >= tsasr_joint_wide_bwd_workspace_bytes(B, T, U1, J, V), "tsasr_joint_wide_bwd: workspace too small");
    const WideWs w = carve(workspace, B, T, U1, J, V);
    hipStream_t st = (hipStream_t)stream;
    if (io_dtype == TSASR_F32) launch_bwd<float>(dlogits, enc, dec, W, denc, ddec, w, tlen, ulen, B, T, U1, J, V, ldl, slope, st);
    else launch_bwd<bf16_t>(dlogits, enc, dec, W, denc, ddec, w, tlen, ulen, B, T, U1, J, V, ldl, slope, st);
    const int nut = cdiv(U1, 32), TS = bwd_tsplit(B, T, U1), S = bwd_wsplit(B, T, J, V), Vp = (V + 15) / 16 * 16;
    tsasr_reduce_submit(w.slab_w, dW, (long long)V * J, S, V * J, 0, st);      // queued while reductions are deferred, else launched on `st`
    tsasr_reduce_submit(w.slab_b, dbias, Vp, B * TS * nut, V, 0, st);
    TSASR_CHECK_LAUNCH("tsasr_joint_wide_bwd");
    return 0;
}

/* ---- fused joint + RNN-T loss: no logits / dlogits tensor (kernels above; include/tsasr_hip.h has the contract) ---- */
size_t tsasr_joint_wide_loss_workspace_bytes(int B, int T, int U1, int J, int V) {
    if (B <= 0 || T <= 0 || U1 <= 0 || J <= 0 || V <= 0) return 0;
    return loss_carve(nullptr, B, T, U1, J, V).bytes;
}

long long tsasr_joint_wide_loss_error_word_offset(int B, int T, int U1, int J, int V) {
    (void)J; (void)V;
    return tsasr_rnnt_loss_error_word_offset(B, T, U1);     // the lattice workspace comes first
}

int tsasr_joint_wide_loss_fwd(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt,
                              const int32_t *tlen, const int32_t *ulen, float *costs, int B, int T, int U1, int J, int V, int blank, int io_dtype,
                              float slope, void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(enc && dec && W && bias && targets && tlen && ulen && costs && workspace, "tsasr_joint_wide_loss_fwd: null pointer");
    if (int rc = check_loss_shape("tsasr_joint_wide_loss_fwd", B, T, U1, J, V, ldt, blank, io_dtype)) return rc;
    TSASR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "tsasr_joint_wide_loss_fwd: workspace must be 16-byte aligned");
    TSASR_CHECK_ARG(workspace_bytes >= tsasr_joint_wide_loss_workspace_bytes(B, T, U1, J, V), "tsasr_joint_wide_loss_fwd: workspace too small");
    const LossWs w = loss_carve(workspace, B, T, U1, J, V);
    hipStream_t st = (hipStream_t)stream;
    if (io_dtype == TSASR_F32) launch_lp_any<float>(enc, dec, W, bias, targets, ldt, tlen, ulen, w.r, B, T, U1, J, V, blank, slope, st);
    else launch_lp_any<bf16_t>(enc, dec, W, bias, targets, ldt, tlen, ulen, w.r, B, T, U1, J, V, blank, slope, st);
    if (int rc = rnnt_launch_alphabeta(w.r, tlen, ulen, costs, B, T, U1, st)) return rc;
    TSASR_CHECK_LAUNCH("tsasr_joint_wide_loss_fwd");
    return 0;
}

int tsasr_joint_wide_loss_bwd(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt,
                              const int32_t *tlen, const int32_t *ulen, const float *gscale, void *denc, void *ddec, float *dW, float *dbias, int B,
                              int T, int U1, int J, int V, int blank, int io_dtype, float slope, void *workspace, size_t workspace_bytes,
                              void *stream) {
    TSASR_CHECK_ARG(enc && dec && W && bias && targets && tlen && ulen && gscale && denc && ddec && dW && dbias && workspace,
                    "tsasr_joint_wide_loss_bwd: null pointer");
    if (int rc = check_loss_shape("tsasr_joint_wide_loss_bwd", B, T, U1, J, V, ldt, blank, io_dtype)) return rc;
    TSASR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "tsasr_joint_wide_loss_bwd: workspace must be 16-byte aligned");
    TSASR_CHECK_ARG(workspace_bytes >= tsasr_joint_wide_loss_workspace_bytes(B, T, U1, J, V), "tsasr_joint_wide_loss_bwd: workspace too small");
    const LossWs w = loss_carve(workspace, B, T, U1, J, V);
    hipStream_t st = (hipStream_t)stream;
    if (io_dtype == TSASR_F32) launch_lazy_bwd<float>(enc, dec, W, bias, targets, ldt, gscale, denc, ddec, w, tlen, ulen, B, T, U1, J, V, blank, slope, st);
    else launch_lazy_bwd<bf16_t>(enc, dec, W, bias, targets, ldt, gscale, denc, ddec, w, tlen, ulen, B, T, U1, J, V, blank, slope, st);
    const int S = lazy_wsplit(B, T, J, V), nvt = cdiv(V, 32);
    tsasr_reduce_submit(w.slab_w, dW, (long long)V * J, S, V * J, 0, st);      // queued while reductions are deferred, else launched on `st`
    tsasr_reduce_submit(w.slab_b, dbias, (long long)nvt * 32, S, V, 0, st);
    TSASR_CHECK_LAUNCH("tsasr_joint_wide_loss_bwd");
    return 0;
}

size_t tsasr_joint_wide_align_workspace_bytes(int B, int T, int U1, int J, int V) {
    (void)J; (void)V;
    return tsasr_rnnt_align_workspace_bytes(B, T, U1);      // three lattice planes and one backpointer bit per cell: nothing grows with V
}

int tsasr_joint_wide_align(const void *enc, const void *dec, const float *W, const float *bias, const int32_t *targets, int ldt,
                           const int32_t *tlen, const int32_t *ulen, int32_t *frames, int ldf, float *scores, int B, int T, int U1, int J, int V,
                           int blank, int io_dtype, float slope, void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(enc && dec && W && bias && targets && tlen && ulen && frames && scores && workspace, "tsasr_joint_wide_align: null pointer");
    if (int rc = check_loss_shape("tsasr_joint_wide_align", B, T, U1, J, V, ldt, blank, io_dtype)) return rc;
    TSASR_CHECK_ARG(ldf >= std::max(U1 - 1, 1), "tsasr_joint_wide_align: ldf=%d < max(U1-1, 1)=%d", ldf, std::max(U1 - 1, 1));
    TSASR_CHECK_ARG(workspace_bytes >= tsasr_joint_wide_align_workspace_bytes(B, T, U1, J, V), "tsasr_joint_wide_align: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    unsigned *bits = nullptr;
    const RnntWs w = align_carve(workspace, B, T, U1, &bits);
    if (io_dtype == TSASR_F32) launch_lp_any<float>(enc, dec, W, bias, targets, ldt, tlen, ulen, w, B, T, U1, J, V, blank, slope, st);
    else launch_lp_any<bf16_t>(enc, dec, W, bias, targets, ldt, tlen, ulen, w, B, T, U1, J, V, blank, slope, st);
    if (int rc = rnnt_launch_viterbi(w, bits, tlen, ulen, frames, ldf, scores, B, T, U1, st)) return rc;
    TSASR_CHECK_LAUNCH("tsasr_joint_wide_align");
    return 0;
}

}  // extern "C"
