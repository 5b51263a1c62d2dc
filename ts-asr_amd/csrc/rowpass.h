// The row pass of the residual tail + LayerNorm family, its arithmetic written once:
//     s = res + alpha * timemask(dropout_p(x + bias)) ;  y = LayerNorm(s) * gamma + beta  [;  z = LayerNorm(y) * gamma2 + beta2]
// and its backward. elementwise.hip builds add_layernorm{,2}_{fwd,bwd}_kernel from these pieces, linear_ln.hip the row pass behind its
// GEMM; what differs between them - where x comes from, how many LayerNorms follow - stays in the kernels. A lane owns ITERS chunks of
// N = 16 bytes / sizeof(T) columns, chunk `it` at column (it * LPR + l) * N, LPR = 64 lanes per row (one wave) or 32 (half a wave).
// Every piece is forced inline and keeps nothing alive of its own: several instantiations of the kernels stand at 256 VGPRs.
#pragma once
#include "common.h"

template <typename T> struct Vec;  // 16-byte vector of T
template <> struct Vec<float> { static constexpr int N = 4; };
template <> struct Vec<bf16_t> { static constexpr int N = 8; };

template <typename T, int N> __device__ __forceinline__ void ldv(const T *p, float (&o)[N]);
template <> __device__ __forceinline__ void ldv<float, 4>(const float *p, float (&o)[4]) {
    const float4 a = *reinterpret_cast<const float4 *>(p);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
}
template <> __device__ __forceinline__ void ldv<bf16_t, 8>(const bf16_t *p, float (&o)[8]) { ld8(p, o); }
template <> __device__ __forceinline__ void ldv<float, 8>(const float *p, float (&o)[8]) { ld8(p, o); }   // fp32 parameters beside bf16 rows
template <typename T, int N> __device__ __forceinline__ void stv(T *p, const float (&v)[N]);
template <> __device__ __forceinline__ void stv<float, 4>(float *p, const float (&v)[4]) {
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void stv<bf16_t, 8>(bf16_t *p, const float (&v)[8]) { st8(p, v); }

// sum over the LPR lanes of a row. Both are made of wave-wide instructions: the two halves of a half-wave kernel stay in every loop
// together, up to the last reduction (loads clamped, stores guarded by row_valid, no early exit)
template <int LPR> __device__ __forceinline__ float lanes_sum(float v) { return LPR == 32 ? half_wave_sum(v) : wave_sum(v); }

// ---- operand prologue -----------------------------------------------------------------------------------------------------------
// ONE round trip: every operand of a row - the device seed, the utterance length, the parameters, the row - is requested up front,
// unconditionally (optional ones from a stand-in address, columns clamped) and masked afterwards. `if (seed_dev) seed += *seed_dev`,
// `valid_lens ? valid_lens[..] : ..` and `if (bias) load` are guarded loads: each was waited for where it stood, and drained every
// other request of the row with it - three dependent round trips in front of the row's own.
struct TailOperands {
    const unsigned long long *seed_p;
    const int32_t *vl_p;
    const float *bias_p;
    int trows;
    bool has_bias, has_vl;
    __device__ __forceinline__ int length_of(long long row) const { return vl_p[has_vl ? row / trows : 0]; }
    __device__ __forceinline__ bool live(long long row, int vl) const { return !has_vl || ((int)(row % trows) < vl); }
};
__device__ __forceinline__ TailOperands tail_operands(const float *bias, const unsigned long long *seed_dev, const int32_t *valid_lens,
                                                      int Trows, const float *standin) {
    const bool has_bias = bias != nullptr, has_vl = valid_lens != nullptr;
    return {seed_dev ? seed_dev : reinterpret_cast<const unsigned long long *>(standin),
            has_vl ? valid_lens : reinterpret_cast<const int32_t *>(standin), has_bias ? bias : standin, has_vl ? max(Trows, 1) : 1,
            has_bias, has_vl};
}
// column of this lane's chunk `it`, clamped into the row: where the row's operands and the parameters are requested from
template <int N, int LPR> __device__ __forceinline__ int col_clamped(int it, int l, int D) { return min((it * LPR + l) * N, D - N); }

// counter-based dropout of the tail: the keep mask of the chunk at column c of `row` (thr, dk: drop_thr16(p), drop_key(seed)); the
// backward regenerates it
template <int N> __device__ __forceinline__ unsigned tail_keep_mask(long long row, int D, int c, float p, DropKey dk, unsigned thr) {
    return p > 0.f ? drop_keep_mask<N>((unsigned long long)row * D + c, dk, thr) : ~0u;
}

// The pieces below work on ONE element: the loops over a lane's chunks stay in the kernels, which index their register arrays directly.
// (Handing a chunk to a piece by reference lets the compiler turn a whole [ITERS][N] array into one wide vector, which costs the larger
// instantiations an occupancy step: profiles/rowpass_refactor_notes.md.)

// ---- forward --------------------------------------------------------------------------------------------------------------------
// the tail: s, rounded to the stored type - the statistics are those of the STORED row, as a separate LayerNorm reading it would see.
// x: the value from global memory (linear_ln.hip: the GEMM's accumulator rounded to bf16), keep: this element's bit of the keep mask,
// ks: drop_scale16(thr)
template <typename T>
__device__ __forceinline__ float tail_value(float x, float b, float r, bool has_bias, float p, bool keep, float ks, bool live, float alpha) {
    float t = x + (has_bias ? b : 0.f);
    if (p > 0.f) t = keep ? t * ks : 0.f;
    t = live ? t * alpha : 0.f;
    t += r;
    if (sizeof(T) == 2) t = (float)(bf16_t)t;
    return t;
}

// row statistics: the mean from the lanes' sums, then (over the register copy of the row) the centred squares and 1 / sqrt(var + eps)
template <int LPR> __device__ __forceinline__ float row_mean(float sum, int D) { return lanes_sum<LPR>(sum) / D; }
__device__ __forceinline__ float centred_sq(float v, float mu) { const float d = v - mu; return d * d; }
template <int LPR> __device__ __forceinline__ float row_rstd(float q, int D, float eps) { return rsqrtf(lanes_sum<LPR>(q) / D + eps); }

// normalise and affine. ROUND: to the stored type, for a LayerNorm whose output the next one reads
template <typename T, bool ROUND> __device__ __forceinline__ float ln_value(float v, float mu, float rs, float g, float b) {
    float t = (v - mu) * rs * g + b;
    if (ROUND && sizeof(T) == 2) t = (float)(bf16_t)t;
    return t;
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// LayerNorm backward of one row, first half: the two row sums that the second half needs after their reductions. dv: gradient of the
// LayerNorm's output, h: its normalised input. Returns dv * gamma. (The column partials dgamma += dv * h, dbeta += dv are the caller's:
// accumulators reached through a reference are vectorised differently.)
__device__ __forceinline__ float ln_bwd_sums(float dv, float h, float gm, float &s1, float &s2) {
    const float g = dv * gm;
    s1 += g;
    s2 += g * h;
    return g;
}
// second half: gradient of the LayerNorm's input, m1 / m2 the row means of the two sums
__device__ __forceinline__ float ln_bwd_dx(float gd, float h, float rs, float m1, float m2) { return rs * (gd - m1 - h * m2); }

// tail backward: dx = alpha * timemask * dropmask/(1-p) * ds (also what the column partial of dbias sums)
__device__ __forceinline__ float tail_bwd_value(float ds, float p, bool keep, float ks, bool live, float alpha) {
    float g = live ? ds * alpha : 0.f;
    if (p > 0.f) g = keep ? g * ks : 0.f;
    return g;
}
