// The RNN-T lattice workspace: plane layout, lattice plans and carving, shared by csrc/rnnt.hip (rnnt_lp / rnnt_alphabeta / rnnt_grad /
// rnnt_viterbi) and csrc/joint_wide.hip (the fused joint + loss kernels, which fill the same planes without a logits tensor).
#pragma once
#include <algorithm>

#include "common.h"

struct RnntWs {
    float *lpb, *lpe_in, *lpe_out, *alpha, *beta, *lse, *logp, *xch;
    unsigned *err;   // split lattice only: set to 1 by a workgroup whose wait for its neighbour's edge value ran out (the costs are then NaN)
    int U1P, K;      // padded columns per frame; columns per lane of the ONE-wave layout
    int KT, NW, NC;  // the lattice kernel's plan: columns per thread, waves per workgroup, column blocks (workgroups) per (utterance, direction)
    int R, sh;       // rows per utterance plane; column -> skew shift (31: no skew)
};

inline int rnnt_K(int U1) {
    int K = 1;
    while (64 * K < U1) K *= 2;
    return K;
}

// Lattice plan: columns per thread x waves x column blocks of rnnt_alphabeta_kernel, and whether the planes are stored SKEWED.
// A lattice step is an anti-diagonal: thread g (columns KT*g ..) works on frame t = s - g (alpha) resp. t + g = const (beta). Stored frame-major
// (row t), the 64 lanes of a wave touch 64 different rows per load / store - 64 cache lines per wave-instruction through the CU's one address
// path: at B = 1, T' = 4000, U = 1920 the four waves spent 1.36 us per step on six such instructions (5.8 ms per direction, "17 GB/s"). Stored at
// row t + g(u) instead (g(u) = u / KT; G - 1 more rows per utterance), a step's operands and results are ONE contiguous row for the whole
// lattice, in both directions. The layout is private to this header: rnnt_lp / joint_wide_lp write it, rnnt_grad / joint_wide_cell read it through ws_at().
//   U1 <= 256 (the benchmark's U = 120): one wave per lattice, frame-major planes (skewing them costs rnnt_lp / rnnt_grad their coalescing:
//            +10 - 20 us per step at configs[1], measured);
//   longer targets: skewed planes, up to 8 waves in one workgroup per lattice (2.5 ms at B = 1, T' = 4000, U = 1920: the CU's VALUs, ~0.55 us per
//            step for 2048 columns); a single long utterance (2 B NC <= 32 workgroups): one single-wave workgroup per block of 128 columns
//            instead (rnnt_alphabeta_kernel MC: 1.9 ms; at B = 8, T' = 1000, U = 400 the 8-wave form was faster, 0.72 against 0.75 ms).
// tsasr_rnnt_lattice_plan() overrides the choice (tests run all three forms against each other, bit for bit; tools/rnnt_bench.py).
inline int g_plan_skew = -1, g_plan_waves = -1, g_plan_mc = -1;      // -1: default (C++17 inline variables: one instance for the library)
inline void rnnt_plan(int B, int U1, int *KT, int *NW, int *NC, int *skew) {
    const int max_waves = g_plan_waves > 0 ? g_plan_waves : 8;
    const int skew_mode = g_plan_skew >= 0 ? g_plan_skew : 1;        // 0 never, 1 when the lattice runs on more than one wave, 2 always
    const int mc_cols = g_plan_mc >= 0 ? g_plan_mc : 2;              // 0: never split a lattice over workgroups; 1, 2, 4: columns per thread of a split one
    const int mc_limit = g_plan_mc > 0 ? 2048 : 32;                  // (forced: whatever still fits on the chip at once)
    const int K = rnnt_K(U1);
    *NC = 1;
    if (K >= 8 && skew_mode != 0 && (mc_cols == 1 || mc_cols == 2 || mc_cols == 4) && (long long)2 * B * (K / mc_cols) <= mc_limit) {
        *KT = mc_cols; *NW = 1; *NC = K / mc_cols; *skew = 1;
        return;
    }
    int nw = 1;
    if (K >= 8) {                                  // at least 2 columns per thread
        nw = std::min(max_waves, K / 2);
        while (nw & (nw - 1)) nw &= nw - 1;        // power of two
    }
    *KT = K / nw;
    *NW = nw;
    *skew = skew_mode == 2 || (skew_mode == 1 && nw > 1);
}

inline size_t rnnt_plane_floats(int B, int T, int U1) {
    int kt, nw, nc, skew;
    rnnt_plan(B, U1, &kt, &nw, &nc, &skew);
    return (size_t)B * (T + (skew ? 64 * nw * nc - 1 : 0)) * 64 * rnnt_K(U1);
}
inline size_t rnnt_xch_floats(int B, int T, int U1) {
    int kt, nw, nc, skew;
    rnnt_plan(B, U1, &kt, &nw, &nc, &skew);
    return nc > 1 ? (size_t)2 * B * nc * (T + 1) + 64 : 0;      // (+ 64: the split lattice's error word, see AB_SPIN_LIMIT)
}

inline RnntWs rnnt_carve(void *ws, int B, int T, int U1) {
    RnntWs w;
    int skew;
    w.K = rnnt_K(U1);
    w.U1P = 64 * w.K;
    rnnt_plan(B, U1, &w.KT, &w.NW, &w.NC, &skew);
    w.R = T + (skew ? 64 * w.NW * w.NC - 1 : 0);
    w.sh = 31;
    if (skew) { w.sh = 0; while ((1 << w.sh) < w.KT) ++w.sh; }
    const size_t n = rnnt_plane_floats(B, T, U1);
    float *p = reinterpret_cast<float *>(ws);
    w.lpb = p; w.lpe_in = p + n; w.lpe_out = p + 2 * n; w.alpha = p + 3 * n; w.beta = p + 4 * n; w.lse = p + 5 * n;
    w.logp = p + 6 * n;
    w.xch = w.logp + align_up((size_t)B, 64);
    w.err = w.NC > 1 ? reinterpret_cast<unsigned *>(w.xch + rnnt_xch_floats(B, T, U1) - 64) : nullptr;
    return w;
}

// element (b, t, u) of a lattice plane
__device__ __forceinline__ size_t ws_at(const RnntWs &w, int b, int t, int u) { return ((size_t)b * w.R + t + (u >> w.sh)) * w.U1P + u; }

// ---- forced alignment: plan and workspace of rnnt_viterbi_kernel (csrc/rnnt.hip has the description) ----
inline void align_plan(int U1, int *KT, int *NW) {
    const int K = rnnt_K(U1);
    int nw = 1;
    if (K >= 8) {
        nw = std::min(8, K / 2);
        while (nw & (nw - 1)) nw &= nw - 1;
    }
    *KT = K / nw;
    *NW = nw;
}
inline size_t align_plane_floats(int B, int T, int U1) {
    int kt, nw;
    align_plan(U1, &kt, &nw);
    return (size_t)B * (T + (nw > 1 ? 64 * nw - 1 : 0)) * 64 * rnnt_K(U1);
}
inline size_t align_bits_words(int B, int T, int U1) { return (size_t)B * cdiv(T, 32) * 64 * rnnt_K(U1); }

inline RnntWs align_carve(void *ws, int B, int T, int U1, unsigned **bits) {
    RnntWs w = {};
    w.K = rnnt_K(U1);
    w.U1P = 64 * w.K;
    align_plan(U1, &w.KT, &w.NW);
    w.NC = 1;
    w.R = T + (w.NW > 1 ? 64 * w.NW - 1 : 0);
    w.sh = 31;
    if (w.NW > 1) { w.sh = 0; while ((1 << w.sh) < w.KT) ++w.sh; }
    const size_t n = align_plane_floats(B, T, U1);
    float *p = reinterpret_cast<float *>(ws);
    w.lpb = p; w.lpe_in = p + n; w.lpe_out = w.lse = p + 2 * n;      // (lpe_out / lse: written by rnnt_lp, same cell by the same lane; not read)
    *bits = reinterpret_cast<unsigned *>(p + 3 * n);
    return w;
}

// csrc/rnnt.hip: the lattice and the best-path kernels on planes that are already filled (whoever filled them)
int rnnt_launch_alphabeta(RnntWs w, const int32_t *tlen, const int32_t *ulen, float *costs, int B, int T, int U1, hipStream_t st);
int rnnt_launch_viterbi(RnntWs w, unsigned *bits, const int32_t *tlen, const int32_t *ulen, int32_t *frames, int ldf, float *scores, int B, int T,
                        int U1, hipStream_t st);
