// CTC on the encoder's frames (include/tsasr_hip.h "Auxiliary CTC loss"): loss, gradient w.r.t. the raw scores and greedy decoding.
//
//   forward : (1) ctc_row_kernel     one wave per (b,t) row: log-sum-exp over the V valid columns and the COMPACT emission planes
//                                    lpb[b,t] = lp(blank), lpl[b,t,u] = lp(y_u), so that the lattice reads contiguous rows;
//             (2) ctc_chain_kernel   per utterance, for every vocabulary entry the ascending chain of the target positions that carry
//                                    it (head[b,v] -> next[b,u] -> ... -> -1): the gradient sums a repeated label's occupancies along
//                                    it, in that fixed order, instead of with atomics;
//             (3) ctc_lattice_kernel one workgroup per (utterance, direction): alpha and beta' over the S_b = 2 U_b + 1 extended
//                                    states, CTC_K = 4 CONSECUTIVE states per thread (state 4 i is a blank, so thread i needs ONE value
//                                    of thread i - 1 going forward and TWO of thread i + 1 going backward), exchanged through a
//                                    double-buffered LDS row: one barrier per frame. fp32 log space (a row's maximum is taken out every 32 frames), rows
//                                    kept in the workspace.
//   backward: ctc_grad_kernel        one wave per row: dlogits = gscale * (softmax - occupancy).
// beta'(t,s) EXCLUDES the emission of frame t (alpha includes it): occupancy(t,s) = exp(alpha + beta' - log P) needs no emission.
// No atomics, nothing waits for another workgroup, no allocation, no host read: capturable, re-entrant per stream, same bits every run.
#include "common.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int CTC_VMAX = 1024, CTC_UMAX = 2047, CTC_K = 4, CTC_RENORM = 32;
constexpr float LOG2E = 1.44269504089f, LN2 = 0.69314718056f;

struct CtcWs {
    float *lse, *lpb, *lpl, *alpha, *beta, *logp;   // [B*T], [B*T], [B*T,UP], [B*T,SP], [B*T,SP], [B]
    int *head, *next;                               // [B,V], [B,UP]
    int UP, SP;                                     // row lengths: labels (even, >= 2), states (multiple of CTC_K)
};

inline int ctc_up(int U) { return std::max((U + 1) / 2 * 2, 2); }
inline int ctc_sp(int U) { return (2 * U + 1 + CTC_K - 1) / CTC_K * CTC_K; }
inline int ctc_threads(int U) { return std::min(1024, (ctc_sp(U) / CTC_K + 63) / 64 * 64); }

inline size_t ctc_ws_floats(int B, int T, int U, int V) {
    const size_t rows = (size_t)B * T;
    return 2 * rows + rows * ctc_up(U) + 2 * rows * ctc_sp(U) + align_up((size_t)B, 64) + (size_t)B * V + (size_t)B * ctc_up(U);
}

inline CtcWs ctc_carve(void *ws, int B, int T, int U, int V) {
    const size_t rows = (size_t)B * T;
    CtcWs w;
    w.UP = ctc_up(U);
    w.SP = ctc_sp(U);
    float *p = (float *)ws;
    w.alpha = p; p += rows * w.SP;          // (16-byte rows first: the workspace itself is 256-byte aligned)
    w.beta = p; p += rows * w.SP;
    w.lpl = p; p += rows * w.UP;
    w.lse = p; p += rows;
    w.lpb = p; p += rows;
    w.logp = p; p += align_up((size_t)B, 64);
    w.head = (int *)p; p += (size_t)B * V;
    w.next = (int *)p;
    return w;
}

// log(e^a + e^b [+ e^c]) for arguments finite or -inf, as csrc/rnnt.hip's logaddexp_f: (-inf) - (-inf) = NaN is clamped to -200 (IEEE maxNum),
// so an all -inf cell comes out as log(0) + (-inf) = -inf without a branch.
__device__ __forceinline__ float ex2d(float x, float m) { return __builtin_amdgcn_exp2f(fmaxf(x - m, -200.f) * LOG2E); }
__device__ __forceinline__ float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    return fmaf(__builtin_amdgcn_logf(ex2d(a, m) + ex2d(b, m)), LN2, m);
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(fmaxf(a, b), c);
    return fmaf(__builtin_amdgcn_logf(ex2d(a, m) + ex2d(b, m) + ex2d(c, m)), LN2, m);
}

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

// (1) one wave per row, four rows per block. Rows at or beyond T_b are neither read nor written.
template <typename T>
__global__ __launch_bounds__(256) void ctc_row_kernel(const T *__restrict__ x, const int32_t *__restrict__ targets, int ldt,
                                                      const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen, CtcWs w,
                                                      int B, int Tn, int U, int V, int ldl, int blank) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * Tn) return;
    const int b = (int)(row / Tn), t = (int)(row - (long long)b * Tn);
    if (t >= clampi(tlen[b], 1, Tn)) return;
    const T *xr = x + row * ldl;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, ld1(xr + v));
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += __expf(ld1(xr + v) - m);
    s = wave_sum(s);
    const float lse = m + __logf(s);
    if (lane == 0) {
        w.lse[row] = lse;
        w.lpb[row] = ld1(xr + blank) - lse;
    }
    const int Ub = clampi(ulen[b], 0, U);
    const int32_t *tg = targets + (long long)b * ldt;
    float *lp = w.lpl + row * w.UP;
    for (int u = lane; u < Ub; u += 64) lp[u] = ld1(xr + clampi(tg[u], 0, V - 1)) - lse;
}

// (2) one block per utterance; the clamped labels sit in LDS (every thread of a scan reads the same word: a broadcast)
__global__ __launch_bounds__(256) void ctc_chain_kernel(const int32_t *__restrict__ targets, int ldt, const int32_t *__restrict__ ulen, CtcWs w,
                                                        int U, int V) {
    __shared__ short y[CTC_UMAX + 1];
    const int b = blockIdx.x, Ub = clampi(ulen[b], 0, U);
    const int32_t *tg = targets + (long long)b * ldt;
    for (int u = threadIdx.x; u < Ub; u += 256) y[u] = (short)clampi(tg[u], 0, V - 1);
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 256) {
        int h = -1;
        for (int u = 0; u < Ub; ++u)
            if (y[u] == v) { h = u; break; }
        w.head[(size_t)b * V + v] = h;
    }
    for (int u = threadIdx.x; u < Ub; u += 256) {
        int n = -1;
        for (int k = u + 1; k < Ub; ++k)
            if (y[k] == y[u]) { n = k; break; }
        w.next[(size_t)b * w.UP + u] = n;
    }
}

// (3) blockIdx.y = 0: alpha and the cost; 1: beta'. Thread i owns states 4 i .. 4 i + 3 = blank, label 2 i, blank, label 2 i + 1.
// Emissions of the next frame are requested before the current frame's arithmetic; states at or beyond S_b are held at -inf by a select,
// so whatever the unwritten part of an emission row holds never enters a sum.
__global__ __launch_bounds__(1024) void ctc_lattice_kernel(const int32_t *__restrict__ targets, int ldt, const int32_t *__restrict__ tlen,
                                                           const int32_t *__restrict__ ulen, float *__restrict__ costs, CtcWs w, int Tn, int U,
                                                           int V) {
    __shared__ float2 xch[2][1024];
    __shared__ float fin[2], red[16];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int Tb = clampi(tlen[b], 1, Tn), Ub = clampi(ulen[b], 0, U), Sb = 2 * Ub + 1;
    const int s0 = CTC_K * tid, u0 = 2 * tid;
    const int32_t *tg = targets + (long long)b * ldt;
    int y[4];   // labels u0 - 1 .. u0 + 2; distinct negatives where there is none
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int u = u0 - 1 + j;
        y[j] = (u >= 0 && u < Ub) ? clampi(tg[u], 0, V - 1) : -1 - j;
    }
    const bool v0 = s0 < Sb, v1 = s0 + 1 < Sb, v2 = s0 + 2 < Sb, v3 = s0 + 3 < Sb;
    const bool lab = u0 < w.UP;                  // this thread's two label emissions lie inside the (even-length) row
    const bool own = s0 < w.SP;                  // ... and its four states inside the state row
    const size_t row0 = (size_t)b * Tn;
    const float NI = -INFINITY;
    // Every CTC_RENORM frames the row's maximum is taken out of all its states (one more barrier on those frames): log-space values
    // stay within a few hundred units of zero, where fp32 still resolves 1e-5, instead of drifting to -1.5 T (T = 4000: steps of 5e-4).
    // The gradient normalises every row by its own sum, so it never sees the offsets; the cost adds alpha's back (in double).
    auto renorm = [&](float &p0, float &p1, float &p2, float &p3) -> float {
        const float mw = wave_max(fmaxf(fmaxf(p0, p1), fmaxf(p2, p3)));
        if ((tid & 63) == 0) red[tid >> 6] = mw;
        __syncthreads();
        float m = red[0];
        for (int k = 1; k < (nt >> 6); ++k) m = fmaxf(m, red[k]);
        if (m == NI) return 0.f;                  // an infeasible utterance's row: nothing to take out
        p0 -= m; p1 -= m; p2 -= m; p3 -= m;
        return m;
    };

    if (blockIdx.y == 0) {
        const bool sk1 = u0 >= 1 && v1 && y[1] != y[0], sk3 = v3 && y[2] != y[1];
        float lb = w.lpb[row0];
        float2 ll = lab ? *reinterpret_cast<const float2 *>(w.lpl + row0 * w.UP + u0) : make_float2(0.f, 0.f);
        double off = 0.0;
        float a0 = s0 == 0 ? lb : NI, a1 = (s0 == 0 && v1) ? ll.x : NI, a2 = NI, a3 = NI;
        if (own) *reinterpret_cast<float4 *>(w.alpha + row0 * w.SP + s0) = make_float4(a0, a1, a2, a3);
        if (Tb > 1) {
            lb = w.lpb[row0 + 1];
            if (lab) ll = *reinterpret_cast<const float2 *>(w.lpl + (row0 + 1) * w.UP + u0);
        }
        for (int t = 1; t < Tb; ++t) {
            const float cb = lb, c0 = ll.x, c1 = ll.y;
            if (t + 1 < Tb) {
                lb = w.lpb[row0 + t + 1];
                if (lab) ll = *reinterpret_cast<const float2 *>(w.lpl + (row0 + t + 1) * w.UP + u0);
            }
            xch[t & 1][tid].x = a3;
            __syncthreads();
            const float p = tid > 0 ? xch[t & 1][tid - 1].x : NI;
            const float n0 = lse2(a0, p) + cb;
            const float n1 = lse3(a1, a0, sk1 ? p : NI) + c0;
            const float n2 = lse2(a2, a1) + cb;
            const float n3 = lse3(a3, a2, sk3 ? a1 : NI) + c1;
            a0 = v0 ? n0 : NI; a1 = v1 ? n1 : NI; a2 = v2 ? n2 : NI; a3 = v3 ? n3 : NI;
            if ((t & (CTC_RENORM - 1)) == 0) off += (double)renorm(a0, a1, a2, a3);
            if (own) *reinterpret_cast<float4 *>(w.alpha + (row0 + t) * w.SP + s0) = make_float4(a0, a1, a2, a3);
        }
        // log P = log(e^alpha(T_b-1, S_b-1) + e^alpha(T_b-1, S_b-2))
        if (tid == 0) fin[1] = NI;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int s = Sb - 1 - e;
            if (s >= 0 && (s >> 2) == tid) {
                const int k = s & 3;
                fin[e] = k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
            }
        }
        __syncthreads();
        if (tid == 0) {
            const float logp = lse2(fin[0], fin[1]);
            w.logp[b] = logp;
            costs[b] = logp == NI ? 0.f : (float)-((double)logp + off);      // infeasible (T_b < U_b + repeats): zero_infinity
        }
    } else {
        const bool skA = v3 && y[2] != y[1];                       // state 4 i + 1 -> 4 i + 3
        const bool skB = s0 + 5 < Sb && y[3] != y[2];              // state 4 i + 3 -> 4 i + 5
        float b0 = (s0 == Sb - 1 || s0 == Sb - 2) ? 0.f : NI, b1 = (s0 + 1 == Sb - 1 || s0 + 1 == Sb - 2) ? 0.f : NI;
        float b2 = (s0 + 2 == Sb - 1 || s0 + 2 == Sb - 2) ? 0.f : NI, b3 = (s0 + 3 == Sb - 1 || s0 + 3 == Sb - 2) ? 0.f : NI;
        if (own) *reinterpret_cast<float4 *>(w.beta + (row0 + Tb - 1) * w.SP + s0) = make_float4(b0, b1, b2, b3);
        float lb = w.lpb[row0 + Tb - 1];
        float2 ll = lab ? *reinterpret_cast<const float2 *>(w.lpl + (row0 + Tb - 1) * w.UP + u0) : make_float2(0.f, 0.f);
        int buf = 0;
        for (int t = Tb - 2; t >= 0; --t, buf ^= 1) {
            const float cb = lb, c0 = ll.x, c1 = ll.y;                // emissions of frame t + 1
            lb = w.lpb[row0 + t];
            if (lab) ll = *reinterpret_cast<const float2 *>(w.lpl + (row0 + t) * w.UP + u0);
            const float g0 = v0 ? b0 + cb : NI, g1 = v1 ? b1 + c0 : NI, g2 = v2 ? b2 + cb : NI, g3 = v3 ? b3 + c1 : NI;
            xch[buf][tid] = make_float2(g0, g1);
            __syncthreads();
            const float2 q = tid + 1 < nt ? xch[buf][tid + 1] : make_float2(NI, NI);
            b0 = lse2(g0, g1);
            b1 = lse3(g1, g2, skA ? g3 : NI);
            b2 = lse2(g2, g3);
            b3 = lse3(g3, q.x, skB ? q.y : NI);
            if ((t & (CTC_RENORM - 1)) == 0) renorm(b0, b1, b2, b3);
            if (own) *reinterpret_cast<float4 *>(w.beta + (row0 + t) * w.SP + s0) = make_float4(b0, b1, b2, b3);
        }
    }
}

// backward: one wave per row. Blank occupancy = wave sum over the U_b + 1 even states; a label's = the walk along its chain (ascending u).
template <typename T>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const T *__restrict__ x, const int32_t *__restrict__ tlen, const int32_t *__restrict__ ulen,
                                                       const float *__restrict__ gscale, T *__restrict__ dx, CtcWs w, int B, int Tn, int U, int V,
                                                       int ldl, int blank) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * Tn) return;
    const int b = (int)(row / Tn), t = (int)(row - (long long)b * Tn);
    T *dr = dx + row * ldl;
    const float logp = w.logp[b];
    if (t >= clampi(tlen[b], 1, Tn) || logp == -INFINITY) {
        for (int v = lane; v < ldl; v += 64) st1(dr + v, 0.f);
        return;
    }
    const T *xr = x + row * ldl;
    const int Ub = clampi(ulen[b], 0, U);
    const float *al = w.alpha + row * w.SP, *be = w.beta + row * w.SP;
    // Every frame's occupancies sum to one (sum_s alpha(t,s) beta'(t,s) = P for every t): normalise them by the ROW's own sum instead of by
    // log P, so that the drift alpha and beta have gathered over their T_b - 1 steps cancels and a row of dlogits sums to zero.
    const int Sb = 2 * Ub + 1;
    float m = -INFINITY;
    for (int s = lane; s < Sb; s += 64) m = fmaxf(m, al[s] + be[s]);
    m = wave_max(m);
    float z = 0.f, ob = 0.f;
    for (int s = lane; s < Sb; s += 64) {      // (64 is even: a lane sees blanks only or labels only)
        const float e = __builtin_amdgcn_exp2f((al[s] + be[s] - m) * LOG2E);
        z += e;
        ob += (s & 1) ? 0.f : e;
    }
    z = wave_sum(z);
    ob = wave_sum(ob);
    const float rz = 1.f / z;
    ob *= rz;
    const float lse = w.lse[row], g = gscale[b];
    const int *head = w.head + (size_t)b * V, *next = w.next + (size_t)b * w.UP;
    for (int v = lane; v < ldl; v += 64) {
        float r = 0.f;
        if (v < V) {
            float occ = v == blank ? ob : 0.f;
            for (int u = head[v]; u >= 0; u = next[u]) occ += __builtin_amdgcn_exp2f((al[2 * u + 1] + be[2 * u + 1] - m) * LOG2E) * rz;
            r = g * (__expf(ld1(xr + v) - lse) - occ);
        }
        st1(dr + v, r);
    }
}

// greedy decoding: one block per utterance walks its frames in chunks of 256: a wave takes the argmax of a frame (lowest index among equal
// scores), then the chunk's kept frames (not blank, not the previous frame's label) are compacted behind the running count with a ballot.
template <typename T>
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const T *__restrict__ x, const int32_t *__restrict__ tlen, int32_t *__restrict__ tokens,
                                                         int ldo, int32_t *__restrict__ ntok, int Tn, int V, int ldl, int blank) {
    __shared__ int arg[256];
    __shared__ int wtot[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Tb = clampi(tlen[b], 0, Tn);
    int32_t *out = tokens + (long long)b * ldo;
    int count = 0, prev = -1;
    for (int c0 = 0; c0 < Tb; c0 += 256) {
        for (int i = 0; i < 64; ++i) {
            const int t = c0 + wv * 64 + i;
            if (t >= Tb) break;
            const T *xr = x + ((long long)b * Tn + t) * ldl;
            float best = -INFINITY;
            int bi = 0x7fffffff;
            for (int v = lane; v < V; v += 64) {
                const float xv = ld1(xr + v);
                if (xv > best || bi == 0x7fffffff) { best = xv; bi = v; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(best, off);
                const int oi = __shfl_xor(bi, off);
                if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            if (lane == 0) arg[wv * 64 + i] = bi;
        }
        __syncthreads();
        const int t = c0 + tid;
        const int a = t < Tb ? arg[tid] : blank;
        const int p = tid > 0 ? arg[tid > 0 ? tid - 1 : 0] : prev;
        const bool keep = t < Tb && a != blank && a != p;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wtot[wv] = __popcll(bal);
        const int nprev = arg[min(255, Tb - 1 - c0)];
        __syncthreads();
        int off = count + __popcll(bal & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; ++k) off += wtot[k];
        if (keep) out[off] = a;
        count += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        prev = nprev;
        __syncthreads();
    }
    for (int i = count + tid; i < ldo; i += 256) out[i] = -1;
    if (tid == 0) ntok[b] = count;
}

int ctc_check(const char *who, int B, int T, int U, int V, int ldl, int blank, int io_dtype) {
    TSASR_CHECK_ARG(B > 0 && T > 0, "%s: empty batch (B=%d T=%d)", who, B, T);
    TSASR_CHECK_ARG(V >= 1 && V <= CTC_VMAX, "%s: V=%d outside [1, %d]", who, V, CTC_VMAX);
    TSASR_CHECK_ARG(ldl >= V && ldl % 8 == 0, "%s: rows must be padded to a multiple of 8 elements (V=%d ldl=%d)", who, V, ldl);
    TSASR_CHECK_ARG(U >= 0 && U <= CTC_UMAX, "%s: U=%d outside [0, %d] (one workgroup owns a lattice: 2 U + 1 <= 4095 states)", who, U, CTC_UMAX);
    TSASR_CHECK_ARG(blank >= 0 && blank < V, "%s: blank=%d outside [0,%d)", who, blank, V);
    TSASR_CHECK_ARG(io_dtype == TSASR_F32 || io_dtype == TSASR_BF16, "%s: io_dtype=%d", who, io_dtype);
    return 0;
}

}  // namespace

extern "C" {

size_t tsasr_ctc_loss_workspace_bytes(int B, int T, int U, int V) {
    if (B <= 0 || T <= 0 || U < 0 || U > CTC_UMAX || V < 1 || V > CTC_VMAX) return 0;
    return align_up(ctc_ws_floats(B, T, U, V) * sizeof(float), 256);
}

int tsasr_ctc_loss_fwd(const void *logits, const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen, float *costs, int B, int T,
                       int U, int V, int ldl, int blank, int io_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(logits && targets && tlen && ulen && costs && workspace, "tsasr_ctc_loss_fwd: null pointer");
    if (int rc = ctc_check("tsasr_ctc_loss_fwd", B, T, U, V, ldl, blank, io_dtype)) return rc;
    TSASR_CHECK_ARG(ldt >= U, "tsasr_ctc_loss_fwd: ldt=%d < U=%d", ldt, U);
    TSASR_CHECK_ARG((size_t)workspace % 16 == 0 && workspace_bytes >= tsasr_ctc_loss_workspace_bytes(B, T, U, V),
                    "tsasr_ctc_loss_fwd: workspace too small or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const CtcWs w = ctc_carve(workspace, B, T, U, V);
    const unsigned rowblocks = (unsigned)(((long long)B * T + 3) / 4);
    if (io_dtype == TSASR_BF16)
        ctc_row_kernel<bf16_t><<<rowblocks, 256, 0, st>>>((const bf16_t *)logits, targets, ldt, tlen, ulen, w, B, T, U, V, ldl, blank);
    else
        ctc_row_kernel<float><<<rowblocks, 256, 0, st>>>((const float *)logits, targets, ldt, tlen, ulen, w, B, T, U, V, ldl, blank);
    ctc_chain_kernel<<<B, 256, 0, st>>>(targets, ldt, ulen, w, U, V);
    ctc_lattice_kernel<<<dim3(B, 2), ctc_threads(U), 0, st>>>(targets, ldt, tlen, ulen, costs, w, T, U, V);
    TSASR_CHECK_LAUNCH("tsasr_ctc_loss_fwd");
    return 0;
}

int tsasr_ctc_loss_bwd(const void *logits, const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen, const float *gscale,
                       void *dlogits, int B, int T, int U, int V, int ldl, int blank, int io_dtype, const void *workspace, size_t workspace_bytes,
                       void *stream) {
    TSASR_CHECK_ARG(logits && targets && tlen && ulen && gscale && dlogits && workspace, "tsasr_ctc_loss_bwd: null pointer");
    if (int rc = ctc_check("tsasr_ctc_loss_bwd", B, T, U, V, ldl, blank, io_dtype)) return rc;
    TSASR_CHECK_ARG(ldt >= U, "tsasr_ctc_loss_bwd: ldt=%d < U=%d", ldt, U);
    TSASR_CHECK_ARG((size_t)workspace % 16 == 0 && workspace_bytes >= tsasr_ctc_loss_workspace_bytes(B, T, U, V),
                    "tsasr_ctc_loss_bwd: workspace too small or not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const CtcWs w = ctc_carve(const_cast<void *>(workspace), B, T, U, V);
    const unsigned rowblocks = (unsigned)(((long long)B * T + 3) / 4);
    if (io_dtype == TSASR_BF16)
        ctc_grad_kernel<bf16_t><<<rowblocks, 256, 0, st>>>((const bf16_t *)logits, tlen, ulen, gscale, (bf16_t *)dlogits, w, B, T, U, V, ldl, blank);
    else
        ctc_grad_kernel<float><<<rowblocks, 256, 0, st>>>((const float *)logits, tlen, ulen, gscale, (float *)dlogits, w, B, T, U, V, ldl, blank);
    TSASR_CHECK_LAUNCH("tsasr_ctc_loss_bwd");
    return 0;
}

int tsasr_ctc_greedy(const void *logits, const int32_t *tlen, int32_t *tokens, int ldo, int32_t *ntok, int B, int T, int V, int ldl, int blank,
                     int io_dtype, void *stream) {
    TSASR_CHECK_ARG(logits && tlen && tokens && ntok, "tsasr_ctc_greedy: null pointer");
    if (int rc = ctc_check("tsasr_ctc_greedy", B, T, 0, V, ldl, blank, io_dtype)) return rc;
    TSASR_CHECK_ARG(ldo >= T, "tsasr_ctc_greedy: ldo=%d < T=%d (a frame can emit a token)", ldo, T);
    hipStream_t st = (hipStream_t)stream;
    if (io_dtype == TSASR_BF16)
        ctc_greedy_kernel<bf16_t><<<B, 256, 0, st>>>((const bf16_t *)logits, tlen, tokens, ldo, ntok, T, V, ldl, blank);
    else
        ctc_greedy_kernel<float><<<B, 256, 0, st>>>((const float *)logits, tlen, tokens, ldo, ntok, T, V, ldl, blank);
    TSASR_CHECK_LAUNCH("tsasr_ctc_greedy");
    return 0;
}

}  // extern "C"
