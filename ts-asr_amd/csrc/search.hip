// Greedy transducer search on the device (gfx950): one persistent workgroup per utterance walks the encoder frames.
//
// Replaces speechbrain/decoders/transducer.py:138-218 (transducer_greedy_decode): per frame the joint of the frame with the current
// predictor output, the classifier, log-softmax, argmax; an utterance whose best symbol is not blank appends it and advances its
// predictor (embedding -> one LSTM step -> projection) - at most one symbol per frame. The reference (and ts-asr_amd/decoders.py's host
// loop, kept for other network shapes) issues ~15 library launches per frame; here the predictor state (h, c, projected output)
// stays in LDS for the whole utterance and one launch decodes the batch.
//
//   logits[v] = b_head[v] + sum_k W_head[v][k] * LeakyReLU(enc[b,t,k] + pn[k])            (Transducer_joint "sum" + Linear head)
//   LSTM step (torch gate order i, f, g, o):  gates = W_ih x + b_ih + W_hh h + b_hh,  x = emb[token]
//   pn = W_proj h + b_proj
// Matrix-vector products: one wave per output row (rows w, w+4, ...), lanes split the inner dimension in 16-byte pieces (whole rows
// are read as contiguous lines, from L2: the 2-4 MB of recurrent weights are shared by all utterances), DPP wave reduction, the row's
// value lands in LDS. All arithmetic fp32; weights fp32 (master parameters) or bf16 (the training step's shadow copies).
#include "common.h"

#include <algorithm>

namespace {

constexpr int SEARCH_THREADS = 1024;   // 16 waves: the matrix-vector products are latency chains per wave

__host__ __device__ inline int round4(int v) { return (v + 3) & ~3; }

// The weights of the predictor and of the joint's head
struct NetArgs {
    const float *emb;           // [V_emb, E] fp32 (one-hot table or learned)
    const void *w_ih, *w_hh;    // [4H, E], [4H, H]  (wdtype)
    const float *b_ih, *b_hh;   // [4H] fp32 (may be NULL)
    const void *w_proj;         // [J, H] (wdtype)
    const float *b_proj;        // [J] or NULL
    const void *w_head;         // [V, J] (wdtype)
    const float *b_head;        // [V] or NULL
};

struct GreedyArgs {
    const void *enc;            // [B, T, J] io dtype
    NetArgs net;
    int *preds;                 // [B, T]: symbol emitted at frame t, -1 = blank
    float *logp_sum;            // [B]: sum of the emitted symbols' log-probabilities
    int B, T, J, H, E, V, blank;
    float slope;
    float *state;               // STREAM: [B, S] fp32, S = 2H + J + 4 (tsasr_greedy_decode's state)
    const int *n_valid;         // STREAM: [B] frames of this chunk to decode
};

template <typename WT> __device__ __forceinline__ void ld4w(const WT *p, float (&o)[4]);
template <> __device__ __forceinline__ void ld4w<float>(const float *p, float (&o)[4]) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <> __device__ __forceinline__ void ld4w<bf16_t>(const bf16_t *p, float (&o)[4]) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
}

// out[r] = bias[r] (+ bias2[r]) + sum_k W[r][k] x[k]  (+ sum_e W2[r][e] x2[e], E2 <= 64), r < rows; x in LDS, K % 4 == 0, K <= 1024.
// A wave takes RB rows per pass: all their 16-byte pieces are requested before the first is used (one memory round trip per RB rows,
// not per row: with one row at a time a predictor step took 380 us), the lane's slice of x sits in registers for the whole call.
// ACC (the LM's LSTM cells: the input and the recurrent product are two calls): out[r] += the row's value.
template <typename WT, int RB, int NC, bool ACC = false>   // NC = pieces of 256 columns per row (K <= 256 * NC)
__device__ __forceinline__ void gemv_rows_nc(const WT *__restrict__ W, int rows, int K, const float *x, const float *__restrict__ bias,
                                             const float *__restrict__ bias2, const WT *__restrict__ W2, int E2, const float *x2, float *out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const float xe = (W2 && lane < E2) ? x2[lane] : 0.f;
    float xr[NC][4];                                  // x[k], k = c * 256 + lane * 4 .. +3
    constexpr int nc = NC;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = c * 256 + lane * 4 + q;
            xr[c][q] = k < K ? x[k] : 0.f;
        }
    for (int r0 = wave * RB; r0 < rows; r0 += nw * RB) {
        float w[RB][NC][4], w2[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int r = min(r0 + i, rows - 1);      // clamped: always issued, the surplus rows are not stored
            const WT *wr = W + (size_t)r * K;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = min(c * 256 + lane * 4, K - 4);
                ld4w<WT>(wr + k, w[i][c]);
            }
            w2[i] = W2 ? (float)W2[(size_t)r * E2 + min(lane, E2 - 1)] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            float acc = (W2 && lane < E2) ? w2[i] * xe : 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                acc += w[i][c][0] * xr[c][0] + w[i][c][1] * xr[c][1] + w[i][c][2] * xr[c][2] + w[i][c][3] * xr[c][3];
            acc = wave_sum(acc);
            const int r = r0 + i;
            if constexpr (ACC) {
                if (lane == 0 && r < rows) out[r] += acc;
            } else {
                if (lane == 0 && r < rows) out[r] = acc + (bias ? bias[r] : 0.f) + (bias2 ? bias2[r] : 0.f);
            }
        }
    }
}

template <typename WT>
__device__ __forceinline__ void gemv_rows(const WT *__restrict__ W, int rows, int K, const float *x, const float *__restrict__ bias,
                                          const float *__restrict__ bias2, const WT *__restrict__ W2, int E2, const float *x2, float *out) {
    if (K <= 512) gemv_rows_nc<WT, 8, 2>(W, rows, K, x, bias, bias2, W2, E2, x2, out);         // (registers: RB * NC * 4 weights in flight)
    else if (K <= 768) gemv_rows_nc<WT, 4, 3>(W, rows, K, x, bias, bias2, W2, E2, x2, out);
    else gemv_rows_nc<WT, 4, 4>(W, rows, K, x, bias, bias2, W2, E2, x2, out);
}

// out[r] += sum_k W[r][k] x[k]: the second operand of a sum whose width is past gemv_rows' 64-column side operand
template <typename WT>
__device__ __forceinline__ void gemv_rows_acc(const WT *__restrict__ W, int rows, int K, const float *x, float *out) {
    if (K <= 512) gemv_rows_nc<WT, 8, 2, true>(W, rows, K, x, nullptr, nullptr, nullptr, 0, nullptr, out);
    else if (K <= 768) gemv_rows_nc<WT, 4, 3, true>(W, rows, K, x, nullptr, nullptr, nullptr, 0, nullptr, out);
    else gemv_rows_nc<WT, 4, 4, true>(W, rows, K, x, nullptr, nullptr, nullptr, 0, nullptr, out);
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + __expf(-x)); }

// One predictor step by the whole workgroup, all in LDS: x = emb[tok] (E floats), gates = W_ih x + b_ih + W_hh h + b_hh, the LSTM cell on
// h | c in place, pn = W_proj h + b_proj. h | c are the caller's; ends behind a barrier. The embedding row enters the gates as the
// 64-column side operand of the recurrent product; WIDE (E <= 1024) keeps that route for E <= 64 and otherwise adds a second product: a
// dense one (gemv_rows_acc) when the rows of W_ih are 16-byte pieces (E % 4 == 0, a learned embedding), else one thread per gate row adds
// W_ih[r][e] * x[e] over the NON-ZERO x[e] only - for the frozen one-hot table (E = V - 1) that is one column of W_ih per token.
template <typename WT, bool WIDE>
__device__ __forceinline__ void predictor_step(const NetArgs &N, int E, int H, int J, int tok, float *x, float *h, float *c, float *gates,
                                               float *pn) {
    const int tid = threadIdx.x;
    const WT *w_ih = (const WT *)N.w_ih, *w_hh = (const WT *)N.w_hh;
    for (int e = tid; e < E; e += SEARCH_THREADS) x[e] = N.emb[(size_t)tok * E + e];
    __syncthreads();
    if (!WIDE || E <= 64) {
        gemv_rows<WT>(w_hh, 4 * H, H, h, N.b_ih, N.b_hh, w_ih, E, x, gates);
    } else {
        gemv_rows<WT>(w_hh, 4 * H, H, h, N.b_ih, N.b_hh, nullptr, 0, nullptr, gates);
        __syncthreads();
        if (E % 4 == 0) {
            gemv_rows_acc<WT>(w_ih, 4 * H, E, x, gates);
        } else {
            for (int r = tid; r < 4 * H; r += SEARCH_THREADS) {
                float acc = 0.f;
                for (int e = 0; e < E; ++e) {
                    const float xe = x[e];                     // the same LDS word for every thread: a uniform branch
                    if (xe != 0.f) acc += (float)w_ih[(size_t)r * E + e] * xe;
                }
                gates[r] += acc;
            }
        }
    }
    __syncthreads();
    for (int u = tid; u < H; u += SEARCH_THREADS) {
        const float ig = sigmoid_f(gates[u]), fg = sigmoid_f(gates[H + u]), gg = tanhf(gates[2 * H + u]), og = sigmoid_f(gates[3 * H + u]);
        const float cn = fg * c[u] + ig * gg;
        c[u] = cn;
        h[u] = og * tanhf(cn);
    }
    __syncthreads();
    gemv_rows<WT>((const WT *)N.w_proj, J, H, h, N.b_proj, nullptr, nullptr, 0, nullptr, pn);
    __syncthreads();
}

// STREAM: the predictor state of utterance b is loaded from / stored to A.state[b] = [h (H) | c (H) | pn (J) | last symbol | logp sum |
// primed flag | 0]; a state with primed flag 0 (all zeros) is primed with the blank symbol first, as the one-call decoder does. Only the
// first n_valid[b] frames are decoded (preds of the rest: -1); with n_valid[b] == 0 the state is neither read for priming nor written.
//
// WIDE (tsasr_greedy_decode's wide: V <= 1024, E <= 1024) switches three things, the rest is one body:
//   - x and logits hold round_up(E, 4) and round_up(V, 4) floats instead of 64 each, and 64 floats of reduction space follow them:
//     red[16] wave maxima | redi[16] wave candidates | reds[16] wave sums | the emit flag;
//   - the arg max (lowest index among ties) and the sum of its log-softmax term: one vocabulary entry per thread, reduced per wave and
//     then over the workgroup's 16 waves in wave order, instead of in wave 0 alone;
//   - the emit flag reaches the workgroup through red[48] instead of logits[63].
// and predictor_step<WT, true> takes the embedding row by its three routes.
template <typename T, typename WT, bool STREAM, bool WIDE>
__global__ __launch_bounds__(SEARCH_THREADS) void greedy_decode_kernel(const GreedyArgs A) {
    extern __shared__ __attribute__((aligned(16))) float gs[];
    const int Ep = WIDE ? round4(A.E) : 64, Vp = WIDE ? round4(A.V) : 64;
    float *h = gs, *c = h + A.H, *pn = c + A.H, *z = pn + A.J, *gates = z + A.J, *x = gates + 4 * A.H, *logits = x + Ep, *red = logits + Vp;
    float *flag = WIDE ? red + 48 : logits + 63;
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x;
    const T *enc = (const T *)A.enc + (size_t)b * A.T * A.J;
    float lsum = 0.f;
    int tbeg = -1, tend = A.T;
    float *st = nullptr;
    if (STREAM) {
        const int S = 2 * A.H + A.J + 4;
        st = A.state + (size_t)b * S;
        tend = min(max(A.n_valid[b], 0), A.T);
        for (int t = tid; t < A.T; t += SEARCH_THREADS)
            if (t >= tend) A.preds[(size_t)b * A.T + t] = -1;
        if (tend == 0) {                            // workgroup-uniform: nothing to decode, the state stays as it is
            if (tid == 0) A.logp_sum[b] = st[2 * A.H + A.J + 1];
            return;
        }
        const bool primed = st[2 * A.H + A.J + 2] != 0.f;
        for (int i = tid; i < 2 * A.H + A.J; i += SEARCH_THREADS) gs[i] = st[i];   // h | c | pn are contiguous in LDS and in the state
        if (tid == 0) s_tok = primed ? (int)st[2 * A.H + A.J] : A.blank;
        lsum = st[2 * A.H + A.J + 1];
        if (primed) tbeg = 0;
    } else {
        for (int i = tid; i < A.H; i += SEARCH_THREADS) h[i] = c[i] = 0.f;
        if (tid == 0) s_tok = A.blank;
    }
    __syncthreads();
    // step(-1): the predictor is primed with the blank symbol (transducer.py:160-170); then one pass per frame
    for (int t = tbeg; t < tend; ++t) {
        int tok = s_tok;                        // symbol to feed the predictor with (every thread reads the same LDS word)
        bool advance = (t < 0);
        if (t >= 0) {
            for (int k = tid; k < A.J; k += SEARCH_THREADS) {
                const float v = ld1(enc + (size_t)t * A.J + k) + pn[k];
                z[k] = v > 0.f ? v : v * A.slope;
            }
            __syncthreads();
            gemv_rows<WT>((const WT *)A.net.w_head, A.V, A.J, z, A.net.b_head, nullptr, nullptr, 0, nullptr, logits);
            __syncthreads();
            // arg max (lowest index among ties) and the sum of its log-softmax term; thread 0 gets both
            int pos = 0;
            float s = 0.f;
            if constexpr (WIDE) {
                const int lane = tid & 63, wave = tid >> 6;
                int *redi = reinterpret_cast<int *>(red + 16);
                float *reds = red + 32;
                const float v = tid < A.V ? logits[tid] : -INFINITY;      // V <= SEARCH_THREADS: one vocabulary entry per thread
                const float wm = wave_max(v);
                if (lane == 0) red[wave] = wm;
                __syncthreads();
                float m = red[0];
#pragma unroll
                for (int w = 1; w < SEARCH_THREADS / 64; ++w) m = fmaxf(m, red[w]);
                const unsigned long long eq = __ballot(v == m && tid < A.V);
                const float ws = wave_sum(tid < A.V ? __expf(v - m) : 0.f);
                if (lane == 0) {
                    redi[wave] = eq ? wave * 64 + __ffsll((long long)eq) - 1 : 0x7fffffff;
                    reds[wave] = ws;
                }
                __syncthreads();
                if (tid == 0) {
                    pos = redi[0];
                    s = reds[0];
#pragma unroll
                    for (int w = 1; w < SEARCH_THREADS / 64; ++w) {
                        pos = min(pos, redi[w]);
                        s += reds[w];
                    }
                }
            } else if (tid < 64) {              // one wave holds the vocabulary
                const float v = tid < A.V ? logits[tid] : -INFINITY;
                float m = v;
                m = wave_max(m);
                const unsigned long long eq = __ballot(v == m && tid < A.V);
                pos = __ffsll((long long)eq) - 1;
                s = wave_sum(tid < A.V ? __expf(v - m) : 0.f);
            }
            if (tid == 0) {
                const bool emit = pos != A.blank && pos < A.V;             // (pos >= V: no entry equals the maximum, a NaN among the logits)
                A.preds[(size_t)b * A.T + t] = emit ? pos : -1;
                if (emit) { lsum += -__logf(s); s_tok = pos; }     // log-softmax at the maximum = -log(sum exp(v - m))
                *flag = emit ? 1.f : 0.f;
            }
            __syncthreads();
            advance = *flag != 0.f;
            tok = s_tok;
        }
        if (advance) predictor_step<WT, WIDE>(A.net, A.E, A.H, A.J, tok, x, h, c, gates, pn);   // workgroup-uniform
    }
    if (tid == 0) A.logp_sum[b] = lsum;
    if (STREAM) {
        __syncthreads();
        for (int i = tid; i < 2 * A.H + A.J; i += SEARCH_THREADS) st[i] = gs[i];
        if (tid == 0) {
            st[2 * A.H + A.J] = (float)s_tok;
            st[2 * A.H + A.J + 1] = lsum;
            st[2 * A.H + A.J + 2] = 1.f;
        }
    }
}


// ------------------------------------------------------------------------------------------------------------------------------------
// Beam transducer search (speechbrain/decoders/transducer.py:220-373, restated in decoders.py's host loop and oracle beam_decode): one
// persistent workgroup per utterance. Per frame, A = hypotheses to extend (the last frame's beam), beam = those that emitted blank here.
// Until |beam| >= beam_size: a = first entry of A with the largest logp / len (len counts the blank prefix); stop once the first best
// beam entry has logp >= state_beam + logp(a); remove a; run the predictor on a's last token from a's state; top-k (k = beam_size) of
// log_softmax(head(LeakyReLU(enc[t] + pn))); blank appends a copy of a (same node, same state) to the beam, a non-blank within
// expand_beam of the best non-blank appends a's extension (new state) to A. Scores are fp64 (the host loop adds Python floats).
//
// Bookkeeping: A lives in LDS as an append-only array (removal = a flag, so "first in insertion order" is "lowest index"); a hypothesis
// is a node of a token tree ((token, parent) int pairs in the workspace) and the predictor step of a node (pn | h | c) is computed once,
// on its first expansion, into a slot of the workspace: a hypothesis that survives a frame is re-expanded with the joint alone. At the
// end of a frame the new nodes on the beam's paths are promoted into the tree (in creation order), all other new nodes and every slot
// not held by the beam are recycled. Workspace of one utterance: header (16 ints: primed, status, nbeam, tree size, frames) + beam
// entries | tree | slots; a zeroed header is the start of a stream.
//
// TIMES (tsasr_beam_search's frames): the search also reports the encoder frame at which each token was emitted. The search
// never merges paths, so a tree node is one concrete path and its emission frame is one value: an extension appended to A at loop index t
// records (frames of this stream decoded by earlier calls) + t in Afrm, beside Atok / Alen; the promotion step copies it into a node-frame
// array parallel to the tree (after the slots in the workspace: the timed layout is the untimed one plus align16(4 * nodes) bytes per
// utterance), and the n-best read-out walks it up the tree beside the tokens. Nothing the search decides reads a frame: hypotheses and
// scores are those of the untimed form, bit for bit. The frames of a stream are absolute only if its header was zeroed as a whole at the
// start: the stream form takes "frames decoded so far" from hdr[4] whether or not the stream is primed, so hdr[0] == 0 over a stale
// hdr[4] would shift every frame of the stream by that stale count (the untimed form only ever adds to the word).
//
// Contextual biasing (tsasr_beam_search's bias; the BIAS instantiations, whose arguments alone carry BeamBiasArgs): a prefix trie of phrases per utterance in CSR form
// (child_off / child_tok / child_to / pending, states relative to the utterance's own graph at row base[b]) and one trie state per
// hypothesis: Actx beside Afrm in LDS, nctx[node] in the workspace after the node-frame array (align16(4 * nodes) bytes more per
// utterance), written at promotion beside nfrm. A non-blank extension by sym moves the state (beam_bias_step: a binary search over the
// state's child_tok by the appending thread) and adds d last, one __dadd_rn: +w for a matched token, -pending[s] for a match given up
// (+w again if sym opens a phrase at the root). The n-best read-out ranks and reports (logp - pending[state]) / len, the stored beam keeps
// logp as it is, so pieces give the bits of one call. No failure links: a failed match restarts at the root with the current token only.
// base[b] < 0: utterance b is not biased (its scores are those of the plain search, bit for bit).
constexpr int BEAM_MAXK = 64;            // beam_size <= min(V, 64), nbest <= 64

struct BeamEnt {
    double logp;
    int node, len, slot, tok;
};

struct BeamLayout {
    size_t hdr, tree, per_utt;
    int nn, ns;
};

__host__ __device__ inline size_t beam_align16(size_t v) { return (v + 15) & ~(size_t)15; }
// lmw (LM fusion): floats a slot holds after pn | h | c, the LM step of the node: lm_logp[64, WIDE: round_up(V, 4)] | lm_h[L * Hl] | lm_c[L * Hl]
__host__ __device__ inline BeamLayout beam_layout(int T, int H, int J, int beam, int cap, int lmw = 0) {
    BeamLayout L;
    L.nn = 1 + (T + 1) * beam + cap;                          // tree nodes: root + (typically <= beam promoted per frame) + slack
    L.ns = cap + beam;                                         // slots: the beam's + one per node expanded in a frame (<= cap)
    L.hdr = beam_align16(64 + sizeof(BeamEnt) * (size_t)beam);
    L.tree = beam_align16(8 * (size_t)L.nn);
    L.per_utt = L.hdr + L.tree + (size_t)L.ns * (size_t)(J + 2 * H + lmw) * sizeof(float);
    return L;
}
__host__ __device__ inline int beam_lm_slot_floats(bool wide, int V, int layers, int hidden) {
    return (wide ? round4(V) : 64) + 2 * layers * hidden;
}
// TIMES: the node-frame array (one int per tree node) follows the untimed layout of each utterance; bias: then the node-state array
__host__ __device__ inline size_t beam_per_utt(const BeamLayout &L, bool times, bool bias = false) {
    return L.per_utt + ((times ? 1 : 0) + (bias ? 1 : 0)) * beam_align16(sizeof(int) * (size_t)L.nn);
}

struct BeamBiasArgs {
    const int *child_off, *child_tok, *child_to;   // CSR over the packed rows; child_off holds absolute edge indices
    const double *pending;                          // [rows] bonus a half-matched phrase would have to give back
    const int *base;                                // [B] first row of the utterance's graph (< 0: none)
    const double *weight;                           // [B] nats per matched token
    int rows;
};

// step(s, v) of the graph at row gb: the child of s on v, else the root's child on v, else the root
__device__ __forceinline__ int beam_bias_child(const BeamBiasArgs &G, int row, int v) {
    int lo = G.child_off[row], hi = G.child_off[row + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, t = G.child_tok[mid];
        if (t == v) return G.child_to[mid];
        if (t < v) lo = mid + 1; else hi = mid;
    }
    return -1;
}
__device__ __forceinline__ int beam_bias_step(const BeamBiasArgs &G, int gb, double w, int s, int v, double &d) {
    int c = beam_bias_child(G, gb + s, v);
    if (c >= 0) { d = w; return c; }
    d = -G.pending[gb + s];
    c = beam_bias_child(G, gb, v);
    if (c >= 0) { d = __dadd_rn(d, w); return c; }
    return 0;
}

struct BeamArgs {
    const void *enc;            // [B, T, J] io dtype (T = frames of this call)
    NetArgs net;
    unsigned char *ws;          // [B, layout.per_utt]
    const int *n_valid;         // [B] or NULL (= T, and the workspace is started afresh)
    int *hyps;                  // [B, nbest, Lmax]
    int *lens;                  // [B, nbest]: tokens of the hypothesis (-1: no such entry)
    double *scores;             // [B, nbest]: logp / len
    int *status;                // [B]
    int B, T, J, H, E, V, blank, beam, nbest, cap, Lmax, max_frames;
    double state_beam, expand_beam;
    float slope;
    int *frames;                // TIMES: [B, nbest, Lmax] emission frame of each token of hyps (absolute in the stream)
};

// LM fusion (tsasr_beam_search's lm; transducer.py:264-266, 311-351, 386-409 with lobes/models/RNNLM.py): a second recurrent network beside
// the predictor, embedding -> L stacked LSTM cells -> nb blocks of Linear, LayerNorm, LeakyReLU -> Linear to V -> log_softmax. Its step is a
// function of (token, parent's LM state) like the predictor's, so it runs once per node, in the node's predictor phase, into the node's
// slot; a non-blank extension by sym scores (logp(a) + logp_joint[sym]) + weight * lm_logp[sym]; the top-k, the expand_beam test and the
// blank copies read the joint alone. The kernel's arguments grow only for the LM instantiations (BeamKernArgs<true>).
struct BeamLmArgs {
    const float *emb;                     // [V, E] fp32
    const void *w_ih[4], *w_hh[4];        // layer l: [4 Hl, l == 0 ? E : Hl], [4 Hl, Hl] (wdtype)
    const float *b_ih[4], *b_hh[4];       // [4 Hl] fp32 or NULL
    const void *w_dnn[2];                 // block k: [D, k == 0 ? Hl : D] (wdtype)
    const float *b_dnn[2], *ln_g[2], *ln_b[2];   // [D] fp32 (NULL: no bias / no affine)
    const void *w_out;                    // [V, nb > 0 ? D : Hl] (wdtype)
    const float *b_out;
    float ln_eps[2];
    int L, Hl, E, nb, D;
    float slope;
    double weight;
};
template <bool LM, bool BIAS = false> struct BeamKernArgs : BeamArgs {};
template <> struct BeamKernArgs<true, false> : BeamArgs { BeamLmArgs lm; };
template <> struct BeamKernArgs<false, true> : BeamArgs { BeamBiasArgs bias; };
template <> struct BeamKernArgs<true, true> : BeamArgs { BeamLmArgs lm; BeamBiasArgs bias; };

template <typename P> __device__ __forceinline__ P beam_pick4(const P (&a)[4], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }

// log_softmax over the workgroup, one entry per thread (v = -INFINITY for a thread past the vocabulary): the maximum and the sum of
// exp(v - max) are reduced per wave, then over the 16 waves in wave order by every thread alike, so the bits do not depend on which wave
// arrives first. expf / logf, not the fast intrinsics: the values enter fp64 score sums. red: 32 floats of LDS; two barriers.
__device__ __forceinline__ float beam_wide_log_softmax(float v, float *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float wm = wave_max(v);
    if (lane == 0) red[wave] = wm;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    const float ws = wave_sum(v == -INFINITY ? 0.f : expf(v - m));
    if (lane == 0) red[16 + wave] = ws;
    __syncthreads();
    float s = red[16];
#pragma unroll
    for (int w = 1; w < 16; ++w) s += red[16 + w];
    return (v - m) - logf(s);
}

// One LM step of a node, by the whole workgroup: token, the parent's LM state plm (a slot's LM part, or null: zeros) -> this node's LM part
// slm = lm_logp[64] | lm_h[L Hl] | lm_c[L Hl] and s_lmlp[64]. LDS: lx[max(E, Hl, D)], lh[2 Hl] (h | c of the layer), lgt[max(4 Hl, D)],
// llg[64], s_stat[2]. Ends behind a barrier. WIDE (beam_search_kernel's): lm_logp, llg and s_lmlp hold round_up(V, 4) floats, the
// head's log-softmax is taken over the workgroup (red: beam_wide_log_softmax's 32 floats).
template <typename WT, bool WIDE = false>
__device__ __forceinline__ void beam_lm_step(const BeamLmArgs &M, int V, int tok, const float *plm, float *slm, float *lx, float *lh,
                                             float *lgt, float *llg, float *s_lmlp, float *s_stat, float *red = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hl = M.Hl, L = M.L, D = M.D;
    const int lmo = WIDE ? (V + 3) & ~3 : 64;                // floats of lm_logp in a slot's LM part
    for (int e = tid; e < M.E; e += SEARCH_THREADS) lx[e] = M.emb[(size_t)tok * M.E + e];
    for (int l = 0; l < L; ++l) {
        const WT *w_ih = (const WT *)beam_pick4(M.w_ih, l), *w_hh = (const WT *)beam_pick4(M.w_hh, l);
        const float *b_ih = beam_pick4(M.b_ih, l), *b_hh = beam_pick4(M.b_hh, l);
        for (int i = tid; i < 2 * Hl; i += SEARCH_THREADS)
            lh[i] = plm ? plm[lmo + (i < Hl ? l * Hl + i : (L + l) * Hl + (i - Hl))] : 0.f;
        __syncthreads();
        gemv_rows<WT>(w_ih, 4 * Hl, l == 0 ? M.E : Hl, lx, b_ih, b_hh, nullptr, 0, nullptr, lgt);
        __syncthreads();
        gemv_rows_acc<WT>(w_hh, 4 * Hl, Hl, lh, lgt);
        __syncthreads();
        for (int u = tid; u < Hl; u += SEARCH_THREADS) {
            const float ig = sigmoid_f(lgt[u]), fg = sigmoid_f(lgt[Hl + u]), gg = tanhf(lgt[2 * Hl + u]), og = sigmoid_f(lgt[3 * Hl + u]);
            const float cn = fg * lh[Hl + u] + ig * gg;
            const float hn = og * tanhf(cn);
            lx[u] = hn;                                      // the next layer's input
            slm[lmo + l * Hl + u] = hn;
            slm[lmo + (L + l) * Hl + u] = cn;
        }
        __syncthreads();
    }
    int K = Hl;
    for (int k = 0; k < M.nb; ++k) {                        // Linear -> LayerNorm (two passes) -> LeakyReLU
        const WT *w = (const WT *)(k == 0 ? M.w_dnn[0] : M.w_dnn[1]);
        const float *bv = k == 0 ? M.b_dnn[0] : M.b_dnn[1], *g = k == 0 ? M.ln_g[0] : M.ln_g[1], *be = k == 0 ? M.ln_b[0] : M.ln_b[1];
        const float eps = k == 0 ? M.ln_eps[0] : M.ln_eps[1];
        gemv_rows<WT>(w, D, K, lx, bv, nullptr, nullptr, 0, nullptr, lgt);
        __syncthreads();
        if (wave == 0) {
            float s = 0.f;
            for (int i = lane; i < D; i += 64) s += lgt[i];
            const float mean = wave_sum(s) / (float)D;
            float q = 0.f;
            for (int i = lane; i < D; i += 64) { const float d = lgt[i] - mean; q += d * d; }
            const float var = wave_sum(q) / (float)D;
            if (lane == 0) { s_stat[0] = mean; s_stat[1] = 1.f / sqrtf(var + eps); }
        }
        __syncthreads();
        for (int i = tid; i < D; i += SEARCH_THREADS) {
            const float v = (lgt[i] - s_stat[0]) * s_stat[1] * (g ? g[i] : 1.f) + (be ? be[i] : 0.f);
            lx[i] = v > 0.f ? v : v * M.slope;
        }
        __syncthreads();
        K = D;
    }
    gemv_rows<WT>((const WT *)M.w_out, V, K, lx, M.b_out, nullptr, nullptr, 0, nullptr, llg);
    __syncthreads();
    if constexpr (WIDE) {
        const float lp = beam_wide_log_softmax(tid < V ? llg[tid] : -INFINITY, red);
        if (tid < V) {
            s_lmlp[tid] = lp;
            slm[tid] = lp;
        }
    } else if (wave == 0) {
        const float v = lane < V ? llg[lane] : -INFINITY;
        const float m = wave_max(v);
        const float s = wave_sum(lane < V ? expf(v - m) : 0.f);
        const float lp = lane < V ? (v - m) - logf(s) : 0.f;
        s_lmlp[lane] = lp;
        slm[lane] = lp;
    }
    __syncthreads();
}

// (key, index) of the larger key; equal keys: the lower index (Python max: the first maximal entry)
__device__ __forceinline__ void beam_argmax_step(double &k, int &i, int mask) {
    const double k2 = __shfl_xor(k, mask);
    const int i2 = __shfl_xor(i, mask);
    if (k2 > k || (k2 == k && i2 < i)) { k = k2; i = i2; }
}

// (key, index) of the better top-k candidate: the larger value, equal values: the lower index; index INT_MAX = no candidate
__device__ __forceinline__ void beam_topk_pick(float &k, int &i, float k2, int i2) {
    if (i2 != INT_MAX && (i == INT_MAX || k2 > k || (k2 == k && i2 < i))) { k = k2; i = i2; }
}

// WIDE (tsasr_beam_search's wide: subword vocabularies, V <= 1024 and E <= 1024) switches four things; the search itself - A in LDS, fp64
// scores and keys, memoised predictor (and LM) steps in slots, promotion into the token tree, status words, stream resume, TIMES - is
// one body:
//   - widths: x, lg, s_lmlp, llg and the lm_logp part of a slot hold round_up(E, 4) / round_up(V, 4) floats instead of 64;
//   - embedding x = emb[token]: predictor_step<WT, true>'s three routes instead of the one side operand;
//   - log-softmax: one vocabulary entry per thread, maximum and sum reduced over the 16 waves in wave order (beam_wide_log_softmax)
//     instead of in wave 0; top-k: beam rounds of a workgroup arg max over the entries not taken yet, ordered by (value descending,
//     index ascending) - the order the one-wave rank counting gives. A round: the wave's best by shuffles, the 16 wave candidates
//     through LDS (two buffers in turn: one barrier per round), every thread reduces them alike, the winner's thread records itself.
//     No atomics, no dependence on which wave arrives first;
//   - the appends: by thread 0 behind a barrier instead of by lane 0 of wave 0 behind a wave fence.
// Dynamic LDS: h | c | pn | z | gates | x[Ep] | lg[Vp] | WIDE: red[96] | A arrays (cap) | LM: lx | lh | lgt | llg[Vp] | s_lmlp[Vp] |
// s_stat[2], Ep = Vp = 64 unless WIDE; red = wave maxima[16] | wave sums[16] | top-k wave values[2][16] | top-k wave indices[2][16].
template <typename T, typename WT, bool TIMES, bool LM, bool WIDE, bool BIAS>
__global__ __launch_bounds__(SEARCH_THREADS) void beam_search_kernel(const BeamKernArgs<LM, BIAS> A) {
    extern __shared__ __attribute__((aligned(16))) float bsm[];
    const int H = A.H, J = A.J, cap = A.cap;
    const int Ep = WIDE ? round4(A.E) : 64, Vp = WIDE ? round4(A.V) : 64;
    float *h = bsm, *c = h + H, *pn = c + H, *z = pn + J, *gates = z + J, *x = gates + 4 * H, *lg = x + Ep;
    float *red = WIDE ? lg + Vp : nullptr;
    double *Alp = reinterpret_cast<double *>(lg + Vp + (WIDE ? 96 : 0)), *Akey = Alp + cap;
    int *Apar = reinterpret_cast<int *>(Akey + cap), *Atok = Apar + cap, *Alen = Atok + cap, *Aslot = Alen + cap, *Anode = Aslot + cap,
        *Aflag = Anode + cap;                               // flag bit 0: live in A, bit 1: on a path of the closing beam
    int *Afrm = Aflag + cap;                                 // TIMES: frame at which the extension was appended (cap ints more of LDS)
    constexpr bool biased = BIAS;
    int *Actx = Aflag + cap + (TIMES ? cap : 0);             // bias: trie state of the hypothesis (cap ints more of LDS)
    // LM: the LM step's own LDS after the A arrays: lx[max(E, Hl, D)] | lh[2 Hl] | lgt[max(4 Hl, D)] | llg[Vp] (beam_lm_step) |
    // s_lmlp[Vp] (lm_logp of the node being expanded) | s_stat[2] (LayerNorm mean, rstd)
    float *lx = nullptr, *lh = nullptr, *lgt = nullptr, *llg = nullptr, *s_lmlp = nullptr, *s_stat = nullptr;
    int lmw = 0;
    if constexpr (LM) {
        lx = reinterpret_cast<float *>(Aflag + cap + (TIMES ? cap : 0) + (biased ? cap : 0));
        lh = lx + max(max(A.lm.E, A.lm.Hl), A.lm.D);
        lgt = lh + 2 * A.lm.Hl;
        llg = lgt + max(4 * A.lm.Hl, A.lm.D);
        s_lmlp = llg + Vp;
        s_stat = s_lmlp + Vp;
        lmw = beam_lm_slot_floats(WIDE, A.V, A.lm.L, A.lm.Hl);
    }
    __shared__ double s_blp[BEAM_MAXK], s_bkey[BEAM_MAXK], s_tlp[BEAM_MAXK];
    __shared__ int s_bidx[BEAM_MAXK], s_tpos[BEAM_MAXK], s_order[BEAM_MAXK];
    // s_ctl: 0 nA, 1 nbeam (this frame), 2 chosen a, 3 stop (1 frame done, 2 status set), 4 status, 5 n_init, 6 next slot, 7 tree size,
    //        8 compute the predictor step, 9 parent slot, 10 token, 11 A full (appends), 12 tree full (promotion). Each flag is written in
    //        one phase and read right after that phase's barrier, so that no wave reads a word another wave is writing.
    __shared__ int s_ctl[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BeamLayout L = beam_layout(A.max_frames, H, J, A.beam, cap, lmw);
    unsigned char *wsu = A.ws + (size_t)b * beam_per_utt(L, TIMES, biased);
    int *hdr = reinterpret_cast<int *>(wsu);
    BeamEnt *bent = reinterpret_cast<BeamEnt *>(wsu + 64);
    int2 *tree = reinterpret_cast<int2 *>(wsu + L.hdr);
    float *slots = reinterpret_cast<float *>(wsu + L.hdr + L.tree);
    int *nfrm = reinterpret_cast<int *>(wsu + L.per_utt);   // TIMES: nfrm[node] = emission frame of the node's token
    int *nctx = reinterpret_cast<int *>(wsu + beam_per_utt(L, TIMES));   // bias: nctx[node] = trie state of the node's path
    int gb = -1;                                             // bias: first row of this utterance's graph (< 0: not biased)
    double bw = 0.0;
    if constexpr (BIAS) {
        gb = A.bias.base[b];
        if (gb < 0 || gb + 1 >= A.bias.rows) gb = -1;       // (a graph holds at least its root's row and the closing one)
        else bw = A.bias.weight[b];
    }
    const int SWP = J + 2 * H;                               // floats per slot: pn | h | c
    const int SW = SWP + lmw;                                // LM: | lm_logp[Vp] | lm_h | lm_c
    const T *enc = (const T *)A.enc + (size_t)b * A.T * J;
    const bool fresh = A.n_valid == nullptr;
    const int tend = fresh ? A.T : min(max(A.n_valid[b], 0), A.T);
    const int fbase = (TIMES && !fresh) ? hdr[4] : 0;        // frames of this stream decoded before this call (written after the last frame)

    if (tid == 0) {
        const bool primed = !fresh && hdr[0] != 0;
        s_ctl[4] = fresh ? 0 : hdr[1];
        s_ctl[11] = s_ctl[12] = 0;
        if (primed) {
            const int nb = min(max(hdr[2], 1), A.beam);
            s_ctl[5] = nb;
            s_ctl[7] = hdr[3];
        } else {
            s_ctl[5] = 1;
            s_ctl[7] = 1;
        }
    }
    __syncthreads();
    const bool primed = !fresh && hdr[0] != 0;
    if (tid < s_ctl[5]) {                                    // the beam entering this call = the first frame's A
        BeamEnt e = primed ? bent[tid] : BeamEnt{0.0, 0, 1, -1, A.blank};
        Alp[tid] = e.logp;
        Akey[tid] = e.logp / (double)e.len;
        Apar[tid] = -1;
        Atok[tid] = e.tok;
        Alen[tid] = e.len;
        Aslot[tid] = e.slot;
        Anode[tid] = e.node;
        Aflag[tid] = 1;
        if (biased) Actx[tid] = primed ? nctx[e.node] : 0;
    }
    __syncthreads();
    const bool run = s_ctl[4] == 0 && tend > 0;              // workgroup-uniform
    if (run && !primed && tid == 0) {
        tree[0] = make_int2(A.blank, -1);
        if (biased) nctx[0] = 0;
    }

    for (int t = 0; run && t < tend; ++t) {
        if (tid == 0) { s_ctl[0] = s_ctl[5]; s_ctl[1] = 0; s_ctl[6] = 0; s_ctl[3] = 0; }
        __syncthreads();
        while (true) {
            if (wave == 0) {
                const int nA = s_ctl[0], nb = s_ctl[1];
                double bk = -INFINITY;
                int bi = INT_MAX;
                if (nb < A.beam) {
                    for (int i = lane; i < nA; i += 64)
                        if ((Aflag[i] & 1) && (Akey[i] > bk || bi == INT_MAX)) { bk = Akey[i]; bi = i; }
#pragma unroll
                    for (int m = 1; m < 64; m <<= 1) beam_argmax_step(bk, bi, m);
                }
                if (lane == 0) {
                    int stop = 0;
                    if (nb >= A.beam) stop = 1;
                    else if (bi == INT_MAX) { s_ctl[4] = 3; stop = 2; }          // A ran empty (the reference's max() raises)
                    else if (nb > 0) {
                        int bm = 0;
                        for (int j = 1; j < nb; ++j)
                            if (s_bkey[j] > s_bkey[bm]) bm = j;
                        if (s_blp[bm] >= A.state_beam + Alp[bi]) stop = 1;
                    }
                    if (!stop) {
                        Aflag[bi] &= ~1;
                        s_ctl[2] = bi;
                        s_ctl[8] = Aslot[bi] < 0;
                        if (Aslot[bi] < 0) {                         // first expansion of this node: a slot for its predictor step
                            int p = s_ctl[6];
                            const int ni = s_ctl[5];
                            for (bool used = true; used && p < L.ns;) {
                                used = false;
                                for (int j = 0; j < ni; ++j) used |= Aslot[j] == p;
                                if (used) ++p;
                            }
                            if (p >= L.ns) { s_ctl[4] = 1; stop = 2; }
                            else {
                                Aslot[bi] = p;
                                s_ctl[6] = p + 1;
                                s_ctl[9] = Apar[bi] >= 0 ? Aslot[Apar[bi]] : -1;
                                s_ctl[10] = Atok[bi];
                            }
                        }
                    }
                    s_ctl[3] = stop;
                }
            }
            __syncthreads();
            if (s_ctl[3] != 0) break;
            const int a = s_ctl[2];
            float *sl = slots + (size_t)Aslot[a] * SW;
            if (s_ctl[8]) {                                  // predictor step of node a: pn(token, parent's state), once per node
                const int ps = s_ctl[9], tok = s_ctl[10];
                const float *pst = ps >= 0 ? slots + (size_t)ps * SW : nullptr;
                for (int i = tid; i < 2 * H; i += SEARCH_THREADS) h[i] = pst ? pst[J + i] : 0.f;   // h | c contiguous in LDS and in a slot
                predictor_step<WT, WIDE>(A.net, A.E, H, J, tok, x, h, c, gates, pn);
                for (int i = tid; i < SWP; i += SEARCH_THREADS) sl[i] = i < J ? pn[i] : h[i - J];    // slot = pn | h | c (h, c adjacent in LDS)
                if constexpr (LM)                            // the LM step of the same token from the parent slot's LM state
                    beam_lm_step<WT, WIDE>(A.lm, A.V, tok, pst ? pst + SWP : nullptr, sl + SWP, lx, lh, lgt, llg, s_lmlp, s_stat, red);
            } else {
                for (int k = tid; k < J; k += SEARCH_THREADS) pn[k] = sl[k];
                if constexpr (LM)
                    for (int i = tid; i < (WIDE ? A.V : 64); i += SEARCH_THREADS) s_lmlp[i] = sl[SWP + i];
                __syncthreads();
            }
            for (int k = tid; k < J; k += SEARCH_THREADS) {
                const float v = ld1(enc + (size_t)t * J + k) + pn[k];
                z[k] = v > 0.f ? v : v * A.slope;
            }
            __syncthreads();
            gemv_rows<WT>((const WT *)A.net.w_head, A.V, J, z, A.net.b_head, nullptr, nullptr, 0, nullptr, lg);
            __syncthreads();
            // the appends, in top-k order: run by ONE thread once s_tlp / s_tpos hold the top-k of log_softmax(lg)
            const auto append = [&]() __attribute__((always_inline)) {
                const double alp = Alp[a];
                const int alen = Alen[a];
                const double bnb = s_tpos[0] != A.blank ? s_tlp[0] : s_tlp[1];
                int nA = s_ctl[0], nb = s_ctl[1];
                for (int j = 0; j < A.beam; ++j) {
                    const double sc = alp + s_tlp[j];
                    const int sym = s_tpos[j];
                    if (sym == A.blank) {
                        s_blp[nb] = sc;
                        s_bkey[nb] = sc / (double)alen;
                        s_bidx[nb] = a;
                        ++nb;
                    } else if (s_tlp[j] >= bnb - A.expand_beam) {
                        if (nA >= cap) { s_ctl[4] = 1; s_ctl[11] = 1; break; }
                        double sx = sc;                      // LM: (alp + joint) + weight * lm, a product and a sum (no fused multiply-add)
                        if constexpr (LM) sx = __dadd_rn(sc, __dmul_rn(A.lm.weight, (double)s_lmlp[sym]));
                        if constexpr (BIAS) {                // the trie step of a's state on sym; its bonus comes last
                            int cs = 0;
                            if (gb >= 0) {
                                double d;
                                cs = beam_bias_step(A.bias, gb, bw, Actx[a], sym, d);
                                sx = __dadd_rn(sx, d);
                            }
                            Actx[nA] = cs;
                        }
                        Alp[nA] = sx;
                        Akey[nA] = sx / (double)(alen + 1);
                        Apar[nA] = a;
                        Atok[nA] = sym;
                        Alen[nA] = alen + 1;
                        Aslot[nA] = -1;
                        Anode[nA] = -1;
                        Aflag[nA] = 1;
                        if (TIMES) Afrm[nA] = fbase + t;
                        ++nA;
                    }
                }
                s_ctl[0] = nA;
                s_ctl[1] = nb;
            };
            if constexpr (WIDE) {                            // log_softmax and top-k over the workgroup (V <= SEARCH_THREADS: one entry per thread)
                const float lp = beam_wide_log_softmax(tid < A.V ? lg[tid] : -INFINITY, red);
                bool taken = tid >= A.V;
                for (int r = 0; r < A.beam; ++r) {
                    float k = lp;
                    int i = taken ? INT_MAX : tid;
#pragma unroll
                    for (int m = 1; m < 64; m <<= 1) {
                        const float k2 = __shfl_xor(k, m);
                        const int i2 = __shfl_xor(i, m);
                        beam_topk_pick(k, i, k2, i2);
                    }
                    float *rk = red + 32 + (r & 1) * 16;
                    int *ri = reinterpret_cast<int *>(red + 64) + (r & 1) * 16;
                    if (lane == 0) { rk[wave] = k; ri[wave] = i; }
                    __syncthreads();
                    float bk = rk[0];
                    int bi = ri[0];
#pragma unroll
                    for (int w = 1; w < SEARCH_THREADS / 64; ++w) beam_topk_pick(bk, bi, rk[w], ri[w]);
                    if (tid == bi) {
                        taken = true;
                        s_tlp[r] = (double)lp;
                        s_tpos[r] = tid;
                    }
                }
                __syncthreads();
                if (tid == 0) append();
            } else if (wave == 0) {                          // log_softmax, top-k (equal values: lower index first), the appends: one wave
                __shared__ float s_lp[64];
                const float v = lane < A.V ? lg[lane] : -INFINITY;
                const float m = wave_max(v);
                const float s = wave_sum(lane < A.V ? expf(v - m) : 0.f);
                const float lp = (v - m) - logf(s);
                s_lp[lane] = lp;
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (lane < A.V) {
                    int rank = 0;
                    for (int u = 0; u < A.V; ++u) {
                        const float o = s_lp[u];
                        rank += (o > lp) || (o == lp && u < lane);
                    }
                    if (rank < A.beam) { s_tlp[rank] = (double)lp; s_tpos[rank] = lane; }
                }
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                if (lane == 0) append();
            }
            __syncthreads();
            if (s_ctl[11] != 0) break;
        }
        __syncthreads();
        if (s_ctl[4] != 0) break;
        // End of the frame: promote the new nodes on the beam's paths into the tree, in creation (index) order.
        if (tid == 0) {
            int cnt = 0;
            for (int j = 0; j < s_ctl[1]; ++j)
                for (int e = s_bidx[j]; e >= 0 && Anode[e] < 0 && !(Aflag[e] & 2); e = Apar[e]) { Aflag[e] |= 2; ++cnt; }
            if (s_ctl[7] + cnt > L.nn) s_ctl[12] = 1;
        }
        __syncthreads();
        if (s_ctl[12] != 0) break;
        if (wave == 0) {
            int base = s_ctl[7];
            const int nA = s_ctl[0];
            for (int i0 = 0; i0 < nA; i0 += 64) {
                const int i = i0 + lane;
                const bool mk = i < nA && (Aflag[i] & 2);
                const unsigned long long bal = __ballot(mk);
                if (mk) Anode[i] = base + __popcll(bal & ((1ull << lane) - 1));
                base += __popcll(bal);
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            for (int i = lane; i < nA; i += 64)
                if (Aflag[i] & 2) {
                    tree[Anode[i]] = make_int2(Atok[i], Anode[Apar[i]]);
                    if (TIMES) nfrm[Anode[i]] = Afrm[i];
                    if (biased) nctx[Anode[i]] = Actx[i];
                }
            if (lane == 0) s_ctl[7] = base;
        }
        __syncthreads();
        BeamEnt ne{};
        int nc = 0;
        const int nb = s_ctl[1];
        if (tid < nb) {
            const int e = s_bidx[tid];
            ne = BeamEnt{s_blp[tid], Anode[e], Alen[e], Aslot[e], Atok[e]};
            if (biased) nc = Actx[e];
        }
        __syncthreads();
        if (tid < nb) {
            Alp[tid] = ne.logp;
            Akey[tid] = s_bkey[tid];
            Apar[tid] = -1;
            Atok[tid] = ne.tok;
            Alen[tid] = ne.len;
            Aslot[tid] = ne.slot;
            Anode[tid] = ne.node;
            Aflag[tid] = 1;
            if (biased) Actx[tid] = nc;
        }
        if (tid == 0) s_ctl[5] = nb;
        __syncthreads();
    }
    __syncthreads();
    const int st = s_ctl[4] != 0 ? s_ctl[4] : (s_ctl[12] != 0 ? 2 : 0), nbeam = s_ctl[5];
    if (tid == 0) {
        if (run) {                                           // the state this call leaves (a zero count leaves it untouched)
            hdr[1] = st;
            if (st == 0) {
                hdr[0] = 1;
                hdr[2] = nbeam;
                hdr[3] = s_ctl[7];
                hdr[4] = (fresh ? 0 : hdr[4]) + tend;
            }
        }
        A.status[b] = st;
        // n-best: sorted(beam, key=logp/len, reverse=True)[:nbest], stable -> repeated first-maximum selection
        // bias: ranked and reported with the bonus of a half-matched phrase given back (Alp, the stored beam, keeps it)
        if constexpr (BIAS)
            if (gb >= 0 && st == 0)
                for (int j = 0; j < nbeam; ++j) Akey[j] = __dsub_rn(Alp[j], A.bias.pending[gb + Actx[j]]) / (double)Alen[j];
        for (int r = 0; r < A.nbest; ++r) {
            int best = -1;
            if (st == 0)
                for (int j = 0; j < nbeam; ++j)
                    if (Aflag[j] & 1 && (best < 0 || Akey[j] > Akey[best])) best = j;
            if (best >= 0) Aflag[best] &= ~1;
            s_order[r] = best;
            A.lens[(size_t)b * A.nbest + r] = best >= 0 ? Alen[best] - 1 : -1;
            A.scores[(size_t)b * A.nbest + r] = best >= 0 ? Akey[best] : -INFINITY;
        }
    }
    if (tid < nbeam && st == 0 && run) bent[tid] = BeamEnt{Alp[tid], Anode[tid], Alen[tid], Aslot[tid], Atok[tid]};
    __syncthreads();
    for (int r = wave; r < A.nbest; r += SEARCH_THREADS / 64) {  // one wave's lane 0 walks a hypothesis up the tree
        const int e = s_order[r];
        if (lane == 0 && e >= 0) {
            int node = Anode[e];
            int *out = A.hyps + ((size_t)b * A.nbest + r) * A.Lmax;
            int *fout = TIMES ? A.frames + ((size_t)b * A.nbest + r) * A.Lmax : nullptr;
            for (int d = Alen[e] - 2; d >= 0 && node > 0; --d) {
                const int2 nd = tree[node];
                if (d < A.Lmax) {
                    out[d] = nd.x;
                    if (TIMES) fout[d] = nfrm[node];
                }
                node = nd.y;
            }
        }
    }
}

// RUN(T, WT) with the io and the weight type that the two (checked) dtype codes name
#define SEARCH_DTYPES(io_dtype, wdtype, RUN)                                                        \
    if (io_dtype == TSASR_F32) { if (wdtype == TSASR_F32) RUN(float, float) else RUN(float, bf16_t) } \
    else { if (wdtype == TSASR_F32) RUN(bf16_t, float) else RUN(bf16_t, bf16_t) }

template <typename Args>
void search_launch(void (*kern)(const Args), int B, size_t lds, void *stream, const Args &a) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    kern<<<B, SEARCH_THREADS, lds, (hipStream_t)stream>>>(a);
}

// tsasr_greedy_decode's checks and launch. wide: V <= 1024 and E <= 1024 instead of V <= 63 and E <= 64; streamed: state and n_valid are given.
int greedy_launch(const char *name, bool wide, bool streamed, const void *enc, const NetArgs &net, float *state, const int32_t *n_valid,
                  int *preds, float *logp_sum, int B, int T, int J, int H, int E, int V, int blank, float slope, int io_dtype, int wdtype,
                  void *stream) {
    TSASR_CHECK_ARG(enc && net.emb && net.w_ih && net.w_hh && net.w_proj && net.w_head && preds && logp_sum && (!streamed || (state && n_valid)),
                    "%s: null pointer", name);
    TSASR_CHECK_ARG(B > 0 && T > 0 && J > 0 && J % 4 == 0 && H > 0 && H % 4 == 0 && E > 0 && E <= (wide ? 1024 : 64) && V > 1 &&
                    V <= (wide ? 1024 : 63) && blank >= 0 && blank < V,
                    "%s: bad shape (B=%d T=%d J=%d H=%d E=%d V=%d blank=%d)", name, B, T, J, H, E, V, blank);
    TSASR_CHECK_ARG(J <= 1024 && H <= 1024, "%s: J=%d H=%d above 1024", name, J, H);
    TSASR_CHECK_ARG((io_dtype == TSASR_F32 || io_dtype == TSASR_BF16) && (wdtype == TSASR_F32 || wdtype == TSASR_BF16), "%s: bad dtype", name);
    const size_t lds = (size_t)(2 * H + 2 * J + 4 * H + (wide ? round4(E) + round4(V) + 64 : 64 + 64)) * sizeof(float);
    if (wide) TSASR_CHECK_ARG(lds <= 160 * 1024, "%s: H=%d J=%d E=%d V=%d need %zu B of LDS", name, H, J, E, V, lds);
    else TSASR_CHECK_ARG(lds <= 160 * 1024, "%s: H=%d J=%d need %zu B of LDS", name, H, J, lds);
    const GreedyArgs a{enc, net, preds, logp_sum, B, T, J, H, E, V, blank, slope, state, n_valid};
#define GREEDY(TT, WW)                                                                                                                  \
    search_launch(wide ? (streamed ? greedy_decode_kernel<TT, WW, true, true> : greedy_decode_kernel<TT, WW, false, true>)              \
                       : (streamed ? greedy_decode_kernel<TT, WW, true, false> : greedy_decode_kernel<TT, WW, false, false>),           \
                  B, lds, stream, a);
    SEARCH_DTYPES(io_dtype, wdtype, GREEDY)
#undef GREEDY
    TSASR_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" {

/* Greedy transducer search (speechbrain/decoders/transducer.py:138-218) for a predictor = embedding table -> one-layer LSTM -> Linear and
 * a joiner = LeakyReLU(enc + pn) -> Linear head; include/tsasr_hip.h states the arguments. state and n_valid both NULL: the offline
 * search; both given: one chunk of a stream (pieces give the bits of one offline call). One launch. */
int tsasr_greedy_decode(const void *enc, const float *emb, const void *w_ih, const void *w_hh, const float *b_ih, const float *b_hh,
                        const void *w_proj, const float *b_proj, const void *w_head, const float *b_head, float *state, const int32_t *n_valid,
                        int *preds, float *logp_sum, int B, int T, int J, int H, int E, int V, int blank, float slope, int io_dtype,
                        int wdtype, void *stream, int wide) {
    TSASR_CHECK_ARG(!state == !n_valid, "tsasr_greedy_decode: state and n_valid are given together (a stream chunk) or both NULL");
    return greedy_launch("tsasr_greedy_decode", wide != 0, state != nullptr, enc, {emb, w_ih, w_hh, b_ih, b_hh, w_proj, b_proj, w_head, b_head},
                         state, n_valid, preds, logp_sum, B, T, J, H, E, V, blank, slope, io_dtype, wdtype, stream);
}

/* The beam search's workspace (see the kernel's comment), the host's one statement of its layout: a slot's LM part is beam_lm_slot_floats
 * (lm_layers 0: no LM, lm_hidden is not read), times and bias add one int per tree node each. 0 for a shape no call takes. */
size_t tsasr_beam_search_workspace_bytes(int B, int T, int H, int J, int V, int beam, int cap, int lm_layers, int lm_hidden, int times,
                                         int bias, int wide) {
    if (B <= 0 || T <= 0 || H <= 0 || J <= 0 || V <= 0 || beam <= 0 || cap <= 0 || lm_layers < 0 || (lm_layers > 0 && lm_hidden <= 0)) return 0;
    const int lmw = lm_layers > 0 ? beam_lm_slot_floats(wide != 0, V, lm_layers, lm_hidden) : 0;
    return (size_t)B * beam_per_utt(beam_layout(T, H, J, beam, cap, lmw), times != 0, bias != 0);
}

// Checks an LM descriptor and restates it, with the fusion weight, as the kernel's arguments
static int beam_lm_args(const char *name, const tsasr_lm_desc *lm, double lm_weight, BeamLmArgs &m) {
    const int Ll = lm->layers, Hl = lm->hidden, El = lm->emb_dim, nb = lm->dnn_blocks, D = lm->dnn_neurons;
    TSASR_CHECK_ARG(Ll >= 1 && Ll <= 4 && Hl > 0 && Hl % 4 == 0 && Hl <= 1024 && El > 0 && El % 4 == 0 && El <= 1024 && nb >= 0 && nb <= 2 &&
                    D > 0 && D % 4 == 0 && D <= 1024 && (nb > 0 || D == Hl),
                    "%s: bad LM shape (layers=%d hidden=%d emb_dim=%d dnn_blocks=%d dnn_neurons=%d)", name, Ll, Hl, El, nb, D);
    bool ptrs = lm->emb && lm->w_out;
    for (int l = 0; l < Ll; ++l) ptrs = ptrs && lm->w_ih[l] && lm->w_hh[l];
    for (int k = 0; k < nb; ++k) ptrs = ptrs && lm->w_dnn[k];
    TSASR_CHECK_ARG(ptrs, "%s: null LM pointer", name);
    m.emb = lm->emb;
    for (int l = 0; l < 4; ++l) { m.w_ih[l] = lm->w_ih[l]; m.w_hh[l] = lm->w_hh[l]; m.b_ih[l] = lm->b_ih[l]; m.b_hh[l] = lm->b_hh[l]; }
    for (int k = 0; k < 2; ++k) {
        m.w_dnn[k] = lm->w_dnn[k]; m.b_dnn[k] = lm->b_dnn[k]; m.ln_g[k] = lm->ln_g[k]; m.ln_b[k] = lm->ln_b[k]; m.ln_eps[k] = lm->ln_eps[k];
    }
    m.w_out = lm->w_out; m.b_out = lm->b_out;
    m.L = Ll; m.Hl = Hl; m.E = El; m.nb = nb; m.D = D; m.slope = lm->slope; m.weight = lm_weight;
    return 0;
}

// tsasr_beam_search's checks and launch. wide: V <= 1024, E <= 1024 and the LDS budget of the wide instantiations; frames given: timed.
static int beam_launch(const char *name, bool wide, const void *enc, const NetArgs &net, void *workspace, size_t workspace_bytes,
                       const int32_t *n_valid, int *hyps, int *frames, int *lens, double *scores, int *status, int B, int T, int max_frames,
                       int J, int H, int E, int V, int blank, int beam, int nbest, int cap, int Lmax, double state_beam, double expand_beam,
                       float slope, int io_dtype, int wdtype, void *stream, const tsasr_lm_desc *lm, double lm_weight,
                       const tsasr_bias_desc *bias) {
    const bool times = frames != nullptr;
    TSASR_CHECK_ARG(enc && net.emb && net.w_ih && net.w_hh && net.w_proj && net.w_head && workspace && hyps && lens && scores && status,
                    "%s: null pointer", name);
    TSASR_CHECK_ARG(B > 0 && T > 0 && J > 0 && J % 4 == 0 && H > 0 && H % 4 == 0 && E > 0 && E <= (wide ? 1024 : 64) && V > 1 &&
                    V <= (wide ? SEARCH_THREADS : 63) && blank >= 0 && blank < V,
                    "%s: bad shape (B=%d T=%d J=%d H=%d E=%d V=%d blank=%d)", name, B, T, J, H, E, V, blank);
    TSASR_CHECK_ARG(J <= 1024 && H <= 1024, "%s: J=%d H=%d above 1024", name, J, H);
    TSASR_CHECK_ARG(beam >= 2 && beam <= V && beam <= BEAM_MAXK && nbest >= 1 && nbest <= BEAM_MAXK && cap >= beam && Lmax >= 1 && max_frames >= 1,
                    "%s: bad search settings (beam=%d V=%d nbest=%d cap=%d Lmax=%d max_frames=%d)", name, beam, V, nbest, cap, Lmax, max_frames);
    TSASR_CHECK_ARG((io_dtype == TSASR_F32 || io_dtype == TSASR_BF16) && (wdtype == TSASR_F32 || wdtype == TSASR_BF16), "%s: bad dtype", name);
    const int Ep = wide ? round4(E) : 64, Vp = wide ? round4(V) : 64;
    BeamLmArgs m{};
    size_t lm_lds = 0;
    if (lm) {
        if (const int err = beam_lm_args(name, lm, lm_weight, m)) return err;
        lm_lds = (size_t)(std::max(std::max(m.E, m.Hl), m.D) + 2 * m.Hl + std::max(4 * m.Hl, m.D) + 2 * Vp + 2) * sizeof(float);
    }
    BeamBiasArgs g{};
    if (bias) {
        TSASR_CHECK_ARG(bias->child_off && bias->child_tok && bias->child_to && bias->pending && bias->base && bias->weight,
                        "%s: null bias pointer", name);
        TSASR_CHECK_ARG(bias->rows >= 1 && bias->edges >= 0, "%s: bad bias sizes (rows=%d edges=%d)", name, bias->rows, bias->edges);
        g = BeamBiasArgs{bias->child_off, bias->child_tok, bias->child_to, bias->pending, bias->base, bias->weight, bias->rows};
    }
    const size_t need = tsasr_beam_search_workspace_bytes(B, max_frames, H, J, V, beam, cap, lm ? lm->layers : 0, lm ? lm->hidden : 0, times,
                                                          bias != nullptr, wide);
    TSASR_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu B, need %zu", name, workspace_bytes, need);
    // dynamic LDS (the kernel's comment); wide: + 4 KB for its static arrays (the beam's and the top-k's, 2.4 KB) within the CU's 160 KB
    const size_t lds = (size_t)(6 * H + 2 * J + Ep + Vp + (wide ? 96 : 0)) * sizeof(float) +
                       (size_t)cap * (2 * sizeof(double) + ((times ? 7 : 6) + (bias ? 1 : 0)) * sizeof(int)) + lm_lds;
    if (wide) TSASR_CHECK_ARG(lds + 4096 <= 160 * 1024, "%s: H=%d J=%d E=%d V=%d cap=%d need %zu B of LDS", name, H, J, E, V, cap, lds);
    else TSASR_CHECK_ARG(lds <= 152 * 1024, "%s: H=%d J=%d cap=%d need %zu B of LDS", name, H, J, cap, lds);
    const BeamArgs a{enc, net, (unsigned char *)workspace, n_valid, hyps, lens, scores, status, B, T, J, H, E, V, blank, beam, nbest, cap,
                     Lmax, max_frames, state_beam, expand_beam, slope, frames};
#define BEAM_KERN(TT, WW, LM, BS) (wide ? (times ? beam_search_kernel<TT, WW, true, LM, true, BS> : beam_search_kernel<TT, WW, false, LM, true, BS>) \
                                        : (times ? beam_search_kernel<TT, WW, true, LM, false, BS> : beam_search_kernel<TT, WW, false, LM, false, BS>))
#define BEAM(TT, WW)                                                                                                      \
    {                                                                                                                     \
        if (lm && bias) search_launch(BEAM_KERN(TT, WW, true, true), B, lds, stream, BeamKernArgs<true, true>{a, m, g});  \
        else if (bias) search_launch(BEAM_KERN(TT, WW, false, true), B, lds, stream, BeamKernArgs<false, true>{a, g});    \
        else if (lm) search_launch(BEAM_KERN(TT, WW, true, false), B, lds, stream, BeamKernArgs<true, false>{a, m});      \
        else search_launch(BEAM_KERN(TT, WW, false, false), B, lds, stream, BeamKernArgs<false, false>{a});               \
    }
    SEARCH_DTYPES(io_dtype, wdtype, BEAM)
#undef BEAM
#undef BEAM_KERN
    TSASR_CHECK_LAUNCH(name);
    return 0;
}

/* Beam transducer search (speechbrain/decoders/transducer.py:220-373) for the networks tsasr_greedy_decode takes; see the kernel's comment
 * and include/tsasr_hip.h. n_valid NULL: the offline search over every frame of enc [B,T,J], padding included, as the reference (the
 * workspace is started afresh and left holding the final beam: a call with zero counts reads the n-best out again, e.g. with a larger
 * Lmax); given: one chunk of a stream resumed from the workspace (zeroed = start of the stream). frames NULL: untimed; lm NULL: no LM
 * fusion (see BeamLmArgs; lm_weight is then not read); bias NULL: no phrase graphs (see BeamBiasArgs). wide: the WIDE instantiation; a
 * biased call has only ever run the one its shape needs, so with a graph wide must say V > 63 || E > 64. */
int tsasr_beam_search(const void *enc, const float *emb, const void *w_ih, const void *w_hh, const float *b_ih, const float *b_hh,
                      const void *w_proj, const float *b_proj, const void *w_head, const float *b_head, void *workspace, size_t workspace_bytes,
                      const int32_t *n_valid, int *hyps, int *lens, double *scores, int *status, int B, int T, int max_frames, int J, int H,
                      int E, int V, int blank, int beam, int nbest, int cap, int Lmax, double state_beam, double expand_beam, float slope,
                      int io_dtype, int wdtype, void *stream, int *frames, const tsasr_lm_desc *lm, double lm_weight,
                      const tsasr_bias_desc *bias, int wide) {
    TSASR_CHECK_ARG(n_valid || max_frames == T, "tsasr_beam_search: the offline search (n_valid NULL) takes max_frames = T, got %d and T=%d",
                    max_frames, T);
    TSASR_CHECK_ARG(!bias || (wide != 0) == (V > 63 || E > 64), "tsasr_beam_search: bias with wide=%d but V=%d E=%d", wide, V, E);
    return beam_launch("tsasr_beam_search", wide != 0, enc, {emb, w_ih, w_hh, b_ih, b_hh, w_proj, b_proj, w_head, b_head}, workspace,
                       workspace_bytes, n_valid, hyps, frames, lens, scores, status, B, T, max_frames, J, H, E, V, blank, beam, nbest, cap, Lmax,
                       state_beam, expand_beam, slope, io_dtype, wdtype, stream, lm, lm_weight, bias);
}

}  // extern "C"
