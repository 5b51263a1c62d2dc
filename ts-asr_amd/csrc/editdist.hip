// Batched edit distance with the path choice of the reference's WER statistics (SB/utils/edit_distance.py:124-334, which copies Kaldi's
// compute-wer): per pair the operation table, the walk back from (n, m), the four counts and the alignment in forward order.
//
// One workgroup per pair, no communication between workgroups. Thread t owns the strip of W hypothesis columns [tW + 1, tW + W] and
// keeps the previous row's costs of its strip in registers; it works on reference row i at step s = i - 1 + t, so that the cost to
// its left (row i, column tW) was produced by thread t - 1 one step earlier. That one value per thread and step crosses through a
// double-buffered LDS array, one barrier per step that waits for LDS traffic only (the reference's symbols are staged in LDS up
// front, so no global load sits in the loop; a one-wave workgroup serves short hypotheses). n + ceil(m / W) - 1 steps in all. The
// operation of a cell follows from its three neighbouring costs with the reference's comparison order and goes into the table as
// 2 bits; a pair whose table fits the LDS tile never touches the workspace. The walk back is one thread reading the table from LDS
// (tables in the workspace are staged there a block of rows at a time); it writes the alignment from the end of the pair's slot
// backwards, and the workgroup then moves it to the front.
#include "common.h"

namespace {

constexpr int ED_TILE = 60 * 1024;      // bytes of LDS for the operation table (whole, or the staged rows of the walk back)
constexpr int ED_MAX_THREADS = 256;
constexpr int ED_MAX_REF = 16384;       // reference symbols staged in (dynamic) LDS: 64 KiB beside the 62 KiB of static LDS
enum { OP_EQ = 0, OP_SUB = 1, OP_DEL = 2, OP_INS = 3 };

struct EdArgs {
    const int32_t *ref_sym, *ref_off, *hyp_sym, *hyp_off, *ref_count;
    int32_t *counts;
    uint8_t *align_op;
    int32_t *align_i, *align_j, *align_len;
    unsigned long long *totals;
    unsigned char *ws;
    unsigned long long ws_bytes;
    int N, max_ref;
};

// columns per thread for a hypothesis of m symbols in a workgroup of T threads (0: too long), and the table's bytes per row
__host__ __device__ inline int ed_strip(int m, int T) { return m <= 4 * T ? 4 : m <= 8 * T ? 8 : m <= 16 * T ? 16 : m <= 64 * T ? 64 : 0; }
__host__ __device__ inline long long ed_table_bytes(int n, int m, int T) {
    const int W = ed_strip(m, T);
    if (n <= 0 || m <= 0 || W == 0) return 0;
    const long long stride = (long long)((m + W - 1) / W) * (W / 4);
    return (n * stride + 15) / 16 * 16;
}

// (inlined once with the LDS tile and once with the workspace as `tab`, so that the table stores are LDS or global instructions, not flat ones)
template <int W>
__device__ __forceinline__ void ed_sweep(const int *a_lds, const int32_t *b, int n, int m, unsigned char *tab, int stride, int *hand) {
    const int t = threadIdx.x, T = blockDim.x;
    const int Ta = (m + W - 1) / W;
    int hb[W], prev[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int c = t * W + k;
        hb[k] = c < m ? b[c] : -1;      // columns past m: computed, stored inside the row's padding, never read
        prev[k] = c + 1;                // row 0: insertions
    }
    int dl = t * W;                     // cost at (i - 1, tW): the diagonal neighbour of the strip's first cell
    const int steps = n + Ta - 1;
    int a_next = t == 0 ? a_lds[0] : 0;
    for (int s = 0; s < steps; ++s) {
        const int i = s - t + 1;
        const bool on = t < Ta && i >= 1 && i <= n;
        const int ai = a_next;
        a_next = (t < Ta && i >= 0 && i < n) ? a_lds[i] : 0;      // next step's reference symbol: an LDS read that lands behind this step's cells
        if (on) {
            int left = t == 0 ? i : hand[((s - 1) & 1) * T + t - 1];
            int diag = dl;
            dl = left;
            unsigned bits[(W + 15) / 16] = {};
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int up = prev[k];
                const int ne = ai != hb[k];
                const int sc = diag + ne, dc = up + 1, ic = left + 1;
                const bool take_s = sc < ic && sc < dc;       // substitution / match only if strictly cheaper than both
                const bool take_d = !take_s && dc < ic;       // then the deletion if strictly cheaper than the insertion
                const int v = take_s ? sc : take_d ? dc : ic;
                const unsigned op = take_s ? (unsigned)ne : take_d ? OP_DEL : OP_INS;
                bits[k / 16] |= op << (2 * (k % 16));
                diag = up;
                prev[k] = v;
                left = v;
            }
            unsigned char *p = tab + (long long)(i - 1) * stride + t * (W / 4);
            if (W == 4) *p = (unsigned char)bits[0];
            else if (W == 8) *reinterpret_cast<unsigned short *>(p) = (unsigned short)bits[0];
            else {
#pragma unroll
                for (int q = 0; q < (W + 15) / 16; ++q) reinterpret_cast<unsigned *>(p)[q] = bits[q];
            }
            hand[(s & 1) * T + t] = left;
        }
        // only LDS traffic has to be visible across this barrier (the hand-off; a table in the workspace is read after the sweep, behind
        // a full __syncthreads): a __syncthreads here would wait for the step's global store, a memory round trip per step
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    }
    __syncthreads();
}

__device__ __forceinline__ void ed_sweep_w(int W, const int *a_lds, const int32_t *b, int n, int m, unsigned char *tab, int stride, int *hand) {
    switch (W) {
    case 4: ed_sweep<4>(a_lds, b, n, m, tab, stride, hand); break;
    case 8: ed_sweep<8>(a_lds, b, n, m, tab, stride, hand); break;
    case 16: ed_sweep<16>(a_lds, b, n, m, tab, stride, hand); break;
    default: ed_sweep<64>(a_lds, b, n, m, tab, stride, hand); break;
    }
}

__global__ void __launch_bounds__(ED_MAX_THREADS) edit_distance_kernel(EdArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[ED_TILE];
    __shared__ int hand[2 * ED_MAX_THREADS];
    __shared__ unsigned long long base_sh;
    __shared__ int walk_ij[2], first_sh;
    extern __shared__ int ref_lds[];      // max_ref ints (dynamic)
    const int k = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    const int r0 = A.ref_off[k], h0 = A.hyp_off[k];
    const int n = A.ref_off[k + 1] - r0, m = A.hyp_off[k + 1] - h0;
    const long long slot = (long long)r0 + h0;
    const int W = (n >= 0 && n <= A.max_ref && m >= 0) ? ed_strip(m, T) : 0;

    // where this pair's table starts in the workspace: the sum of the tables before it
    if (t == 0) base_sh = 0;
    __syncthreads();
    {
        unsigned long long part = 0;
        for (int q = t; q < k; q += T)
            part += (unsigned long long)ed_table_bytes(A.ref_off[q + 1] - A.ref_off[q], A.hyp_off[q + 1] - A.hyp_off[q], T);
        if (part) atomicAdd(&base_sh, part);
    }
    __syncthreads();
    const unsigned long long base = base_sh;
    const long long bytes = ed_table_bytes(n, m, T);
    const int stride = (n > 0 && m > 0 && W) ? ((m + W - 1) / W) * (W / 4) : 0;
    const bool resident = bytes <= ED_TILE;
    if (W == 0 || (!resident && base + (unsigned long long)bytes > A.ws_bytes)) {      // refused by the host entry; never reached through it
        if (t < 4) A.counts[4 * k + t] = -1;
        if (t == 0) A.align_len[k] = 0;
        return;
    }
    const int32_t *a = A.ref_sym + r0, *b = A.hyp_sym + h0;
    const unsigned char *tab = A.ws + base;      // (read by the walk back only when the table is not resident)
    if (n > 0 && m > 0) {
        for (int q = t; q < n; q += T) ref_lds[q] = a[q];      // the reference's symbols: read once per row, by a different thread each step
        __syncthreads();
        if (resident) ed_sweep_w(W, ref_lds, b, n, m, tile, stride, hand);
        else ed_sweep_w(W, ref_lds, b, n, m, A.ws + base, stride, hand);
    }

    // ---- the walk back: thread 0, over table rows held in LDS ---------------------------------
    uint8_t *aop = A.align_op + slot;
    int32_t *ai_ = A.align_i + slot, *aj_ = A.align_j + slot;
    const int rows_fit = stride ? (ED_TILE - 32) / stride : 0;
    int p = n + m - 1, n_ins = 0, n_del = 0, n_sub = 0;      // thread 0's
    if (t == 0) { walk_ij[0] = n; walk_ij[1] = m; }
    __syncthreads();
    for (;;) {
        const int i0 = walk_ij[0], j0 = walk_ij[1];
        if (i0 == 0 || j0 == 0) break;
        int lo = 0;
        long long a0 = 0;
        if (!resident) {
            lo = max(0, i0 - rows_fit);
            a0 = ((long long)lo * stride) & ~15ll;
            const long long end = ((long long)i0 * stride + 15) & ~15ll;      // inside the table's own 16-byte padding
            const uint4 *src = reinterpret_cast<const uint4 *>(tab + a0);
            uint4 *dst = reinterpret_cast<uint4 *>(tile);
            for (int q = t; q < (int)((end - a0) / 16); q += T) dst[q] = src[q];
        }
        __syncthreads();
        if (t == 0) {
            int i = i0, j = j0;
            while (i > lo && j > 0) {
                const unsigned byte = tile[(long long)(i - 1) * stride + ((j - 1) >> 2) - a0];
                const unsigned op = (byte >> (((j - 1) & 3) * 2)) & 3u;
                if (op == OP_INS) { --j; aop[p] = 'I'; ai_[p] = -1; aj_[p] = j; ++n_ins; }
                else if (op == OP_DEL) { --i; aop[p] = 'D'; ai_[p] = i; aj_[p] = -1; ++n_del; }
                else { --i; --j; aop[p] = op == OP_SUB ? 'S' : '='; ai_[p] = i; aj_[p] = j; n_sub += op == OP_SUB; }
                --p;
            }
            walk_ij[0] = i;
            walk_ij[1] = j;
        }
        __syncthreads();
    }
    if (t == 0) {
        int i = walk_ij[0], j = walk_ij[1];
        for (; j > 0 && i == 0; --p) { --j; aop[p] = 'I'; ai_[p] = -1; aj_[p] = j; ++n_ins; }      // row 0: insertions
        for (; i > 0; --p) { --i; aop[p] = 'D'; ai_[p] = i; aj_[p] = -1; ++n_del; }                 // column 0: deletions
        const int edits = n_ins + n_del + n_sub;
        A.counts[4 * k + 0] = edits; A.counts[4 * k + 1] = n_ins; A.counts[4 * k + 2] = n_del; A.counts[4 * k + 3] = n_sub;
        A.align_len[k] = n + m - 1 - p;
        first_sh = p + 1;        // the alignment now lies in [p + 1, n + m)
        if (edits) atomicAdd(A.totals + 0, (unsigned long long)edits);
        if (n_ins) atomicAdd(A.totals + 1, (unsigned long long)n_ins);
        if (n_del) atomicAdd(A.totals + 2, (unsigned long long)n_del);
        if (n_sub) atomicAdd(A.totals + 3, (unsigned long long)n_sub);
        atomicAdd(A.totals + 4, (unsigned long long)(long long)A.ref_count[k]);
        atomicAdd(A.totals + 5, 1ull);
        if (edits) atomicAdd(A.totals + 6, 1ull);
    }
    __syncthreads();
    // ---- forward order: move [shift, n + m) to [0, len), a block of T entries at a time (a block's targets lie below every later source) ----
    const int shift = first_sh, len = n + m - shift;
    if (shift > 0) {
        for (int q0 = 0; q0 < len; q0 += T) {
            const int q = q0 + t;
            uint8_t o = 0;
            int vi = 0, vj = 0;
            if (q < len) { o = aop[q + shift]; vi = ai_[q + shift]; vj = aj_[q + shift]; }
            __syncthreads();
            if (q < len) { aop[q] = o; ai_[q] = vi; aj_[q] = vj; }
            __syncthreads();
        }
    }
}

}  // namespace

extern "C" {

/* Upper bound of the workspace tsasr_edit_distance needs for N pairs with `cells` = sum over pairs of (n + 1) * (m + 1). */
size_t tsasr_edit_distance_workspace_bytes(int N, long long cells) {
    if (N <= 0 || cells <= 0) return 0;
    return (size_t)N * 16 + (size_t)cells / 2 + 16;
}

int tsasr_edit_distance(const int32_t *ref_sym, const int32_t *ref_off, const int32_t *hyp_sym, const int32_t *hyp_off,
                        const int32_t *ref_count, int N, int max_ref, int max_hyp, long long cells, int32_t *counts, uint8_t *align_op,
                        int32_t *align_i, int32_t *align_j, int32_t *align_len, long long *totals, void *workspace,
                        size_t workspace_bytes, void *stream) {
    const char *name = "tsasr_edit_distance";
    TSASR_CHECK_ARG(ref_off && hyp_off && ref_count && counts && align_len && totals, "%s: null pointer", name);
    TSASR_CHECK_ARG(N > 0 && max_ref >= 0 && max_hyp >= 0, "%s: bad sizes (N=%d max_ref=%d max_hyp=%d)", name, N, max_ref, max_hyp);
    TSASR_CHECK_ARG(max_ref == 0 || ref_sym, "%s: null ref_sym", name);
    TSASR_CHECK_ARG(max_hyp == 0 || hyp_sym, "%s: null hyp_sym", name);
    TSASR_CHECK_ARG((max_ref == 0 && max_hyp == 0) || (align_op && align_i && align_j), "%s: null alignment buffer", name);
    TSASR_CHECK_ARG(max_hyp <= 64 * ED_MAX_THREADS, "%s: hypothesis of %d symbols, at most %d", name, max_hyp, 64 * ED_MAX_THREADS);
    TSASR_CHECK_ARG(max_ref <= ED_MAX_REF, "%s: reference of %d symbols, at most %d", name, max_ref, ED_MAX_REF);
    TSASR_CHECK_ARG(cells >= (long long)N, "%s: cells=%lld below N=%d", name, cells, N);
    const size_t need = tsasr_edit_distance_workspace_bytes(N, cells);
    TSASR_CHECK_ARG(workspace && workspace_bytes >= need, "%s: workspace of %zu B, need %zu", name, workspace_bytes, need);
    TSASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace not 16-byte aligned", name);
    EdArgs a{ref_sym, ref_off, hyp_sym, hyp_off, ref_count, counts, align_op, align_i, align_j, align_len,
             (unsigned long long *)totals, (unsigned char *)workspace, (unsigned long long)workspace_bytes, N, max_ref};
    // short hypotheses (word level, a character-level utterance): one wave per pair; longer ones 256 threads
    const int threads = max_hyp <= 4 * WAVE ? WAVE : ED_MAX_THREADS;
    const size_t lds = (size_t)max_ref * sizeof(int);      // beside the kernel's 62 KiB of static LDS
    if (lds > 0) (void)hipFuncSetAttribute((const void *)edit_distance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    edit_distance_kernel<<<N, threads, lds, (hipStream_t)stream>>>(a);
    TSASR_CHECK_LAUNCH(name);
    return 0;
}

}  // extern "C"
