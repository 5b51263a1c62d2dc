// Causal features for streams (build extension, no counterpart in the reference): raw log-mel frames of a signal segment and a running
// floor + running mean / deviation normalisation whose result does not depend on how the signal is cut into pushes.
//
// fbank_frames: the offline fbank_kernel (csrc/features.hip) over a segment that carries its own padding: frame i covers
// seg[i*hop, i*hop + 512) - the bits of the offline center=True frame over the same samples, before the floor.
// audio_ring_append / fbank_frames_slots: the same frames for sessions that enter and leave a running batch (slots), each with its own
// sample count and frame position: the samples wait in a ring per slot, the frame kernel (csrc/features.hip) reads them from there.
// running_norm: per stream a state of fp64 column sums S1, S2 [n_mels], the frame count n (a prior's pseudo-frames included), the running
// maximum and a flag that it exists. For frame k: rmax = max(rmax, max_m db[k][m]); x = max(db, rmax - top_db) (fp32, as
// fbank_floor_kernel subtracts); S1 += x, S2 += x*x, n += 1 in fp64 IN FRAME ORDER; y = (x - S1/n) / max(sqrt(max(0, (S2 - S1*S1/n) / (n-1))), eps)
// (n < 2: deviation 1) in fp64, rounded once to fp32. One workgroup per stream, one thread per bin: every bin's chain of additions is the
// same whatever the split, which a tree over frames would not give. The only cross-bin quantity, the frame maximum, is exact under any
// association: a tile's frame maxima are taken by all threads first, then every bin thread folds them into its own copy of the running one.
#include "common.h"

void tsasr_fbank_launch_frames(const float *seg, const float *window, const float *melmat, float *out_db, int *band, int B, int Lseg, int F,
                               int n_mels, int hop, float amin, hipStream_t st);   // csrc/features.hip

void tsasr_fbank_launch_frames_slots(const float *ring, const int *tbl, const float *window, const float *melmat, float *out_db, int *band, int B,
                                     int cap, int F, int n_mels, int hop, float amin, hipStream_t st);   // csrc/features.hip

// Slots (sessions that enter and leave a running batch, each fed its own audio): a sample ring [B, cap] fp32 on the device. Slot b holds
// sample s of its session at ring[b][s % cap]; the host keeps the counts. audio_ring_append writes the lens[b] samples of row b of
// this push behind the slot's have[b] samples (tbl [2][B] int32: have[b] % cap, lens[b]); one launch for the batch, thread i of a row
// stores sample i: a wave's 64 stores are contiguous except at the one wrap point. A row with lens[b] == 0 is not touched.
// The ring must still hold every sample a later frame reads. Frame k reads samples [k*hop - 256, k*hop + 256). With e frames emitted and
// g frames per group, a drained live session has fewer than g available frames left: (have - 256)/hop + 1 - e <= g - 1, so
// have < (e + g - 1)*hop + 256, and the oldest sample still needed is e*hop - 256: fewer than (g - 1)*hop + 512 samples are needed.
// A push adds at most max_audio_samples, so cap = max_audio_samples + (g - 1)*hop + 512 never overwrites a needed sample (the host
// checks have + lens - max(e*hop - 256, 0) <= cap before every append: a call that a stopped beam stream cut short leaves more).
#define RA_NT 256
__global__ __launch_bounds__(RA_NT) void audio_ring_append_kernel(float *__restrict__ ring, const float *__restrict__ wav, const int *__restrict__ tbl,
                                                                  int B, int N, long long wav_stride, int cap) {
    const int b = blockIdx.y;
    const int n = min(min(tbl[B + b], N), cap);
    const int i = blockIdx.x * RA_NT + threadIdx.x;
    if (i >= n) return;
    const int pos = (int)((unsigned)tbl[b] % (unsigned)cap);
    const int r = pos + i;   // i < cap
    ring[(long long)b * cap + (r >= cap ? r - cap : r)] = wav[(long long)b * wav_stride + i];
}

#define RN_NT 128     // threads = bins (n_mels <= 128: 80 bins use both waves)
#define RN_TILE 128   // frames whose maxima are taken at once

// state of stream b: double S1[n_mels], S2[n_mels], n; float rmax; int32 seen (0: no maximum yet) - all zero = a fresh stream
__host__ __device__ static inline size_t rn_state_doubles(int n_mels) { return (size_t)2 * n_mels + 2; }

template <typename TO>
__global__ __launch_bounds__(RN_NT) void running_norm_kernel(const float *__restrict__ db, const int32_t *__restrict__ n_valid, double *__restrict__ state,
                                                             TO *__restrict__ y, int F, int n_mels, float top_db, double eps) {
#pragma clang fp contract(off)   // one rounding per operation in every copy of the loop body: the bits must not depend on where a push starts
    __shared__ float fmx[RN_TILE];
    const int b = blockIdx.x, m = threadIdx.x;
    const int nv = min(max(n_valid[b], 0), F);
    double *sb = state + (size_t)b * rn_state_doubles(n_mels);
    const float *xb = db + (size_t)b * F * n_mels;
    TO *yb = y + (size_t)b * F * n_mels;
    const bool bin = m < n_mels;
    double s1 = bin ? sb[m] : 0.0, s2 = bin ? sb[n_mels + m] : 0.0, n = sb[2 * n_mels];
    const float *tail = reinterpret_cast<const float *>(sb + 2 * n_mels + 1);
    float rmax = reinterpret_cast<const int *>(tail)[1] ? tail[0] : -INFINITY;
    for (int f0 = 0; f0 < F; f0 += RN_TILE) {
        const int nf = min(RN_TILE, F - f0);
        if (m < nf) {   // thread m: the maximum of frame f0 + m (-inf past the stream's end: such frames leave the state alone)
            float mx = -INFINITY;
            if (f0 + m < nv) {
                const float *row = xb + (size_t)(f0 + m) * n_mels;
                for (int j = 0; j < n_mels; ++j) mx = fmaxf(mx, row[j]);
            }
            fmx[m] = mx;
        }
        __syncthreads();
        if (bin) {
            for (int i = 0; i < nf; ++i) {
                const int k = f0 + i;
                rmax = fmaxf(rmax, fmx[i]);
                const float x = fmaxf(xb[(size_t)k * n_mels + m], rmax - top_db);
                const double xd = (double)x;
                if (k < nv) { s1 += xd; s2 += xd * xd; n += 1.0; }
                const double mean = n > 0.0 ? s1 / n : 0.0;
                double sd = 1.0;
                if (n >= 2.0) sd = fmax(sqrt(fmax(0.0, (s2 - s1 * s1 / n) / (n - 1.0))), eps);
                st1(yb + (size_t)k * n_mels + m, (float)((xd - mean) / sd));
            }
        }
        __syncthreads();
    }
    if (nv > 0) {   // (every thread read the tail before the first barrier)
        if (bin) { sb[m] = s1; sb[n_mels + m] = s2; }
        if (m == 0) {
            sb[2 * n_mels] = n;
            float *t = reinterpret_cast<float *>(sb + 2 * n_mels + 1);
            t[0] = rmax;
            reinterpret_cast<int *>(t)[1] = 1;
        }
    }
}

extern "C" {

size_t tsasr_fbank_frames_workspace_bytes(int n_mels) { return align_up((size_t)2 * n_mels * sizeof(int), 256); }

/* seg [B,Lseg] fp32 (a slice of the padded signal) -> out_db [B, F = (Lseg - 512)/hop + 1, n_mels] fp32: raw dB of the frames
 * seg[i*hop, i*hop + 512), the bits tsasr_fbank_fwd computes for the same samples before its floor. */
int tsasr_fbank_frames(const float *seg, const float *window, const float *melmat, float *out_db, int B, int Lseg, int F, int n_mels, int hop,
                       float amin, void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(seg && window && melmat && out_db && workspace, "tsasr_fbank_frames: null pointer");
    TSASR_CHECK_ARG(B > 0 && hop > 0 && Lseg >= 512 && F == (Lseg - 512) / hop + 1 && n_mels > 0 && n_mels <= 128,
                    "tsasr_fbank_frames: bad shape (Lseg=%d hop=%d F=%d n_mels=%d)", Lseg, hop, F, n_mels);
    TSASR_CHECK_ARG(workspace_bytes >= tsasr_fbank_frames_workspace_bytes(n_mels), "tsasr_fbank_frames: workspace too small");
    tsasr_fbank_launch_frames(seg, window, melmat, out_db, (int *)workspace, B, Lseg, F, n_mels, hop, amin, (hipStream_t)stream);
    TSASR_CHECK_LAUNCH("tsasr_fbank_frames");
    return 0;
}

/* ring [B,cap] fp32, wav [B,N] fp32 with row stride wav_stride >= 0 (elements), tbl [2][B] int32 on the device = {have[b] % cap, lens[b]}:
 * ring[b][(have[b] + i) % cap] = wav[b][i] for i < lens[b] (clamped to N). N <= cap. */
int tsasr_audio_ring_append(float *ring, const float *wav, const int32_t *tbl, int B, int N, long long wav_stride, int cap, void *stream) {
    TSASR_CHECK_ARG(ring && wav && tbl, "tsasr_audio_ring_append: null pointer");
    TSASR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && cap >= 512 && N <= cap && wav_stride >= 0, "tsasr_audio_ring_append: bad shape (B=%d N=%d cap=%d stride=%lld)", B, N, cap,
                    wav_stride);
    audio_ring_append_kernel<<<dim3(cdiv(N, RA_NT), B), RA_NT, 0, (hipStream_t)stream>>>(ring, wav, tbl, B, N, wav_stride, cap);
    TSASR_CHECK_LAUNCH("tsasr_audio_ring_append");
    return 0;
}

/* ring [B,cap] fp32 (tsasr_audio_ring_append), tbl [3][B] int32 on the device = {first[b], count[b], total[b]} -> out_db [B,F,n_mels] fp32:
 * row i < count[b] of slot b = raw dB of frame first[b] + i of the session's signal padded with 256 zeros on the left and with zeros from
 * sample total[b] on (the frame arithmetic of tsasr_fbank_fwd / tsasr_fbank_frames, bit for bit); rows count[b] .. F-1 are zeros. The
 * caller guarantees that the ring still holds samples (first[b]*hop - 256) .. min(total[b], (first[b] + count[b] - 1)*hop + 256) - 1. */
int tsasr_fbank_frames_slots(const float *ring, const int32_t *tbl, const float *window, const float *melmat, float *out_db, int B, int cap, int F,
                             int n_mels, int hop, float amin, void *workspace, size_t workspace_bytes, void *stream) {
    TSASR_CHECK_ARG(ring && tbl && window && melmat && out_db && workspace, "tsasr_fbank_frames_slots: null pointer");
    TSASR_CHECK_ARG(B > 0 && B <= 65535 && hop > 0 && cap >= 512 && F > 0 && n_mels > 0 && n_mels <= 128,
                    "tsasr_fbank_frames_slots: bad shape (B=%d cap=%d F=%d n_mels=%d hop=%d)", B, cap, F, n_mels, hop);
    TSASR_CHECK_ARG(workspace_bytes >= tsasr_fbank_frames_workspace_bytes(n_mels), "tsasr_fbank_frames_slots: workspace too small");
    tsasr_fbank_launch_frames_slots(ring, tbl, window, melmat, out_db, (int *)workspace, B, cap, F, n_mels, hop, amin, (hipStream_t)stream);
    TSASR_CHECK_LAUNCH("tsasr_fbank_frames_slots");
    return 0;
}

size_t tsasr_running_norm_state_bytes(int B, int n_mels) { return (size_t)B * rn_state_doubles(n_mels) * sizeof(double); }

/* db [B,F,n_mels] fp32 raw dB -> y [B,F,n_mels] (out_dtype): causal floor and running normalisation (see the head of this file). The state
 * ([B, 2*n_mels + 2] doubles, zero = fresh) advances by the first n_valid[b] frames of stream b; later frames are normalised with it frozen. */
int tsasr_running_norm_fwd(const float *db, const int32_t *n_valid, void *state, void *y, int B, int F, int n_mels, float top_db, double eps,
                           int out_dtype, void *stream) {
    TSASR_CHECK_ARG(db && n_valid && state && y, "tsasr_running_norm_fwd: null pointer");
    TSASR_CHECK_ARG(B > 0 && F > 0 && n_mels > 0 && n_mels <= RN_NT, "tsasr_running_norm_fwd: bad shape (B=%d F=%d n_mels=%d, at most %d bins)", B, F, n_mels, RN_NT);
    hipStream_t st = (hipStream_t)stream;
    if (out_dtype == TSASR_F32) running_norm_kernel<float><<<B, RN_NT, 0, st>>>(db, n_valid, (double *)state, (float *)y, F, n_mels, top_db, eps);
    else if (out_dtype == TSASR_BF16) running_norm_kernel<bf16_t><<<B, RN_NT, 0, st>>>(db, n_valid, (double *)state, (bf16_t *)y, F, n_mels, top_db, eps);
    else TSASR_CHECK_ARG(false, "tsasr_running_norm_fwd: bad out_dtype %d", out_dtype);
    TSASR_CHECK_LAUNCH("tsasr_running_norm_fwd");
    return 0;
}

}  // extern "C"
