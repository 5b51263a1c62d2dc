/* libtsasr_hip.so - C-ABI of the MI355X (gfx950) TS-ASR Conformer-Transducer hot path.
 *
 * The reference (lucadellalib/ts-asr) is 100 % Python: it has no FFI for this path. The boundary a
 * maintainer binds is therefore the set of torch.nn.Module / loss callables the hparams YAML
 * instantiates; every entry point below names the reference call it
 * replaces (paths relative to the reference root; SB = vendor/speechbrain/speechbrain).
 * The ctypes stubs a maintainer would add are in INTEGRATION.md; ts-asr_amd/_capi.py holds ours.
 *
 * Conventions
 *   - plain pointers and sizes; every pointer is a DEVICE pointer unless named host_*;
 *   - `stream` is a hipStream_t; nothing allocates, nothing synchronises, nothing touches the
 *     default stream: calls are graph-capturable and re-entrant per stream;
 *   - scratch memory comes from the caller: `*_workspace_bytes()` says how much;
 *   - return value: 0 = ok, <0 = error (TSASR_E_*); tsasr_last_error() gives the message of the
 *     last failure on the calling thread;
 *   - io_dtype: TSASR_F32 (0) or TSASR_BF16 (1) = storage type of activations; contractions use
 *     bf16 MFMA operands with fp32 accumulation, every reduction / softmax / LSE is fp32;
 *   - lengths are ABSOLUTE int32 counts on the device (the host mirror converts the reference's
 *     relative lengths with the reference's own rounding rule before the call).
 */
#ifndef TSASR_HIP_H
#define TSASR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSASR_F32 0
#define TSASR_BF16 1

#define TSASR_E_INVALID (-1)  /* bad shape / unsupported size / null pointer */
#define TSASR_E_LAUNCH (-2)   /* hipLaunch / runtime failure */
#define TSASR_E_WORKSPACE (-3)

const char *tsasr_last_error(void);
int tsasr_version(void);
/* 1 when a gfx950 device is current, 0 otherwise (no kernel is launched). */
int tsasr_device_ok(void);

/* ------------------------------------------------------------------------------------------
 * RNN-T joint + head  (replaces SB/nnet/transducer/transducer_joint.py:73-95 `Transducer_joint.forward`
 * (joint="sum", LeakyReLU) followed by SB/nnet/linear.py:64-78 `Linear.forward` of `transducer_head`,
 * call site train_librispeechmix_scratch.py:132-135) - the [B,T,U1,J] joint tensor is never materialised.
 *   logits[b,t,u,v] = bias[v] + sum_k W[v,k] * lrelu(enc[b,t,k] + dec[b,u,k])      v < V <= 32
 * logits rows are padded to `ldl` floats (ldl % 4 == 0, ldl >= V; columns >= V are written as 0).
 * ------------------------------------------------------------------------------------------ */
int tsasr_joint_fwd(const void *enc, const void *dec, const float *W, const float *bias, float *logits,
                    int B, int T, int U1, int J, int V, int ldl, int io_dtype, float slope, void *stream);

/* The same joint + head in EXACT fp32 arithmetic (csrc/joint_f32.hip: no matrix cores, no bf16 rounding of h, W or dlogits): the
 * `compute_dtype: fp32` parity mode. fp32 storage only; V <= 32, J <= 768; dW / dbias through the deferrable batched reduction. */
int tsasr_joint_f32_fwd(const float *enc, const float *dec, const float *W, const float *bias, float *logits, int B, int T, int U1, int J, int V,
                        int ldl, float slope, void *stream);
size_t tsasr_joint_f32_bwd_workspace_bytes(int B, int U1, int J);
int tsasr_joint_f32_bwd(const float *dlogits, const float *enc, const float *dec, const float *W, float *denc, float *ddec, float *dW,
                        float *dbias, const int32_t *tlen, const int32_t *ulen, int B, int T, int U1, int J, int V, int ldl, float slope,
                        void *workspace, size_t workspace_bytes, void *stream);

size_t tsasr_joint_bwd_workspace_bytes(int B, int T, int U1, int J);
/* Backward of the above: denc[b,t,:], ddec[b,u,:] (io_dtype), dW[V,J], dbias[V] (fp32, OVERWRITTEN; while tsasr_reduce_defer(1)
 * is in force the two are parameter-gradient outputs like the others: written by tsasr_reduce_flush, workspace kept until then).
 * tlen/ulen (may be NULL = full) let the kernel skip the part of the lattice whose dlogits are zero. */
int tsasr_joint_bwd(const float *dlogits, const void *enc, const void *dec, const float *W,
                    void *denc, void *ddec, float *dW, float *dbias,
                    const int32_t *tlen, const int32_t *ulen,
                    int B, int T, int U1, int J, int V, int ldl, int io_dtype, float slope,
                    void *workspace, size_t workspace_bytes, void *stream);

/* The same joint + head for subword vocabularies, 32 < V <= 1024 (csrc/joint_wide.hip): the head matrix is streamed from the fp32 masters
 * in 32-row vocabulary tiles inside the kernels, h and W rounded to bf16 for the matrix cores (backward: dlogits too), sums in fp32.
 * J % 32 == 0, J <= 1024. Forward: ldl % 32 == 0, ldl >= V, columns >= V written as 0 (ldl = V rounded up to 32 is what the host passes).
 * Backward: any ldl % 4 == 0, ldl >= V; outputs, tlen / ulen, deferral of dW / dbias and bitwise reproducibility as the narrow call. The
 * workspace (which depends on V here) holds partial sums of denc / ddec and at most 64 slabs of dW (128 MiB of them at most). io_dtype TSASR_F32 stores fp32
 * activations and still rounds the operands to bf16: there is no exact-fp32 wide joint. */
int tsasr_joint_wide_fwd(const void *enc, const void *dec, const float *W, const float *bias, float *logits,
                         int B, int T, int U1, int J, int V, int ldl, int io_dtype, float slope, void *stream);
size_t tsasr_joint_wide_bwd_workspace_bytes(int B, int T, int U1, int J, int V);
int tsasr_joint_wide_bwd(const float *dlogits, const void *enc, const void *dec, const float *W,
                         void *denc, void *ddec, float *dW, float *dbias,
                         const int32_t *tlen, const int32_t *ulen,
                         int B, int T, int U1, int J, int V, int ldl, int io_dtype, float slope,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * RNN-T loss  (replaces SB/nnet/losses.py:29-87 `transducer_loss` -> torchaudio.functional.rnnt_loss,
 * call site train_librispeechmix_scratch.py:158-160; lattice math as SB/nnet/loss/transducer_loss.py:60-236)
 *   costs[b] = -log P(y_b | x_b)  (no /T), fused log-softmax over the V valid columns of each row.
 * fwd keeps alpha/beta/lse in `workspace` (same pointer must be handed to bwd);
 * bwd writes dlogits[b,t,u,v] = gscale[b] * d costs[b] / d logits  (zeros outside the lattice / v >= V).
 * ------------------------------------------------------------------------------------------ */
long long tsasr_rnnt_loss_error_word_offset(int B, int T, int U1);   /* split lattices (long targets, small batches): byte offset of the time-out word (1 = timed out), -1 = none */
/* Read-only, host-only view of the workspace's plane layout under the current lattice plan (tests read the planes cell by cell). Fills
 * out[0 .. min(n, 17)): plane size in floats, R, U1P, sh, K, KT, NW, NC, skew flag, then the float offsets of lpb, lpe_in, lpe_out, alpha,
 * beta, lse, xch (the split lattice's exchange rows) and logp. Element (b, t, u) of a plane is ((b * R + t + (u >> sh)) * U1P + u)
 * (sh = 31: frame-major planes). Returns 17, or -1 for a shape the loss does not take. */
int tsasr_rnnt_loss_workspace_layout(int B, int T, int U1, long long *out, int n);
size_t tsasr_rnnt_loss_workspace_bytes(int B, int T, int U1);
int tsasr_rnnt_loss_fwd(const float *logits, const int32_t *targets, int ldt, const int32_t *tlen,
                        const int32_t *ulen, float *costs, int B, int T, int U1, int V, int ldl, int blank,
                        void *workspace, size_t workspace_bytes, void *stream);
int tsasr_rnnt_loss_bwd(const float *logits, const int32_t *targets, int ldt, const int32_t *tlen,
                        const int32_t *ulen, const float *gscale /* [B] */, float *dlogits,
                        int B, int T, int U1, int V, int ldl, int blank,
                        const void *workspace, size_t workspace_bytes, void *stream);
/* Lab / test switch, no reference counterpart: how the next tsasr_rnnt_loss_* calls lay out and walk the alpha / beta lattice (-1 = the
 * default of each): skew 0 / 1 / 2 = frame-major planes always / anti-diagonal ("skewed") planes when a lattice runs on more than one
 * wave / always; waves = cap on the waves of a one-workgroup lattice; mc = 0 never split a lattice over workgroups, 1 / 2 / 4 = split
 * whenever the blocks fit on the chip, that many columns per thread. Changes tsasr_rnnt_loss_workspace_bytes; the forward and backward of
 * one loss must run under the same plan. Every plan returns the same bits (tests/test_rnnt_gpu.py). */
void tsasr_rnnt_lattice_plan(int skew, int waves, int mc);

/* ------------------------------------------------------------------------------------------
 * Auxiliary CTC loss on the encoder's frames  (csrc/ctc.hip; replaces SB/nnet/losses.py `ctc_loss` -> torch.nn.functional.ctc_loss with
 * zero_infinity=True on the output of `proj_ctc`, call site SB recipes/LibriSpeech/ASR/transducer/train.py:104-174, and
 * SB/decoders/ctc.py `ctc_greedy_decode`).
 *   logits [B,T,ldl]: the RAW per-frame scores (io_dtype); the row log-softmax over the V valid columns is fused, no log-prob tensor exists.
 *   costs[b] = -log P(y_b | x_b) over the S_b = 2 U_b + 1 extended states, T_b = clamp(tlen[b], 1, T), U_b = clamp(ulen[b], 0, U);
 *   target ids are clamped into [0, V-1] (as the RNN-T loss clamps them), columns of `targets` [B,ldt] at or beyond U_b never reach a result;
 *   an infeasible utterance (T_b < U_b + number of adjacent equal labels) gets costs[b] = 0 and an all-zero gradient (zero_infinity);
 *   dlogits[b,t,v] = gscale[b] * (softmax(x_{b,t})_v - occ_b(t,v)), occ = posterior occupancy of the states that carry v; EVERY row is
 *   written: rows t >= T_b and columns V <= v < ldl are zero.
 * Ranges: 1 <= V <= 1024, ldl >= V and ldl % 8 == 0, T >= 1, 0 <= U <= 2047 (one workgroup of at most 1024 threads owns an utterance's
 * lattice, four consecutive states per thread: S <= 4095), ldt >= U, 0 <= blank < V; anything else is TSASR_E_INVALID before any launch.
 * fwd: row pass (lse + compact emission planes lp(blank), lp(y_u)), the per-vocabulary chains of target positions, then one workgroup per
 * utterance and direction (alpha, beta in fp32 log space, kept in `workspace`; one barrier per frame). bwd: one kernel over all rows; a
 * label that occurs several times has its occupancies summed along its chain in ascending position: no float atomics. Nothing waits for
 * another workgroup, allocates or reads on the host: capturable, re-entrant per stream, identical bits run to run. The workspace size is
 * a function of (B, T, U, V) alone; bwd takes the forward's workspace.
 * tsasr_ctc_greedy: per-frame argmax over the V valid columns (lowest index among equal scores) of frames t < clamp(tlen[b], 0, T),
 * repeats collapsed, blanks dropped, compacted on the device in one launch: tokens[b, :ntok[b]], the rest of the row (ldo >= T) is -1.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_ctc_loss_workspace_bytes(int B, int T, int U, int V);
int tsasr_ctc_loss_fwd(const void *logits /* [B,T,ldl] */, const int32_t *targets /* [B,ldt] */, int ldt, const int32_t *tlen,
                       const int32_t *ulen, float *costs /* [B] */, int B, int T, int U, int V, int ldl, int blank, int io_dtype,
                       void *workspace, size_t workspace_bytes, void *stream);
int tsasr_ctc_loss_bwd(const void *logits, const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen,
                       const float *gscale /* [B] */, void *dlogits /* [B,T,ldl], io dtype */, int B, int T, int U, int V, int ldl, int blank,
                       int io_dtype, const void *workspace /* the forward's */, size_t workspace_bytes, void *stream);
int tsasr_ctc_greedy(const void *logits, const int32_t *tlen, int32_t *tokens /* [B,ldo] */, int ldo, int32_t *ntok /* [B] */,
                     int B, int T, int V, int ldl, int blank, int io_dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * Forced alignment on the same lattice (no reference counterpart): the best path instead of the sum over all paths.
 *   delta(0,0) = 0,  delta(t,u) = max(delta(t-1,u) + lp_blank(t-1,u), delta(t,u-1) + lp_label(t,u-1)),  fp32, lp_* as in the loss;
 *   scores[b] = delta(T_b-1, U_b) + lp_blank(T_b-1, U_b)  = log-probability of the best path  (<= -costs[b]);
 *   frames[b, u] = frame at which label u of that path is emitted (non-decreasing in u) for u < U_b, -1 for U_b <= u < U1-1.
 * Equal candidates (in the kernel's own fp32 arithmetic): the blank predecessor (t-1) wins, i.e. among equal paths the one whose
 * (f_{U-1}, ..., f_0) is lexicographically smallest; identical logits in every cell give frames == 0.
 * logits / targets / ldt / tlen / ulen / ldl / blank as tsasr_rnnt_loss_fwd (T_b = clamp(tlen[b], 1, T), U_b = clamp(ulen[b], 0, U1-1);
 * V <= 32 fast path and general V). frames: [B, ldf] int32, ldf >= max(U1-1, 1). One backpointer bit per cell in `workspace`
 * (plus three fp32 planes); no allocation, no host sync, nothing shared between calls: re-entrant per stream, capturable.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_rnnt_align_workspace_bytes(int B, int T, int U1);
int tsasr_rnnt_align(const float *logits, const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen,
                     int32_t *frames /* [B, ldf] */, int ldf, float *scores /* [B] */,
                     int B, int T, int U1, int V, int ldl, int blank, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fused joint + RNN-T loss for subword vocabularies, 32 < V <= 1024 (csrc/joint_wide.hip): the loss and the forced alignment of
 * tsasr_joint_wide_fwd's logits WITHOUT the [B,T,U1,V] logits / dlogits tensors (3.97 GB each at the benchmark batch and V = 1024).
 *   fwd  : the vocabulary tiles of a lattice cell are folded into its log-sum-exp as they leave the matrix cores (online, in tile order);
 *          lse / lp(blank) / lp(label) go straight into the lattice planes, then the lattice of tsasr_rnnt_loss_fwd runs. costs[b] as there.
 *   bwd  : denc / ddec (io dtype) and dW [V,J] / dbias [V] (fp32) of sum_b gscale[b] * costs[b]. Both backward products recompute their
 *          dlogits operand tile by tile from W, h and three scalars per lattice cell; rounding as tsasr_joint_wide_bwd (dlogits, W, h to
 *          bf16, sums in fp32). dW / dbias are deferred like every parameter gradient while tsasr_reduce_defer(1) is in force.
 *   align: tsasr_rnnt_align's best path (same tie rule, same outputs) on planes filled the same way.
 * Ranges as tsasr_joint_wide_fwd (J % 32 == 0, J <= 1024), U1 <= 2048, targets [B, ldt] with ldt >= max(U1 - 1, 1); tlen / ulen are required
 * and clamped as tsasr_rnnt_loss_fwd clamps them. tsasr_rnnt_lattice_plan governs these calls as it governs tsasr_rnnt_loss_*.
 * Workspace = tsasr_rnnt_loss_workspace_bytes (first, so the split lattice's time-out word keeps its offset) + 3 floats per lattice cell
 * + the denc shares of the cdiv(U1, 32) u tiles + the ddec shares of at most 8 frame ranges + at most 64 slabs of dW [V,J] and dbias
 * (128 MiB of dW slabs at most): a function of the shape alone, nothing in it grows with B*T*U1*V. bwd takes the forward's workspace.
 * No float atomics, no waiting between workgroups in the new kernels: two runs give the same bits. No allocation, no host read: capturable.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_joint_wide_loss_workspace_bytes(int B, int T, int U1, int J, int V);
long long tsasr_joint_wide_loss_error_word_offset(int B, int T, int U1, int J, int V);   /* as tsasr_rnnt_loss_error_word_offset, in this workspace */
int tsasr_joint_wide_loss_fwd(const void *enc, const void *dec, const float *W, const float *bias,
                              const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen, float *costs,
                              int B, int T, int U1, int J, int V, int blank, int io_dtype, float slope,
                              void *workspace, size_t workspace_bytes, void *stream);
int tsasr_joint_wide_loss_bwd(const void *enc, const void *dec, const float *W, const float *bias,
                              const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen, const float *gscale /* [B] */,
                              void *denc, void *ddec, float *dW, float *dbias,
                              int B, int T, int U1, int J, int V, int blank, int io_dtype, float slope,
                              void *workspace /* the forward's */, size_t workspace_bytes, void *stream);
size_t tsasr_joint_wide_align_workspace_bytes(int B, int T, int U1, int J, int V);
int tsasr_joint_wide_align(const void *enc, const void *dec, const float *W, const float *bias,
                           const int32_t *targets, int ldt, const int32_t *tlen, const int32_t *ulen,
                           int32_t *frames /* [B, ldf] */, int ldf, float *scores /* [B] */,
                           int B, int T, int U1, int J, int V, int blank, int io_dtype, float slope,
                           void *workspace, size_t workspace_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Row kernels of the Conformer block (HBM-bound, one pass each, fp32 math, deterministic column reductions).
 * LayerNorm: replaces torch.nn.LayerNorm / SB/nnet/normalization.py:172-223 as used at
 *   SB/lobes/models/transformer/Conformer.py:73,93,194-217 and SB/lobes/models/convolution.py (norm over [F,C]);
 *   act_slope >= 0 fuses the LeakyReLU that follows it (Conformer.py:93-95, convolution.py ConvBlock); < 0 = none.
 * x,y: [M, D] io_dtype; gamma,beta,dgamma,dbeta: fp32 [D]; mean,rstd: fp32 [M] (saved for backward). D % 8 == 0.
 *
 * Row kernels: which kernel serves which width (csrc/elementwise.hip; tests/helpers/rowkern_ref.py expected_path() mirrors every rule
 * and tests/test_rowkern_paths_gpu.py launches every instantiation). A lane moves 16 bytes: 8 bf16 or 4 fp32 elements.
 *   tsasr_layernorm_fwd / _bwd         D (bf16)        D (fp32)       kernel
 *                                      8 .. 256        8 .. 128       layernorm_{fwd,bwd}_kernel<T, 32, 1>   two rows per wave
 *                                      264 .. 512      136 .. 256     <T, 64, 1>   one wave per row
 *                                      520 .. 1024     264 .. 512     <T, 64, 2>
 *                                      1032 .. 2048    520 .. 1024    <T, 64, 4>
 *                                      .. 4096         .. 2048        layernorm_{fwd,bwd}_wide_kernel<T, 2>  one workgroup per row
 *                                      .. 6144         .. 3072        <T, 3>
 *                                      .. 8192         .. 4096        <T, 4>
 *                                      .. 12288        .. 6144        <T, 6>
 *                                      .. 16384        .. 8192        <T, 8>       larger D: rejected
 *   tsasr_layernorm_bwd_add            the one-wave-per-row kernels only: D <= 2048 (bf16) / 1024 (fp32), larger D rejected
 *   tsasr_add_layernorm_fwd / _bwd     bf16: D <= 256 <bf16, 1, half-wave>, <= 512 <1>, <= 1024 <2>, <= 2048 <4>; fp32: D <= 256 <1>, <= 512 <2>,
 *                                      <= 1024 <4>, <= 2048 <8>; larger D rejected
 *   tsasr_add_layernorm2_fwd / _bwd    the same table up to D <= 1024; larger D rejected
 *   bias_act_dropout / dropout_add backward, tsasr_colsum: 256 threads = (256 / tpr) row slots x tpr column chunks, tpr = min(256, N / 8
 *                                      (bf16) or N / 4 (fp32)); the row slots meet in LDS (at most 8 KB); tsasr_colsum: N <= 2048
 * Backward workgroups walk rows_per_wg = max(16, ceil(M / 1024)) consecutive rows (the wide LayerNorm backward: max of that and
 * ceil(M / 512); tsasr_colsum: max(64, ceil(M / 1024))) and leave one partial row of k x D floats each in the workspace (k = 2 LayerNorm,
 * 3 add_layernorm, 5 add_layernorm2, 1 the bias-gradient producers and colsum), summed over workgroups in a fixed order.
 * LDS per launch, static + dynamic: layernorm_bwd_kernel<T, TPR, .> 20 B + (256 / TPR) x 2 x D x 4 B (at most 64 KB + 20 B, bf16 D = 2048);
 * add_layernorm_bwd 48 D B (half-wave: 96 D <= 24 KB), 96 KB at D = 2048; add_layernorm2_bwd 80 D B (half-wave: 160 D <= 40 KB), 80 KB at
 * D = 1024; the forward kernels and the wide kernels 64 B or less. The three launches that pass 64 KB raise their kernel's dynamic-LDS
 * limit first; all stay under the 160 KB of a gfx950 workgroup.
 * ------------------------------------------------------------------------------------------ */
int tsasr_layernorm_fwd(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd,
                        long long M, int D, float eps, float act_slope, int io_dtype, void *stream);
size_t tsasr_layernorm_bwd_workspace_bytes(long long M, int D);
int tsasr_layernorm_bwd(const void *dy, const void *x, const float *gamma, const float *beta, const float *mean,
                        const float *rstd, void *dx, float *dgamma, float *dbeta, long long M, int D, float act_slope,
                        int io_dtype, void *workspace, size_t workspace_bytes, void *stream);
/* ... with dx = LayerNorm_bwd(dy) + dadd: the gradient that reached x along a residual path is summed in the same pass (rows of at
 * most 2048 bf16 / 1024 fp32 elements). */
int tsasr_layernorm_bwd_add(const void *dy, const void *dadd, const void *x, const float *gamma, const float *beta, const float *mean,
                            const float *rstd, void *dx, float *dgamma, float *dbeta, long long M, int D, float act_slope,
                            int io_dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Dropout masks are a pure function of (seed + *seed_dev, element index); seed_dev (device uint64, may be NULL) is advanced once per
 * training step by tsasr_seed_advance so that a captured hipGraph still draws fresh masks every replay. */
int tsasr_seed_advance(unsigned long long *seed_dev, unsigned long long increment, void *stream);

/* y = dropout_p(act(x + bias))  - the Linear-bias + activation() + Dropout chain of PositionalwiseFeedForward
 * (SB/nnet/attention.py:820-836). bias may be NULL; act_slope < 0 = no activation; the dropout mask is a pure function
 * of (seed, element index) and is regenerated by the backward (never stored). dbias may be NULL. N % 8 == 0. */
int tsasr_bias_act_dropout_fwd(const void *x, const float *bias, void *y, long long M, int N, float act_slope, float p,
                               unsigned long long seed, const unsigned long long *seed_dev, int io_dtype, void *stream);
size_t tsasr_colpart_workspace_bytes(long long M, int N);
int tsasr_bias_act_dropout_bwd(const void *dy, const void *y, void *dx, float *dbias, long long M, int N, float act_slope,
                               float p, unsigned long long seed, const unsigned long long *seed_dev, int io_dtype, void *workspace,
                               size_t workspace_bytes, void *stream);

/* out = res + alpha * timemask(dropout_p(x + bias)) - the "Dropout -> 0.5*x + residual" and
 * "Dropout -> masked_fill_(pad) -> + residual" tails of ConformerEncoderLayer / ConvolutionModule
 * (Conformer.py:113-114,239-259). rows = [B, Trows] flattened; valid_lens (int32 [B], may be NULL) zeroes frames
 * t >= valid_lens[b] of the x branch. res may be NULL. Backward gives dx (dres = dout needs no kernel). */
int tsasr_dropout_add_fwd(const void *x, const float *bias, const void *res, void *out, long long M, int N, float alpha,
                          float p, unsigned long long seed, const unsigned long long *seed_dev, const int32_t *valid_lens, int Trows,
                          int io_dtype, void *stream);
int tsasr_dropout_add_bwd(const void *dout, void *dx, float *dbias, long long M, int N, float alpha, float p,
                          unsigned long long seed, const unsigned long long *seed_dev, const int32_t *valid_lens, int Trows, int io_dtype,
                          void *workspace, size_t workspace_bytes, void *stream);
/* out = dropout_p2( res + alpha * timemask(dropout_p(x + bias)) ): the residual tail of a front-end ConvBlock together with the block's
 * outer Dropout (speechbrain/lobes/models/convolution.py:260-266) in one pass. Backward: dres = dropout_p2'(dout) (written; also the
 * gradient of `res`), dx = alpha * timemask * dropout_p'(dres); dres is required when p2 > 0. Both masks are counter-based
 * (seed / seed2 + *seed_dev) and regenerated in the backward. */
int tsasr_dropout_add2_fwd(const void *x, const float *bias, const void *res, void *out, long long M, int N, float alpha, float p,
                           unsigned long long seed, float p2, unsigned long long seed2, const unsigned long long *seed_dev,
                           const int32_t *valid_lens, int Trows, int io_dtype, void *stream);
int tsasr_dropout_add2_bwd(const void *dout, void *dx, void *dres, float *dbias, long long M, int N, float alpha, float p,
                           unsigned long long seed, float p2, unsigned long long seed2, const unsigned long long *seed_dev,
                           const int32_t *valid_lens, int Trows, int io_dtype, void *workspace, size_t workspace_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Conformer convolution-module core: z = LeakyReLU(LayerNorm(depthwise_conv1d_K(GLU(y2 + b2)))) on channels-last rows.
 * Replaces SB/lobes/models/transformer/Conformer.py:101-115 between the two pointwise GEMMs: bottleneck bias + nn.GLU
 * (:76-82), depthwise nn.Conv1d(D,D,K,groups=D) 'same' or causal pad+chomp (:68-71,84-93,108-110), after_conv LayerNorm +
 * activation (:95-97).  y2 [B,T,2D] io_dtype = bottleneck GEMM output without bias; b2 [2D] or NULL; conv_w [D,K] (the
 * [D,1,K] parameter); conv_b, gamma, beta [D]. D % 8 == 0, D <= 2048, K in {31,15,7,3}. c_save [B,T,D], mean/rstd [B*T] are
 * written by fwd and read by bwd. bwd: dparams fp32 = [dgamma D | dbeta D | dconv_b D | db2 2D | dconv_w D*K], overwritten.
 * Pinned by tests/test_convmod_paths_gpu.py: slope < 0 means no activation, in both directions; any T >= 1 (shorter than the
 * filter or its padding included); dparams and the workspace need NO initialisation - every word of dparams is written, db2
 * also when b2 is NULL, and a workspace of exactly tsasr_convmod_bwd_workspace_bytes suffices; bwd leaves z, c_save, mean and
 * rstd as they were; a rejected call (K not instantiated, D % 8 != 0, D > 2048, workspace too small) writes nothing. The
 * io_dtype / D / TSASR_CONVMOD_FUSED dispatch (bf16 rows of 256 channels: one launch per direction) changes no output bit of
 * z, c_save, mean, rstd and dy2.
 * ------------------------------------------------------------------------------------------ */
int tsasr_convmod_fwd(const void *y2, const float *b2, const float *conv_w, const float *conv_b, const float *gamma,
                      const float *beta, void *z, void *c_save, float *mean, float *rstd, int B, int T, int D, int K, int causal,
                      float eps, float slope, int io_dtype, void *stream);
size_t tsasr_convmod_bwd_workspace_bytes(int B, int T, int D, int K);
int tsasr_convmod_bwd(const void *dz, const void *y2, const float *b2, const float *conv_w, const float *gamma, const float *beta,
                      const void *c_save, const float *mean, const float *rstd, void *dy2, float *dparams, int B, int T, int D,
                      int K, int causal, float slope, int io_dtype, void *workspace, size_t workspace_bytes, void *stream);


/* Front-end block 2 as IMPLICIT GEMMs (csrc/gemm.hip conv_s2_*): the 3x3 stride-2 Conv2d + 1x1 stride-2 residual conv of a ConvBlock with
 * C_in > 1 (SB/lobes/models/convolution.py:178-266, SB/nnet/CNN.py:629-711) without the [P, 9*Ci] patch matrix: the ring kernels' loader
 * waves gather the patch rows from x [B,T,F,Ci] (bf16, channels-last) with the padding rule folded into the source address. Wm [128, 9*Ci] =
 * the 3x3 filter as [Co, (kt, kf, ci)], W2 [128, Ci] (bf16); b1 / b2 fp32 [128]; y1, y2 [B,T',F',128] bf16. Co == 128, Ci in {64, 128}.
 * Filter gradients: dWm [128, 9*Ci], dW2 [128, Ci] fp32 (overwritten; split-K slabs in the workspace, summed in fixed order) from dy1, dy2
 * [P,128] and x. Data gradient: dx [B,T,F,Ci] bf16 (every element written) as ONE gathered GEMM launch over classes of input pixels (which
 * taps and output positions reach a pixel depends on its parity and on the reflected border rows) - no [P, 9*Ci] gradient matrix, no inverse
 * gather pass (tsasr_frontend_col2im remains the fp32 / other-shape path). The plan (classes + launch order of their 128-pixel tiles)
 * depends on (B, T, F, causal) only: tsasr_conv3x3s2_dgrad_plan fills a HOST buffer of tsasr_conv3x3s2_dgrad_plan_bytes (0 = unsupported
 * shape), the caller uploads it once and passes the device copy. */
int tsasr_conv3x3s2_fwd(const void *x, const void *Wm, const float *b1, const void *W2, const float *b2, void *y1, void *y2, int B, int T, int F,
                        int Ci, int Co, int causal, void *stream);
size_t tsasr_conv3x3s2_wgrad_workspace_bytes(int B, int T, int F, int Ci);
int tsasr_conv3x3s2_wgrad(const void *dy1, const void *dy2, const void *x, float *dWm, float *dW2, int B, int T, int F, int Ci, int Co, int causal,
                          void *workspace, size_t workspace_bytes, void *stream);
/* the same with the 3x3 gradient in the reference's parameter layout dW1 [128][Ci][kF][kT] (torch Conv2d weight, SB/nnet/CNN.py:629-711): added to
 * the parameter's gradient as it is */
int tsasr_conv3x3s2_wgrad_filters(const void *dy1, const void *dy2, const void *x, float *dW1, float *dW2, int B, int T, int F, int Ci, int Co, int causal,
                                  void *workspace, size_t workspace_bytes, void *stream);
size_t tsasr_conv3x3s2_dgrad_plan_bytes(int B, int T, int F, int causal);
int tsasr_conv3x3s2_dgrad_plan(int B, int T, int F, int causal, void *plan_host, size_t plan_bytes);
int tsasr_conv3x3s2_dgrad(const void *dy1, const void *dy2, const void *Wm, const void *W2, void *dx, int B, int T, int F, int Ci, int Co, int causal,
                          const void *plan_dev, size_t plan_bytes, void *stream);
/* ------------------------------------------------------------------------------------------
 * Convolutional front-end (SB/lobes/models/convolution.py:103-266, Conv2d.forward SB/nnet/CNN.py:629-711): stride-2 3x3
 * conv ('same' = reflect padding, or causal = (2,0) zero pad on time, (1,1) on frequency) + 1x1 stride-2 residual conv.
 * Tensors are the reference's [B,T,F,C]. Block 1 (C_in = 1) is a direct kernel producing both branches; for wider inputs
 * the taps are gathered (im2col, column order (kt,kf,c)) so that the contraction is a plain library GEMM, and col2im is the
 * deterministic inverse gather-sum for the input gradient (dR = gradient of the 1x1 branch w.r.t. its sub-sampled input).
 * ------------------------------------------------------------------------------------------ */
int tsasr_frontend_out_len(int n);
int tsasr_frontend_c1_fwd(const void *x, const float *w1, const float *b1, const float *w2, const float *b2, void *y1, void *y2,
                          int B, int T, int F, int C, int causal, int io_dtype, void *stream);
size_t tsasr_frontend_c1_bwd_workspace_bytes(int C);
int tsasr_frontend_c1_bwd(const void *x, const void *dy1, const void *dy2, float *dparams, int B, int T, int F, int C, int causal,
                          int io_dtype, void *workspace, size_t workspace_bytes, void *stream);
int tsasr_frontend_im2col(const void *x, void *A, int B, int T, int F, int C, int causal, int io_dtype, void *stream);
int tsasr_frontend_col2im(const void *dA, const void *dR, void *dx, int B, int T, int F, int C, int causal, int io_dtype, void *stream);

/* One whole ConvBlock per direction (SB/lobes/models/convolution.py:187-266: convs = Conv2d 3x3 s2 -> LayerNorm([F',C]) -> LeakyReLU ->
 * Dropout; reduce_conv = Conv2d 1x1 s2 -> LayerNorm([F',C]); out = Dropout(convs(x) + reduce_conv(x))):
 *   out = Drop_p_outer( LN_r(r) + Drop_p_inner( LeakyReLU_slope( LN_y(y) ) ) ),   (y, r) = the two convolution outputs.
 * x != NULL (block 1, C_in = 1): (y, r) are computed on the fly from the features x [B,T,F] with filters w1 [C,1,3,3] (kernel axes (F,T)),
 *   b1, w2 [C], b2, and recomputed in the backward: nothing but `out` and 4 floats of statistics per (b, t') reach memory.
 * x == NULL (wider blocks): (y, r) = y1, y2 [B*T', F', C] as produced by the im2col GEMMs; the backward writes their gradients dy1, dy2.
 * T, F are always the block's INPUT sizes (T' = (T-1)/2+1, F' likewise). g1/be1, g2/be2 fp32 [F'*C] = LayerNorm affine of the 3x3 / 1x1
 * branch. stats fp32 [B*T'][4] = (mean_y, rstd_y, mean_r, rstd_r). Dropout masks are f(seed + *seed_dev, element index of out).
 * dparams fp32 (tsasr_frontend_block_dparams floats, overwritten): [dw1 C*9 | db1 C | dw2 C | db2 C] (x != NULL only), then
 * [dg1 | dbe1 | dg2 | dbe2] (F'*C each). Supported: tsasr_frontend_block_supported(F', C) (C = 128, F' <= 40). */
int tsasr_frontend_block_supported(int Fo, int C);
int tsasr_frontend_block_fwd(const void *x, const void *y1, const void *y2, const float *w1, const float *b1, const float *w2,
                             const float *b2, const float *g1, const float *be1, const float *g2, const float *be2, void *out,
                             float *stats, int B, int T, int F, int C, int causal, float slope, float eps, float p_inner,
                             unsigned long long seed_inner, float p_outer, unsigned long long seed_outer,
                             const unsigned long long *seed_dev, int io_dtype, void *stream);
size_t tsasr_frontend_block_dparams(int Fo, int C, int with_conv);
size_t tsasr_frontend_block_bwd_workspace_bytes(int Fo, int C, int with_conv);
int tsasr_frontend_block_bwd(const void *x, const void *y1, const void *y2, const void *dout, const float *w1, const float *b1,
                             const float *w2, const float *b2, const float *g1, const float *be1, const float *g2,
                             const float *stats, void *dy1, void *dy2, float *dparams, int B, int T, int F, int C, int causal,
                             float slope, float p_inner, unsigned long long seed_inner, float p_outer,
                             unsigned long long seed_outer, const unsigned long long *seed_dev, int io_dtype, void *workspace,
                             size_t workspace_bytes, void *stream);


/* ------------------------------------------------------------------------------------------
 * Fused relative-position multi-head self-attention: replaces the body of RelPosMHAXL.forward between in_proj and out_proj,
 * SB/nnet/attention.py:586-633 (q+u/q+v, matrix_ac, matrix_bd + rel_shift :468-483, 1/sqrt(embed_dim) scale, -inf masks,
 * softmax, dropout, .V) without any T x T tensor in HBM.
 *   qkv [B,T,H,3*Dh] (per head Q|K|V, attention.py:549-553), pk [2T-1, H*Dh] = linear_pos(pos_embs),
 *   bias_u/bias_v fp32 [H*Dh] = the (Dh,H) parameters' storage read as [H,Dh] (a view, attention.py:586-592),
 *   key_lens int32 [B] or NULL (keys j >= key_lens[b] are masked), causal != 0 masks j > i.
 *   out [B,T,H*Dh]; lse fp32 [B,H,T] (log-sum-exp of the scaled scores; needed by the backward). Dh <= 64.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_relpos_attn_lds_bytes(void);
int tsasr_relpos_attn_fwd(const void *qkv, const void *pk, const float *bias_u, const float *bias_v, const int32_t *key_lens,
                          void *out, float *lse, int B, int T, int H, int Dh, float scale, int causal, float pdrop,
                          unsigned long long seed, const unsigned long long *seed_dev, int io_dtype, void *stream);
/* Same with a caller-owned workspace: long sequences in small batches (B * H * T/128 < 512 workgroups, T > 1024) are split along the keys
 * across workgroups and merged by a second launch. workspace may be NULL (no split). */
size_t tsasr_relpos_attn_fwd_workspace_bytes(int B, int T, int H);
int tsasr_relpos_attn_fwd_ws(const void *qkv, const void *pk, const float *bias_u, const float *bias_v, const int32_t *key_lens,
                             void *out, float *lse, int B, int T, int H, int Dh, float scale, int causal, float pdrop,
                             unsigned long long seed, const unsigned long long *seed_dev, int io_dtype, void *workspace,
                             size_t workspace_bytes, void *stream);
size_t tsasr_relpos_attn_bwd_workspace_bytes(int B, int T, int H);
/* Backward: dqkv [B,T,H,3*Dh] fully written; d_bias_u/d_bias_v fp32 [H*Dh] ([H,Dh] reading of the parameter storage); dpk [2T-1, H*Dh]
 * (io_dtype, fully written) = gradient of pk = linear_pos(pos_embs). The workspace holds P_d and scale*dS as [B,H,T,ceil64(T)] tensors
 * between the query-major pass (which computes them) and the key-major pass (dK, dV = two contractions over the queries), the
 * q + pos_bias_v rows and the per-utterance-group partial sums of the d(pk) pass. */
int tsasr_relpos_attn_bwd(const void *qkv, const void *pk, const float *bias_u, const float *bias_v, const int32_t *key_lens,
                          const void *out, const void *dout, const float *lse, void *dqkv, void *dpk, float *d_bias_u,
                          float *d_bias_v, int B, int T, int H, int Dh, float scale, int causal, float pdrop,
                          unsigned long long seed, const unsigned long long *seed_dev, int io_dtype, void *workspace, size_t workspace_bytes,
                          void *stream);
/* Deferred d(pk) (csrc/attention.hip): the d(pk) pass of tsasr_relpos_attn_bwd feeds only the weight gradient of linear_pos. While
 * tsasr_relpos_dpk_defer(1) is in force the call QUEUES the pass (workspace, key_lens and dpk of each call stay alive and untouched;
 * dpk is not written yet) and tsasr_relpos_dpk_flush runs all queued passes as one launch + one launch for the sums of their partials
 * (same blocks and order of sums as the per-call launches: bit-identical dpk). table_host: pinned host memory, table_dev: device memory,
 * both >= tsasr_relpos_dpk_table_bytes(tsasr_relpos_dpk_pending()); the tsasr_wgrad_flush protocol under stream capture. */
int tsasr_relpos_dpk_defer(int on);
int tsasr_relpos_dpk_pending(void);
size_t tsasr_relpos_dpk_table_bytes(int max_jobs);
int tsasr_relpos_dpk_flush(void *table_host, void *table_dev, size_t table_bytes, void *stream);
void tsasr_relpos_dpk_discard(void);
/* Dropout keep-bits handed from the forward to the backward (an optimisation of the pair above, not a change of their results): with
 * bits = tsasr_relpos_attn_keepbits_bytes(B, T, H) > 0 bytes of device memory set by tsasr_relpos_attn_keepbits right before
 * tsasr_relpos_attn_fwd[_ws] (bf16, Dh = 64, 2 <= T <= 256, pdrop > 0) the forward stores the mask bits it hashed, and set again right
 * before the matching tsasr_relpos_attn_bwd the backward reads them (one 16-byte load per query row) instead of hashing every element
 * again. The setting is consumed by the next forward / backward call; without it both hash - the same bits. */
size_t tsasr_relpos_attn_keepbits_bytes(int B, int T, int H);
void tsasr_relpos_attn_keepbits(void *bits);

/* ------------------------------------------------------------------------------------------
 * Global-norm clipping + AdamW over the flat parameter arena: replaces SB/core.py:1082-1093
 * (torch.nn.utils.clip_grad_norm_ -> torch.optim.AdamW.step) with two launches; the norm stays on the device.
 * p, g, m, v: flat fp32 [n]; p_bf16 (may be NULL): bf16 shadow of p rewritten in the same pass; hyper: DEVICE float[3] = {lr, 1-beta1^t, 1-beta2^t} (graph-capturable Noam schedule).
 * norm_out (may be NULL): DEVICE float = L2 norm of g before clipping (finite whenever the norm is an fp32 number: the squares are summed a second time in
 * scaled form where they overflow). skipped_out: NULL = the reference's behaviour on a non-finite norm (SB/core.py:1072-1093: the step is
 * applied - clip_grad_norm_'s factor is NaN / 0 - and only the non-finite loss is counted); a DEVICE float = such a step is SKIPPED (parameters and moments untouched) and
 * counted there (+= 1): the build's `skip_nonfinite_step: True` option.
 * ------------------------------------------------------------------------------------------ */
/* dst[i] += src[i] for `count` small fp32 vectors in one launch; table (DEVICE) = [count src ptrs][count dst ptrs][count int32 lengths]. */
int tsasr_accumulate_many(const void *table, int count, void *stream);
size_t tsasr_clip_adamw_workspace_bytes(void);
int tsasr_clip_adamw_step(float *p, void *p_bf16, const float *g, float *m, float *v, const float *hyper, float *norm_out, float *skipped_out,
                          long long n, float beta1, float beta2, float eps, float weight_decay, float max_norm, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with the operand layouts of a Linear layer (replaces the library GEMMs behind torch.nn.functional.linear on
 * SB/nnet/attention.py:549-553,581-583,635,820-836, Conformer.py:76-82,98, SB/nnet/linear.py:64-78):
 *   C[M,N] (+)= op(A)[M,K] . op(B)[K,N];  transA=0: A [M,K], 1: A [K,M];  transB=0: B [N,K] (a Linear weight), 1: B [K,N].
 *   out_dtype TSASR_BF16 | TSASR_F32; accumulate (fp32 only; 2 = the slab sum may be deferred, see tsasr_reduce_defer): C += result, used to add weight gradients straight into the
 *   fp32 gradient arena (long inner dimensions are split into fp32 slabs in `workspace`, summed in a fixed order).
 * ------------------------------------------------------------------------------------------ */
void tsasr_gemm_set_ring(int on);                 /* 1 (default): LDS-DMA ring main loop for long inner dimensions; 2: whenever K % 64 == 0; 0: register-staged loop (A/B tests) */
void tsasr_gemm_set_lab_floor(int floor_mode);   /* lab (tools/gemm_bench.py --floors): -1 off; 0/1/2 = round-3 four-wave loop / its DMA ring alone / its MFMA part alone */
void tsasr_gemm_set_plan(int tile, int splits);   /* A/B tests only: force macro-tile (0 = 128x128, 1 = 128x64, 2 = 64x64, -1 = automatic) and split-K */
size_t tsasr_gemm_bf16_workspace_bytes(int M, int N, int K, int out_dtype);
int tsasr_gemm_bf16(const void *A, const void *B, void *C, int M, int N, int K, long long lda, long long ldb, long long ldc,
                    int transA, int transB, int out_dtype, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
/* Same GEMM (bf16 out) with a fused elementwise epilogue - the Linear + activation() + Dropout of PositionalwiseFeedForward
 * (SB/nnet/attention.py:820-836) without a separate pass over the [M, d_ffn] hidden activation:
 *   epi_mode 1: C = dropout_p(LeakyReLU_slope(A.B + bias[n]));   epi_mode 2 (its backward on the dgrad GEMM):
 *   C = (A.B) * keep(m,n)/(1-p) * LeakyReLU'(y[m,n]) and dbias[n] = column sums of C.  Masks: counter-based, (seed + *seed_dev, m*N+n). */
/* fp32 GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): the Linear layers of the PARITY mode - the reference's default precision is
 * fp32 (conformer-t_scratch.yaml:88; SB/nnet/linear.py:64-78, attention.py:549-553, 581-583, 820-836, Conformer.py:76-82, 98), the
 * benchmarked step computes them in bf16. C[M,N] (+)= op(A) . op(B), operands and sums in fp32, layouts as tsasr_gemm_bf16; accumulate
 * != 0: C += result. Any shape and stride. */
int tsasr_gemm_f32(const float *A, const float *B, float *C, int M, int N, int K, long long lda, long long ldb, long long ldc, int transA,
                   int transB, int accumulate, void *stream);
/* nbatch products with one shared left operand in ONE launch: C_i [M,N] = A [M,K] . B_i^T, B_i = btab[i] (a DEVICE array of device
 * pointers to bf16 [N,K] matrices, row stride ldb), C_i = C + i * c_batch elements. The 12 + 6 `linear_pos` projections of the one
 * positional table (SB/nnet/attention.py:433, 560: every RelPosMHAXL layer projects the same pos_embs). K % 64 == 0, N % 8 == 0. */
int tsasr_gemm_bf16_nt_batched(const void *A, const void *const *btab, void *C, int M, int N, int K, long long lda, long long ldb,
                               long long ldc, long long c_batch, int nbatch, void *stream);
size_t tsasr_gemm_bf16_fused_workspace_bytes(int M, int N);
/* `mask` (may be NULL; only where tsasr_gemm_bf16_fused_mask_ok(M, N, K) and transA = transB = 0): uint16 [M][N/8], one word per 8
 * consecutive outputs - bits 0-7 the dropout keep-bits, bits 8-15 "the stored activation is negative". The mode-1 call writes it; the
 * mode-2 call given the same words reads them INSTEAD of y and of re-hashing the keep-bits (y must still be passed): M*N/4 bytes read
 * instead of 2*M*N. Same results bit for bit. */
int tsasr_gemm_bf16_fused_mask_ok(int M, int N, int K);
int tsasr_gemm_bf16_fused(const void *A, const void *B, void *C, int M, int N, int K, long long lda, long long ldb, long long ldc,
                          int transA, int transB, int epi_mode, const float *bias, const void *y, long long ldy, float slope, float p,
                          unsigned long long seed, const unsigned long long *seed_dev, float *dbias, void *mask, void *workspace,
                          size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * LSTM cell steps of the prediction network (replaces torch.nn.LSTM behind SB/nnet/RNN.py:244-278; gate order i,f,g,o).
 * gates [B,U,H,4] fp32 - GATE-MINOR: the gates (i,f,g,o) of a unit are one float4, i.e. column 4*k + g of a [B*U, 4H] matrix, so
 * the caller permutes the rows of W_ih (and of W_hh if it adds h_{t-1} W_hh^T itself with tsasr_gemm_bf16 accumulate) from the
 * reference's gate-major order: pre-activations in, ACTIVATED gates out; c [B,U,H] fp32; h [B,U,H] io_dtype. One launch per time step; step t reads step t-1.
 * bwd: dout [B,U,H] (gradient of the layer output), dh_rec [B,H] fp32 (= dgates_{t+1} . W_hh, ignored at t = U-1),
 * dc_io [B,H] fp32 carried between steps, dgates [B,U,4H] io_dtype out (operand of the dh / dW GEMMs).
 * ------------------------------------------------------------------------------------------ */
int tsasr_lstm_cell_fwd(float *gates, float *c, void *h, int B, int U, int H, int t, int io_dtype, void *stream);
/* Fused variants: recurrent product (MFMA, K split over the waves) + cell update in one launch per step; whh bf16 [4H,H], whhT bf16 [H,4H]. */
int tsasr_lstm_step_fwd(float *gates, float *c, void *h, const void *whh, int B, int U, int H, int t, int io_dtype, void *stream);
int tsasr_lstm_step_bwd(const float *gates, const float *c, const void *dout, void *dgates, const void *whhT, float *dc_io, int B, int U,
                        int H, int t, int io_dtype, void *stream);
int tsasr_lstm_cell_bwd(const float *gates, const float *c, const void *dout, const float *dh_rec, float *dc_io, void *dgates, int B,
                        int U, int H, int t, int io_dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * A1 Fbank: replaces SB/lobes/features.py:130-147 = STFT (SB/processing/features.py:134-178; n_fft 512, periodic Hamming 512,
 * center=True zero padding, one-sided) + spectral_magnitude power=1 (:317-348) + Filterbank (:482-552) + _amplitude_to_DB
 * (:683-704; floor at per-utterance max - top_db over ALL frames incl. padding).  wav [B,L] fp32 -> out [B,T=1+L/hop,n_mels].
 * A2 InputNormalization(norm_type="sentence"): SB/processing/features.py:1012-1025,1107-1132 (mean / unbiased std over the
 * first lens[b] frames per feature bin, applied to the whole padded row; eps clamps the std).
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_fbank_workspace_bytes(int B, int T, int n_mels);
int tsasr_fbank_fwd(const float *wav, const float *window, const float *melmat, void *out, int B, int L, int T, int n_mels, int hop,
                    float top_db, float amin, int out_dtype, void *workspace, size_t workspace_bytes, void *stream);
int tsasr_sentence_norm_fwd(const void *x, const int32_t *lens, void *y, int B, int T, int F, float eps, int in_dtype, int out_dtype,
                            void *stream);

/* Causal features for streams (build extension; csrc/features_stream.hip).
 * tsasr_fbank_frames: seg [B,Lseg] fp32, a slice of the zero-padded signal -> out_db [B, F = (Lseg-512)/hop + 1, n_mels] fp32, the raw dB
 * of the frames seg[i*hop, i*hop+512): the bits tsasr_fbank_fwd computes for the same samples before its floor.
 * tsasr_running_norm_fwd: db [B,F,n_mels] fp32 -> y (out_dtype): x = max(db, running max over frames so far and bins - top_db);
 * y = (x - mean)/max(std, eps) with the running per-bin mean / unbiased std over the frames so far (fp64 sums in frame order; fewer than
 * 2 frames: std 1), rounded once to fp32 (bf16: that value rounded again). state: per stream 2*n_mels + 2 doubles = S1[n_mels],
 * S2[n_mels], the count (a prior's pseudo-frames included), {float running max, int32 maximum-seen}; all zero = a fresh stream. It
 * advances by the first n_valid[b] frames of stream b only; later frames are normalised with it frozen. n_mels <= 128. */
size_t tsasr_fbank_frames_workspace_bytes(int n_mels);
int tsasr_fbank_frames(const float *seg, const float *window, const float *melmat, float *out_db, int B, int Lseg, int F, int n_mels, int hop,
                       float amin, void *workspace, size_t workspace_bytes, void *stream);
size_t tsasr_running_norm_state_bytes(int B, int n_mels);
int tsasr_running_norm_fwd(const float *db, const int32_t *n_valid, void *state, void *y, int B, int F, int n_mels, float top_db, double eps,
                           int out_dtype, void *stream);

/* Causal features of slot sessions (StreamingTranscriber.admit(..., audio=True)): every row of the batch is a session with its own sample
 * count and frame position. The samples live in a ring [B,cap] fp32 on the device, sample s of slot b at ring[b][s % cap]; the host keeps
 * the counts and sends them per call as a small int32 table.
 * tsasr_audio_ring_append: tbl [2][B] = {have[b] % cap, lens[b]}; ring[b][(have[b] + i) % cap] = wav[b][i], i < lens[b], wav [B,N] fp32 with
 * row stride wav_stride elements. One launch; a row with lens[b] == 0 is not touched. N <= cap, cap >= 512.
 * tsasr_fbank_frames_slots: tbl [3][B] = {first[b], count[b], total[b]} -> out_db [B,F,n_mels] fp32. Row i < count[b] of slot b is the raw
 * dB of frame first[b] + i of the session's signal with 256 zeros on the left and zeros from sample total[b] on (the right padding of an
 * ended session; bytes an earlier session left in the ring are never read): the bits tsasr_fbank_fwd / tsasr_fbank_frames compute for the
 * same samples, from the same frame body. Rows count[b] .. F-1 are zeros. The caller keeps cap large enough that no sample a later frame
 * reads has been overwritten (csrc/features_stream.hip derives cap). Workspace: tsasr_fbank_frames_workspace_bytes(n_mels).
 * The normalisation of such frames is tsasr_running_norm_fwd on a [B] state (n_valid[b] = 0 leaves a slot's state alone). */
int tsasr_audio_ring_append(float *ring, const float *wav, const int32_t *tbl, int B, int N, long long wav_stride, int cap, void *stream);
int tsasr_fbank_frames_slots(const float *ring, const int32_t *tbl, const float *window, const float *melmat, float *out_db, int B, int cap, int F,
                             int n_mels, int hop, float amin, void *workspace, size_t workspace_bytes, void *stream);

/* Fused seam between two Conformer sub-blocks: s = res + alpha*timemask(dropout_p(x + bias)); y = LayerNorm(s)
 * (Dropout -> [0.5*]x + residual -> masked_fill_ -> nn.LayerNorm; Conformer.py:113-114,194-217,239-259) and its backward
 * (dres = LN_bwd(dy) + dout; dx = alpha*timemask*dropmask/(1-p)*dres; dgamma, dbeta, dbias; dout and any of the three parameter
 * gradients may be NULL). D % 8 == 0, D <= 2048; kernel per width and LDS per launch: the "Row kernels" table above. */
int tsasr_add_layernorm_fwd(const void *x, const float *bias, const void *res, void *s, void *y, float *mean, float *rstd,
                            const float *gamma, const float *beta, long long M, int D, float alpha, float p, unsigned long long seed,
                            const unsigned long long *seed_dev, const int32_t *valid_lens, int Trows, float eps, int io_dtype,
                            void *stream);
size_t tsasr_add_layernorm_bwd_workspace_bytes(long long M, int D);
int tsasr_add_layernorm_bwd(const void *dy, const void *dout, const void *s, const float *gamma, const float *mean, const float *rstd,
                            void *dres, void *dx, float *dgamma, float *dbeta, float *dbias, long long M, int D, float alpha, float p,
                            unsigned long long seed, const unsigned long long *seed_dev, const int32_t *valid_lens, int Trows,
                            int io_dtype, void *workspace, size_t workspace_bytes, void *stream);
/* The same seam with the GEMM that produces x in front of it, in one launch: x = A[M,K] . W[N,K]^T (bf16, never written) for N = K = 256 -
 * the attention's out_proj (SB/nnet/attention.py:549-553) and the convolution module's last point-wise convolution (Conformer.py:76-98)
 * followed by `x + skip` / `x + conv(..)` and the LayerNorm that reads the sum (Conformer.py:243-259). (s, y, mean, rstd) are bit-identical
 * to tsasr_gemm_bf16 + tsasr_add_layernorm_fwd; the backward is tsasr_add_layernorm_bwd + the GEMM's. lda / ldw: row strides in elements. */
int tsasr_linear_add_layernorm_ok(long long M, int N, int K, long long lda, long long ldw);
int tsasr_linear_add_layernorm_fwd(const void *A, long long lda, const void *W, long long ldw, const float *bias, const void *res, void *s,
                                   void *y, float *mean, float *rstd, const float *gamma, const float *beta, long long M, int N, int K,
                                   float alpha, float p, unsigned long long seed, const unsigned long long *seed_dev,
                                   const int32_t *valid_lens, int Trows, float eps, void *stream);
/* Two LayerNorms in a row with the residual tail in front - norm2 of a Conformer layer and the next layer's first LayerNorm (or the
 * encoder's final norm): Conformer.py:194-217,259, models/conformer.py:223-233. (s, y, z) bit-identical to tsasr_add_layernorm_fwd +
 * tsasr_layernorm_fwd; the backward takes dz and (optionally) the gradients reaching y and s along other paths. D % 8 == 0, D <= 1024
 * ("Row kernels" table above); any of the five parameter gradients may be NULL. */
int tsasr_add_layernorm2_fwd(const void *x, const float *bias, const void *res, void *s, void *y, void *z, float *mean, float *rstd,
                             float *mean2, float *rstd2, const float *gamma, const float *beta, const float *gamma2, const float *beta2,
                             long long M, int D, float alpha, float p, unsigned long long seed, const unsigned long long *seed_dev,
                             const int32_t *valid_lens, int Trows, float eps, float eps2, int io_dtype, void *stream);
size_t tsasr_add_layernorm2_bwd_workspace_bytes(long long M, int D);
int tsasr_add_layernorm2_bwd(const void *dz, const void *dy, const void *dout, const void *s, const float *gamma, const float *beta,
                             const float *gamma2, const float *mean, const float *rstd, const float *mean2, const float *rstd2, void *dres,
                             void *dx, float *dgamma, float *dbeta, float *dbias, float *dgamma2, float *dbeta2, long long M, int D,
                             float alpha, float p, unsigned long long seed, const unsigned long long *seed_dev, const int32_t *valid_lens,
                             int Trows, int io_dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Whole-sequence LSTM recurrences (all U steps of tsasr_lstm_step_fwd / _bwd). One persistent launch per direction (workgroups
 * exchange h_t / dG_t through write-through stores and an arrival counter) when io_dtype is bf16, H is 256 or 512, and the grid fits
 * the device: G = ceil(B / BR) exchange groups of BR = 8 (B <= 8) or 16 rows, G <= 16 (so B <= 256) and G * H / 32 workgroups <= the
 * compute units THIS device exposes (tsasr_lstm_seq_persistent tells); B = 1 with H = 512 runs the single-utterance kernels unless
 * TSASR_LSTM_SEQ1=0. Otherwise (any other H % 16 == 0, fp32 io, B > 256, too few CUs) a loop of the per-step kernels.
 * Replaces the time loop inside torch.nn.LSTM (speechbrain/nnet/RNN.py:244-278). */
/* Input projection of the predictor when its Embedding is one-hot and frozen (speechbrain/nnet/embedding.py:76-95 consider_as_one_hot,
 * train_librispeechmix_scratch.py:117-119 `embedding` -> `decoder`): gates [B,U,H,4] fp32 = b_ih + b_hh + the token's column of w_ih
 * [4H, I] (fp32), i.e. F.embedding + x . W_ih^T + biases of torch.nn.LSTM without the gather, the casts and the GEMM. tokens int64 [B,U];
 * token k -> column k-1 above `blank`, k below it, blank -> zeros. xp (may be NULL): bf16 [B*U, Ip] one-hot rows + ones in columns I, I+1
 * (I + 2 <= Ip <= H): the operand the backward's weight-gradient GEMM contracts with. */
int tsasr_lstm_onehot_gates(const long long *tokens, const float *w_ih, const float *b_ih, const float *b_hh, float *gates, void *xp, int B,
                            int U, int H, int I, int Ip, int blank, void *stream);
int tsasr_lstm_seq_persistent(int B, int H, int io_dtype);   /* 1: one persistent launch per direction on this device for this shape */
size_t tsasr_lstm_seq_workspace_bytes(int B, int U, int H);   /* first 256 bytes: uint32 {arrival counter, error word} per batch group; a non-zero error word = an inter-workgroup wait timed out (outputs poisoned with NaN) */
int tsasr_lstm_seq_fwd(float *gates, float *c, void *h, const void *whh, int B, int U, int H, int io_dtype, void *workspace,
                       size_t workspace_bytes, void *stream);
int tsasr_lstm_seq_bwd(const float *gates, const float *c, const void *dout, void *dgates, const void *whhT, int B, int U, int H,
                       int io_dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Transposed bf16 copies of a list of row-major matrices (GEMM weights -> k-contiguous operands of the input-gradient GEMMs), one
 * launch. jobs: DEVICE int32 [njobs][5] = {src offset, dst offset (elements), rows, cols, first 64x64 tile index}. */
int tsasr_transpose_many_bf16(const void *src_base, void *dst_base, const void *jobs, int njobs, int ntiles, void *stream);

/* Grouped weight gradients (csrc/wgrad.hip): replaces, for every Linear / kernel-size-1 Conv1d weight of the path, the reference's
 * autograd AccumulateGrad of dW = dy^T . x (SB/nnet/linear.py:64-78, SB/nnet/attention.py:549-553,820-836,
 * SB/lobes/models/transformer/Conformer.py:76-98) and the per-weight split-K launches of round 1. tsasr_wgrad_queue only records
 *   dW[M,N] (fp32, row stride ldc) += dy[K,M]^T . x[K,N]      (bf16 row-major, K = tokens; M, N, ld_dy, ld_x multiples of 8)
 * - dy, x and dW must stay alive and unmodified until tsasr_wgrad_flush runs every queued job in ONE launch of 256x256 output
 * tiles (no split along K: each tile owns its piece of dW, plain read-add-store, bit-reproducible). Two queued jobs must not
 * target overlapping dW. Job table protocol as tsasr_reduce_flush (pinned host + device table; under stream capture the caller
 * uploads the table after the capture). */
int tsasr_wgrad_queue(const void *dy, const void *x, float *dW, int M, int N, int K, long long ld_dy, long long ld_x, long long ldc);
int tsasr_wgrad_pending(void);
size_t tsasr_wgrad_table_bytes(int max_jobs);
int tsasr_wgrad_flush(void *table_host, void *table_dev, size_t table_bytes, void *stream);
void tsasr_wgrad_discard(void);
/* The NEXT tsasr_wgrad_flush runs with `slots` LDS-DMA slots (2: 64 KB of LDS per workgroup, for a launch that should share the CUs
 * with another stream's kernels; 0: default 128 KB). One-shot. */
void tsasr_wgrad_next_flush_slots(int slots);
/* The NEXT tsasr_wgrad_flush launches at most `wgs` workgroups that walk the tiles persistently (0: one workgroup per tile). One-shot. */
void tsasr_wgrad_next_flush_wgs(int wgs);

/* Recipe glue on the device (csrc/misc.hip), each ONE launch instead of a chain of tiny library kernels:
 * tsasr_mean_pool_*: masked mean over time of the speaker encoder's output (train_librispeechmix_scratch.py:52-64);
 * tsasr_abs_lengths: relative -> absolute lengths (round half to even: models/conformer.py:272, SB/nnet/losses.py:58-59; floor:
 *   SB/nnet/RNN.py:35; ceil clamped: train_librispeechmix_scratch.py:54-58) for up to 8 vectors at once;
 * tsasr_count_nonfinite: the non-finite-loss counter of SB/core.py:1115-1150 kept on the device. */
int tsasr_mean_pool_fwd(const void *x, const float *rel, void *out, int B, int T, int D, int io_dtype, void *stream);
int tsasr_mean_pool_bwd(const void *dout, const float *rel, void *dx, int B, int T, int D, int io_dtype, void *stream);
int tsasr_abs_lengths(const float *const *rel, int *const *out, const int *dim, const int *mode, int n, int B, void *stream);
/* Speaker-embedding injection modes `sum` / `prod` (models/conformer.py:247-253; mode 0 / 1): out [B,T,D] = src [B,T,D] (+ | *) spk [B,1,D],
 * D % 8 == 0; backward in one pass over dout: dsrc [B,T,D] (mode 0: may be NULL - it equals dout), dspk [B,1,D] (sums over t in a fixed order). (`cat` = column ranges of
 * tsasr_gemm_bf16*, `cross_attention` = tsasr_attn_f32_* between GEMMs.) */
int tsasr_inject_fwd(const void *src, const void *spk, void *out, int B, int T, int D, int mode, int io_dtype, void *stream);
int tsasr_inject_bwd(const void *dout, const void *src, const void *spk, void *dsrc, void *dspk, int B, int T, int D, int mode, int io_dtype,
                     void *stream);
/* ------------------------------------------------------------------------------------------
 * Greedy transducer search on the device (SB/decoders/transducer.py:138-218, transducer_greedy_decode; csrc/search.hip
 * greedy_decode_kernel): one launch decodes the batch, one persistent workgroup per utterance; predictor = embedding table -> one-layer
 * LSTM -> Linear, joiner = LeakyReLU(enc + pn) -> Linear head; at most one symbol per frame, the predictor advances only on a non-blank;
 * the arg max takes the lowest index among ties. enc [B,T,J] (io_dtype); emb fp32 [n_emb, E]; LSTM weights in torch layout (w_ih [4H,E],
 * w_hh [4H,H], gate order i,f,g,o); w_proj [J,H]; w_head [V,J]; matrices in `wdtype` (TSASR_F32 | TSASR_BF16), biases fp32 or NULL;
 * H, J multiples of 4 and <= 1024. preds int32 [B,T]: symbol emitted at frame t or -1; logp_sum fp32 [B]: sum of the emitted symbols'
 * log-probabilities.
 * wide == 0: V <= 63 and E <= 64 (character models). wide != 0, the WIDE instantiations for subword vocabularies: V <= 1024 and E <= 1024
 * (a one-hot table has E = V - 1; E % 4 == 0 runs a dense product, any other E adds the columns of w_ih that meet a non-zero entry of the
 * embedding row); a character model through them gives its own result.
 * state and n_valid both NULL: the offline search. Both given: one chunk of a stream; state fp32 [B, 2H + J + 4] (caller-owned, zeroed
 * before the first chunk) carries h, c, the projected predictor output, the last symbol, the running log-prob sum and a primed flag
 * between calls; n_valid int32 [B] = frames of this chunk to decode per utterance (preds of the others are -1; a zero count leaves the
 * state untouched); logp_sum [B] receives the running sum. A tensor decoded in pieces gives the bits of one offline call over it.
 * Exactly one of the two NULL is TSASR_E_INVALID.
 * ------------------------------------------------------------------------------------------ */
int tsasr_greedy_decode(const void *enc, const float *emb, const void *w_ih, const void *w_hh, const float *b_ih, const float *b_hh,
                        const void *w_proj, const float *b_proj, const void *w_head, const float *b_head, float *state, const int32_t *n_valid,
                        int *preds, float *logp_sum, int B, int T, int J, int H, int E, int V, int blank, float slope, int io_dtype,
                        int wdtype, void *stream, int wide);

/* ------------------------------------------------------------------------------------------
 * The beam search's workspace, a function of the shape alone:
 *   B * (align16(64 + 24 beam) + align16(8 nodes) + 4 (cap + beam)(J + 2H + lmw) + ((times ? 1 : 0) + (bias ? 1 : 0)) align16(4 nodes)),
 *   nodes = 1 + (T + 1) beam + cap, lmw = lm_layers > 0 ? (wide ? round_up(V, 4) : 64) + 2 lm_layers lm_hidden : 0
 * per utterance a header with the beam, the token tree, cap + beam predictor slots (each with the node's LM step lm_logp | lm_h | lm_c
 * when an LM is fused: lm_layers 0 = no LM, lm_hidden is then not read), one int per tree node for the emission frames of a timed search
 * and one for the trie states of a biased one. T = max_frames of the calls that use it. 0 when B, T, H, J, V, beam or cap is not
 * positive, lm_layers < 0, or lm_layers > 0 with lm_hidden <= 0 (V sizes nothing unless wide and lm_layers > 0).
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_beam_search_workspace_bytes(int B, int T, int H, int J, int V, int beam, int cap, int lm_layers, int lm_hidden, int times,
                                         int bias, int wide);

/* LM of the fused beam search: embedding -> `layers` stacked LSTM cells -> `dnn_blocks` blocks of Linear, LayerNorm, LeakyReLU -> Linear
 * to V (SB/lobes/models/RNNLM.py). 1 <= layers <= 4, 0 <= dnn_blocks <= 2; hidden, emb_dim, dnn_neurons multiples of 4 <= 1024
 * (dnn_blocks == 0: dnn_neurons == hidden). Matrices in the call's wdtype, torch layouts (w_ih[l] [4 hidden, l == 0 ? emb_dim : hidden],
 * w_hh[l] [4 hidden, hidden], w_dnn[k] [dnn_neurons, k == 0 ? hidden : dnn_neurons], w_out [V, dnn_neurons]); emb [V, emb_dim], biases
 * and LayerNorm vectors fp32 (NULL: none). */
typedef struct tsasr_lm_desc {
    const float *emb;
    const void *w_ih[4], *w_hh[4];
    const float *b_ih[4], *b_hh[4];
    const void *w_dnn[2];
    const float *b_dnn[2], *ln_g[2], *ln_b[2];
    const void *w_out;
    const float *b_out;
    float ln_eps[2];
    int layers, hidden, emb_dim, dnn_blocks, dnn_neurons;
    float slope; /* LeakyReLU of the dnn blocks */
} tsasr_lm_desc;

/* Phrase graphs of the biased beam search, as prefix tries. A graph has states 0 (root) .. S-1; the packed arrays hold the graphs one
 * after another, S + 1 rows each: child_off int32 [rows] (absolute indices into child_tok / child_to; state row r's edges are
 * child_off[r] .. child_off[r + 1], a graph's last row only closes the one before it), child_tok int32 [edges] ascending within a row,
 * child_to int32 [edges] = the graph's own state ids, pending fp64 [rows] = weight * (depth - depth of the deepest terminal on the
 * path), base int32 [B] = first row of utterance b's graph (< 0 or >= rows: b is not biased), weight fp64 [B]. That child_tok ascends
 * within a row is NOT checked on the device: a binary search reads it, the host constructor (biasing.ContextGraph) guarantees it. */
typedef struct tsasr_bias_desc {
    const int32_t *child_off, *child_tok, *child_to;
    const double *pending;
    const int32_t *base;
    const double *weight;
    int rows, edges;
} tsasr_bias_desc;

/* ------------------------------------------------------------------------------------------
 * Beam transducer search on the device (SB/decoders/transducer.py:220-373, transducer_beam_search_decode; csrc/search.hip
 * beam_search_kernel) for the networks tsasr_greedy_decode takes: one persistent workgroup per utterance, one launch decodes the batch.
 * Scores in fp64 as the host loop; list order as the reference (first maximum of logp / len, appends in top-k order, stable n-best
 * sort, top-k ties: lower index); the log-softmax and the top-k are taken in a fixed order: two calls give the same bits. Each node of
 * the hypothesis tree runs its predictor step once. 2 <= beam <= min(V, 64), 1 <= nbest <= 64, cap >= beam = hypotheses a frame may
 * hold (its A list). workspace >= tsasr_beam_search_workspace_bytes(B, max_frames, H, J, V, beam, cap, lm layers, lm hidden, frames != NULL,
 * bias != NULL, wide). hyps int32 [B,nbest,Lmax] (first min(len, Lmax) tokens), lens int32 [B,nbest] (-1: the beam holds fewer),
 * scores fp64 [B,nbest] = logp / len(prediction incl. the blank prefix), status int32 [B]: 0 ok, 1 a frame needed more than cap
 * hypotheses, 2 token tree full, 3 no hypothesis left to expand; such an utterance stops there, the others are unaffected.
 * n_valid NULL: the offline search over every frame of enc, padding included; it starts the workspace afresh, leaves the final beam in
 * it and takes max_frames == T. n_valid int32 [B]: one chunk of a stream; the beam, token tree and predictor slots are resumed from the
 * workspace (laid out for max_frames; zeroed = start of the stream); n_valid[b] = frames of this chunk to decode (0: the state is left
 * as it is, the outputs describe it, so a zero-count call reads the n-best out again). A nonzero status is sticky. A tensor decoded in
 * pieces gives the bits of one offline call over it. Every call on a workspace has the same frames / lm / bias / wide form.
 * frames NULL: untimed. frames int32 [B,nbest,Lmax]: frames[b,r,i] = index of the encoder frame whose joint emitted hyps[b,r,i],
 * absolute from the start of the utterance or stream, for the first min(len, Lmax) tokens; non-decreasing along a hypothesis (several
 * tokens may share a frame; the offline search decodes padded frames too). hyps, lens, scores and status are the bits of the untimed call.
 * lm NULL: no LM fusion (lm_weight is not read). Else (SB/decoders/transducer.py:264-266, 311-351, 386-409) the LM is evaluated once per
 * hypothesis node on the node's token (blank = the LM's BOS) from the parent's LM state, and a non-blank extension by sym scores
 * (logp(a) + logp_joint[sym]) + lm_weight * log_softmax(lm)[sym] in fp64; the top-k, the expand_beam test and the blank copies read the
 * joint alone.
 * bias NULL: no phrase graphs. Else each hypothesis carries a trie state s (0 at the start). A non-blank extension by v: s has a child
 * c on v -> s' = c, d = w; else d = -pending[s], and if the root has a child c on v -> s' = c, d = d + w, else s' = 0 (no failure
 * links). The extension scores ((logp(a) + logp_joint[v]) [+ lm_weight * lm_logp[v]]) + d in fp64, d last; the top-k, the expand_beam
 * test and the blank copies read the joint alone. The n-best is ranked and reported with (logp - pending[s]) / len; the stored beam
 * keeps logp, so a stream in pieces gives the bits of one call.
 * wide == 0: V <= 63 and E <= 64. LDS: 4 (6H + 2J + 128) + cap (16 + 4 (6 + timed + biased)) bytes, with an LM
 * 4 (max(emb_dim, hidden, dnn_neurons) + 2 hidden + max(4 hidden, dnn_neurons) + 130) more, together <= 152 KB.
 * wide != 0, the WIDE instantiations for subword vocabularies: 2 <= V <= 1024 and E <= 1024 (E <= 64: a side operand of the recurrent
 * product; E % 4 == 0: a dense second product; any other E, the frozen one-hot table's V - 1: one gate row per thread over the non-zero
 * columns); a character model through them gives the bits of wide == 0. LDS, Vp = round_up(V, 4): 4 (6H + 2J + round_up(E, 4) + Vp +
 * 96) + cap (16 + 4 (6 + timed + biased)) bytes, with an LM 4 (max(emb_dim, hidden, dnn_neurons) + 2 hidden + max(4 hidden,
 * dnn_neurons) + 2 Vp + 2) more, together <= 156 KB. A shape past its LDS budget is TSASR_E_INVALID. With a graph, wide must equal
 * V > 63 || E > 64 (the instantiation the biased search of that shape has always run), else TSASR_E_INVALID.
 * ------------------------------------------------------------------------------------------ */
int tsasr_beam_search(const void *enc, const float *emb, const void *w_ih, const void *w_hh, const float *b_ih, const float *b_hh,
                      const void *w_proj, const float *b_proj, const void *w_head, const float *b_head, void *workspace, size_t workspace_bytes,
                      const int32_t *n_valid, int *hyps, int *lens, double *scores, int *status, int B, int T, int max_frames, int J, int H,
                      int E, int V, int blank, int beam, int nbest, int cap, int Lmax, double state_beam, double expand_beam, float slope,
                      int io_dtype, int wdtype, void *stream, int *frames, const tsasr_lm_desc *lm, double lm_weight,
                      const tsasr_bias_desc *bias, int wide);

/* ------------------------------------------------------------------------------------------
 * Edit distance of N pairs of symbol sequences with the path choice of the reference's WER/CER statistics (SB/utils/edit_distance.py:
 * 124-334, Kaldi's compute-wer order: the substitution / match only if strictly cheaper than both others, else the deletion if strictly
 * cheaper than the insertion, else the insertion; row 0 insertions, column 0 deletions; the walk back from (n, m) follows the cell's
 * operation). One launch, one workgroup per pair (csrc/editdist.hip). Ragged int32 input: pair k is ref_sym[ref_off[k] .. ref_off[k+1])
 * against hyp_sym[hyp_off[k] .. hyp_off[k+1]), lengths n, m >= 0; max_ref / max_hyp = the longest of each side (both <= 16384; max_ref ints of dynamic LDS), cells = sum
 * over pairs of (n + 1) * (m + 1). counts int32 [N,4] = edits, insertions, deletions, substitutions; the alignment of pair k in forward
 * order at offset ref_off[k] + hyp_off[k] of align_op uint8 ('=', 'S', 'D', 'I'), align_i, align_j int32 (index into the pair's reference
 * / hypothesis, -1 = aligned to nothing), align_len int32 [N] entries of it (<= n + m; the buffers hold sum(n + m) entries). totals
 * int64 [8] is ADDED to with device-scope atomics: edits, insertions, deletions, substitutions, sum of ref_count[k] (int32 [N]: the
 * reference tokens pair k counts for), pairs, pairs with >= 1 edit, spare. workspace >= tsasr_edit_distance_workspace_bytes(N, cells)
 * = 16 N + cells / 2 + 16 bytes (an upper bound: 2 bits per cell are used, and nothing for a pair whose table fits in 60 KiB), 16-byte
 * aligned; results do not depend on its contents. All pointers are device memory.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_edit_distance_workspace_bytes(int N, long long cells);
int tsasr_edit_distance(const int32_t *ref_sym, const int32_t *ref_off, const int32_t *hyp_sym, const int32_t *hyp_off,
                        const int32_t *ref_count, int N, int max_ref, int max_hyp, long long cells, int32_t *counts, uint8_t *align_op,
                        int32_t *align_i, int32_t *align_j, int32_t *align_len, long long *totals, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Chunk-by-chunk inference of the causal encoder (csrc/stream.hip); eval only, no backward.
 * Relative-position attention of a chunk of C query frames at absolute offset t0: qkv [B,C,H,3*Dh] (RelPosMHAXL's per-head Q|K|V);
 * k_cache / v_cache [B,H,Tmax,Dh] (io_dtype) hold frames 0 .. t0-1 and receive the chunk's K, V at rows t0 .. t0+C-1 (t0 + C <= Tmax);
 * pk_half [Tmax, H*Dh] = linear_pos(PE(d)), d = 0 .. Tmax-1 (RelPosEncXL's table is symmetric: the offline row j - i + T - 1 is row
 * |i - j| here); bias_u / bias_v fp32 [H*Dh] as tsasr_relpos_attn_fwd; key_lens int32 [B] (absolute valid frames) or NULL; causal as
 * tsasr_relpos_attn_fwd on absolute positions (1: look-ahead mask, c > 1: chunks of c frames). out [B,C,H*Dh]. Dh <= 64; bf16 with
 * Dh = 32 / 64 on the matrix cores (bf16 operands, fp32 softmax and sums), fp32 in exact fp32 arithmetic. workspace (>= tsasr_relpos_attn_stream_workspace_bytes, which is 0 when no split is made; NULL = no
 * split): small batches with long caches split the keys across workgroups, merged by a second launch.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_relpos_attn_stream_workspace_bytes(int B, int C, int H, int Dh, int Tmax);
int tsasr_relpos_attn_stream_fwd(const void *qkv, void *k_cache, void *v_cache, const void *pk_half, const float *bias_u, const float *bias_v,
                                 const int32_t *key_lens, void *out, int B, int C, int H, int Dh, int Tmax, int t0, int causal, float scale,
                                 int io_dtype, void *workspace, size_t workspace_bytes, void *stream);
/* The same launch for a batch of slots that do not run in lockstep (same kernels, same key split, same workspace size): the scalar t0 is
 * replaced by t0s, a DEVICE int32 [B], so no launch argument changes from chunk to chunk.
 *   t0s[b] >= 0: slot b is active in this launch. Its chunk's queries sit at absolute frames t0s[b] .. t0s[b]+C-1 of its own stream; its
 *     K and V rows are appended to its cache at t0s[b]; keys < t0s[b] come from its cache, the rest from qkv. key_lens[b], the causal
 *     limit and the block-causal limit are all on that slot's own absolute frames; the band row is |i - j|.
 *   t0s[b] < 0: slot b is idle. Nothing of its K/V cache is read or written, its `out` rows are written as exact zeros, its workgroups
 *     leave at once (split, merge and unsplit launches alike).
 * The caller checks t0s before the launch (the device array cannot be read here); in the kernel a slot whose t0s[b] + C > Tmax is
 * treated as idle, so no row past the cache can be written. A slot's output equals tsasr_relpos_attn_stream_fwd's at t0 = t0s[b] for the
 * same (B, C, Tmax) bit for bit. */
int tsasr_relpos_attn_stream_slots_fwd(const void *qkv, void *k_cache, void *v_cache, const void *pk_half, const float *bias_u,
                                       const float *bias_v, const int32_t *key_lens, void *out, int B, int C, int H, int Dh, int Tmax,
                                       const int32_t *t0s, int causal, float scale, int io_dtype, void *workspace, size_t workspace_bytes,
                                       void *stream);
/* tsasr_convmod_fwd with causal = 1 on a chunk y2 [B,C,2D], no saved tensors: the K-1 GLU rows in front of the chunk come from
 * hist_in fp32 [B,K-1,D] (zeros = the offline zero pad), the last K-1 GLU rows of [history | chunk] are written to hist_out (a second
 * buffer: swap the two per chunk). z [B,C,D] (io_dtype). Every row of hist_out is written by every call (rows carried over from
 * hist_in bit for bit when C < K-1); slope < 0 means no activation, as in tsasr_convmod_fwd; hist_in == hist_out is rejected. */
int tsasr_convmod_stream_fwd(const void *y2, const float *b2, const float *conv_w, const float *conv_b, const float *gamma,
                             const float *beta, const float *hist_in, float *hist_out, void *z, int B, int C, int D, int K, float eps,
                             float slope, int io_dtype, void *stream);
/* tsasr_convmod_stream_fwd's arguments plus t0s, the device int32 [B] of tsasr_relpos_attn_stream_slots_fwd (only its sign is read):
 * t0s[b] >= 0: slot b is active, its z rows and hist_out rows are tsasr_convmod_stream_fwd's bit for bit. t0s[b] < 0: slot b is idle,
 * hist_out receives hist_in's rows bit for bit and its z rows are zeros. The caller keeps swapping the two buffers per chunk. */
int tsasr_convmod_stream_slots_fwd(const void *y2, const float *b2, const float *conv_w, const float *conv_b, const float *gamma,
                                   const float *beta, const float *hist_in, float *hist_out, void *z, int B, int C, int D, int K, float eps,
                                   float slope, int io_dtype, const int32_t *t0s, void *stream);

int tsasr_count_nonfinite(const float *x, int n, int *counter, void *stream);

/* Direct RCCL gradient all-reduce over xGMI (csrc/comm.hip): replaces the NCCL calls behind the reference's per-module
 * DistributedDataParallel reducers (SB/core.py:1464-1484; `no_sync` :1585-1615) and SB/utils/distributed.py:123-201's process-group
 * collectives for the gradient path. One communicator per process (one process per GPU). librccl is dlopen()ed
 * (tsasr_allreduce_load; NULL = "librccl.so" on the loader path - pass the copy PyTorch has loaded); rank 0 makes the 128-byte unique
 * id (tsasr_allreduce_unique_id), the caller ships it to the other ranks, every rank calls tsasr_allreduce_init. A bucket is reduced
 * IN PLACE on `stream` (sum or average over the ranks), asynchronously and graph-capturably; "wait" is a stream join by the caller. */
int tsasr_allreduce_load(const char *librccl_path);
int tsasr_allreduce_unique_id(void *host_id128);
int tsasr_allreduce_init(const void *host_id128, int nranks, int rank);
int tsasr_allreduce_ready(void);   /* number of ranks of the communicator, 0 = none */
int tsasr_allreduce_bucket(void *buf, size_t count, int dtype, int average, void *stream);
int tsasr_allreduce_destroy(void);

/* Batched deterministic reductions of partial gradient rows / split-K slabs (csrc/reduce.hip). While tsasr_reduce_defer(1) is in
 * force the parameter-gradient outputs of the *_bwd entry points (dgamma, dbeta, dbias, conv-module dparams, fused-GEMM dbias)
 * and of tsasr_gemm_bf16(accumulate = 2) are only QUEUED: their workspaces and outputs must stay alive and untouched until
 * tsasr_reduce_flush runs all queued jobs in one launch (table_host: pinned host memory, table_dev: device memory, both at least
 * tsasr_reduce_table_bytes(tsasr_reduce_pending()) bytes; must outlive a captured graph). While `stream` is being captured the flush
 * fills table_host only: the caller copies it to table_dev once, after the capture has ended, so a replayed graph carries no memcpy
 * node. Replaces ~310 small launches per step. */
int tsasr_reduce_defer(int on);
int tsasr_reduce_pending(void);
/* Drops every queued reduction without running it and switches deferral off (error path of a step that raised half-way). */
void tsasr_reduce_discard(void);
size_t tsasr_reduce_table_bytes(int max_jobs);
int tsasr_reduce_flush(void *table_host, void *table_dev, size_t table_bytes, void *stream);
/* Only the jobs whose partial rows were produced on `stream` (complete in its order): the main stream reduces its share while a
 * forked stream still runs its part of backward; the rest goes with the final tsasr_reduce_flush. Needs its own table pair. */
int tsasr_reduce_flush_stream(void *table_host, void *table_dev, size_t table_bytes, void *stream);

/* SpecAugment on the normalised features (speechbrain/lobes/augment.py:32-201, applied at train_librispeechmix_scratch.py:91-94;
 * recipe settings conformer-t_scratch.yaml:132-142). tsasr_specaug_draw produces every random number of one call on the device
 * (params: tsasr_specaug_params_words(B, n_freq_mask, n_time_mask) int32 = {c, w, freq widths [B][nf], freq starts, time widths
 * [B][nt], time starts}; c ~ U[window, T-window), w ~ U[c-window, c+window)+1, width ~ U[lo, hi), start ~ U[0, max(1, D - max width
 * over the batch)); window == 0 or T - window <= window: c = w = 0 = no warp). tsasr_specaug_apply: y = masks(warp(x)) for x, y
 * [B,T,F] (y != x): bicubic (cubic convolution, align_corners) resize of [0,c) -> [0,w) and [c,T) -> [w,T) along time, then frequency
 * masks filled with mean(warped) and time masks filled with mean(frequency-masked) (0 when replace_with_zero). At most 8 masks per
 * axis. No host synchronisation anywhere (the reference syncs once per mask axis on mask_len.max()). */
size_t tsasr_specaug_params_words(int B, int n_freq_mask, int n_time_mask);
int tsasr_specaug_draw(int32_t *params, int B, int T, int F, int window, int n_freq_mask, int f_lo, int f_hi, int n_time_mask, int t_lo,
                       int t_hi, unsigned long long seed, const unsigned long long *seed_dev, void *stream);
size_t tsasr_specaug_workspace_bytes(void);
int tsasr_specaug_apply(const void *x, void *y, const int32_t *params, int B, int T, int F, int n_freq_mask, int n_time_mask,
                        int replace_with_zero, int io_dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Speed perturbation = polyphase windowed-sinc resampling of the waveform (speechbrain/processing/speech_augmentation.py:435-820,
 * applied at train_librispeechmix_scratch.py:82-85; recipe: 16 kHz -> 15.2 / 16 / 16.8 kHz). x [B,L] fp32 -> y [B,n_out] with
 * n_out = tsasr_resample_out_len(L, orig, new); weights [P,W] fp32 / first [P] int32 (device) are the filter bank and first input
 * index per phase (P = new/gcd phases, stride = orig/gcd input samples per unit), built by the host as Resample._indices_and_weights
 * does. Output n = q*P + i is sum_j weights[i][j] * x[first[i] + q*stride + j] with zeros outside the signal. */
long long tsasr_resample_out_len(long long n_in, int orig_freq, int new_freq);
int tsasr_resample_fwd(const float *x, float *y, const float *weights, const int32_t *first, int B, int L, int n_out, int P, int stride,
                       int W, void *stream);

/* out[c] (+)= sum_m x[m][c], x [M, N] io_dtype (N % 8 == 0, N <= 2048): bias gradient of a GEMM-shaped layer (front-end convolutions,
 * speechbrain/nnet/CNN.py:629-676). The final sum over per-workgroup partials goes through the deferrable batched reduction. */
size_t tsasr_colsum_workspace_bytes(long long M, int N);
int tsasr_colsum(const void *x, float *out, long long M, int N, int accumulate, int io_dtype, void *workspace, size_t workspace_bytes,
                 void *stream);

/* ------------------------------------------------------------------------------------------
 * Single-layer LSTM in EXACT fp32 arithmetic with an optional initial state (csrc/lstm_f32.hip): the `compute_dtype: fp32` parity mode of
 * the predictor (torch.nn.LSTM behind SB/nnet/RNN.py:170-278) and the step-wise predictor calls of the searchers
 * (SB/decoders/transducer.py:246-353,411-466: one token, carried (h, c)). Gate order i, f, g, o; x [B,U,I], w_ih [4H,I], w_hh [4H,H],
 * biases [4H] or NULL, h0 / c0 [B,H] or NULL (zeros). hs [B,U,H]; hn / cn [B,H] or NULL; cs [B,U,H] and gates [B,U,4H] (activated) are
 * what the backward needs (NULL when not training). Backward: dgates [B,U,4H] w.r.t. the gate pre-activations (the weight / bias / input
 * gradients are GEMMs over all (b,t): tsasr_gemm_f32), dh0 / dc0 optional. H <= 1024.
 * ------------------------------------------------------------------------------------------ */
int tsasr_lstm_f32_fwd(const float *x, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, const float *h0,
                       const float *c0, float *hs, float *cs, float *gates, float *hn, float *cn, int B, int U, int I, int H, void *stream);
int tsasr_lstm_f32_bwd(const float *dout, const float *dhn, const float *dcn, const float *gates, const float *cs, const float *c0,
                       const float *w_hh, float *dgates, float *dh0, float *dc0, int B, int U, int H, void *stream);

/* ------------------------------------------------------------------------------------------
 * Attention in EXACT fp32 arithmetic (csrc/attention_f32.hip; no matrix cores, no bf16 rounding of operands): the `compute_dtype: fp32`
 * parity mode of RelPosMHAXL (same reference lines as tsasr_relpos_attn_*: SB/nnet/attention.py:586-633, rel_shift :468-483) and, with
 * pk == NULL and Tq != Tk, the core of torch.nn.MultiheadAttention for the `cross_attention` speaker injection (models/conformer.py:263-266).
 * q / k / v are strided views: strides[9] (HOST, in elements) = {q batch, q row, q head, k batch, k row, k head, v batch, v row, v head}
 * (RelPosMHAXL's interleaved qkv [B,T,H,3*Dh]: {T*3D, 3D, 3Dh} with k = qkv + Dh, v = qkv + 2*Dh). pk [2*Tk-1, H*Dh] or NULL,
 * bias_u / bias_v fp32 [H*Dh] or NULL; key_lens int32 [B] or NULL; causal as tsasr_relpos_attn_fwd (C > 1: block-causal extension).
 * out [B,Tq,H*Dh] (io_dtype), lse fp32 [B,H,Tq]. Dropout bit of element ((b*H+h)*Tq+i)*Tk+j from (seed + *seed_dev). Dh <= 64.
 * Backward: dq / dk / dv through dstrides[9] (same meaning), dpk [2*Tk-1, H*Dh] when pk != NULL, d_bias_u / d_bias_v fp32 [H*Dh] or NULL
 * (queued while tsasr_reduce_defer(1) is in force, like every parameter-gradient output). Three deterministic passes, no atomics;
 * the workspace holds two fp32 [B,H,Tq,Tk] planes.
 * ------------------------------------------------------------------------------------------ */
int tsasr_attn_f32_fwd(const void *q, const void *k, const void *v, const long long *strides, const void *pk, const float *bias_u,
                       const float *bias_v, const int32_t *key_lens, void *out, float *lse, int B, int Tq, int Tk, int H, int Dh, float scale,
                       int causal, float pdrop, unsigned long long seed, const unsigned long long *seed_dev, int io_dtype, void *stream);
size_t tsasr_attn_f32_bwd_workspace_bytes(int B, int Tq, int Tk, int H, int Dh);
int tsasr_attn_f32_bwd(const void *q, const void *k, const void *v, const long long *strides, const void *pk, const float *bias_u,
                       const float *bias_v, const int32_t *key_lens, const void *out, const void *dout, const float *lse, void *dq, void *dk,
                       void *dv, const long long *dstrides, void *dpk, float *d_bias_u, float *d_bias_v, int B, int Tq, int Tk, int H, int Dh,
                       float scale, int causal, float pdrop, unsigned long long seed, const unsigned long long *seed_dev, int io_dtype,
                       void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * LibriSpeechMix mixture on the device (csrc/dataio.hip): the arithmetic of the reference's `audio_pipeline`
 * (train_librispeechmix_scratch.py:356-386), which the reference runs per utterance in DataLoader workers on the host.
 * src = the utterance's sources back to back (fp32, device); host_off [nsrc+1] (HOST) their element offsets; host_delay [nsrc] (HOST)
 * ceil(delay_j * sample_rate) in samples; rescale != 0 (gain_nontarget != 0): every non-target source is multiplied by
 * sqrt(ratio * mean(target^2) / mean(src_j^2)), ratio = (float)10^(gain_nontarget/10), each operation in fp32 as the reference's 0-dim
 * tensor expression (:361-369; the mean powers are fp64 sums rounded once - the reference's fp32 cascade sum depends on the host's SIMD
 * width); sources are shifted right by their delay, zero-padded to the longest and summed LEFT TO RIGHT in fp32 (:372-377);
 * out [tsasr_mix_sources_out_len(...)] = mixture[start : start + duration] (both in samples; clipped to the mixture as a Python slice).
 * workspace: tsasr_mix_sources_workspace_bytes() (the mean powers), only read when rescale != 0. At most 8 sources.
 * ------------------------------------------------------------------------------------------ */
size_t tsasr_mix_sources_workspace_bytes(void);
long long tsasr_mix_sources_out_len(const long long *host_off, const int *host_delay, int nsrc, long long start, long long duration);
int tsasr_mix_sources(const float *src, const long long *host_off, const int *host_delay, int nsrc, int target, float ratio, int rescale,
                      long long start, long long duration, float *out, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
