/* libtsasr_lab.so - LAB EQUIPMENT, not part of the product ABI (include/tsasr_hip.h): aids that tests / tools use to stress, time or
 * take apart the product library from the outside. Built by `make -C ts-asr_amd/csrc` next to the product library, loaded only by
 * tests/helpers/, tools/ and ts-asr_amd/prof.py's TSASR_STAMPS mode (ts-asr_amd/_capi.py::lab()). Nothing here computes anything of the
 * training step (tsasr_lab_dpk runs one of its passes on tensors of the caller's). */
#ifndef TSASR_LAB_H
#define TSASR_LAB_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
/* overwrite the whole LDS of every CU with a 32-bit pattern: a kernel that reads LDS it never wrote then sees the pattern, not leftovers
 * (tests/helpers/lds_garbage.py) */
int tsasr_lab_fill_lds(unsigned pattern, void *stream);
/* nwords 32-bit words at p <- pattern (poisoning the captured step's free pool memory between replays: tools/det_stress.py) */
int tsasr_lab_fill(void *p, unsigned pattern, size_t nwords, void *stream);
/* *out (uint64, device) = the device wall clock (100 MHz ticks) when a one-thread kernel reaches the head of `stream`
 * (tools/step_stamps.py: phase stamps inside an unprofiled replay of the captured step) */
int tsasr_lab_stamp(void *out, void *stream);
/* The d(pk) pass of the relative-position attention backward (csrc/dpk_pass.h) on the caller's tensors, bf16, Dh = 64, 2 <= T <= 256:
 * dpk [2T-1, H*64] bf16 = sum_b sum_i ds[b][h][i][j = r + i - (T-1)] * qv[h][b*T + i][:], keys j < key_lens[b] (NULL: T) and inside the
 * look-ahead limit only (causal as in tsasr_relpos_attn_bwd). ds: bf16 [B, H, T, Tp], Tp = T rounded up to 64 (what lies beyond the valid
 * keys is never used); qv: bf16 [H, B*T, 64]; part: tsasr_lab_dpk_part_bytes(B, T, H) bytes, on return the fp32 partial planes
 * [groups][2T-1][H*64] that the reduction summed. body 0: dpk_body (one workgroup per 64 band rows, head and utterance group),
 * body 1: dpk_once_body (reads ds once). Both launched as the product launches them stand-alone, followed by the product's reduction. */
size_t tsasr_lab_dpk_part_bytes(int B, int T, int H);
int tsasr_lab_dpk(int body, const void *ds, const void *qv, const int *key_lens, void *part, void *dpk, int B, int T, int H, int causal, void *stream);
#ifdef __cplusplus
}
#endif
#endif
