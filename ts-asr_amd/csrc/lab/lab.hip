// libtsasr_lab.so: lab equipment (include/tsasr_lab.h) - LDS / memory fills, a wall-clock stamp and the d(pk) pass of the attention
// backward on caller-supplied tensors. Not linked into the product library.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "../../../include/tsasr_lab.h"
#include "../dpk_pass.h"

__global__ __launch_bounds__(256) void lab_fill_lds_kernel(unsigned pattern, int words, unsigned *sink) {
    extern __shared__ unsigned fill_lds[];
    for (int i = threadIdx.x; i < words; i += 256) fill_lds[i] = pattern;
    __syncthreads();
    if (sink && fill_lds[(threadIdx.x * 97) % words] != pattern) *sink = 1;   // keeps the stores alive
}

__global__ void lab_fill_words_kernel(unsigned *p, unsigned pattern, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = pattern;
}

__global__ void lab_stamp_kernel(unsigned long long *out) { *out = __builtin_amdgcn_s_memrealtime(); }

// the two bodies of csrc/dpk_pass.h, launched as csrc/attention.hip launches them stand-alone
__global__ __launch_bounds__(256) void lab_dpk_kernel(const bf16_t *__restrict__ ds, const bf16_t *__restrict__ qv, const int32_t *__restrict__ key_lens,
                                                      float *__restrict__ part, int Bn, int Tn, int Tp, int H, int causal, int bgroup) {
    dpk_body<bf16_t>(ds, qv, key_lens, part, Bn, Tn, Tp, H, 64, causal, bgroup, 1, Tp, blockIdx.x, blockIdx.y, blockIdx.z);
}
__global__ __launch_bounds__(DPO_TH, 4) void lab_dpk_once_kernel(const bf16_t *__restrict__ ds, const bf16_t *__restrict__ qv,
                                                                 const int32_t *__restrict__ key_lens, float *__restrict__ part, int Bn, int Tn, int Tp,
                                                                 int H, int causal, int bgroup) {
    dpk_once_body(ds, qv, key_lens, part, Bn, Tn, Tp, H, causal, bgroup, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void lab_dpk_reduce_kernel(const float *__restrict__ part, bf16_t *__restrict__ dpk, int R, int H, int G) {
    dpk_reduce_body<bf16_t>(part, dpk, R, H, 64, G, blockIdx.x, gridDim.x);
}

static int launched(void) { return hipGetLastError() == hipSuccess ? 0 : -2; }

extern "C" {

int tsasr_lab_fill_lds(unsigned pattern, void *stream) {
    const int bytes = 160 * 1024;
    (void)hipFuncSetAttribute((const void *)lab_fill_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    lab_fill_lds_kernel<<<4 * cus, 256, bytes, (hipStream_t)stream>>>(pattern, bytes / 4, nullptr);
    return launched();
}

int tsasr_lab_fill(void *p, unsigned pattern, size_t nwords, void *stream) {
    if (!p || ((uintptr_t)p & 3)) return -1;
    if (nwords == 0) return 0;
    lab_fill_words_kernel<<<(unsigned)std::min<size_t>(4096, (nwords + 255) / 256), 256, 0, (hipStream_t)stream>>>((unsigned *)p, pattern, nwords);
    return launched();
}

int tsasr_lab_stamp(void *out, void *stream) {
    if (!out || ((uintptr_t)out & 7)) return -1;
    lab_stamp_kernel<<<1, 1, 0, (hipStream_t)stream>>>((unsigned long long *)out);
    return launched();
}

size_t tsasr_lab_dpk_part_bytes(int B, int T, int H) {
    if (B < 1 || H < 1 || !dpk_once_shape(T)) return 0;
    return (size_t)cdiv(B, dpk_bgroup(B, T)) * (2 * T - 1) * H * 64 * sizeof(float);
}

int tsasr_lab_dpk(int body, const void *ds, const void *qv, const int *key_lens, void *part, void *dpk, int B, int T, int H, int causal, void *stream) {
    if (!ds || !qv || !part || !dpk || B < 1 || H < 1 || !dpk_once_shape(T) || causal < 0 || (body != 0 && body != 1)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int Tp = cdiv(T, 64) * 64, R = 2 * T - 1, bg = dpk_bgroup(B, T), G = cdiv(B, bg);
    if (body == 1)
        lab_dpk_once_kernel<<<dim3(H, G), DPO_TH, 0, st>>>((const bf16_t *)ds, (const bf16_t *)qv, key_lens, (float *)part, B, T, Tp, H, causal, bg);
    else
        lab_dpk_kernel<<<dim3(cdiv(R, 64), H, G), 256, 0, st>>>((const bf16_t *)ds, (const bf16_t *)qv, key_lens, (float *)part, B, T, Tp, H, causal, bg);
    lab_dpk_reduce_kernel<<<std::min(1024, cdiv(R * H * 64, 256)), 256, 0, st>>>((const float *)part, (bf16_t *)dpk, R, H, G);
    return launched();
}

}  // extern "C"
