// mfma_i8_map.hip — the operand and accumulator lane maps of v_mfma_i32_32x32x32_i8 on gfx950, checked with exact integer data
// (the guide gives the maps for the bf16 forms only).  Claim under test (what pq_gqa.hip relies on):
//   A: lane l holds row l & 31, k-bytes 16 (l >> 5) .. + 16 (byte t of the 4 dwords = k 16 (l >> 5) + t); B: the same with columns;
//   C: register r of lane l = row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
// Random int8 A [32][32], B [32][32]; C = A B^T against the host's int32 sum.  Prints "i8 map OK" or the first mismatch.
//   hipcc --offload-arch=gfx950 -O2 -o tools/mb/mfma_i8_map tools/mb/mfma_i8_map.hip && tools/mb/mfma_i8_map
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

__global__ void probe(const signed char* A, const signed char* B, int* C) {
  const int l = threadIdx.x, idx = l & 31, hi = l >> 5;
  const i32x4 a = *reinterpret_cast<const i32x4*>(A + idx * 32 + 16 * hi);
  const i32x4 b = *reinterpret_cast<const i32x4*>(B + idx * 32 + 16 * hi);
  i32x16 c;
  for (int r = 0; r < 16; ++r) c[r] = 0;
  c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
  for (int r = 0; r < 16; ++r) C[((r & 3) + 8 * (r >> 2) + 4 * hi) * 32 + idx] = c[r];
}

int main() {
  signed char hA[1024], hB[1024];
  int hC[1024];
  srand(7);
  for (int i = 0; i < 1024; ++i) { hA[i] = (signed char)(rand() % 256 - 128); hB[i] = (signed char)(rand() % 255 - 127); }
  signed char *dA, *dB;
  int* dC;
  if (hipMalloc(&dA, 1024) != hipSuccess || hipMalloc(&dB, 1024) != hipSuccess || hipMalloc(&dC, 4096) != hipSuccess) return 2;
  hipMemcpy(dA, hA, 1024, hipMemcpyHostToDevice);
  hipMemcpy(dB, hB, 1024, hipMemcpyHostToDevice);
  hipMemset(dC, 0xFF, 4096);
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dC);
  if (hipMemcpy(hC, dC, 4096, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  for (int m = 0; m < 32; ++m)
    for (int n = 0; n < 32; ++n) {
      int want = 0;
      for (int k = 0; k < 32; ++k) want += (int)hA[m * 32 + k] * (int)hB[n * 32 + k];
      if (hC[m * 32 + n] != want) { printf("i8 map MISMATCH at row %d col %d: got %d want %d\n", m, n, hC[m * 32 + n], want); return 1; }
    }
  printf("i8 map OK\n");
  return 0;
}
