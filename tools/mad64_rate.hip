// Register-only rate of the 32 x 32 + 64-bit integer multiply-add (v_mad_i64_i32) on the device, the instruction pca_scatter_kernel is
// made of:  hipcc --offload-arch=gfx950 -O3 tools/mad64_rate.hip -o tools/mad64_rate && tools/mad64_rate
// Every lane keeps a 4 x 4 block of int64 accumulators and feeds it from eight registers that change every round, as the kernel does
// with its LDS reads; nothing is loaded or stored inside the loop.  Prints multiply-adds per second over the whole chip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

__global__ __launch_bounds__(256) void mad64_kernel(long long* out, int rounds, int seed) {
  long long acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;
  int a[4], b[4];
  for (int i = 0; i < 4; ++i) a[i] = seed + threadIdx.x * 7 + i, b[i] = seed * 3 + blockIdx.x + i * 5;
  for (int r = 0; r < rounds; ++r) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] += (long long)a[i] * (long long)b[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] += 3, b[i] -= 5;
  }
  long long s = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) s ^= acc[i][j];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

#define CHECK(x)                                                         \
  do {                                                                   \
    hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                              \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));       \
      return 1;                                                          \
    }                                                                    \
  } while (0)

int main() {
  const int blocks = 256 * 8, rounds = 1 << 14;
  long long* out = nullptr;
  CHECK(hipMalloc(&out, (size_t)blocks * 256 * 8));
  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  double best = 0;
  for (int rep = 0; rep < 5; ++rep) {  // (the first is the warm-up)
    CHECK(hipEventRecord(t0));
    hipLaunchKernelGGL(mad64_kernel, dim3(blocks), dim3(256), 0, 0, out, rounds, rep + 1);
    CHECK(hipGetLastError());
    CHECK(hipEventRecord(t1));
    CHECK(hipEventSynchronize(t1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    const double rate = 16.0 * rounds * blocks * 256 / (ms * 1e-3);
    if (rep > 0 && rate > best) best = rate;
    std::printf("run %d: %.3f ms, %.3f T multiply-adds / s\n", rep, ms, rate / 1e12);
  }
  std::printf("mad64_rate %.6e\n", best);
  CHECK(hipFree(out));
  return 0;
}
