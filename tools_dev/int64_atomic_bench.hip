// Rate of global 64-bit integer atomics against fp32 atomics on gfx950 -- the number that decides what the
// fixed-point splats of deterministic mode cost.  Three address patterns:
//   stream    every lane its own consecutive element (the best case: coalesced, no collisions)
//   scatter   a pseudo-random element of a 16 M element plane per lane (a splat onto a large image)
//   collide   64 lanes on 4 neighbouring elements, all waves inside one 64 x 64 canvas (an object canvas warped into a
//             frame: the pattern grid_sample2d's backward is bound by)
//   hipcc --offload-arch=gfx950 -O3 tools_dev/int64_atomic_bench.hip -o tools_dev/int64_atomic_bench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      std::printf("%s failed: %s\n", #x, hipGetErrorString(e_));                   \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

constexpr size_t kElems = (size_t)1 << 24;
constexpr int kBlock = 256, kBlocks = 16384, kPerThread = 16;

__device__ __forceinline__ size_t address(int pattern, size_t i) {
  if (pattern == 0) return i & (kElems - 1);
  if (pattern == 1) return (i * 2654435761ull >> 7) & (kElems - 1);
  return ((i >> 6) * 2654435761ull >> 9 & 4095) / 4 * 4 + (i & 3);  // a 4096-element canvas, 4 targets per wave
}

template <typename T>
__global__ __launch_bounds__(kBlock) void add_kernel(T* dst, int pattern, T v) {
  const size_t base = ((size_t)blockIdx.x * kPerThread) * kBlock + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) atomicAdd(dst + address(pattern, base + (size_t)k * kBlock), v);
}

template <typename T>
float time_ms(T* dst, int pattern, T v) {
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(add_kernel<T>, dim3(kBlocks), dim3(kBlock), 0, 0, dst, pattern, v);
  CHECK(hipEventRecord(a));
  const int reps = 10;
  for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(add_kernel<T>, dim3(kBlocks), dim3(kBlock), 0, 0, dst, pattern, v);
  CHECK(hipEventRecord(b));
  CHECK(hipEventSynchronize(b));
  float ms = 0.0f;
  CHECK(hipEventElapsedTime(&ms, a, b));
  return ms / reps;
}

int main() {
  float* f = nullptr;
  unsigned long long* u = nullptr;
  CHECK(hipMalloc(&f, kElems * sizeof(float)));
  CHECK(hipMalloc(&u, kElems * sizeof(unsigned long long)));
  CHECK(hipMemset(f, 0, kElems * sizeof(float)));
  CHECK(hipMemset(u, 0, kElems * sizeof(unsigned long long)));
  const double n = (double)kBlocks * kBlock * kPerThread;
  const char* names[3] = {"stream", "scatter", "collide"};
  std::printf("%.0f atomics per launch, mean of 10 launches\n", n);
  std::printf("%-8s %14s %14s %8s\n", "pattern", "f32 Gatomic/s", "u64 Gatomic/s", "u64/f32");
  for (int p = 0; p < 3; ++p) {
    const float tf = time_ms<float>(f, p, 1.0f), tu = time_ms<unsigned long long>(u, p, 1ull);
    std::printf("%-8s %14.2f %14.2f %8.2f   (%.3f ms, %.3f ms; %.0f / %.0f GB/s of added bytes)\n", names[p],
                n / tf * 1e-6, n / tu * 1e-6, tf / tu, tf, tu, n * 4 / tf * 1e-6, n * 8 / tu * 1e-6);
  }
  CHECK(hipFree(f));
  CHECK(hipFree(u));
  return 0;
}
