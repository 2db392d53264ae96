// Error reporting, version and the test-only debug options of the C ABI (include/waldo_hip.h).
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

#include "waldo_common.hip.h"

namespace waldo {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return WALDO_ELAUNCH;
  }
  return WALDO_OK;
}

__global__ __launch_bounds__(kBlock) void fill_words_kernel(unsigned* __restrict__ dst, unsigned word, size_t n) {
  const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) * 4;
  if (i + 3 < n && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    *reinterpret_cast<uint4*>(dst + i) = make_uint4(word, word, word, word);
  } else {
    for (size_t k = i; k < n && k < i + 4; ++k) dst[k] = word;
  }
}

__global__ __launch_bounds__(kBlock) void copy_bytes_kernel(unsigned char* __restrict__ dst,
                                                            const unsigned char* __restrict__ src, size_t n) {
  const size_t i = ((size_t)blockIdx.x * kBlock + threadIdx.x) * 16;
  const bool wide = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
  if (i + 15 < n && wide) {
    *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
  } else {
    for (size_t k = i; k < n && k < i + 16; ++k) dst[k] = src[k];
  }
}

void fill_words(void* dst, unsigned word, size_t bytes, hipStream_t st) {
  const size_t n = bytes / 4;
  if (n == 0) return;
  hipLaunchKernelGGL(fill_words_kernel, dim3((unsigned)((n + 4 * kBlock - 1) / (4 * kBlock))), dim3(kBlock), 0, st,
                     reinterpret_cast<unsigned*>(dst), word, n);
}

void copy_bytes(void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (bytes == 0) return;
  hipLaunchKernelGGL(copy_bytes_kernel, dim3((unsigned)((bytes + 16 * kBlock - 1) / (16 * kBlock))), dim3(kBlock), 0, st,
                     reinterpret_cast<unsigned char*>(dst), reinterpret_cast<const unsigned char*>(src), bytes);
}

static std::atomic<int> g_debug[WALDO_DEBUG_COUNT];

bool debug_option(int option) {
  return option >= 0 && option < WALDO_DEBUG_COUNT && g_debug[option].load(std::memory_order_relaxed) != 0;
}

}  // namespace waldo

extern "C" int waldo_version(void) { return 1020; }

extern "C" int waldo_set_debug_option(int option, int value) {
  if (option < 0 || option >= WALDO_DEBUG_COUNT) {
    waldo::set_error("waldo_set_debug_option: unknown option %d", option);
    return WALDO_EINVAL;
  }
  waldo::g_debug[option].store(value, std::memory_order_relaxed);
  return WALDO_OK;
}

extern "C" int waldo_host_device_pointer(void* host, void** device) {
  if (!host || !device) {
    waldo::set_error("waldo_host_device_pointer: null pointer");
    return WALDO_EINVAL;
  }
  void* dev = nullptr;
  const hipError_t e = hipHostGetDevicePointer(&dev, host, 0);
  if (e != hipSuccess || dev == nullptr) {
    (void)hipGetLastError();  // (the failed query must not show up as the next launch's status)
    waldo::set_error("waldo_host_device_pointer: %p is not pinned, mapped host memory (%s)", host, hipGetErrorString(e));
    return WALDO_EINVAL;
  }
  *device = dev;
  return WALDO_OK;
}

extern "C" const char* waldo_last_error_string(void) { return waldo::g_err; }
