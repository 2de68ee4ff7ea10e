// Where the one-workgroup rotational histogram (cartographer_amd/csrc/histogram_batch_device.h)
// spends its time: one workgroup on a cloud of 64, 700 and 4000 points (normal, sigma 8 m in x and
// y, 1.6 m in z: many short slices, `last` moves at almost every point), thread 0 stamps the
// 100 MHz wall clock at the hook between the steps.  Prints microseconds since the first stamp:
//   1 keys built   2 sorted by slice   3 slices known   4 first centroids   5 angle keys built
//   6 sorted by angle   7 coordinates in angle order   8 second centroids   9 walked
//   10 votes and their keys   11 sorted by bucket   12 votes in bucket order   13 histogram written
// Build: hipcc --offload-arch=gfx950 -O3 tools/probes/histogram_phases.hip -o tools/bin/histogram_phases
#include <hip/hip_runtime.h>

#include <cstdio>
#include <random>
#include <vector>

__device__ unsigned long long g_stamps[16];
#define CMX_HISTOGRAM_STAMP(k)                             \
  do {                                                     \
    if (threadIdx.x == 0) g_stamps[k] = wall_clock64();    \
  } while (0)
#include "../../cartographer_amd/csrc/histogram_batch_device.h"

__global__ void __launch_bounds__(cmx::kSmallThreads)
Probe(const float* xyz, int n, int N, float min_sq, float max_sq, float* histogram) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cmx::HistogramWorkgroup(smem, xyz, n, N, 120, min_sq, max_sq, histogram);
}

#define CHECK(expr)                                                    \
  do {                                                                 \
    const hipError_t e = (expr);                                       \
    if (e != hipSuccess) {                                             \
      std::printf("%s: %s\n", #expr, hipGetErrorString(e));            \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Probe),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256));
  for (int n : {64, 700, 4000}) {
    std::mt19937 rng(n);
    std::normal_distribution<float> normal(0.f, 8.f);
    std::vector<float> cloud(3 * n);
    for (int i = 0; i < n; ++i) {
      cloud[3 * i] = normal(rng);
      cloud[3 * i + 1] = normal(rng);
      cloud[3 * i + 2] = 0.2f * normal(rng);
    }
    float *d_cloud = nullptr, *d_histogram = nullptr;
    CHECK(hipMalloc(&d_cloud, 12 * n));
    CHECK(hipMalloc(&d_histogram, 4 * 120));
    CHECK(hipMemcpy(d_cloud, cloud.data(), 12 * n, hipMemcpyHostToDevice));
    const int N = cmx::HistogramN(n);
    for (int rep = 0; rep < 3; ++rep) {
      Probe<<<1, cmx::kSmallThreads, cmx::HistogramLdsBytes(N)>>>(
          d_cloud, n, N, cmx::HistogramMinDistanceSq(), cmx::HistogramMaxDistanceSq(), d_histogram);
      CHECK(hipDeviceSynchronize());
    }
    unsigned long long stamps[16];
    CHECK(hipMemcpyFromSymbol(stamps, HIP_SYMBOL(g_stamps), sizeof(stamps)));
    std::printf("n=%d N=%d us since the first stamp:", n, N);
    for (int k = 1; k <= 13; ++k) std::printf(" %d:%.1f", k, (stamps[k] - stamps[0]) / 100.0);
    std::printf("\n");
    CHECK(hipFree(d_cloud));
    CHECK(hipFree(d_histogram));
  }
  return 0;
}
