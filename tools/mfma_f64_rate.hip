// Issue rate of v_mfma_f64_16x16x4_f64 on the device it runs on (structural regression probes).
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_f64_rate.hip -o tools/mfma_f64_rate && tools/mfma_f64_rate
// Every wave runs ITER rounds of NACC independent accumulator chains; the grid puts `waves` waves on every
// SIMD of every CU.  Prints one line per (NACC, waves per SIMD): time of the best of 5 launches, TFLOP/s
// (2048 FLOP per instruction), and the cycles per instruction per SIMD that this is at the device's
// reported peak clock.
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef double v4d __attribute__((ext_vector_type(4)));
constexpr int ITER = 4096;

template <int NACC>
__global__ __launch_bounds__(256) void rate_kernel(double* out, double a0, double b0) {
  v4d acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
  const double a = a0 + threadIdx.x, b = b0 - threadIdx.x;
  for (int it = 0; it < ITER; ++it) {
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NACC; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  if (s == 12345.678) out[0] = s;  // keeps the chains alive; never true for the inputs below
}

#define CHECK(x)                                                              \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      return 1;                                                               \
    }                                                                         \
  } while (0)

template <int NACC>
int run(int cus, int waves_per_simd, double clock_ghz, double* out) {
  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  const int blocks = cus * waves_per_simd;  // 4 waves per block, one per SIMD
  float best = 1e30f;
  for (int rep = 0; rep < 6; ++rep) {
    CHECK(hipEventRecord(t0));
    hipLaunchKernelGGL(rate_kernel<NACC>, dim3(blocks), dim3(256), 0, 0, out, 0.5, 0.25);
    CHECK(hipEventRecord(t1));
    CHECK(hipEventSynchronize(t1));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    if (rep > 0 && ms < best) best = ms;
  }
  const double n = (double)blocks * 4 * ITER * NACC;  // instructions
  const double per_simd = (double)waves_per_simd * ITER * NACC;
  printf("{\"what\": \"mfma_f64_16x16x4\", \"nacc\": %d, \"waves_per_simd\": %d, \"ms\": %.4f, \"tflops\": %.2f, "
         "\"cycles_per_instr_at_%.2f_ghz\": %.2f}\n",
         NACC, waves_per_simd, best, n * 2048.0 / (best * 1e-3) / 1e12, clock_ghz,
         best * 1e-3 * clock_ghz * 1e9 / per_simd);
  return 0;
}

int main() {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  const double ghz = p.clockRate / 1e6;
  printf("{\"device\": \"%s\", \"cus\": %d, \"clock_ghz\": %.3f}\n", p.gcnArchName, p.multiProcessorCount, ghz);
  double* out;
  CHECK(hipMalloc(&out, 64));
  for (int w = 1; w <= 4; w *= 2) {
    if (run<1>(p.multiProcessorCount, w, ghz, out)) return 1;
    if (run<2>(p.multiProcessorCount, w, ghz, out)) return 1;
    if (run<4>(p.multiProcessorCount, w, ghz, out)) return 1;
  }
  CHECK(hipFree(out));
  return 0;
}
