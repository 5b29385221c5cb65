// Where the noise kernel's time goes at 3 x 2160 x 3840 (csrc/noise.hip): Philox4x32-10 + one 16-byte store per thread,
// with the rounds or the stores taken out, a grid capped at 2048 / 4096 / 8192 workgroups against one block of four floats per thread, and
// nontemporal stores.  200 back-to-back launches per batch between two events, best and mean of 5 batches.  Self-contained:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/experiments/noise_grid_probe.hip -o tools/experiments/noise_grid_probe
#include <hip/hip_runtime.h>
#include "../../collaborative-distillation_amd/csrc/noise.hip"   // the library's kernel itself, for the last two rows
#include <cstdio>
#include <algorithm>
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct P4 { unsigned v[4]; };
template <int R>
__device__ inline P4 philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (unsigned)p1; c2 = n2; c3 = (unsigned)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return P4{{c0, c1, c2, c3}};
}
// R rounds; STORE 1: normal, 0: store only when an (impossible, data-dependent) condition holds
template <int R, int STORE, int NT>
__global__ __launch_bounds__(256) void k(unsigned k0, unsigned k1, unsigned long long nblk, float* out) {
  const unsigned long long step = (unsigned long long)gridDim.x * 256;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < nblk; i += step) {
    const P4 r = philox<R>((unsigned)i, (unsigned)(i >> 32), 0u, 0u, k0, k1);
    f32x4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (float)(r.v[q] >> 8) * 0x1p-24f;
    f32x4* dst = reinterpret_cast<f32x4*>(out + (i << 2));
    if (STORE || v[0] + v[1] + v[2] + v[3] > 5.f) {
      if (NT) __builtin_nontemporal_store(v, dst); else *dst = v;
    }
  }
}
int main() {
  const unsigned long long total = 3ull * 2160 * 3840, nblk = total / 4;   // multiple of 4: every block is whole, all stores in bounds
  float* buf; if (hipMalloc(&buf, total * 4) != hipSuccess) return 1;
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  auto run = [&](const char* name, auto kern, unsigned blocks) {
    for (int i = 0; i < 20; ++i) hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, 1u, 2u, nblk, buf);
    float best = 1e9, sum = 0;
    for (int b = 0; b < 5; ++b) {
      hipEventRecord(e0, 0);
      for (int i = 0; i < 200; ++i) hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, 1u + i, 2u, nblk, buf);
      hipEventRecord(e1, 0); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1); best = std::min(best, ms / 200); sum += ms / 200;
    }
    printf("%-34s blocks %6u  %.2f us (best of 5 batches), mean %.2f\n", name, blocks, best * 1e3, sum / 5 * 1e3);
    return hipGetLastError() == hipSuccess;
  };
  const unsigned full = (unsigned)((nblk + 255) / 256);
  bool ok = run("10 rounds, store, grid 2048", k<10, 1, 0>, 2048) && run("10 rounds, store, grid 4096", k<10, 1, 0>, 4096) &&
            run("10 rounds, store, grid 8192", k<10, 1, 0>, 8192) && run("10 rounds, store, one block/thread", k<10, 1, 0>, full) &&
            run("10 rounds, NO store, grid 2048", k<10, 0, 0>, 2048) && run("10 rounds, NO store, one block/thr", k<10, 0, 0>, full) &&
            run("0 rounds, store, grid 2048", k<0, 1, 0>, 2048) && run("0 rounds, store, one block/thread", k<0, 1, 0>, full) &&
            run("10 rounds, nontemporal, grid 2048", k<10, 1, 1>, 2048) && run("10 rounds, nontemporal, one blk/thr", k<10, 1, 1>, full);
  // the library's own kernel (alignment test, partial last block, stream id) under both grids
  auto lib = [&](const char* name, unsigned blocks) {
    for (int i = 0; i < 20; ++i) hipLaunchKernelGGL(noise_uniform_kernel, dim3(blocks), dim3(256), 0, 0, 1u, 2u, 0u, total, buf);
    float best = 1e9, sum = 0;
    for (int b = 0; b < 5; ++b) {
      hipEventRecord(e0, 0);
      for (int i = 0; i < 200; ++i) hipLaunchKernelGGL(noise_uniform_kernel, dim3(blocks), dim3(256), 0, 0, 1u + i, 2u, 0u, total, buf);
      hipEventRecord(e1, 0); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1); best = std::min(best, ms / 200); sum += ms / 200;
    }
    printf("%-34s blocks %6u  %.2f us (best of 5 batches), mean %.2f\n", name, blocks, best * 1e3, sum / 5 * 1e3);
  };
  lib("csrc/noise.hip kernel, grid 2048", 2048);
  lib("csrc/noise.hip kernel, one blk/thr", full);
  hipDeviceSynchronize();
  hipFree(buf);
  return ok ? 0 : 2;
}
