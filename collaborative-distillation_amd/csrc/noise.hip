// Seeded uniform noise on the device: the content image of texture synthesis (PytorchWCT/data_loader.py:74 intends
// torch.rand_like of the texture), made where the cascade reads it instead of on the host (a 4K fp32 image is 99.5 MB).
//
// The values are a function of (seed, stream_id, position) alone -- never of the launch geometry, the library version or torch's
// generator -- so that a C host, the Python binding and a 30-line numpy oracle (tests/synth_oracle.py) agree bit for bit:
//   generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123)
//   key         (seed & 0xffffffff, seed >> 32)
//   counter     (i & 0xffffffff, i >> 32, stream_id, 0) for block i = e >> 2 of the flat element index e = c H W + y W + x
//   element e   output word e & 3 of its block;  value = float(word >> 8) * 2^-24 -- exact in fp32, in [0, 1 - 2^-24] like torch.rand
// A thread produces whole blocks: four consecutive floats, one 16-byte store where the destination is 16-byte aligned (a view
// into a larger buffer need not be), four 4-byte stores otherwise; the last block of an image whose 3 H W is not a multiple of 4 is
// partial.  20 32 x 32 -> 64-bit multiplies per 16 bytes stored: the arithmetic hides behind the stores (see launch_noise_uniform).
#include "wct_common.h"
#include "philox_dev.h"
#include <algorithm>

namespace {

// grid-stride over the blocks of four elements; `total` = 3 H W
__global__ __launch_bounds__(256) void noise_uniform_kernel(unsigned k0, unsigned k1, unsigned stream_id, unsigned long long total, float* out) {
  const unsigned long long nblk = (total + 3) >> 2, step = (unsigned long long)gridDim.x * 256;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < nblk; i += step) {
    const Philox4 r = philox4x32_10((unsigned)i, (unsigned)(i >> 32), stream_id, 0u, k0, k1);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)(r.v[k] >> 8) * 0x1p-24f;
    const unsigned long long e = i << 2;
    float* dst = out + e;
    if (e + 4 <= total) {
      if ((reinterpret_cast<size_t>(dst) & 15) == 0) *reinterpret_cast<f32x4*>(dst) = v;
      else { dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
    } else {
      const int n = (int)(total - e);   // 1 .. 3
      for (int k = 0; k < n; ++k) dst[k] = v[k];
    }
  }
}

}  // namespace

hipError_t launch_noise_uniform(unsigned long long seed, unsigned stream_id, int H, int W, float* planar, hipStream_t s) {
  if (H < 1 || W < 1 || !planar) return hipErrorInvalidValue;
  const unsigned long long total = 3ull * (unsigned long long)H * (unsigned long long)W, nblk = (total + 3) >> 2;
  // one block of four floats per thread, the grid stride only beyond 2^30 threads.  Measured at 3 x 2160 x 3840
  // (tools/experiments/noise_grid_probe.hip, profiles/synthesis_noise_4k.json), back-to-back launches: 17.3 - 17.7 us this way
  // against 18.2 - 18.6 us from a grid capped at 2048 workgroups.  The generator alone takes 13 us and the stores alone 16 us (16.4 - 17.6 us
  // from the capped grid: the cap costs a pure store kernel too), so most of the arithmetic hides behind the stores.
  const unsigned blocks = (unsigned)std::min<unsigned long long>((nblk + 255) / 256, 1ull << 22);
  hipLaunchKernelGGL(noise_uniform_kernel, dim3(blocks), dim3(256), 0, s, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), stream_id, total,
                     planar);
  return hipGetLastError();
}
