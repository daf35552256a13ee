// Dev tool: does k_slam's in-register 16 x 16 inversion slow down when the other waves of the workgroup run LDS traffic /
// fp64 MFMAs (as the U phase does)?  mode 0: alone, 1: others do LDS b128 reads, 2: others do fp64 MFMAs, 3: both.
#include "../../drl_graph_exploration_amd/csrc/k_sweep_ws.hip"  // inv16; brings k_sweep.hip (inv16_blk) with it
#include <cstdio>
#include <vector>
using namespace kslam;

__global__ __launch_bounds__(512) void k(const double *Din, double *Eout, long long *cyc, int mode, int partner_only) {
  __shared__ int bad[2];
  __shared__ double buf[4096];
  __shared__ int stop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) stop = 0;
  for (int i = tid; i < 4096; i += 512) buf[i] = i * 1e-3;
  __syncthreads();
  if (wave == 0) {
    SweepCtx x{0, lane, lane & 15, lane >> 4, 16, 16, true, true, bad, nullptr};
    v4d d;
    for (int r = 0; r < 4; ++r) d[r] = Din[(x.lr + 4 * r) * 16 + x.lc];
    __builtin_amdgcn_s_waitcnt(0);
    long long t0 = clock64();
    inv16(x, 0, d);
    long long t1 = clock64() + (d[0] == 1.2345e300 ? 1 : 0);
    for (int r = 0; r < 4; ++r) Eout[(x.lr + 4 * r) * 16 + x.lc] = d[r];
    if (lane == 0) { cyc[0] = t1 - t0; atomicExch(&stop, 1); }
  } else if (!partner_only || wave == 4) {
    v4d c = {0, 0, 0, 0};
    double acc = 0;
    volatile int *vs = &stop;
    int it = 0;
    while (!*vs && it < 100000) {
      ++it;
      if (mode & 1) {
        for (int k = 0; k < 8; ++k) {
          const double2 v = *reinterpret_cast<const double2 *>(&buf[((tid * 2 + k * 257 + it) & 2047) * 2]);
          acc += v.x + v.y;
        }
      }
      if (mode & 2) {
        for (int k = 0; k < 4; ++k) c = __builtin_amdgcn_mfma_f64_16x16x4f64(acc + 1.0, 2.0, c, 0, 0, 0);
      }
    }
    if (acc + c[0] == 1.2345e300) Eout[0] = acc;
  }
}

int main() {
  const int n = 16;
  std::vector<double> D(n * n, 0.0), B(n * n);
  srand(1);
  for (auto &v : B) v = rand() / (double)RAND_MAX - 0.5;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0;
      for (int k = 0; k < n; ++k) s += B[i * n + k] * B[j * n + k];
      D[i * n + j] = s + (i == j ? 1.0 : 0.0);
    }
  double *dD, *dE; long long *dc;
  hipMalloc(&dD, n * n * 8); hipMalloc(&dE, n * n * 8); hipMalloc(&dc, 8);
  hipMemcpy(dD, D.data(), n * n * 8, hipMemcpyHostToDevice);
  for (int partner = 0; partner < 2; ++partner)
    for (int mode = 0; mode < 4; ++mode) {
      long long best = 1ll << 60, c;
      for (int rep = 0; rep < 5; ++rep) {
        hipLaunchKernelGGL(k, dim3(1), dim3(512), 0, 0, dD, dE, dc, mode, partner);
        hipDeviceSynchronize();
        hipMemcpy(&c, dc, 8, hipMemcpyDeviceToHost);
        if (c < best) best = c;
      }
      printf("%s mode %d (1 = LDS reads, 2 = fp64 MFMA): inv16 %lld cycles\n", partner ? "same-SIMD partner only" : "7 other waves", mode, best);
    }
  return 0;
}
