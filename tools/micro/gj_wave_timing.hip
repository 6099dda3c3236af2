// Micro-benchmark: one super-row elimination of the cyclic reduction (gj_wave, pba_gn_solve_cr.hip) — X = D⁻¹[U | b] by a single
// wave with one lane per column, 4-column pivot blocks — in two forms:
//   lds: the pivot columns published to LDS and read back as broadcasts (pba_gn_solve_cr.hip until round 5);
//   rl : the pivot columns read straight from their owner lanes' registers with v_readlane (uniform values; no LDS,
//        no wave barriers, no pr[24][4] register block).
// 251 workgroups of one wave (the C4 level), M = 24; per-wave cycles (s_memtime) and the launch time by events; the
// two forms' outputs compared.  Diagnostic only: not part of the library.
//   hipcc -O3 --offload-arch=gfx950 -I../../photometric-bundle-adjustment_amd/csrc gj_wave_timing.hip -o gj_wave_timing
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pba_device.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
using pba::rcp_nr;

constexpr int M = 24, PB = 4;

__device__ __forceinline__ void load_cols(const double* D, const double* R1, const double* b, int ncol, int c, double* a) {
  const double* base = D + min(c, M - 1);
  int stride = M;
  bool zero = c >= M + ncol;
  if (c >= M && c < 2 * M) {
    base = R1 + (c - M);
  } else if (c >= 2 * M && c < M + ncol) {
    base = b;
    stride = 1;
  }
#pragma unroll
  for (int r = 0; r < M; ++r) a[r] = base[r * stride];
#pragma unroll
  for (int r = 0; r < M; ++r) a[r] = zero ? 0.0 : a[r];
}

__device__ __forceinline__ bool solve_pivot(double (&P)[PB][PB], double (&t)[PB]) {
  bool bad = false;
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    bad |= !(P[i][i] > 0.0);
    const double inv = rcp_nr(P[i][i]);
#pragma unroll
    for (int j = i + 1; j < PB; ++j) P[i][j] *= inv;
    t[i] *= inv;
#pragma unroll
    for (int q = 0; q < PB; ++q) {
      if (q == i) continue;
      const double f = P[q][i];
#pragma unroll
      for (int j = i + 1; j < PB; ++j) P[q][j] -= f * P[i][j];
      t[q] -= f * t[i];
    }
  }
  return bad;
}

// the round-5 form (pba_gn_solve_cr.hip gj_wave)
__device__ __forceinline__ bool gj_lds(int c, double* piv, double* a) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < M; k += PB) {
    if (c >= k && c < k + PB) {
      double* dst = piv + (c - k);
#pragma unroll
      for (int r = 0; r < M; ++r) dst[PB * r] = a[r];
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    double pr[M][PB];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const int r = (i + k) % M;
#pragma unroll
      for (int j = 0; j < PB; ++j) pr[r][j] = piv[PB * r + j];
    }
    double P[PB][PB], t[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
#pragma unroll
      for (int j = 0; j < PB; ++j) P[i][j] = pr[k + i][j];
      t[i] = a[k + i];
    }
    bad |= solve_pivot(P, t);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      if (r >= k && r < k + PB) {
        a[r] = t[r - k];
      } else {
        double v = a[r];
#pragma unroll
        for (int j = 0; j < PB; ++j) v -= pr[r][j] * t[j];
        a[r] = v;
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
  }
  return !bad;
}

__device__ __forceinline__ double readlane_d(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// pivot columns from their owner lanes' registers
__device__ __forceinline__ bool gj_rl(int c, double* a) {
  bool bad = false;
#pragma unroll
  for (int k = 0; k < M; k += PB) {
    double P[PB][PB], t[PB];
#pragma unroll
    for (int i = 0; i < PB; ++i) {
#pragma unroll
      for (int j = 0; j < PB; ++j) P[i][j] = readlane_d(a[k + i], k + j);
      t[i] = a[k + i];
    }
    bad |= solve_pivot(P, t);
#pragma unroll
    for (int r = 0; r < M; ++r) {
      if (r >= k && r < k + PB) continue;
      double v = a[r];
#pragma unroll
      for (int j = 0; j < PB; ++j) v -= readlane_d(a[r], k + j) * t[j];
      a[r] = v;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) a[k + i] = t[i];
  }
  return !bad;
}

template <int FORM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void gj_kernel(
    const double* D, const double* U, const double* b, double* out, long long* cyc, int* status) {
  __shared__ __attribute__((aligned(16))) double piv[M * PB];
  const int i = blockIdx.x, c = threadIdx.x;
  double a[M];
  load_cols(D + (long long)i * M * M, U + (long long)i * M * M, b + (long long)i * M, M + 1, c, a);
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < M; ++r) s += a[r];
  if (s == 12345.678) a[0] = 1.0;  // the loads have landed before the first stamp
  const long long t0 = clock64();
  const bool ok = FORM == 0 ? gj_lds(c, piv, a) : gj_rl(c, a);
  double z = 0.0;
#pragma unroll
  for (int r = 0; r < M; ++r) z += a[r];
  if (z == 12345.678) a[1] = 2.0;
  const long long t1 = clock64();
  if (!ok && c == 0) atomicOr(status, 1);
#pragma unroll
  for (int r = 0; r < M; ++r) out[((long long)i * M + r) * 64 + c] = a[r];
  if (c == 0) cyc[i] = t1 - t0;
}

int main() {
  const int n = 251;
  std::vector<double> D((size_t)n * M * M), U((size_t)n * M * M), b((size_t)n * M);
  srand(7);
  auto rnd = [] { return (double)rand() / RAND_MAX - 0.5; };
  for (int i = 0; i < n; ++i) {
    std::vector<double> A((size_t)M * M);
    for (auto& x : A) x = rnd();
    for (int r = 0; r < M; ++r)
      for (int cc = 0; cc < M; ++cc) {
        double v = 0.0;
        for (int q = 0; q < M; ++q) v += A[r * M + q] * A[cc * M + q];
        D[(size_t)i * M * M + r * M + cc] = v + (r == cc ? 1.0 : 0.0);
      }
    for (int e = 0; e < M * M; ++e) U[(size_t)i * M * M + e] = rnd();
    for (int r = 0; r < M; ++r) b[(size_t)i * M + r] = rnd();
  }
  double *dD, *dU, *db, *o0, *o1;
  long long* cyc;
  int* st;
  CK(hipMalloc(&dD, D.size() * 8)); CK(hipMalloc(&dU, U.size() * 8)); CK(hipMalloc(&db, b.size() * 8));
  CK(hipMalloc(&o0, (size_t)n * M * 64 * 8)); CK(hipMalloc(&o1, (size_t)n * M * 64 * 8));
  CK(hipMalloc(&cyc, n * 8)); CK(hipMalloc(&st, 4));
  CK(hipMemcpy(dD, D.data(), D.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(dU, U.data(), U.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(db, b.data(), b.size() * 8, hipMemcpyHostToDevice));
  CK(hipMemset(st, 0, 4));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int form = 0; form < 2; ++form) {
    auto launch = [&] {
      if (form == 0) gj_kernel<0><<<n, 64>>>(dD, dU, db, o0, cyc, st);
      else gj_kernel<1><<<n, 64>>>(dD, dU, db, o1, cyc, st);
    };
    for (int r = 0; r < 200; ++r) launch();
    CK(hipEventRecord(e0));
    for (int r = 0; r < 200; ++r) launch();
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<long long> c(n);
    CK(hipMemcpy(c.data(), cyc, n * 8, hipMemcpyDeviceToHost));
    std::sort(c.begin(), c.end());
    printf("%s: launch %.2f us, elimination cycles median %lld max %lld (%.2f us at 2.4 GHz)\n", form ? "rl " : "lds",
           1e3 * ms / 200, c[n / 2], c[n - 1], c[n / 2] / 2400.0);
  }
  std::vector<double> a0((size_t)n * M * 64), a1(a0.size());
  CK(hipMemcpy(a0.data(), o0, a0.size() * 8, hipMemcpyDeviceToHost));
  CK(hipMemcpy(a1.data(), o1, a1.size() * 8, hipMemcpyDeviceToHost));
  double md = 0, mx = 0;
  for (size_t q = 0; q < a0.size(); ++q) {
    if ((q % 64) >= 2 * M + 1) continue;
    md = std::max(md, std::fabs(a0[q] - a1[q]));
    mx = std::max(mx, std::fabs(a0[q]));
  }
  int h = 0;
  CK(hipMemcpy(&h, st, 4, hipMemcpyDeviceToHost));
  printf("max |lds - rl| %.3e of max %.3e; status %d\n", md, mx, h);
  return 0;
}
