// pba_gn_solve_sky.hip — the direct solvers of a Gauss-Newton trial's reduced camera system (pba_gn.hip): block Cholesky
// over a skyline profile through global memory (skyline_solve_kernel) or with the active front in LDS
// (front_solve_kernel), and over a band with the window in LDS (band_solve_kernel).
//
// Replaces the reduced camera system's Cholesky of SPARSE_SCHUR (schur_complement_solver.cc:138-146).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pba_gn_solve.h"

using namespace pba;
using namespace pba::detail;

namespace {

// ------------------------------------------------------------------------------------------------
// skyline_solve_kernel: S δ = −g, S = LLᵀ in place (block skyline, right-looking), one workgroup
// ------------------------------------------------------------------------------------------------
// chol6 / inv_lower6: the 6×6 diagonal block's Cholesky factor and its inverse, on register arrays (fully unrolled)
__device__ __forceinline__ bool chol6_reg(const double (&A)[36], double (&L)[36]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 36; ++i) L[i] = 0.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
    ok = ok && s > 0.0;
    const double ljj = sqrt(fmax(s, 1e-300));
    L[j * 6 + j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = t / ljj;
    }
  }
  return ok;
}
__device__ __forceinline__ void inv_lower6_reg(const double (&L)[36], double (&Li)[36]) {
#pragma unroll
  for (int i = 0; i < 36; ++i) Li[i] = 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    Li[c * 6 + c] = 1.0 / L[c * 6 + c];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = c; k < r; ++k) s += L[r * 6 + k] * Li[k * 6 + c];
      Li[r * 6 + c] = -s / L[r * 6 + r];
    }
  }
}

struct SolveArgs {
  double* S;
  const int* first;
  const int* row;
  const int* last;
  const double* g;
  double* Linv;
  double* x;
  int* status;
  int N;
  const int* cptr;   // column k's profile rows crows[cptr[k] … cptr[k+1]) (every i > k with first(i) ≤ k, in order)
  const int* crows;
};

__device__ __forceinline__ long long sky_off(const SolveArgs& a, int i, int j) {  // block (i, j), j ≥ first(i)
  return ((long long)a.row[i] + (j - a.first[i])) * 36;
}

__global__ __launch_bounds__(256) void skyline_solve_kernel(const SolveArgs a) {
  __shared__ double sA[36], sL[36], sLi[36];
  __shared__ int s_fail;
  const int tid = threadIdx.x;
  if (tid == 0) s_fail = 0;
  for (int k = 0; k < a.N; ++k) {
    const long long okk = sky_off(a, k, k);
    if (tid < 36) sA[tid] = a.S[okk + tid];
    __syncthreads();
    if (tid == 0) {  // in registers: the LDS-pointer forms' dependent LDS round trips were most of a column's time
      double A[36], L[36], Li[36];
#pragma unroll
      for (int q = 0; q < 36; ++q) A[q] = sA[q];
      if (!chol6_reg(A, L)) {
        s_fail = k + 1;
      } else {
        inv_lower6_reg(L, Li);
#pragma unroll
        for (int q = 0; q < 36; ++q) {
          sL[q] = L[q];
          sLi[q] = Li[q];
        }
      }
    }
    __syncthreads();
    if (s_fail) {
      if (tid == 0) *a.status = s_fail;
      return;
    }
    if (tid < 36) {
      a.S[okk + tid] = sL[tid];
      a.Linv[(long long)k * 36 + tid] = sLi[tid];
    }
    // column k's profile rows: the band below the diagonal and, with free intrinsics, the dense border rows — walking
    // (k, last(k)] instead enumerated every row pair up to the border, O(N²) per column (C3 with free intrinsics: 0.7 s
    // per solve)
    const int c0 = a.cptr[k], na = a.cptr[k + 1] - c0;
    const int* rows = a.crows + c0;
    // column panel L_ik = A_ik · L_kk⁻ᵀ, 7 blocks per pass (read all, barrier, write)
    for (int i0 = 0; i0 < na; i0 += 7) {
      double val = 0.0;
      long long dst = -1;
      const int li = i0 + tid / 36;
      if (tid < 252 && li < na) {
        const int i = rows[li], e = tid % 36, r = e / 6, c = e % 6;
        const long long o = sky_off(a, i, k);
        for (int m = 0; m <= c; ++m) val += a.S[o + r * 6 + m] * sLi[c * 6 + m];
        dst = o + e;
      }
      __syncthreads();
      if (dst >= 0) a.S[dst] = val;
      __threadfence_block();
      __syncthreads();
    }
    // trailing update A_ij −= L_ik L_jkᵀ over the pairs of the column's rows (i ≥ j)
    const int npairs = na * (na + 1) / 2;
    for (int idx = tid; idx < npairs * 36; idx += 256) {
      const int pidx = idx / 36, e = idx % 36, r = e / 6, c = e % 6;
      int ii = 0;  // decode lower-triangular pair index → (ii ≥ jj)
      while ((ii + 1) * (ii + 2) / 2 <= pidx) ++ii;
      const int jj = pidx - ii * (ii + 1) / 2;
      const int i = rows[ii], j = rows[jj];
      const long long oi = sky_off(a, i, k), oj = sky_off(a, j, k);
      double s = 0.0;
      for (int m = 0; m < 6; ++m) s += a.S[oi + r * 6 + m] * a.S[oj + c * 6 + m];
      a.S[sky_off(a, i, j) + e] -= s;
    }
    __threadfence_block();
    __syncthreads();
  }
  // forward substitution L y = −g (y in x)
  for (int t = tid; t < 6 * a.N; t += 256) a.x[t] = -a.g[t];
  __threadfence_block();
  __syncthreads();
  for (int k = 0; k < a.N; ++k) {
    __shared__ double yk[6];
    if (tid < 6) {
      double s = 0.0;
      for (int m = 0; m <= tid; ++m) s += a.Linv[(long long)k * 36 + tid * 6 + m] * a.x[6 * k + m];
      yk[tid] = s;
    }
    __syncthreads();
    if (tid < 6) a.x[6 * k + tid] = yk[tid];
    const int c0 = a.cptr[k], na = a.cptr[k + 1] - c0;
    for (int idx = tid; idx < na * 6; idx += 256) {
      const int i = a.crows[c0 + idx / 6], r = idx % 6;
      const long long o = sky_off(a, i, k);
      double s = 0.0;
      for (int m = 0; m < 6; ++m) s += a.S[o + r * 6 + m] * yk[m];
      a.x[6 * i + r] -= s;
    }
    __threadfence_block();
    __syncthreads();
  }
  // back substitution Lᵀ x = y
  for (int k = a.N - 1; k >= 0; --k) {
    __shared__ double tk[6];
    if (tid < 6) {
      double s = a.x[6 * k + tid];
      for (int q = a.cptr[k]; q < a.cptr[k + 1]; ++q) {
        const int i = a.crows[q];
        const long long o = sky_off(a, i, k);
        for (int m = 0; m < 6; ++m) s -= a.S[o + m * 6 + tid] * a.x[6 * i + m];
      }
      tk[tid] = s;
    }
    __syncthreads();
    if (tid < 6) {
      double s = 0.0;
      for (int m = tid; m < 6; ++m) s += a.Linv[(long long)k * 36 + m * 6 + tid] * tk[m];
      a.x[6 * k + tid] = s;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (tid == 0) *a.status = 0;
}

// rsqrt_nr (pba_device.h): hardware v_rsq_f64 seed + two Newton steps — the pivot is on the solver's
// serial critical path; this is ~3x shorter than sqrt() + division.
__device__ inline bool chol6_rcp(double* A, double* invd) {  // in place, lower; returns reciprocal pivots
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= A[j * 6 + k] * A[j * 6 + k];
    if (!(s > 0.0)) return false;
    const double il = rsqrt_nr(s), l = s * il;
    A[j * 6 + j] = l;
    invd[j] = il;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= A[i * 6 + k] * A[j * 6 + k];
      A[i * 6 + j] = t * il;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i + 1; j < 6; ++j) A[i * 6 + j] = 0.0;
  return true;
}

// ------------------------------------------------------------------------------------------------
// front_solve_kernel: the same factorisation and solve with the ACTIVE FRONT in LDS (one workgroup)
// ------------------------------------------------------------------------------------------------
// Right-looking block Cholesky touches, at column k, only the blocks among {k} ∪ rows(k), rows(k) = {i > k : first(i) ≤ k}
// — the front.  It moves by one row per column: k leaves, the rows with first(i) = k + 1 enter with their blocks fresh
// from S (no earlier column touched them).  gn_prepare gives every row a static LDS slot (a row admitted for column k + 1
// never takes a slot in use at column k) and writes per column a record: the slots, row indices and factor-block
// indices of rows(k), and the fresh blocks of the next column's admissions (source skyline block → front position
// slot_hi·F + slot_lo) — build_front_plan; a multi-GPU free-intrinsics solve has a plan of its own for the summed
// profile (ensure_dist_sky).  skyline_solve_kernel walks the same factorisation through global memory, a dependent L2
// round trip per phase (≈ 9 µs per column); here the front, the forward vector and the records live in LDS and the
// next column's fresh blocks and record are loaded while this column is factored.  Free intrinsics make the profile a
// band plus 2·nc dense border rows: F = K + 1 + 2nc slots (C3/C4: 7).
// Every lane issues its share of the global loads of the record two columns ahead and of the next column's fresh
// blocks (backward: its staged factor blocks) at a column's start and stores them to LDS at its end.  (A dedicated
// loader wave measured slower: the compiler's conservative waits then stalled that wave at the barriers.)
// Forward (2 barriers per column): 6·|rows(k)| lanes form L_ik = A_ik L_kk⁻ᵀ row by row (to LDS, to L, v_i −= L_ik y_k);
// then the trailing pairs A_ij −= L_ik L_jkᵀ while one lane finishes and factors the next diagonal block (look-ahead:
// L_kk, reciprocal pivots and y_k = L_kk⁻¹ v_k were formed during column k − 1).
// Backward (2 barriers per column): 6·|rows(k)| lanes form the products L_ikᵀ x_i, six lanes add them in order and one
// solves x_k = L_kk⁻ᵀ (y_k − Σ_i L_ikᵀ x_i).
constexpr int kFrontHdr = 3;
struct FrontArgs {
  const double* S;      // the assembled skyline system
  const double* g;
  double* L;            // the factor's off-diagonal blocks (skyline layout)
  double* lrec;         // per column: L_kk | 1/pivots | y_k
  const int* rec;       // per column: kFrontHdr + 3·fm + 2·mf ints
  const int2* init;     // the rows of column 0's front: (source block, front position)
  double* x;
  int* status;
  int N, F, fm, mf, R, n_init;
};
constexpr int kFrontPf = 4;  // doubles per lane per column: fresh blocks (mf·36) / staged blocks (fm·36 + 48)
constexpr int kFrontPr = 1;  // record ints per lane (R ≤ 256)

__global__ __launch_bounds__(256) void front_solve_kernel(const FrontArgs a) {
  extern __shared__ double front_lds[];
  const int tid = threadIdx.x, N = a.N, F = a.F, fm = a.fm, mf = a.mf, R = a.R;
  const int SB = fm * 36 + 48, ld = tid;
  double* fr = front_lds;                                // F·F blocks: block (i ≥ j) at slot_i·F + slot_j
  double* ys = fr + (size_t)F * F * 36;                  // v → y → x, 6 per row
  double* stg = ys + 6 * N;                              // backward: 2 × SB
  int* recb = reinterpret_cast<int*>(stg + 2 * SB);      // 3 × R: records k, k + 1, k + 2 (backward: k, k − 1, k − 2)
  int* pairs = recb + 3 * R;                             // lower-triangle pair p → (ii << 16) | jj
  __shared__ double sL[2][36], sd[2][6], sy[2][6], sp[6 * 32];  // the diagonal factor of columns k, k + 1
  __shared__ double sDn[36];                                       // column k + 1's diagonal block (look-ahead)
  __shared__ int s_fail;
#ifdef PBA_FRONT_STAMPS  // timing variant: per-phase wall-clock sums of lanes 0, 64 and 192, written over x[0 … 29]
  unsigned long long fts[10] = {}, ft0 = 0;
#define FRONT_STAMP(i) { const unsigned long long t_ = wall_clock64(); if ((i) > 0) fts[(i) - 1] += t_ - ft0; ft0 = t_; }
#else
#define FRONT_STAMP(i)
#endif
  // the prefetch loads: unconditional (clamped addresses; the stores are guarded) — under a branch, the compiler waited
  // for every load in flight at the first use of any
  auto load_rec = [&](int k, int (&regs)[kFrontPr]) {
#pragma unroll
    for (int q = 0; q < kFrontPr; ++q)
      regs[q] = a.rec[(long long)min(max(k, 0), N - 1) * R + min(ld + 256 * q, R - 1)];
  };
  auto store_rec = [&](int k, const int (&regs)[kFrontPr]) {
#pragma unroll
    for (int q = 0; q < kFrontPr; ++q)
      if (ld + 256 * q < R) recb[(k % 3) * R + ld + 256 * q] = regs[q];
  };
  auto load_fresh = [&](const int* rk, double (&regs)[kFrontPf]) {  // the blocks column k admits for column k + 1
    const int nfr = rk[2];
    const int* fsrc = rk + kFrontHdr + 3 * fm;
#pragma unroll
    for (int q = 0; q < kFrontPf; ++q) {
      const int idx = min(ld + 256 * q, max(nfr * 36 - 1, 0));
      regs[q] = a.S[(long long)(nfr ? fsrc[idx / 36] : 0) * 36 + idx % 36];
    }
  };
  if (tid == 0) s_fail = 0;
  for (int t = tid; t < 6 * N; t += 256) ys[t] = -a.g[t];
  for (int t = tid; t < a.n_init * 36; t += 256) {
    const int2 q = a.init[t / 36];
    fr[(long long)q.y * 36 + t % 36] = a.S[(long long)q.x * 36 + t % 36];
  }
  for (int t = tid; t < 2 * R; t += 256)
    if (t / R < N) recb[t] = a.rec[t];
  for (int p = tid; p < fm * (fm + 1) / 2; p += 256) {
    int ii = 0;
    while ((ii + 1) * (ii + 2) / 2 <= p) ++ii;
    pairs[p] = (ii << 16) | (p - ii * (ii + 1) / 2);
  }
  __syncthreads();

  // the 6×6 factor of a diagonal block, y = L⁻¹ v, into buffer set q (one lane); false: not positive definite
  auto factor = [&](const double (&D)[36], int col, int q) -> bool {
    double A[36], d[6];
#pragma unroll
    for (int e = 0; e < 36; ++e) A[e] = D[e];
    if (!chol6_rcp(A, d)) return false;
    double b[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) b[r] = ys[6 * col + r];
#pragma unroll
    for (int c = 0; c < 6; ++c) {  // y_col = L⁻¹ v_col
      double t = b[c];
#pragma unroll
      for (int m = 0; m < c; ++m) t -= A[c * 6 + m] * b[m];
      b[c] = t * d[c];
    }
#pragma unroll
    for (int e = 0; e < 36; ++e) sL[q][e] = A[e];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      sd[q][r] = d[r];
      sy[q][r] = b[r];
      ys[6 * col + r] = b[r];
    }
    return true;
  };
  auto factor_lds = [&](int col, int slot, int q) {  // column col's diagonal block as it stands in the front
    double D[36];
    const double* Dk = fr + (long long)(slot * F + slot) * 36;
#pragma unroll
    for (int e = 0; e < 36; ++e) D[e] = Dk[e];
    if (!factor(D, col, q)) s_fail = col + 1;
  };
  if (N > 0 && tid == 0) factor_lds(0, recb[0], 0);
  __syncthreads();
  if (s_fail) {
    if (tid == 0) *a.status = s_fail;
    return;
  }

  // One column, LOOK-AHEAD: its diagonal block was factored during the previous column (buffer set k & 1).  Panel,
  // then — while lanes 0-191 run the trailing update — lane 192 forms column k + 1's diagonal block (its last update,
  // −L_{k+1,k} L_{k+1,k}ᵀ, when k + 1 is the column's first row) and factors it: the 6×6 factor's serial chain is off
  // the critical path.  A column k + 1 outside rows(k) (admitted fresh at k + 1) is factored after the barrier.
  // cur holds the column's admissions (loaded during the previous column), nxt receives the next column's — two
  // columns per pass with the arrays swapped (no register copies).
  auto column = [&](int k, double (&cur)[kFrontPf], double (&nxt)[kFrontPf]) -> bool {
    const int* rk = recb + (k % 3) * R;
    const int sk = rk[0], na = rk[1], nfr = rk[2], q = k & 1;
    const int* slots = rk + kFrontHdr;
    const int* rows = slots + fm;
    const int* gbl = rows + fm;
    const int* fdst = gbl + fm + mf;
    FRONT_STAMP(0);
    int pr[kFrontPr];
    load_rec(k + 2, pr);  // before the fresh loads: waiting for it must not wait for them
    if (k + 1 < N) load_fresh(recb + ((k + 1) % 3) * R, nxt);
    FRONT_STAMP(1);
    FRONT_STAMP(2);
    if (tid < na * 6) {  // panel row r of L_ik = A_ik L_kk⁻ᵀ; v_i −= L_ik y_k
      const int li = tid / 6, r = tid % 6;
      double* A = fr + (long long)(slots[li] * F + sk) * 36 + r * 6;
      double X[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double t = A[c];
#pragma unroll
        for (int m = 0; m < c; ++m) t -= X[m] * sL[q][c * 6 + m];
        X[c] = t * sd[q][c];
      }
      double* Lg = a.L + (long long)gbl[li] * 36 + r * 6;
      double dv = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        A[c] = X[c];
        Lg[c] = X[c];
        dv += X[c] * sy[q][c];
      }
      ys[6 * rows[li] + r] -= dv;
    } else if (tid >= 192 && tid < 240) {
      const int e = tid - 192;
      a.lrec[(long long)k * 48 + e] = e < 36 ? sL[q][e] : (e < 42 ? sd[q][e - 36] : sy[q][e - 42]);
    }
    FRONT_STAMP(3);
    __syncthreads();
    FRONT_STAMP(4);
    const bool ahead = k + 1 < N && na > 0 && rows[0] == k + 1;  // (uniform)
    const int np = na * (na + 1) / 2;  // trailing A_ij −= L_ik L_jkᵀ (i ≥ j in rows(k)); pair 0 = (k+1, k+1) if ahead
    if (tid < 192) {  // four items per lane in flight: their dependent LDS rounds (pair → slots → rows → element) overlap
      constexpr int TR = 4;
      const int i0 = ahead ? 36 : 0, ne = np * 36;
      for (int base = i0 + tid; base < ne; base += 192 * TR) {
        double acc[TR];
        int dst[TR];
#pragma unroll
        for (int u = 0; u < TR; ++u) {
          const int idx = min(base + 192 * u, ne - 1);
          const int pq = pairs[idx / 36], e = idx % 36, r = e / 6, c = e % 6;
          const int si = slots[pq >> 16], sj = slots[pq & 0xffff];
          const double* Li = fr + (si * F + sk) * 36 + r * 6;
          const double* Lj = fr + (sj * F + sk) * 36 + c * 6;
          double t = 0.0;
#pragma unroll
          for (int m = 0; m < 6; ++m) t += Li[m] * Lj[m];
          acc[u] = t;
          dst[u] = (si * F + sj) * 36 + e;
        }
#pragma unroll
        for (int u = 0; u < TR; ++u)
          if (base + 192 * u < ne) fr[dst[u]] -= acc[u];
      }
    } else if (ahead) {  // wave 3: column k + 1's diagonal block, final (lane e: entry e), then lane 192 factors it
      const int s1 = slots[0], e = tid - 192;
      if (e < 36) {
        const double* Li = fr + (long long)(s1 * F + sk) * 36 + (e / 6) * 6;
        const double* Lj = fr + (long long)(s1 * F + sk) * 36 + (e % 6) * 6;
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) acc += Li[m] * Lj[m];
        sDn[e] = fr[(long long)(s1 * F + s1) * 36 + e] - acc;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (e == 0) {
        double D[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) D[i] = sDn[i];
        if (!factor(D, k + 1, q ^ 1)) s_fail = k + 2;
      }
    }
#pragma unroll
    for (int qq = 0; qq < kFrontPf; ++qq) {  // column k's admissions (slots unused at column k), the record of k + 2
      const int idx = ld + 256 * qq;
      if (idx < nfr * 36) fr[(long long)fdst[idx / 36] * 36 + idx % 36] = cur[qq];
    }
    if (k + 2 < N) store_rec(k + 2, pr);
    FRONT_STAMP(5);
    __syncthreads();
    FRONT_STAMP(6);
    if (k + 1 < N && !ahead) {  // column k + 1 entered the front fresh: factor it now
      if (tid == 0) factor_lds(k + 1, recb[((k + 1) % 3) * R], q ^ 1);
      __syncthreads();
    }
    if (s_fail) {
      if (tid == 0) *a.status = s_fail;
      return false;
    }
    return true;
  };
  double pf[kFrontPf], pfn[kFrontPf];
  load_fresh(recb, pf);
  for (int k = 0; k < N; k += 2) {
    if (!column(k, pf, pfn)) return;
    if (k + 1 < N && !column(k + 1, pfn, pf)) return;
  }
  __threadfence();
  __syncthreads();

  // backward: x_k = L_kk⁻ᵀ (y_k − Σ_i L_ikᵀ x_i); column k's blocks staged during column k + 1, loaded during k + 2
  auto load_stage = [&](int k, const int* rk, double (&regs)[kFrontPf]) {
    const int na = rk[1];
    const int* gbl = rk + kFrontHdr + 2 * fm;
#pragma unroll
    for (int q = 0; q < kFrontPf; ++q) {  // unused stage entries hold any value
      const int idx = ld + 256 * q;
      const double* src = a.lrec;
      if (k >= 0 && idx < na * 36) src = a.L + (long long)gbl[idx / 36] * 36 + idx % 36;
      else if (k >= 0 && idx >= fm * 36 && idx < SB) src = a.lrec + (long long)k * 48 + idx - fm * 36;
      regs[q] = *src;
    }
  };
  auto store_stage = [&](int k, const double (&regs)[kFrontPf]) {
#pragma unroll
    for (int q = 0; q < kFrontPf; ++q)
      if (ld + 256 * q < SB) stg[(k & 1) * SB + ld + 256 * q] = regs[q];
  };
  double pb[kFrontPf], pbn[kFrontPf];  // cur / nxt of bcolumn, swapped per column as the forward pass
  for (int t = tid; t < 3 * R; t += 256) {
    const int k = N - 1 - t / R;
    if (k >= 0) recb[(k % 3) * R + t % R] = a.rec[(long long)k * R + t % R];
  }
  __syncthreads();
  {
    const int* rk = recb + ((N - 1) % 3) * R;
    for (int t = tid; t < SB; t += 256) {
      double v = 0.0;
      if (t < rk[1] * 36) v = a.L[(long long)rk[kFrontHdr + 2 * fm + t / 36] * 36 + t % 36];
      else if (t >= fm * 36) v = a.lrec[(long long)(N - 1) * 48 + t - fm * 36];
      stg[((N - 1) & 1) * SB + t] = v;
    }
  }
  load_stage(N - 2, recb + (((N - 2) % 3 + 3) % 3) * R, pb);
  __syncthreads();
  auto bcolumn = [&](int k, double (&cur)[kFrontPf], double (&nxt)[kFrontPf]) {
    const int* rk = recb + (k % 3) * R;
    const double* st = stg + (k & 1) * SB;
    const int na = rk[1];
    FRONT_STAMP(0);
    int pr[kFrontPr];
    load_rec(k - 3, pr);
    load_stage(k - 2, recb + (((k - 2) % 3 + 3) % 3) * R, nxt);
    if (tid < na * 6) {  // (L_ikᵀ x_i)_r
      const int li = tid / 6, r = tid % 6;
      const double* Lb = st + li * 36 + r;
      const double* xi = ys + 6 * rk[kFrontHdr + fm + li];
      double p = 0.0;
#pragma unroll
      for (int m = 0; m < 6; ++m) p += Lb[m * 6] * xi[m];
      sp[tid] = p;
    }
    FRONT_STAMP(7);
    __syncthreads();
    FRONT_STAMP(8);
    if (tid < 64) {  // lanes 0-5 add the products of entry r in order, lane 0 solves
      double tr = 0.0;
      if (tid < 6) {
        tr = st[fm * 36 + 42 + tid];
        for (int li = 0; li < na; ++li) tr -= sp[li * 6 + tid];
      }
      double t[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) t[r] = __shfl(tr, r, 64);
      if (tid == 0) {
#pragma unroll
      for (int r = 5; r >= 0; --r) {  // L_kkᵀ x = t
        double v = t[r];
#pragma unroll
        for (int m = r + 1; m < 6; ++m) v -= st[fm * 36 + m * 6 + r] * t[m];
        t[r] = v * st[fm * 36 + 36 + r];
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        ys[6 * k + r] = t[r];
        a.x[6 * k + r] = t[r];
      }
      }
    }
    if (k >= 1) store_stage(k - 1, cur);  // column k − 1's stage (not read at column k)
    if (k >= 3) store_rec(k - 3, pr);     // the record of k − 3 (over record k)
    FRONT_STAMP(9);
    __syncthreads();
    FRONT_STAMP(10);
  };
  for (int k = N - 1; k >= 0; k -= 2) {
    bcolumn(k, pb, pbn);
    if (k >= 1) bcolumn(k - 1, pbn, pb);
  }
  if (tid == 0) *a.status = 0;
#ifdef PBA_FRONT_STAMPS
  __syncthreads();
  if (tid == 0 || tid == 64 || tid == 192)
    for (int i = 0; i < 10; ++i) a.x[(tid == 0 ? 0 : (tid == 64 ? 10 : 20)) + i] = (double)fts[i];
#endif
#undef FRONT_STAMP
}

// ------------------------------------------------------------------------------------------------
// band_solve_kernel<B>: the same factorisation when every block row satisfies first(i) ≥ i − B (the
// structure of windowed/sequential BA — C3/C4 have B = 4).  The assembly also writes S in dense band
// layout (block c of row i = column i − B + c), so the next block row's address needs no indirection.
// The active window of the factor (block rows k..k+B) lives in LDS as a ring; block row k+B+2 is
// prefetched into registers two steps ahead.  Per step: one lane factors the 6×6 diagonal block
// (reciprocal pivots, no inverse), B·6 lanes solve the column panel L_ik = A_ik L_kk⁻ᵀ row by row, the
// trailing triangle is updated in parallel, and forward substitution is fused in.  Finished rows of L and
// the reciprocal pivots go to global memory for the backward pass, which prefetches one step ahead.
// ------------------------------------------------------------------------------------------------
struct BandArgs {
  const double* Sband;  // N rows × ((B+1)·36 + 6): blocks of columns i−B..i, then g_i
  double* Lcol;         // N column records × (B·36 + 48): L_(k+q),k for q = 1..B | L_kk | 1/pivots | y_k
  double* x;            // the step δ_poses
  int* status;
  int N;
};

template <int B>
__global__ __launch_bounds__(256) void band_solve_kernel(const BandArgs a) {
  constexpr int W = B + 1;
  constexpr int ROWF = W * 36;
  constexpr int ROWG = ROWF + 6;
  constexpr int COLF = B * 36 + 48;
  constexpr int CH = B <= 8 ? 16 : 4;      // rows / column records per prefetch chunk
  constexpr int STG = CH * COLF;           // ≥ CH·ROWG
  constexpr int PCH = (STG + 255) / 256;
  __shared__ double win[W * ROWG];         // ring of block rows k..k+B (slot i % W)
  __shared__ double stage[2 * STG];        // double-buffered prefetch chunks
  __shared__ double ring[W * 6];           // y (forward) / x (backward) of the last B+1 block rows
  __shared__ double sd[6], sv[6];
  __shared__ int s_fail;
  const int tid = threadIdx.x, N = a.N;

  // ---- forward: factor + fused forward substitution -------------------------------------------------
  auto load_rows = [&](int r0, double* regs) {  // rows r0 .. r0+CH−1 (zero beyond N)
#pragma unroll
    for (int q = 0; q < PCH; ++q) {
      const int idx = tid + q * 256;
      const int i = r0 + idx / ROWG;
      regs[q] = (idx < CH * ROWG && i < N) ? a.Sband[(long long)r0 * ROWG + idx] : 0.0;
    }
  };
  auto put_stage = [&](int buf, const double* regs, int n) {
#pragma unroll
    for (int q = 0; q < PCH; ++q) {
      const int idx = tid + q * 256;
      if (idx < n) stage[buf * STG + idx] = regs[q];
    }
  };
  if (tid == 0) s_fail = 0;
  for (int idx = tid; idx < W * ROWG; idx += 256)
    win[idx] = (idx / ROWG < N) ? a.Sband[idx] : 0.0;  // rows 0..B into slots 0..B
  if (tid < W * 6) ring[tid] = 0.0;
  double pf[PCH];
  load_rows(W, pf);
  put_stage(0, pf, CH * ROWG);
  __syncthreads();

  for (int k = 0; k < N; ++k) {
    const int c = k / CH, o = k % CH;
    double* rk = win + (k % W) * ROWG;
    double* Lkk = rk + B * 36;
    if (o == 0) load_rows(W + (c + 1) * CH, pf);  // next chunk, lands during the next CH steps
    if (tid == 0) {
      double A[36], d[6];
#pragma unroll
      for (int e = 0; e < 36; ++e) A[e] = Lkk[e];
      if (!chol6_rcp(A, d)) {
        s_fail = k + 1;
      } else {
#pragma unroll
        for (int e = 0; e < 36; ++e) Lkk[e] = A[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) sd[e] = d[e];
      }
    } else if (tid >= 64 && tid < 70) {  // b_k = −g_k − Σ_j L_kj y_j   (L_kj final, y_j in the ring)
      const int r = tid - 64;
      double v = -rk[ROWF + r];
#pragma unroll
      for (int cc = 0; cc < B; ++cc) {
        const int j = k - B + cc;
        if (j < 0) continue;
        const double* Lb = rk + cc * 36 + r * 6;
        const double* yj = ring + (j % W) * 6;
#pragma unroll
        for (int m = 0; m < 6; ++m) v -= Lb[m] * yj[m];
      }
      sv[r] = v;
    }
    __syncthreads();
    if (s_fail) {
      if (tid == 0) *a.status = s_fail;
      return;
    }
    const int nk = min(B, N - 1 - k);
    double* rec = a.Lcol + (long long)k * COLF;
    if (tid < nk * 6) {  // panel row r of L_ik = A_ik L_kk⁻ᵀ
      const int ii = 1 + tid / 6, r = tid % 6;
      double* A = win + ((k + ii) % W) * ROWG + (B - ii) * 36 + r * 6;
      double X[6];
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        double t = A[cc];
#pragma unroll
        for (int m = 0; m < cc; ++m) t -= X[m] * Lkk[cc * 6 + m];
        X[cc] = t * sd[cc];
      }
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) A[cc] = X[cc];
    } else if (tid >= 192 && tid < 228) {
      rec[B * 36 + (tid - 192)] = Lkk[tid - 192];
    } else if (tid >= 228 && tid < 234) {
      rec[B * 36 + 36 + (tid - 228)] = sd[tid - 228];
    } else if (tid == 255) {  // y_k = L_kk⁻¹ b_k
      double L[36], bb[6], d[6];
#pragma unroll
      for (int e = 0; e < 36; ++e) L[e] = Lkk[e];
#pragma unroll
      for (int r = 0; r < 6; ++r) { bb[r] = sv[r]; d[r] = sd[r]; }
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        double t = bb[cc];
#pragma unroll
        for (int m = 0; m < cc; ++m) t -= L[cc * 6 + m] * bb[m];
        bb[cc] = t * d[cc];
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        ring[(k % W) * 6 + r] = bb[r];
        rec[B * 36 + 42 + r] = bb[r];
      }
    }
    __syncthreads();
    // trailing update A_ij −= L_ik L_jkᵀ (k < j ≤ i ≤ k+nk); column k of L to the record
    const int npairs = nk * (nk + 1) / 2;
    for (int idx = tid; idx < npairs * 36; idx += 256) {
      const int pidx = idx / 36, e = idx % 36, r = e / 6, cc = e % 6;
      int ii = 0;
      while ((ii + 1) * (ii + 2) / 2 <= pidx) ++ii;
      const int jj = pidx - ii * (ii + 1) / 2;
      const int i = k + 1 + ii, j = k + 1 + jj;
      const double* Li_ = win + (i % W) * ROWG + (k - i + B) * 36;
      const double* Lj_ = win + (j % W) * ROWG + (k - j + B) * 36;
      double sacc = 0.0;
#pragma unroll
      for (int m = 0; m < 6; ++m) sacc += Li_[r * 6 + m] * Lj_[cc * 6 + m];
      win[(i % W) * ROWG + (j - i + B) * 36 + e] -= sacc;
    }
    for (int idx = tid; idx < B * 36; idx += 256) {
      const int q = 1 + idx / 36, e = idx % 36;
      rec[idx] = (q <= nk) ? win[((k + q) % W) * ROWG + (B - q) * 36 + e] : 0.0;
    }
    // row k+B+1 from the staged chunk into row k's slot (first read by the next step's panel)
    {
      const double* src = stage + (c & 1) * STG + o * ROWG;
      for (int idx = tid; idx < ROWG; idx += 256) rk[idx] = src[idx];
    }
    if (o == CH - 1) put_stage((c + 1) & 1, pf, CH * ROWG);
    __syncthreads();
  }
  __threadfence();
  __syncthreads();

  // ---- backward: x_k = L_kk⁻ᵀ (y_k − Σ_q L_(k+q),kᵀ x_(k+q)), column records streamed in reverse ---------
  auto load_cols = [&](int s0, double* regs) {  // records for steps s0..s0+CH−1, k = N−1−s
#pragma unroll
    for (int q = 0; q < PCH; ++q) {
      const int idx = tid + q * 256;
      const int sidx = s0 + idx / COLF;
      regs[q] = (idx < STG && sidx < N) ? a.Lcol[(long long)(N - 1 - sidx) * COLF + idx % COLF] : 0.0;
    }
  };
  if (tid < W * 6) ring[tid] = 0.0;
  load_cols(0, pf);
  put_stage(0, pf, STG);
  __syncthreads();
  for (int sstep = 0; sstep < N; ++sstep) {
    const int k = N - 1 - sstep, c = sstep / CH, o = sstep % CH;
    if (o == 0) load_cols((c + 1) * CH, pf);
    const double* rec = stage + (c & 1) * STG + o * COLF;
    if (tid < 6) {
      const int r = tid;
      double v = rec[B * 36 + 42 + r];
#pragma unroll
      for (int q = 1; q <= B; ++q) {
        if (k + q >= N) break;
        const double* Lq = rec + (q - 1) * 36;
        const double* xq = ring + ((k + q) % W) * 6;
#pragma unroll
        for (int m = 0; m < 6; ++m) v -= Lq[m * 6 + r] * xq[m];
      }
      sv[r] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double L[36], t[6], id[6];
#pragma unroll
      for (int e = 0; e < 36; ++e) L[e] = rec[B * 36 + e];
#pragma unroll
      for (int r = 0; r < 6; ++r) { t[r] = sv[r]; id[r] = rec[B * 36 + 36 + r]; }
#pragma unroll
      for (int r = 5; r >= 0; --r) {  // L_kkᵀ x = t
        double v = t[r];
#pragma unroll
        for (int m = r + 1; m < 6; ++m) v -= L[m * 6 + r] * t[m];
        t[r] = v * id[r];
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        ring[(k % W) * 6 + r] = t[r];
        a.x[6 * k + r] = t[r];
      }
    }
    if (o == CH - 1) put_stage((c + 1) & 1, pf, STG);
    __syncthreads();
  }
  if (tid == 0) *a.status = 0;
}

// S δ = −g by front_solve_kernel with plan P (S: the profile's skyline blocks; L: room for its factor).
int launch_front(pba_engine* e, FrontPlan& P, const double* S, double* L, int N) {
  GnData& G = e->gn;
  FrontArgs fa{S, G.g.p, L, P.lrec.p, P.rec.p, P.init.p, G.x.p, G.status.p, N, P.F, P.fm, P.mf, P.R, P.n_init};
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&front_solve_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds);  // may exceed 64 KB
  front_solve_kernel<<<1, 256, P.lds, e->stream>>>(fa);
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

}  // namespace

namespace pba {
namespace detail {

// front_solve_kernel's plan for a skyline profile (first(i), row offsets rowp, column lists): static slots — a row
// admitted for column k + 1 never takes a slot in use at column k — and the per-column records (see the kernel).
// P.lds = 0 when the front does not fit (or use = false): the caller then takes skyline_solve_kernel.
int build_front_plan(const std::vector<int>& first, const std::vector<int>& rowp, const std::vector<int>& ccptr,
                     const std::vector<int>& ccrows, hipStream_t st, FrontPlan& P, bool use) {
  const int nfs = (int)first.size();
  std::vector<std::vector<int>> adm(nfs);
  for (int i = 0; i < nfs; ++i) adm[first[i]].push_back(i);
  std::vector<int> slot(nfs, -1), freel;
  int F = 0;
  auto alloc = [&]() {
    if (freel.empty()) return F++;
    auto it = std::min_element(freel.begin(), freel.end());
    const int v = *it;
    freel.erase(it);
    return v;
  };
  for (int i : adm[0]) slot[i] = alloc();
  for (int k = 0; k < nfs; ++k) {
    if (k + 1 < nfs)
      for (int i : adm[k + 1]) slot[i] = alloc();
    freel.push_back(slot[k]);
  }
  // active set after column k's admissions: (A_k \ {k}) ∪ adm(k+1), kept sorted
  std::vector<std::vector<int2>> fresh(nfs);  // per column k: the blocks of the rows admitted for k + 1
  std::vector<int2> init;
  std::vector<int> act;
  auto blk = [&](int hi, int lo) { return rowp[hi] + (lo - first[hi]); };
  auto add_rows = [&](const std::vector<int>& newr, std::vector<int>& A, std::vector<int2>& out) {
    for (int i : newr) A.push_back(i);
    std::sort(A.begin(), A.end());
    for (int i : newr)
      for (int j : A) {
        if (j > i && std::binary_search(newr.begin(), newr.end(), j)) continue;  // the pair once (from j)
        const int hi = std::max(i, j), lo = std::min(i, j);
        out.push_back(make_int2(blk(hi, lo), slot[hi] * F + slot[lo]));
      }
  };
  add_rows(adm[0], act, init);
  int fm = 1, mf = 1;
  for (int k = 0; k < nfs; ++k) {
    fm = std::max(fm, ccptr[k + 1] - ccptr[k]);
    act.erase(std::remove(act.begin(), act.end(), k), act.end());
    if (k + 1 < nfs) add_rows(adm[k + 1], act, fresh[k]);
    mf = std::max(mf, (int)fresh[k].size());
  }
  const int R = kFrontHdr + 3 * fm + 2 * mf, SB = fm * 36 + 48;
  const size_t lds = sizeof(double) * ((size_t)F * F * 36 + 6 * (size_t)nfs + 2 * SB) +
                     sizeof(int) * (3 * (size_t)R + fm * (fm + 1) / 2);
  P.lds = 0;
  if (!use || fm > 32 || mf * 36 > 256 * kFrontPf || SB > 256 * kFrontPf || R > 256 * kFrontPr || lds > 150 * 1024)
    return PBA_OK;
  std::vector<int> rec((size_t)nfs * R, 0);
  for (int k = 0; k < nfs; ++k) {
    int* r = rec.data() + (size_t)k * R;
    const int na = ccptr[k + 1] - ccptr[k];
    r[0] = slot[k];
    r[1] = na;
    r[2] = (int)fresh[k].size();
    for (int li = 0; li < na; ++li) {
      const int i = ccrows[ccptr[k] + li];
      r[kFrontHdr + li] = slot[i];
      r[kFrontHdr + fm + li] = i;
      r[kFrontHdr + 2 * fm + li] = blk(i, k);
    }
    for (int q = 0; q < (int)fresh[k].size(); ++q) {
      r[kFrontHdr + 3 * fm + q] = fresh[k][q].x;
      r[kFrontHdr + 3 * fm + mf + q] = fresh[k][q].y;
    }
  }
  PBA_HIP(P.rec.upload(rec, st));
  P.n_init = (int)init.size();
  if (init.empty()) init.push_back(make_int2(0, 0));
  PBA_HIP(P.init.upload(init, st));
  PBA_HIP(P.lrec.resize((size_t)nfs * 48));
  P.F = F;
  P.fm = fm;
  P.mf = mf;
  P.R = R;
  P.lds = lds;
  return PBA_OK;
}

void launch_band_cholesky(pba_engine* e) {
  GnData& G = e->gn;
  BandArgs ba{G.Sband.p, G.Lband.p, G.x.p, G.status.p, e->n_frames};
  if (G.band_kernel == 4) band_solve_kernel<4><<<1, 256, 0, e->stream>>>(ba);
  else if (G.band_kernel == 8) band_solve_kernel<8><<<1, 256, 0, e->stream>>>(ba);
  else band_solve_kernel<16><<<1, 256, 0, e->stream>>>(ba);
}

int skyline_solve(pba_engine* e, const SkylineSystem& s, ArrowUse arrow) {
  GnData& G = e->gn;
  if (arrow != ArrowUse::none) return arrow_solve(e, s.S, s.first, s.row, s.fixed, arrow == ArrowUse::built);
  if (s.front.lds) return launch_front(e, s.front, s.S, s.L, s.N);
  PBA_HIP(hipMemcpyAsync(s.L, s.S, sizeof(double) * 36 * (size_t)s.n_blocks, hipMemcpyDeviceToDevice, e->stream));
  SolveArgs so{s.L, s.first, s.row, s.last, G.g.p, G.Linv.p, G.x.p, G.status.p, s.N, s.colptr, s.colrows};
  skyline_solve_kernel<<<1, 256, 0, e->stream>>>(so);
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

}  // namespace detail
}  // namespace pba
