// pba_gn_solve_cr.hip — block and parallel cyclic reduction of a Gauss-Newton trial's banded reduced camera system
// (pba_gn.hip), the free-intrinsics arrow solve on top of it, and the choice of the reduced-system solver (the direct
// solvers are pba_gn_solve_sky.hip).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "pba_gn.h"
#include "pba_gn_solve.h"

using namespace pba;
using namespace pba::detail;

namespace {

// ------------------------------------------------------------------------------------------------
// Block cyclic reduction (bandwidth B ≤ 8 block rows).  Super-row I = block rows [I·B, (I+1)·B) turns the
// banded reduced camera system into a block-tridiagonal SPD system with m×m blocks (m = 6B): diagonal D_I,
// coupling U_I = S(I, I+1).  Each level eliminates the odd super-rows j in parallel (one workgroup each:
// dense Cholesky of D_j in LDS, X_j = D_j⁻¹ [U_{j−1}ᵀ | U_j | b_j]) and rebuilds the even ones
// (D'_i = D_i − U_{i−1}ᵀ X_{i−1}^U − U_i X_{i+1}^L, U'_i = −U_i X_{i+1}^U, b'_i likewise).  log2(N/B) levels
// replace the N-step sequential factorisation; back-substitution runs the levels in reverse
// (x_j = X_j^b − X_j^L x_{j−1} − X_j^U x_{j+1}).
// ------------------------------------------------------------------------------------------------

template <int M>
__global__ __launch_bounds__(256) void cr_build_kernel(const double* __restrict__ Sband, CrLevel L0, int N, int B,
                                                       int* __restrict__ status) {
  // one thread per element of D_I, U_I and b_I of level 0 (rows ≥ N are identity padding); the solve's failure flag
  // is cleared here (the levels only ever set it), which saves a memset launch per solve
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid == 0) *status = 0;
  const long long nD = (long long)L0.n * M * M;
  const int ROWG = (B + 1) * 36 + 6;
  auto lower = [&](int i, int j, int r, int c) -> double {  // S[6i+r][6j+c] for i ≥ j within the band
    if (i >= N || j >= N) return (i == j && r == c) ? 1.0 : 0.0;
    if (i - j > B) return 0.0;
    return Sband[(long long)i * ROWG + (j - i + B) * 36 + r * 6 + c];
  };
  if (tid < nD) {
    const int I = (int)(tid / (M * M)), e = (int)(tid % (M * M)), R = e / M, C = e % M;
    const int i = I * B + R / 6, j = I * B + C / 6, r = R % 6, c = C % 6;
    L0.D[tid] = i >= j ? lower(i, j, r, c) : lower(j, i, c, r);
    // U_I: rows of super-row I, columns of super-row I+1 → S[6i+r][6j'+c] with j' > i
    const int jn = (I + 1) * B + C / 6;
    L0.U[tid] = (I + 1 < L0.n) ? lower(jn, i, c, r) : 0.0;
    return;
  }
  const long long t = tid - nD;
  if (t < (long long)L0.n * M) {
    const int I = (int)(t / M), R = (int)(t % M), i = I * B + R / 6;
    L0.b[t] = i < N ? -Sband[(long long)i * ROWG + (B + 1) * 36 + R % 6] : 0.0;
  }
}

// Eliminate super-row j (odd rows of the level, or the single root row when `root`): X = D⁻¹ [U_{j−1}ᵀ | U_j | b]
// by 2×2-block Gauss-Jordan on the augmented M × (3M+1) matrix [D | RHS] (no pivoting: D is SPD, so are its
// 2×2 pivot blocks).  Lane c owns column c in registers (steps fully unrolled, so every register index is
// static).  Step k: the pivot columns' owners publish their 2M values to LDS (double-buffered: one barrier per
// step), every lane reads them as broadcasts and updates its own column.  Measured on MI355X
// (tools/micro/cr_odd_timing.hip, M = 24): 12 µs per launch for 1×1 pivots against 29 µs for an element-owner
// formulation whose per-step publish/read traffic was LDS-bound.  A non-positive pivot flags the status.
template <int M>
constexpr int kCrOddThreads = ((3 * M + 1) + 63) / 64 * 64;  // one lane per column of [D | RHS], whole waves

// The elimination of one super-row by kCrOddThreads<M> lanes (tid = lane index within that group, c = its
// column); colk = the group's own publish buffers.  Every lane of the workgroup must call it (barriers).
// Returns false when a pivot block was not positive definite; a[] = column c of [D⁻¹ | D⁻¹RHS].
template <int M>
__device__ __forceinline__ bool gj_row(const CrLevel& L, int j, bool root, int tid, double (*colk)[2][M], double* a) {
  constexpr int NC = 2 * M + 1, W = M + NC;
  const int c = min(tid, W - 1);
  const double* D = L.D + (long long)j * M * M;
#pragma unroll
  for (int r = 0; r < M; ++r) {  // all of a lane's loads in flight at once
    const double* src;
    if (c < M) src = D + r * M + c;
    else if (c < 2 * M) src = root ? nullptr : L.U + (long long)(j - 1) * M * M + (c - M) * M + r;  // U_{j−1}ᵀ
    else if (c < 3 * M) src = (!root && j + 1 < L.n) ? L.U + (long long)j * M * M + r * M + (c - 2 * M) : nullptr;  // U_j
    else src = L.b + (long long)j * M + r;
    a[r] = src ? *src : 0.0;
  }
  bool bad = false;
  auto step = [&](int k) {
    const int buf = (k >> 1) & 1;
    if (tid == k || tid == k + 1) {
      double* dst = colk[buf][tid - k];
#pragma unroll
      for (int r = 0; r < M; ++r) dst[r] = a[r];
    }
    __syncthreads();
    const double* c0 = colk[buf][0];
    const double* c1 = colk[buf][1];
    const double p00 = c0[k], p10 = c0[k + 1], p01 = c1[k], p11 = c1[k + 1];
    const double det = p00 * p11 - p01 * p10;
    bad |= !(p00 > 0.0 && det > 0.0);
    const double rd = rcp_nr(det);
    double ak = a[0], ak1 = a[1];
#pragma unroll
    for (int r = 1; r < M; ++r) ak = r == k ? a[r] : ak;
#pragma unroll
    for (int r = 2; r < M; ++r) ak1 = r == k + 1 ? a[r] : ak1;
    const double t0 = (p11 * ak - p01 * ak1) * rd;
    const double t1 = (p00 * ak1 - p10 * ak) * rd;
#pragma unroll
    for (int r = 0; r < M; ++r) a[r] = r == k ? t0 : (r == k + 1 ? t1 : a[r] - c0[r] * t0 - c1[r] * t1);
  };
  if constexpr (M <= 24) {
#pragma unroll
    for (int k = 0; k < M; k += 2) step(k);
  } else {
#pragma unroll 1
    for (int k = 0; k < M; k += 2) step(k);
  }
  return !bad;
}

// One level of cyclic reduction in ONE launch: workgroup i/2 rebuilds even super-row i.  Its two halves
// eliminate the neighbouring odd rows i−1 and i+1 side by side (gj_row, redundantly with the neighbouring
// workgroups — each odd row is done twice, saving a launch and an HBM round trip of X per level), keep both X in
// LDS, store X_{i+1} for the back-substitution (every odd row is the right neighbour of exactly one even row),
// then form D'_i = D_i − U_{i−1}ᵀX^U_{i−1} − U_i X^L_{i+1}, U'_i = −U_i X^U_{i+1} and b'_i likewise.
template <int M>
constexpr size_t cr_level_lds() { return sizeof(double) * (2 * M * M + 2 * M * (2 * M + 1)); }

template <int M>
__global__ __launch_bounds__(2 * kCrOddThreads<M>) void cr_level_kernel(CrLevel L, CrLevel Ln, int* status) {
  constexpr int NC = 2 * M + 1, W = M + NC, T = kCrOddThreads<M>;
  __shared__ __attribute__((aligned(16))) double colk[2][2][2][M];
  extern __shared__ double smem[];
  double* sUl = smem;               // U_{i−1}   M×M
  double* sUi = sUl + M * M;        // U_i       M×M
  double* sX[2] = {sUi + M * M, sUi + M * M + M * NC};  // X_{i−1}, X_{i+1}   M×NC each
  const int i = 2 * blockIdx.x, in = blockIdx.x;
  const int half = threadIdx.x >= T ? 1 : 0, tl = threadIdx.x - half * T;
  const int j = half ? i + 1 : i - 1;
  const bool has = j >= 0 && j < L.n;
  double a[M];
  const bool ok = gj_row<M>(L, has ? j : 1, false, tl, colk[half], a);
  if (!ok && has && tl == 0) atomicOr(status, 1);
  if (tl >= M && tl < W) {
    double* x = sX[half] + (tl - M);
#pragma unroll
    for (int r = 0; r < M; ++r) x[r * NC] = has ? a[r] : 0.0;
    if (half && has) {
      double* X = L.X + (long long)(j / 2) * M * NC + (tl - M);
#pragma unroll
      for (int r = 0; r < M; ++r) X[r * NC] = a[r];
    }
  }
  const bool left = i - 1 >= 0, right = i + 1 < L.n;
  for (int e = threadIdx.x; e < M * M; e += 2 * T) {
    sUl[e] = left ? L.U[(long long)(i - 1) * M * M + e] : 0.0;
    sUi[e] = L.U[(long long)i * M * M + e];
  }
  __syncthreads();
  const double* sXl = sX[0];
  const double* sXr = sX[1];
  for (int e = threadIdx.x; e < 2 * M * M + M; e += 2 * T) {
    if (e < M * M) {  // D' = D − U_{i−1}ᵀ X^U_{i−1} − U_i X^L_{i+1}
      const int r = e / M, c = e % M;
      double v = L.D[(long long)i * M * M + e];
#pragma unroll 8
      for (int q = 0; q < M; ++q) v -= sUl[q * M + r] * sXl[q * NC + M + c] + sUi[r * M + q] * sXr[q * NC + c];
      Ln.D[(long long)in * M * M + e] = v;
    } else if (e < 2 * M * M) {  // U' = −U_i X^U_{i+1}
      const int f = e - M * M, r = f / M, c = f % M;
      double v = 0.0;
#pragma unroll 8
      for (int q = 0; q < M; ++q) v -= sUi[r * M + q] * sXr[q * NC + M + c];
      Ln.U[(long long)in * M * M + f] = right ? v : 0.0;
    } else {  // b'
      const int r = e - 2 * M * M;
      double v = L.b[(long long)i * M + r];
#pragma unroll 8
      for (int q = 0; q < M; ++q) v -= sUl[q * M + r] * sXl[q * NC + 2 * M] + sUi[r * M + q] * sXr[q * NC + 2 * M];
      Ln.b[(long long)in * M + r] = v;
    }
  }
}

// Wave-level variant for super-rows of ≤ 31 unknowns (B ≤ 5 keyframes), where [D | one coupling block | b] fits one
// wave: lane c < M holds column c of D, lanes M…2M−1 the coupling block's columns, lane 2M b.  The pivot columns are
// then always in the elimination's own wave: the pivot lanes publish them to a per-wave LDS buffer and every lane
// reads them back with no s_barrier (LDS operations of one wave are processed in order).  Measured
// (tools/micro/cr_level_timing.hip, M = 24): 17.0 → 14.5 µs per level launch with 2-column pivots (13.0 with the
// rebuild on the matrix cores, below); 4-column pivot blocks (6 publish/read round trips instead of 12): C4 step
// 0.228 → 0.216 ms per LM iteration (8-column blocks: 0.216-0.220, their per-lane 8×8 solve costs what the saved
// round trips gain).
#ifndef PBA_CR_PIVOT
#define PBA_CR_PIVOT 4
#endif
constexpr int kCrPivot = PBA_CR_PIVOT;  // columns per Gauss-Jordan step of gj_wave (1, 2, 4 or 8; divides M)

// Loads of the rows a launch wrote itself (COH: the last PCR level's solve reads the rows its own workgroup has just
// stored, cr_level_wave_kernel): `sc1` (L1-bypassing) agent-scope loads; plain otherwise.
template <bool COH>
__device__ __forceinline__ double ld_row(const double* p) {
  if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}

// Pivot blocks of PB columns: lanes k … k+PB−1 publish their columns to the wave's LDS buffer (row r: PB doubles),
// every lane reads the PB×PB pivot block P and solves P t = a[k … k+PB−1] in registers (unpivoted Gauss-Jordan:
// D is SPD, so is every pivot block; all of P's pivots must be positive), then updates its other rows
// a[r] −= Σ_j piv[r][j] t_j.  The publish / read round trip is paid M/PB times instead of M/2 times; the updates are
// the same FMAs.
// b: NB right-hand-side columns, row-major (row r of column q at b[r·NB + q]); lanes 2M … M + ncol − 1 take them.
template <int M, bool COH = false, int PB = kCrPivot, int NB = 1>
__device__ __forceinline__ bool gj_wave(const double* __restrict__ D, const double* __restrict__ R1, bool r1_trans,
                                        const double* __restrict__ b, int ncol, int c, double* piv, double* a) {
  static_assert(M % PB == 0, "pivot blocks tile the system");
  // column c of [D | R1 | b] as base + r·stride: one address choice per lane, then M unconditional loads in flight
  // together (a lane without a column reads D's and keeps zeros)
  const double* base = D + min(c, M - 1);
  int stride = M;
  bool zero = c >= M + ncol;
  if (c >= M && c < 2 * M) {
    if (R1) {
      base = r1_trans ? R1 + (c - M) * M : R1 + (c - M);
      stride = r1_trans ? 1 : M;
    } else {
      zero = true;
    }
  } else if (c >= 2 * M && c < M + ncol) {
    if (b) {
      base = b + (c - 2 * M);
      stride = NB;
    } else {
      zero = true;
    }
  }
#pragma unroll
  for (int r = 0; r < M; ++r) a[r] = ld_row<COH>(base + r * stride);
#pragma unroll
  for (int r = 0; r < M; ++r) a[r] = zero ? 0.0 : a[r];
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
    // every pivot row of the step read at once (the pivot block's rows first): the 24·PB broadcast reads are in flight
    // during the PB×PB solve instead of one or two at a time between the update FMAs (the update was LDS-latency
    // bound: ~2200 cycles per step)
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
#pragma unroll
    for (int i = 0; i < PB; ++i) {  // t ← P⁻¹ t
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


// Rebuild of super-row i (next-level index in) from the two eliminations in LDS (sXl = X_{i−1}, sXr = X_{i+1}) and
// U_{i−1}, U_i, D_i, b_i, on RB waves: 4 waves take two column tiles each, 8 waves one.  keep_u: the rebuilt row
// still has a right coupling.  Waves w ≥ RB return at once.
template <int M, int RB, int NB = 1>
__device__ __forceinline__ void cr_rebuild(int w, int lane, const double* sUl, const double* sUi, const double* sD,
                                           const double* sb, const double* sXl, const double* sXr, const CrLevel& Ln,
                                           int in, bool keep_u) {
  constexpr int NC = 2 * M + NB;  // [D | U | b] columns: b's NB columns at 2M …
  static_assert(NC <= 64, "four column tiles");
  // Rebuild of row i on the matrix cores: [D' | U' | b'] = [D | 0 | b] − U_{i−1}ᵀ·[X^U_{i−1} | 0 | X^b_{i−1}]
  // − U_i·X_{i+1}, as 2 × 4 output tiles of v_mfma_f64_16x16x4f64 (rows padded to 32, columns to 64).  Wave w takes
  // row tile w & 1 and column tiles TPW·(w >> 1) + {0 … TPW−1}: a wave's tiles share the A operands and run as
  // independent accumulator chains.  Layouts (tools/micro/mfma_f64_layout.hip): A lane l = (row l%16, k l/16),
  // B lane l = (k l/16, column l%16), accumulator entry v of lane l = (row l/16 + 4v, column l%16).
  // 3.9 → 2.7 µs per level against the scalar LDS products (tools/micro/cr_level_timing.hip, V5).
  static_assert(M % 4 == 0 && M <= 32, "K steps of 4, two row tiles");
  static_assert(RB == 4 || RB == 8, "2 × 4 tiles over the rebuild waves");
  constexpr int TPW = 8 / RB;  // column tiles per wave
  if (w >= RB) return;
  const int rt = w & 1;
  const int arow = 16 * rt + (lane & 15), kq = lane >> 4;
  // every operand of the six K steps read from LDS first, at clamped (in-range) indices and with unconditional reads,
  // then the padding zeroed by selects: conditional reads were issued and waited one at a time (~2.9 µs per level)
  constexpr int KS = M / 4;
  const bool aok = arow < M;
  const int ar = aok ? arow : 0;
  int bcol[TPW];
  double av2[KS], av1[KS], bv2[TPW][KS], bv1[TPW][KS], cv[TPW][4];
#pragma unroll
  for (int h = 0; h < TPW; ++h) {
    bcol[h] = 16 * ((w >> 1) * TPW + h) + (lane & 15);
    const int c = bcol[h];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = 16 * rt + (lane >> 4) + 4 * v;
      cv[h][v] = c < M ? sD[min(r, M - 1) * M + c] : sb[min(r, M - 1) * NB + min(max(c - 2 * M, 0), NB - 1)];
    }
  }
#pragma unroll
  for (int s4 = 0; s4 < KS; ++s4) {
    const int q = 4 * s4 + kq;
    av2[s4] = sUi[ar * M + q];
    av1[s4] = sUl[q * M + ar];
#pragma unroll
    for (int h = 0; h < TPW; ++h) {
      const int c = bcol[h];
      bv2[h][s4] = sXr[q * NC + min(c, NC - 1)];
      bv1[h][s4] = sXl[q * NC + (c < M ? M + c : min(max(c, 2 * M), NC - 1))];
    }
  }
  v4f64 acc[TPW];
#pragma unroll
  for (int h = 0; h < TPW; ++h) {
    const int c = bcol[h];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = 16 * rt + (lane >> 4) + 4 * v;
      acc[h][v] = (r < M && (c < M || (c >= 2 * M && c < NC))) ? cv[h][v] : 0.0;
    }
  }
#pragma unroll
  for (int s4 = 0; s4 < KS; ++s4) {
    const double a2 = aok ? -av2[s4] : 0.0;
    const double a1 = aok ? -av1[s4] : 0.0;
#pragma unroll
    for (int h = 0; h < TPW; ++h) {
      const int c = bcol[h];
      const double b2 = c < NC ? bv2[h][s4] : 0.0;
      const double b1 = (c < M || (c >= 2 * M && c < NC)) ? bv1[h][s4] : 0.0;
      acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, acc[h], 0, 0, 0);
      acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[h], 0, 0, 0);
    }
  }
#pragma unroll
  for (int h = 0; h < TPW; ++h)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = 16 * rt + (lane >> 4) + 4 * v, c = bcol[h];
      if (r < M) {
        if (c < M) Ln.D[(long long)in * M * M + r * M + c] = acc[h][v];
        else if (c < 2 * M) Ln.U[(long long)in * M * M + r * M + (c - M)] = keep_u ? acc[h][v] : 0.0;
        else if (c < NC) Ln.b[((long long)in * M + r) * NB + (c - 2 * M)] = acc[h][v];
      }
    }
}

// per-wave LDS of an elimination: gj_wave's pivot columns
template <int M>
constexpr int kPivBuf = M * kCrPivot;

template <int M, int NB = 1>
constexpr size_t cr_level_wave_lds() { return sizeof(double) * (3 * M * M + M * NB + 2 * M * (2 * M + NB)); }

// One level, 4 waves per rebuilt super-row i: wave 0 eliminates its left neighbour l on [D | U_l | b] (X^U, X^b),
// waves 1 and 2 its right neighbour r on [D | U_iᵀ | b] (X^L, X^b) and [D | U_r] (X^U) — D's columns replicated per
// wave — while wave 3 parks U_l, U_i, D_i and b_i in LDS for the rebuild of row i.
//   CR  (PCR = false): i = 2·blockIdx (the even rows), l = i − 1, r = i + 1, rebuilt row i/2 of the next level; X_r
//       is stored for the back-substitution.
//   PCR (PCR = true, stride s): i = blockIdx (EVERY row), l = i − s, r = i + s, rebuilt row i of the next level
//       (couplings now at stride 2s).  Every row stays in the system, so after ⌈log2 n⌉ levels all couplings are
//       gone and x_i = D_i⁻¹ b_i (pcr_solve_kernel): no back-substitution.  A PCR level runs twice the workgroups of a
//       CR level at the same per-workgroup latency, so it is used while the rows fit one workgroup per CU.
// The D_i' are Schur complements of SPD principal submatrices ({l, i, r}), so every pivot block stays SPD.
// The level's work for row i (rebuilt as row `in` of Ln) by a 4-wave workgroup: piv = 3 × M·kCrPivot doubles, smem =
// cr_level_wave_lds<M>() bytes.
// NB > 1 (PCR only): b holds NB right-hand-side columns (row-major, b[(i·M + r)·NB + q]) — the free-intrinsics
// arrow solve's [−g | border columns] (arrow_solve).
template <int M, bool PCR, int NB = 1>
__device__ __forceinline__ void cr_wave_level(const CrLevel& L, const CrLevel& Ln, int i, int in, int s, int* status,
                                              double (*piv)[kPivBuf<M>], double* smem) {
  static_assert(2 * M + NB <= 64, "one wave per elimination");
  static_assert(PCR || NB == 1, "the back-substitution's X has one right-hand side");
  constexpr int NC = 2 * M + NB;
  double* sUl = smem;
  double* sUi = sUl + M * M;
  double* sD = sUi + M * M;
  double* sb = sD + M * M;
  double* sX[2] = {sb + M * NB, sb + M * NB + M * NC};
  const int il = i - s, ir = i + s;
  const bool left = il >= 0, right = ir < L.n;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#ifdef PBA_CR_STAMPS
  long long t0 = wall_clock64(), t1 = 0, t2 = 0;
#endif
  if (w == 3) {
    // U_l, U_i, D_i, b_i → LDS: every load in flight at once (a loop of load → LDS store pays one memory round trip
    // per element, serially: measured ~10 µs of a 12.4-µs level); missing neighbours read U_i and store zeros
    constexpr int NE = 3 * M * M + M * NB, NQ = (NE + 63) / 64;
    double v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int e = lane + 64 * q;
      const double* src = L.b + (long long)i * M * NB;
      if (e < M * M) src = L.U + (long long)(left ? il : i) * M * M + e;
      else if (e < 2 * M * M) src = L.U + (long long)i * M * M + (e - M * M);
      else if (e < 3 * M * M) src = L.D + (long long)i * M * M + (e - 2 * M * M);
      else if (e < NE) src = L.b + (long long)i * M * NB + (e - 3 * M * M);
      v[q] = *src;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int e = lane + 64 * q;
      const bool zero = (e < M * M && !left) || (e >= M * M && e < 2 * M * M && !right);
      if (e < NE) smem[e] = zero ? 0.0 : v[q];
    }
  } else {
    const int j = w == 0 ? il : ir;
    const bool has = w == 0 ? left : right;
    const int jj = has ? j : i;  // a missing neighbour eliminates a real row and contributes zeros
    const double* D = L.D + (long long)jj * M * M;
    const double* bj = L.b + (long long)jj * M * NB;
    double a[M];
    bool ok;
    if (w == 0) ok = gj_wave<M, false, kCrPivot, NB>(D, L.U + (long long)jj * M * M, false, bj, M + NB, lane, piv[0], a);
    else if (w == 1) ok = gj_wave<M, false, kCrPivot, NB>(D, L.U + (long long)i * M * M, true, bj, M + NB, lane, piv[1], a);
    else ok = gj_wave<M>(D, jj + s < L.n ? L.U + (long long)jj * M * M : nullptr, false, nullptr, M, lane, piv[2], a);
    if (!ok && has && lane == 0) atomicOr(status, 1);
    if (lane >= M && lane < 2 * M + (w == 2 ? 0 : NB)) {
      const int col = lane < 2 * M ? (w == 1 ? lane - M : lane) : lane;  // (b's columns keep their lane index)
      double* x = sX[w == 0 ? 0 : 1] + col;
#pragma unroll
      for (int r = 0; r < M; ++r) x[r * NC] = has ? a[r] : 0.0;
      if (!PCR && w != 0 && has) {  // X_{i+1} for the back-substitution
        double* X = L.X + (long long)(j / 2) * M * NC + col;
#pragma unroll
        for (int r = 0; r < M; ++r) X[r * NC] = a[r];
      }
    }
  }
#ifdef PBA_CR_STAMPS
  t1 = wall_clock64();
#endif
  __syncthreads();
#ifdef PBA_CR_STAMPS
  t2 = wall_clock64();
#endif
  cr_rebuild<M, 4, NB>(w, lane, sUl, sUi, sD, sb, sX[0], sX[1], Ln, in, PCR ? i + 2 * s < L.n : right);
#ifdef PBA_CR_STAMPS
  __syncthreads();
  const long long t3 = wall_clock64();
  if (blockIdx.x == 5 && lane == 0)
    printf("crstamp s=%d w=%d phase_end_us %.2f barrier_us %.2f rebuild_us %.2f\n", s, w, (t1 - t0) * 0.01,
           (t2 - t0) * 0.01, (t3 - t0) * 0.01);
#endif
}

// out != nullptr (the last PCR level): the workgroup then also solves its decoupled row, x_i = D'_i⁻¹ b'_i, from the
// rows it has just written (read back with L1-bypassing loads after every wave's stores completed) — pcr_solve_kernel's
// work without its launch boundary and its reload of the level (out / lim as pcr_solve_kernel).
// NB > 1: out row t = i·M + r holds the NB solution columns at out[t·ld + q].
// Several independent right-hand-side batches in one launch (the arrow solve, gridDim.y = batches): batch y reads L's
// D, U at + y·bs_du and b at + y·bs_b, writes Ln at + y·bs_n and its solution columns at out + y·NB (its own CR run
// over its own copies of the rows: the batches share only L when that is level 0).
template <int M, bool PCR, int NB = 1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void cr_level_wave_kernel(
    CrLevel L, CrLevel Ln, int s, int* status, double* __restrict__ out, int lim, int ld = 1, long long bs_du = 0,
    long long bs_b = 0, long long bs_n = 0) {
  __shared__ __attribute__((aligned(16))) double piv[3][kPivBuf<M>];
  extern __shared__ double smem[];
  if (blockIdx.y) {
    const long long y = blockIdx.y;
    L.D += y * bs_du;
    L.U += y * bs_du;
    L.b += y * bs_b;
    Ln.D += y * bs_n;
    Ln.U += y * bs_n;
    Ln.b += y * bs_n;
    if (out) out += y * NB;
  }
  const int i = PCR ? (int)blockIdx.x : 2 * (int)blockIdx.x;
  cr_wave_level<M, PCR, NB>(L, Ln, i, blockIdx.x, PCR ? s : 1, status, piv, smem);
  if (!PCR || !out) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's row stores have completed
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  double a[M];
  const bool ok = gj_wave<M, true, kCrPivot, NB>(Ln.D + (long long)i * M * M, nullptr, false, Ln.b + (long long)i * M * NB,
                                                 M + NB, lane, piv[0], a);
  if (!ok) {
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  if (lane >= 2 * M && lane < 2 * M + NB)
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (i * M + r < lim) out[((long long)i * M + r) * ld + (lane - 2 * M)] = a[r];
}

// The root super-row on one wave (lane 2M carries b; the coupling lanes are empty).
template <int M>
__global__ __launch_bounds__(64) void cr_root_wave_kernel(CrLevel L, int* status) {
  __shared__ __attribute__((aligned(16))) double piv[kPivBuf<M>];
  double a[M];
  const int lane = threadIdx.x;
  const bool ok = gj_wave<M>(L.D, nullptr, false, L.b, M + 1, lane, piv, a);
  if (!ok) {
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  if (lane == 2 * M)
#pragma unroll
    for (int r = 0; r < M; ++r) L.x[r] = a[r];
}

// The last PCR level's decoupled rows: x_i = D_i⁻¹ b_i, one wave per row; x in the level-0 layout is the step itself
// (out = the step vector, lim = 6N), else the x of the CR level the PCR levels took over from.
template <int M, int NB = 1>
__global__ __launch_bounds__(64) void pcr_solve_kernel(CrLevel L, double* __restrict__ out, int lim, int* status,
                                                       int ld = 1) {
  __shared__ __attribute__((aligned(16))) double piv[kPivBuf<M>];
  const int lane = threadIdx.x, i = blockIdx.x;
  double a[M];
  const bool ok = gj_wave<M, false, kCrPivot, NB>(L.D + (long long)i * M * M, nullptr, false, L.b + (long long)i * M * NB,
                                                  M + NB, lane, piv, a);
  if (!ok) {
    if (lane == 0) atomicOr(status, 1);
    return;
  }
  if (lane >= 2 * M && lane < 2 * M + NB)
#pragma unroll
    for (int r = 0; r < M; ++r)
      if (i * M + r < lim) out[((long long)i * M + r) * ld + (lane - 2 * M)] = a[r];
}

// The root super-row (the last level): x = D⁻¹ b.
template <int M>
__global__ __launch_bounds__(kCrOddThreads<M>) void cr_root_kernel(CrLevel L, int* status) {
  constexpr int W = 3 * M + 1;
  __shared__ __attribute__((aligned(16))) double colk[2][2][M];
  double a[M];
  const bool ok = gj_row<M>(L, 0, true, threadIdx.x, colk, a);
  if (!ok) {  // uniform: every lane saw the same pivots
    if (threadIdx.x == 0) atomicOr(status, 1);
    return;
  }
  if ((int)threadIdx.x == W - 1)
#pragma unroll
    for (int r = 0; r < M; ++r) L.x[r] = a[r];
}

// Back-substitution, level L from level L+1: x_j = X_j^b − X_j^L x_{j−1} − X_j^U x_{j+1} for the odd rows, x of the
// even rows from the next level.  Level 0's x is the step δ itself (super-row I, element R ↔ block row
// I·B + R/6, component R%6), so it is written straight into the step vector.  The small levels at the bottom
// (n ≤ kCrTailRows) run in ONE workgroup with barriers between levels — one launch instead of one per level.
constexpr int kMaxCrLevels = 26;
constexpr int kCrTailRows = 32;
struct CrLevels {
  CrLevel lv[kMaxCrLevels];
  int nl;
};

template <int M>
__device__ __forceinline__ void cr_back_row(const CrLevel& L, const double* __restrict__ xn, double* out, int t) {
  constexpr int NC = 2 * M + 1;
  const int row = t / M, r = t % M;
  double v;
  if ((row & 1) == 0) {
    v = xn[(row / 2) * M + r];
  } else {
    const double* X = L.X + (long long)(row / 2) * M * NC + r * NC;
    v = X[2 * M];
    const double* xl = xn + ((row - 1) / 2) * M;
#pragma unroll 8
    for (int c = 0; c < M; ++c) v -= X[c] * xl[c];
    if (row + 1 < L.n) {
      const double* xr = xn + ((row + 1) / 2) * M;
#pragma unroll 8
      for (int c = 0; c < M; ++c) v -= X[M + c] * xr[c];
    }
  }
  out[t] = v;
}

// one (large) level, one lane per output
template <int M>
__global__ void cr_back_kernel(CrLevel L, const double* __restrict__ xn, double* __restrict__ out, int lim) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < lim) cr_back_row<M>(L, xn, out, t);
}

// levels hi … lo (all small) in one workgroup
template <int M>
__global__ __launch_bounds__(1024) void cr_back_tail_kernel(const CrLevels C, int hi, int lo, double* __restrict__ step,
                                                            int N) {
  for (int l = hi; l >= lo; --l) {
    const CrLevel& L = C.lv[l];
    double* out = l == 0 ? step : L.x;
    const int lim = l == 0 ? 6 * N : L.n * M;
    for (int t = threadIdx.x; t < lim; t += blockDim.x) cr_back_row<M>(L, C.lv[l + 1].x, out, t);
    __syncthreads();  // this level's x is read by the next (lower) level
  }
}

// ------------------------------------------------------------------------------------------------
// Free intrinsics as an arrow system (map_utils.h:339-345)
// ------------------------------------------------------------------------------------------------
// With free intrinsics the reduced camera system is S = [A B; Bᵀ C]: A the keyframes' band (bandwidth ≤ 4 keyframes), B
// the 2·nc border frames' coupling to every keyframe (dense columns), C the border's own 12nc × 12nc block.  The skyline
// factorisation (front_solve_kernel) walks the whole system column by column — one workgroup, ~3.5 µs per keyframe,
// 3.64 ms at C4.  Eliminating the keyframes first is the same factorisation order (border last), so instead:
//   X = A⁻¹ [−g_a | B]          parallel cyclic reduction over the band, the border's 12nc columns as extra right-hand
//                               sides (cr_level_wave_kernel<24, true, kArrowNB>: [D | U | b] = 24 + 24 + 16 lanes),
//                               in batches of kArrowNB columns run side by side (gridDim.y);
//   Sc = C − BᵀX_B,  rc = −g_c − BᵀX_0,  δc = Sc⁻¹ rc     (arrow_reduce_kernel: a workgroup per product;
//                               arrow_cap_kernel: one workgroup, dense Cholesky of the ≤ 48 × 48 border system);
//   δa = X_0 − X_B δc           (arrow_back_kernel).
// The skyline S stays the assembled system (pba_gn_reduced_system, the multi-GPU export read it), g its gradient.
__global__ __launch_bounds__(256) void arrow_build_kernel(const ArrowArgs a, int batches) {
  arrow_build(a, batches, (long long)blockIdx.x * blockDim.x + threadIdx.x);
}

// kArrowSeg workgroups per product: entry e < nb(nb+1)/2 — (q1 ≥ q2) of BᵀX_B — then e − that: q1 of BᵀX_0 (nb = 12nc), a
// dot product over the T = 6nf keyframe rows; workgroup (e, g) takes segment g of the rows (thread k: rows k, k + 256, …
// of it; xor butterflies per wave, the four waves in order) → part[g·n_ent + e]; arrow_cap_kernel adds the kArrowSeg
// segments in order (a fixed order).
constexpr int kArrowSeg = 8;
__global__ __launch_bounds__(256) void arrow_reduce_kernel(const ArrowArgs a) {
  __shared__ double s_w[4];
  const int nb = 12 * a.nc, nsym = nb * (nb + 1) / 2, T = 6 * a.nf, e = blockIdx.x, g = blockIdx.y;
  const int t0 = (int)((long long)g * T / kArrowSeg), t1 = (int)((long long)(g + 1) * T / kArrowSeg);
  int q1, xc;
  if (e < nsym) {
    q1 = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while (q1 * (q1 + 1) / 2 > e) --q1;
    while ((q1 + 1) * (q1 + 2) / 2 <= e) ++q1;
    xc = 1 + (e - q1 * (q1 + 1) / 2);  // X column of q2
  } else {
    q1 = e - nsym;
    xc = 0;
  }
  const int p = a.nf + q1 / 6, c = q1 % 6;
  const double* Sp = a.S + (long long)a.row[p] * 36 + c * 6;  // border row p starts at frame 0
  double acc = 0.0;
  for (int tt = t0 + (int)threadIdx.x; tt < t1; tt += 256)
    acc += Sp[(long long)(tt / 6) * 36 + tt % 6] * a.X[(long long)tt * a.ldx + xc];
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[(long long)g * a.n_ent + e] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// The border system Sc = C − BᵀX_B, rc = −g_c − BᵀX_0, its elimination in LDS and δc = Sc⁻¹ rc (the border's part of
// the step); one workgroup.  (A one-wave form without workgroup barriers measured no faster: 15.4 → 17.0 µs at C4.)
__global__ __launch_bounds__(256) void arrow_cap_kernel(const ArrowArgs a) {
  constexpr int NBM = 12 * kArrowMaxNc;
  __shared__ double sc[NBM][NBM + 1];
  __shared__ double rc[NBM];
  __shared__ int bad;
  const int nb = 12 * a.nc, nsym = nb * (nb + 1) / 2, tid = threadIdx.x;
  if (tid == 0) bad = 0;
  for (int e = tid; e < a.n_ent; e += blockDim.x) {
    double acc = a.part[e];
    for (int g = 1; g < kArrowSeg; ++g) acc += a.part[(long long)g * a.n_ent + e];
    if (e < nsym) {
      int q1 = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while (q1 * (q1 + 1) / 2 > e) --q1;
      while ((q1 + 1) * (q1 + 2) / 2 <= e) ++q1;
      const int q2 = e - q1 * (q1 + 1) / 2;
      const int p1 = a.nf + q1 / 6, c1 = q1 % 6, p2 = a.nf + q2 / 6, c2 = q2 % 6;  // p1 ≥ p2
      const double C = a.S[((long long)a.row[p1] + (p2 - a.first[p1])) * 36 + c1 * 6 + c2];
      sc[q1][q2] = sc[q2][q1] = C - acc;
    } else {
      const int q1 = e - nsym;
      rc[q1] = -a.g[6 * (a.nf + q1 / 6) + q1 % 6] - acc;
    }
  }
  __syncthreads();
  // Gauss-Jordan on [Sc | rc] with one barrier per column (no serial triangular solves: a one-lane substitution paid an
  // LDS round trip per term, ~nb² of them — 30 µs at nb = 24): step k takes every row i ≠ k's columns j > k and rc,
  // a_ij −= a_ik·a_kj / a_kk; column k and row k are only read in step k, so the step needs no second barrier.  The
  // pivots are Gaussian elimination's (Sc is SPD: all positive), δc_i = rc_i / a_ii at the end.
  for (int k = 0; k < nb; ++k) {
    const double dkk = sc[k][k];
    if (tid == 0 && !(dkk > 0.0)) bad = 1;
    const double idk = 1.0 / fmax(dkk, 1e-300);
    const int m = nb - k;  // columns k + 1 … nb − 1, then rc
    for (int idx = tid; idx < nb * m; idx += blockDim.x) {
      const int i = idx / m, jj = idx - m * i;
      if (i == k) continue;
      const double f = sc[i][k] * idk;
      if (jj < m - 1) sc[i][k + 1 + jj] -= f * sc[k][k + 1 + jj];
      else rc[i] -= f * rc[k];
    }
    __syncthreads();
  }
  if (tid == 0 && bad) atomicOr(a.status, 2);
  __syncthreads();
  for (int q = tid; q < nb; q += blockDim.x) {
    const double v = rc[q] / fmax(sc[q][q], 1e-300);
    a.dc[q] = v;
    a.x[6 * a.nf + q] = v;
  }
}

// δa = X_0 − X_B δc, one lane per keyframe unknown.
__global__ __launch_bounds__(256) void arrow_back_kernel(const ArrowArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * a.nf) return;
  const double* Xt = a.X + (long long)t * a.ldx;
  double v = Xt[0];
  for (int q = 0; q < 12 * a.nc; ++q) v -= Xt[1 + q] * a.dc[q];
  a.x[t] = v;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// PBA_SOLVER (test hook), read on every call: the solver it forces where the system allows it
enum class ForcedSolver { none, cr, band, skyline, front };
ForcedSolver forced_solver() {
  const char* fs = getenv("PBA_SOLVER");
  if (!fs) return ForcedSolver::none;
  const std::string f(fs);
  return f == "cr" ? ForcedSolver::cr : f == "band" ? ForcedSolver::band : f == "skyline" ? ForcedSolver::skyline
       : f == "front" ? ForcedSolver::front : ForcedSolver::none;
}

// Reduced-system solver buffers for band K (0: skyline only): band input Sband (row stride (K+1)·36 + 6,
// zero outside the profile), band-Cholesky column records, cyclic-reduction levels.
int configure_solver(pba_engine* e, int K, int solver) {
  GnData& G = e->gn;
  const int nf = e->n_frames;
  hipStream_t st = e->stream;
  G.band_kernel = K;
  G.solver = solver;
  G.sband_dirty = false;
  if (K) {
    const size_t nb_ = (size_t)nf * ((K + 1) * 36 + 6);
    PBA_HIP(G.Lband.resize((size_t)nf * (K * 36 + 48)));  // column records
    PBA_HIP(G.Sband.resize(nb_));
    PBA_HIP(hipMemsetAsync(G.Sband.p, 0, nb_ * sizeof(double), st));  // positions outside the profile stay 0
  }
  G.cr_levels.clear();
  G.cr_pcr = -1;
  if (solver == SOLVER_CR) {
    const int M = 6 * K;
    // Parallel cyclic reduction takes over (wave kernel, M = 24) once the rows fit one workgroup per CU:
    // PBA_PCR_CAP overrides the row limit (0: cyclic reduction only) — the tests force the hybrid with small caps
    int cap = 0;
    if (M == 24) {
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->opt.device) != hipSuccess) cus = 0;
      cap = cus;
      if (const char* v = std::getenv("PBA_PCR_CAP")) cap = std::atoi(v);
    }
    std::vector<int> ns{(nf + K - 1) / K};
    while (ns.back() > (cap > 0 ? cap : 1)) ns.push_back((ns.back() + 1) / 2);
    if (cap > 0) G.cr_pcr = (int)ns.size() - 1;
    const int np = cap > 0 ? ns.back() : 0;
    size_t total = 2 * ((size_t)np * M * M * 2 + (size_t)np * M);
    for (int n : ns) total += (size_t)n * M * M * 2 + (size_t)n * M * 2 + (size_t)(n / 2) * M * (2 * M + 1);
    PBA_HIP(G.cr_buf.resize(total));
    size_t off = 0;
    for (int n : ns) {
      CrLevelHost L;
      L.n = n;
      L.D = off; off += (size_t)n * M * M;
      L.U = off; off += (size_t)n * M * M;
      L.b = off; off += (size_t)n * M;
      L.x = off; off += (size_t)n * M;
      L.X = off; off += (size_t)(n / 2) * M * (2 * M + 1);
      G.cr_levels.push_back(L);
    }
    for (CrLevelHost& P : G.pcr_bufs) {
      P.n = np;
      P.D = off; off += (size_t)np * M * M;
      P.U = off; off += (size_t)np * M * M;
      P.b = off; off += (size_t)np * M;
    }
    G.cr0_dirty = true;  // level 0 is set up for assemble_kernel's direct writes on first use
    G.cr0_inited = false;
  }
  return PBA_OK;
}

CrLevel pcr_level(GnData& G, int i) {  // PCR ping-pong buffer i (D, U, b of the rows of level G.cr_pcr)
  const CrLevelHost& h = G.pcr_bufs[i];
  double* base = G.cr_buf.p;
  return CrLevel{base + h.D, base + h.U, base + h.b, nullptr, nullptr, h.n};
}

// build: level 0 from Sband (cr_build_kernel); false when assemble_kernel wrote it directly
template <int M>
void cr_solve(pba_engine* e, bool build) {
  GnData& G = e->gn;
  if (cr_level_lds<M>() > 65536) {  // above the default dynamic-LDS limit (gfx950 has 160 KiB per CU)
    // the attribute is per device: set it on every solve (cheap) rather than once per process
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cr_level_kernel<M>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)cr_level_lds<M>());
  }
  const int nl = (int)G.cr_levels.size();
  CrLevel L0 = cr_level(G, 0);
  const long long nthreads = (long long)L0.n * M * M + (long long)L0.n * M;
  if (build)
    cr_build_kernel<M><<<(unsigned)((nthreads + 255) / 256), 256, 0, e->stream>>>(G.Sband.p, L0, e->n_frames,
                                                                                  G.band_kernel, G.status.p);
  // CR levels 0 … c−1 (one fused launch each: odd eliminations + even rebuild); level c is solved either by PCR
  // levels (G.cr_pcr = c) or, as the last CR level of one row, by the root kernel
  const int c = G.cr_pcr >= 0 ? G.cr_pcr : nl - 1;
  for (int l = 0; l < c; ++l) {
    CrLevel L = cr_level(G, l), Ln = cr_level(G, l + 1);
    if constexpr (2 * M + 1 <= 64) {
      cr_level_wave_kernel<M, false><<<(L.n + 1) / 2, 256, cr_level_wave_lds<M>(), e->stream>>>(L, Ln, 1, G.status.p,
                                                                                               nullptr, 0);
    } else
      cr_level_kernel<M><<<(L.n + 1) / 2, 2 * kCrOddThreads<M>, cr_level_lds<M>(), e->stream>>>(L, Ln, G.status.p);
  }
  bool solved = false;  // the step vector already written (level c = 0 solved in place)
  if constexpr (2 * M + 1 <= 64) {
    if (G.cr_pcr >= 0) {
      CrLevel src = cr_level(G, c);
      const int n = src.n;
      solved = c == 0;
      double* out = solved ? G.x.p : cr_level(G, c).x;
      const int lim = solved ? 6 * e->n_frames : n * M;
      int pi = 0;
      for (int s = 1; s < n; s *= 2, pi ^= 1) {  // the last level also solves the decoupled rows
        CrLevel dst = pcr_level(G, pi);
        const bool last = 2 * s >= n;
        cr_level_wave_kernel<M, true><<<n, 256, cr_level_wave_lds<M>(), e->stream>>>(src, dst, s, G.status.p,
                                                                                     last ? out : nullptr, lim);
        src = dst;
      }
      if (n <= 1) pcr_solve_kernel<M><<<n, 64, 0, e->stream>>>(src, out, lim, G.status.p);
    } else {
      cr_root_wave_kernel<M><<<1, 64, 0, e->stream>>>(cr_level(G, nl - 1), G.status.p);
    }
  } else {
    cr_root_kernel<M><<<1, kCrOddThreads<M>, 0, e->stream>>>(cr_level(G, nl - 1), G.status.p);
  }
  if (solved) return;
  if (c == 0) {  // a single super-row: the root's x is the step
    (void)hipMemcpyAsync(G.x.p, L0.x, sizeof(double) * 6 * e->n_frames, hipMemcpyDeviceToDevice, e->stream);
    return;
  }
  CrLevels C{};
  C.nl = nl;
  for (int l = 0; l < nl; ++l) C.lv[l] = cr_level(G, l);
  int lo = c;  // the tail: levels c−1 … lo with at most kCrTailRows super-rows, in one workgroup
  while (lo > 0 && C.lv[lo - 1].n <= kCrTailRows) --lo;
  if (lo <= c - 1) cr_back_tail_kernel<M><<<1, 1024, 0, e->stream>>>(C, c - 1, lo, G.x.p, e->n_frames);
  for (int l = lo - 1; l >= 0; --l) {
    const int lim = l == 0 ? 6 * e->n_frames : C.lv[l].n * M;
    cr_back_kernel<M><<<(lim + 255) / 256, 256, 0, e->stream>>>(C.lv[l], C.lv[l + 1].x, l == 0 ? G.x.p : C.lv[l].x, lim);
  }
}

// Free intrinsics: the arrow solve's buffers (gn_prepare; nf keyframes, nc ≤ kArrowMaxNc cameras).
int configure_arrow(pba_engine* e) {
  GnData& G = e->gn;
  constexpr int M = 24, NB = kArrowNB;
  const int nf = e->n_frames, nc = G.nc_sys, nb = 12 * nc;
  G.ar_n = (nf + 3) / 4;
  G.ar_batches = (1 + nb + NB - 1) / NB;
  // level 0: D, U (shared by the batches) and every batch's b; levels 1, 2 (ping-pong): per batch D, U, b
  const size_t lvl = (size_t)G.ar_n * M * M * 2 + (size_t)G.ar_n * M * NB;
  PBA_HIP(G.ar_buf.resize((size_t)G.ar_n * M * M * 2 + (size_t)G.ar_batches * (2 * lvl + (size_t)G.ar_n * M * NB)));
  PBA_HIP(G.ar_X.resize((size_t)6 * nf * NB * G.ar_batches));
  PBA_HIP(G.ar_part.resize((size_t)kArrowSeg * (nb * (nb + 1) / 2 + nb)));
  PBA_HIP(G.ar_dc.resize((size_t)nb));
  return PBA_OK;
}

// Batch 0's rows of arrow level k (configure_arrow's layout) and the arrow kernels' arguments.
CrLevel arrow_level(const GnData& G, int k) {
  constexpr int M = 24, NB = kArrowNB;
  const int n = G.ar_n, nbt = G.ar_batches;
  const size_t lvl = (size_t)n * M * M * 2 + (size_t)n * M * NB, nbq = (size_t)n * M * NB;
  double* p = G.ar_buf.p + (k == 0 ? 0 : (size_t)n * M * M * 2 + nbt * nbq + (size_t)(k - 1) * nbt * lvl);
  return CrLevel{p, p + (size_t)n * M * M, p + (size_t)2 * n * M * M, nullptr, nullptr, n};
}

}  // namespace

namespace pba {
namespace detail {

int configure_local_solver(pba_engine* e) {
  GnData& G = e->gn;
  const int nc = G.nc_sys;
  // solver choice: block cyclic reduction (bandwidth ≤ 8), LDS-window band Cholesky (≤ 16), skyline (any).
  // PBA_SOLVER=cr|band|skyline forces one (test hook; cr/band fall back when the bandwidth does not allow).
  const int K = nc ? 0 : band_kernel_for(G.band);  // the intrinsics border: skyline
  int solver = K && K <= 8 ? SOLVER_CR : (K ? SOLVER_BAND : SOLVER_SKYLINE);
  const ForcedSolver f = forced_solver();
  if (f == ForcedSolver::skyline) solver = SOLVER_SKYLINE;
  else if (f == ForcedSolver::band && K) solver = SOLVER_BAND;
  else if (f == ForcedSolver::cr && K && K <= 8) solver = SOLVER_CR;
  if (int rc = configure_solver(e, solver == SOLVER_SKYLINE ? 0 : K, solver)) return rc;
  G.ar_n = G.ar_batches = 0;  // free intrinsics: the arrow solve's buffers (arrow_for decides per solve)
  if (nc > 0 && nc <= kArrowMaxNc)
    if (int rc = configure_arrow(e)) return rc;
  return PBA_OK;
}

// The band solver for the exchange bandwidth K of a multi-GPU solve (without free intrinsics).
int ensure_exchange_solver(pba_engine* e, int K) {
  GnData& G = e->gn;
  if (!G.nc_sys && (G.band_kernel != K || G.solver == SOLVER_SKYLINE)) {
    const int solver = (K <= 8 && forced_solver() != ForcedSolver::band) ? SOLVER_CR : SOLVER_BAND;
    if (int rc = configure_solver(e, K, solver)) return rc;
  }
  return PBA_OK;
}

CrLevel cr_level(GnData& G, int l) {
  const CrLevelHost& h = G.cr_levels[l];
  double* base = G.cr_buf.p;
  return CrLevel{base + h.D, base + h.U, base + h.b, base + h.X, base + h.x, h.n};
}

// Level 0 of the cyclic reduction as assemble_kernel expects it: zeros (positions outside the reduced system's profile
// are never written), identity diagonal on the padding rows past the last keyframe.
int init_cr_level0(pba_engine* e) {
  GnData& G = e->gn;
  if (G.cr_levels.empty()) return PBA_OK;
  const int B = G.band_kernel, M = 6 * B, N = e->n_frames;
  const CrLevelHost& h = G.cr_levels[0];
  std::vector<double> z((size_t)h.n * M * M * 2 + (size_t)h.n * M, 0.0);  // D | U | b (contiguous: configure_solver)
  for (int I = 0; I < h.n; ++I)
    for (int R = 0; R < M; ++R)
      if (I * B + R / 6 >= N) z[(size_t)I * M * M + (size_t)R * M + R] = 1.0;
  PBA_HIP(hipMemcpyAsync(G.cr_buf.p + h.D, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));  // z is pageable and goes out of scope
  G.cr0_dirty = false;
  G.cr0_inited = true;
  return PBA_OK;
}

// Whether a free-intrinsics system of keyframe bandwidth K is solved as an arrow (arrow_solve): K ≤ 4 (super-rows of 4
// keyframes, M = 24), ≤ kArrowMaxNc cameras, and PBA_SOLVER does not force the skyline solvers ("skyline" / "front":
// the A/B tests of the three solvers).
bool arrow_for(const pba_engine* e, int K) {
  const GnData& G = e->gn;
  if (!G.nc_sys || G.nc_sys > kArrowMaxNc || K > 4 || !G.ar_n) return false;
  const ForcedSolver fs = forced_solver();
  return fs != ForcedSolver::skyline && fs != ForcedSolver::front;
}

ArrowArgs arrow_args(pba_engine* e, const double* S, const int* first, const int* row, const uint8_t* fixed) {
  GnData& G = e->gn;
  const int nb = 12 * G.nc_sys;
  return ArrowArgs{S, first, row, G.g.p, fixed, arrow_level(G, 0), G.ar_X.p, G.ar_part.p, G.ar_dc.p, G.x.p, G.status.p,
                   e->n_frames, G.nc_sys, kArrowNB * G.ar_batches, nb * (nb + 1) / 2 + nb};
}
// arrow_build's threads (level 0: D, U and every batch's right-hand sides)
long long arrow_build_threads(const GnData& G) {
  constexpr int M = 24;
  return 2LL * G.ar_n * M * M + (long long)G.ar_batches * G.ar_n * M * kArrowNB;
}

// X = A⁻¹[−g_a | B] by parallel cyclic reduction (batches of kArrowNB columns), the border system, the step into G.x
// (the kernels above).  S, first, row: the skyline system and its profile; fixed: the constant frames.
// built: level 0 is already in place (intr_cam_fin_build_kernel of the same trial).
int arrow_solve(pba_engine* e, const double* S, const int* first, const int* row, const uint8_t* fixed, bool built) {
  GnData& G = e->gn;
  constexpr int M = 24, NB = kArrowNB;
  const int nf = e->n_frames, n = G.ar_n;
  hipStream_t st = e->stream;
  const int nbt = G.ar_batches;
  const size_t lvl = (size_t)n * M * M * 2 + (size_t)n * M * NB, nbq = (size_t)n * M * NB;
  auto level = [&](int k) { return arrow_level(G, k); };
  const ArrowArgs aa = arrow_args(e, S, first, row, fixed);
  constexpr size_t lds = cr_level_wave_lds<M, NB>();
  static_assert(lds <= 65536, "default dynamic LDS limit");
  if (!built) arrow_build_kernel<<<(unsigned)((arrow_build_threads(G) + 255) / 256), 256, 0, st>>>(aa, nbt);
  // the batches' cyclic reductions side by side (gridDim.y): one launch per level whatever the number of cameras
  CrLevel src = level(0);
  if (n <= 1)
    for (int bt = 0; bt < nbt; ++bt) {
      CrLevel sb = src;
      sb.b += bt * nbq;
      pcr_solve_kernel<M, NB><<<n, 64, 0, st>>>(sb, G.ar_X.p + NB * bt, 6 * nf, G.status.p, aa.ldx);
    }
  int pi = 1;
  long long bs_du = 0, bs_b = (long long)nbq;  // level 0: shared D, U
  for (int s = 1; s < n; s *= 2, pi = 3 - pi) {  // the last level also solves the decoupled rows
    const CrLevel dst = level(pi);
    const bool last = 2 * s >= n;
    cr_level_wave_kernel<M, true, NB><<<dim3(n, nbt), 256, lds, st>>>(src, dst, s, G.status.p, last ? G.ar_X.p : nullptr,
                                                                      6 * nf, aa.ldx, bs_du, bs_b, (long long)lvl);
    src = dst;
    bs_du = bs_b = (long long)lvl;
  }
  arrow_reduce_kernel<<<dim3(aa.n_ent, kArrowSeg), 256, 0, st>>>(aa);
  arrow_cap_kernel<<<1, 256, 0, st>>>(aa);
  arrow_back_kernel<<<(6 * nf + 255) / 256, 256, 0, st>>>(aa);
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

// Band solvers on G.Sband (block cyclic reduction for K ≤ 8, LDS-window band Cholesky for K = 16).
int band_solve(pba_engine* e, bool build) {
  GnData& G = e->gn;
  if (G.solver == SOLVER_CR) {
    if (G.band_kernel == 4) cr_solve<24>(e, build);
    else cr_solve<48>(e, build);
  } else {
    launch_band_cholesky(e);
  }
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

}  // namespace detail
}  // namespace pba
