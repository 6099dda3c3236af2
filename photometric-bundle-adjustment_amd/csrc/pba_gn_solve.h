// pba_gn_solve.h — the reduced-system solvers of a Gauss-Newton trial, as the rest of the GN code (pba_gn.hip) sees them:
// pba_gn_solve_sky.hip (skyline, front and band Cholesky) and pba_gn_solve_cr.hip (block / parallel cyclic reduction, the
// free-intrinsics arrow, the solver choice).  Only what crosses a unit boundary is here.
#pragma once

#include <vector>

#include "pba_internal.h"

namespace pba {
namespace detail {

// One level of the block cyclic reduction (pba_gn_solve_cr.hip).  assemble_kernel and import_kernel (pba_gn.hip) write
// level 0 directly.
struct CrLevel {
  double* D;   // n × m²
  double* U;   // n × m²   (U of the last row = 0)
  double* b;   // n × m
  double* X;   // ⌊n/2⌋ × m × (2m+1)
  double* x;   // n × m
  int n;
};

// The arrow solve of a free-intrinsics system (pba_gn_solve_cr.hip, "Free intrinsics as an arrow system").
constexpr int kArrowNB = 16;   // right-hand-side columns per cyclic-reduction run (2·24 + 16 = 64 lanes)
constexpr int kArrowMaxNc = 4; // border of ≤ 48 unknowns (arrow_cap_kernel's LDS system)

struct ArrowArgs {
  const double* S;       // skyline system (lower blocks; block (i, j) at (row[i] + j − first[i])·36, element r·6 + c)
  const int* first;
  const int* row;
  const double* g;       // gradient, 6 per system frame
  const uint8_t* fixed;  // constant keyframes (their border coupling is dropped: identity rows of S)
  CrLevel L0;            // level 0 of the band (D, U, b of kArrowNB columns)
  double* X;             // 6·nf rows × ldx: A⁻¹[−g_a | B]
  double* part;          // kArrowSeg × n_ent partial products (arrow_reduce_kernel)
  double* dc;            // the border step (12nc)
  double* x;             // the step, 6 per system frame
  int* status;
  int nf, nc, ldx, n_ent;
};

// Device code of two units (arrow_build_kernel; intr_cam_fin_build_kernel in pba_gn_intr.hip), hence in the header:
// level 0 of the band (super-rows of 4 keyframes, identity padding past the last keyframe) and the batch's kArrowNB
// right-hand-side columns: global column 0 = −g_a, 1 + q = column q of B (border frame nf + q/6, component q % 6),
// B[6f + r][q] = S(border row, keyframe f)[q % 6][r].  Every batch's columns in one launch: batch bt's b at
// L0.b + bt·n·M·kArrowNB (the batches share level 0's D and U).
__device__ __forceinline__ void arrow_build(const ArrowArgs& a, int batches, long long tid) {
  constexpr int M = 24, B = 4, NB = kArrowNB;
  const int n = a.L0.n;
  if (tid == 0) *a.status = 0;
  auto blk = [&](int i, int j, int r, int c) -> double {  // S[6i + r][6j + c], i ≥ j, 0 outside the profile
    return j >= a.first[i] ? a.S[((long long)a.row[i] + (j - a.first[i])) * 36 + r * 6 + c] : 0.0;
  };
  const long long nDU = (long long)n * M * M;
  if (tid < 2 * nDU) {
    const bool isU = tid >= nDU;
    const long long e0 = isU ? tid - nDU : tid;
    const int I = (int)(e0 / (M * M)), e = (int)(e0 % (M * M)), R = e / M, C = e % M;
    const int i = I * B + R / 6, r = R % 6, c = C % 6;
    double v;
    if (!isU) {
      const int j = I * B + C / 6;
      if (i >= a.nf || j >= a.nf) v = (i == j && r == c) ? 1.0 : 0.0;
      else v = i >= j ? blk(i, j, r, c) : blk(j, i, c, r);
      a.L0.D[e0] = v;
    } else {
      const int j = (I + 1) * B + C / 6;
      a.L0.U[e0] = (I + 1 < n && i < a.nf && j < a.nf) ? blk(j, i, c, r) : 0.0;
    }
    return;
  }
  const long long t = tid - 2 * nDU;
  if (t >= (long long)batches * n * M * NB) return;
  const int q = (int)(t % NB), R = (int)((t / NB) % M), I = (int)((t / ((long long)NB * M)) % n);
  const int batch = (int)(t / ((long long)n * M * NB));
  const int i = I * B + R / 6, r = R % 6, gq = NB * batch + q;
  double v = 0.0;
  if (i < a.nf && !a.fixed[i]) {
    if (gq == 0) v = -a.g[6 * i + r];
    else if (gq <= 12 * a.nc) v = blk(a.nf + (gq - 1) / 6, i, (gq - 1) % 6, r);
  }
  a.L0.b[t] = v;
}

inline int band_kernel_for(int band) { return band <= 4 ? 4 : (band <= 8 ? 8 : (band <= 16 ? 16 : 0)); }

// ---- pba_gn_solve_cr.hip ----
// gn_prepare: the local system's solver (by bandwidth, or PBA_SOLVER's) and its buffers, the arrow's with free intrinsics
int configure_local_solver(pba_engine* e);
int ensure_exchange_solver(pba_engine* e, int K);
CrLevel cr_level(GnData& G, int l);
int init_cr_level0(pba_engine* e);
int band_solve(pba_engine* e, bool build = true);
bool arrow_for(const pba_engine* e, int K);
ArrowArgs arrow_args(pba_engine* e, const double* S, const int* first, const int* row, const uint8_t* fixed);
long long arrow_build_threads(const GnData& G);
int arrow_solve(pba_engine* e, const double* S, const int* first, const int* row, const uint8_t* fixed,
                bool built = false);

// ---- pba_gn_solve_sky.hip ----  (the profile vectors: skyline_profile, pba_gn_plan.h)
int build_front_plan(const std::vector<int>& first, const std::vector<int>& rowp, const std::vector<int>& ccptr,
                     const std::vector<int>& ccrows, hipStream_t st, FrontPlan& P, bool use);
void launch_band_cholesky(pba_engine* e);  // band_solve's SOLVER_BAND case: band_solve_kernel<G.band_kernel> on G.Sband

// A skyline system — the local one (G.S, G.sky_*, G.front) or a multi-GPU free-intrinsics solve's summed one (G.dS,
// G.dsky_*, G.dfront) — and its solve into G.x: as an arrow (built: level 0 is in place, intr_cam_fin_build_kernel wrote it
// in this trial), else by front_solve_kernel when the plan fits LDS, else S → L and skyline_solve_kernel.
struct SkylineSystem {
  const double* S;
  double* L;
  const int *first, *row, *last, *colptr, *colrows;
  FrontPlan& front;
  const uint8_t* fixed;  // the constant frames
  int N, n_blocks;       // block rows; blocks of S
};
enum class ArrowUse { none, build, built };
int skyline_solve(pba_engine* e, const SkylineSystem& s, ArrowUse arrow);

}  // namespace detail
}  // namespace pba
