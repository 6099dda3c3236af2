// pba_gn.hip — the stages of an on-device Gauss-Newton / Levenberg-Marquardt trial for the photometric (and geometric)
// BA problem: point elimination, assembly, update, multi-GPU export / import, and the host-driven entry points
// (pba_gn_step*, pba_gn_linearize, …).  The LM driver that strings them into trials (the loop, the decision kernels,
// pba_solve*) is pba_gn_lm.hip; pba_gn_lm.h is what the two units share.
//
// Replaces the reference's per-iteration CPU work after the cost functors: the Jacobian writer and
// gradient accumulation (program_evaluator.h:233-257), the Schur eliminator + reduced camera system
// Cholesky of SPARSE_SCHUR (schur_complement_solver.cc:138-146; Schur structure <2,1,6>), and the
// Levenberg-Marquardt trust-region loop (trust_region_minimizer.cc, levenberg_marquardt_strategy.cc).
//
// Pipeline of one single-GPU LM trial (all on the engine stream; DESIGN.md §3 has the measured times):
//   schur_gate_kernel      the previous trial's accept; only for a buffer set flagged degenerate, the λ-specific point
//                          elimination (schur_chunk) — else the λ-free partials below are used.
//   assemble_kernel        one lane (four for the long lists) per element of the reduced camera system S and of g:
//                          fixed-order fp64 sums of the partial slots, + λ·clamp(diag) (Ceres' LM diagonal), identity
//                          rows for constant frames; writes cyclic reduction's level 0 directly.
//   cr_level_wave_kernel   block (parallel) cyclic reduction, one launch per level (band ≤ 8); band_solve_kernel
//                          (band ≤ 16); front_solve_kernel (any profile: loop closures, the free-intrinsics border —
//                          the active front in LDS) or skyline_solve_kernel (global memory).  Cyclic reduction, the
//                          arrow solve of free intrinsics and the solver choice: pba_gn_solve_cr.hip; the band, front
//                          and skyline Cholesky: pba_gn_solve_sky.hip; what this unit calls of them: pba_gn_solve.h.
//   update_kernel          T ← T·exp(δ) (Sophus SE3::exp, fp64), δρ = −(g_ρ + Σ W_aᵀ δ_a)/H'_ρρ, the LM model
//                          decrease ½(λ δᵀDδ − gᵀδ) and the candidate pair table, in one launch.
//   linearize_adj_kernel   at the candidate (photometric, ≤ 32 px): rows of 8 lanes per block, the target's 8-column
//                          products on 4×4×4 fp64 matrix-core tiles, host blocks through the pair's adjoint, chunk
//                          partial slots (fp64) and 8 doubles of point data per block; linearize_kernel: the
//                          14-column form (geometric rows, PBA_LIN_LEGACY).  Both in pba_gn_linearize.hip.
//   schur_free_decide_kernel  the λ-free point elimination of the new linearisation (P/(1 + λ) in the assembly) and,
//                          in 16 workgroups counted in by an atomic, the fixed-order trial sums and Ceres' decision
//                          (trial_sums, lm_decide: pba_gn_lm.h).
// Free intrinsics add intr_rows_kernel and the border kernels (intr_border_*) after the elimination: pba_gn_intr.hip,
// called through pba_gn_intr.h (only AcceptCopy and intr_update_frame, fused into kernels of this unit, are here);
// several GPUs exchange the per-rank systems (export_band_kernel, import_kernel / import_sky_kernel; the dist_* kernels
// of their decision are pba_gn_lm.hip's).
// The index structures all of these read — GN order, chunks, slot offsets, skyline profile, contribution and border
// lists — come from the host-only symbolic analysis build_gn_plan (pba_gn_plan.cpp); gn_prepare uploads them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "pba_gn.h"
#include "pba_gn_intr.h"
#include "pba_gn_lm.h"
#include "pba_gn_solve.h"

using namespace pba;
using namespace pba::detail;

namespace {

struct SchurArgs {
  const int4* desc;       // first GN point, n points, n local poses, partial offset (doubles)
  const int4* aux;        // pair list offset, n pairs, first GN block, n blocks (the last two: diagnostics)
  const uchar2* pairs;    // (a, b) local pose pairs, a ≤ b
  const int2* pt_fb;       // chunk c's point p → {first GN block, block count} at c · SCHUR_PTS + p (padded table)
  const uint8_t* blk_lv;
  const double* blk_schur;
  const double* blk_schur1;  // buffer set 1 (device LM loop)
  double* part_schur;
  double* pt_data;        // per GN point [H_ρρ, g_ρ, W_h(6)] (undamped)
  int n_chunks;
  const double* lm;       // LM record (λ, set; the loop's or GnData::lm_idle)
  // device LM loop: the previous trial's accept (state ← candidate when the record says accepted), done here by the
  // workgroups before their chunks instead of by a launch of its own; poses == nullptr: nothing to apply
  double* poses = nullptr;
  const double* poses_new = nullptr;
  double* rho = nullptr;
  const double* rho_new = nullptr;
  const int* pt_orig = nullptr;
  int n_pose_d = 0, n_gn_points = 0;
  const double* pair_rt;   // per pair [R_th, t_th] of the linearisation in blk_schur / blk_schur1 (W_h = −W_t·Ad)
  const double* pair_rt1;
  const int4* lvp4;        // per chunk: the pairs of local targets 1 … 4
  const int* lvp;          // all of them (from aux.z), for chunks of > 5 local poses
  int rt_off;              // R, t at the start of the dynamic LDS (doubles); W after it
  // free intrinsics (single-GPU LM loop): the previous trial's accept also copies the candidate intrinsics (the copies of
  // intr_accept_kernel, 8 per camera) — k_d == nullptr: not here
  const double* knew_d = nullptr;
  const float* knew_f = nullptr;
  double* k_d = nullptr;
  float* k_f = nullptr;
  int n_intr = 0;
};

// ------------------------------------------------------------------------------------------------
// schur_kernel: point elimination for damping λ
// ------------------------------------------------------------------------------------------------
// One Schur chunk c for damping λ: the points' H_ρρ, g_ρ, W sums from the block data of the linearisation set blk_schur,
// their point data into pt_out (nullptr: not stored), and the chunk's partial slots into part_out.  degen != nullptr (the
// λ-free pass of the device LM loop, λ = 0): set to 1 when a point's H_ρρ lies outside the LM diagonal's clamp [1e-6, 1e32]
// (H = 0 excepted: such a point has W = 0) — only inside it is H + λ·clamp(H) = (1 + λ)·H, the identity the λ-free pass
// relies on (schur_free_decide_kernel).
// A chunk's descriptors and point records: the first loads of its elimination (schur_head), separate so that a kernel
// can issue them in one memory round with loads of its own (schur_free_decide_kernel: the record and the set).
constexpr int kPtIter = (SCHUR_PTS + kBlockThreads / 4 - 1) / (kBlockThreads / 4);
struct SchurHead {
  int4 d, ax, lp4;
  int2 prec[kPtIter];
};
__device__ __forceinline__ SchurHead schur_head(const SchurArgs& g, int c) {
  SchurHead h;
  h.d = g.desc[c];
  h.ax = g.aux[c];
  h.lp4 = g.lvp4[c];
#pragma unroll
  for (int it = 0; it < kPtIter; ++it)
    h.prec[it] = g.pt_fb[(long long)c * SCHUR_PTS + it * (kBlockThreads / 4) + (threadIdx.x >> 2)];
  return h;
}
// The host block of W: a photometric (or geometric) row's host Jacobian is its target Jacobian through the pair's
// adjoint, J_h = −J_t·Ad with Ad = [[R, [t]×R], [0, R]] (R = R_th, t = t_th; linearize_adj_kernel), so
// W_h = J_ρᵀJ_h = −Σ_targets W_t·Ad = −Σ_lv [W_tv·R, (W_tv × t + W_tw)·R] over the point's per-target sums W[p][lv]: the
// blocks carry W_t alone (8 doubles of point data instead of 16).  Point p, all six components (one thread per point:
// per component, the reads of W and R, t were a third of the work); rt: the local targets' [R(9), t(3)] in LDS.
__device__ __forceinline__ void host_w(const double (*W)[6], const double* rt, int p, int nv, double* out) {
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int l = 1; l < nv; ++l) {
    const double2* w2 = reinterpret_cast<const double2*>(W[p * nv + l]);
    const double2* r2 = reinterpret_cast<const double2*>(rt + 12 * (l - 1));
    double w[6], R[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double2 x = w2[i];
      w[2 * i] = x.x;
      w[2 * i + 1] = x.y;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double2 x = r2[i];
      R[2 * i] = x.x;
      R[2 * i + 1] = x.y;
    }
    const double* t = R + 9;
    const double u0 = w[1] * t[2] - w[2] * t[1] + w[3], u1 = w[2] * t[0] - w[0] * t[2] + w[4],
                 u2 = w[0] * t[1] - w[1] * t[0] + w[5];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] += w[0] * R[c] + w[1] * R[3 + c] + w[2] * R[6 + c];
      v[3 + c] += u0 * R[c] + u1 * R[3 + c] + u2 * R[6 + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) out[c] = -v[c];
}
__device__ __forceinline__ void schur_chunk(const SchurArgs& g, const SchurHead& h, double lambda,
                                            const double* __restrict__ blk_schur, const double* __restrict__ pair_rt,
                                            double* __restrict__ part_out, double* __restrict__ pt_out, int* degen,
                                            double* W_dyn, double* s_inv, double* s_gl) {
  const int4 d = h.d;
  const int4 ax = h.ax;
  const int2* prec = h.prec;
  const int first = d.x, npt = d.y, nv = d.z, poff = d.w;
#ifdef PBA_FD_STAMPS
  const long long ts0 = wall_clock64();
  long long ts1 = 0, ts2 = 0, tsa = 0, tsb = 0, tsc = 0;
  auto stamp_out = [&](const char* tag) {
    const int b = blockIdx.x;
    if (threadIdx.x == 0 && (b == 17 || b == 300 || b == 600 || b == 1000))
      printf("fdphase b=%d %s zero %lld acc %lld presync %lld sync %lld wh %lld total %lld\n", b, tag, ts1 - ts0,
             tsa - ts0, tsb - ts0, tsc - ts0, ts2 - ts0, wall_clock64() - ts0);
  };
#endif
  double* const rt = W_dyn;  // the local targets' R_th, t_th (12 each)
  double (*W)[6] = reinterpret_cast<double (*)[6]>(W_dyn + g.rt_off);
  for (int i = threadIdx.x; i < npt * nv * 6; i += kBlockThreads) (&W[0][0])[i] = 0.0;
  __syncthreads();
#ifdef PBA_FD_STAMPS
  ts1 = wall_clock64();
#endif
  // the targets' R, t: loaded beside the block data (the first four pairs came with the descriptors; a chunk of more
  // local poses reads its pair list first), stored to LDS after the accumulation
  double rtv[2];
  int rti[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = threadIdx.x + u * kBlockThreads, l = i / 12;
    rti[u] = i < 12 * (nv - 1) ? i : -1;
    int pr = 0;
    if (rti[u] >= 0) pr = l < 4 ? (l == 0 ? h.lp4.x : l == 1 ? h.lp4.y : l == 2 ? h.lp4.z : h.lp4.w) : g.lvp[ax.z + l];
    rtv[u] = rti[u] >= 0 ? pair_rt[(long long)pr * 12 + (i - 12 * l)] : 0.0;
  }
  // four lanes per point, each summing one 16-B load per block of the point's blocks' 8-value records in block order:
  // q = 0: H_ρρ, g_ρ   q = 1, 2, 3: W_t[0..1], [2..3], [4..5] → W[p][lv] (staging the chunk's records in LDS
  // block-parallel instead measured slower: 23 → 35 µs at C4, its LDS halves the resident workgroups)
  bool bad = false;
  const int q = threadIdx.x & 3;
  // the first kFirst blocks of both of the lane's points in ONE memory round (a point's block loop per point cost a
  // round each), the rest of a point's blocks (more than kFirst observations) in batches after
  constexpr int kFirst = 4, kBatch = 8;
  double2 v0[kPtIter][kFirst];
  int lv0[kPtIter][kFirst];
#pragma unroll
  for (int it = 0; it < kPtIter; ++it) {
    const int fb = prec[it].x, nb = max(prec[it].y, 1);
#pragma unroll
    for (int u = 0; u < kFirst; ++u) {
      const int b = fb + min(u, nb - 1);
      v0[it][u] = reinterpret_cast<const double2*>(blk_schur + (long long)b * kPd)[q];
      lv0[it][u] = q == 0 ? 0 : g.blk_lv[b];
    }
  }
#ifdef PBA_FD_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  tsa = wall_clock64();
#endif
#pragma unroll
  for (int it = 0; it < kPtIter; ++it) {
    const int p = it * (kBlockThreads / 4) + (threadIdx.x >> 2), gp = first + p;
    if (p < npt) {
      const int fb = prec[it].x, nb = prec[it].y;
      double s0 = 0.0, s1 = 0.0;
      auto add = [&](const double2& v, int lv) {
        if (q == 0) {
          s0 += v.x;
          s1 += v.y;
        } else {
          double* wt = W[p * nv + lv] + 2 * (q - 1);
          wt[0] += v.x;
          wt[1] += v.y;
        }
      };
#pragma unroll
      for (int u = 0; u < kFirst; ++u)
        if (u < nb) add(v0[it][u], lv0[it][u]);
      for (int b0 = fb + kFirst; b0 < fb + nb; b0 += kBatch) {
        double2 v[kBatch];
        int lv[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
          const int b = min(b0 + u, fb + nb - 1);
          v[u] = reinterpret_cast<const double2*>(blk_schur + (long long)b * kPd)[q];
          lv[u] = q == 0 ? 0 : g.blk_lv[b];
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u)
          if (b0 + u < fb + nb) add(v[u], lv[u]);
      }
      if (q == 0) {
        const double D = fmin(fmax(s0, 1e-6), 1e32);
        const double Hd = s0 + lambda * D;
        s_inv[p] = Hd > 0.0 ? 1.0 / Hd : 0.0;
        s_gl[p] = s1;
        bad = s0 != 0.0 && !(s0 >= 1e-6 && s0 <= 1e32);
        if (pt_out) {
          pt_out[(long long)gp * 8] = s0;
          pt_out[(long long)gp * 8 + 1] = s1;
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (rti[u] >= 0) rt[rti[u]] = rtv[u];
  for (int i = threadIdx.x + 2 * kBlockThreads; i < 12 * (nv - 1); i += kBlockThreads)  // (> 43 local poses)
    rt[i] = pair_rt[(long long)g.lvp[ax.z + i / 12] * 12 + i % 12];
#ifdef PBA_FD_STAMPS
  tsb = wall_clock64();
#endif
  if (degen && __syncthreads_or(bad) && threadIdx.x == 0) atomicOr(degen, 1);
  __syncthreads();
#ifdef PBA_FD_STAMPS
  tsc = wall_clock64();
#endif
  for (int p = threadIdx.x; p < npt; p += kBlockThreads) {  // W_h = W[p][0] from the targets' sums
    double v[6];
    host_w(W, rt, p, nv, v);
#pragma unroll
    for (int c = 0; c < 6; ++c) W[p * nv][c] = v[c];
    if (pt_out)
#pragma unroll
      for (int c = 0; c < 6; ++c) pt_out[(long long)(first + p) * 8 + 2 + c] = v[c];
  }
  __syncthreads();
#ifdef PBA_FD_STAMPS
  ts2 = wall_clock64();
#endif
  if (nv * 6 + 1 <= 32) {
    // ≤ 5 local poses (a temporal window): the chunk's sums are one small GEMM on the matrix cores,
    // C = (W·diag(1/H'_ρρ))ᵀ [W | g_ρ] over its points (K = points, 4 per v_mfma_f64_16x16x4f64 step), 32 × 32 in
    // four 16 × 16 tiles, one per wave; C's 6 × 6 blocks (a, b) of the used pose pairs and its column nv·6 (the
    // gradient terms) are the partial slots.  Layouts as in cr_level_wave_kernel: A lane l = (row l%16, k l/16),
    // B lane l = (k l/16, column l%16), accumulator entry v of lane l = (row l/16 + 4v, column l%16).
    const int nv6 = nv * 6;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ti = wv & 1, tj = wv >> 1;
    const int ca = 16 * ti + (lane & 15), cb = 16 * tj + (lane & 15), kq = lane >> 4;
    const double* Wf = &W[0][0];
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
    // four K steps per batch: the batch's LDS reads first, at clamped indices with unconditional reads, the padding
    // zeroed by selects afterwards (conditional reads were issued and waited one step at a time)
    constexpr int KB = 4;
    const int cac = min(ca, nv6 - 1), cbc = min(cb, nv6 - 1);
    for (int p0 = 0; p0 < npt; p0 += 4 * KB) {
      double wa[KB], wb[KB], si[KB], sg[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const int pc = min(p0 + 4 * u + kq, npt - 1);
        wa[u] = Wf[pc * nv6 + cac];
        wb[u] = Wf[pc * nv6 + cbc];
        si[u] = s_inv[pc];
        sg[u] = s_gl[pc];
      }
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const bool pin = p0 + 4 * u + kq < npt;
        const double av = (pin && ca < nv6) ? wa[u] * si[u] : 0.0;
        const double bv = !pin ? 0.0 : (cb < nv6 ? wb[u] : (cb == nv6 ? sg[u] : 0.0));
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = 16 * ti + (lane >> 4) + 4 * v;
      if (r >= nv6) continue;
      if (cb < nv6) {
        // canonical pair order (gn_prepare): (0,0) (0,1) … (0,nv−1) (1,1) …; blocks of unused pairs are zero
        const int pa_ = r / 6, pb_ = cb / 6;
        const int u = pa_ * nv - pa_ * (pa_ - 1) / 2 + (pb_ - pa_);
        if (pa_ <= pb_) part_out[(long long)poff + u * 36 + (r % 6) * 6 + cb % 6] = acc[v];
      } else if (cb == nv6) {
        part_out[(long long)poff + ax.y * 36 + r] = acc[v];
      }
    }
#ifdef PBA_FD_STAMPS
    stamp_out("mfma");
#endif
    return;
  }
  const int nout = ax.y * 36 + nv * 6;
  for (int o = threadIdx.x; o < nout; o += kBlockThreads) {
    double acc = 0.0;
    if (o < ax.y * 36) {
      const uchar2 ab = g.pairs[ax.x + o / 36];
      const int r = (o % 36) / 6, cc = o % 6;
      for (int p = 0; p < npt; ++p)
        acc += W[p * nv + ab.x][r] * W[p * nv + ab.y][cc] * s_inv[p];
    } else {
      const int q = o - ax.y * 36, a = q / 6, r = q % 6;
      for (int p = 0; p < npt; ++p) acc += W[p * nv + a][r] * s_gl[p] * s_inv[p];
    }
    part_out[(long long)poff + o] = acc;
  }
}

// The accept of the device LM loop's previous trial (state ← candidate when the record says accepted; the copies of
// lm_accept_kernel): one element per thread, a grid-stride tail beyond the grid.  Loads first (with the kernel's first
// loads), stores after the kernel's own stores (loads and stores share vmcnt).
struct AcceptCopy {
  bool accepted = false;
  int ia = 0, oa = 0, ka = 0;
  double pnew = 0.0, rnew = 0.0, kdnew = 0.0;
  float kfnew = 0.0f;
  __device__ __forceinline__ void load(const SchurArgs& g, const LmView& lv) {
    accepted = g.poses && lv.accept != 0.0 && lv.done == 0.0;
    ia = blockIdx.x * blockDim.x + threadIdx.x;
    if (g.poses) {
      pnew = g.poses_new[min(ia, g.n_pose_d - 1)];
      oa = g.pt_orig[min(ia, g.n_gn_points - 1)];
      rnew = g.rho_new[oa];
    }
    if (g.k_d && ia < 8 * g.n_intr) {
      ka = kCamD * (ia >> 3) + (ia & 7);
      kdnew = g.knew_d[ka];
      kfnew = g.knew_f[ia];
    }
  }
  __device__ __forceinline__ void store(const SchurArgs& g) const {
    if (!accepted) return;
    if (ia < g.n_pose_d) g.poses[ia] = pnew;
    if (ia < g.n_gn_points) g.rho[oa] = rnew;
    if (g.k_d && ia < 8 * g.n_intr) {
      g.k_d[ka] = kdnew;
      g.k_f[ia] = kfnew;
    }
    const int n = max(g.n_pose_d, g.n_gn_points);
    for (int i = ia + gridDim.x * blockDim.x; i < n; i += gridDim.x * blockDim.x) {
      if (i < g.n_pose_d) g.poses[i] = g.poses_new[i];
      if (i < g.n_gn_points) {
        const int o = g.pt_orig[i];
        g.rho[o] = g.rho_new[o];
      }
    }
  }
};

// Point elimination for damping λ (host-driven steps, the multi-GPU loop, free intrinsics): one chunk per workgroup, the
// linearisation set of the record, plus the previous trial's accept when g.poses is set.
__global__ __launch_bounds__(kBlockThreads) void schur_kernel(const SchurArgs g, double lambda) {
  extern __shared__ __attribute__((aligned(16))) double W_dyn[];  // W [points × local poses][6] (gn_prepare: schur_lds)
  __shared__ double s_inv[SCHUR_PTS], s_gl[SCHUR_PTS];
  const int c = blockIdx.x;
  if (c >= g.n_chunks) return;  // (not gated by the record's done flag: a trial after the end only wastes time here)
  // Memory rounds (each dependent one is ~1.7 µs here): 1 — the record, the chunk descriptors, the chunk's point
  // records (padded per-chunk table) and the accept copy's sources; 2 — the points' block data (and the copied ρ);
  // the accept copy's stores come last, so no load of the chunk waits behind them (loads and stores share vmcnt).
  const LmView lv = lm_view(g.lm);
  AcceptCopy ac;
  ac.load(g, lv);
  lambda = lm_lambda(lv, lambda);
  const double* const blk_schur = lv.set != 0.0 ? g.blk_schur1 : g.blk_schur;
  schur_chunk(g, schur_head(g, c), lambda, blk_schur, lv.set != 0.0 ? g.pair_rt1 : g.pair_rt, g.part_schur, g.pt_data,
              nullptr, W_dyn, s_inv, s_gl);
  ac.store(g);
}

struct AsmArgs {
  const double* part_lin;
  const double* part_lin1;  // buffer set 1 (device LM loop)
  const double* lm;        // LM record (λ, set; the loop's or GnData::lm_idle)
  const double* part_schur;
  const int* sky_cptr;
  const int2* sky_contrib;
  const int* g_cptr;
  const int2* g_contrib;
  const int* blk_i;
  const int* blk_j;
  const uint8_t* fixed;
  double* S;
  double* g;
  double* g_dir;
  double* Ddiag;
  // (the fields above and n_sky: asm_args; the rest, zero there, by name where they are used — assemble_kernel's in
  // enqueue_solve, export_band_kernel's in enqueue_export)
  double* Sband;   // optional dense band copy (block c of row i = column i − B + c), B = band
  int band;
  int n_sky;
  int n_frames;
  // optional: level 0 of the block cyclic reduction written directly (super-rows of crB keyframes: D, U, b = −g; the
  // positions outside the profile and the identity padding set once by configure_solver), which replaces cr_build's
  // pass over Sband; status (the solve's failure flag) is then cleared here
  double* crD;
  double* crU;
  double* crb;
  int crB;
  int* status;
  // the single-GPU LM loop: the current set's λ-free Schur partials (scaled by 1/(1 + λ)) unless the set is flagged
  // degen (schur_free_decide_kernel); nullptr: part_schur as it is
  const double* part_free0;
  const double* part_free1;
  const int* degen;
  const int* sky_diag;  // assemble_kernel: the diagonal blocks (long contribution lists: kAsmSeg lanes per element) …
  const int* sky_off;   // … and the off-diagonal ones (one lane)
  int n_diag;
};

// Fixed-order sums over a contribution list (total, and the part that is not a Schur term — the undamped
// JᵀJ diagonal / direct gradient).  The list entries and their values are gathered 8 at a time so eight
// independent loads are in flight per lane instead of one dependent index → value chain per term.  (16 at a time with
// the next batch's entries loaded beside the current batch's values measured slower: 12.8 → 15.0 µs at C4, 128
// VGPRs and twice the clamped loads of the short off-diagonal lists.)
constexpr int GATHER = 8;
// seg / nseg: this lane's share of the list, entries beg + seg, beg + seg + nseg, … (the caller adds the nseg lanes'
// sums in a fixed order).
__device__ __forceinline__ void contrib_sums(const AsmArgs& a, const int2* __restrict__ list, int beg, int end, int e,
                                             int et, double& sum, double& dsum, double pscale = 1.0, int seg = 0,
                                             int nseg = 1) {
  sum = dsum = 0.0;
  for (int q0 = beg + seg; q0 < end; q0 += GATHER * nseg) {
    int2 c[GATHER];
    double v[GATHER];
#pragma unroll
    for (int u = 0; u < GATHER; ++u) c[u] = list[min(q0 + u * nseg, end - 1)];
#pragma unroll
    for (int u = 0; u < GATHER; ++u) {
      // both loads unconditional (the other one at a valid dummy offset): no divergent branch, no wait
      const int off = c[u].x + ((c[u].y & C_TRANSPOSE) ? et : e);
      const bool sc = (c[u].y & C_SCHUR) != 0;
      const double vs = a.part_schur[sc ? off : 0];
      const double vl = a.part_lin[sc ? 0 : off];
      v[u] = sc ? -pscale * vs : vl;
    }
#pragma unroll
    for (int u = 0; u < GATHER; ++u) {
      if (q0 + u * nseg < end) {
        sum += v[u];
        if (!(c[u].y & C_SCHUR)) dsum += v[u];
      }
    }
  }
}
// The kAsmSeg lanes of one element (aligned groups) add their list shares: lane 0 of the group gets the total, in a
// fixed order.
constexpr int kAsmSeg = 4;
__device__ __forceinline__ void seg_total(double& sum, double& dsum) {
#pragma unroll
  for (int m = 1; m < kAsmSeg; m <<= 1) {
    sum += __shfl_xor(sum, m, 64);
    dsum += __shfl_xor(dsum, m, 64);
  }
}

// ------------------------------------------------------------------------------------------------
// assemble_kernel: S (skyline, lower blocks) and g from the partial slots
// ------------------------------------------------------------------------------------------------
__global__ void assemble_kernel(AsmArgs a, double lambda) {
  const LmView lv = lm_view(a.lm);  // (no done gate: see schur_kernel)
  const int dg0 = a.degen ? a.degen[0] : 1, dg1 = a.degen ? a.degen[1] : 1;
  lambda = lm_lambda(lv, lambda);
  if (lv.set != 0.0) a.part_lin = a.part_lin1;
  double pscale = 1.0;  // the λ-free partials of the current set: P / (1 + λ)
  if (a.degen && (lv.set != 0.0 ? dg1 : dg0) == 0) {
    a.part_schur = lv.set != 0.0 ? a.part_free1 : a.part_free0;
    pscale = 1.0 / (1.0 + lambda);
  }
  // thread ranges: the diagonal blocks' elements, kAsmSeg lanes each (their lists are the long ones: every chunk hosted
  // by or targeting the keyframe, ~30 partials at C4, four dependent memory rounds on one lane), then the off-diagonal
  // blocks' elements one lane each, then the gradient rows kAsmSeg lanes each
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int nA = a.n_diag * 36 * kAsmSeg, nS = nA + (a.n_sky - a.n_diag) * 36;
  if (tid < nS) {
    const bool dg = tid < nA;
    const int w = dg ? tid / kAsmSeg : tid - nA, seg = dg ? tid % kAsmSeg : 0;
    const int s = dg ? a.sky_diag[w / 36] : a.sky_off[w / 36], e = w % 36, r = e / 6, cc = e % 6;
    const int i = a.blk_i[s], j = a.blk_j[s];
    double sum, dsum;
    contrib_sums(a, a.sky_contrib, a.sky_cptr[s], a.sky_cptr[s + 1], r * 6 + cc, cc * 6 + r, sum, dsum, pscale, seg,
                 dg ? kAsmSeg : 1);
    if (dg) {
      seg_total(sum, dsum);
      if (seg != 0) return;
    }
    const int tid_s = s * 36 + e;  // the element's position in S
    double val = sum;
    if (a.fixed[i] || a.fixed[j]) {
      val = (i == j && r == cc) ? 1.0 : 0.0;
    } else if (i == j && r == cc) {
      const double D = fmin(fmax(dsum, 1e-6), 1e32);  // levenberg_marquardt_strategy.cc min/max diagonal
      a.Ddiag[6 * i + r] = D;
      val = sum + lambda * D;
    }
    a.S[tid_s] = val;
    if (a.Sband) a.Sband[(long long)i * ((a.band + 1) * 36 + 6) + (j - i + a.band) * 36 + e] = val;
    if (a.crD) {
      const int B = a.crB, M = 6 * B, I = i / B, J = j / B;
      const int Ri = (i % B) * 6 + r, Cj = (j % B) * 6 + cc;  // row of i's entry / column of j's in their super-rows
      if (I == J) {
        // a diagonal block's (r, cc) and (cc, r) are two lanes whose sums may differ in the last bit (the Schur
        // terms' products round differently): only the lower one writes both, so D is symmetric and the solve
        // reproducible (both lanes writing both positions left whichever stored last)
        double* D = a.crD + (long long)I * M * M;
        if (i != j || r >= cc) {
          D[Ri * M + Cj] = val;
          D[Cj * M + Ri] = val;
        }
      } else {  // I == J + 1 (bandwidth ≤ B): U_J[row of j][column of i] = S[6j+cc][6i+r]
        a.crU[(long long)J * M * M + Cj * M + Ri] = val;
      }
    }
    return;
  }
  const int tg = tid - nS, t = tg / kAsmSeg, seg = tg % kAsmSeg;
  if (t >= 6 * a.n_frames) return;
  const int i = t / 6, r = t % 6;
  double sum, dsum;
  contrib_sums(a, a.g_contrib, a.g_cptr[i], a.g_cptr[i + 1], r, r, sum, dsum, pscale, seg, kAsmSeg);
  seg_total(sum, dsum);
  if (seg != 0) return;
  a.g[t] = a.fixed[i] ? 0.0 : sum;
  if (a.Sband) a.Sband[(long long)i * ((a.band + 1) * 36 + 6) + (a.band + 1) * 36 + r] = a.fixed[i] ? 0.0 : sum;
  if (a.crD) {
    a.crb[t] = a.fixed[i] ? 0.0 : -sum;  // super-row i / B, row (i % B)·6 + r: t itself (M = 6B, rows padded after N)
    if (t == 0) *a.status = 0;
  }
  a.g_dir[t] = a.fixed[i] ? 0.0 : dsum;
  if (a.fixed[i]) a.Ddiag[t] = 0.0;
}

// ------------------------------------------------------------------------------------------------
// Multi-GPU exchange (include/pba.h): this rank's partial reduced system in the banded exchange layout,
// and the finalisation of the summed system into the band solvers' input.
// ------------------------------------------------------------------------------------------------
__host__ __device__ constexpr long long ex_row(int K) { return (long long)(K + 1) * 36 + EX_TAIL; }

// One lane per element of the exchange buffer (the local skyline's elements by the contribution lists of
// assemble_kernel, nothing damped or fixed; the pose gradients): positions outside the local profile get their zero here, so the
// buffer needs no fill launch before it (round 3: a 5-µs hipMemsetAsync of the whole band per trial).
__global__ void export_band_kernel(AsmArgs a, const uint8_t* __restrict__ observed, const int* __restrict__ sky_first,
                                   const int* __restrict__ sky_row, double* __restrict__ X, int K) {
  if (lm_view(a.lm).set != 0.0) a.part_lin = a.part_lin1;  // (no done gate: see schur_kernel)
  // lanes [0, nf·(K+1)·36): the band elements; then 24 per frame for the tails, in waves of their own (the gradient lists
  // are long: interleaved with the band's short lists they made every wave wait for them, 12 → 21 µs at C4)
  const long long RS = ex_row(K), t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int QB = (K + 1) * 36;
  const long long nB = (long long)a.n_frames * QB;
  if (t < nB) {
    const int i = (int)(t / QB), q = (int)(t - (long long)i * QB);
    const int c = q / 36, e = q % 36, r = e / 6, cc = e % 6, j = i - K + c;
    double sum = 0.0, dsum = 0.0;
    if (j >= 0 && j >= sky_first[i]) {
      const int s = sky_row[i] + (j - sky_first[i]);
      contrib_sums(a, a.sky_contrib, a.sky_cptr[s], a.sky_cptr[s + 1], r * 6 + cc, cc * 6 + r, sum, dsum);
    }
    double* row = X + (long long)i * RS;
    row[q] = sum;
    if (i == j && r == cc) row[QB + 12 + r] = dsum;  // diag(A)
    return;
  }
  const long long u = t - nB;
  if (u >= (long long)a.n_frames * EX_TAIL) return;
  const int i = (int)(u / EX_TAIL), r = (int)(u % EX_TAIL);
  double* tail = X + (long long)i * RS + QB;
  if (r < 6) {  // g and the direct gradient from one list walk
    double sum, dsum;
    contrib_sums(a, a.g_contrib, a.g_cptr[i], a.g_cptr[i + 1], r, r, sum, dsum);
    tail[r] = sum;
    tail[6 + r] = dsum;
  } else if (r >= 18) {
    tail[r] = r == 18 && observed[i] ? 1.0 : 0.0;
  }
}

struct ImportArgs {
  const double* X;         // summed exchange buffer
  const uint8_t* fixed_req;
  double* Sband;           // band solver input, row stride (K+1)·36 + 6
  double* g;
  double* g_dir;
  double* Ddiag;
  uint8_t* fixed;          // effective constant frames: requested, or observed by no rank
  int n_frames;
  int K;
  // block cyclic reduction: level 0 written directly (super-rows of K keyframes; as assemble_kernel), else Sband
  double* crD;
  double* crU;
  double* crb;
  int* status;
};

// One lane per element of the band solver input: + λ·clamp(diag(A)) (levenberg_marquardt_strategy.cc),
// identity rows/columns for constant frames — the same arithmetic as assemble_kernel on the summed system.
__global__ void import_kernel(const ImportArgs a, double lambda, const double* __restrict__ lm) {
  lambda = lm_lambda(lm_view(lm), lambda);  // the device LM record's λ (host-driven steps: the argument)
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int K = a.K;
  const long long SR = (long long)(K + 1) * 36 + 6, RS = ex_row(K);
  if (t >= SR * a.n_frames) return;
  const int i = (int)(t / SR), q = (int)(t - (long long)i * SR);
  const double* row = a.X + (long long)i * RS;
  const double* tail = row + (K + 1) * 36;
  const bool fi = a.fixed_req[i] || tail[18] == 0.0;
  if (q < (K + 1) * 36) {
    const int c = q / 36, e = q % 36, r = e / 6, cc = e % 6, j = i - K + c;
    double val = 0.0;
    if (j >= 0) {
      const bool fj = a.fixed_req[j] || a.X[(long long)j * RS + (K + 1) * 36 + 18] == 0.0;
      val = row[q];
      if (fi || fj) {
        val = (i == j && r == cc) ? 1.0 : 0.0;
      } else if (i == j && r == cc) {
        val += lambda * fmin(fmax(tail[12 + r], 1e-6), 1e32);
      }
    }
    if (!a.crD) {
      a.Sband[t] = val;
    } else if (j >= 0) {  // the (i, j) entry into level 0 (I = i / K, J = j / K, I − J ≤ 1), as assemble_kernel
      const int M = 6 * K, I = i / K, J = j / K, Ri = (i % K) * 6 + r, Cj = (j % K) * 6 + cc;
      if (I == J) {
        if (i != j || r >= cc) {  // the lower lane writes both positions (a symmetric D, reproducible)
          double* D = a.crD + (long long)I * M * M;
          D[Ri * M + Cj] = val;
          D[Cj * M + Ri] = val;
        }
      } else {
        a.crU[(long long)J * M * M + Cj * M + Ri] = val;
      }
    }
    return;
  }
  const int r = q - (K + 1) * 36;
  if (!a.crD) a.Sband[t] = fi ? 0.0 : tail[r];
  else a.crb[6 * i + r] = fi ? 0.0 : -tail[r];
  if (a.crD && t == (K + 1) * 36) *a.status = 0;  // the solve's failure flag (cr_build_kernel clears it otherwise)
  a.g[6 * i + r] = fi ? 0.0 : tail[r];
  a.g_dir[6 * i + r] = fi ? 0.0 : tail[6 + r];
  a.Ddiag[6 * i + r] = fi ? 0.0 : fmin(fmax(tail[12 + r], 1e-6), 1e32);
  if (r == 0) a.fixed[i] = fi ? 1 : 0;
}

// Free intrinsics on several GPUs: the summed exchange — the keyframes' band rows and the 2·nc border rows (the
// border region after the band, export by intr_border_all_kernel) — into the skyline system of the summed profile
// (keyframe i: columns max(0, i − K) … i; border rows: 0 … P; row offsets `row`), with the single-GPU arithmetic of
// assemble_kernel and border_store: + λ·clamp(diag(A)), identity rows / columns for constant frames (requested, or
// observed by no rank — cameras: seen by no rank), the intrinsics pads (1 + λ on the diagonal, LM diagonal 1).  One lane
// per element, then six per frame for g, the direct gradient, the LM diagonal and the effective constant flag.
struct ImportSkyArgs {
  const double* X;          // summed exchange buffer: band rows
  const double* Xb;         // … its border region
  const uint8_t* fixed_req;
  const int* row;           // skyline row offsets of the summed profile (nfs + 1)
  double* S;
  double* g;
  double* g_dir;
  double* Ddiag;
  uint8_t* fixed;           // effective constant frames (nfs)
  int nf, nc, K;
  long long n_el;           // skyline elements (36 per block)
};
__device__ __forceinline__ bool import_fixed(const ImportSkyArgs& a, int i) {
  const int nfs = a.nf + 2 * a.nc;
  if (i < a.nf) return a.fixed_req[i] || a.X[(long long)i * ex_row(a.K) + (a.K + 1) * 36 + 18] == 0.0;
  return a.Xb[(long long)(i - a.nf) * ((long long)nfs * 36 + EX_TAIL) + (long long)nfs * 36 + 18] == 0.0;
}
__global__ void import_sky_kernel(const ImportSkyArgs a, double lambda, const double* __restrict__ lm) {
  lambda = lm_lambda(lm_view(lm), lambda);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nfs = a.nf + 2 * a.nc, K = a.K;
  const long long RS = ex_row(K), BRS = (long long)nfs * 36 + EX_TAIL;
  auto tail_of = [&](int i) {
    return i < a.nf ? a.X + (long long)i * RS + (K + 1) * 36 : a.Xb + (long long)(i - a.nf) * BRS + (long long)nfs * 36;
  };
  if (t < a.n_el) {
    const int blk = (int)(t / 36), e = (int)(t % 36), r = e / 6, cc = e % 6;
    int lo = 0, hi = nfs;  // the row i with row[i] ≤ blk < row[i + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.row[mid] <= blk) lo = mid;
      else hi = mid;
    }
    const int i = lo, j = (i < a.nf ? max(0, i - K) : 0) + (blk - a.row[i]);
    double val;
    bool pad = false;
    if (i < a.nf) {
      val = a.X[(long long)i * RS + (j - i + K) * 36 + e];
    } else {
      const int p = i - a.nf, d = 6 * (p & 1) + r, d2 = j >= a.nf ? 6 * ((j - a.nf) & 1) + cc : cc;
      pad = d >= 8 || d2 >= 8;
      val = a.Xb[(long long)p * BRS + (long long)j * 36 + e];
    }
    if (import_fixed(a, i) || import_fixed(a, j)) {
      val = (i == j && r == cc) ? 1.0 : 0.0;
    } else if (pad) {
      val = (i == j && r == cc) ? 1.0 + lambda : 0.0;  // border_store: direct 1, LM diagonal 1
    } else if (i == j && r == cc) {
      val += lambda * fmin(fmax(tail_of(i)[12 + r], 1e-6), 1e32);
    }
    a.S[t] = val;
    return;
  }
  const long long u = t - a.n_el;
  if (u >= 6LL * nfs) return;
  const int i = (int)(u / 6), r = (int)(u % 6);
  const double* tail = tail_of(i);
  const bool fi = import_fixed(a, i), pad = i >= a.nf && ((i - a.nf) & 1) && r >= 2;
  a.g[u] = fi || pad ? 0.0 : tail[r];
  a.g_dir[u] = fi || pad ? 0.0 : tail[6 + r];
  a.Ddiag[u] = fi ? 0.0 : (pad ? 1.0 : fmin(fmax(tail[12 + r], 1e-6), 1e32));
  if (r == 0) a.fixed[i] = fi ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// Updates: poses T·exp(δ) (se3_exp_mul, pba_internal.h) and back-substituted inverse distances
// ------------------------------------------------------------------------------------------------
// The update workgroups' partials besides the model decrease (slot layout of red): Σ|x − x_new|² and Σ|x_new|² in the
// ambient parameter space (red2, two doubles per slot: Ceres' step_norm and x_norm, trust_region_minimizer.cc:706-726,
// :813-814) and max |x − (x ⊞ −g)| at the current state (gmax, one double per slot: gradient_max_norm,
// trust_region_minimizer.cc:287-299).  Constant frames and points without blocks are not parameters of the solve.
struct PoseUpdateArgs {
  const double* poses;
  const double* x;
  const double* g_dir;
  const double* Ddiag;
  const uint8_t* fixed;
  double* poses_new;
  double* red;
  double* red2;
  double* gmax;
  int n;                 // system frames: the keyframes, then two per camera with free intrinsics
  int nf;                // keyframes
  const double* kcur;    // free intrinsics: the state's camera records (projection part) …
  double* knew_d;        // … the candidate's (camera records) …
  float* knew_f;         // … and their fp32 copy (8 per camera)
  double kscale;         // 2^−level: the step is the level-0 state's, the records its image at the active level (entries
                         // 0-3 move by 2^−level·δk₀, the distortion by δk₀); 1 at level 0 and on geometric engines
};

// Candidate intrinsics entry d of camera c — the one expression for intr_update_frame and the candidate pair table, so
// both hold the same bits.
__device__ __forceinline__ double candidate_intr(const PoseUpdateArgs& a, int c, int d) {
  const int i = a.nf + 2 * c + (d >= 6), r = d - 6 * (d >= 6);
  const double k = a.kcur[kCamD * c + d], xk = a.x[6 * i + r];
  return a.fixed[i] ? k : k + (d < 4 ? a.kscale * xk : xk);
}


// Frame i's update inputs, all loaded in one memory round (every dependent round trip is ~1.7 µs in these kernels):
// the pose, the step, the gradient direction, the LM diagonal and the constant flag.
struct FrameIn {
  double T[7], x[6], g[6], D[6];
  bool fixed;
};
__device__ __forceinline__ FrameIn frame_in(const PoseUpdateArgs& a, int i, bool grad) {
  FrameIn f;
  const double* P = a.poses + 7 * i;
#pragma unroll
  for (int q = 0; q < 7; ++q) f.T[q] = P[q];
  const double2* X = reinterpret_cast<const double2*>(a.x + 6 * i);
  const double2* G = reinterpret_cast<const double2*>(a.g_dir + 6 * i);
  const double2* Dd = reinterpret_cast<const double2*>(a.Ddiag + 6 * i);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double2 xv = X[q];
    f.x[2 * q] = xv.x;
    f.x[2 * q + 1] = xv.y;
    if (grad) {
      const double2 gv = G[q], dv = Dd[q];
      f.g[2 * q] = gv.x;
      f.g[2 * q + 1] = gv.y;
      f.D[2 * q] = dv.x;
      f.D[2 * q + 1] = dv.y;
    }
  }
  f.fixed = a.fixed[i] != 0;
  return f;
}
// candidate pose T·exp(δ), or T for a constant frame
__device__ __forceinline__ void candidate_pose(const FrameIn& f, double* out) {
  if (f.fixed) {
#pragma unroll
    for (int q = 0; q < 7; ++q) out[q] = f.T[q];
  } else {
    se3_exp_mul(f.T, f.x, out);
  }
}

// A free camera's intrinsics (system frames nf + 2c, nf + 2c + 1: dims 6h … 6h + 5 of the 8, the rest pads): k ← k + δ
// (a plain parameter block, no local parameterisation), with the same model-decrease, norm and gradient partials.
__device__ __forceinline__ void intr_update_frame(const PoseUpdateArgs& a, int i, double* v, double& gm) {
  const int c = (i - a.nf) >> 1, h = (i - a.nf) & 1;
  const bool fx = a.fixed[i] != 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int d = 6 * h + r;
    if (d >= 8) break;
    const double xk = a.x[6 * i + r], gk = a.g_dir[6 * i + r], Dk = a.Ddiag[6 * i + r];
    const double k = a.kcur[kCamD * c + d], kn = candidate_intr(a, c, d);
    a.knew_d[kCamD * c + d] = kn;
    a.knew_f[8 * c + d] = (float)kn;
    if (fx) continue;
    v[0] += xk * gk;
    v[1] += xk * xk * Dk;
    v[2] += (kn - k) * (kn - k);
    v[3] += kn * kn;
    gm = fmax(gm, fabs(gk));  // |k − (k − g)|
  }
}

__device__ __forceinline__ void pose_update_block(const PoseUpdateArgs& a, const LmView& lv, int blk) {
  const int i = blk * blockDim.x + threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // x·g, x·D·x, |T − T_new|², |T_new|²
  double gm = 0.0;
  const FrameIn f = frame_in(a, min(i, a.nf - 1), true);  // in flight with the record's load; then the done test
  if (lv.done != 0.0) return;  // (uniform)
  if (i >= a.nf && i < a.n) {
    intr_update_frame(a, i, v, gm);
  } else if (i < a.n) {
    double tn[7];
    candidate_pose(f, tn);
    double* out = a.poses_new + 7 * i;
#pragma unroll
    for (int q = 0; q < 7; ++q) out[q] = tn[q];
    if (!f.fixed) {
      double ng[6], tg[7];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        v[0] += f.x[r] * f.g[r];
        v[1] += f.x[r] * f.x[r] * f.D[r];
        ng[r] = -f.g[r];
      }
      se3_exp_mul(f.T, ng, tg);  // Plus(x, −gradient)
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const double d = tn[q] - f.T[q];
        v[2] += d * d;
        v[3] += tn[q] * tn[q];
        gm = fmax(gm, fabs(f.T[q] - tg[q]));
      }
    }
  }
  double* const dst[4] = {a.red + 2 * blk, a.red + 2 * blk + 1, a.red2 + 2 * blk, a.red2 + 2 * blk + 1};
  wg_reduce_sum_max<4>(v, gm, dst, a.gmax + blk);
}

struct PointUpdateArgs {
  const double* pt_data;
  const double* pt_data1;  // the single-GPU LM loop: set 1's point data (schur_free_decide_kernel), else pt_data
  const int4* pt_rec;
  const int4* pt_tgt;
  const int* gn_target;
  const double* blk_schur;
  const double* blk_schur1;  // buffer set 1 (device LM loop)
  const double* x;
  const uint8_t* fixed;
  const double* rho;
  double* rho_new;
  double* drho;
  double* red;
  double* red2;
  double* gmax;
  int n_points;
  const double* pw;      // free intrinsics: per GN point its per-camera Σ W_i (ib_pw: intr_rows_kernel / intr_pw_kernel,
  int nc;                // 8·nc + 6 per point), the cameras and the keyframe count (the intrinsics steps start at
  int nf;                // x[6·nf], 12 per camera)
};

// blk: the point workgroup's index among the point workgroups; slot: its reduction slot
// lm: the LM record (done → return before any store; read with the point's first loads, not ahead of them)
__device__ __forceinline__ void point_update_block(const PointUpdateArgs& a, const double* lm, double lambda, int blk,
                                                   int slot) {
  const int p = blk * blockDim.x + threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};  // δρ·g, δρ·D·δρ, δρ², ρ_new²
  double gm = 0.0;
  const LmView lv = lm_view(lm);
  const int pc = min(p, a.n_points - 1);
  const int4 pr = a.pt_rec[pc];  // first block, block count, host, original point
  const int4 pt4 = a.pt_tgt[pc];  // the targets of its first four blocks
  // both sets' point data with the record (which of them is current is the record's): no dependent round for the choice
  double pd[8], pd1[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double2 d2 = reinterpret_cast<const double2*>(a.pt_data + (long long)pc * 8)[i];
    const double2 e2 = reinterpret_cast<const double2*>(a.pt_data1 + (long long)pc * 8)[i];
    pd[2 * i] = d2.x;
    pd[2 * i + 1] = d2.y;
    pd1[2 * i] = e2.x;
    pd1[2 * i + 1] = e2.y;
  }
  if (lv.set != 0.0)
#pragma unroll
    for (int i = 0; i < 8; ++i) pd[i] = pd1[i];
  if (lv.done != 0.0) return;  // (uniform: every thread of the workgroup returns)
#ifdef PBA_UPD_STAMPS
  long long ts[4];
  ts[0] = wall_clock64();
#endif
  lambda = lm_lambda(lv, lambda);
  const double* blk_schur = lv.set != 0.0 ? a.blk_schur1 : a.blk_schur;
  if (p < a.n_points) {
    const double H = pd[0], gl = pd[1];
    const double D = fmin(fmax(H, 1e-6), 1e32);
    const double Hd = H + lambda * D;
    const int h = pr.z;
    // vector loads (16 B) and every load of a batch in flight before the first use: the target steps' loads used to sit
    // behind a data-dependent break (one memory round trip per block) and 4-B / 8-B scalar loads of scattered rows
    auto x6 = [&](int f, double* o) {
      const double2* q = reinterpret_cast<const double2*>(a.x + 6 * f);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double2 d2 = q[i];
        o[2 * i] = d2.x;
        o[2 * i + 1] = d2.y;
      }
    };
    double xh[6];
    x6(h, xh);
    double s = gl;
    for (int i = 0; i < 6; ++i) s += pd[2 + i] * xh[i];
    const int fb = pr.x, nb = pr.y;
    constexpr int kBatch = 4;  // a batch's loads issued together, then summed in block order
    for (int b0 = fb; b0 < fb + nb; b0 += kBatch) {
      double w[kBatch][6];
      int t[kBatch];
      const bool first = b0 == fb;  // the first batch's targets came with the point record
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int b = min(b0 + u, fb + nb - 1);
        t[u] = first ? (u == 0 ? pt4.x : u == 1 ? pt4.y : u == 2 ? pt4.z : pt4.w) : a.gn_target[b];
        const double2* wt = reinterpret_cast<const double2*>(blk_schur + (long long)b * kPd + 2);  // W_t
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double2 q2 = wt[i];
          w[u][2 * i] = q2.x;
          w[u][2 * i + 1] = q2.y;
        }
      }
      double xt[kBatch][6];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) x6(t[u], xt[u]);
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        if (b0 + u < fb + nb)
#pragma unroll
          for (int i = 0; i < 6; ++i) s += w[u][i] * xt[u][i];
    }
    if (a.pw) {  // + Σ_b W_i(b)·δk(camera of b's target) = Σ_c W_c·δk_c from the point's camera sums (one load round,
                 // not a camera index then its step per block)
      const double* wc = a.pw + (long long)p * (8 * a.nc + 6);
      for (int c = 0; c < a.nc; ++c) {
        const double* xk = a.x + 6 * a.nf + 12 * c;
#pragma unroll
        for (int d = 0; d < 8; ++d) s += wc[8 * c + d] * xk[d];
      }
    }
#ifdef PBA_UPD_STAMPS
    ts[1] = wall_clock64();
#endif
    const double dr = Hd > 0.0 ? -s / Hd : 0.0;
    const int o = pr.w;
    const double rn = a.rho[o] + dr;
    a.rho_new[o] = rn;
    a.drho[o] = dr;
    v[0] = dr * gl;
    v[1] = dr * dr * D;
    v[2] = dr * dr;
    v[3] = rn * rn;
    gm = fabs(gl);  // ρ has no local parameterisation: |ρ − (ρ − g_ρ)|
  }
#ifdef PBA_UPD_STAMPS
  ts[2] = wall_clock64();
#endif
  double* const dst[4] = {a.red + 2 * slot, a.red + 2 * slot + 1, a.red2 + 2 * slot, a.red2 + 2 * slot + 1};
  wg_reduce_sum_max<4>(v, gm, dst, a.gmax + slot);
#ifdef PBA_UPD_STAMPS
  ts[3] = wall_clock64();
  if (threadIdx.x == 0 && (blk == 0 || blk == 196))
    printf("updpoint blk=%d loads %lld loop %lld stores %lld reduce %lld\n", blk, ts[0], ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2]);
#endif
}

struct PairUpdateArgs {
  const int4* pair_rec;  // {host, target, host camera, target camera}
  const double* cams;
  PairRec* pairs_new;  // nullptr: no candidate pair table (geometric engines form theirs in the cost path too)
  int n_pairs;
  bool cand_tk;        // photometric free intrinsics: the target part is the CANDIDATE intrinsics' (candidate_intr; the
                       // state's pair table carries the state, launch_pairs), not the cameras'
};

// The step's candidate state in ONE launch: workgroups [0, gp) update the poses (T·exp(δ)) and reduce the pose part
// of the model decrease, [gp, gp + gq) back-substitute the inverse distances and reduce the point part (partial slots
// in the same fixed order as two separate launches), and the rest form the candidate pair table straight from
// T_h·exp(δ_h), T_t·exp(δ_t) — candidate_pose, the same arithmetic as the pose workgroups, so the pairs equal
// form_pair(poses_new) bit for bit — which saves the separate pair launch before the candidate cost.
__global__ __launch_bounds__(kBlockThreads) void update_kernel(const PoseUpdateArgs pa, PointUpdateArgs qa,
                                                               const PairUpdateArgs ra, int gp, int gq, double lambda,
                                                               const double* __restrict__ lm) {
  // gated: a trial after the end must not touch the last step (pba_gn_get_step).  Each part tests the record after
  // its own first loads are issued (a test ahead of them cost a memory round trip of its own)
  const int b = blockIdx.x;
#ifdef PBA_UPD_STAMPS  // timing dissection only: absolute 100-MHz stamps at the start and end of chosen workgroups
  const long long t0 = wall_clock64();
  struct Stamp {
    long long t0;
    int b;
    __device__ ~Stamp() {
      if (threadIdx.x == 0 && (b == 0 || b == 4 || b == 200 || b == 394 || b == 395 || b == 410))
        printf("updstamp b=%d start %lld end %lld\n", b, t0, wall_clock64());
    }
  } stamp{t0, b};
#endif
  if (b >= gp && b < gp + gq) {
    point_update_block(qa, lm, lambda, b - gp, b);
    return;
  }
  const LmView lv = lm_view(lm);
  if (b < gp) {
    pose_update_block(pa, lv, b);
  } else {
    // two memory rounds: the pair record, then both frames' inputs and both cameras' constants together
    const int i = (b - gp - gq) * blockDim.x + threadIdx.x;
    const int4 pr = ra.pair_rec[min(i, ra.n_pairs - 1)];
    const FrameIn fh = frame_in(pa, pr.x, false), ft = frame_in(pa, pr.y, false);
    double hk[kCamK], tk[kCamK];
#pragma unroll
    for (int j = 0; j < kCamK; ++j) {
      hk[j] = ra.cams[kCamD * pr.z + kCamHk + j];
      tk[j] = ra.cand_tk ? candidate_intr(pa, pr.w, j) : ra.cams[kCamD * pr.w + j];
    }
    if (lv.done != 0.0 || i >= ra.n_pairs) return;
    double H[7], T[7];
    candidate_pose(fh, H);
    candidate_pose(ft, T);
    PairRec r;
    pair_rotation(H, T, r);
    pair_translation(H, T, r);
    r.host_cam = pr.z;
    r.target_cam = pr.w;
    r.target = pr.y;
    r.host = pr.x;
#pragma unroll
    for (int j = 0; j < kCamK; ++j) {
      r.hk[j] = hk[j];
      r.tk[j] = tk[j];
    }
    camera_kf(tk, r.kf);
    ra.pairs_new[i] = r;
  }
}

__global__ __launch_bounds__(kBlockThreads) void cost_reduce_kernel(const float* cost, const uint8_t* valid, int n,
                                                                    double* red) {
  double c = 0.0, v = 0.0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    c += cost[i];
    v += valid[i];
  }
  wg_reduce2(c, v, red + 2 * blockIdx.x);
}

// ---- the single-GPU LM loop's λ-free point elimination ---------------------------------------------------------------
// For a point whose H_ρρ lies inside the LM diagonal's clamp [1e-6, 1e32] (levenberg_marquardt_strategy.cc), the damped
// H' = H + λ·clamp(H) = (1 + λ)·H, so its Schur terms W Wᵀ / H' and W g / H' are (1 + λ)⁻¹ times the λ-free W Wᵀ / H and
// W g / H.  A linearisation set's λ-free partials P are therefore formed once, right after the set is linearised, and every
// trial on that set (an accepted candidate's first, or the retries after rejections) assembles A + λD − P / (1 + λ):
// no per-trial point elimination.  A set with a point outside the clamp (H ≠ 0: a point with H = 0 has W = 0) is flagged
// (degen[set]) and its trials form the λ-specific partials in schur_gate_kernel, exactly as schur_kernel does.
//
// The kernel after the candidate linearisation: workgroup 0 takes the trial's decision (lm_decide_kernel's sums and
// decision, 256 threads) — or, init, forms the record of a new solve (lm_init_kernel's) — while workgroups 1 … n_schur
// form the λ-free partials and point data of the set linearize_kernel has just written (lin_set); the two parts share no
// data, so the decision costs no launch and runs beside the elimination.  The elimination never reads the record's set
// (the decision may flip it meanwhile); only its done flag (a workgroup that sees the solve ended skips its chunk: nothing
// reads it then).  (DecideArgs, kDecideWgs and the decision's device code: pba_gn_lm.h.)
struct FreeSets {
  double* part[2];    // λ-free Schur partials per linearisation set
  double* pt[2];      // point data per set ([H, g, W_h(6)] per GN point, undamped)
  int* degen;         // [2]: a point of the set outside the clamp
  const int* lin_set; // the set the last linearisation wrote
};

__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(4, 8))) void schur_free_decide_kernel(const SchurArgs g, const DecideArgs da,
                                                                        const FreeSets fs) {
  extern __shared__ __attribute__((aligned(16))) double W_dyn[];
  __shared__ double s_inv[SCHUR_PTS], s_gl[SCHUR_PTS];
#ifdef PBA_FD_STAMPS  // timing dissection only: 100-MHz stamps at the start and end of chosen workgroups
  struct Stamp {
    long long t0 = wall_clock64();
    __device__ ~Stamp() {
      const int b = blockIdx.x;
      if (threadIdx.x == 0 && (b == 0 || b == 1 || b == 300 || b == 600 || b == (int)gridDim.x - 1))
        printf("fdstamp b=%d start %lld end %lld\n", b, t0, wall_clock64());
    }
  } stamp;
#endif
  if (blockIdx.x < kDecideWgs) {
    // a slice of the sums per workgroup → sc1 stores → (every store completed, release) → arrival count; the last
    // workgroup to arrive (acquire) adds the slices in workgroup order — the same totals whichever arrives last — and
    // decides (or, init, writes the new solve's record)
    __shared__ double t[kTsCount];
    __shared__ int s_last;
    const double done = da.init ? 0.0 : da.lm[kLmDone];  // (tested after the sums, as lm_decide_kernel)
    {
      const int E = da.init ? da.gc : da.gp + da.gq + da.gc, per = (E + kDecideWgs - 1) / kDecideWgs;
      const int lo = (int)blockIdx.x * per, hi = min(E, lo + per);
      if (da.init) trial_sums<kBlockThreads>(da.red, da.red, da.red, 0, 0, da.gc, t, lo, hi);
      else trial_sums<kBlockThreads>(da.red, da.red2, da.gmax, da.gp, da.gq, da.gc, t, lo, hi);
      if (threadIdx.x < kTsCount)
        __hip_atomic_store(da.ts_part + blockIdx.x * kTsCount + threadIdx.x, t[threadIdx.x], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = __hip_atomic_fetch_add(da.ts_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kDecideWgs - 1;
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __syncthreads();
      if (!s_last) return;
      if (threadIdx.x < kTsCount) {
        const int q = threadIdx.x;
        const bool mx = q == kTsPoseGMax || q == kTsPtGMax;
        double v = 0.0;
#pragma unroll 1
        for (int b0 = 0; b0 < kDecideWgs; b0 += 4) {  // (4 loads in flight: 16 held the elimination to 3 waves/SIMD)
          double x[4];
#pragma unroll
          for (int b = 0; b < 4; ++b)
            x[b] = __hip_atomic_load(da.ts_part + (b0 + b) * kTsCount + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
          for (int b = 0; b < 4; ++b) v = mx ? fmax(v, x[b]) : v + x[b];
        }
        t[q] = v;
      }
      if (threadIdx.x == 0) *da.ts_count = 0;  // for the next launch (ordered by the launch boundary)
      __syncthreads();
    }
    if (da.init) {
      if (threadIdx.x != 0) return;
      double* lm = da.lm;
      for (int i = 0; i < kLmFields; ++i) lm[i] = 0.0;
      lm[kLmCost] = t[kTsCost];
      lm[kLmValid] = t[kTsValid];
      lm[kLmXNorm] = -1.0;
      lm[kLmRadius] = da.radius;
      lm[kLmFactor] = 2.0;
      lm[kLmLambda] = 1.0 / da.radius;
      da.init_out[0] = t[kTsCost];
      da.init_out[1] = t[kTsValid];
      return;
    }
    if (done != 0.0 || threadIdx.x >= 64) return;
    __shared__ double s_rec[kLmFields];
    if (threadIdx.x == 0) {
      lm_decide(t, *da.status, da.o, da.lm);
      for (int i = 0; i < kLmFields; ++i) s_rec[i] = da.lm[i];
    }
    if (da.host_rec) publish_record(s_rec, da.host_rec, da.seq);
    return;
  }
  const int c = blockIdx.x - kDecideWgs;
  if (c >= g.n_chunks) return;
  // one memory round: the chunk's descriptors, the record's done flag and the set, all issued before the exit (the
  // compiler otherwise waited for the flag, then for the set, then issued the descriptors)
  const SchurHead h = schur_head(g, c);
  const double done = da.lm[kLmDone];
  const int lset = *fs.lin_set;
  asm volatile("" ::"v"(done), "v"(lset), "v"(h.d.x), "v"(h.ax.x), "v"(h.lp4.x));
#pragma unroll
  for (int it = 0; it < kPtIter; ++it) asm volatile("" ::"v"(h.prec[it].x), "v"(h.prec[it].y));
  if (!da.init && done != 0.0) return;
  const int set = lset != 0;
  schur_chunk(g, h, 0.0, set ? g.blk_schur1 : g.blk_schur, set ? g.pair_rt1 : g.pair_rt, fs.part[set], fs.pt[set],
              fs.degen + set, W_dyn, s_inv, s_gl);
}

// The single-GPU LM trial's first kernel: the previous trial's accept, and — only for a set flagged degen — the
// λ-specific point elimination of the current set into part_schur (every chunk, grid-stride), which the assembly then
// takes instead of the λ-free partials.
__global__ __launch_bounds__(kBlockThreads) void schur_gate_kernel(const SchurArgs g, const int* __restrict__ degen) {
  extern __shared__ __attribute__((aligned(16))) double W_dyn[];
  __shared__ double s_inv[SCHUR_PTS], s_gl[SCHUR_PTS];
  const LmView lv = lm_view(g.lm);
  const int dg0 = degen[0], dg1 = degen[1];
  AcceptCopy ac;
  ac.load(g, lv);
  const int set = lv.set != 0.0;
  if ((set ? dg1 : dg0) != 0 && lv.done == 0.0) {
    const double* blk_schur = set ? g.blk_schur1 : g.blk_schur;
    for (int c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
      schur_chunk(g, schur_head(g, c), lv.lambda, blk_schur, set ? g.pair_rt1 : g.pair_rt, g.part_schur, nullptr,
                  nullptr, W_dyn, s_inv, s_gl);
      __syncthreads();
    }
  }
  ac.store(g);
}

// The accepted candidate becomes the state (device-side accept, gated by the decision record; lm == nullptr: always).
// Only the points of the Gauss-Newton problem are copied (through pt_orig): rho_new holds nothing for a point with
// no residual block, and such a point keeps its state, as a parameter Ceres never sees would.
__global__ void lm_accept_kernel(const double* __restrict__ lm, const double* __restrict__ poses_new,
                                 const double* __restrict__ rho_new, const int* __restrict__ pt_orig,
                                 double* __restrict__ poses, double* __restrict__ rho, int n_pose_d, int n_gn_points) {
  if (lm && (lm[kLmAccept] == 0.0 || lm[kLmDone] != 0.0)) return;
  const int n = max(n_pose_d, n_gn_points);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (i < n_pose_d) poses[i] = poses_new[i];
    if (i < n_gn_points) {
      const int o = pt_orig[i];
      rho[o] = rho_new[o];
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side: the stages the LM driver calls (declared in pba_gn_lm.h), and — static — what only this unit uses
// ------------------------------------------------------------------------------------------------
namespace pba {
namespace detail {

static int gn_lpb(const pba_engine* e) { return e->opt.residual_kind == PBA_RESIDUAL_GEOMETRIC ? 4 : 8; }
// rows per lane of the linearisation: 1 up to 8 px (one lane per row), ⌈P/8⌉ above (linearize_adj_kernel<·, PPL>)
static int gn_ppl(const pba_engine* e) { return e->opt.residual_kind == PBA_RESIDUAL_GEOMETRIC ? 1 : (e->P + 7) / 8; }

// A plan vector (pba_gn_plan.h) into its device buffer: the plan's records are the device's int4 / int2 / uchar2 byte
// for byte.
static_assert(sizeof(PlanInt4) == sizeof(int4) && sizeof(PlanInt2) == sizeof(int2) && sizeof(PlanUchar2) == sizeof(uchar2),
              "the plan's records are uploaded as the device's vector types");
template <class D, class H>
static hipError_t upload_plan(DevBuf<D>& buf, const std::vector<H>& h, hipStream_t s) {
  static_assert(sizeof(D) == sizeof(H), "element for element");
  const hipError_t rc = buf.resize(h.size());
  if (rc != hipSuccess || h.empty()) return rc;
  return hipMemcpyAsync(buf.p, h.data(), h.size() * sizeof(H), hipMemcpyHostToDevice, s);
}

// The symbolic analysis (build_gn_plan: GN block order, chunks, slot layouts, skyline profile, contribution and border
// lists) into GnData, in upload order, and the buffers sized by it.
static int gn_prepare(pba_engine* e) {
  GnData& G = e->gn;
  const int nb = e->n_blocks, nf = e->n_frames;
  if (nb <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  G.lpb = gn_lpb(e);
  G.ppl = gn_ppl(e);
  G.bpw = kBlockThreads / G.lpb;
  // free intrinsics (geometric engines; photometric ones with pba_gn_set_solve_intrinsics): nc cameras in the system
  const int nc = e->gn_free_intr() ? e->n_cams : 0;
  const GnPlanInput in{nf, e->n_cams, e->n_pairs, e->n_points, nb,
                       e->block_point_h.data(), e->block_target_h.data(), e->point_host_h.data(),
                       e->pair_of_h.data(), e->pair_host_h.data(), e->pair_target_h.data(), e->frame_cam_h.data(),
                       G.fixed_h.data(), (int)G.fixed_h.size(), G.lpb, G.ppl, G.bpw, nc,
                       test_hook("PBA_TEST_PBLK_WALK") != nullptr, test_hook("PBA_TEST_ROW_WAVES64") != nullptr,
                       getenv("PBA_SKYLINE_GLOBAL") != nullptr};
  GnPlan P;
  if (int rc = build_gn_plan(in, P)) return rc;
  G.lin_slots = P.lin_slots;
  G.n_chunks = P.n_chunks;
  G.n_gn_points = P.n_gn_points;
  G.schur_doubles = P.schur_doubles;
  G.schur_rt_off = P.schur_rt_off;
  G.schur_lds = P.schur_lds;
  G.n_schur = P.n_schur;
  G.nc_sys = in.nc;
  G.nfs = P.nfs;
  G.dsky_K = -1;  // the multi-GPU summed profile is rebuilt for this problem (ensure_dist_sky)
  G.n_sky = P.n_sky;
  G.n_sky_diag = P.n_sky_diag;
  G.band = P.band;
  // (the photometric producer has no point-aligned form: its points' sums always come from intr_pw_kernel)
  G.ir_waves = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC ? 0 : P.ir_waves;
  const int ngp = P.n_gn_points, nfs = P.nfs;
  hipStream_t st = e->stream;
  if (int rc = build_front_plan(P.sky_first, P.sky_row, P.sky_colptr, P.sky_colrows, st, G.front, !in.skyline_global))
    return rc;
#define PBA_UP(name) PBA_HIP(upload_plan(G.name, P.name, st))
  PBA_UP(pt_fb);
  if (in.nc) {
    PBA_UP(ib_rec);
    PBA_UP(ib_cam);
    PBA_UP(ib_bptr);
    PBA_UP(ib_blist);
    PBA_UP(ib_pptr);
    PBA_UP(ib_plist);
    PBA_UP(ib_pblk);
    if (G.ir_waves) PBA_UP(ir_wave);
    if (int rc = intr_prepare_buffers(e)) return rc;
  }
  PBA_UP(lin_rec);
  PBA_UP(chunk_desc);
  PBA_HIP(G.blk_schur.resize((size_t)nb * kPd));
  PBA_HIP(G.part_lin.resize(std::max<size_t>(G.lin_slots, 1)));
  PBA_HIP(G.blk_schur1.resize((size_t)nb * kPd));  // the device LM loop's second linearisation set
  PBA_HIP(G.pair_rt.resize((size_t)std::max(e->n_pairs, 1) * 12));
  PBA_HIP(G.pair_rt1.resize((size_t)std::max(e->n_pairs, 1) * 12));
  PBA_HIP(G.part_lin1.resize(std::max<size_t>(G.lin_slots, 1)));
  PBA_UP(pt_first);
  PBA_UP(pt_nblk);
  PBA_UP(pt_orig);
  PBA_UP(pt_host);
  PBA_UP(pt_rec);
  PBA_UP(pt_tgt);
  PBA_UP(pair_rec);
  PBA_UP(gn_target);
  PBA_UP(schur_desc);
  PBA_UP(schur_aux);
  PBA_UP(schur_pairs);
  PBA_UP(blk_lv);
  PBA_UP(schur_lvp4);
  PBA_UP(schur_lvp);
  PBA_HIP(G.part_schur.resize(std::max<size_t>(G.schur_doubles, 1)));
  PBA_HIP(G.pt_data.resize((size_t)ngp * 8));
  PBA_HIP(G.pt_data1.resize((size_t)ngp * 8));
  PBA_HIP(G.part_free0.resize(std::max<size_t>(G.schur_doubles, 1)));
  PBA_HIP(G.part_free1.resize(std::max<size_t>(G.schur_doubles, 1)));
  PBA_HIP(G.degen.resize(2));
  PBA_HIP(G.lin_set.resize(1));
  PBA_HIP(hipMemsetAsync(G.degen.p, 0, 2 * sizeof(int), st));
  PBA_HIP(G.ts_part.resize((size_t)kDecideWgs * kTsCount));
  PBA_HIP(G.ts_count.resize(1));
  PBA_HIP(hipMemsetAsync(G.ts_count.p, 0, sizeof(int), st));
  PBA_UP(sky_first);
  PBA_UP(sky_row);
  PBA_UP(sky_last);
  PBA_UP(sky_colptr);
  PBA_UP(sky_colrows);
  PBA_UP(sky_cptr);
  PBA_UP(sky_contrib);
  PBA_UP(g_cptr);
  PBA_UP(g_contrib);
  PBA_UP(sky_blk_i);
  PBA_UP(sky_blk_j);
  PBA_UP(sky_diag);
  PBA_UP(sky_off);
  PBA_UP(fixed);
  PBA_HIP(G.S.resize((size_t)G.n_sky * 36));
  PBA_HIP(G.L.resize((size_t)G.n_sky * 36));
  if (int rc = configure_local_solver(e)) return rc;
  PBA_UP(observed);
  PBA_UP(fixed_req);
#undef PBA_UP
  PBA_HIP(G.fixed_dist.resize(nfs));
  PBA_HIP(G.g.resize((size_t)nfs * 6));
  PBA_HIP(G.g_dir.resize((size_t)nfs * 6));
  PBA_HIP(G.Ddiag.resize((size_t)nfs * 6));
  PBA_HIP(G.Linv.resize((size_t)nfs * 36));
  PBA_HIP(G.x.resize((size_t)nfs * 6));
  PBA_HIP(G.poses_new.resize((size_t)nf * 7));
  PBA_HIP(G.rho_new.resize((size_t)e->n_points));
  PBA_HIP(G.drho.resize((size_t)e->n_points));
  PBA_HIP(G.pairs_new.resize((size_t)e->n_pairs));
  PBA_HIP(G.status.resize(1));
  const int red_pose = (nfs + kBlockThreads - 1) / kBlockThreads;
  const int red_pt = (ngp + kBlockThreads - 1) / kBlockThreads;
  // update partials, then the candidate cost's workgroup partials (≤ one per 16 blocks: launch_cost_only's grids)
  G.red_slots = red_pose + red_pt + std::max({1024, nb / 16 + 2, G.n_chunks});
  PBA_HIP(G.red.resize((size_t)2 * G.red_slots));
  PBA_HIP(G.red2.resize((size_t)2 * (red_pose + red_pt)));
  PBA_HIP(G.gmax.resize((size_t)(red_pose + red_pt)));
  PBA_HIP(G.red_h.resize(2 * G.red_slots));
  PBA_HIP(G.lm.resize(kLmFields));
  PBA_HIP(G.tpose.resize(8));  // pose part (5), point gradient max-norm, solve status
  {  // the record of host-driven steps: not done, buffer set 0, λ NaN (the kernels then use their λ argument)
    std::vector<double> idle(kLmFields, 0.0);
    idle[kLmLambda] = std::numeric_limits<double>::quiet_NaN();
    PBA_HIP(G.lm_idle.upload(idle, st));
  }
  // decision record + sequence number, written by lm_decide_kernel over the bus (fine-grained host memory)
  PBA_HIP(G.lm_h.resize(kRecRing * kRecStride, hipHostMallocCoherent | hipHostMallocMapped));
  PBA_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&G.lm_host_d), G.lm_h.p, 0));
  PBA_HIP(hipMemsetAsync(G.drho.p, 0, sizeof(double) * e->n_points, st));
  PBA_HIP(hipStreamSynchronize(st));
  G.prepared = true;
  G.pairs_new_fresh = false;
  G.fixed_eff = std::move(P.fixed);
  return PBA_OK;
}

int ensure_prepared(pba_engine* e, bool distributed) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (int rc = solve_refuses_both(e)) return rc;  // (the two solve switches below make no difference to it)
  if (e->n_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  if (!e->state_set) return fail(PBA_ERR_NOT_READY, "pba_set_state first");
  if (e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC && (!e->have_images || e->P <= 0))
    return fail(PBA_ERR_NOT_READY, "images/pattern missing");
  // without pba_gn_set_solve_intrinsics the solve would hold the intrinsics fixed (nc = 0): refused; the multi-GPU
  // entry points (distributed) have no photometric border exchange and refuse either way
  if (e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC && e->opt_intr && (!e->gn_solve_intr || distributed))
    return fail(PBA_ERR_INVALID_ARGUMENT,
                "the on-device Gauss-Newton solve does not support free intrinsics on a photometric engine");
  // without pba_gn_set_solve_affine the caller has not asked for a solve that holds (a, b) constant: refused, as
  // before that switch existed; the multi-GPU entry points refuse either way
  if (e->affine && (!e->gn_solve_affine || distributed))
    return fail(PBA_ERR_INVALID_ARGUMENT, "the on-device Gauss-Newton solve does not support affine brightness");
  // the 14-column lineariser of the test build (its A/B hook) has no affine form: it would solve at a = b = 0
  // (the hook's name stays out of the message: the product library carries no hook names)
  if (e->affine && e->gn.lin_legacy)
    return fail(PBA_ERR_INVALID_ARGUMENT, "the 14-column lineariser has no affine brightness form");
  if (int rc = check_device(e)) return rc;
  if (!e->gn.prepared)
    if (int rc = gn_prepare(e)) return rc;
  return PBA_OK;
}

// Σ of 2-vectors over `slots` reduction slots, in fixed order on the host.
static int read_red(pba_engine* e, int slots, double* a, double* b) {
  GnData& G = e->gn;
  PBA_HIP(hipMemcpyAsync(G.red_h.data(), G.red.p, sizeof(double) * 2 * slots, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  double x = 0, y = 0;
  for (int i = 0; i < slots; ++i) {
    x += G.red_h[2 * i];
    y += G.red_h[2 * i + 1];
  }
  *a = x;
  if (b) *b = y;
  return PBA_OK;
}

static int total_cost(pba_engine* e, double* cost, int* n_valid) {
  const int grid = std::min(1024, (e->n_blocks + kBlockThreads - 1) / kBlockThreads);
  cost_reduce_kernel<<<grid, kBlockThreads, 0, e->stream>>>(e->cost.p, e->valid.p, e->n_blocks, e->gn.red.p);
  PBA_HIP(hipGetLastError());
  double c, v;
  if (int rc = read_red(e, grid, &c, &v)) return rc;
  *cost = c;
  if (n_valid) *n_valid = (int)v;
  return PBA_OK;
}

// Linearisation at the engine's state (pairs == nullptr: formed here), or — the device LM loop — at the candidate:
// lm = the device LM record (the pieces go to the spare buffer set, nothing runs once the solve is done), pairs / rho
// the candidate's, and wg_red the slots of the per-chunk cost partials the decision sums.
// cand_intr: with free intrinsics, project with the candidate's (G.intr_new_*) instead of the state's.
// mark_set: record the set written (and clear its degen flag) for the λ-free elimination that follows.
int linearize(pba_engine* e, double* cost, const double* lm, const PairRec* pairs, const double* rho, double* wg_red,
              int* n_valid, bool cand_intr, bool mark_set) {
  GnData& G = e->gn;
  if (!pairs) {
    launch_pairs(e, e->poses.p, e->pairs.p);
    pairs = e->pairs.p;
  }
  KernelArgs ka = make_kernel_args(e, pairs, rho ? rho : e->rho.p);
  if (cand_intr && G.nc_sys) {
    ka.intr_t = G.intr_new_f.p;
    ka.intr_t_d = G.intr_new_d.p;
  }
  LinArgs la{G.lin_rec.p, G.blk_schur1.p, G.part_lin1.p, wg_red, G.chunk_desc.p, G.blk_schur.p, G.part_lin.p, G.n_chunks,
             lm ? lm : G.lm_idle.p, lm != nullptr, mark_set ? G.lin_set.p : nullptr, mark_set ? G.degen.p : nullptr,
             G.pair_rt.p, G.pair_rt1.p};
  if (e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC) launch_linearize_photometric(e, ka, la);
  else launch_linearize_geometric(e, ka, la);
  PBA_HIP(hipGetLastError());
  e->evaluated = false;  // records are not written in GN mode
  if (cost) return total_cost(e, cost, n_valid);
  return PBA_OK;
}

// After a solve into G.x: solver status, candidate poses/points, and the two parts of the LM model decrease
// L(0) − L(δ) = −gᵀδ − ½δᵀHδ = ½(λ δᵀDδ − gᵀδ)  (since (H + λD)δ = −g): pose part and point part.
// Candidate poses/points and the model-decrease partials into reduction slots [0, gp + gq) of G.red.
// free_sets: the single-GPU LM loop's per-set point data (the record says which set is current), else G.pt_data.
void enqueue_updates(pba_engine* e, double lambda, const uint8_t* fixed, int* gp_out, int* gq_out, const double* lm,
                     bool free_sets) {
  GnData& G = e->gn;
  const int nf = e->n_frames, nfs = G.nc_sys ? G.nfs : nf;
  const int gp = (nfs + kBlockThreads - 1) / kBlockThreads;
  const int gq = (G.n_gn_points + kBlockThreads - 1) / kBlockThreads;
  const int gr = (e->n_pairs + kBlockThreads - 1) / kBlockThreads;
  const bool ki = G.nc_sys > 0;
  const bool photo = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC;
  PoseUpdateArgs pa{e->poses.p, G.x.p, G.g_dir.p, G.Ddiag.p, fixed, G.poses_new.p, G.red.p, G.red2.p, G.gmax.p, nfs, nf,
                    ki ? e->intr_state_d.p : nullptr, ki ? G.intr_new_d.p : nullptr, ki ? G.intr_new_f.p : nullptr,
                    photo ? std::ldexp(1.0, -e->level) : 1.0};
  // point workgroup q writes reduction slot gp + q, as the separate launches did
  PointUpdateArgs qa{G.pt_data.p, free_sets ? G.pt_data1.p : G.pt_data.p, G.pt_rec.p, G.pt_tgt.p, G.gn_target.p,
                     G.blk_schur.p, G.blk_schur1.p, G.x.p, fixed, e->rho.p, G.rho_new.p, G.drho.p, G.red.p,
                     G.red2.p, G.gmax.p, G.n_gn_points, ki ? G.ib_pw.p : nullptr, G.nc_sys, nf};
  PairUpdateArgs ra{G.pair_rec.p, e->intr_d.p, G.pairs_new.p, e->n_pairs, ki && photo};
  update_kernel<<<gp + gq + gr, kBlockThreads, 0, e->stream>>>(pa, qa, ra, gp, gq, lambda, lm ? lm : G.lm_idle.p);
  G.pairs_new_fresh = true;
  *gp_out = gp;
  *gq_out = gq;
}

static void model_from_slots(const GnData& G, double lambda, int gp, int gq, double* model_pose, double* model_points) {
  double dg = 0, dD = 0, qg = 0, qD = 0;
  for (int i = 0; i < gp; ++i) { dg += G.red_h[2 * i]; dD += G.red_h[2 * i + 1]; }
  for (int i = gp; i < gp + gq; ++i) { qg += G.red_h[2 * i]; qD += G.red_h[2 * i + 1]; }
  *model_pose = 0.5 * (lambda * dD - dg);
  *model_points = 0.5 * (lambda * qD - qg);
}

static int finish_step(pba_engine* e, double lambda, const uint8_t* fixed, double* model_pose,
                       double* model_points, int* solver_status) {
  GnData& G = e->gn;
  int status = 0;
  PBA_HIP(hipMemcpyAsync(&status, G.status.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  if (solver_status) *solver_status = status;
  *model_pose = *model_points = 0.0;
  if (status != 0) return PBA_OK;
  int gp = 0, gq = 0;
  enqueue_updates(e, lambda, fixed, &gp, &gq);
  PBA_HIP(hipGetLastError());
  PBA_HIP(hipMemcpyAsync(G.red_h.data(), G.red.p, sizeof(double) * 2 * (gp + gq), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  model_from_slots(G, lambda, gp, gq, model_pose, model_points);
  return PBA_OK;
}

// The elimination kernels' arguments that every launch shares — the chunk tables, both linearisation sets, the outputs —
// with the record lm; no accept (poses == nullptr) and no intrinsics copy: a launch that applies them sets them by name.
static SchurArgs schur_args(const pba_engine* e, const double* lm) {
  const GnData& G = e->gn;
  SchurArgs sa{};
  sa.desc = G.schur_desc.p;
  sa.aux = G.schur_aux.p;
  sa.pairs = G.schur_pairs.p;
  sa.pt_fb = G.pt_fb.p;
  sa.blk_lv = G.blk_lv.p;
  sa.blk_schur = G.blk_schur.p;
  sa.blk_schur1 = G.blk_schur1.p;
  sa.part_schur = G.part_schur.p;
  sa.pt_data = G.pt_data.p;
  sa.n_chunks = G.n_schur;
  sa.lm = lm;
  sa.pair_rt = G.pair_rt.p;
  sa.pair_rt1 = G.pair_rt1.p;
  sa.lvp4 = G.schur_lvp4.p;
  sa.lvp = G.schur_lvp.p;
  sa.rt_off = G.schur_rt_off;
  return sa;
}
// … and the previous trial's accept with them: state ← candidate where the record says accepted (AcceptCopy)
static void schur_accept_args(SchurArgs& sa, pba_engine* e) {
  const GnData& G = e->gn;
  sa.poses = e->poses.p;
  sa.poses_new = G.poses_new.p;
  sa.rho = e->rho.p;
  sa.rho_new = G.rho_new.p;
  sa.pt_orig = G.pt_orig.p;
  sa.n_pose_d = 7 * e->n_frames;
  sa.n_gn_points = G.n_gn_points;
}

// What assemble_kernel and export_band_kernel both read: the linearisation and Schur partials, the contribution lists,
// the system's outputs, with the record lm.  Everything else zero, set by name where it is used.
static AsmArgs asm_args(const GnData& G, const double* lm) {
  AsmArgs a{};
  a.part_lin = G.part_lin.p;
  a.part_lin1 = G.part_lin1.p;
  a.lm = lm;
  a.part_schur = G.part_schur.p;
  a.sky_cptr = G.sky_cptr.p;
  a.sky_contrib = G.sky_contrib.p;
  a.g_cptr = G.g_cptr.p;
  a.g_contrib = G.g_contrib.p;
  a.blk_i = G.sky_blk_i.p;
  a.blk_j = G.sky_blk_j.p;
  a.fixed = G.fixed.p;
  a.S = G.S.p;
  a.g = G.g.p;
  a.g_dir = G.g_dir.p;
  a.Ddiag = G.Ddiag.p;
  a.n_sky = G.n_sky;
  return a;
}

// Dynamic LDS above the default 64 KiB limit (the attribute is per device: set on every launch, cheap).
static void schur_lds_limit(const GnData& G) {
  if (G.schur_lds > 65536)
    for (const void* f : {reinterpret_cast<const void*>(&schur_kernel), reinterpret_cast<const void*>(&schur_gate_kernel),
                          reinterpret_cast<const void*>(&schur_free_decide_kernel)})
      (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G.schur_lds);
}

// Schur complement for λ, assembly and reduced-system solve into G.x (enqueued only).
// lm: the device LM record (λ, buffer set, done flag read on the device; lambda unused) or nullptr.
// free_sets (the single-GPU LM loop without free intrinsics): the current set's λ-free partials, scaled in the assembly,
// and schur_gate_kernel (the accept, the λ-specific elimination only for a degen set) instead of schur_kernel.
int enqueue_solve(pba_engine* e, double lambda, const double* lm, bool free_sets) {
  GnData& G = e->gn;
  const int nf = e->n_frames, nfs = G.nc_sys ? G.nfs : nf;
  SchurArgs sa = schur_args(e, lm ? lm : G.lm_idle.p);
  schur_accept_args(sa, e);
  if (!lm) sa.poses = nullptr;  // a host-driven step: no accept to apply
  // free intrinsics: the elimination's launch also applies the previous trial's intrinsics accept (no launch of its own)
  const bool kacc = G.nc_sys && lm && !free_sets && G.n_schur > 0;
  if (kacc) {
    sa.knew_d = G.intr_new_d.p;
    sa.knew_f = G.intr_new_f.p;
    sa.k_d = e->intr_state_d.p;
    sa.k_f = e->intr_state.p;
    sa.n_intr = G.nc_sys;
  }
  schur_lds_limit(G);
  if (free_sets)
    schur_gate_kernel<<<std::max(1, std::min(G.n_schur, 512)), kBlockThreads, G.schur_lds, e->stream>>>(sa, G.degen.p);
  else
    schur_kernel<<<G.n_schur, kBlockThreads, G.schur_lds, e->stream>>>(sa, lambda);
  if (G.nc_sys) enqueue_intr_rows(e, lm, !kacc);
  // block cyclic reduction: assemble writes its level 0 directly (no Sband, no cr_build pass)
  const bool direct = G.band_kernel && G.solver == SOLVER_CR;
  if (direct && G.cr0_dirty)  // a distributed solve rebuilt level 0 over the whole band: back to zeros + padding
    if (int rc = init_cr_level0(e)) return rc;
  CrLevel L0 = direct ? cr_level(G, 0) : CrLevel{};
  AsmArgs aa = asm_args(G, lm ? lm : G.lm_idle.p);
  aa.Sband = G.band_kernel && !direct ? G.Sband.p : nullptr;
  aa.band = G.band_kernel;
  aa.n_frames = nfs;
  aa.crD = direct ? L0.D : nullptr;
  aa.crU = L0.U;
  aa.crb = L0.b;
  aa.crB = G.band_kernel;
  aa.status = G.status.p;
  if (free_sets) {
    aa.part_free0 = G.part_free0.p;
    aa.part_free1 = G.part_free1.p;
    aa.degen = G.degen.p;
  }
  aa.sky_diag = G.sky_diag.p;
  aa.sky_off = G.sky_off.p;
  aa.n_diag = G.n_sky_diag;
  if (G.sband_dirty && G.band_kernel && !direct) {  // a distributed import filled the whole band: clear the off-profile part
    PBA_HIP(hipMemsetAsync(G.Sband.p, 0, sizeof(double) * (size_t)nf * ((G.band_kernel + 1) * 36 + 6), e->stream));
    G.sband_dirty = false;
  }
  const int nthreads = (G.n_sky + (kAsmSeg - 1) * G.n_sky_diag) * 36 + 6 * nfs * kAsmSeg;
  assemble_kernel<<<(nthreads + 255) / 256, 256, 0, e->stream>>>(aa, lambda);
  // the intrinsics rows of the skyline system (over assemble's zeros); an arrow solve's level 0 in the same launch
  const bool arrow = G.nc_sys && !G.band_kernel && arrow_for(e, G.band);
  if (G.nc_sys) enqueue_border(e, lambda, lm, nullptr, arrow);
  if (G.band_kernel) {
    if (int rc = band_solve(e, !direct)) return rc;
  } else {
    const SkylineSystem s{G.S.p, G.L.p, G.sky_first.p, G.sky_row.p, G.sky_last.p, G.sky_colptr.p, G.sky_colrows.p,
                          G.front, G.fixed.p, nfs, G.n_sky};
    return skyline_solve(e, s, arrow ? ArrowUse::built : ArrowUse::none);
  }
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

// Schur complement for λ, assembly, solve and candidate state; returns the LM model decrease.
static int gn_step(pba_engine* e, double lambda, double* model_decrease, int* solver_status) {
  if (int rc = enqueue_solve(e, lambda)) return rc;
  double mp = 0.0, mq = 0.0;
  if (int rc = finish_step(e, lambda, e->gn.fixed.p, &mp, &mq, solver_status)) return rc;
  if (model_decrease) *model_decrease = mp + mq;
  return PBA_OK;
}

// state ← candidate (poses, and the inverse distances of the Gauss-Newton points), gated by lm when given
void launch_accept(pba_engine* e, const double* lm) {
  GnData& G = e->gn;
  const int npd = 7 * e->n_frames;
  const int na = std::max(npd, G.n_gn_points);
  lm_accept_kernel<<<std::min(1024, (na + 255) / 256), 256, 0, e->stream>>>(lm, G.poses_new.p, G.rho_new.p, G.pt_orig.p,
                                                                             e->poses.p, e->rho.p, npd, G.n_gn_points);
  if (G.nc_sys) launch_intr_accept(e, lm);
  e->pairs_fresh = false;
}

// A multi-GPU trial's first launch: the point elimination at the record's λ, which applies the previous trial's accept
// first — or, on a rank without points, the accept alone.
void launch_schur_accept(pba_engine* e, const double* lm) {
  GnData& G = e->gn;
  SchurArgs sa = schur_args(e, lm);
  schur_accept_args(sa, e);
  schur_lds_limit(G);
  if (G.n_schur > 0) schur_kernel<<<G.n_schur, kBlockThreads, G.schur_lds, e->stream>>>(sa, 0.0);
  else launch_accept(e, lm);
}

// The λ-free point elimination's launch after a linearisation (schur_free_decide_kernel): workgroup 0 the decision of
// trial seq (init: the record of a new solve), the others the set's partials.
void launch_free_decide(pba_engine* e, const DecideOpts& dopt, double seq, int gp, int gq, bool init, double radius) {
  GnData& G = e->gn;
  SchurArgs sa = schur_args(e, G.lm.p);  // (no accept here; the counts as the other launches of the loop pass them)
  sa.n_pose_d = 7 * e->n_frames;
  sa.n_gn_points = G.n_gn_points;
  DecideArgs da{G.red.p, G.red2.p, G.gmax.p, gp, gq, G.n_chunks, G.status.p, dopt, G.lm.p,
                init ? nullptr : G.lm_host_d + rec_slot(seq), seq, init ? 1 : 0, radius, G.lm_init.p,
                G.ts_part.p, G.ts_count.p};
  FreeSets fs{{G.part_free0.p, G.part_free1.p}, {G.pt_data.p, G.pt_data1.p}, G.degen.p, G.lin_set.p};
  schur_lds_limit(G);
  schur_free_decide_kernel<<<kDecideWgs + G.n_schur, kBlockThreads, G.schur_lds, e->stream>>>(sa, da, fs);
  // tests: every set flagged, so every trial takes the λ-specific elimination (the degenerate-point path)
  if (G.force_degen) (void)hipMemsetAsync(G.degen.p, 0x01, 2 * sizeof(int), e->stream);
}

// free intrinsics keep the per-trial elimination (their border kernels read its point data at the trial's λ)
bool lm_free_sets(const pba_engine* e) { return e->gn.nc_sys == 0 && e->gn.n_schur > 0; }

static int candidate_cost(pba_engine* e, double* cost) {
  GnData& G = e->gn;
  if (e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC) {
    // the candidate poses straight into the fused-state prologue: no pair-table launch (C4: 32.4 → 29.8 µs for the
    // cost launch, and the 7.6-µs pair launch gone)
    if (int rc = launch_cost_only(e, G.pairs_new.p, G.rho_new.p, nullptr, nullptr, G.poses_new.p,
                                  G.nc_sys ? G.intr_new_f.p : nullptr, G.nc_sys ? G.intr_new_d.p : nullptr))
      return rc;
    return total_cost(e, cost, nullptr);
  }
  if (!G.pairs_new_fresh) launch_pairs(e, G.poses_new.p, G.pairs_new.p);
  if (int rc = launch_cost_only(e, G.pairs_new.p, G.rho_new.p, nullptr, nullptr, nullptr,
                                G.nc_sys ? G.intr_new_f.p : nullptr, G.nc_sys ? G.intr_new_d.p : nullptr))
    return rc;
  return total_cost(e, cost, nullptr);
}

static int accept(pba_engine* e) {
  launch_accept(e, nullptr);
  e->joint.linearized = false;
  PBA_HIP(hipGetLastError());
  // a photometric engine's host copy of the (level-0) intrinsics state follows the device state
  if (e->gn.nc_sys) return download_intrinsics_state(e);
  return PBA_OK;
}

// ---- multi-GPU step (include/pba.h) ------------------------------------------------------------
int exchange_K(pba_engine* e, int band, int* K) {
  *K = band_kernel_for(std::max(band, e->gn.band));
  if (band < e->gn.band) return fail(PBA_ERR_INVALID_ARGUMENT, "band below this rank's reduced-system bandwidth");
  if (*K == 0) return fail(PBA_ERR_INVALID_ARGUMENT, "distributed solve needs a reduced-system bandwidth <= 16");
  return PBA_OK;
}

// The exchange buffer: the keyframes' band rows (nf × ex_row(K)), with free intrinsics the 2·nc border rows
// (nfs·36 + EX_TAIL each), then the kExScalars scalar slots of the device-steered loop.
static long long ex_border(const pba_engine* e) {
  const GnData& G = e->gn;
  return G.nc_sys ? 2LL * G.nc_sys * ((long long)G.nfs * 36 + EX_TAIL) : 0;
}
long long ex_scalar_off(const pba_engine* e, int K) { return (long long)e->n_frames * ex_row(K) + ex_border(e); }
long long exchange_count(pba_engine* e, int K) { return ex_scalar_off(e, K) + kExScalars; }

// The summed profile of a multi-GPU free-intrinsics solve (band K over the keyframes, border rows from frame 0): its
// skyline layout and front_solve_kernel plan, built once per K.
static int ensure_dist_sky(pba_engine* e, int K) {
  GnData& G = e->gn;
  if (G.dsky_K == K) return PBA_OK;
  const int nf = e->n_frames, nfs = G.nfs;
  std::vector<int> first(nfs), rowp, last, ccptr, ccrows;
  for (int i = 0; i < nfs; ++i) first[i] = i < nf ? std::max(0, i - K) : 0;
  skyline_profile(first, rowp, last, ccptr, ccrows);
  if (int rc = build_front_plan(first, rowp, ccptr, ccrows, e->stream, G.dfront, true)) return rc;
  // (a front beyond LDS — many cameras or a wide band — is solved through global memory, skyline_solve_kernel)
  G.n_dsky = rowp[nfs];
  PBA_HIP(G.dS.resize((size_t)G.n_dsky * 36));
  PBA_HIP(G.dL.resize((size_t)G.n_dsky * 36));
  PBA_HIP(G.dsky_row.upload(rowp, e->stream));
  PBA_HIP(G.dsky_first.upload(first, e->stream));
  PBA_HIP(G.dsky_last.upload(last, e->stream));
  PBA_HIP(G.dsky_colptr.upload(ccptr, e->stream));
  PBA_HIP(G.dsky_colrows.upload(ccrows, e->stream));  // (never empty: profile_columns)
  G.dsky_K = K;
  return PBA_OK;
}

// This rank's partial system into the exchange buffer X (every element written: no fill launch); with free
// intrinsics also the border rows (after this trial's accept and point elimination: the rows at the state, the Schur
// terms at λ — the LM record's, or `lambda` for a host-driven step).
int enqueue_export(pba_engine* e, double lambda, const double* lm, double* X, int K) {
  GnData& G = e->gn;
  const int nf = e->n_frames;
  AsmArgs aa = asm_args(G, lm);
  aa.band = K;
  aa.n_frames = nf;
  const long long n = (long long)nf * ex_row(K);  // (K+1)·36 band + EX_TAIL tail lanes per frame
  export_band_kernel<<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(aa, G.observed.p, G.sky_first.p, G.sky_row.p,
                                                                        X, K);
  if (G.nc_sys) {
    enqueue_intr_rows(e, lm == G.lm_idle.p ? nullptr : lm);
    enqueue_border(e, lambda, lm, X + n);
  }
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

// The summed exchange → damping, constant frames and the band solver's input — for block cyclic reduction its level 0
// directly (no Sband, no cr_build pass), as assemble_kernel does on one GPU — then the reduced solve into G.x.
int enqueue_import(pba_engine* e, double lambda, const double* lm, const double* X, int K) {
  GnData& G = e->gn;
  const int nf = e->n_frames;
  if (G.nc_sys) {  // free intrinsics: the summed skyline system (band + border) — an arrow, or the skyline solvers
    if (int rc = ensure_dist_sky(e, K)) return rc;
    const int nfs = G.nfs;
    ImportSkyArgs ia{X, X + (long long)nf * ex_row(K), G.fixed_req.p, G.dsky_row.p, G.dS.p, G.g.p, G.g_dir.p,
                     G.Ddiag.p, G.fixed_dist.p, nf, G.nc_sys, K, (long long)G.n_dsky * 36};
    const long long n = ia.n_el + 6LL * nfs;
    import_sky_kernel<<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(ia, lambda, lm);
    PBA_HIP(hipGetLastError());
    const SkylineSystem s{G.dS.p, G.dL.p, G.dsky_first.p, G.dsky_row.p, G.dsky_last.p, G.dsky_colptr.p, G.dsky_colrows.p,
                          G.dfront, G.fixed_dist.p, nfs, G.n_dsky};
    return skyline_solve(e, s, arrow_for(e, K) ? ArrowUse::build : ArrowUse::none);
  }
  const bool direct = G.solver == SOLVER_CR;
  if (direct && !G.cr0_inited)  // zeros outside the band, identity padding rows
    if (int rc = init_cr_level0(e)) return rc;
  CrLevel L0 = direct ? cr_level(G, 0) : CrLevel{};
  ImportArgs ia{X, G.fixed_req.p, G.Sband.p, G.g.p, G.g_dir.p, G.Ddiag.p, G.fixed_dist.p, nf, K,
                direct ? L0.D : nullptr, L0.U, L0.b, G.status.p};
  const long long n = (long long)nf * ((K + 1) * 36 + 6);
  import_kernel<<<(unsigned)((n + 255) / 256), 256, 0, e->stream>>>(ia, lambda, lm);
  PBA_HIP(hipGetLastError());
  G.sband_dirty = !direct;
  G.cr0_dirty = true;  // level 0 holds the whole band now: a single-GPU assembly re-initialises it first
  return band_solve(e, !direct);
}

static int step_export(pba_engine* e, double lambda, int band, double* X) {
  GnData& G = e->gn;
  int K;
  if (int rc = exchange_K(e, band, &K)) return rc;
  const SchurArgs sa = schur_args(e, G.lm_idle.p);  // (a host-driven step: no accept, the counts 0)
  schur_lds_limit(G);
  if (G.n_schur > 0) schur_kernel<<<G.n_schur, kBlockThreads, G.schur_lds, e->stream>>>(sa, lambda);
  return enqueue_export(e, lambda, G.lm_idle.p, X, K);
}

static int step_import(pba_engine* e, double lambda, int band, const double* X, double* model_pose,
                       double* model_points, int* solver_status) {
  GnData& G = e->gn;
  int K;
  if (int rc = exchange_K(e, band, &K)) return rc;
  if (int rc = ensure_exchange_solver(e, K)) return rc;
  if (int rc = enqueue_import(e, lambda, G.lm_idle.p, X, K)) return rc;
  return finish_step(e, lambda, G.fixed_dist.p, model_pose, model_points, solver_status);
}

}  // namespace detail
}  // namespace pba

extern "C" {

int pba_set_fixed_frames(pba_engine* e, int32_t n, const int32_t* frames) {
  if (!e || n < 0 || (n > 0 && !frames)) return fail(PBA_ERR_INVALID_ARGUMENT, "bad fixed-frame arguments");
  if (e->n_frames <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_frames first");
  std::vector<uint8_t> f(e->n_frames, 0);
  for (int i = 0; i < n; ++i) {
    if (frames[i] < 0 || frames[i] >= e->n_frames) return fail(PBA_ERR_INVALID_ARGUMENT, "fixed frame out of range");
    f[frames[i]] = 1;
  }
  e->gn.fixed_h = f;
  e->gn.prepared = false;
  e->joint.linearized = false;
  return PBA_OK;
}

int pba_gn_linearize(pba_engine* e, double* cost) {
  if (int rc = ensure_prepared(e)) return rc;
  return linearize(e, cost);
}

int pba_gn_step(pba_engine* e, double lambda, double* model_decrease, int32_t* solver_status) {
  if (int rc = ensure_prepared(e)) return rc;
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  int st = 0;
  const int rc = gn_step(e, lambda, model_decrease, &st);
  if (solver_status) *solver_status = st;
  return rc;
}

int pba_gn_candidate_cost(pba_engine* e, double* cost) {
  if (int rc = ensure_prepared(e)) return rc;
  if (!cost) return fail(PBA_ERR_INVALID_ARGUMENT, "null cost");
  return candidate_cost(e, cost);
}

int pba_gn_accept(pba_engine* e) {
  if (int rc = ensure_prepared(e)) return rc;
  return accept(e);
}

int pba_get_state(pba_engine* e, double* poses, double* inv_dist) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (!e->state_set) return fail(PBA_ERR_NOT_READY, "pba_set_state first");
  if (int rc = check_device(e)) return rc;
  if (poses) PBA_HIP(hipMemcpyAsync(poses, e->poses.p, sizeof(double) * 7 * e->n_frames, hipMemcpyDeviceToHost, e->stream));
  if (inv_dist) PBA_HIP(hipMemcpyAsync(inv_dist, e->rho.p, sizeof(double) * e->n_points, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_gn_get_reduced_system(pba_engine* e, double* S_dense, double* g) {
  if (int rc = ensure_prepared(e)) return rc;
  GnData& G = e->gn;
  const int nf = G.nc_sys ? G.nfs : e->n_frames;  // system frames (pba_gn_system_size)
  std::vector<int> first(nf), row(nf + 1);
  PBA_HIP(hipMemcpy(first.data(), G.sky_first.p, sizeof(int) * nf, hipMemcpyDeviceToHost));
  PBA_HIP(hipMemcpy(row.data(), G.sky_row.p, sizeof(int) * (nf + 1), hipMemcpyDeviceToHost));
  if (S_dense) {
    std::vector<double> sky((size_t)G.n_sky * 36);
    PBA_HIP(hipMemcpy(sky.data(), G.S.p, sizeof(double) * sky.size(), hipMemcpyDeviceToHost));
    const size_t n = 6 * (size_t)nf;
    std::fill(S_dense, S_dense + n * n, 0.0);
    for (int i = 0; i < nf; ++i)
      for (int j = first[i]; j <= i; ++j) {
        const double* B = &sky[((size_t)row[i] + (j - first[i])) * 36];
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) {
            S_dense[(6 * i + r) * n + 6 * j + c] = B[r * 6 + c];
            S_dense[(6 * j + c) * n + 6 * i + r] = B[r * 6 + c];
          }
      }
  }
  if (g) PBA_HIP(hipMemcpy(g, G.g.p, sizeof(double) * 6 * nf, hipMemcpyDeviceToHost));
  return PBA_OK;
}

int pba_gn_get_step(pba_engine* e, double* dposes, double* drho) {
  if (int rc = ensure_prepared(e)) return rc;
  GnData& G = e->gn;
  if (dposes) PBA_HIP(hipMemcpy(dposes, G.x.p, sizeof(double) * 6 * e->n_frames, hipMemcpyDeviceToHost));
  if (drho) PBA_HIP(hipMemcpy(drho, G.drho.p, sizeof(double) * e->n_points, hipMemcpyDeviceToHost));
  return PBA_OK;
}

int pba_gn_set_rank(pba_engine* e, int32_t rank) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  e->gn.dist_rank = rank < 0 ? -1 : rank;
  return PBA_OK;
}

int pba_gn_system_size(pba_engine* e, int32_t* n) {
  if (int rc = ensure_prepared(e)) return rc;
  if (!n) return fail(PBA_ERR_INVALID_ARGUMENT, "null size");
  *n = 6 * (e->gn.nc_sys ? e->gn.nfs : e->n_frames);
  return PBA_OK;
}

int pba_gn_band(pba_engine* e, int32_t* band) {
  if (int rc = ensure_prepared(e)) return rc;
  if (!band) return fail(PBA_ERR_INVALID_ARGUMENT, "null band");
  *band = e->gn.band;
  return PBA_OK;
}

int pba_gn_exchange_size(pba_engine* e, int32_t band, int64_t* count) {
  if (int rc = ensure_prepared(e)) return rc;
  if (!count) return fail(PBA_ERR_INVALID_ARGUMENT, "null count");
  int K;
  if (int rc = exchange_K(e, band, &K)) return rc;
  *count = exchange_count(e, K);
  return PBA_OK;
}

int pba_gn_step_export(pba_engine* e, double lambda, int32_t band, double* d_exchange) {
  if (int rc = ensure_prepared(e, true)) return rc;
  if (!d_exchange) return fail(PBA_ERR_INVALID_ARGUMENT, "null exchange buffer");
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  if (int rc = step_export(e, lambda, band, d_exchange)) return rc;
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_gn_step_import(pba_engine* e, double lambda, int32_t band, const double* d_exchange, double* model_pose,
                       double* model_points, int32_t* solver_status) {
  if (int rc = ensure_prepared(e, true)) return rc;
  if (!d_exchange) return fail(PBA_ERR_INVALID_ARGUMENT, "null exchange buffer");
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  double mp = 0.0, mq = 0.0;
  int st = 0;
  if (int rc = step_import(e, lambda, band, d_exchange, &mp, &mq, &st)) return rc;
  if (model_pose) *model_pose = mp;
  if (model_points) *model_points = mq;
  if (solver_status) *solver_status = st;
  return PBA_OK;
}

}  // extern "C"
