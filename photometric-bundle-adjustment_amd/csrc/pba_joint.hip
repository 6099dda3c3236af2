// pba_joint.hip — the joint solve of poses, inverse distances and affine brightness (include/pba.h pba_joint_*,
// pba_solve_joint): photometric engines with pba_set_affine_brightness — and, under pba_joint_set_solve_intrinsics, of
// the target cameras' intrinsics too (engines with pba_set_optimize_intrinsics as well; the second half of the kernels,
// from joint_intr_moments_kernel on).
//
// Unknowns: 8 per keyframe, [δpose (6, T·exp δ) | δa δb], and one δρ per point.  A block (host h, target t, point p) has
// the rows J = [J_h | J_ab,h | J_t | J_ab,t | J_ρ] and r of the 18·P record.  With Ad the adjoint of T_th,
// [hv hw] = −[tv tw]·Ad (pba_gn_linearize.hip), and with E = exp(a_t − a_h), c_k = I_h,k − b_h,
// J_ab,h = [E·c, E], J_ab,t = [−E·c, −1]: every column is a combination of the ten columns
//   x = [tv(3) tw(3) jr c 1 r],
// so a block's whole contribution to the normal equations is w·xᵀx (w = ρ′(Σr²), Ceres' Corrector with ρ″ ≤ 0) — 55
// doubles whatever P — and Ad and E are the pair's.
//
// Moment record, 64 doubles per block (joint_moments_kernel): [0, 55) the upper triangle of w·xᵀx, row-major
// (up(i, j) = 10·i − i(i−1)/2 + j − i, i ≤ j); 55 w; 56 E; 57 the block's cost ½ρ(Σr²); 58 valid (1 / 0); 59…63 zero.
// An invalid block's record is all zeros.
// Pair record, kPairRec doubles (joint_pair_kernel): the 16×16 JᵀwJ over [pose_h(6) a_h b_h pose_t(6) a_t b_t], row
// major; 256 the 16 gradient entries; 272 the pair's valid blocks.  pair_ad: Ad (36, row-major) and E.
// Block data, kBlk doubles (joint_block_kernel): H_ρρ, g_ρ, W_t(8), W_h(8) with W = JᵀwJ_ρ.
// Point data, kPt doubles (joint_point_kernel): H_ρρ, g_ρ, has blocks, 0, W_h(8) summed over its blocks.
// Frame data, kFrame doubles (joint_frame_kernel): the direct gradient (8) and the direct diagonal (8).
// Everything across blocks is fp64 in the fixed order of the host-built lists (pba_joint_plan.h), without atomics.
// The reduced system is an 8×8-block lower skyline over the pose system's profile, damped as Ceres' LM strategy does
// (levenberg_marquardt_strategy.cc) and factored right-looking by one workgroup (joint_solve_kernel, modelled on
// skyline_solve_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "pba_host_lm.h"
#include "pba_internal.h"
#include "pba_joint_plan.h"

using namespace pba;
using namespace pba::detail;

namespace {

constexpr int kCols = 10;      // x = [tv tw jr c 1 r]
constexpr int kMom = 55;       // upper triangle of xᵀx
constexpr int kRec = 64;       // doubles per block moment record
constexpr int kPairRec = 280;  // doubles per pair record (256 + 16 + valid, padded)
constexpr int kPairAd = 40;    // Ad (36), E, padding
constexpr int kBlk = 20;       // H_ρρ, g_ρ, W_t(8), W_h(8), padding
constexpr int kPt = 12;        // H_ρρ, g_ρ, has blocks, 0, W_h(8)
constexpr int kFrame = 16;     // direct gradient (8), direct diagonal (8)

__host__ __device__ constexpr int up(int i, int j) { return 10 * i - i * (i - 1) / 2 + (j - i); }  // i ≤ j < 10
static_assert(up(9, 9) == kMom - 1, "upper triangle of 10 columns");

__device__ __forceinline__ double lm_clamp(double d) { return fmin(fmax(d, 1e-6), 1e32); }

// Free intrinsics (pba_joint_set_solve_intrinsics; the layouts are at joint_intr_moments_kernel below)
constexpr int kColsI = 18;                  // x = [tv tw jr c 1 r | ji(8)]
constexpr int kCross = 80, kTri = 36;       // ji × x (8×10), upper triangle of ji × ji
constexpr int kMomI = kMom + kCross + kTri; // 171 moments per block
constexpr int kIntrRec = 128;               // doubles per block intrinsics record (80 + 36, padded: 1 KB)
constexpr int kPairIntr = 208;              // doubles per pair: border 8×16, jiᵀwji 8×8 at 128, jiᵀwr at 192, padding
constexpr int kCam = 80;                    // per camera: direct gradient (8), direct jiᵀwji (8×8, full; the diagonal at 8 + 9r), padding
constexpr int kCamVals = 73;                // … summed over the camera's pairs: those 72 and the valid blocks
constexpr int kTermChunk = 1024;            // Schur terms per partial sum of a camera's skyline block
constexpr int kEntryChunk = 2048;           // entries per partial sum of a camera's gradient
__host__ __device__ constexpr int up8(int i, int j) { return 8 * i - i * (i - 1) / 2 + (j - i); }  // i ≤ j < 8
static_assert(up8(7, 7) == kTri - 1, "upper triangle of 8 columns");

// Producer.  The layout of affine_moments_kernel: 8 lanes per block, ⌈P/8⌉ rows per lane (a launch scalar), the
// fused-state prologue (a.poses), block_affine and photometric_row<…, JAC, …, AFF> — the record path's rows.  Each pass
// stages its 8 rows per block in LDS and the block's lanes deal the 55 moments among them (lane k: moments k, k + 8, …),
// summing the rows in pixel order: a fixed order, no atomics.  Products of fp32 values are exact in fp64.  ρ′ and the
// block's validity are formed as the linearisation forms them (fp32 Σr² per lane, the DPP group sum, huber_weight) and
// ρ′ scales the moments after the last pass.
template <int PM>
__global__ __launch_bounds__(kBlockThreads) void joint_moments_kernel(const KernelArgs a, double* __restrict__ rec,
                                                                     int ppl) {
  constexpr int LPB = 8, BPW = kBlockThreads / LPB, NQ = (kMom + LPB - 1) / LPB;
  __shared__ __attribute__((aligned(16))) TileBlock s_tb[BPW];
  __shared__ float2 s_pat[PBA_MAX_PATTERN];
  __shared__ float s_x[BPW][LPB][kCols];
  const int P = a.P;
  const int blk0 = logical_tile() * BPW;
  const int lb = threadIdx.x / LPB, k = threadIdx.x % LPB;
  const int blk = blk0 + lb;
  const bool live = blk < a.n_blocks;
  const int bq = live ? blk : a.n_blocks - 1;  // a dead block evaluates the last block, masked below
  for (int i = threadIdx.x; i < P; i += kBlockThreads) s_pat[i] = make_float2(a.pattern[2 * i], a.pattern[2 * i + 1]);
  const int pt = stage_tile<LPB>(a, s_tb, lb, k, blk, live);
  const Affine af = block_affine(a, bq);
  int mi[NQ], mj[NQ];  // this lane's moments (i ≤ j); a lane past the last moment repeats moment 0 and does not store
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int m = k + LPB * q;
    int i = 0, rem = m < kMom ? m : 0;
    while (rem >= kCols - i) {
      rem -= kCols - i;
      ++i;
    }
    mi[q] = i;
    mj[q] = i + rem;
  }
  __syncthreads();
  int okl = 1;
  float s = 0.0f;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int j = 0; j < ppl; ++j) {
    const int px = k + LPB * j;
    const bool act = live && px < P;
    const float Ih = act ? a.host_int[(long long)pt * P + px] : 0.0f;
    const Row row = photometric_row<PM, true, TileBlock, false, false, true>(a, s_tb[lb], s_pat[act ? px : 0], Ih,
                                                                              nullptr, nullptr, &af);
    const bool use = act && row.ok;
    okl &= act ? row.ok : 1;
    s += use ? row.r * row.r : 0.0f;
    float* x = s_x[lb][k];
    x[0] = use ? row.tv.x : 0.0f;
    x[1] = use ? row.tv.y : 0.0f;
    x[2] = use ? row.tv.z : 0.0f;
    x[3] = use ? row.tw.x : 0.0f;
    x[4] = use ? row.tw.y : 0.0f;
    x[5] = use ? row.tw.z : 0.0f;
    x[6] = use ? row.jr : 0.0f;
    x[7] = use ? Ih - af.bh : 0.0f;
    x[8] = use ? 1.0f : 0.0f;
    x[9] = use ? row.r : 0.0f;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      for (int r = 0; r < LPB; ++r) acc[q] += (double)s_x[lb][r][mi[q]] * (double)s_x[lb][r][mj[q]];
    __syncthreads();
  }
  const int ok = group_all<LPB>(okl);
  s = group_sum<LPB>(s);
  const float w = ok ? huber_weight(s, a.huber) : 0.0f;
  const float bc = ok ? huber_cost(s, a.huber) : 0.0f;
  if (live) {
    double* o = rec + (long long)blk * kRec;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int m = k + LPB * q;
      if (m < kMom) o[m] = ok ? (double)w * acc[q] : 0.0;
    }
    // the tail: 55 w, 56 E, 57 cost, 58 valid, 59…63 zero — one value per lane, lane 7 the last two
    const double tail = k == 0 ? (double)w : k == 1 ? (ok ? (double)af.E : 0.0) : k == 2 ? (double)bc : k == 3 ? (ok ? 1.0 : 0.0) : 0.0;
    o[kMom + k] = tail;
    if (k == LPB - 1) o[kRec - 1] = 0.0;
  }
  if (a.wg_red) {
    const bool one = live && k == 0;
    wg_reduce2(one ? (double)bc : 0.0, one && ok ? 1.0 : 0.0, a.wg_red + 2 * logical_tile());
  }
}

struct RelPose {  // pair_rotation / pair_translation's fields
  double R[9], t[3];
  float Rf[9], tf[3];
};

// One 64-thread workgroup per pair: its blocks' moments summed in block order, then JᵀwJ = Mᵀ(Σ w xᵀx)M and
// Jᵀwr = Mᵀ(Σ w xᵀr) with the 10×16 map M from x to [J_h | J_ab,h | J_t | J_ab,t]: J_h = −J_t·Ad, J_ab,h = [E·c, E],
// J_ab,t = [−E·c, −1].  Ad = [[R, [t]×R], [0, R]] of T_th from the two state poses in fp64 (form_pair's arithmetic).
__global__ __launch_bounds__(64) void joint_pair_kernel(const double* __restrict__ rec, const int* __restrict__ pair_ptr,
                                                        const int* __restrict__ pair_blocks,
                                                        const int* __restrict__ pair_host,
                                                        const int* __restrict__ pair_target,
                                                        const double* __restrict__ poses, double* __restrict__ pair_rec,
                                                        double* __restrict__ pair_ad) {
  __shared__ double sQ[kCols][kCols], sM[kCols][16], sT[kCols][16], sAd[36], sE[2];
  const int p = blockIdx.x, t = threadIdx.x;
  const int q0 = pair_ptr[p], q1 = pair_ptr[p + 1];
  if (t < kMom) {
    double m = 0.0;
    for (int q = q0; q < q1; ++q) m += rec[(long long)pair_blocks[q] * kRec + t];
    int i = 0, rem = t;
    while (rem >= kCols - i) {
      rem -= kCols - i;
      ++i;
    }
    sQ[i][i + rem] = m;
    sQ[i + rem][i] = m;
  } else if (t == kMom) {
    double E = 0.0, nv = 0.0;  // every valid block of the pair has the pair's E
    for (int q = q1 - 1; q >= q0; --q) {
      const double* b = rec + (long long)pair_blocks[q] * kRec;
      if (b[58] != 0.0) E = b[56];
      nv += b[58];
    }
    sE[0] = E;
    sE[1] = nv;
  } else if (t == kMom + 1) {
    RelPose rp;
    pair_rotation(poses + 7 * pair_host[p], poses + 7 * pair_target[p], rp);
    pair_translation(poses + 7 * pair_host[p], poses + 7 * pair_target[p], rp);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
        sAd[r * 6 + c] = rp.R[r * 3 + c];
        sAd[r * 6 + 3 + c] = rp.t[r1] * rp.R[r2 * 3 + c] - rp.t[r2] * rp.R[r1 * 3 + c];
        sAd[(3 + r) * 6 + c] = 0.0;
        sAd[(3 + r) * 6 + 3 + c] = rp.R[r * 3 + c];
      }
  }
  __syncthreads();
  const double E = sE[0];
  for (int idx = t; idx < kCols * 16; idx += 64) {
    const int q = idx / 16, c = idx % 16;
    double v = 0.0;
    if (c < 6) v = q < 6 ? -sAd[q * 6 + c] : 0.0;
    else if (c == 6) v = q == 7 ? E : 0.0;
    else if (c == 7) v = q == 8 ? E : 0.0;
    else if (c < 14) v = q == c - 8 ? 1.0 : 0.0;
    else if (c == 14) v = q == 7 ? -E : 0.0;
    else v = q == 8 ? -1.0 : 0.0;
    sM[q][c] = v;
  }
  __syncthreads();
  for (int idx = t; idx < kCols * 16; idx += 64) {
    const int q = idx / 16, c = idx % 16;
    double v = 0.0;
    for (int m = 0; m < kCols - 1; ++m) v += sQ[q][m] * sM[m][c];  // (M's row of r is zero)
    sT[q][c] = v;
  }
  __syncthreads();
  double* o = pair_rec + (long long)p * kPairRec;
  for (int idx = t; idx < 256; idx += 64) {
    const int r = idx / 16, c = idx % 16;
    double v = 0.0;
    for (int q = 0; q < kCols - 1; ++q) v += sM[q][r] * sT[q][c];
    o[idx] = v;
  }
  if (t < 16) o[256 + t] = sT[kCols - 1][t];
  if (t == 16) o[272] = sE[1];
  if (t > 16 && t < 24) o[256 + t] = 0.0;
  double* ad = pair_ad + (long long)p * kPairAd;
  if (t < 36) ad[t] = sAd[t];
  if (t >= 36 && t < kPairAd) ad[t] = t == 36 ? E : 0.0;
}

// One thread per block: H_ρρ, g_ρ and the two 8-vectors W_t, W_h = JᵀwJ_ρ from its moments of column jr.
__global__ void joint_block_kernel(const double* __restrict__ rec, const int* __restrict__ block_pair,
                                   const double* __restrict__ pair_ad, int n_blocks, double* __restrict__ blk_data) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const double* m = rec + (long long)b * kRec;
  const double* ad = pair_ad + (long long)block_pair[b] * kPairAd;
  const double E = ad[36];
  double* o = blk_data + (long long)b * kBlk;
  double t6[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) t6[q] = m[up(q, 6)];
  const double mc = m[up(6, 7)], m1 = m[up(6, 8)];
  o[0] = m[up(6, 6)];
  o[1] = m[up(6, 9)];
#pragma unroll
  for (int q = 0; q < 6; ++q) o[2 + q] = t6[q];
  o[8] = -E * mc;
  o[9] = -m1;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) v += ad[q * 6 + c] * t6[q];
    o[10 + c] = -v;
  }
  o[16] = E * mc;
  o[17] = E * m1;
  o[18] = o[19] = 0.0;
}

// One thread per point: its blocks' H_ρρ, g_ρ and W_h in block order; per workgroup max |g_ρ| over the points with
// blocks (the LM loop's gradient norm).
__global__ __launch_bounds__(256) void joint_point_kernel(const double* __restrict__ blk_data,
                                                          const int* __restrict__ pt_ptr,
                                                          const int* __restrict__ pt_blocks, int n_points,
                                                          double* __restrict__ pt_data, double* __restrict__ gmax_p) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  double gm = 0.0;
  if (p < n_points) {
    double H = 0.0, g = 0.0, W[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) W[r] = 0.0;
    const int q0 = pt_ptr[p], q1 = pt_ptr[p + 1];
    for (int q = q0; q < q1; ++q) {
      const double* b = blk_data + (long long)pt_blocks[q] * kBlk;
      H += b[0];
      g += b[1];
#pragma unroll
      for (int r = 0; r < 8; ++r) W[r] += b[10 + r];
    }
    double* o = pt_data + (long long)p * kPt;
    o[0] = H;
    o[1] = g;
    o[2] = q1 > q0 ? 1.0 : 0.0;
    o[3] = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) o[4 + r] = W[r];
    if (q1 > q0) gm = fabs(g);
  }
  double none[1] = {0.0};
  double* const slot[1] = {gmax_p + 2 * blockIdx.x};
  wg_reduce_sum_max<1>(none, gm, slot, slot[0] + 1);
}

// One thread per keyframe: the direct gradient and diagonal over its pairs (as host, then as target), its constants —
// the pose when requested or without a valid block, (a, b) when requested, without a valid block or not finite — and
// its part of the gradient norm max |x − (x ⊞ −g)| (trust_region_minimizer.cc:312-355) over its free halves.
__global__ void joint_frame_kernel(const double* __restrict__ pair_rec, const int* __restrict__ frame_ptr,
                                   const int* __restrict__ frame_pairs, const uint8_t* __restrict__ fixed,
                                   const double* __restrict__ poses, const double* __restrict__ ab, int n_frames,
                                   double* __restrict__ frame_data, uint8_t* __restrict__ cst,
                                   double* __restrict__ gmax_f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_frames) return;
  double g[8], d[8], nv = 0.0;
#pragma unroll
  for (int r = 0; r < 8; ++r) g[r] = d[r] = 0.0;
  for (int q = frame_ptr[i]; q < frame_ptr[i + 1]; ++q) {
    const int e = frame_pairs[q];
    const double* pr = pair_rec + (long long)(e >> 1) * kPairRec;
    const int o = (e & 1) ? 8 : 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      g[r] += pr[256 + o + r];
      d[r] += pr[(o + r) * 16 + o + r];
    }
    nv += pr[272];
  }
  const bool seen = nv > 0.0;
  const bool cp = fixed[2 * i] != 0 || !seen;
  const bool ca = fixed[2 * i + 1] != 0 || !seen || !isfinite(ab[2 * i]) || !isfinite(ab[2 * i + 1]);
  cst[2 * i] = cp ? 1 : 0;
  cst[2 * i + 1] = ca ? 1 : 0;
  double* o = frame_data + (long long)i * kFrame;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    o[r] = g[r];
    o[8 + r] = d[r];
  }
  double gm = 0.0;
  if (!cp) {
    double ng[6], tg[7];
#pragma unroll
    for (int r = 0; r < 6; ++r) ng[r] = -g[r];
    se3_exp_mul(poses + 7 * i, ng, tg);
#pragma unroll
    for (int r = 0; r < 7; ++r) gm = fmax(gm, fabs(poses[7 * i + r] - tg[r]));
  }
  if (!ca) gm = fmax(gm, fmax(fabs(g[6]), fabs(g[7])));
  gmax_f[i] = gm;
}

// ---- free intrinsics (pba_joint_set_solve_intrinsics): poses, ρ, (a, b) and the target cameras' intrinsics -----------
// Unknowns: the keyframes' 8, then 8 per camera, δk with respect to the level-0 intrinsics state, then δρ.  A block's row
// gains J_intr = ji (photometric_row<…, INTR, AFF, PFIN>: the 26-column evaluation's row, columns 0–3 with 2^−level), on
// the camera of its target, so its whole contribution is w·xᵀx over the 18 columns x = [tv tw jr c 1 r | ji(8)].
// joint_intr_moments_kernel is joint_moments_kernel with those rows and writes two records per block: the 64-double
// moment record above, byte for byte in its layout (the keyframe kernels run on it as they are), and the intrinsics
// record, kIntrRec doubles in a second buffer: [0, 80) the cross moments w·ji_a·x_j at 10·a + j, [80, 116) the upper
// triangle of w·ji_a·ji_b at 80 + up8(a, b), zeros to 128; all zeros for an invalid block.
// Pair intrinsics record, kPairIntr doubles (joint_intr_pair_kernel): the 8×16 border jiᵀwJ over [pose_h a_h b_h pose_t
// a_t b_t], row-major; 128 jiᵀwji (8×8, full); 192 jiᵀwr (8).  blk_wc: per block W_c = jiᵀwJ_ρ (8).  Camera data, kCam
// doubles (joint_cam_kernel): the direct gradient (8) and jiᵀwji (8×8) over the camera's pairs; cstc: 1 for a camera no
// valid block targets (identity rows, zero gradient, zero step).
// A rig has few cameras and each sees most of the problem: a camera's diagonal block takes a Schur term from every two
// blocks of every point, its gradient an entry from every block.  So the cameras' sums run in two fixed stages — partial
// sums over chunks of the plan's lists (kTermChunk terms, kEntryChunk entries, the camera's pairs dealt to 64 threads),
// one workgroup each, then the partials in chunk order: still one fixed order, and parallel.
// The reduced system has n_frames + n_cams block rows, the cameras' with a dense profile behind the keyframes' skyline
// (pba_joint_plan.h): joint_assemble_kernel and joint_gradient_kernel fill the keyframes' rows as before, the two
// kernels below the cameras', and joint_solve_kernel factors the whole.
template <int PM>
__global__ __launch_bounds__(kBlockThreads) void joint_intr_moments_kernel(const KernelArgs a, double* __restrict__ rec,
                                                                          double* __restrict__ irec, int ppl) {
  constexpr int LPB = 8, BPW = kBlockThreads / LPB, NQ = (kMomI + LPB - 1) / LPB;
  __shared__ __attribute__((aligned(16))) TileBlock s_tb[BPW];
  __shared__ float2 s_pat[PBA_MAX_PATTERN];
  __shared__ float s_x[BPW][LPB][kColsI];
  const int P = a.P;
  const int blk0 = logical_tile() * BPW;
  const int lb = threadIdx.x / LPB, k = threadIdx.x % LPB;
  const int blk = blk0 + lb;
  const bool live = blk < a.n_blocks;
  const int bq = live ? blk : a.n_blocks - 1;  // a dead block evaluates the last block, masked below
  for (int i = threadIdx.x; i < P; i += kBlockThreads) s_pat[i] = make_float2(a.pattern[2 * i], a.pattern[2 * i + 1]);
  const int pt = stage_tile<LPB>(a, s_tb, lb, k, blk, live);
  const Affine af = block_affine(a, bq);
  // this lane's moments m = k, k + 8, … as column pairs (i, j): [0, 55) joint_moments_kernel's, [55, 135) ji_a × x_j,
  // [135, 171) ji_a × ji_b; a lane past the last moment repeats moment 0 and stores a padding zero
  unsigned char mi[NQ], mj[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int m = k + LPB * q;
    int i = 0, j = 0;
    if (m < kMom) {
      int rem = m;
      while (rem >= kCols - i) {
        rem -= kCols - i;
        ++i;
      }
      j = i + rem;
    } else if (m < kMom + kCross) {
      i = kCols + (m - kMom) / kCols;
      j = (m - kMom) % kCols;
    } else if (m < kMomI) {
      int rem = m - kMom - kCross;
      while (rem >= 8 - i) {
        rem -= 8 - i;
        ++i;
      }
      j = kCols + i + rem;
      i += kCols;
    }
    mi[q] = (unsigned char)i;
    mj[q] = (unsigned char)j;
  }
  __syncthreads();
  int okl = 1;
  float s = 0.0f;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int j = 0; j < ppl; ++j) {
    const int px = k + LPB * j;
    const bool act = live && px < P;
    const float Ih = act ? a.host_int[(long long)pt * P + px] : 0.0f;
    float ji[8];
    const Row row = photometric_row<PM, true, TileBlock, false, true, true, true>(a, s_tb[lb], s_pat[act ? px : 0], Ih,
                                                                                  nullptr, ji, &af);
    const bool use = act && row.ok;
    okl &= act ? row.ok : 1;
    s += use ? row.r * row.r : 0.0f;
    float* x = s_x[lb][k];
    x[0] = use ? row.tv.x : 0.0f;
    x[1] = use ? row.tv.y : 0.0f;
    x[2] = use ? row.tv.z : 0.0f;
    x[3] = use ? row.tw.x : 0.0f;
    x[4] = use ? row.tw.y : 0.0f;
    x[5] = use ? row.tw.z : 0.0f;
    x[6] = use ? row.jr : 0.0f;
    x[7] = use ? Ih - af.bh : 0.0f;
    x[8] = use ? 1.0f : 0.0f;
    x[9] = use ? row.r : 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) x[kCols + c] = use ? ji[c] : 0.0f;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      for (int r = 0; r < LPB; ++r) acc[q] += (double)s_x[lb][r][mi[q]] * (double)s_x[lb][r][mj[q]];
    __syncthreads();
  }
  const int ok = group_all<LPB>(okl);
  s = group_sum<LPB>(s);
  const float w = ok ? huber_weight(s, a.huber) : 0.0f;
  const float bc = ok ? huber_cost(s, a.huber) : 0.0f;
  if (live) {
    double* o = rec + (long long)blk * kRec;
    double* oi = irec + (long long)blk * kIntrRec;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int m = k + LPB * q;
      const double v = ok ? (double)w * acc[q] : 0.0;
      if (m < kMom) o[m] = v;
      else oi[m - kMom] = m < kMomI ? v : 0.0;  // (m < 8·NQ = 176: the padding up to 120)
    }
    if (k < kIntrRec - (LPB * NQ - kMom)) oi[LPB * NQ - kMom + k] = 0.0;  // the padding 121 … 127
    // the tail: 55 w, 56 E, 57 cost, 58 valid, 59…63 zero — one value per lane, lane 7 the last two
    const double tail = k == 0 ? (double)w : k == 1 ? (ok ? (double)af.E : 0.0) : k == 2 ? (double)bc : k == 3 ? (ok ? 1.0 : 0.0) : 0.0;
    o[kMom + k] = tail;
    if (k == LPB - 1) o[kRec - 1] = 0.0;
  }
  if (a.wg_red) {
    const bool one = live && k == 0;
    wg_reduce2(one ? (double)bc : 0.0, one && ok ? 1.0 : 0.0, a.wg_red + 2 * logical_tile());
  }
}
static_assert(8 * ((kMomI + 7) / 8) - kMom <= kIntrRec && kIntrRec - (8 * ((kMomI + 7) / 8) - kMom) <= 8,
              "the intrinsics record's padding is written by the moment lanes and one more store per lane");

// One 128-thread workgroup per pair, after joint_pair_kernel (Ad and E are its pair_ad): the intrinsics records of the
// pair's blocks summed in block order, then the border jiᵀwJ = (Σ w jiᵀx)·M with joint_pair_kernel's map M —
// jiᵀJ_h = −(jiᵀ[tv tw])·Ad, jiᵀJ_ab,h = [E·jiᵀc, E·jiᵀ1], jiᵀJ_t = jiᵀ[tv tw], jiᵀJ_ab,t = [−E·jiᵀc, −jiᵀ1] — and the
// pair's jiᵀwji and jiᵀwr.
__global__ __launch_bounds__(128) void joint_intr_pair_kernel(const double* __restrict__ irec,
                                                              const int* __restrict__ pair_ptr,
                                                              const int* __restrict__ pair_blocks,
                                                              const double* __restrict__ pair_ad,
                                                              double* __restrict__ pair_intr) {
  __shared__ double sC[8][kCols], sT[kTri];
  const int p = blockIdx.x, t = threadIdx.x;
  if (t < kCross + kTri) {
    double m = 0.0;
    for (int q = pair_ptr[p]; q < pair_ptr[p + 1]; ++q) m += irec[(long long)pair_blocks[q] * kIntrRec + t];
    if (t < kCross) sC[t / kCols][t % kCols] = m;
    else sT[t - kCross] = m;
  }
  __syncthreads();
  const double* ad = pair_ad + (long long)p * kPairAd;
  const double E = ad[36];
  double* o = pair_intr + (long long)p * kPairIntr;
  {
    const int r = t / 16, c = t % 16;
    double v = 0.0;
    if (c < 6) {
      for (int q = 0; q < 6; ++q) v += sC[r][q] * ad[q * 6 + c];
      v = -v;
    } else if (c == 6) v = E * sC[r][7];
    else if (c == 7) v = E * sC[r][8];
    else if (c < 14) v = sC[r][c - 8];
    else if (c == 14) v = -E * sC[r][7];
    else v = -sC[r][8];
    o[t] = v;
  }
  if (t < 64) {
    const int r = t / 8, c = t % 8;
    o[128 + t] = sT[up8(r < c ? r : c, r < c ? c : r)];
  }
  if (t < 16) o[192 + t] = t < 8 ? sC[t][kCols - 1] : 0.0;
}

// One thread per block: W_c = jiᵀwJ_ρ (8), the cross moments with column jr.
__global__ void joint_intr_block_kernel(const double* __restrict__ irec, int n_blocks, double* __restrict__ blk_wc) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
#pragma unroll
  for (int r = 0; r < 8; ++r) blk_wc[(long long)b * 8 + r] = irec[(long long)b * kIntrRec + kCols * r + 6];
}

// One 64-thread workgroup per camera: the direct gradient and jiᵀwji over its pairs — thread t sums the pairs t, t + 64,
// … of the list, then thread v sums value v of the 64 partials in thread order — whether a valid block targets it, and
// its part of the gradient norm, max |g| (a plain parameter block: |k − (k − g)|).
__global__ __launch_bounds__(64) void joint_cam_kernel(const double* __restrict__ pair_intr,
                                                        const double* __restrict__ pair_rec,
                                                        const int* __restrict__ cam_ptr, const int* __restrict__ cam_pairs,
                                                        double* __restrict__ cam_data, uint8_t* __restrict__ cstc,
                                                        double* __restrict__ gmax_c) {
  __shared__ double s_p[64][kCamVals], s_v[kCamVals];
  const int c = blockIdx.x, t = threadIdx.x;
  double acc[kCamVals];
#pragma unroll
  for (int v = 0; v < kCamVals; ++v) acc[v] = 0.0;
  for (int q = cam_ptr[c] + t; q < cam_ptr[c + 1]; q += 64) {
    const int p = cam_pairs[q];
    const double* pi = pair_intr + (long long)p * kPairIntr;
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] += pi[192 + r];
#pragma unroll
    for (int v = 0; v < 64; ++v) acc[8 + v] += pi[128 + v];
    acc[72] += pair_rec[(long long)p * kPairRec + 272];
  }
#pragma unroll
  for (int v = 0; v < kCamVals; ++v) s_p[t][v] = acc[v];
  __syncthreads();
  for (int v = t; v < kCamVals; v += 64) {
    double sum = 0.0;
    for (int k = 0; k < 64; ++k) sum += s_p[k][v];
    s_v[v] = sum;
    if (v < 72) cam_data[(long long)c * kCam + v] = sum;
  }
  __syncthreads();
  if (t == 0) {
    const bool seen = s_v[72] > 0.0;
    cstc[c] = seen ? 0 : 1;
    double gm = 0.0;
    for (int r = 0; r < 8; ++r) gm = fmax(gm, fabs(s_v[r]));
    gmax_c[c] = seen ? gm : 0.0;
  }
  if (t >= 72 - 64 && t < kCam - 64) cam_data[(long long)c * kCam + 64 + t] = 0.0;  // the padding 72 … 79
}

// Per point: 1 / H′_ρρ, H′ = H + λ·clamp(H, 1e-6, 1e32); 0 for a point without a valid block (no step).
__global__ void joint_damp_kernel(const double* __restrict__ pt_data, int n_points, double lambda,
                                  double* __restrict__ inv) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_points) return;
  const double H = pt_data[(long long)p * kPt];
  inv[p] = H > 0.0 ? 1.0 / (H + lambda * lm_clamp(H)) : 0.0;
}

struct AsmArgsJ {
  const double *pair_rec, *blk_data, *pt_data, *inv, *frame_data;
  const int *frame_ptr, *frame_pairs, *off_ptr, *off_pairs, *term_ptr, *fe_ptr, *fe_entries, *sky_i, *sky_j, *block_point;
  const int2* terms;
  const uint8_t* cst;
  double *S, *L, *g;
  int n_frames, n_sky;
  double lambda;
};

// W of an entry (pba_joint_plan.h): block e's W_t, or point ~e's W_h; *p its point
__device__ __forceinline__ const double* entry_w(const AsmArgsJ& a, int e, int* p) {
  if (e < 0) {
    *p = ~e;
    return a.pt_data + (long long)(~e) * kPt + 4;
  }
  *p = a.block_point[e];
  return a.blk_data + (long long)e * kBlk + 2;
}

// One 64-thread workgroup per lower skyline block (i, j), thread = element (r, c): its pairs' direct terms in list
// order, then its Schur terms −W_a W_bᵀ/H′_ρρ in list order; then λ·clamp(diag) on the free diagonal and identity rows
// and columns for the constants.  S keeps the system (pba_joint_get_reduced_system), L is factored in place.
__global__ __launch_bounds__(64) void joint_assemble_kernel(const AsmArgsJ a) {
  const int s = blockIdx.x, t = threadIdx.x, r = t >> 3, c = t & 7;
  const int i = a.sky_i[s], j = a.sky_j[s];
  double v = 0.0;
  if (i == j) {
    for (int q = a.frame_ptr[i]; q < a.frame_ptr[i + 1]; ++q) {
      const int e = a.frame_pairs[q], o = (e & 1) ? 8 : 0;
      v += a.pair_rec[(long long)(e >> 1) * kPairRec + (o + r) * 16 + o + c];
    }
  } else {
    for (int q = a.off_ptr[s]; q < a.off_ptr[s + 1]; ++q) {
      const int e = a.off_pairs[q];
      const double* pr = a.pair_rec + (long long)(e >> 1) * kPairRec;
      v += (e & 1) ? pr[(8 + r) * 16 + c] : pr[r * 16 + 8 + c];  // host = column: H_th; host = row: H_ht
    }
  }
  for (int q = a.term_ptr[s]; q < a.term_ptr[s + 1]; ++q) {
    const int2 tm = a.terms[q];
    int p, p2;
    const double* wa = entry_w(a, tm.x, &p);
    const double* wb = entry_w(a, tm.y, &p2);
    v -= wa[r] * wb[c] * a.inv[p];
  }
  const bool ci = a.cst[2 * i + (r >= 6)] != 0, cj = a.cst[2 * j + (c >= 6)] != 0;
  if (ci || cj) v = i == j && r == c ? 1.0 : 0.0;
  else if (i == j && r == c) v += a.lambda * lm_clamp(a.frame_data[(long long)i * kFrame + 8 + r]);
  a.S[(long long)s * 64 + t] = v;
  a.L[(long long)s * 64 + t] = v;
}

// One thread per keyframe unknown: g_S = g − Σ W·g_ρ/H′_ρρ over the entries on the keyframe, 0 for a constant.
__global__ void joint_gradient_kernel(const AsmArgsJ a) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= 8 * a.n_frames) return;
  const int i = u >> 3, r = u & 7;
  double v = a.frame_data[(long long)i * kFrame + r];
  for (int q = a.fe_ptr[i]; q < a.fe_ptr[i + 1]; ++q) {
    int p;
    const double* w = entry_w(a, a.fe_entries[q], &p);
    v -= w[r] * a.pt_data[(long long)p * kPt + 1] * a.inv[p];
  }
  a.g[u] = a.cst[2 * i + (r >= 6)] ? 0.0 : v;
}

struct AsmArgsI {
  AsmArgsJ a;  // sky_i / sky_j, off_*, term_*, fe_* cover the cameras' rows too (pba_joint_plan.h); a.g the whole gradient
  const double *pair_intr, *cam_data, *blk_wc;
  const uint8_t* cstc;
  int n_blocks, n_cams, n_sky_kf;
  // the two-stage sums: per chunk of Schur terms {skyline block, first term, end, 0} and its 64 partials; per camera's
  // skyline block (CSR) its chunks; per chunk of a camera's entries {first entry, end} and its 8 partials; per camera
  // (CSR) its chunks
  const int4* tchunks;
  const int* tchunk_ptr;
  double* tpart;
  const int2* gchunks;
  const int* gchunk_ptr;
  double* gpart;
};

// entry_w with the third kind of entry: e ≥ n_blocks is block e − n_blocks' camera part W_c
__device__ __forceinline__ const double* entry_w3(const AsmArgsI& x, int e, int* p) {
  if (e >= x.n_blocks) {
    *p = x.a.block_point[e - x.n_blocks];
    return x.blk_wc + (long long)(e - x.n_blocks) * 8;
  }
  return entry_w(x.a, e, p);
}

// One 64-thread workgroup per chunk of a camera block's Schur terms, thread = element (r, c): Σ W_a W_bᵀ/H′_ρρ over
// the chunk's terms in list order.
__global__ __launch_bounds__(64) void joint_intr_terms_kernel(const AsmArgsI x) {
  const AsmArgsJ& a = x.a;
  const int4 ch = x.tchunks[blockIdx.x];
  const int t = threadIdx.x, r = t >> 3, c = t & 7;
  double v = 0.0;
  for (int q = ch.y; q < ch.z; ++q) {
    const int2 tm = a.terms[q];
    int p, p2;
    const double* wa = entry_w3(x, tm.x, &p);
    const double* wb = entry_w3(x, tm.y, &p2);
    v += wa[r] * wb[c] * a.inv[p];
  }
  x.tpart[(long long)blockIdx.x * 64 + t] = v;
}

// One 64-thread workgroup per chunk of a camera's entries: Σ W_c·g_ρ/H′_ρρ — thread t the entries t, t + 64, … of the
// chunk, then thread r < 8 sums row r of the 64 partials in thread order.
__global__ __launch_bounds__(64) void joint_intr_gradient_parts_kernel(const AsmArgsI x) {
  __shared__ double s_p[64][8];
  const AsmArgsJ& a = x.a;
  const int2 ch = x.gchunks[blockIdx.x];
  const int t = threadIdx.x;
  double acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.0;
  for (int q = ch.x + t; q < ch.y; q += 64) {
    int p;
    const double* w = entry_w3(x, a.fe_entries[q], &p);
    const double f = a.pt_data[(long long)p * kPt + 1] * a.inv[p];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] += w[r] * f;
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) s_p[t][r] = acc[r];
  __syncthreads();
  if (t < 8) {
    double sum = 0.0;
    for (int k = 0; k < 64; ++k) sum += s_p[k][t];
    x.gpart[(long long)blockIdx.x * 8 + t] = sum;
  }
}

// joint_assemble_kernel for the cameras' rows: one 64-thread workgroup per skyline block (n_frames + c, j) — the border
// parts of camera c's pairs that touch keyframe j in list order, or the camera's jiᵀwji on the diagonal
// (joint_cam_kernel); then the block's Schur partials (joint_intr_terms_kernel) in chunk order; then the damping and the
// constants (camera c without a valid block, the column's keyframe half or camera).
__global__ __launch_bounds__(64) void joint_intr_assemble_kernel(const AsmArgsI x) {
  const AsmArgsJ& a = x.a;
  const int s = x.n_sky_kf + blockIdx.x, t = threadIdx.x, r = t >> 3, c = t & 7;
  const int i = a.sky_i[s], j = a.sky_j[s], cam = i - a.n_frames;
  double v = 0.0;
  if (j < a.n_frames) {
    for (int q = a.off_ptr[s]; q < a.off_ptr[s + 1]; ++q) {
      const int e = a.off_pairs[q];
      v += x.pair_intr[(long long)(e >> 1) * kPairIntr + r * 16 + ((e & 1) ? 8 : 0) + c];
    }
  } else if (i == j) {
    v = x.cam_data[(long long)cam * kCam + 8 + t];
  }
  for (int q = x.tchunk_ptr[blockIdx.x]; q < x.tchunk_ptr[blockIdx.x + 1]; ++q) v -= x.tpart[(long long)q * 64 + t];
  const bool ci = x.cstc[cam] != 0;
  const bool cj = j < a.n_frames ? a.cst[2 * j + (c >= 6)] != 0 : x.cstc[j - a.n_frames] != 0;
  if (ci || cj) v = i == j && r == c ? 1.0 : 0.0;
  else if (i == j && r == c) v += a.lambda * lm_clamp(x.cam_data[(long long)cam * kCam + 8 + 9 * r]);
  a.S[(long long)s * 64 + t] = v;
  a.L[(long long)s * 64 + t] = v;
}

// One thread per camera unknown: g_S = g − Σ W_c·g_ρ/H′_ρρ, the camera's partials (joint_intr_gradient_parts_kernel) in
// chunk order; 0 for a constant.
__global__ void joint_intr_gradient_kernel(const AsmArgsI x) {
  const AsmArgsJ& a = x.a;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= 8 * x.n_cams) return;
  const int cam = u >> 3, r = u & 7;
  double v = x.cam_data[(long long)cam * kCam + r];
  for (int q = x.gchunk_ptr[cam]; q < x.gchunk_ptr[cam + 1]; ++q) v -= x.gpart[(long long)q * 8 + r];
  a.g[8 * a.n_frames + u] = x.cstc[cam] ? 0.0 : v;
}

// ---- the reduced solve: S δ = −g, S = LLᵀ in place (8×8-block skyline, right-looking), one workgroup ----------------
__device__ __forceinline__ bool chol8_reg(const double (&A)[64], double (&L)[64]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 64; ++i) L[i] = 0.0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double s = A[j * 8 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * 8 + k] * L[j * 8 + k];
    ok = ok && s > 0.0 && isfinite(s);
    const double ljj = sqrt(fmax(s, 1e-300));
    L[j * 8 + j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 8; ++i) {
      double t = A[i * 8 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i * 8 + k] * L[j * 8 + k];
      L[i * 8 + j] = t / ljj;
    }
  }
  return ok;
}
__device__ __forceinline__ void inv_lower8_reg(const double (&L)[64], double (&Li)[64]) {
#pragma unroll
  for (int i = 0; i < 64; ++i) Li[i] = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    Li[c * 8 + c] = 1.0 / L[c * 8 + c];
#pragma unroll
    for (int r = c + 1; r < 8; ++r) {
      double s = 0.0;
#pragma unroll
      for (int k = c; k < r; ++k) s += L[r * 8 + k] * Li[k * 8 + c];
      Li[r * 8 + c] = -s / L[r * 8 + r];
    }
  }
}

struct SolveArgsJ {
  double* S;  // the damped system, factored in place
  const int *first, *row;
  const double* g;
  double *Linv, *x;
  int* status;
  int N;
  const int *cptr, *crows;  // column k's profile rows crows[cptr[k] … cptr[k+1]) (every i > k with first(i) ≤ k, in order)
};

__device__ __forceinline__ long long sky8(const SolveArgsJ& a, int i, int j) {  // block (i, j), j ≥ first(i)
  return ((long long)a.row[i] + (j - a.first[i])) * 64;
}

// skyline_solve_kernel with 8×8 blocks: per column k the diagonal block's factor and inverse (one thread, registers), the
// column panel L_ik = A_ik·L_kk⁻ᵀ four blocks per pass, then the trailing update A_ij −= L_ik L_jkᵀ over the pairs of the
// column's rows — every element by one thread, the columns in order: a fixed order.  status = k + 1 when column k's
// pivot is not positive (or not finite).
__global__ __launch_bounds__(256) void joint_solve_kernel(const SolveArgsJ a) {
  __shared__ double sA[64], sL[64], sLi[64];
  __shared__ int s_fail;
  const int tid = threadIdx.x;
  if (tid == 0) s_fail = 0;
  for (int k = 0; k < a.N; ++k) {
    const long long okk = sky8(a, k, k);
    if (tid < 64) sA[tid] = a.S[okk + tid];
    __syncthreads();
    if (tid == 0) {
      double A[64], L[64], Li[64];
#pragma unroll
      for (int q = 0; q < 64; ++q) A[q] = sA[q];
      if (!chol8_reg(A, L)) {
        s_fail = k + 1;
      } else {
        inv_lower8_reg(L, Li);
#pragma unroll
        for (int q = 0; q < 64; ++q) {
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
    if (tid < 64) {
      a.S[okk + tid] = sL[tid];
      a.Linv[(long long)k * 64 + tid] = sLi[tid];
    }
    const int c0 = a.cptr[k], na = a.cptr[k + 1] - c0;
    const int* rows = a.crows + c0;
    for (int i0 = 0; i0 < na; i0 += 4) {  // (read all, barrier, write)
      double val = 0.0;
      long long dst = -1;
      const int li = i0 + tid / 64;
      if (li < na) {
        const int i = rows[li], e = tid % 64, r = e / 8, c = e % 8;
        const long long o = sky8(a, i, k);
        for (int m = 0; m <= c; ++m) val += a.S[o + r * 8 + m] * sLi[c * 8 + m];
        dst = o + e;
      }
      __syncthreads();
      if (dst >= 0) a.S[dst] = val;
      __threadfence_block();
      __syncthreads();
    }
    const int npairs = na * (na + 1) / 2;
    for (int idx = tid; idx < npairs * 64; idx += 256) {
      const int pidx = idx / 64, e = idx % 64, r = e / 8, c = e % 8;
      int ii = 0;  // lower-triangular pair index → (ii ≥ jj)
      while ((ii + 1) * (ii + 2) / 2 <= pidx) ++ii;
      const int jj = pidx - ii * (ii + 1) / 2;
      const int i = rows[ii], j = rows[jj];
      const long long oi = sky8(a, i, k), oj = sky8(a, j, k);
      double s = 0.0;
      for (int m = 0; m < 8; ++m) s += a.S[oi + r * 8 + m] * a.S[oj + c * 8 + m];
      a.S[sky8(a, i, j) + e] -= s;
    }
    __threadfence_block();
    __syncthreads();
  }
  // forward substitution L y = −g (y in x)
  for (int t = tid; t < 8 * a.N; t += 256) a.x[t] = -a.g[t];
  __threadfence_block();
  __syncthreads();
  for (int k = 0; k < a.N; ++k) {
    __shared__ double yk[8];
    if (tid < 8) {
      double s = 0.0;
      for (int m = 0; m <= tid; ++m) s += a.Linv[(long long)k * 64 + tid * 8 + m] * a.x[8 * k + m];
      yk[tid] = s;
    }
    __syncthreads();
    if (tid < 8) a.x[8 * k + tid] = yk[tid];
    const int c0 = a.cptr[k], na = a.cptr[k + 1] - c0;
    for (int idx = tid; idx < na * 8; idx += 256) {
      const int i = a.crows[c0 + idx / 8], r = idx % 8;
      const long long o = sky8(a, i, k);
      double s = 0.0;
      for (int m = 0; m < 8; ++m) s += a.S[o + r * 8 + m] * yk[m];
      a.x[8 * i + r] -= s;
    }
    __threadfence_block();
    __syncthreads();
  }
  // back substitution Lᵀ x = y
  for (int k = a.N - 1; k >= 0; --k) {
    __shared__ double tk[8];
    if (tid < 8) {
      double s = a.x[8 * k + tid];
      for (int q = a.cptr[k]; q < a.cptr[k + 1]; ++q) {
        const int i = a.crows[q];
        const long long o = sky8(a, i, k);
        for (int m = 0; m < 8; ++m) s -= a.S[o + m * 8 + tid] * a.x[8 * i + m];
      }
      tk[tid] = s;
    }
    __syncthreads();
    if (tid < 8) {
      double s = 0.0;
      for (int m = tid; m < 8; ++m) s += a.Linv[(long long)k * 64 + m * 8 + tid] * tk[m];
      a.x[8 * k + tid] = s;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (tid == 0) *a.status = 0;
}

struct UpdArgs {
  const double *x, *pt_data, *blk_data, *inv, *frame_data, *poses, *rho, *ab;
  const int *pt_ptr, *pt_blocks, *point_host, *status;
  const int4* block_rec;
  const uint8_t* cst;
  double *drho, *poses_new, *rho_new, *ab_new, *red3;
  int n_points, n_frames;
  double lambda;
};

// Threads [0, n_points): δρ = −(g_ρ + Wᵀδ_kf)/H′_ρρ and ρ + δρ.  Threads [n_points, n_points + n_frames): T·exp(δpose),
// (a, b) + (δa, δb), constants copied.  Per workgroup the parts of 2·model decrease = λ δᵀDδ − gᵀδ, ‖step‖² and
// ‖candidate‖² in the ambient space of the free unknowns (free poses as [q | t], ρ of points with blocks, free (a, b)).
// (A constant's step is exactly zero out of the solve: identity rows, zero right-hand side.)
__global__ __launch_bounds__(256) void joint_update_kernel(const UpdArgs a) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (*a.status == 0) {
    if (u < a.n_points) {
      const double* pd = a.pt_data + (long long)u * kPt;
      const double inv = a.inv[u];
      const int q0 = a.pt_ptr[u], q1 = a.pt_ptr[u + 1];
      double d = 0.0;
      if (inv > 0.0) {
        double acc = pd[1];
        const double* xh = a.x + 8 * a.point_host[u];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc += pd[4 + r] * xh[r];
        for (int q = q0; q < q1; ++q) {
          const int b = a.pt_blocks[q];
          const double* w = a.blk_data + (long long)b * kBlk + 2;
          const double* xt = a.x + 8 * a.block_rec[b].z;
#pragma unroll
          for (int r = 0; r < 8; ++r) acc += w[r] * xt[r];
        }
        d = -acc * inv;
        v[0] = a.lambda * lm_clamp(pd[0]) * d * d - pd[1] * d;
      }
      const double rn = a.rho[u] + d;
      a.drho[u] = d;
      a.rho_new[u] = rn;
      if (q1 > q0) {
        v[1] = d * d;
        v[2] = rn * rn;
      }
    } else if (u < a.n_points + a.n_frames) {
      const int i = u - a.n_points;
      const double* fd = a.frame_data + (long long)i * kFrame;
      const bool cp = a.cst[2 * i] != 0, ca = a.cst[2 * i + 1] != 0;
      double d[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        d[r] = (r < 6 ? cp : ca) ? 0.0 : a.x[8 * i + r];
        if (!(r < 6 ? cp : ca)) v[0] += a.lambda * lm_clamp(fd[8 + r]) * d[r] * d[r] - fd[r] * d[r];
      }
      double T[7], Tn[7];
#pragma unroll
      for (int r = 0; r < 7; ++r) T[r] = Tn[r] = a.poses[7 * i + r];
      if (!cp) {
        se3_exp_mul(T, d, Tn);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
          v[1] += (Tn[r] - T[r]) * (Tn[r] - T[r]);
          v[2] += Tn[r] * Tn[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 7; ++r) a.poses_new[7 * i + r] = Tn[r];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double o = a.ab[2 * i + r], n = ca ? o : o + d[6 + r];
        a.ab_new[2 * i + r] = n;
        if (!ca) {
          v[1] += d[6 + r] * d[6 + r];
          v[2] += n * n;
        }
      }
    }
  }
  double* const r = a.red3 + 4 * blockIdx.x;
  double* const slot[3] = {r, r + 1, r + 2};
  wg_reduce_sum_max<3>(v, 0.0, slot, r + 3);
}

struct UpdArgsI {
  UpdArgs u;  // x holds the keyframes' steps, then the cameras'
  const double *blk_wc, *cam_data, *kcur;  // kcur: the intrinsics state's camera records at the active level
  const uint8_t* cstc;
  double* knew_d;  // the candidate's camera records at the active level …
  float* knew_f;   // … and its projection constants (8 floats per camera): launch_cost_only's two buffers
  int n_cams;
  double kscale;   // 2^−level: entries 0–3 of the level's image move by 2^−level·δk, the distortion by δk
};

// joint_update_kernel with free intrinsics: δρ's sum runs over the point's camera entries too (after its blocks'
// target parts, the entry order), and threads [n_points + n_frames, n_points + n_frames + n_cams) form the candidate
// intrinsics k + δk as the level's camera record [k(8) | cx cy 1/fx 1/fy p1…p4] (upload_cameras' layout) and its fp32
// copy.  The cameras' parts of the three sums go into the same slots: the model decrease over the 8 unknowns of a camera
// with a valid block, and ‖δk‖², ‖k + δk‖² of the level-0 state.
__global__ __launch_bounds__(256) void joint_intr_update_kernel(const UpdArgsI x) {
  const UpdArgs& a = x.u;
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};
  if (*a.status == 0) {
    if (u < a.n_points) {
      const double* pd = a.pt_data + (long long)u * kPt;
      const double inv = a.inv[u];
      const int q0 = a.pt_ptr[u], q1 = a.pt_ptr[u + 1];
      double d = 0.0;
      if (inv > 0.0) {
        double acc = pd[1];
        const double* xh = a.x + 8 * a.point_host[u];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc += pd[4 + r] * xh[r];
        for (int q = q0; q < q1; ++q) {
          const int b = a.pt_blocks[q];
          const double* w = a.blk_data + (long long)b * kBlk + 2;
          const double* xt = a.x + 8 * a.block_rec[b].z;
#pragma unroll
          for (int r = 0; r < 8; ++r) acc += w[r] * xt[r];
        }
        for (int q = q0; q < q1; ++q) {
          const int b = a.pt_blocks[q];
          const double* w = x.blk_wc + (long long)b * 8;
          const double* xc = a.x + 8 * (a.n_frames + (a.block_rec[b].w & 0xffff));
#pragma unroll
          for (int r = 0; r < 8; ++r) acc += w[r] * xc[r];
        }
        d = -acc * inv;
        v[0] = a.lambda * lm_clamp(pd[0]) * d * d - pd[1] * d;
      }
      const double rn = a.rho[u] + d;
      a.drho[u] = d;
      a.rho_new[u] = rn;
      if (q1 > q0) {
        v[1] = d * d;
        v[2] = rn * rn;
      }
    } else if (u < a.n_points + a.n_frames) {
      const int i = u - a.n_points;
      const double* fd = a.frame_data + (long long)i * kFrame;
      const bool cp = a.cst[2 * i] != 0, ca = a.cst[2 * i + 1] != 0;
      double d[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        d[r] = (r < 6 ? cp : ca) ? 0.0 : a.x[8 * i + r];
        if (!(r < 6 ? cp : ca)) v[0] += a.lambda * lm_clamp(fd[8 + r]) * d[r] * d[r] - fd[r] * d[r];
      }
      double T[7], Tn[7];
#pragma unroll
      for (int r = 0; r < 7; ++r) T[r] = Tn[r] = a.poses[7 * i + r];
      if (!cp) {
        se3_exp_mul(T, d, Tn);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
          v[1] += (Tn[r] - T[r]) * (Tn[r] - T[r]);
          v[2] += Tn[r] * Tn[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 7; ++r) a.poses_new[7 * i + r] = Tn[r];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double o = a.ab[2 * i + r], n = ca ? o : o + d[6 + r];
        a.ab_new[2 * i + r] = n;
        if (!ca) {
          v[1] += d[6 + r] * d[6 + r];
          v[2] += n * n;
        }
      }
    } else if (u < a.n_points + a.n_frames + x.n_cams) {
      const int c = u - a.n_points - a.n_frames;
      const double* cd = x.cam_data + (long long)c * kCam;
      const bool cc = x.cstc[c] != 0;
      double kn[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double d = cc ? 0.0 : a.x[8 * (a.n_frames + c) + r];
        const double k = x.kcur[kCamD * c + r];
        kn[r] = cc ? k : k + (r < 4 ? x.kscale * d : d);
        if (!cc) {
          // the level-0 state's entry (upload_intrinsics_state's map inverted; the level's own at level 0)
          const double k0 = x.kscale == 1.0 || r >= 4 ? k : r < 2 ? k / x.kscale : (k + 0.5) / x.kscale - 0.5;
          v[0] += a.lambda * lm_clamp(cd[8 + 9 * r]) * d * d - cd[r] * d;
          v[1] += d * d;
          v[2] += (k0 + d) * (k0 + d);
        }
      }
      double* od = x.knew_d + (long long)kCamD * c;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        od[r] = kn[r];
        x.knew_f[8 * c + r] = (float)kn[r];
      }
      od[8] = kn[2];
      od[9] = kn[3];
      od[10] = 1.0 / kn[0];
      od[11] = 1.0 / kn[1];
#pragma unroll
      for (int r = 4; r < 8; ++r) od[8 + r] = kn[r];
    }
  }
  double* const r = a.red3 + 4 * blockIdx.x;
  double* const slot[3] = {r, r + 1, r + 2};
  wg_reduce_sum_max<3>(v, 0.0, slot, r + 3);
}

// ---- the multi-GPU exchange (pba.h pba_joint_step_export / import; the layout: pba_joint_plan.h) ---------------------
struct ExArgsJ {
  AsmArgsJ a;      // the sources; its cst, S, L, g and lambda are not read
  const int* src;  // per (keyframe, band column): the local skyline block, −1 none
  double* X;
  int K;
  long long stride;
};

// This rank's undamped reduced system into the exchange buffer.  Workgroups [0, n_frames·(K + 1)): one per (keyframe,
// band column) block, thread = element — joint_assemble_kernel's sums in its order (the direct pair terms, then the Schur
// terms), without its damping and constants, which are decided after the sum over the ranks; zeros where the rank has
// no block.  The next n_frames workgroups: the keyframe's tail — joint_gradient_kernel's sum without its constant mask,
// the direct gradient and diagonal of frame_data, and the valid blocks of the keyframe's pairs in list order.  The last
// workgroup clears the scalar slots, so every double of the buffer is written.
__global__ __launch_bounds__(64) void joint_export_kernel(const ExArgsJ x) {
  const AsmArgsJ& a = x.a;
  const int w = blockIdx.x, t = threadIdx.x, nb = a.n_frames * (x.K + 1);
  if (w < nb) {
    const int i = w / (x.K + 1), cb = w % (x.K + 1), s = x.src[w], r = t >> 3, c = t & 7;
    double v = 0.0;
    if (s >= 0) {
      if (cb == x.K) {
        for (int q = a.frame_ptr[i]; q < a.frame_ptr[i + 1]; ++q) {
          const int e = a.frame_pairs[q], o = (e & 1) ? 8 : 0;
          v += a.pair_rec[(long long)(e >> 1) * kPairRec + (o + r) * 16 + o + c];
        }
      } else {
        for (int q = a.off_ptr[s]; q < a.off_ptr[s + 1]; ++q) {
          const int e = a.off_pairs[q];
          const double* pr = a.pair_rec + (long long)(e >> 1) * kPairRec;
          v += (e & 1) ? pr[(8 + r) * 16 + c] : pr[r * 16 + 8 + c];
        }
      }
      for (int q = a.term_ptr[s]; q < a.term_ptr[s + 1]; ++q) {
        const int2 tm = a.terms[q];
        int p, p2;
        const double* wa = entry_w(a, tm.x, &p);
        const double* wb = entry_w(a, tm.y, &p2);
        v -= wa[r] * wb[c] * a.inv[p];
      }
    }
    x.X[(long long)i * x.stride + cb * 64 + t] = v;
  } else if (w < nb + a.n_frames) {
    if (t >= kJointExTail) return;
    const int i = w - nb;
    double v = 0.0;
    if (t < 8) {
      v = a.frame_data[(long long)i * kFrame + t];
      for (int q = a.fe_ptr[i]; q < a.fe_ptr[i + 1]; ++q) {
        int p;
        const double* wv = entry_w(a, a.fe_entries[q], &p);
        v -= wv[t] * a.pt_data[(long long)p * kPt + 1] * a.inv[p];
      }
    } else if (t < 24) {
      v = a.frame_data[(long long)i * kFrame + t - 8];
    } else if (t == 24) {
      for (int q = a.frame_ptr[i]; q < a.frame_ptr[i + 1]; ++q)
        v += a.pair_rec[(long long)(a.frame_pairs[q] >> 1) * kPairRec + 272];
    }
    x.X[(long long)i * x.stride + (long long)(x.K + 1) * 64 + t] = v;
  } else if (t < kJointExScalars) {
    x.X[(long long)a.n_frames * x.stride + t] = 0.0;
  }
}

struct ImpArgsJ {
  const double* X;  // the sum over the ranks
  const uint8_t* fixed;
  const double *poses, *ab;
  const int *sky_i, *sky_j;
  double *S, *L, *g, *frame_data, *gmax_f;
  uint8_t* cst;
  int K;
  long long stride;
  double lambda;
};

// joint_frame_kernel's constants from the summed count of valid blocks: half 0 the pose, 1 the (a, b)
__device__ __forceinline__ bool import_constant(const ImpArgsJ& a, int i, int half) {
  const bool seen = a.X[(long long)i * a.stride + (long long)(a.K + 1) * 64 + 24] > 0.0;
  if (half == 0) return a.fixed[2 * i] != 0 || !seen;
  return a.fixed[2 * i + 1] != 0 || !seen || !isfinite(a.ab[2 * i]) || !isfinite(a.ab[2 * i + 1]);
}

// The summed band into factor storage over the band profile: one 64-thread workgroup per block (i, j), thread =
// element, with joint_assemble_kernel's damping and constants from the summed diagonal and the summed counts.  The
// diagonal workgroups also write their keyframe's g_S (0 for a constant), the summed direct gradient and diagonal in
// frame_data's layout, the constant mask the update reads, and joint_frame_kernel's gradient norm from the summed
// direct gradient.  Every rank runs this on the same buffer: the same system bit for bit.
__global__ __launch_bounds__(64) void joint_import_kernel(const ImpArgsJ a) {
  const int s = blockIdx.x, t = threadIdx.x, r = t >> 3, c = t & 7;
  const int i = a.sky_i[s], j = a.sky_j[s];
  const double* tail = a.X + (long long)i * a.stride + (long long)(a.K + 1) * 64;
  double v = a.X[(long long)i * a.stride + (long long)(j - (i - a.K)) * 64 + t];
  const bool ci = import_constant(a, i, r >= 6), cj = import_constant(a, j, c >= 6);
  if (ci || cj) v = i == j && r == c ? 1.0 : 0.0;
  else if (i == j && r == c) v += a.lambda * lm_clamp(tail[16 + r]);
  a.S[(long long)s * 64 + t] = v;
  a.L[(long long)s * 64 + t] = v;
  if (i != j) return;
  if (t < 8) {
    a.g[8 * i + t] = import_constant(a, i, t >= 6) ? 0.0 : tail[t];
  } else if (t < 24) {
    a.frame_data[(long long)i * kFrame + t - 8] = tail[t];
  } else if (t < 26) {
    a.cst[2 * i + t - 24] = import_constant(a, i, t - 24) ? 1 : 0;
  } else if (t == 26) {
    double gm = 0.0;
    if (!import_constant(a, i, 0)) {
      double ng[6], tg[7];
#pragma unroll
      for (int q = 0; q < 6; ++q) ng[q] = -tail[8 + q];
      se3_exp_mul(a.poses + 7 * i, ng, tg);
#pragma unroll
      for (int q = 0; q < 7; ++q) gm = fmax(gm, fabs(a.poses[7 * i + q] - tg[q]));
    }
    if (!import_constant(a, i, 1)) gm = fmax(gm, fmax(fabs(tail[14]), fabs(tail[15])));
    a.gmax_f[i] = gm;
  }
}

// joint_update_kernel for a step from the summed system, with the keyframe and the point parts of its three sums in
// separate slots (0…2 the points', 3…5 the keyframes'): the point parts differ from rank to rank and are summed over the
// ranks, the keyframe parts are every rank's own copy of one number.  The keyframes come first, threads [0, n_frames),
// so that their partition into workgroups, and with it the order of their sums, is the same on every rank; the points
// follow, threads [n_frames, n_frames + n_points).
__global__ __launch_bounds__(256) void joint_update_parts_kernel(const UpdArgs a) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (*a.status == 0) {
    if (u < a.n_frames) {
      const int i = u;
      const double* fd = a.frame_data + (long long)i * kFrame;
      const bool cp = a.cst[2 * i] != 0, ca = a.cst[2 * i + 1] != 0;
      double d[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        d[r] = (r < 6 ? cp : ca) ? 0.0 : a.x[8 * i + r];
        if (!(r < 6 ? cp : ca)) v[3] += a.lambda * lm_clamp(fd[8 + r]) * d[r] * d[r] - fd[r] * d[r];
      }
      double T[7], Tn[7];
#pragma unroll
      for (int r = 0; r < 7; ++r) T[r] = Tn[r] = a.poses[7 * i + r];
      if (!cp) {
        se3_exp_mul(T, d, Tn);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
          v[4] += (Tn[r] - T[r]) * (Tn[r] - T[r]);
          v[5] += Tn[r] * Tn[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 7; ++r) a.poses_new[7 * i + r] = Tn[r];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double o = a.ab[2 * i + r], n = ca ? o : o + d[6 + r];
        a.ab_new[2 * i + r] = n;
        if (!ca) {
          v[4] += d[6 + r] * d[6 + r];
          v[5] += n * n;
        }
      }
    } else if (u < a.n_frames + a.n_points) {
      const int p = u - a.n_frames;
      const double* pd = a.pt_data + (long long)p * kPt;
      const double inv = a.inv[p];
      const int q0 = a.pt_ptr[p], q1 = a.pt_ptr[p + 1];
      double d = 0.0;
      if (inv > 0.0) {
        double acc = pd[1];
        const double* xh = a.x + 8 * a.point_host[p];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc += pd[4 + r] * xh[r];
        for (int q = q0; q < q1; ++q) {
          const int b = a.pt_blocks[q];
          const double* w = a.blk_data + (long long)b * kBlk + 2;
          const double* xt = a.x + 8 * a.block_rec[b].z;
#pragma unroll
          for (int r = 0; r < 8; ++r) acc += w[r] * xt[r];
        }
        d = -acc * inv;
        v[0] = a.lambda * lm_clamp(pd[0]) * d * d - pd[1] * d;
      }
      const double rn = a.rho[p] + d;
      a.drho[p] = d;
      a.rho_new[p] = rn;
      if (q1 > q0) {
        v[1] = d * d;
        v[2] = rn * rn;
      }
    }
  }
  double* const r = a.red3 + 8 * blockIdx.x;
  double* const slot[6] = {r, r + 1, r + 2, r + 3, r + 4, r + 5};
  wg_reduce_sum_max<6>(v, 0.0, slot, r + 6);
}

// intr_ok: the entry point runs with free intrinsics under pba_joint_set_solve_intrinsics (the single-GPU ones); the
// multi-GPU exchange refuses them either way.
int ready(pba_engine* e, bool intr_ok = false) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC || !e->affine)
    return fail(PBA_ERR_INVALID_ARGUMENT, "the joint solve needs a photometric engine with pba_set_affine_brightness");
  if (e->opt_intr && !(intr_ok && e->joint_solve_intr))
    return fail(PBA_ERR_INVALID_ARGUMENT,
                intr_ok ? "the joint solve frees the intrinsics of pba_set_optimize_intrinsics only with pba_joint_set_solve_intrinsics"
                        : "the multi-GPU joint solve does not combine with pba_set_optimize_intrinsics");
  if (e->n_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  if (!e->state_set) return fail(PBA_ERR_NOT_READY, "pba_set_state first");
  if (!e->have_images || e->P <= 0) return fail(PBA_ERR_NOT_READY, "images/pattern missing");
  if (int rc = check_device(e)) return rc;
  JointSolve& J = e->joint;
  const int nc = e->opt_intr ? e->n_cams : 0;  // cameras among the unknowns
  if (J.planned && J.nc != nc) J.planned = false;
  if (!J.planned) {
    JointPlanInput in;
    in.n_cams = nc;
    in.frame_cam = e->frame_cam_h.data();
    in.n_frames = e->n_frames;
    in.n_pairs = e->n_pairs;
    in.n_points = e->n_points;
    in.n_blocks = e->n_blocks;
    in.pair_host = e->pair_host_h.data();
    in.pair_target = e->pair_target_h.data();
    in.block_pair = e->pair_of_h.data();
    in.block_point = e->block_point_h.data();
    in.point_host = e->point_host_h.data();
    JointPlan P;
    if (!build_joint_plan(in, P)) return fail(PBA_ERR_INVALID_ARGUMENT, "inconsistent pairs (or a block whose target is its host)");
    const int nf = e->n_frames, N = nf + nc;
    std::vector<int> si(P.n_sky), sj(P.n_sky);
    for (int i = 0; i < N; ++i)
      for (int j = P.first[i]; j <= i; ++j) {
        si[P.row[i] + (j - P.first[i])] = i;
        sj[P.row[i] + (j - P.first[i])] = j;
      }
    std::vector<int2> terms(P.terms.size());
    for (size_t q = 0; q < terms.size(); ++q) terms[q] = make_int2(P.terms[q].a, P.terms[q].b);
    PBA_HIP(J.pair_ptr.upload(P.pair_ptr, e->stream));
    PBA_HIP(J.pair_blocks.upload(P.pair_blocks, e->stream));
    PBA_HIP(J.frame_ptr.upload(P.frame_ptr, e->stream));
    PBA_HIP(J.frame_pairs.upload(P.frame_pairs, e->stream));
    PBA_HIP(J.pt_ptr.upload(P.pt_ptr, e->stream));
    PBA_HIP(J.pt_blocks.upload(P.pt_blocks, e->stream));
    PBA_HIP(J.first.upload(P.first, e->stream));
    PBA_HIP(J.row.upload(P.row, e->stream));
    PBA_HIP(J.colptr.upload(P.colptr, e->stream));
    PBA_HIP(J.colrows.upload(P.colrows, e->stream));
    PBA_HIP(J.off_ptr.upload(P.off_ptr, e->stream));
    PBA_HIP(J.off_pairs.upload(P.off_pairs, e->stream));
    PBA_HIP(J.term_ptr.upload(P.term_ptr, e->stream));
    PBA_HIP(J.terms.upload(terms, e->stream));
    PBA_HIP(J.fe_ptr.upload(P.fe_ptr, e->stream));
    PBA_HIP(J.fe_entries.upload(P.fe_entries, e->stream));
    PBA_HIP(J.sky_i.upload(si, e->stream));
    PBA_HIP(J.sky_j.upload(sj, e->stream));
    if (nc > 0) {
      PBA_HIP(J.cam_ptr.upload(P.cam_ptr, e->stream));
      PBA_HIP(J.cam_pairs.upload(P.cam_pairs, e->stream));
      // the chunks of the cameras' two-stage sums: of each camera block's Schur terms, of each camera's entries
      std::vector<int4> tch;
      std::vector<int2> gch;
      std::vector<int> tptr(1, 0), gptr(1, 0);
      for (int s = P.n_sky_kf; s < P.n_sky; ++s) {
        for (int q = P.term_ptr[s]; q < P.term_ptr[s + 1]; q += kTermChunk)
          tch.push_back(make_int4(s, q, std::min(q + kTermChunk, P.term_ptr[s + 1]), 0));
        tptr.push_back((int)tch.size());
      }
      for (int c = 0; c < nc; ++c) {
        for (int q = P.fe_ptr[nf + c]; q < P.fe_ptr[nf + c + 1]; q += kEntryChunk)
          gch.push_back(make_int2(q, std::min(q + kEntryChunk, P.fe_ptr[nf + c + 1])));
        gptr.push_back((int)gch.size());
      }
      J.n_tchunks = (int)tch.size();
      J.n_gchunks = (int)gch.size();
      PBA_HIP(J.tchunks.upload(tch, e->stream));
      PBA_HIP(J.gchunks.upload(gch, e->stream));
      PBA_HIP(J.tchunk_ptr.upload(tptr, e->stream));
      PBA_HIP(J.gchunk_ptr.upload(gptr, e->stream));
      PBA_HIP(J.tpart.resize(64 * (size_t)std::max(J.n_tchunks, 1)));
      PBA_HIP(J.gpart.resize(8 * (size_t)std::max(J.n_gchunks, 1)));
    }
    PBA_HIP(hipStreamSynchronize(e->stream));  // (the plan's vectors die with this scope)
    J.n_sky = P.n_sky;
    J.n_sky_kf = P.n_sky_kf;
    J.nc = nc;
    J.first_h = P.first;
    J.row_h = P.row;
    const size_t nb = e->n_blocks, npt = e->n_points, np = std::max(e->n_pairs, 1);
    J.lin_slots = (int)((nb * 8 + kBlockThreads - 1) / kBlockThreads);
    J.pt_slots = (int)((npt + 255) / 256);
    J.upd_slots = (int)((npt + N + 255) / 256);
    PBA_HIP(J.rec.resize(nb * kRec));
    PBA_HIP(J.pair_rec.resize(np * kPairRec));
    PBA_HIP(J.pair_ad.resize(np * kPairAd));
    PBA_HIP(J.blk_data.resize(nb * kBlk));
    PBA_HIP(J.pt_data.resize(npt * kPt));
    PBA_HIP(J.inv.resize(npt));
    PBA_HIP(J.frame_data.resize((size_t)nf * kFrame));
    PBA_HIP(J.gmax_f.resize(nf));
    PBA_HIP(J.gmax_p.resize(2 * (size_t)std::max(J.pt_slots, 1)));
    PBA_HIP(J.cst.resize(2 * (size_t)nf));
    PBA_HIP(J.S.resize(64 * (size_t)J.n_sky));
    PBA_HIP(J.L.resize(64 * (size_t)J.n_sky));
    PBA_HIP(J.Linv.resize(64 * (size_t)N));
    PBA_HIP(J.g.resize(8 * (size_t)N));
    PBA_HIP(J.x.resize(8 * (size_t)N));
    PBA_HIP(J.drho.resize(npt));
    PBA_HIP(J.poses_new.resize(7 * (size_t)nf));
    PBA_HIP(J.rho_new.resize(npt));
    PBA_HIP(J.ab_new.resize(2 * (size_t)nf));
    PBA_HIP(J.red.resize(2 * (nb / 16 + 2)));
    PBA_HIP(J.red3.resize(4 * (size_t)J.upd_slots));
    PBA_HIP(J.status.resize(1));
    if (nc > 0) {
      PBA_HIP(J.irec.resize(nb * kIntrRec));
      PBA_HIP(J.pair_intr.resize(np * kPairIntr));
      PBA_HIP(J.blk_wc.resize(nb * 8));
      PBA_HIP(J.cam_data.resize((size_t)nc * kCam));
      PBA_HIP(J.gmax_c.resize(nc));
      PBA_HIP(J.cstc.resize(nc));
      PBA_HIP(J.intr_new_d.resize((size_t)nc * kCamD));
      PBA_HIP(J.intr_new_f.resize((size_t)nc * 8));
    }
    J.planned = true;
    J.linearized = J.have_step = false;
    J.ex_K = -1;  // (the exchange plan is the profile's)
  }
  return PBA_OK;
}

int linearize_j(pba_engine* e, double* cost) {
  JointSolve& J = e->joint;
  const int nf = e->n_frames;
  std::vector<uint8_t> f(2 * (size_t)nf, 0);  // the requested constants: a few bytes per keyframe, before every linearisation
  for (int i = 0; i < nf; ++i) {
    f[2 * i] = i < (int)e->gn.fixed_h.size() && e->gn.fixed_h[i];
    f[2 * i + 1] = i < (int)e->aff.fixed_h.size() && e->aff.fixed_h[i];
  }
  PBA_HIP(J.fixed.upload(f, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  KernelArgs ka = make_kernel_args(e, e->pairs.p, e->rho.p);
  ka.poses = e->poses.p;  // the fused-state prologue, as the public evaluations
  ka.wg_red = J.red.p;
  const int grid = J.lin_slots;
  dispatch_pm(e, [&](auto pm) {
    if (J.nc > 0)  // (ka's target intrinsics are the state's: make_kernel_args)
      joint_intr_moments_kernel<decltype(pm)::value><<<grid, kBlockThreads, 0, e->stream>>>(ka, J.rec.p, J.irec.p, (e->P + 7) / 8);
    else
      joint_moments_kernel<decltype(pm)::value><<<grid, kBlockThreads, 0, e->stream>>>(ka, J.rec.p, (e->P + 7) / 8);
  });
  PBA_HIP(hipGetLastError());
  if (e->n_pairs > 0)
    joint_pair_kernel<<<e->n_pairs, 64, 0, e->stream>>>(J.rec.p, J.pair_ptr.p, J.pair_blocks.p, e->pair_host.p,
                                                        e->pair_target.p, e->poses.p, J.pair_rec.p, J.pair_ad.p);
  joint_block_kernel<<<(e->n_blocks + 255) / 256, 256, 0, e->stream>>>(J.rec.p, e->block_pair.p, J.pair_ad.p, e->n_blocks,
                                                                      J.blk_data.p);
  if (J.pt_slots > 0)
    joint_point_kernel<<<J.pt_slots, 256, 0, e->stream>>>(J.blk_data.p, J.pt_ptr.p, J.pt_blocks.p, e->n_points, J.pt_data.p,
                                                          J.gmax_p.p);
  joint_frame_kernel<<<(nf + 255) / 256, 256, 0, e->stream>>>(J.pair_rec.p, J.frame_ptr.p, J.frame_pairs.p, J.fixed.p,
                                                             e->poses.p, e->affine_state.p, nf, J.frame_data.p, J.cst.p,
                                                             J.gmax_f.p);
  if (J.nc > 0) {
    if (e->n_pairs > 0)
      joint_intr_pair_kernel<<<e->n_pairs, 128, 0, e->stream>>>(J.irec.p, J.pair_ptr.p, J.pair_blocks.p, J.pair_ad.p,
                                                                J.pair_intr.p);
    joint_intr_block_kernel<<<(e->n_blocks + 255) / 256, 256, 0, e->stream>>>(J.irec.p, e->n_blocks, J.blk_wc.p);
    joint_cam_kernel<<<J.nc, 64, 0, e->stream>>>(J.pair_intr.p, J.pair_rec.p, J.cam_ptr.p, J.cam_pairs.p, J.cam_data.p,
                                                 J.cstc.p, J.gmax_c.p);
  }
  PBA_HIP(hipGetLastError());
  J.linearized = true;
  J.have_step = false;
  ++J.lin_id;  // (an export stands for one linearisation)
  double c = 0.0;
  if (int rc = sum_red(e, J.red.p, grid, &c, &J.n_valid)) return rc;
  if (cost) *cost = c;
  return PBA_OK;
}

// the gradient max norm of the linearisation (free poses, points with blocks, free (a, b))
int gradient_norm(pba_engine* e, double* gmax) {
  JointSolve& J = e->joint;
  std::vector<double> f(e->n_frames), p(2 * (size_t)std::max(J.pt_slots, 1), 0.0);
  PBA_HIP(hipMemcpyAsync(f.data(), J.gmax_f.p, sizeof(double) * f.size(), hipMemcpyDeviceToHost, e->stream));
  if (J.pt_slots > 0)
    PBA_HIP(hipMemcpyAsync(p.data(), J.gmax_p.p, sizeof(double) * 2 * (size_t)J.pt_slots, hipMemcpyDeviceToHost, e->stream));
  std::vector<double> c(J.nc);
  if (J.nc > 0) PBA_HIP(hipMemcpyAsync(c.data(), J.gmax_c.p, sizeof(double) * c.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  double g = 0.0;
  for (double v : f) g = std::max(g, v);
  for (double v : c) g = std::max(g, v);
  for (int s = 0; s < J.pt_slots; ++s) g = std::max(g, p[2 * s + 1]);
  *gmax = g;
  return PBA_OK;
}

int step_j(pba_engine* e, double lambda, double* model, int* status, double* sq_step, double* sq_x) {
  JointSolve& J = e->joint;
  const int nf = e->n_frames, npt = e->n_points;
  if (npt > 0) joint_damp_kernel<<<(npt + 255) / 256, 256, 0, e->stream>>>(J.pt_data.p, npt, lambda, J.inv.p);
  AsmArgsJ aa{J.pair_rec.p, J.blk_data.p, J.pt_data.p, J.inv.p, J.frame_data.p, J.frame_ptr.p, J.frame_pairs.p,
              J.off_ptr.p, J.off_pairs.p, J.term_ptr.p, J.fe_ptr.p, J.fe_entries.p, J.sky_i.p, J.sky_j.p,
              e->block_point.p, J.terms.p, J.cst.p, J.S.p, J.L.p, J.g.p, nf, J.n_sky, lambda};
  joint_assemble_kernel<<<J.nc > 0 ? J.n_sky_kf : J.n_sky, 64, 0, e->stream>>>(aa);
  joint_gradient_kernel<<<(8 * nf + 255) / 256, 256, 0, e->stream>>>(aa);
  const AsmArgsI ai{aa, J.pair_intr.p, J.cam_data.p, J.blk_wc.p, J.cstc.p, e->n_blocks, J.nc, J.n_sky_kf, J.tchunks.p,
                    J.tchunk_ptr.p, J.tpart.p, J.gchunks.p, J.gchunk_ptr.p, J.gpart.p};
  if (J.nc > 0) {
    if (J.n_tchunks > 0) joint_intr_terms_kernel<<<J.n_tchunks, 64, 0, e->stream>>>(ai);
    if (J.n_gchunks > 0) joint_intr_gradient_parts_kernel<<<J.n_gchunks, 64, 0, e->stream>>>(ai);
    joint_intr_assemble_kernel<<<J.n_sky - J.n_sky_kf, 64, 0, e->stream>>>(ai);
    joint_intr_gradient_kernel<<<(8 * J.nc + 63) / 64, 64, 0, e->stream>>>(ai);
  }
  SolveArgsJ so{J.L.p, J.first.p, J.row.p, J.g.p, J.Linv.p, J.x.p, J.status.p, nf + J.nc, J.colptr.p, J.colrows.p};
  joint_solve_kernel<<<1, 256, 0, e->stream>>>(so);
  UpdArgs ua{J.x.p, J.pt_data.p, J.blk_data.p, J.inv.p, J.frame_data.p, e->poses.p, e->rho.p, e->affine_state.p,
             J.pt_ptr.p, J.pt_blocks.p, e->point_host_d.p, J.status.p, e->block_rec.p, J.cst.p, J.drho.p,
             J.poses_new.p, J.rho_new.p, J.ab_new.p, J.red3.p, npt, nf, lambda};
  if (J.nc > 0)
    joint_intr_update_kernel<<<J.upd_slots, 256, 0, e->stream>>>(UpdArgsI{
        ua, J.blk_wc.p, J.cam_data.p, e->intr_state_d.p, J.cstc.p, J.intr_new_d.p, J.intr_new_f.p, J.nc, std::ldexp(1.0, -e->level)});
  else
    joint_update_kernel<<<J.upd_slots, 256, 0, e->stream>>>(ua);
  PBA_HIP(hipGetLastError());
  int st = 0;
  std::vector<double> h(4 * (size_t)J.upd_slots);
  PBA_HIP(hipMemcpyAsync(&st, J.status.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipMemcpyAsync(h.data(), J.red3.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  double m = 0.0, ss = 0.0, xx = 0.0;
  for (int s = 0; s < J.upd_slots; ++s) {
    m += h[4 * s];
    ss += h[4 * s + 1];
    xx += h[4 * s + 2];
  }
  J.have_step = st == 0;
  J.step_band = false;
  if (status) *status = st != 0 ? 1 : 0;
  if (model) *model = st == 0 ? 0.5 * m : 0.0;
  if (sq_step) *sq_step = ss;
  if (sq_x) *sq_x = xx;
  return PBA_OK;
}

int candidate_cost_j(pba_engine* e, double* cost, double* n_valid) {
  JointSolve& J = e->joint;
  int slots = 0;
  if (int rc = launch_cost_only(e, e->pairs.p, J.rho_new.p, J.red.p, &slots, J.poses_new.p,
                                J.nc > 0 ? J.intr_new_f.p : nullptr, J.nc > 0 ? J.intr_new_d.p : nullptr, J.ab_new.p))
    return rc;
  return sum_red(e, J.red.p, slots, cost, n_valid);
}

int accept_j(pba_engine* e) {
  JointSolve& J = e->joint;
  const size_t nf = e->n_frames;
  PBA_HIP(hipMemcpyAsync(e->poses.p, J.poses_new.p, sizeof(double) * 7 * nf, hipMemcpyDeviceToDevice, e->stream));
  PBA_HIP(hipMemcpyAsync(e->rho.p, J.rho_new.p, sizeof(double) * (size_t)e->n_points, hipMemcpyDeviceToDevice, e->stream));
  PBA_HIP(hipMemcpyAsync(e->affine_state.p, J.ab_new.p, sizeof(double) * 2 * nf, hipMemcpyDeviceToDevice, e->stream));
  if (J.nc > 0) {  // the intrinsics state at the active level, then its level-0 copy on the host (pba_get_intrinsics)
    PBA_HIP(hipMemcpyAsync(e->intr_state_d.p, J.intr_new_d.p, sizeof(double) * kCamD * (size_t)J.nc, hipMemcpyDeviceToDevice, e->stream));
    PBA_HIP(hipMemcpyAsync(e->intr_state.p, J.intr_new_f.p, sizeof(float) * 8 * (size_t)J.nc, hipMemcpyDeviceToDevice, e->stream));
    if (int rc = download_intrinsics_state(e)) return rc;
  }
  J.linearized = J.have_step = false;
  e->aff.linearized = e->aff.have_step = false;
  e->pairs_fresh = false;
  e->evaluated = false;
  e->res_fresh = false;
  return PBA_OK;
}

// ---- the multi-GPU exchange: host side -------------------------------------------------------------------------------
int local_band(const pba_engine* e) { return joint_local_band(e->joint.first_h); }

int check_band(pba_engine* e, int band) {
  if (band < local_band(e) || band > e->n_frames - 1)
    return fail(PBA_ERR_INVALID_ARGUMENT, "band must lie between pba_joint_band (" + std::to_string(local_band(e)) +
                                              ") and n_frames - 1 (" + std::to_string(e->n_frames - 1) + ")");
  return PBA_OK;
}

// the exchange plan and the band storage for K (kept until K or the problem changes)
int ensure_exchange(pba_engine* e, int K) {
  JointSolve& J = e->joint;
  if (J.ex_K == K) return PBA_OK;
  JointExchangePlan X;
  if (!build_joint_exchange(J.first_h, J.row_h, K, X)) return fail(PBA_ERR_INVALID_ARGUMENT, "band out of range");
  const size_t nf = e->n_frames;
  J.ex_K = -1;
  PBA_HIP(J.ex_src.upload(X.src, e->stream));
  PBA_HIP(J.ex_first.upload(X.first, e->stream));
  PBA_HIP(J.ex_row.upload(X.row, e->stream));
  PBA_HIP(J.ex_colptr.upload(X.colptr, e->stream));
  PBA_HIP(J.ex_colrows.upload(X.colrows, e->stream));
  PBA_HIP(J.ex_sky_i.upload(X.sky_i, e->stream));
  PBA_HIP(J.ex_sky_j.upload(X.sky_j, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));  // (the plan's vectors die with this scope)
  PBA_HIP(J.ex_S.resize(64 * (size_t)X.n_sky));
  PBA_HIP(J.ex_L.resize(64 * (size_t)X.n_sky));
  PBA_HIP(J.ex_cst.resize(2 * nf));
  PBA_HIP(J.ex_frame.resize(nf * kFrame));
  PBA_HIP(J.ex_gmax_f.resize(nf));
  PBA_HIP(J.red6.resize(8 * (size_t)J.upd_slots));
  J.ex_first_h = X.first;
  J.ex_row_h = X.row;
  J.ex_n_sky = X.n_sky;
  J.ex_stride = X.stride;
  J.ex_scalar_off = X.scalar_off;
  J.ex_count = X.count;
  J.ex_K = K;
  J.ex_lin = -1;
  return PBA_OK;
}

int export_j(pba_engine* e, double lambda, int K, double* X) {
  JointSolve& J = e->joint;
  if (int rc = ensure_exchange(e, K)) return rc;
  const int nf = e->n_frames, npt = e->n_points;
  if (npt > 0) joint_damp_kernel<<<(npt + 255) / 256, 256, 0, e->stream>>>(J.pt_data.p, npt, lambda, J.inv.p);
  const AsmArgsJ aa{J.pair_rec.p, J.blk_data.p, J.pt_data.p, J.inv.p, J.frame_data.p, J.frame_ptr.p, J.frame_pairs.p,
                    J.off_ptr.p, J.off_pairs.p, J.term_ptr.p, J.fe_ptr.p, J.fe_entries.p, J.sky_i.p, J.sky_j.p,
                    e->block_point.p, J.terms.p, nullptr, nullptr, nullptr, nullptr, nf, J.n_sky, lambda};
  joint_export_kernel<<<nf * (K + 1) + nf + 1, 64, 0, e->stream>>>(ExArgsJ{aa, J.ex_src.p, X, K, J.ex_stride});
  PBA_HIP(hipGetLastError());
  J.ex_lin = J.lin_id;
  J.ex_lambda = lambda;
  J.ex_band = K;
  J.have_step = false;  // (inv is this export's: a step of another λ no longer has its point part)
  return PBA_OK;
}

struct ImportParts {
  double model_kf = 0.0, model_pt = 0.0, sq_step_kf = 0.0, sq_step_pt = 0.0, sq_x_kf = 0.0, sq_x_pt = 0.0;
  double gmax_kf = 0.0;  // the keyframes' part of the linearisation's gradient norm, from the summed direct gradient
  int status = 0;
};

// X holds the sum over the ranks of an export at (λ, K).  solve = false: only the summed system and the keyframes'
// gradient norm (the LM loop's gradient test where no trial follows).
int import_j(pba_engine* e, double lambda, int K, const double* X, bool solve, ImportParts* out) {
  JointSolve& J = e->joint;
  const int nf = e->n_frames, npt = e->n_points;
  joint_import_kernel<<<J.ex_n_sky, 64, 0, e->stream>>>(ImpArgsJ{X, J.fixed.p, e->poses.p, e->affine_state.p, J.ex_sky_i.p,
                                                                 J.ex_sky_j.p, J.ex_S.p, J.ex_L.p, J.g.p, J.ex_frame.p,
                                                                 J.ex_gmax_f.p, J.ex_cst.p, K, J.ex_stride, lambda});
  PBA_HIP(hipGetLastError());
  std::vector<double> gf(nf), h;
  int st = 0;
  if (solve) {
    SolveArgsJ so{J.ex_L.p, J.ex_first.p, J.ex_row.p, J.g.p, J.Linv.p, J.x.p, J.status.p, nf, J.ex_colptr.p, J.ex_colrows.p};
    joint_solve_kernel<<<1, 256, 0, e->stream>>>(so);
    UpdArgs ua{J.x.p, J.pt_data.p, J.blk_data.p, J.inv.p, J.ex_frame.p, e->poses.p, e->rho.p, e->affine_state.p,
               J.pt_ptr.p, J.pt_blocks.p, e->point_host_d.p, J.status.p, e->block_rec.p, J.ex_cst.p, J.drho.p,
               J.poses_new.p, J.rho_new.p, J.ab_new.p, J.red6.p, npt, nf, lambda};
    joint_update_parts_kernel<<<J.upd_slots, 256, 0, e->stream>>>(ua);
    PBA_HIP(hipGetLastError());
    h.resize(8 * (size_t)J.upd_slots);
    PBA_HIP(hipMemcpyAsync(&st, J.status.p, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    PBA_HIP(hipMemcpyAsync(h.data(), J.red6.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, e->stream));
  }
  PBA_HIP(hipMemcpyAsync(gf.data(), J.ex_gmax_f.p, sizeof(double) * gf.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  ImportParts p;
  for (int s = 0; solve && s < J.upd_slots; ++s) {
    p.model_pt += h[8 * s];
    p.sq_step_pt += h[8 * s + 1];
    p.sq_x_pt += h[8 * s + 2];
    p.model_kf += h[8 * s + 3];
    p.sq_step_kf += h[8 * s + 4];
    p.sq_x_kf += h[8 * s + 5];
  }
  for (double v : gf) p.gmax_kf = std::max(p.gmax_kf, v);
  p.status = st != 0 ? 1 : 0;
  if (solve) {
    J.have_step = st == 0;
    J.step_band = true;
  }
  *out = p;
  return PBA_OK;
}

// the checks pba_joint_step_import and the LM loop share: the export this import follows
int exported(pba_engine* e, double lambda, int K) {
  const JointSolve& J = e->joint;
  if (!J.linearized) return fail(PBA_ERR_NOT_READY, "pba_joint_linearize first");
  if (J.ex_K != K || J.ex_lin != J.lin_id || J.ex_band != K || J.ex_lambda != lambda)
    return fail(PBA_ERR_NOT_READY, "pba_joint_step_export at this lambda and band first");
  return PBA_OK;
}

}  // namespace

extern "C" {

int pba_joint_set_solve_intrinsics(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (enable && (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC || !e->opt_intr || !e->affine))
    return fail(PBA_ERR_INVALID_ARGUMENT,
                "pba_joint_set_solve_intrinsics needs pba_set_optimize_intrinsics and pba_set_affine_brightness");
  e->joint_solve_intr = enable != 0;
  return PBA_OK;
}

int pba_joint_linearize(pba_engine* e, double* cost) {
  if (int rc = ready(e, true)) return rc;
  return linearize_j(e, cost);
}

int pba_joint_system_size(pba_engine* e, int32_t* n) {
  if (int rc = ready(e, true)) return rc;
  if (!n) return fail(PBA_ERR_INVALID_ARGUMENT, "null size");
  *n = 8 * (e->n_frames + e->joint.nc);  // keyframes first, then the cameras of pba_joint_set_solve_intrinsics
  return PBA_OK;
}

int pba_joint_step(pba_engine* e, double lambda, double* model_decrease, int32_t* solver_status) {
  if (int rc = ready(e, true)) return rc;
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  if (!e->joint.linearized) return fail(PBA_ERR_NOT_READY, "pba_joint_linearize first");
  int st = 0;
  const int rc = step_j(e, lambda, model_decrease, &st, nullptr, nullptr);
  if (solver_status) *solver_status = st;
  return rc;
}

int pba_joint_get_reduced_system(pba_engine* e, double* S_dense, double* g) {
  if (int rc = ready(e, true)) return rc;
  JointSolve& J = e->joint;
  if (!J.linearized || !J.have_step) return fail(PBA_ERR_NOT_READY, "pba_joint_step first");
  const int nf = e->n_frames + J.nc;  // block rows
  const size_t n = 8 * (size_t)nf;
  if (S_dense) {  // after an import: the summed system over the band profile
    std::vector<double> S((size_t)64 * (J.step_band ? J.ex_n_sky : J.n_sky));
    PBA_HIP(hipMemcpyAsync(S.data(), J.step_band ? J.ex_S.p : J.S.p, sizeof(double) * S.size(), hipMemcpyDeviceToHost,
                           e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));
    // (a diagonal block's lower triangle is what is factored)
    skyline_to_dense<8>(S, J.step_band ? J.ex_first_h : J.first_h, J.step_band ? J.ex_row_h : J.row_h, nf, true,
                        [](int, int, int, int, double v) { return v; }, S_dense);
  }
  if (g) {
    PBA_HIP(hipMemcpyAsync(g, J.g.p, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));
  }
  return PBA_OK;
}

int pba_joint_get_step(pba_engine* e, double* d_keyframes, double* d_inv_dist) {
  if (int rc = ready(e, true)) return rc;
  JointSolve& J = e->joint;
  if (!J.linearized || !J.have_step) return fail(PBA_ERR_NOT_READY, "pba_joint_step first");
  if (d_keyframes)
    PBA_HIP(hipMemcpyAsync(d_keyframes, J.x.p, sizeof(double) * 8 * (size_t)e->n_frames, hipMemcpyDeviceToHost, e->stream));
  if (d_inv_dist)
    PBA_HIP(hipMemcpyAsync(d_inv_dist, J.drho.p, sizeof(double) * (size_t)e->n_points, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_joint_get_intrinsics_step(pba_engine* e, double* d_intrinsics) {
  if (int rc = ready(e, true)) return rc;
  JointSolve& J = e->joint;
  if (J.nc <= 0) return fail(PBA_ERR_INVALID_ARGUMENT, "pba_joint_set_solve_intrinsics first");
  if (!J.linearized || !J.have_step) return fail(PBA_ERR_NOT_READY, "pba_joint_step first");
  if (d_intrinsics) {
    PBA_HIP(hipMemcpyAsync(d_intrinsics, J.x.p + 8 * (size_t)e->n_frames, sizeof(double) * 8 * (size_t)J.nc,
                           hipMemcpyDeviceToHost, e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));
  }
  return PBA_OK;
}

int pba_joint_candidate_cost(pba_engine* e, double* cost) {
  if (int rc = ready(e, true)) return rc;
  if (!cost) return fail(PBA_ERR_INVALID_ARGUMENT, "null cost");
  if (!e->joint.linearized || !e->joint.have_step) return fail(PBA_ERR_NOT_READY, "pba_joint_step first");
  double nv = 0.0;
  return candidate_cost_j(e, cost, &nv);
}

int pba_joint_accept(pba_engine* e) {
  if (int rc = ready(e, true)) return rc;
  if (!e->joint.linearized || !e->joint.have_step) return fail(PBA_ERR_NOT_READY, "pba_joint_step first");
  return accept_j(e);
}

// The host-driven trust-region loop (pba_host_lm.h); norms over the free poses (ambient [q | t]), the ρ of points with
// blocks and the free (a, b).  ‖x‖ after an accepted step is its candidate's, from the step's ‖candidate‖².
int pba_solve_joint(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum) {
  if (int rc = ready(e, true)) return rc;
  double sq_x = 0.0;
  HostLmStages stages{
      [&](double* cost, double* gmax, double* x_norm) {
        if (int rc = linearize_j(e, cost)) return rc;
        *x_norm = std::sqrt(sq_x);
        return gradient_norm(e, gmax);
      },
      [&](double lambda, int* status, double* model, double* sq_step) {
        return step_j(e, lambda, model, status, sq_step, &sq_x);
      },
      [&](double* cost) {
        double nv = 0.0;
        if (int rc = candidate_cost_j(e, cost, &nv)) return rc;
        if (nv < e->joint.n_valid) *cost = DBL_MAX;  // a failed evaluation (pba_solve's rule)
        return PBA_OK;
      },
      [&]() { return accept_j(e); }};
  return host_lm(o, stages, e->gn.history, sum);
}

int pba_joint_band(pba_engine* e, int32_t* band) {
  if (int rc = ready(e)) return rc;
  if (!band) return fail(PBA_ERR_INVALID_ARGUMENT, "null band");
  *band = local_band(e);
  return PBA_OK;
}

int pba_joint_exchange_size(pba_engine* e, int32_t band, int64_t* count) {
  if (int rc = ready(e)) return rc;
  if (!count) return fail(PBA_ERR_INVALID_ARGUMENT, "null count");
  if (int rc = check_band(e, band)) return rc;
  *count = ((int64_t)(band + 1) * 64 + kJointExTail) * e->n_frames + kJointExScalars;
  return PBA_OK;
}

int pba_joint_step_export(pba_engine* e, double lambda, int32_t band, double* d_exchange) {
  if (int rc = ready(e)) return rc;
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  if (!d_exchange) return fail(PBA_ERR_INVALID_ARGUMENT, "null exchange buffer");
  if (int rc = check_band(e, band)) return rc;
  if (!e->joint.linearized) return fail(PBA_ERR_NOT_READY, "pba_joint_linearize first");
  return export_j(e, lambda, band, d_exchange);
}

int pba_joint_step_import(pba_engine* e, double lambda, int32_t band, const double* d_exchange, double* model_keyframes,
                          double* model_points, int32_t* solver_status) {
  if (int rc = ready(e)) return rc;
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  if (!d_exchange) return fail(PBA_ERR_INVALID_ARGUMENT, "null exchange buffer");
  if (int rc = check_band(e, band)) return rc;
  if (int rc = exported(e, lambda, band)) return rc;
  ImportParts p;
  if (int rc = import_j(e, lambda, band, d_exchange, true, &p)) return rc;
  if (solver_status) *solver_status = p.status;
  if (model_keyframes) *model_keyframes = p.status == 0 ? 0.5 * p.model_kf : 0.0;
  if (model_points) *model_points = p.status == 0 ? 0.5 * p.model_pt : 0.0;
  return PBA_OK;
}

// pba_solve_joint's loop over all ranks: host_lm with the stages below.  One sum of the scalar slots per linearisation,
// and per trial the sum of the system, then of the scalar slots.  What decides — cost, valid blocks, model decrease,
// norms, the solve's status, the gradient test — is either a sum over the ranks or computed by every rank from the
// summed buffer, so every rank takes the same decisions and none is exchanged.
// The gradient norm: max(the keyframes' part, this rank's points).  The keyframes' part needs the summed direct
// gradient, which a linearisation has only once its first trial has summed the system, so the value reported with a
// linearisation carries the keyframes' part of the last summed system.  The gradient-tolerance stop does not rest on
// that: it can apply only where no rank holds a point above the tolerance (slot 3 sums to 0), and there every rank
// exports at λ = 0 and the system is summed once more for this linearisation's own keyframe part.
int pba_solve_joint_distributed(pba_engine* e, const pba_solver_options* o, int32_t band, double* d_exchange,
                                pba_allreduce_fn allreduce, void* user, pba_solver_summary* sum) {
  if (int rc = ready(e)) return rc;
  if (!d_exchange || !allreduce) return fail(PBA_ERR_INVALID_ARGUMENT, "null exchange buffer or allreduce");
  if (int rc = check_band(e, band)) return rc;
  if (int rc = ensure_exchange(e, band)) return rc;
  JointSolve& J = e->joint;
  const int K = band;
  const long long nx = J.ex_scalar_off;
  double* const Y = d_exchange + nx;
  const double gtol = o ? o->gradient_tolerance : 1e-10;
  auto reduce = [&](double* buf, long long n) {  // the host callback: after the stream has drained, complete on return
    PBA_HIP(hipStreamSynchronize(e->stream));
    if (int rc = allreduce(user, buf, n)) return fail(PBA_ERR_DEVICE, "allreduce callback failed (" + std::to_string(rc) + ")");
    return (int)PBA_OK;
  };
  auto reduce_scalars = [&](double (&v)[kJointExScalars]) {
    PBA_HIP(hipMemcpyAsync(Y, v, sizeof v, hipMemcpyHostToDevice, e->stream));
    if (int rc = reduce(Y, kJointExScalars)) return rc;
    PBA_HIP(hipMemcpyAsync(v, Y, sizeof v, hipMemcpyDeviceToHost, e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));
    return (int)PBA_OK;
  };
  double n_valid = 0.0;            // Σ over the ranks, of the current linearisation
  double sq_x_kf = 0.0, sq_x_pt = 0.0;  // ‖candidate‖² of the last step: the keyframes', this rank's points'
  double gmax_kf = 0.0;            // the keyframes' part of the gradient norm, of the last summed system
  double cand = 0.0, cand_valid = 0.0;
  HostLmStages stages{
      [&](double* cost, double* gmax, double* x_norm) {
        double c = 0.0, gp = 0.0;
        if (int rc = linearize_j(e, &c)) return rc;
        std::vector<double> p(2 * (size_t)std::max(J.pt_slots, 1), 0.0);
        if (J.pt_slots > 0) {
          PBA_HIP(hipMemcpyAsync(p.data(), J.gmax_p.p, sizeof(double) * 2 * (size_t)J.pt_slots, hipMemcpyDeviceToHost, e->stream));
          PBA_HIP(hipStreamSynchronize(e->stream));
        }
        double above = 0.0;  // this rank's point groups (joint_point_kernel's workgroups) with an entry above the tolerance
        for (int s = 0; s < J.pt_slots; ++s) {
          gp = std::max(gp, p[2 * s + 1]);
          above += p[2 * s + 1] > gtol ? 1.0 : 0.0;
        }
        double v[kJointExScalars] = {c, J.n_valid, sq_x_pt, above};
        if (int rc = reduce_scalars(v)) return rc;
        *cost = v[0];
        n_valid = v[1];
        *x_norm = std::sqrt(sq_x_kf + v[2]);
        if (v[3] == 0.0) {  // no point above the tolerance on any rank: the keyframes decide
          if (int rc = export_j(e, 0.0, K, d_exchange)) return rc;
          if (int rc = reduce(d_exchange, nx)) return rc;
          ImportParts ip;
          if (int rc = import_j(e, 0.0, K, d_exchange, false, &ip)) return rc;
          gmax_kf = ip.gmax_kf;
        }
        double g = std::max(gmax_kf, gp);
        if (v[3] > 0.0 && !(g > gtol)) g = std::nextafter(gtol, DBL_MAX);  // (above the tolerance on another rank)
        *gmax = g;
        return (int)PBA_OK;
      },
      [&](double lambda, int* status, double* model, double* sq_step) {
        if (int rc = export_j(e, lambda, K, d_exchange)) return rc;
        if (int rc = reduce(d_exchange, nx)) return rc;
        ImportParts ip;
        if (int rc = import_j(e, lambda, K, d_exchange, true, &ip)) return rc;
        gmax_kf = ip.gmax_kf;
        *status = ip.status;
        *model = 0.0;
        *sq_step = 0.0;
        if (ip.status != 0) return (int)PBA_OK;  // (the same status on every rank: none sums the scalars)
        double c = 0.0, nv = 0.0;
        if (int rc = candidate_cost_j(e, &c, &nv)) return rc;
        double v[kJointExScalars] = {ip.model_pt, c, nv, ip.sq_step_pt, ip.sq_x_pt};
        if (int rc = reduce_scalars(v)) return rc;
        *model = 0.5 * (ip.model_kf + v[0]);
        cand = v[1];
        cand_valid = v[2];
        *sq_step = ip.sq_step_kf + v[3];
        sq_x_kf = ip.sq_x_kf;
        sq_x_pt = ip.sq_x_pt;
        return (int)PBA_OK;
      },
      [&](double* cost) {
        *cost = cand_valid < n_valid ? DBL_MAX : cand;  // a failed evaluation (pba_solve's rule), over all ranks
        return (int)PBA_OK;
      },
      [&]() { return accept_j(e); }};
  return host_lm(o, stages, e->gn.history, sum);
}

}  // extern "C"
