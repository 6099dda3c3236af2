// pba_gn_intr.hip — free intrinsics in the reduced camera system of a Gauss-Newton trial (pba_gn.hip): the weighted
// fp64 rows (intr_rows_kernel; photometric engines: the blocks' moment records, intr_rows_photometric_kernel), the points'
// camera sums (intr_pw_kernel), the border kernels (intr_border_*, intr_cam_*) and the candidate intrinsics' accept (intr_accept_kernel), with their launchers (pba_gn_intr.h).  The part fused into
// other kernels stays with them in pba_gn.hip: AcceptCopy (the elimination's launch applies the accept) and
// intr_update_frame (update_kernel).  intr_cam_fin_build_kernel builds the arrow solve's level 0 with arrow_build
// (pba_gn_solve.h).
//
// bundle_adjustment() with BundleAdjustmentOptions::optimize_intrinsics leaves the cameras' 8-vector intrinsics blocks
// free (map_utils.h:339-345); the functor differentiates the TARGET camera's intrinsics (reprojection.h:83-86, :108) and
// SPARSE_SCHUR keeps those blocks among the f-blocks of the reduced camera system (schur_complement_solver.cc:138-146).
// Here camera c's intrinsics are the system frames nf + 2c (dims 0-5) and nf + 2c + 1 (dims 6-7, then four identity
// pads): a dense border of the skyline system (their profile starts at frame 0).  The keyframe part is linearised,
// eliminated and assembled as without intrinsics; the border — the blocks' direct terms J_iᵀJ_x and the points' Schur
// terms −W_i,c W_xᵀ / H'_ρρ — is formed in fp64 by the border kernels below (a wave per keyframe block, camera blocks
// split over workgroups) in a fixed order (the CSR lists of gn_prepare), from weighted fp64 rows (intr_rows_kernel) and
// schur_kernel's undamped H_ρρ; on several GPUs each rank exports its border rows undamped (import_sky_kernel sums them).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "pba_gn.h"
#include "pba_gn_intr.h"
#include "pba_gn_solve.h"

using namespace pba;
using namespace pba::detail;

namespace {

// ib_data per GN block (free intrinsics, intr_rows_kernel): weighted fp64 rows J_i (2×8) | J_h (2×6) | J_t (2×6) | J_ρ (2) |
// r (2), and W_i = J_iᵀJ_ρ (8)
constexpr int kIbStride = 52;
constexpr int kIbJi = 0, kIbJh = 16, kIbJt = 28, kIbJr = 40, kIbR = 42, kIbWi = 44;

// ib_data per GN block of a PHOTOMETRIC engine (intr_rows_photometric_kernel): the second moments of the block's P weighted
// rows [r | J_i (8) | J_h (6) | J_t (6) | J_ρ] that the border kernels use — 160 doubles whatever P (the rows themselves
// would be 22·P): M_h = J_iᵀJ_h (8×6) | M_t = J_iᵀJ_t (8×6) | the upper triangle of J_iᵀJ_i (36) | J_iᵀr (8) |
// W_i = J_iᵀJ_ρ (8) | w_h = J_hᵀJ_ρ (6) | w_t = J_tᵀJ_ρ (6)
constexpr int kMomStride = 160;
constexpr int kMomMh = 0, kMomMt = 48, kMomTri = 96, kMomJr = 132, kMomWi = 140, kMomWh = 148, kMomWt = 154;
template <bool MOM>
constexpr int kStrideOf = MOM ? kMomStride : kIbStride;

struct IntrRowsArgs {
  const int4* rec;       // GN block → {block, point, host, target}
  const double* poses;
  const double* rho;
  const double2* u_ref;
  const double2* u_obs;
  const int* frame_cam;
  const double* cams;    // host unprojection: the cameras (the functor's captured intrinsics, reprojection.h:93-98)
  const double* kt;      // target projection: the intrinsics state (camera records)
  double huber;
  double* out;           // ib_data
  int n;
  const double* lm;      // LM record: nothing to do once the solve is done
  // point-aligned waves (gn_prepare, every GN point ≤ 64 blocks): wave w takes GN blocks wave_tab[w].x … + .y − 1, whole
  // points from GN point wave_tab[w].z on, and also writes their W sums into pw (intr_pw_kernel's work); else nullptr
  const int4* wave_tab = nullptr;
  int n_waves = 0;
  double* pw = nullptr;
  int nc = 0;
};
struct PoseT {  // a relative pose for pair_rotation / pair_translation
  double R[9], t[3];
  float Rf[9], tf[3];
};

// One lane per GN block at the current state: r = u_obs − π_t(T_th b/ρ) and its Jacobians (the geometric_row chain, in
// fp64), J_i = −∂π/∂k (project_intr_jac), Ceres' Corrector weighting √ρ' (corrector.cc, ρ'' ≤ 0 for Huber), W_i = J_iᵀJ_ρ.
// The rows leave through LDS (PBA_IB_DIRECT: straight from the lanes): a lane's 416-B row stored from registers is 26
// 16-B stores 416 B apart per instruction — 64 partial lines each — so each wave stages its 64 rows in two halves of 26
// doubles and stores every half as the 13 16-B chunks of each row, consecutive lanes on consecutive chunks.
#ifndef PBA_IB_DIRECT
constexpr int kIbStage = 27;  // doubles per staged half row (26 used; odd: 2-way LDS bank conflicts at most)
#endif
template <int MODEL>
__global__ __launch_bounds__(256) void intr_rows_kernel(const IntrRowsArgs a) {
  const int lane = threadIdx.x & 63;
#ifdef PBA_IB_DIRECT
  const int gb0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (gb0 >= a.n || lm_view(a.lm).done != 0.0) return;
  const int gb = gb0;
#else
  // the wave's rows: 64 consecutive GN blocks, or (wave_tab) a point-aligned run of ≤ 64
  int row0, nrow;
  int4 wt = make_int4(0, 0, 0, 0);
  if (a.wave_tab) {
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= a.n_waves) return;  // (whole waves)
    wt = a.wave_tab[w];
    row0 = wt.x;
    nrow = wt.y;
  } else {
    row0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63);
    nrow = min(64, a.n - row0);
    if (nrow <= 0) return;  // (whole waves: the last workgroup's waves past the end — rec has a.n entries)
  }
  if (lm_view(a.lm).done != 0.0) return;       // (uniform)
  const int gb = row0 + max(min(lane, nrow - 1), 0);  // every lane of a wave takes part in its stores
#endif
  const int4 br = a.rec[gb];
  PoseT T;
  pair_rotation(a.poses + 7 * br.z, a.poses + 7 * br.w, T);
  pair_translation(a.poses + 7 * br.z, a.poses + 7 * br.w, T);
  const int hc = a.frame_cam[br.z], tc = a.frame_cam[br.w];
  const double* kt = a.kt + kCamD * tc;
  const double2 ur = a.u_ref[br.y], uo = a.u_obs[br.x];
  const double irho = 1.0 / a.rho[br.y];
  const Vec3d b = unproject<MODEL>(a.cams + kCamD * hc + kCamHk, ur.x, ur.y);
  const Vec3d ph = {b.x * irho, b.y * irho, b.z * irho};
  const Vec3d Rp = mat_mul(T.R, ph);
  const Vec3d p = {Rp.x + T.t[0], Rp.y + T.t[1], Rp.z + T.t[2]};
  double u, v;
  const double iden = project<MODEL>(kt, p, u, v);
  double J[kIbStride];
  J[kIbR] = uo.x - u;
  J[kIbR + 1] = uo.y - v;
  Vec3d du, dv;
  project_jac<MODEL>(kt, p, iden, du, dv);
  double ku[8], kv[8];
  project_intr_jac<MODEL>(kt, p, iden, ku, kv);
  const Vec3d td = {T.t[0], T.t[1], T.t[2]};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const Vec3d d = i == 0 ? du : dv;
    const Vec3d g = {-d.x, -d.y, -d.z};  // ∂r/∂p = −∂π/∂p
    const Vec3d gR = row_mul(g, T.R);
    const Vec3d wh = cross(ph, gR);
    const Vec3d wt = cross(g, p);
    double* jh = J + kIbJh + 6 * i;
    double* jt = J + kIbJt + 6 * i;
    jh[0] = gR.x; jh[1] = gR.y; jh[2] = gR.z; jh[3] = wh.x; jh[4] = wh.y; jh[5] = wh.z;
    jt[0] = -g.x; jt[1] = -g.y; jt[2] = -g.z; jt[3] = wt.x; jt[4] = wt.y; jt[5] = wt.z;
    J[kIbJr + i] = dot(g, td) * irho;
#pragma unroll
    for (int j = 0; j < 8; ++j) J[kIbJi + 8 * i + j] = -(i == 0 ? ku[j] : kv[j]);
  }
  bool ok = true;
#pragma unroll
  for (int q = 0; q < kIbWi; ++q) ok = ok && isfinite(J[q]);
  const double s2 = J[kIbR] * J[kIbR] + J[kIbR + 1] * J[kIbR + 1], hb = a.huber;
  const double w = (hb <= 0.0 || s2 <= hb * hb) ? 1.0 : hb / sqrt(s2);
  const double sw = ok ? sqrt(w) : 0.0;
#pragma unroll
  for (int q = 0; q < kIbWi; ++q) J[q] = ok ? sw * J[q] : 0.0;
#pragma unroll
  for (int d = 0; d < 8; ++d) J[kIbWi + d] = J[kIbJi + d] * J[kIbJr] + J[kIbJi + 8 + d] * J[kIbJr + 1];
#ifdef PBA_IB_DIRECT
  double* o = a.out + (long long)gb * kIbStride;
#pragma unroll
  for (int q = 0; q < kIbStride; q += 2) *reinterpret_cast<double2*>(o + q) = make_double2(J[q], J[q + 1]);
#else
  constexpr int HALF = kIbStride / 2, CH = HALF / 2;  // 26 doubles, 13 chunks of 16 B per half row
  __shared__ double stage[4][64 * kIbStage];
  double* st = stage[threadIdx.x >> 6];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int q = 0; q < HALF; ++q) st[lane * kIbStage + q] = J[HALF * h + q];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int c0 = 0; c0 < 64 * CH; c0 += 64) {
      const int c = c0 + lane, r = c / CH, j = c - CH * r;
      if (r < nrow)
        *reinterpret_cast<double2*>(a.out + (long long)(row0 + r) * kIbStride + HALF * h + 2 * j) =
            make_double2(st[r * kIbStage + 2 * j], st[r * kIbStage + 2 * j + 1]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // this half's reads before the next half's writes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (!a.wave_tab) return;
  // the points' W sums (intr_pw_kernel's, in the same block order): each block's W_i, J_hᵀJ_ρ and camera through the
  // stage, then the first block of every point adds its point's blocks
  const int cam = a.frame_cam[br.w];
#pragma unroll
  for (int d = 0; d < 8; ++d) st[lane * kIbStage + d] = J[kIbWi + d];
#pragma unroll
  for (int k = 0; k < 6; ++k)
    st[lane * kIbStage + 8 + k] = J[kIbJh + k] * J[kIbJr] + J[kIbJh + 6 + k] * J[kIbJr + 1];
  st[lane * kIbStage + 14] = (double)cam;
  const bool live = lane < nrow;
  const int prev_pt = __shfl(br.y, (lane + 63) & 63, 64);
  const unsigned long long firsts = __ballot(live && (lane == 0 || br.y != prev_pt));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (!((firsts >> lane) & 1ull)) return;
  const unsigned long long later = lane == 63 ? 0ull : firsts >> (lane + 1);
  const int nb = later ? __builtin_ctzll(later) + 1 : nrow - lane;  // this point's blocks: lanes lane … lane + nb − 1
  const int gp = wt.z + __popcll(firsts & ((1ull << lane) - 1ull));
  double* o = a.pw + (long long)gp * (8 * a.nc + 6);
  double wh[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < a.nc; c0 += 4) {  // cameras in groups of four, as intr_pw_kernel
    double wc[4][8];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int d = 0; d < 8; ++d) wc[c][d] = 0.0;
    for (int b = lane; b < lane + nb; ++b) {
      const double* sb = st + b * kIbStage;
      const int cb = (int)sb[14] - c0;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const double w = sb[d];
#pragma unroll
        for (int c = 0; c < 4; ++c) wc[c][d] += c == cb ? w : 0.0;
      }
      if (c0 == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) wh[k] += sb[8 + k];
    }
    for (int c = 0; c < 4 && c0 + c < a.nc; ++c)
#pragma unroll
      for (int d = 0; d < 8; ++d) o[8 * (c0 + c) + d] = wc[c][d];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) o[8 * a.nc + k] = wh[k];
#endif
}

// ---- the photometric producer --------------------------------------------------------------------------------------
// The columns (ca, cb) of the staged row [r | J_i (1-8) | J_h (9-14) | J_t (15-20) | J_ρ (21)] whose product is moment m
// of the record (kMom*).
__device__ __forceinline__ int2 mom_cols(int m) {
  if (m < kMomMt) return make_int2(1 + m / 6, 9 + m % 6);
  if (m < kMomTri) return make_int2(1 + (m - kMomMt) / 6, 15 + (m - kMomMt) % 6);
  if (m < kMomJr) {  // row i of the 8 × 8 upper triangle holds 8 − i entries (upper8i)
    int i = 0, q = m - kMomTri;
    while (q >= 8 - i) {
      q -= 8 - i;
      ++i;
    }
    return make_int2(1 + i, 1 + i + q);
  }
  if (m < kMomWi) return make_int2(1 + (m - kMomJr), 0);
  if (m < kMomWh) return make_int2(1 + (m - kMomWi), 21);
  if (m < kMomWt) return make_int2(9 + (m - kMomWh), 21);
  return make_int2(15 + (m - kMomWt), 21);
}

struct IntrMomArgs {
  const int4* rec;   // GN block → {block, point, host, target}
  double* out;       // ib_data: kMomStride doubles per GN block
  int n;             // GN blocks
  const double* lm;  // LM record: nothing to do once the solve is done
};

// Eight lanes per GN block at the current state, eight blocks per wave (the linearisation's split): lane k evaluates
// pattern pixels k, k + 8, … in ⌈P/8⌉ passes — photometric_row with INTR, the 22 columns of the record path (fp64 warp
// and projection, fp32 chain; J_i columns 0-3 scaled by 2^−level), the block formed from the state's poses and the
// intrinsics state (stage_tile's fused-state prologue) — and stages the pass's rows, unweighted and as doubles, in the
// wave's LDS (a row that is not ok: zeros).  The wave's 8 × 160 moments are dealt over its lanes, 20 each, moment
// o = lane + 64·i of the wave's record run: each is Σ over the block's rows in pixel order of the product of two staged
// columns, in fp64 (the products of fp32 values are exact), a fixed order and no atomics.  The block's Corrector weight
// ρ' from Σ r_k² and the Huber width (the linearisation's float arithmetic) then scales every moment (x̃ᵀỹ = ρ'·xᵀy); a
// block the linearisation counts invalid (a pixel outside the projection domain or not finite) is zero.  The wave's
// records are 1280 consecutive doubles: every store instruction writes 512 consecutive bytes.
template <int PM>
__global__ __launch_bounds__(256) void intr_rows_photometric_kernel(const KernelArgs a, const IntrMomArgs g) {
  constexpr int LPB = 8, BW = 8, NM = kMomStride * BW / 64;  // 20 moments per lane
  constexpr int kRowS = 23;  // doubles per staged row (22 used; odd: no systematic bank conflicts)
  static_assert(kMomStride * BW % 64 == 0, "the wave's moments dealt evenly");
  __shared__ __attribute__((aligned(16))) TileBlock s_tile[4][BW];
  __shared__ double s_rows[4][64 * kRowS];
  __shared__ float2 s_pat[4][PBA_MAX_PATTERN];
  __shared__ float s_w[4][BW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = lane & (LPB - 1), wb = lane >> 3;
  const int gb0 = (blockIdx.x * 4 + wave) * BW;
  // (whole waves leave; everything below is private to the wave: no workgroup barrier)
  if (gb0 >= g.n || lm_view(g.lm).done != 0.0) return;
  const int nbw = min(BW, g.n - gb0);
  const bool live = wb < nbw;
  const int4 br = g.rec[live ? gb0 + wb : g.n - 1];  // a dead block evaluates the last block, masked below
  const int P = a.P;
  if (lane < PBA_MAX_PATTERN) s_pat[wave][lane] = pattern_at<PBA_MAX_PATTERN>(a, lane);
  stage_tile<LPB>(a, s_tile[wave], wb, k, br.x, true);
  // the moments of this lane: both columns' offsets in the staged rows of the moment's block
  int off[NM];
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    const int o = lane + 64 * i, b = o / kMomStride;
    const int2 c = mom_cols(o - kMomStride * b);
    off[i] = (b * LPB * kRowS + c.x) | ((b * LPB * kRowS + c.y) << 16);
  }
  double acc[NM];
#pragma unroll
  for (int i = 0; i < NM; ++i) acc[i] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const TileBlock& tb = s_tile[wave][wb];
  double* X = s_rows[wave];
  int okl = 1;
  float s = 0.0f;
#pragma unroll 1
  for (int px0 = 0; px0 < P; px0 += LPB) {
    const int px = px0 + k;
    const bool act = live && px < P;
    const float Ih = act ? a.host_int[(long long)br.y * P + px] : 0.0f;
    float ji[8];
    const Row row = photometric_row<PM, true, TileBlock, false, true>(a, tb, s_pat[wave][act ? px : 0], Ih, nullptr, ji);
    const bool use = act && row.ok;
    okl &= act ? row.ok : 1;
    s += use ? row.r * row.r : 0.0f;
    auto xv = [&](float v) { return use ? (double)v : 0.0; };  // selects: a row that is not ok may hold inf / NaN
    double* xr = X + lane * kRowS;
    xr[0] = xv(row.r);
#pragma unroll
    for (int j = 0; j < 8; ++j) xr[1 + j] = xv(ji[j]);
    xr[9] = xv(row.hv.x); xr[10] = xv(row.hv.y); xr[11] = xv(row.hv.z);
    xr[12] = xv(row.hw.x); xr[13] = xv(row.hw.y); xr[14] = xv(row.hw.z);
    xr[15] = xv(row.tv.x); xr[16] = xv(row.tv.y); xr[17] = xv(row.tv.z);
    xr[18] = xv(row.tw.x); xr[19] = xv(row.tw.y); xr[20] = xv(row.tw.z);
    xr[21] = xv(row.jr);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int i = 0; i < NM; ++i) {
      const double* xa = X + (off[i] & 0xffff);
      const double* xb = X + (off[i] >> 16);
#pragma unroll
      for (int q = 0; q < LPB; ++q) acc[i] += xa[q * kRowS] * xb[q * kRowS];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // this pass's reads before the next pass's row stores
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  const int ok = group_all<LPB>(okl);
  s = group_sum<LPB>(s);
  if (k == 0) s_w[wave][wb] = live && ok ? huber_weight(s, a.huber) : 0.0f;  // (> 0 for a valid block)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double* out = g.out + (long long)gb0 * kMomStride;
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    const int o = lane + 64 * i;
    const float w = s_w[wave][o / kMomStride];
    if (o < nbw * kMomStride) out[o] = w > 0.0f ? (double)w * acc[i] : 0.0;
  }
}

struct IntrBorderArgs {
  const double* ib;        // ib_data
  const int4* ib_rec;      // GN block → {block, point, host, target}
  const int* ib_cam;       // GN block → its target's camera
  const int4* pt_rec;      // GN point → {first GN block, block count, host, point}
  const double* pt_data;   // GN point → [H_ρρ (undamped), g_ρ, …] (schur_kernel of this solve)
  const int* bptr;         // border unit pair (c, u) = c·(nf + nc) + u → direct-term GN blocks …
  const int* blist;        // (keyframe units: bit 31 set when the keyframe hosts the block)
  const int* pptr;         // … and Schur-term GN points
  const int* plist;
  const int* sky_first;
  const int* sky_row;
  const uint8_t* fixed;    // system frames
  const double* lm;
  double* S;
  double* g;
  double* g_dir;
  double* Ddiag;
  int nf, nc;
  double* X = nullptr;     // multi-GPU export (pba_gn_step_export): this rank's border rows, undamped, into the exchange
  long long xs = 0;        // buffer's border region (row stride nfs·36 + EX_TAIL) instead of S
  const double* pw = nullptr;  // GN point → its camera sums W_c (8 per camera) and W_h = Σ J_hᵀJ_ρ (6): intr_pw_kernel
  const int* pblk = nullptr;   // per plist entry of a keyframe unit: −1 the keyframe hosts the point, else the point's
                               // one block targeting it (−2: several — walk the point's blocks)
};

// Per GN point, over its blocks in order: W_c = Σ_{b: camera(b) = c} W_i(b) for every camera c, and W_h = Σ_b J_h(b)ᵀJ_ρ(b)
// (every block of a point has the point's host).  The border kernels' Schur terms read these 8·nc + 6 values instead of
// walking the point's blocks (4-5 × 52 doubles) once per (point, list) — at C4 that walk re-read the blocks' rows five
// times per kernel, ≈ 0.4 GB per launch.  The same sums in the same order: the border is unchanged bit for bit.
// MOM (here and in the border kernels): the blocks are moment records (photometric engines) — W_i and w_h are read, not
// formed from two rows; the sums and their order are the same.
template <bool MOM>
__global__ __launch_bounds__(256) void intr_pw_kernel(const IntrBorderArgs a, int n_points) {
  // 8 lanes per point: lane k sums component k of every camera's W_c and (k < 6) of W_h, over the blocks in order
  const int t = blockIdx.x * blockDim.x + threadIdx.x, gp = t >> 3, k = t & 7;
  if (gp >= n_points) return;
  const int4 pr = a.pt_rec[gp];
  const int st = 8 * a.nc + 6;
  double* o = const_cast<double*>(a.pw) + (long long)gp * st;
  double wh = 0.0;
  for (int c0 = 0; c0 < a.nc; c0 += 4) {  // cameras in groups of four (one pass over the blocks per group)
    double wc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = pr.x; b < pr.x + pr.y; ++b) {
      const double* B = a.ib + (long long)b * kStrideOf<MOM>;
      const int cb = a.ib_cam[b] - c0;
      const double w = B[(MOM ? kMomWi : kIbWi) + k];
#pragma unroll
      for (int c = 0; c < 4; ++c) wc[c] += c == cb ? w : 0.0;
      if constexpr (MOM) {
        if (c0 == 0 && k < 6) wh += B[kMomWh + k];
      } else {
        if (c0 == 0 && k < 6) wh += B[kIbJh + k] * B[kIbJr] + B[kIbJh + 6 + k] * B[kIbJr + 1];
      }
    }
    for (int c = 0; c < 4 && c0 + c < a.nc; ++c) o[8 * (c0 + c) + k] = wc[c];
  }
  if (k < 6) o[8 * a.nc + k] = wh;
}

// Element t of border row `row` (system frame P = nf + row): t < (P + 1)·36 → entry (r, cc) of block (P, y = t / 36) of
// the skyline system; t = nfs·36 … nfs·36 + 5 → g of P.  The keyframe blocks (P, x < nf) and the camera blocks (P, y ≥ nf)
// get direct − Schur terms, + λ·clamp(diag) on the diagonal (the direct part is Ceres' LM diagonal), identity pads, and
// — constant frames / unobserved cameras — identity rows and columns, as assemble_kernel.  border_store writes element t
// from its two totals (direct, Schur).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double border_inv(const IntrBorderArgs& a, int gp, double lambda) {
  const double H = a.pt_data[(long long)gp * 8];
  const double Hd = H + lambda * fmin(fmax(H, 1e-6), 1e32);
  return Hd > 0.0 ? 1.0 / Hd : 0.0;
}
__device__ __forceinline__ void border_store(const IntrBorderArgs& a, double lambda, int row, int t, double dir,
                                             double sch) {
  const int P = a.nf + row, nfs = a.nf + 2 * a.nc, h = row & 1;
  if (a.X) {  // export: direct − Schur, the direct diagonal, g, the direct gradient, observed (import_sky_kernel damps,
              // pads and fixes the summed rows)
    double* xr = a.X + (long long)row * a.xs;
    double* tail = xr + (long long)nfs * 36;
    if (t >= nfs * 36) {
      const int r = t - nfs * 36;
      tail[r] = dir - sch;
      tail[6 + r] = dir;
      if (r == 0) tail[18] = a.fixed[P] ? 0.0 : 1.0;  // a camera this rank observes
      return;
    }
    const int y = t / 36, e = t % 36, r = e / 6, cc = e % 6, d = 6 * h + r;
    const int d2 = y >= a.nf ? 6 * ((y - a.nf) & 1) + cc : cc;
    const bool pad = d >= 8 || d2 >= 8;
    xr[(long long)y * 36 + e] = pad ? 0.0 : dir - sch;
    if (y == P && r == cc) tail[12 + r] = pad ? 0.0 : dir;
    return;
  }
  if (t >= nfs * 36) {
    const int r = t - nfs * 36;
    const bool fx = a.fixed[P] != 0;
    a.g[6 * P + r] = fx ? 0.0 : dir - sch;
    a.g_dir[6 * P + r] = fx ? 0.0 : dir;
    if (fx) a.Ddiag[6 * P + r] = 0.0;
    return;
  }
  const int y = t / 36, e = t % 36, r = e / 6, cc = e % 6, d = 6 * h + r;
  const bool cam = y >= a.nf;
  const int d2 = cam ? 6 * ((y - a.nf) & 1) + cc : cc;
  if (d >= 8 || d2 >= 8) {  // pad
    dir = (y == P && r == cc) ? 1.0 : 0.0;
    sch = 0.0;
  }
  double val = dir - sch;
  if (a.fixed[P] || a.fixed[y]) {
    val = (y == P && r == cc) ? 1.0 : 0.0;
  } else if (y == P && r == cc) {
    const double D = fmin(fmax(dir, 1e-6), 1e32);  // levenberg_marquardt_strategy.cc: the undamped JᵀJ diagonal
    a.Ddiag[6 * P + r] = D;
    val += lambda * D;
  }
  a.S[((long long)a.sky_row[P] + (y - a.sky_first[P])) * 36 + e] = val;
}

// Σ over the wave of 48 per-lane values v[0 … 47] by recursive halving (a reduce-scatter: 24 + 12 + 6 + 3 + 6 shuffles
// instead of 48 six-step butterflies): after the xor-32 / 16 / 8 / 4 steps lane l holds partial sums of the three values
// base(l) … base(l) + 2, base = 24·b5 + 12·b4 + 6·b3 + 3·b2 of l's bits, completed over its quad by xor 2 and xor 1 (a + b
// and b + a: the quad's lanes agree bit for bit).  Returns the total of value *vi = base(l) + (l & 3) for l & 3 < 3
// (*vi = −1 and 0 otherwise).  A fixed order.
__device__ __forceinline__ double wave_rs48(const double (&v)[48], int lane, int* vi) {
  double a24[24], a12[12], a6[6], a3[3];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
#pragma unroll
  for (int i = 0; i < 24; ++i) a24[i] = (h5 ? v[24 + i] : v[i]) + __shfl_xor(h5 ? v[i] : v[24 + i], 32, 64);
#pragma unroll
  for (int i = 0; i < 12; ++i) a12[i] = (h4 ? a24[12 + i] : a24[i]) + __shfl_xor(h4 ? a24[i] : a24[12 + i], 16, 64);
#pragma unroll
  for (int i = 0; i < 6; ++i) a6[i] = (h3 ? a12[6 + i] : a12[i]) + __shfl_xor(h3 ? a12[i] : a12[6 + i], 8, 64);
#pragma unroll
  for (int i = 0; i < 3; ++i) a3[i] = (h2 ? a6[3 + i] : a6[i]) + __shfl_xor(h2 ? a6[i] : a6[3 + i], 4, 64);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    a3[i] += __shfl_xor(a3[i], 2, 64);
    a3[i] += __shfl_xor(a3[i], 1, 64);
  }
  const int j = lane & 3;
  *vi = j < 3 ? 24 * h5 + 12 * h4 + 6 * h3 + 3 * h2 + j : -1;
  return j == 0 ? a3[0] : j == 1 ? a3[1] : j == 2 ? a3[2] : 0.0;
}

// The keyframe blocks (P, y < nf) of both border rows of a camera: kpw WAVES per keyframe y (grid x: 4/kpw keyframes per
// workgroup; y: camera c) form the 8 × 6 live entries of (2c, y) and (2c + 1, y) — row 2c + 1's frame holds intrinsics 6,
// 7 and four pads — at once: a lane takes every (64·kpw)th entry of the keyframe's lists (its blocks and points seen by
// the camera), each wave adds its lanes' sums (wave_rs48) and the kpw waves' sums are added in order (a fixed order).
// kpw = 4 while the keyframe waves would not fill the SIMDs (C3, 200 keyframes), else 2 (C4: 2008 waves; 1 and 4 measured
// 80.5 and 82.4 against 76.5 µs).  Round 5 walked the lists twice (one kernel per border row: 133 + 117 µs at C4) and
// each point's blocks once per (point, list).
template <bool MOM>
__device__ __forceinline__ void border_keyframes(const IntrBorderArgs& a, double lambda, int kpw, int bx, int by) {
  __shared__ double2 s_w[4][48];
  lambda = lm_lambda(lm_view(a.lm), lambda);
  const int c = by, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int gw = bx * 4 + w, y0 = gw / kpw, sub = gw % kpw;
  const int y = min(y0, a.nf - 1);  // (a wave past the last keyframe walks nothing and stores nothing)
  const int L = c * (a.nf + a.nc) + y;
  const int q0 = sub * 64 + lane, dq = y0 < a.nf ? 64 * kpw : 1 << 30;
  // the 8 intrinsics rows d of camera c (border rows 2c: d = 0…5, 2c + 1: d = 6, 7) × the keyframe's 6 columns, value
  // v = 6d + cc; the direct terms first, then the Schur terms in the same registers; lane l ends with value vi (wave_rs48)
  double acc[8][6];
#pragma unroll
  for (int d = 0; d < 8; ++d)
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) acc[d][cc] = 0.0;
  // the next entry's list index is loaded during this one (a list walk was two dependent memory rounds per entry: the
  // index, then the row — and the host / target test on the block record before the row's Jacobian)
  const int qb = a.bptr[L + 1];
  int q = a.bptr[L] + (y0 < a.nf ? q0 : 1 << 30);
  int bn = q < qb ? a.blist[q] : 0;
  for (; q < qb; q += dq) {
    const int bf = bn;
    if (q + dq < qb) bn = a.blist[q + dq];
    const double* B = a.ib + (long long)(bf & 0x7fffffff) * kStrideOf<MOM>;
    if constexpr (MOM) {  // the block's J_iᵀJ_h / J_iᵀJ_t, formed by the producer
      const double* M = B + (bf < 0 ? kMomMh : kMomMt);
#pragma unroll
      for (int d = 0; d < 8; ++d)
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) acc[d][cc] += M[6 * d + cc];
    } else {
      const double* Jc = B + (bf < 0 ? kIbJh : kIbJt);
      double c0[6], c1[6];
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        c0[cc] = Jc[cc];
        c1[cc] = Jc[6 + cc];
      }
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const double j0 = B[kIbJi + d], j1 = B[kIbJi + 8 + d];
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) acc[d][cc] += j0 * c0[cc] + j1 * c1[cc];
      }
    }
  }
  int vi;
  double vd = wave_rs48(reinterpret_cast<const double(&)[48]>(acc), lane, &vi);
#pragma unroll
  for (int d = 0; d < 8; ++d)
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) acc[d][cc] = 0.0;
  const int qp = a.pptr[L + 1];
  q = a.pptr[L] + (y0 < a.nf ? q0 : 1 << 30);
  int gpn = q < qp ? a.plist[q] : 0, byn = q < qp ? a.pblk[q] : -1;
  for (; q < qp; q += dq) {
    const int gp = gpn, by = byn;
    if (q + dq < qp) {
      gpn = a.plist[q + dq];
      byn = a.pblk[q + dq];
    }
    double wc[8], wy[6];  // W of the point for camera c (Σ W_i over its blocks seen by c, intr_pw_kernel) and for
                          // keyframe y (Σ J_h / J_t ᵀJ_ρ over its blocks hosted / targeted by y)
    const double* pw = a.pw + (long long)gp * (8 * a.nc + 6);
#pragma unroll
    for (int d = 0; d < 8; ++d) wc[d] = pw[8 * c + d];
    if (by == -1) {  // y hosts the point: every block's J_hᵀJ_ρ (intr_pw_kernel)
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) wy[cc] = pw[8 * a.nc + cc];
    } else if (by >= 0) {  // y is a target: the point's block targeting it
      const double* B = a.ib + (long long)by * kStrideOf<MOM>;
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) {
        if constexpr (MOM) wy[cc] = 0.0 + B[kMomWt + cc];
        else wy[cc] = 0.0 + (B[kIbJt + cc] * B[kIbJr] + B[kIbJt + 6 + cc] * B[kIbJr + 1]);
      }
    } else {  // several blocks of the point target y: their sum, in block order
      const int4 pr = a.pt_rec[gp];
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) wy[cc] = 0.0;
      for (int b = pr.x; b < pr.x + pr.y; ++b) {
        if (a.ib_rec[b].w != y) continue;
        const double* B = a.ib + (long long)b * kStrideOf<MOM>;
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) {
          if constexpr (MOM) wy[cc] += B[kMomWt + cc];
          else wy[cc] += B[kIbJt + cc] * B[kIbJr] + B[kIbJt + 6 + cc] * B[kIbJr + 1];
        }
      }
    }
    const double inv = border_inv(a, gp, lambda);
#pragma unroll
    for (int d = 0; d < 8; ++d)
#pragma unroll
      for (int cc = 0; cc < 6; ++cc) acc[d][cc] += inv * wc[d] * wy[cc];
  }
  double vs = wave_rs48(reinterpret_cast<const double(&)[48]>(acc), lane, &vi);
  if (kpw > 1) {  // the keyframe's kpw waves, in order
    if (vi >= 0) s_w[w][vi] = make_double2(vd, vs);
    __syncthreads();
    if (sub == 0 && vi >= 0) {
      double2 t = s_w[w][vi];
      for (int k = 1; k < kpw; ++k) {
        t.x += s_w[w + k][vi].x;
        t.y += s_w[w + k][vi].y;
      }
      vd = t.x;
      vs = t.y;
    }
    if (sub != 0) return;  // (whole waves)
  }
  // row 2c: values 0 … 35 (element v); row 2c + 1: values 36 … 47 (d = 6, 7) as its elements 0 … 11, its elements
  // 12 … 35 pads (border_store) from lanes 12 … 35
  if (y0 < a.nf) {
    if (vi >= 0) border_store(a, lambda, vi < 36 ? 2 * c : 2 * c + 1, y * 36 + (vi < 36 ? vi : vi - 36), vd, vs);
    if (lane >= 12 && lane < 36) border_store(a, lambda, 2 * c + 1, y * 36 + lane, 0.0, 0.0);
  }
}

// The camera blocks (P = nf + 2c + h, y = nf + 2c2 + h2 ≥ nf, c2 ≤ c) and the gradient rows of the border, as two
// reductions over whole lists instead of one list walk per (border row, column block) — the list of a camera holds ALL
// of its blocks (400k at C4) and points (100k), and round 5 walked it six times per trial (two row kernels × three column
// blocks, 165 µs at C4 with the finishing kernel):
//   cam_dir — per camera c, over its blocks: Σ J_iᵀJ_i (the 8 × 8 upper triangle, 36) and Σ J_iᵀr (8): the
//     direct terms (a block's intrinsics Jacobian is its target camera's, so the direct part couples a camera only with
//     itself);
//   cam_sch — per camera pair (c, c2 ≤ c), over the points seen by both: Σ_p W_c W_c2ᵀ / H'_ρρ (8 × 8) and,
//     for c2 = c, Σ_p W_c g_ρ / H'_ρρ (8): the Schur terms (W_c from intr_pw_kernel);
// each over kCamSplit workgroups (a thread takes every (256·kCamSplit)th entry; wave butterflies, then the four waves in
// order), and intr_cam_fin_kernel adds the kCamSplit totals in order per element and stores it (border_store) — a fixed
// order end to end.
constexpr int kCamSplit = 128;  // (512 measured no faster at C4, 2.7× slower for two cameras' Schur sums at C3)
constexpr int kCamDir = 44, kCamSch = 72;  // accumulators per thread

__device__ __forceinline__ int upper8i(int i, int j) { return i * 8 - i * (i - 1) / 2 + (j - i); }  // i ≤ j < 8

// Σ over the wave of N per-lane values (N a multiple of 16) into dst[0 … N) by recursive halving, as wave_rs48: after the
// xor-32 / 16 / 8 / 4 steps lane l holds partial sums of values base(l) … base(l) + N/16 − 1 (base = N/2·b5 + N/4·b4 +
// N/8·b3 + N/16·b2), completed over its quad by xor 2 and xor 1; the quad's lanes store them.  A fixed order.
template <int N>
__device__ __forceinline__ void wave_rs_lds(const double (&v)[N], int lane, double* dst) {
  static_assert(N % 16 == 0, "four halvings");
  constexpr int H1 = N / 2, H2 = N / 4, H3 = N / 8, H4 = N / 16;
  double a1[H1], a2[H2], a3[H3], a4[H4];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
#pragma unroll
  for (int i = 0; i < H1; ++i) a1[i] = (h5 ? v[H1 + i] : v[i]) + __shfl_xor(h5 ? v[i] : v[H1 + i], 32, 64);
#pragma unroll
  for (int i = 0; i < H2; ++i) a2[i] = (h4 ? a1[H2 + i] : a1[i]) + __shfl_xor(h4 ? a1[i] : a1[H2 + i], 16, 64);
#pragma unroll
  for (int i = 0; i < H3; ++i) a3[i] = (h3 ? a2[H3 + i] : a2[i]) + __shfl_xor(h3 ? a2[i] : a2[H3 + i], 8, 64);
#pragma unroll
  for (int i = 0; i < H4; ++i) a4[i] = (h2 ? a3[H4 + i] : a3[i]) + __shfl_xor(h2 ? a3[i] : a3[H4 + i], 4, 64);
  const int base = H1 * h5 + H2 * h4 + H3 * h3 + H4 * h2;
#pragma unroll
  for (int i = 0; i < H4; ++i) {
    a4[i] += __shfl_xor(a4[i], 2, 64);
    a4[i] += __shfl_xor(a4[i], 1, 64);
    if ((i & 3) == (lane & 3)) dst[base + i] = a4[i];
  }
}
constexpr int pad16(int n) { return (n + 15) / 16 * 16; }

// Σ over the workgroup of NV per-thread accumulators in a fixed order → out[0 … NV): each wave's sums by wave_rs_lds
// into s_w (4·pad16(NV) doubles), then the four waves in order.  Every thread calls it.
template <int NV>
__device__ __forceinline__ void wg_sum_store(const double* acc, double* s_w, double* out) {
  constexpr int NP = pad16(NV);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double v[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) v[i] = i < NV ? acc[i] : 0.0;
  wave_rs_lds<NP>(v, lane, s_w + w * NP);
  __syncthreads();
  for (int i = threadIdx.x; i < NV; i += blockDim.x) out[i] = ((s_w[i] + s_w[NP + i]) + s_w[2 * NP + i]) + s_w[3 * NP + i];
}

template <bool MOM>
__device__ __forceinline__ void cam_dir(const IntrBorderArgs& a, double* part, int bx, int by) {
  __shared__ double s_w[4 * pad16(kCamDir)];
  const int c = by, L = c * (a.nf + a.nc) + a.nf + c;  // (camera c, unit nf + c): every block of camera c
  double acc[kCamDir];
#pragma unroll
  for (int v = 0; v < kCamDir; ++v) acc[v] = 0.0;
  const int qe = a.bptr[L + 1];
  int q = a.bptr[L] + threadIdx.x + 256 * bx;
  int bn = q < qe ? a.blist[q] : 0;  // (the next entry's index loaded during this one)
  for (; q < qe; q += 256 * kCamSplit) {
    const double* B = a.ib + (long long)bn * kStrideOf<MOM>;
    if (q + 256 * kCamSplit < qe) bn = a.blist[q + 256 * kCamSplit];
    if constexpr (MOM) {  // the block's J_iᵀJ_i triangle and J_iᵀr, in cam_dir's accumulator order
      static_assert(kMomJr == kMomTri + 36, "triangle then J_iᵀr: contiguous as the accumulators");
#pragma unroll
      for (int v = 0; v < kCamDir; ++v) acc[v] += B[kMomTri + v];
      continue;
    }
    double j0[8], j1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      j0[k] = B[kIbJi + k];
      j1[k] = B[kIbJi + 8 + k];
    }
    const double r0 = B[kIbR], r1 = B[kIbR + 1];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int j = i; j < 8; ++j) acc[upper8i(i, j)] += j0[i] * j0[j] + j1[i] * j1[j];
      acc[36 + i] += j0[i] * r0 + j1[i] * r1;
    }
  }
  wg_sum_store<kCamDir>(acc, s_w, part + ((long long)c * kCamSplit + bx) * kCamDir);
}

__device__ __forceinline__ void cam_sch(const IntrBorderArgs& a, double lambda, double* part, int bx, int by) {
  __shared__ double s_w[4 * pad16(kCamSch)];
  lambda = lm_lambda(lm_view(a.lm), lambda);
  const int pc = by;  // camera pair (c, c2 ≤ c), pc = c(c+1)/2 + c2
  int c = 0;
  while ((c + 1) * (c + 2) / 2 <= pc) ++c;
  const int c2 = pc - c * (c + 1) / 2, L = c * (a.nf + a.nc) + a.nf + c2;  // points seen by c and c2
  const int st = 8 * a.nc + 6;
  double acc[kCamSch];
#pragma unroll
  for (int v = 0; v < kCamSch; ++v) acc[v] = 0.0;
  for (int q = a.pptr[L] + threadIdx.x + 256 * bx; q < a.pptr[L + 1]; q += 256 * kCamSplit) {
    const int gp = a.plist[q];
    const double* pw = a.pw + (long long)gp * st;
    const double inv = border_inv(a, gp, lambda), gr = a.pt_data[(long long)gp * 8 + 1];
    double wc[8], w2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      wc[k] = pw[8 * c + k];
      w2[k] = pw[8 * c2 + k];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double iw = inv * wc[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[8 * i + j] += iw * w2[j];
      acc[64 + i] += iw * gr;
    }
  }
  wg_sum_store<kCamSch>(acc, s_w, part + ((long long)pc * kCamSplit + bx) * kCamSch);
}

template <bool MOM>
__global__ __launch_bounds__(256) void intr_border_kernel(const IntrBorderArgs a, double lambda, int kpw) {
  border_keyframes<MOM>(a, lambda, kpw, blockIdx.x, blockIdx.y);
}
template <bool MOM>
__global__ __launch_bounds__(256) void intr_cam_dir_kernel(const IntrBorderArgs a, double* part) {
  cam_dir<MOM>(a, part, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void intr_cam_sch_kernel(const IntrBorderArgs a, double lambda, double* part) {
  cam_sch(a, lambda, part, blockIdx.x, blockIdx.y);
}
// The three border reductions are independent (they read the rows, the points' sums and the lists, and write
// different outputs): while the keyframe part is small (nf·nc < 512 keyframe blocks, the 4-waves-per-keyframe regime:
// C3), one launch runs them side by side — workgroups [0, nk) the keyframe blocks (nk_x per camera), then kCamSplit per
// camera of direct sums, then kCamSplit per camera pair of Schur sums — instead of three launches in sequence, each a
// fraction of the chip (C3: 35.3 → 24.6 µs, two cameras 41.3 → 31.1; at C4, where the keyframe part alone fills the
// chip, side by side measured 108 against 102 µs in sequence).
template <bool MOM>
__global__ __launch_bounds__(256) void intr_border_all_kernel(const IntrBorderArgs a, double lambda, int kpw, int nk_x,
                                                             double* dpart, double* spart) {
  int b = blockIdx.x;
  const int nk = nk_x * a.nc, nd = kCamSplit * a.nc;
  if (b < nk) {
    border_keyframes<MOM>(a, lambda, kpw, b % nk_x, b / nk_x);
    return;
  }
  b -= nk;
  if (b < nd) {
    cam_dir<MOM>(a, dpart, b % kCamSplit, b / kCamSplit);
    return;
  }
  b -= nd;
  cam_sch(a, lambda, spart, b % kCamSplit, b / kCamSplit);
}

// One WAVE per (border row, camera column block yb ≤ row, entry e) and per border gradient element: lane l adds totals l,
// l + 64, … of the kCamSplit in order, the wave's lanes by xor butterflies (a fixed order); then border_store.
__device__ __forceinline__ void cam_fin(const IntrBorderArgs& a, double lambda, const double* dpart, const double* spart,
                                        int blk) {
  lambda = lm_lambda(lm_view(a.lm), lambda);
  const int nb = 2 * a.nc + 1, i = blk * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= 2 * a.nc * nb * 36) return;
  const int e = i % 36, yb = (i / 36) % nb, row = i / (36 * nb);
  const bool grad = yb == 2 * a.nc;
  if (grad ? (e % 6 != 0) : (yb > row)) return;  // (the upper camera blocks are not stored; whole waves)
  const int c = row >> 1, h = row & 1, r = e / 6, cc = e % 6, d = 6 * h + r;
  auto sum = [&](const double* p, int stride, int idx) {
    double v = 0.0;
    for (int s = lane; s < kCamSplit; s += 64) v += p[(long long)s * stride + idx];
    return wave_sum(v);
  };
  double dir = 0.0, sch = 0.0;
  if (grad) {
    if (d < 8) {
      dir = sum(dpart + (long long)c * kCamSplit * kCamDir, kCamDir, 36 + d);
      sch = sum(spart + (long long)(c * (c + 1) / 2 + c) * kCamSplit * kCamSch, kCamSch, 64 + d);
    }
    if (lane == 0) border_store(a, lambda, row, (a.nf + 2 * a.nc) * 36 + r, dir, sch);
    return;
  }
  const int c2 = yb >> 1, d2 = 6 * (yb & 1) + cc;
  if (d < 8 && d2 < 8) {  // (pads: border_store's identity rows)
    if (c2 == c) dir = sum(dpart + (long long)c * kCamSplit * kCamDir, kCamDir, upper8i(min(d, d2), max(d, d2)));
    sch = sum(spart + (long long)(c * (c + 1) / 2 + c2) * kCamSplit * kCamSch, kCamSch, 8 * d + d2);
  }
  if (lane == 0) border_store(a, lambda, row, (a.nf + yb) * 36 + e, dir, sch);
}
__global__ __launch_bounds__(256) void intr_cam_fin_kernel(const IntrBorderArgs a, double lambda, const double* dpart,
                                                          const double* spart) {
  cam_fin(a, lambda, dpart, spart, blockIdx.x);
}
// The same, with the arrow solve's level 0 (arrow_build) in workgroups fin_blocks … of the same launch: it reads the
// keyframe band and g (assemble_kernel) and the border rows' keyframe blocks (border_keyframes), nothing this launch
// writes — one launch fewer per trial.
__global__ __launch_bounds__(256) void intr_cam_fin_build_kernel(const IntrBorderArgs a, double lambda,
                                                                const double* dpart, const double* spart,
                                                                const ArrowArgs aa, int batches, int fin_blocks) {
  if ((int)blockIdx.x < fin_blocks) cam_fin(a, lambda, dpart, spart, blockIdx.x);
  else arrow_build(aa, batches, (long long)(blockIdx.x - fin_blocks) * blockDim.x + threadIdx.x);
}

// The candidate intrinsics become the state (after an accepted trial; lm == nullptr: always), fp64 records and fp32 copy.
__global__ void intr_accept_kernel(const double* __restrict__ lm, const double* __restrict__ knew_d,
                                   const float* __restrict__ knew_f, double* __restrict__ k_d, float* __restrict__ k_f,
                                   int nc) {
  if (lm && (lm[kLmAccept] == 0.0 || lm[kLmDone] != 0.0)) return;
  const int i = threadIdx.x, c = i >> 3, d = i & 7;
  if (c >= nc) return;
  k_d[kCamD * c + d] = knew_d[kCamD * c + d];
  k_f[8 * c + d] = knew_f[8 * c + d];
}

}  // namespace

namespace pba {
namespace detail {

int intr_prepare_buffers(pba_engine* e) {
  GnData& G = e->gn;
  const int nb = e->n_blocks, ngp = G.n_gn_points, nc = G.nc_sys;
  hipStream_t st0 = e->stream;
  // per GN block: the two weighted rows (geometric), or the moment record of its P rows (photometric)
  const bool mom = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC;
  PBA_HIP(G.ib_data.resize((size_t)nb * (mom ? kMomStride : kIbStride)));
  PBA_HIP(G.ib_pw.resize((size_t)std::max(ngp, 1) * (8 * nc + 6)));
  PBA_HIP(G.ib_part.resize((size_t)kCamSplit * (nc * kCamDir + nc * (nc + 1) / 2 * kCamSch)));
  PBA_HIP(G.intr_new_d.resize((size_t)kCamD * nc));
  PBA_HIP(G.intr_new_f.resize((size_t)8 * nc));
  // the candidate records start as the state's (their unprojection half is never read: hosts unproject with the cameras)
  PBA_HIP(hipMemcpyAsync(G.intr_new_d.p, e->intr_state_d.p, sizeof(double) * kCamD * nc, hipMemcpyDeviceToDevice, st0));
  PBA_HIP(hipMemcpyAsync(G.intr_new_f.p, e->intr_state.p, sizeof(float) * 8 * nc, hipMemcpyDeviceToDevice, st0));
  return PBA_OK;
}

void launch_intr_accept(pba_engine* e, const double* lm) {
  GnData& G = e->gn;
  intr_accept_kernel<<<1, 256, 0, e->stream>>>(lm, G.intr_new_d.p, G.intr_new_f.p, e->intr_state_d.p, e->intr_state.p,
                                               G.nc_sys);
}

// The photometric producer runs at the engine's state: the state's poses and inverse distances, the intrinsics state for
// the target projection (make_kernel_args), the active level's images.
void enqueue_intr_rows(pba_engine* e, const double* lm, bool accept) {
  GnData& G = e->gn;
  if (lm && accept) launch_intr_accept(e, lm);
  if (e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC) {
    KernelArgs ka = make_kernel_args(e, nullptr, e->rho.p);
    ka.poses = e->poses.p;
    const IntrMomArgs ma{G.ib_rec.p, G.ib_data.p, e->n_blocks, lm ? lm : G.lm_idle.p};
    dispatch_pm(e, [&](auto pm) {
      intr_rows_photometric_kernel<decltype(pm)::value><<<(ma.n + 31) / 32, 256, 0, e->stream>>>(ka, ma);
    });
    return;
  }
  IntrRowsArgs ra{G.ib_rec.p, e->poses.p, e->rho.p, e->u_ref.p, e->u_obs.p, e->frame_cam.p, e->intr_d.p,
                  e->intr_state_d.p, (double)e->opt.huber_width, G.ib_data.p, e->n_blocks, lm ? lm : G.lm_idle.p};
  int grid = (e->n_blocks + 255) / 256;
  if (G.ir_waves > 0) {  // point-aligned waves: the points' W sums too (no intr_pw_kernel)
    ra.wave_tab = G.ir_wave.p;
    ra.n_waves = G.ir_waves;
    ra.pw = G.ib_pw.p;
    ra.nc = G.nc_sys;
    grid = (G.ir_waves + 3) / 4;
  }
  switch (e->opt.camera_model) {
    case PBA_CAMERA_PINHOLE: intr_rows_kernel<CAM_PINHOLE><<<grid, 256, 0, e->stream>>>(ra); break;
    case PBA_CAMERA_DOUBLE_SPHERE: intr_rows_kernel<CAM_DS><<<grid, 256, 0, e->stream>>>(ra); break;
    case PBA_CAMERA_EUCM: intr_rows_kernel<CAM_EUCM><<<grid, 256, 0, e->stream>>>(ra); break;
    default: intr_rows_kernel<CAM_KB4><<<grid, 256, 0, e->stream>>>(ra); break;
  }
}

template <bool MOM>
static void launch_border(pba_engine* e, const IntrBorderArgs& ba, double lambda, bool fused, int kpw, int nk_x, int ncp,
                          double* dpart, double* spart) {
  const GnData& G = e->gn;
  if (G.ir_waves == 0)  // (else intr_rows_kernel has formed them)
    intr_pw_kernel<MOM><<<(8 * G.n_gn_points + 255) / 256, 256, 0, e->stream>>>(ba, G.n_gn_points);
  if (fused) {
    const int n_wg = nk_x * G.nc_sys + kCamSplit * (G.nc_sys + ncp);
    intr_border_all_kernel<MOM><<<n_wg, 256, 0, e->stream>>>(ba, lambda, kpw, nk_x, dpart, spart);
  } else {
    intr_border_kernel<MOM><<<dim3(nk_x, G.nc_sys), 256, 0, e->stream>>>(ba, lambda, kpw);
    intr_cam_dir_kernel<MOM><<<dim3(kCamSplit, G.nc_sys), 256, 0, e->stream>>>(ba, dpart);
    intr_cam_sch_kernel<<<dim3(kCamSplit, ncp), 256, 0, e->stream>>>(ba, lambda, spart);
  }
}

void enqueue_border(pba_engine* e, double lambda, const double* lm, double* X, bool arrow) {
  GnData& G = e->gn;
  const int nf = e->n_frames, nfs = G.nfs;
  IntrBorderArgs ba{G.ib_data.p, G.ib_rec.p, G.ib_cam.p, G.pt_rec.p, G.pt_data.p, G.ib_bptr.p, G.ib_blist.p,
                    G.ib_pptr.p, G.ib_plist.p, G.sky_first.p, G.sky_row.p, G.fixed.p, lm ? lm : G.lm_idle.p, G.S.p,
                    G.g.p, G.g_dir.p, G.Ddiag.p, nf, G.nc_sys, X, (long long)nfs * 36 + EX_TAIL, G.ib_pw.p, G.ib_pblk.p};
  const int nb = 2 * G.nc_sys + 1;
#ifndef PBA_INTR_KPW_BIG
#define PBA_INTR_KPW_BIG 2
#endif
  bool fused = nf * G.nc_sys < 512;  // one launch (below) while the keyframe part is small, else three
  if (const char* tb = test_hook("PBA_TEST_BORDER")) {  // (tests: "fused" / "split" whatever the size)
    if (!std::strcmp(tb, "fused")) fused = true;
    else if (!std::strcmp(tb, "split")) fused = false;
  }
  const int kpw = fused ? 4 : PBA_INTR_KPW_BIG;  // waves per keyframe block (border_keyframes)
  double* dpart = G.ib_part.p;
  double* spart = dpart + (size_t)G.nc_sys * kCamSplit * kCamDir;
  const int nk_x = (nf * kpw + 3) / 4, ncp = G.nc_sys * (G.nc_sys + 1) / 2;
  // the blocks as the producer left them: two weighted rows (geometric) or moment records (photometric)
  if (e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC) launch_border<true>(e, ba, lambda, fused, kpw, nk_x, ncp, dpart, spart);
  else launch_border<false>(e, ba, lambda, fused, kpw, nk_x, ncp, dpart, spart);
  const int fin_blocks = (2 * G.nc_sys * nb * 36 + 3) / 4;
  if (arrow) {
    const ArrowArgs aa = arrow_args(e, G.S.p, G.sky_first.p, G.sky_row.p, G.fixed.p);
    const int build_blocks = (int)((arrow_build_threads(G) + 255) / 256);
    intr_cam_fin_build_kernel<<<fin_blocks + build_blocks, 256, 0, e->stream>>>(ba, lambda, dpart, spart, aa,
                                                                               G.ar_batches, fin_blocks);
  } else {
    intr_cam_fin_kernel<<<fin_blocks, 256, 0, e->stream>>>(ba, lambda, dpart, spart);
  }
}

}  // namespace detail
}  // namespace pba
