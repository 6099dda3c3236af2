// pba_evaluate.hip — the evaluation path of the photometric BA residual/Jacobian engine: the block kernels, the record
// decode and their launches (the C ABI that calls them is pba_engine.hip).
//
// Replaces, for every residual block of a problem at once, the reference's per-block CPU evaluation:
//   ProgramEvaluator::Evaluate ParallelFor (program_evaluator.h:187-258) →
//   ResidualBlock::Evaluate (residual_block.cc:69-158) → AutoDiffCostFunction<Functor,…> →
//   BundleAdjustmentReprojectionCostFunctor (reprojection.h:83-112) / PhotometricError (photometric_error.h:139-182)
//
// Photometric evaluation is ONE launch (photometric_block_kernel): one lane per (block, pattern pixel), a wave =
// 64/LPB blocks.  Each block's lanes form its relative pose T_th = T_w_t⁻¹ T_w_h in fp64 from the state poses in
// the tile prologue (fused state, pba_internal.h:stage_tile) — or copy it from the pair table (pair_kernel /
// state_kernel in pba_engine.hip: the geometric kernels and the Gauss-Newton path) — with u_ref and ρ into LDS; image
// taps are gathered from the target keyframe's tiled u8 image, the Jacobian chain stays in registers, per-block ‖r‖²
// and validity come from wave shuffles, and the workgroup's records (pba_record.h) leave as one contiguous slab.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "pba_internal.h"
#include "pba_record.h"

using namespace pba;
using namespace pba::detail;

namespace {

// PBA_EVAL_STAMPS (a variant built with tools/build_variant.sh, never the product or the test library): wave 0 of every
// workgroup of the 8-lane record kernel takes 100-MHz stamps along its chain of loads and barriers — kept in scalar
// registers and stored behind the slab, so that a stamp's store is not in the vector-memory counter a later stamp
// waits for.  "Arrived" stamps wait for every outstanding load first, which the unstamped kernel does only where it
// needs a value: the stamped variant times the chain's links, not the product kernel.  tools/probe/block_chain_stamps.py.
#ifdef PBA_EVAL_STAMPS
// entry | block_rec | prologue loads | barrier 1 | I_h | row | stage may begin | staged | stored
constexpr int kEvalStamps = 9;
__device__ long long* g_eval_stamps = nullptr;  // 16 per workgroup, at blockIdx.x
#define PBA_STAMP(i, wait_loads)                                        \
  do {                                                                  \
    if (wait_loads) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    \
    __builtin_amdgcn_sched_barrier(0);                                  \
    stamps[i] = wall_clock64();                                         \
    __builtin_amdgcn_sched_barrier(0);                                  \
  } while (0)
#else
#define PBA_STAMP(i, wait_loads) \
  do {                           \
  } while (0)
#endif

// PM = camera model + 4 · interpolator; T = float, _Float16, ScaledF16, IntrF32, AffineF32 or IntrAffineF32 (RecFormat;
// the last stages 32·26·8·4 = 26,624 B)
template <int PM, int LPB, int MODE, class T>
__global__ __launch_bounds__(kBlockThreads) void photometric_block_kernel(const KernelArgs a) {
  constexpr int BPW = kBlockThreads / LPB;  // blocks per workgroup
  constexpr bool JAC = MODE == 1;
  using S = typename RecFormat<T>::S;  // the stored type
  constexpr int kCols = RecFormat<T>::kCols;
  // one LDS region per wave: its 8 tile blocks, then over the same bytes its 8 staged records (pba_wave_slab.h)
  static_assert(LPB == kSlabMaxPattern && BPW == kSlabWaves * kSlabWaveBlocks && sizeof(TileBlock) == kSlabTileBytes,
                "pba_wave_slab.h: 4 waves of 8 blocks, 8 lanes each");
  static_assert(slab_format_known(kCols, (int)sizeof(S)), "pba_wave_slab.h: kSlabFormats has no entry for this format");
  constexpr int kRegion = wave_region_bytes(kCols, (int)sizeof(S), JAC);
  __shared__ __attribute__((aligned(16))) unsigned char lds[wg_lds_bytes(kCols, (int)sizeof(S), JAC)];
  auto tile_at = [&](int b) { return reinterpret_cast<TileBlock*>(lds + tile_block_offset(b, kRegion)); };
  // the wave's own region from a scalar register (the wave index is uniform): a lane's tile block and staged record
  // then hang off one per-lane value, its block's index in the wave, as they hung off lb before the regions
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  unsigned char* const region = lds + wave_region_offset(w, kRegion);
  const int P = a.P;
  const int rec_f = kCols * P;
  const int blk0 = logical_tile() * BPW;
  const int wb = (threadIdx.x / LPB) % kSlabWaveBlocks;  // the block's index in its wave
  const int lb = w * kSlabWaveBlocks + wb;               // and in the tile
  const int k = threadIdx.x % LPB;
  const int blk = blk0 + lb;
  const bool live = blk < a.n_blocks;  // a block's LPB lanes agree
  const bool act = live && k < P;
  TileBlock* const own_tile = reinterpret_cast<TileBlock*>(region + wb * kSlabTileBytes);  // = tile_at(lb)
  S* out = reinterpret_cast<S*>(a.out);  // records in the engine's format (fp32, or halves: PBA_RECORD_F16 / _SCALED)

#ifdef PBA_EVAL_STAMPS
  long long stamps[kEvalStamps] = {};
#endif
  PBA_STAMP(0, false);
  const float2 off = pattern_at<LPB>(a, k);
  adopt_state(a);
  int pt;
  float Ih;
  auto host_intensity = [&]() { return act ? a.host_int[(long long)pt * P + k] : 0.0f; };
  if (LPB == 8 && a.poses) {  // fused state: the workgroup-cooperative prologue (BPW = 32)
    static_assert(kBlockThreads == 256, "stage_tile_wg: 4 waves, 32 blocks");
    // lane b (and b + 32) of every wave loads tile block b's record for the prologue: the lane's own point comes
    // from it by a lane move, not from a second load.  I_h needs only the point: issued before the prologue's loads,
    // it is in flight with them (a cold line, like u_ref) and the prologue's own wait covers it — the vector-memory
    // counter retires in order
    const int4 br = tile_block_rec(a, blk0);
#ifdef PBA_EVAL_STAMPS
    asm volatile("" ::"v"(br.x));
    PBA_STAMP(1, true);
#endif
    pt = __shfl(br.x, lb, 64);
    Ih = host_intensity();
    stage_tile_wg(a, tile_at, br);
  } else {
    pt = stage_tile<LPB>(a, own_tile, 0, k, blk, live);
    Ih = host_intensity();
  }
  constexpr bool AFF = RecFormat<T>::kAffine;
  Affine af = {1.0f, 0.0f, 0.0f};
  if constexpr (AFF) af = block_affine(a, live ? blk : a.n_blocks - 1);
  PBA_STAMP(2, true);
  __syncthreads();
  PBA_STAMP(3, false);
#ifdef PBA_EVAL_STAMPS
  asm volatile("" ::"v"(Ih));
  PBA_STAMP(4, true);
#endif
  constexpr bool INTR = JAC && RecFormat<T>::kIntr;
  constexpr bool PFIN = RecFormat<T>::kIntr && AFF;  // the 26-column records: a non-finite projection is invalid
  float ji[8];
  // dead lanes evaluate a staged block, masked by act
  const Row row =
      photometric_row<PM, JAC, TileBlock, false, INTR, AFF, PFIN>(a, *own_tile, off, Ih, nullptr, ji, &af);
  // per-block validity (ballot over the wave: the block's LPB lanes are an aligned bit field) and ‖r‖²
  const int ok = group_all<LPB>(act ? row.ok : 1);
  const float s = group_sum<LPB>(act ? row.r * row.r : 0.0f);
  const float bc = ok ? huber_cost(s, a.huber) : 0.0f;
#ifdef PBA_EVAL_STAMPS
  asm volatile("" ::"v"(bc));
  PBA_STAMP(5, false);
#endif
  if (live && k == 0) {
    a.valid[blk] = (uint8_t)ok;
    a.cost[blk] = bc;
  }
  if (MODE == 2) {
    if (a.wg_red) {
      const bool one = live && k == 0;
      wg_reduce2(one ? (double)bc : 0.0, one && ok ? 1.0 : 0.0, a.wg_red + 2 * logical_tile());
    }
    return;
  }
  if (!JAC) {
    if (act) {
      out[(long long)blk * rec_f + k] = rec_val<S>(ok ? row.r : 0.0f);
      if (a.res_out) a.res_out[(long long)blk * P + k] = ok ? row.r : 0.0f;  // contiguous: one D2H copy for Ceres
    }
    return;
  }
  // the record stage overwrites the wave's own tile blocks, which only its lanes read (one wave's LDS operations
  // stay in order): no barrier.  The tile was read as TileBlock, the stage is written as S: the compiler must not
  // move the stores above the reads
  asm volatile("" ::: "memory");
  PBA_STAMP(6, false);
  // stage the record row of pixel k (pba_record.h), zeros for invalid blocks.  The form of these stores is pinned: the
  // rows' fp32 arithmetic contracts differently around other stores, which changes record bytes
  S* s_rec = reinterpret_cast<S*>(region + wb * rec_f * (int)sizeof(S));  // lds + staged_record_offset(lb, …)
  if constexpr (RecFormat<T>::kScaled) {
    stage_row_scaled(s_rec, lb, P, k, row, act && ok);
    if (act && !ok) {
      s_rec[k] = s_rec[col_jrho(P) + k] = s_rec[col_tail(P) + k] = (S)0.0f;
      for (int j = 0; j < 6; ++j) s_rec[col_jhost(P) + 6 * k + j] = s_rec[col_jtarget(P) + 6 * k + j] = (S)0.0f;
    }
  } else if (act) {
    if (ok) {
      stage_row_each<S>(s_rec, P, k, row);
    } else {
      S* h = s_rec + col_jhost(P) + 6 * k;
      S* t = s_rec + col_jtarget(P) + 6 * k;
      s_rec[k] = (S)0.0f;
      for (int j = 0; j < 6; ++j) h[j] = t[j] = (S)0.0f;
      s_rec[col_jrho(P) + k] = (S)0.0f;
    }
    if constexpr (INTR) {
      if (!ok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ji[j] = 0.0f;
      }
      stage_intr(s_rec, P, k, ji);
    }
    if constexpr (AFF) stage_affine<RecFormat<T>::kIntr>(s_rec, P, k, af.E * (Ih - af.bh), af.E, ok != 0);
  }
  // each wave stores its own run of records (contiguous in LDS and in the record array) once its lanes have staged
  // them: no barrier, a wave does not wait for another wave's taps
  asm volatile("" ::: "memory");
  PBA_STAMP(7, false);
  const int nblk = min(BPW, a.n_blocks - blk0);
  if (nblk <= 0) return;
  const WaveStore ws = wave_store_range(w, nblk, rec_f * (int)sizeof(S));
  store_slab<S, 64>(region, reinterpret_cast<unsigned char*>(out + (long long)blk0 * rec_f) + ws.begin,
                    ws.bytes, a.slab_wt, threadIdx.x % 64);
#ifdef PBA_EVAL_STAMPS
  PBA_STAMP(8, true);
  if (threadIdx.x == 0 && g_eval_stamps)
    for (int i = 0; i < kEvalStamps; ++i) g_eval_stamps[16LL * blockIdx.x + i] = stamps[i];
#endif
}

// Patterns of 9…32 pixels (the 21-px pattern of config C5): still 8 lanes per block, each lane evaluating pixels
// k, k+8, … (PPL of them), so a wave carries 8 blocks and the per-block prologue (pair record, point) is paid once
// per 8 blocks — one lane per pixel (32 lanes per block) ran the 21-px C4 shard at 181 µs per launch with a third
// of its lanes idle and the prologue amortised over 2 blocks per wave.  Rows go to the record stage as they are
// produced (stage and tile in separate LDS regions); an invalid block's record is zeroed once its validity is known
// (the same lanes rewrite their own rows: LDS operations of one wave stay in order).  256 threads per workgroup,
// 128 when the fp32 stage of 32 blocks would not fit the 64 KiB of static LDS.
__host__ __device__ constexpr int multi_stage_bytes(int bpw, int P, int tsize, int cols = 14) {
  return (bpw * cols * P * tsize + 15) & ~15;
}

template <int PPL, class T>
constexpr int kMultiThreads = 32 * RecFormat<T>::kCols * 8 * PPL * (int)sizeof(typename RecFormat<T>::S) +
                                          32 * (int)sizeof(TileBlock) > 60 * 1024 ? 128 : 256;

// CT: the camera-table form (fused state, ≤ kCamTab cameras, 256 threads): compact 192-B tile blocks plus one LDS
// CamRec per camera instead of 352-B tile blocks carrying both cameras (the 21-px fp16 launch: 30.1 → 25.6 KB of LDS
// per workgroup, 5 → 6 workgroups per CU, which its 78 VGPRs also allow).
// C1 (with CT, one camera): the rows take the camera constants from scalar loads of the engine's camera record instead
// of the LDS table (no per-row LDS reads of them, no VGPRs).
// kMultiWaves: the waves per SIMD the camera-table form is compiled for.  6, except the scaled-half records of 9–16 and
// 25–32 px: held to 80 VGPRs those spilled 8–28 B per lane, and six workgroups are out of reach of the 25–32-px stage
// anyway (15 halves per row: 30.7 KB of stage per workgroup, 4 per CU).
// The 22-column records (IntrF32; the camera-table form serves their 9–16 px): 45 KB of stage per workgroup at 16 px,
// 3 workgroups per CU, so 3 waves per SIMD is all the LDS allows and the rows keep their registers.
// The 18-column records (AffineF32) likewise: 37 KB of stage + 6 KB of tile at 16 px, 3 workgroups per CU; their
// 17–32 px run 128 threads (kMultiThreads) and never take the camera-table form.
// KB4 with affine brightness: held to 168 VGPRs its rows spilled 24–128 B per lane (the table-free form takes 182–198),
// so that camera-table form is compiled for 2 waves per SIMD.
// The 26-column records (IntrAffineF32) never take the camera-table form: 26,624·PPL B of stage for 32 blocks plus their
// tile blocks is past 60 KiB at every PPL ≥ 2, so kMultiThreads gives them 128 threads (16·104·P + 16·352 B of dynamic
// LDS: 58,880 B at 32 px).
template <int PPL, class T>
constexpr int kMultiWaves =
    RecFormat<T>::kIntr || RecFormat<T>::kAffine ? 3 : (RecFormat<T>::kScaled && PPL != 3 ? 5 : 6);
template <int PM, int PPL, class T>
constexpr int kMultiWavesPM = RecFormat<T>::kAffine && cam_of(PM) == CAM_KB4 ? 2 : kMultiWaves<PPL, T>;

template <int PM, int MODE, class T, int PPL, bool CT = false, bool C1 = false>
__global__ __launch_bounds__((kMultiThreads<PPL, T>))
__attribute__((amdgpu_waves_per_eu(CT ? (kMultiWavesPM<PM, PPL, T>) : 1, 8)))
void photometric_block_kernel_multi(const KernelArgs a) {
  constexpr int LPB = 8, NTH = kMultiThreads<PPL, T>, BPW = NTH / LPB;
  constexpr bool JAC = MODE == 1;
  static_assert(!CT || NTH == 256, "camera table: the workgroup-cooperative prologue");
  using TB = typename std::conditional<CT, TileBlockC, TileBlock>::type;
  // dynamic LDS sized for the actual P (multi_stage_bytes): the 21-px fp16 stage is 18.4 KB instead of 21 KB for
  // 24 px, which lets a fifth workgroup onto the CU (LDS is what bounds this kernel's occupancy)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ float2 s_pat[LPB * PPL];
  __shared__ CamRec s_cam[CT ? kCamTab : 1];
  using S = typename RecFormat<T>::S;  // the stored type
  constexpr int kCols = RecFormat<T>::kCols;
  const int P = a.P;
  S* stage = reinterpret_cast<S*>(lds);
  TB* s_tb = reinterpret_cast<TB*>(lds + (JAC ? multi_stage_bytes(BPW, P, (int)sizeof(S), kCols) : 0));
  const int rec_f = kCols * P;
  const int blk0 = logical_tile() * BPW;
  const int lb = threadIdx.x / LPB;
  const int k = threadIdx.x % LPB;
  const int blk = blk0 + lb;
  const bool live = blk < a.n_blocks;  // a block's LPB lanes agree
  S* out = reinterpret_cast<S*>(a.out);

  if ((int)threadIdx.x < LPB * PPL) s_pat[threadIdx.x] = pattern_at<LPB * PPL>(a, threadIdx.x);
  adopt_state(a);
  int pt;
  if constexpr (CT) {
    pt = a.block_rec[live ? blk : a.n_blocks - 1].x;
    stage_tile_wg_ct(a, s_tb, s_cam, a.n_cams, blk0);
  } else if (NTH == 256 && a.poses) {  // fused state: the workgroup-cooperative prologue (BPW = 32)
    pt = a.block_rec[live ? blk : a.n_blocks - 1].x;
    stage_tile_wg(a, s_tb, blk0);
  } else {
    pt = stage_tile<LPB>(a, s_tb, lb, k, blk, live);
  }
  float Ih[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int px = k + LPB * j;
    Ih[j] = live && px < P ? a.host_int[(long long)pt * P + px] : 0.0f;
  }
  constexpr bool AFF = RecFormat<T>::kAffine;
  Affine af = {1.0f, 0.0f, 0.0f};
  if constexpr (AFF) af = block_affine(a, live ? blk : a.n_blocks - 1);
  __syncthreads();
  S* s_rec = stage + lb * rec_f;
  int okl = 1;
  float s = 0.0f, rr[PPL];
  auto pixel = [&](int j, float ih) {
    const int px = k + LPB * j;
    const bool act = live && px < P;
    constexpr bool INTR = JAC && RecFormat<T>::kIntr;
    constexpr bool PFIN = RecFormat<T>::kIntr && AFF;  // the 26-column records: a non-finite projection is invalid
    float ji[8];
    const Row row =  // masked by act
        photometric_row<PM, JAC, TB, C1, INTR, AFF, PFIN>(a, s_tb[lb], s_pat[px < P ? px : 0], ih, s_cam, ji, &af);
    okl &= act ? row.ok : 1;
    s += act ? row.r * row.r : 0.0f;
    if constexpr (JAC && RecFormat<T>::kScaled) stage_row_scaled(s_rec, lb, P, px, row, act);
    else if constexpr (JAC) stage_row<S>(s_rec, P, px, row, act);
    if constexpr (INTR) {
      if (act) stage_intr(s_rec, P, px, ji);
    }
    if constexpr (JAC && AFF) {
      if (act) stage_affine<RecFormat<T>::kIntr>(s_rec, P, px, af.E * (ih - af.bh), af.E, true);
    }
    return row.r;
  };
  if constexpr (JAC) {
    // one pixel at a time (no unrolling: an unrolled loop interleaves the PPL rows' evaluations and needed 122 VGPRs,
    // 4 waves per SIMD); the pixel's I_h,k selected from the registers by a compare chain
#pragma unroll 1
    for (int j = 0; j < PPL; ++j) {
      float ih = Ih[0];
#pragma unroll
      for (int q = 1; q < PPL; ++q) ih = j == q ? Ih[q] : ih;
      // the tile block (pair record, cameras, point: ~70 registers) is read from LDS again by every pixel instead of
      // being hoisted out of the loop and kept live across it
      asm volatile("" ::: "memory");
      pixel(j, ih);
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPL; ++j) rr[j] = pixel(j, Ih[j]);
  }
  // per-block validity (ballot over the wave: the block's LPB lanes are an aligned bit field) and ‖r‖²
  const int ok = group_all<LPB>(okl);
  s = group_sum<LPB>(s);
  const float bc = ok ? huber_cost(s, a.huber) : 0.0f;
  if (live && k == 0) {
    a.valid[blk] = (uint8_t)ok;
    a.cost[blk] = bc;
  }
  if (MODE == 2) {
    if (a.wg_red) {
      const bool one = live && k == 0;
      wg_reduce2(one ? (double)bc : 0.0, one && ok ? 1.0 : 0.0, a.wg_red + 2 * logical_tile());
    }
    return;
  }
  if (!JAC) {
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int px = k + LPB * j;
      if (live && px < P) {
        out[(long long)blk * rec_f + px] = rec_val<S>(ok ? rr[j] : 0.0f);
        if (a.res_out) a.res_out[(long long)blk * P + px] = ok ? rr[j] : 0.0f;
      }
    }
    return;
  }
  if (live && !ok) {  // an invalid block leaves a zero record (Ceres' Evaluate returning false)
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int px = k + LPB * j;
      if (px >= P) continue;
      s_rec[px] = (S)0.0f;
      s_rec[col_jrho(P) + px] = (S)0.0f;
      for (int q = 0; q < 6; ++q) s_rec[col_jhost(P) + 6 * px + q] = s_rec[col_jtarget(P) + 6 * px + q] = (S)0.0f;
      if constexpr (RecFormat<T>::kScaled) s_rec[col_tail(P) + px] = (S)0.0f;
      if constexpr (RecFormat<T>::kIntr) {
        const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        stage_intr(s_rec, P, px, z);
      }
      if constexpr (AFF) stage_affine<RecFormat<T>::kIntr>(s_rec, P, px, 0.0f, 0.0f, false);
    }
  }
  __syncthreads();
  const int nblk = min(BPW, a.n_blocks - blk0);
  if (nblk <= 0) return;
  store_slab<S, NTH>(lds, reinterpret_cast<unsigned char*>(out + (long long)blk0 * rec_f), nblk * rec_f * (int)sizeof(S));
}

// ------------------------------------------------------------------------------------------------
// Geometric block kernel (reprojection.h:105-108): lane = block, record 28 floats = 7 float4 stores, or with the
// target-intrinsics Jacobian (INTR, pba_set_optimize_intrinsics) 44 floats = 11 float4 stores
// ------------------------------------------------------------------------------------------------
template <int MODEL, bool JAC, bool INTR>
__global__ __launch_bounds__(kBlockThreads) void geometric_block_kernel(const KernelArgs a) {
  constexpr int NR = INTR ? 44 : 28;
  const int blk_ = logical_tile() * kBlockThreads + threadIdx.x;
  const bool live = blk_ < a.n_blocks;
  if (!live && !a.wg_red) return;  // (with wg_red every thread reaches the workgroup reduction)
  const int blk = live ? blk_ : a.n_blocks - 1;
  const int pt = a.block_point[blk];
  const PairRec& pp = a.pairs[a.block_pair[blk]];
  // the host camera unprojects with the constant intrinsics (the functor's captured ref_intrinsics, reprojection.h:
  // 93-98), the target camera projects with the intrinsics parameter block (sIntr_c2)
  const double* khd = a.intr_d + kCamD * pp.host_cam;
  const double* ktd = a.intr_t_d + kCamD * pp.target_cam;
  const double2 ur = a.u_ref[pt];
  const double2 uo = a.u_obs[blk];
  const double rho = a.rho[pt];
  const double irho = rcp_nr(rho);
  // p = T_w_t⁻¹ · T_w_h · (b / ρ) in fp64
  const Vec3d b = unproject<MODEL>(khd + kCamHk, ur.x, ur.y);
  const Vec3d ph = {b.x * irho, b.y * irho, b.z * irho};
  const Vec3d Rp = mat_mul(pp.R, ph);
  const Vec3d p = {Rp.x + pp.t[0], Rp.y + pp.t[1], Rp.z + pp.t[2]};
  double u, v;
  const double iden = project<MODEL>(ktd, p, u, v);
  const float r0 = (float)(uo.x - u), r1 = (float)(uo.y - v);
  f32x4* rec = reinterpret_cast<f32x4*>(a.out + (long long)blk * NR);
  float J[NR];
  J[0] = r0;
  J[1] = r1;
  bool ok = isfinite(r0) && isfinite(r1);
  if (JAC) {
    const Vec3 pf = to_f(p), phf = to_f(ph);
    const Vec3 tf = {(float)pp.t[0], (float)pp.t[1], (float)pp.t[2]};
    const float irf = (float)irho;
    Vec3 du, dv;
    project_jac<MODEL>(a.intr_t + 8 * pp.target_cam, pf, (float)iden, du, dv);
    if (INTR) {  // ∂r/∂k = −∂π/∂k (2×8, row-major) after J_rho
      double ku[8], kv[8];
      project_intr_jac<MODEL>(ktd, p, iden, ku, kv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        J[28 + j] = (float)-ku[j];
        J[36 + j] = (float)-kv[j];
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const Vec3 d = i == 0 ? du : dv;
      const Vec3 g = {-d.x, -d.y, -d.z};  // ∂r/∂p = −∂π/∂p
      const Vec3 gR = row_mul(g, pp.R);
      const Vec3 wh = cross(phf, gR);
      const Vec3 wt = cross(g, pf);
      float* jh = J + 2 + 6 * i;
      float* jt = J + 14 + 6 * i;
      jh[0] = gR.x; jh[1] = gR.y; jh[2] = gR.z; jh[3] = wh.x; jh[4] = wh.y; jh[5] = wh.z;
      jt[0] = -g.x; jt[1] = -g.y; jt[2] = -g.z; jt[3] = wt.x; jt[4] = wt.y; jt[5] = wt.z;
      J[26 + i] = dot(g, tf) * irf;  // = ∂π/∂p·R b/ρ² without the cancellation (∂π/∂p·p = 0), pba_internal.h
    }
#pragma unroll
    for (int i = 2; i < NR; ++i) ok = ok && isfinite(J[i]);
  }
  const float bc = ok ? huber_cost(r0 * r0 + r1 * r1, a.huber) : 0.0f;
  if (a.wg_red) {
    wg_reduce2(live ? (double)bc : 0.0, live && ok ? 1.0 : 0.0, a.wg_red + 2 * logical_tile());
    if (!live) return;
  }
  a.valid[blk] = (uint8_t)ok;
  a.cost[blk] = bc;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < NR; ++i) J[i] = 0.0f;
  }
  if (JAC) {
#pragma unroll
    for (int i = 0; i < NR / 4; ++i)
      __builtin_nontemporal_store(f32x4{J[4 * i], J[4 * i + 1], J[4 * i + 2], J[4 * i + 3]}, rec + i);
  } else {
    reinterpret_cast<float2*>(rec)[0] = make_float2(J[0], J[1]);
    if (a.res_out) reinterpret_cast<float2*>(a.res_out)[blk] = make_float2(J[0], J[1]);
  }
}

// ------------------------------------------------------------------------------------------------
// Record decode (pba_decode_records_device): half records → 14·P floats per block.  A workgroup takes kDecodeBlocks
// blocks: their contiguous half records into LDS by 16-B loads (32 records start on a 64-B boundary of the engine's
// record array), then 4 consecutive output values per lane as one 16-B store.  cols = 14 (PBA_RECORD_F16: a plain
// conversion) or 15 (PBA_RECORD_F16_SCALED: a Jacobian entry of pixel row k times the row's scale e[k], exact).
// ------------------------------------------------------------------------------------------------
constexpr int kDecodeBlocks = 32;

__global__ __launch_bounds__(kBlockThreads) void decode_records_kernel(const _Float16* __restrict__ in,
                                                                        float* __restrict__ out, int n_blocks, int P,
                                                                        int cols) {
  constexpr int kScaledCols = RecFormat<ScaledF16>::kCols;
  __shared__ __attribute__((aligned(16))) _Float16 s[kDecodeBlocks * kScaledCols * PBA_MAX_PATTERN];
  const int b0 = blockIdx.x * kDecodeBlocks;
  const int nb = min(kDecodeBlocks, n_blocks - b0);
  const int rec_i = cols * P, rec_o = col_tail(P);
  const int n_in = nb * rec_i, n_out = nb * rec_o;
  const _Float16* src = in + (long long)b0 * rec_i;
  {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
    f32x4* d4 = reinterpret_cast<f32x4*>(s);
    for (int i = threadIdx.x; i < (n_in >> 3); i += kBlockThreads) d4[i] = __builtin_nontemporal_load(s4 + i);
    for (int i = (n_in & ~7) + threadIdx.x; i < n_in; i += kBlockThreads) s[i] = src[i];
  }
  __syncthreads();
  auto value = [&](int o) -> float {
    const int b = o / rec_o, c = o - b * rec_o;
    const _Float16* r = s + b * rec_i;
    float v = (float)r[c];
    if (cols == kScaledCols && c >= col_jhost(P)) v *= (float)r[col_tail(P) + scale_row_of(c, P)];
    return v;
  };
  float* dst = out + (long long)b0 * rec_o;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
    for (int i = threadIdx.x; i < (n_out >> 2); i += kBlockThreads)
      __builtin_nontemporal_store(f32x4{value(4 * i), value(4 * i + 1), value(4 * i + 2), value(4 * i + 3)}, d4 + i);
    for (int i = (n_out & ~3) + threadIdx.x; i < n_out; i += kBlockThreads) dst[i] = value(i);
  } else {
    for (int i = threadIdx.x; i < n_out; i += kBlockThreads) dst[i] = value(i);
  }
}

template <int MODEL>
void launch_geometric(pba_engine* e, const KernelArgs& ka, int mode) {
  const int grid = (e->n_blocks + kBlockThreads - 1) / kBlockThreads;
  e->last_grid = grid;
  if (mode == 1 && e->opt_intr) geometric_block_kernel<MODEL, true, true><<<grid, kBlockThreads, 0, e->stream>>>(ka);
  else if (mode == 1) geometric_block_kernel<MODEL, true, false><<<grid, kBlockThreads, 0, e->stream>>>(ka);
  else if (e->opt_intr) geometric_block_kernel<MODEL, false, true><<<grid, kBlockThreads, 0, e->stream>>>(ka);
  else geometric_block_kernel<MODEL, false, false><<<grid, kBlockThreads, 0, e->stream>>>(ka);
}

// The record format T and the compile-time mode M (1 records, 0 residuals, 2 costs only) of a photometric launch, from
// the engine's state: calls fn(Tag<T>, Mode<M>).  The first row that holds:
//   engine state                                    modes 1 and 0   mode 2
//   affine brightness and free intrinsics           IntrAffineF32   IntrAffineF32
//   affine brightness                               AffineF32       AffineF32
//   free intrinsics                                 IntrF32         float
//   PBA_RECORD_F16_SCALED                           ScaledF16       float
//   PBA_RECORD_F16                                  _Float16        float
//   PBA_RECORD_F32                                  float           float
// (the half formats are refused with free intrinsics and with affine brightness, and those two with each other unless
// pba_set_intrinsics_with_affine allows it.)  A cost-only launch stores no record, so only the affine residual — another
// residual — has a kernel of its own for it, and with both switches on the 26-column tag has its own too: its validity
// differs (PFIN: a projection that is not finite makes the block invalid), and the joint solve with free intrinsics
// (pba_joint_set_solve_intrinsics) must count a candidate's valid blocks as its linearisation does.
template <class T>
struct Tag { using type = T; };
template <int M>
using Mode = std::integral_constant<int, M>;

template <class F>
void dispatch_format(const pba_engine* e, int mode, F&& fn) {
  auto modes = [&](auto tag) {
    if (mode == 1) fn(tag, Mode<1>{});
    else if (mode == 0) fn(tag, Mode<0>{});
    else if constexpr (RecFormat<typename decltype(tag)::type>::kAffine && RecFormat<typename decltype(tag)::type>::kIntr)
      fn(Tag<IntrAffineF32>{}, Mode<2>{});
    else if constexpr (RecFormat<typename decltype(tag)::type>::kAffine) fn(Tag<AffineF32>{}, Mode<2>{});
    else fn(Tag<float>{}, Mode<2>{});
  };
  if (e->affine && e->opt_intr) modes(Tag<IntrAffineF32>{});
  else if (e->affine) modes(Tag<AffineF32>{});
  else if (e->opt_intr) modes(Tag<IntrF32>{});
  else if (e->record_format == PBA_RECORD_F16_SCALED) modes(Tag<ScaledF16>{});
  else if (e->record_format == PBA_RECORD_F16) modes(Tag<_Float16>{});
  else modes(Tag<float>{});
}

// Patterns of at most 8 pixels: one lane per (block, pixel).  PM = camera model + 4 · interpolator (pba_device.h)
template <int PM, int M, class T>
void launch_block(pba_engine* e, KernelArgs ka) {
  const int grid = (int)(((long long)e->n_blocks * 8 + kBlockThreads - 1) / kBlockThreads);
  e->last_grid = grid;
  ka.slab_wt = grid <= kSlabWtGrid;  // one wave of workgroups: write-through record stores (store_slab)
  photometric_block_kernel<PM, 8, M, T><<<grid, kBlockThreads, 0, e->stream>>>(ka);
}

// 9…32 pixels: 8 lanes per block, PPL = ⌈P/8⌉ pixels per lane
template <int PM, int PPL, int M, class T>
void launch_multi(pba_engine* e, const KernelArgs& ka) {
  constexpr int nth = kMultiThreads<PPL, T>;
  const int grid = (int)(((long long)e->n_blocks * 8 + nth - 1) / nth);
  e->last_grid = grid;
  const size_t stage =
      M == 1 ? multi_stage_bytes(nth / 8, e->P, (int)sizeof(typename RecFormat<T>::S), RecFormat<T>::kCols) : 0;
  if constexpr (M == 1 && nth == 256) {
    // the camera-table form for record launches at a fused state with few cameras (the C5 configuration)
    if (ka.poses != nullptr && ka.n_cams <= kCamTab) {
      const size_t lds = stage + (size_t)(nth / 8) * sizeof(TileBlockC);
      if (ka.n_cams == 1) photometric_block_kernel_multi<PM, M, T, PPL, true, true><<<grid, nth, lds, e->stream>>>(ka);
      else photometric_block_kernel_multi<PM, M, T, PPL, true><<<grid, nth, lds, e->stream>>>(ka);
      return;
    }
  }
  photometric_block_kernel_multi<PM, M, T, PPL>
      <<<grid, nth, stage + (size_t)(nth / 8) * sizeof(TileBlock), e->stream>>>(ka);
}

template <int PM>
void launch_photometric(pba_engine* e, const KernelArgs& ka, int mode) {
  const int ppl = (e->P + 7) / 8;
  dispatch_format(e, mode, [&](auto tag, auto m) {
    using T = typename decltype(tag)::type;
    constexpr int M = decltype(m)::value;
    if (ppl <= 1) launch_block<PM, M, T>(e, ka);
    else if (ppl == 2) launch_multi<PM, 2, M, T>(e, ka);
    else if (ppl == 3) launch_multi<PM, 3, M, T>(e, ka);
    else launch_multi<PM, 4, M, T>(e, ka);
  });
}

}  // namespace

#ifdef PBA_EVAL_STAMPS
// test-only entry of the stamped variant: 16 int64 per workgroup of the next 8-lane record launches (nullptr: none)
extern "C" int pba_test_set_eval_stamps(long long* d_stamps) {
  return hipMemcpyToSymbol(HIP_SYMBOL(g_eval_stamps), &d_stamps, sizeof(d_stamps)) == hipSuccess ? 0 : -1;
}
#endif

namespace pba {
namespace detail {

void launch_mode(pba_engine* e, const KernelArgs& ka, int mode) {
  if (e->opt.residual_kind == PBA_RESIDUAL_GEOMETRIC) {
    switch (e->opt.camera_model) {
      case PBA_CAMERA_PINHOLE: launch_geometric<CAM_PINHOLE>(e, ka, mode); break;
      case PBA_CAMERA_DOUBLE_SPHERE: launch_geometric<CAM_DS>(e, ka, mode); break;
      case PBA_CAMERA_EUCM: launch_geometric<CAM_EUCM>(e, ka, mode); break;
      default: launch_geometric<CAM_KB4>(e, ka, mode); break;
    }
    return;
  }
  dispatch_pm(e, [&](auto pm) { launch_photometric<decltype(pm)::value>(e, ka, mode); });
}

KernelArgs make_kernel_args(pba_engine* e, const PairRec* pairs, const double* rho) {
  KernelArgs ka{};
  ka.images = e->images.p;
  ka.width = e->width;
  ka.height = e->height;
  ka.tiles_x = tiles_x_of(e->width);
  ka.frame_stride = tiled_frame_bytes(e->width, e->height);
  ka.umax = e->width + 1.0;
  ka.vmax = e->height + 1.0;
  ka.intr = e->intr.p;
  ka.intr_d = e->intr_d.p;
  ka.intr_t = e->opt_intr ? e->intr_state.p : e->intr.p;
  ka.intr_t_d = e->opt_intr ? e->intr_state_d.p : e->intr_d.p;
  ka.intr_scale = std::ldexp(1.0f, -e->level);
  ka.block_point = e->block_point.p;
  ka.block_pair = e->block_pair.p;
  ka.block_pp = e->block_pp.p;
  ka.pairs = pairs;
  ka.block_rec = e->block_rec.p;
  ka.n_pose_d = 7 * e->n_frames;
  ka.n_points = e->n_points;
  ka.u_ref = e->u_ref.p;
  ka.host_int = e->host_int.p;
  ka.rho = rho;
  ka.u_obs = e->u_obs.p;
  if (e->affine) ka.affine = e->affine_state.p;  // (photometric: u_obs unused, the slot is shared)
  ka.out = e->out.p;
  ka.cost = e->cost.p;
  ka.valid = e->valid.p;
  ka.n_blocks = e->n_blocks;
  ka.n_cams = e->n_cams;
  ka.P = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC ? e->P : 2;
  ka.huber = e->opt.huber_width;
  for (size_t i = 0; i < e->pattern_h.size() && i < 2 * PBA_MAX_PATTERN; ++i) ka.pattern[i] = e->pattern_h[i];
  return ka;
}

int launch_cost_only(pba_engine* e, const PairRec* pairs, const double* rho, double* wg_red, int* n_slots,
                     const double* poses, const float* intr_t, const double* intr_t_d, const double* affine) {
  KernelArgs ka = make_kernel_args(e, pairs, rho);
  ka.poses = poses;
  if (affine && e->affine) ka.affine = affine;
  if (intr_t) ka.intr_t = intr_t;
  if (intr_t_d) ka.intr_t_d = intr_t_d;
  ka.wg_red = wg_red;
  launch_mode(e, ka, 2);
  if (n_slots) *n_slots = e->last_grid;
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

int launch_decode_records(pba_engine* e, float* d_out) {
  if (e->record_format == PBA_RECORD_F32) {
    PBA_HIP(hipMemcpyAsync(d_out, e->out.p, (size_t)e->n_blocks * e->rec_floats() * sizeof(float),
                           hipMemcpyDeviceToDevice, e->stream));
    return PBA_OK;
  }
  const int grid = (e->n_blocks + kDecodeBlocks - 1) / kDecodeBlocks;
  const bool scaled = e->record_format == PBA_RECORD_F16_SCALED;
  decode_records_kernel<<<grid, kBlockThreads, 0, e->stream>>>(
      reinterpret_cast<const _Float16*>(e->out.p), d_out, e->n_blocks, e->P,
      scaled ? (int)RecFormat<ScaledF16>::kCols : (int)RecFormat<_Float16>::kCols);
  PBA_HIP(hipGetLastError());
  return PBA_OK;
}

}  // namespace detail
}  // namespace pba
