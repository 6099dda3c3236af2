// pba_gn_linearize.hip — the linearisation of a Gauss-Newton trial (pba_gn.hip): linearize_adj_kernel / linearize_kernel.
//
// Replaces the reference's Jacobian writer and gradient accumulation (program_evaluator.h:233-257).
#include <hip/hip_runtime.h>

#include <utility>

#include "pba_gn.h"

using namespace pba;
using namespace pba::detail;

namespace {

constexpr int NV = 104;          // normal-equation products per residual row

// x = [J_h(6) | J_t(6) | J_ρ | r]; product v = x[pa(v)] · x[pb(v)]
__host__ __device__ constexpr int upper_index(int i, int j) {  // 6×6 upper triangle, i ≤ j
  return i * 6 - i * (i - 1) / 2 + (j - i);
}
__host__ __device__ constexpr int pa(int v) {
  if (v < 21) { int i = 0; while (upper_index(i, 5) < v) ++i; return i; }
  if (v < 57) return (v - 21) / 6;
  if (v < 78) { int i = 0; while (upper_index(i, 5) < v - 57) ++i; return 6 + i; }
  if (v < 84) return v - 78;
  if (v < 90) return 6 + (v - 84);
  if (v < 92) return 12;
  if (v < 98) return v - 92;
  if (v < 104) return 6 + (v - 98);
  return 13;
}
__host__ __device__ constexpr int pb(int v) {
  if (v < 21) { const int i = pa(v); return i + (v - upper_index(i, i)); }
  if (v < 57) return 6 + (v - 21) % 6;
  if (v < 78) { const int i = pa(v) - 6; return 6 + i + (v - 57 - upper_index(i, i)); }
  if (v < 90) return 13;
  if (v == 90) return 12;
  if (v == 91) return 13;
  if (v < 104) return 12;
  return 13;
}
static_assert(pa(0) == 0 && pb(0) == 0 && pa(20) == 5 && pb(20) == 5 && pa(6) == 1 && pb(6) == 1, "table");
static_assert(pa(57) == 6 && pb(57) == 6 && pa(77) == 11 && pb(77) == 11, "table");
static_assert(pa(21) == 0 && pb(21) == 6 && pa(56) == 5 && pb(56) == 11, "table");

// The linearisation's R_th, t_th of pair `pair` into pair_rt, by lanes k < 12 of the LPB lanes of the first block of
// each target in the wave (the same values where a pair's blocks span waves or chunks)
template <int LPB>
__device__ __forceinline__ void store_pair_rt(double* pair_rt, const double* R, const double* t, int pair, int lt, int k,
                                              bool live) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl(lt, (lane - LPB) & 63, 64);
  if (live && ((lane & ~(LPB - 1)) == 0 || prev != lt))
    for (int e = k; e < 12; e += LPB) pair_rt[(long long)pair * 12 + e] = e < 9 ? R[e] : t[e - 9];
}

// ------------------------------------------------------------------------------------------------
// linearize_kernel
// ------------------------------------------------------------------------------------------------
// Slot of the product x[r]·x[c] (r ≤ c) in the 104-product layout, or 255 when not needed (x13·x13, pad columns).
__host__ __device__ constexpr int slot_of(int r, int c) {
  for (int v = 0; v < NV; ++v)
    if (pa(v) == r && pb(v) == c) return v;
  return 255;
}
// MFMA 16×16 output held by lane l, entry m = 0..3: v_mfma_f32_16x16x4f32 C[4(l/16) + m][l%16], v_mfma_f64_16x16x4f64
// C[l/16 + 4m][l%16] (cdna_hip_programming.md: the f64 form has a layout of its own) → the four slots of lane l (upper
// triangle only, so each product is written once), packed as bytes.
__host__ __device__ constexpr unsigned slot_word(int lane, bool f64) {
  unsigned w = 0;
  for (int m = 0; m < 4; ++m) {
    const int r = f64 ? (lane >> 4) + 4 * m : 4 * (lane >> 4) + m, c = lane & 15;
    w |= (unsigned)(r <= c ? slot_of(r, c) : 255) << (8 * m);
  }
  return w;
}
template <int... L>
constexpr auto make_slot_table(bool f64, std::integer_sequence<int, L...>) {
  struct T { unsigned w[64]; };
  return T{{slot_word(L, f64)...}};
}
__constant__ const auto kSlotTable64 = make_slot_table(true, std::make_integer_sequence<int, 64>{});

// Normal-equation products by matrix cores: weighted rows X (R × 14, padded to LPB × 16 per block; fp32) give
// XᵀX = Σ_k x_kᵀx_k as v_mfma_f64_16x16x4f64 steps (operand A = Xᵀ and B = X are the same register: lane l holds
// X[4s + l/16][l%16], converted to fp64) — the products of fp32 rows are exact in fp64, so the system is the Gram
// matrix of the rows to fp64 rounding.  A chunk's blocks are ordered by target (gn_prepare), so the blocks of one
// target are consecutive in a wave: each block's product set is added to its target run's sum, and a wave stores one
// product set per distinct target (≤ kChunkTargets) instead of one per block.
template <int KIND, int MODEL, int LPB>
constexpr int kLinWaves = KIND == PBA_RESIDUAL_PHOTOMETRIC && MODEL == CAM_PINHOLE + 4 * INTERP_BILINEAR && LPB == 8 ? 8 : 1;

template <int KIND, int MODEL, int LPB>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(kLinWaves<KIND, MODEL, LPB>, 8)))
void linearize_kernel(const KernelArgs a, const LinArgs g) {
  constexpr int BW = 64 / LPB;              // blocks per wave
  constexpr int NW = kBlockThreads / 64;    // waves per workgroup
  constexpr int SPB = LPB / 4;              // MFMA steps per block
  constexpr int NVP = 108;                  // 104 products, padded
  constexpr int kTileW = KIND == PBA_RESIDUAL_PHOTOMETRIC ? BW * (int)sizeof(TileBlock) : 0;
  constexpr int kRowsW = 64 * 16 * 4, kProdW = kChunkTargets * NVP * 8;
  constexpr int kArena = (kTileW > kRowsW ? (kTileW > kProdW ? kTileW : kProdW) : (kRowsW > kProdW ? kRowsW : kProdW));
  // per-wave arena, used in turn by the wave's tile blocks, its weighted rows and its per-target products
  // (each phase only touches the wave's own blocks; LDS is in order within a wave)
  __shared__ __attribute__((aligned(16))) unsigned char arena[NW][kArena];
  __shared__ int s_wlo[NW], s_wn[NW];
  __shared__ float s_bc[kBlockThreads / LPB];  // block costs (0: invalid or dead), for the chunk's cost partial
  __shared__ unsigned s_slots[NW][64];          // the product slot table (kSlotTable64), each lane's word parked in LDS
  const int chunk = logical_tile();
  const int lb = threadIdx.x / LPB;
  // one memory round: the record, the chunk descriptor, the block's linearise record and the slot table are all issued
  // before either exit (at a clamped chunk), and the exits test them together — the compiler otherwise issued the record
  // behind the chunk test, the descriptor behind the record's done test and the linearise record behind both (three
  // dependent rounds before the tile's loads)
  const int cc = min(chunk, g.n_chunks - 1);
  const int4 d = g.chunk_desc[cc];
  const int4 lr = g.lin_rec[(long long)cc * (kBlockThreads / LPB) + lb];
  const unsigned slot_w = kSlotTable64.w[threadIdx.x & 63];
  const LmView lv = lm_view(g.lm);
  asm volatile("" ::"v"(lr.x), "v"(lr.y), "v"(lr.z), "v"(lr.w), "v"(slot_w), "s"(d.x), "s"(d.y), "s"(d.z), "s"(d.w));
  s_slots[threadIdx.x >> 6][threadIdx.x & 63] = slot_w;  // (read back by the same lane: no barrier)
  if (chunk >= g.n_chunks || lv.done != 0.0) return;
  const bool s1 = (lv.set != 0.0) != g.spare;
  double* const blk_schur = s1 ? g.blk_schur1 : g.blk_schur;
  double* const part_lin = s1 ? g.part_lin1 : g.part_lin;
  if (g.lin_set && chunk == 0 && threadIdx.x == 0) {  // (the λ-free elimination after this launch reads them)
    *g.lin_set = s1 ? 1 : 0;
    g.degen[s1 ? 1 : 0] = 0;
  }
  const int count = d.y, n_t = d.z, poff = d.w;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = threadIdx.x % LPB, wb = lb % BW;
  const bool live = lb < count;
  const int R = KIND == PBA_RESIDUAL_PHOTOMETRIC ? a.P : 2;
  const bool act = live && k < R;
  // the chunk's slots are padded to the workgroup's blocks (dead slots repeat slot 0), so the record is read with the
  // chunk descriptor, not behind it, and carries the block's point and pair: the tile prologue's loads come next
  const int blk = lr.x, gpos = lr.w, lt = (int)((unsigned)lr.z >> 24);
  Row row;
  if constexpr (KIND == PBA_RESIDUAL_PHOTOMETRIC) {
    TileBlock* s_tb = reinterpret_cast<TileBlock*>(arena[wave]);
    const float2 off = pattern_at<LPB>(a, k);
    // the host intensity in the tile's memory round (its point is in the linearise record): issued behind the tile's
    // loads it cost a round of its own at the barrier
    const float Ih = act ? a.host_int[(long long)lr.y * R + k] : 0.0f;
    stage_tile_pp<LPB>(a, s_tb, wb, k, make_int2(lr.y, lr.z & 0xffffff));
    asm volatile("" ::"v"(Ih));
    __syncthreads();
#ifdef PBA_ABL_NOROW  // ablation builds (tools/build_variant.sh): timing of the parts, results are garbage
    row.r = Ih + s_tb[wb].pr.Rf[k & 7] + off.x;
    row.jr = row.hv.x = row.hv.y = row.hv.z = row.hw.x = row.hw.y = row.hw.z = row.r;
    row.tv = row.hv;
    row.tw = row.hw;
#else
    row = photometric_row<MODEL, true>(a, s_tb[wb], off, Ih);  // dead lanes evaluate a staged block, masked below
#endif
    store_pair_rt<LPB>(s1 ? g.pair_rt1 : g.pair_rt, s_tb[wb].pr.R, s_tb[wb].pr.t, lr.z & 0xffffff, lt, k, live);
  } else {
    if (act) row = geometric_row<MODEL, true>(a, blk, k);
    const PairRec& pr = a.pairs[lr.z & 0xffffff];
    store_pair_rt<LPB>(s1 ? g.pair_rt1 : g.pair_rt, pr.R, pr.t, lr.z & 0xffffff, lt, k, live);
  }
  const int ok = group_all<LPB>(act ? row.ok : 1);
  const float s = group_sum<LPB>(act && ok ? row.r * row.r : 0.0f);
  const float w = ok ? huber_weight(s, a.huber) : 0.0f;
  const float bcost = ok ? huber_cost(s, a.huber) : 0.0f;
  if (k == 0) s_bc[lb] = live && ok ? bcost : -1.0f;  // read after the barrier below
  // weighted row x̃ = √w · x  → products carry w (Ceres Corrector with ρ'' ≤ 0: J̃ = √ρ' J, r̃ = √ρ' r)
  // the product slot table, loaded in the first memory round and parked in LDS across the row (one register fewer
  // there: the row's peak pressure spilled at 8 waves/SIMD)
  const unsigned slots = s_slots[wave][lane];
  // rows outside the domain / of dead lanes are all zero (selects, not a zero weight: such a row may hold inf / NaN)
  const bool use = act && ok;
  const float sw = use ? sqrtf(w) : 0.0f;
  auto wx = [&](float v) { return use ? sw * v : 0.0f; };
  const float x[14] = {wx(row.hv.x), wx(row.hv.y), wx(row.hv.z), wx(row.hw.x), wx(row.hw.y), wx(row.hw.z),
                       wx(row.tv.x), wx(row.tv.y), wx(row.tv.z), wx(row.tw.x), wx(row.tw.y), wx(row.tw.z),
                       wx(row.jr), wx(row.r)};
  float* sX = reinterpret_cast<float*>(arena[wave]);  // the wave's 64 rows × 16 floats (overwrites its tile blocks)
  {
    float4* xr = reinterpret_cast<float4*>(sX + lane * 16);
    xr[0] = make_float4(x[0], x[1], x[2], x[3]);
    xr[1] = make_float4(x[4], x[5], x[6], x[7]);
    xr[2] = make_float4(x[8], x[9], x[10], x[11]);
    xr[3] = make_float4(x[12], x[13], 0.0f, 0.0f);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  {
    // every operand first (the product sets below overwrite the rows), then the wave's blocks in order; each run of
    // equal local target is summed in registers and its 16×16 result scattered as the 104 products of that slot
    const int ci = lane & 15, kq = lane >> 4;
    float op[BW * SPB];
#pragma unroll
    for (int st = 0; st < BW * SPB; ++st) op[st] = sX[(4 * st + kq) * 16 + ci];
    double* sP = reinterpret_cast<double*>(arena[wave]);
    const int nbw = min(max(count - wave * BW, 0), BW);  // live blocks of this wave (wave-uniform)
    const int lo = __builtin_amdgcn_readfirstlane(lt);     // lane 0 holds the wave's first block
    auto flush = [&](const v4f64& acc, int slot) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const unsigned v = (slots >> (8 * m)) & 255u;
        if (v < (unsigned)NV) sP[slot * NVP + v] = acc[m];
      }
    };
    // per block: its own chain (SPB steps); row 12 of the result, C[12][c] in entry 3 of lanes c < 16, is the block's
    // point-elimination data x̃_ρ·x̃_c → [H_ρρ, g_ρ, W_h(6), W_t(6), 0, 0] at its GN position (schur_kernel walks
    // them point by point); the block's products are then added to its target run's sum
    // (column c of row 12: W_h for c < 6 — not stored, schur_chunk forms it from W_t — W_t for 6 ≤ c < 12, H_ρρ, g_ρ)
    const int pc = lane < 16 ? lane : -1, pq = pc >= 6 && pc < 12 ? pc - 4 : (pc == 12 ? 0 : (pc == 13 ? 1 : -1));
    v4f64 tacc = {0.0, 0.0, 0.0, 0.0};
    int cur = lo;
    // block b's chain (SPB dependent steps); a dead block's rows are zeros, so its chain is issued unconditionally
#ifndef PBA_ABL_NOMFMA
    auto chain = [&](int b) {
      v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int st = 0; st < SPB; ++st) {
        const double o = (double)op[b * SPB + st];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(o, o, acc, 0, 0, 0);
      }
      return acc;
    };
#endif
    // two blocks in flight: block b + 1's matrix-core steps are issued before block b's result is consumed (each
    // dependent fp64 step waited out its latency before the point-data store and the run sum otherwise)
#ifdef PBA_ABL_NOMFMA
    auto chain = [&](int b) {
      const double o = (double)op[b * SPB];
      return v4f64{o, o, o, o};
    };
#endif
    v4f64 nxt = chain(0);
#pragma unroll
    for (int b = 0; b < BW; ++b) {
      const v4f64 acc = nxt;
      if (b + 1 < BW) nxt = chain(b + 1);
#ifdef PBA_ABL_NOBLK
      if (b == 0) {
        tacc = acc;
        cur = lo;
      }
      if (false) {
#else
      if (b < nbw) {
#endif
        const int gpb = __builtin_amdgcn_readlane(gpos, b * LPB);
        if (pq >= 0) blk_schur[(long long)gpb * kPd + pq] = acc[3];
#ifndef PBA_ABL_NORUN
        const int ltb = __builtin_amdgcn_readlane(lt, b * LPB);
        if (ltb != cur) {
          flush(tacc, cur - lo);
          tacc = v4f64{0.0, 0.0, 0.0, 0.0};
          cur = ltb;
        }
        tacc += acc;
#endif
      }
    }
    if (nbw > 0) flush(tacc, cur - lo);
    if (lane == 0) {
      s_wlo[wave] = lo;
      s_wn[wave] = nbw > 0 ? cur - lo + 1 : 0;
    }
  }
  __syncthreads();
  // chunk partial slots, fixed summation order (wave, then slot): H_hh / g_h over every product set of the chunk,
  // H_ht / H_tt / g_t of local target j from the ≤ NW sets of j (one per wave that holds j's blocks)
  auto sset = [&](int w, int i, int v) -> double { return reinterpret_cast<const double*>(arena[w])[i * NVP + v]; };
#ifdef PBA_ABL_NOPART
  const int nout = 0;
#else
  const int nout = SLOT_LIN_BASE + SLOT_LIN_T * n_t;
#endif
  for (int o = threadIdx.x; o < nout; o += kBlockThreads) {
    int v, j = -1;
    if (o < 36) {
      const int r = o / 6, c = o % 6;
      v = upper_index(min(r, c), max(r, c));
    } else if (o < 42) {
      v = 78 + (o - 36);
    } else {
      j = (o - 42) / SLOT_LIN_T;
      const int q = (o - 42) % SLOT_LIN_T;
      if (q < 36) v = 21 + q;
      else if (q < 72) { const int r = (q - 36) / 6, c = (q - 36) % 6; v = 57 + upper_index(min(r, c), max(r, c)); }
      else v = 84 + (q - 72);
    }
    double acc = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int wl = s_wlo[w], wn = s_wn[w];
      if (j < 0) {
        for (int i = 0; i < wn; ++i) acc += sset(w, i, v);
      } else if (j >= wl && j < wl + wn) {
        acc += sset(w, j - wl, v);
      }
    }
    part_lin[(long long)poff + o] = acc;
  }
  // the block costs last: a store issued before a load makes the wait for that load wait for the store too (GFX9
  // counts loads and stores in one counter), so the stores go after every load of the kernel
  if (live && k == 0) {
    a.valid[blk] = (uint8_t)ok;
    a.cost[blk] = bcost;
  }
  if (g.wg_red && wave == 0) {  // the chunk's (Σ cost, Σ valid): lane b takes block b, xor butterflies (fixed order)
    static_assert(kBlockThreads / LPB <= 64, "one lane per block of the chunk");
    const float x = lane < count ? s_bc[lane] : -1.0f;
    double c = x >= 0.0f ? (double)x : 0.0, v = x >= 0.0f ? 1.0 : 0.0;
    for (int m = 32; m >= 1; m >>= 1) {
      c += __shfl_xor(c, m, 64);
      v += __shfl_xor(v, m, 64);
    }
    if (lane == 0) {
      g.wg_red[2 * chunk] = c;
      g.wg_red[2 * chunk + 1] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// linearize_adj_kernel: the photometric linearisation of ≤ 8-px patterns through the pair's adjoint
// ------------------------------------------------------------------------------------------------
// A photometric row's host Jacobian is its target Jacobian through the relative pose: with p̃ = R b + ρ t (R = R_th,
// t = t_th) the rows of photometric_row satisfy [hv hw] = −[tv tw]·Ad, Ad = [[R, [t]×R], [0, R]] — the SE(3) adjoint of
// T_th (exact algebra: hv = ρ qR = −tv R, hw = b × qR = −tw R − tv [t]× R).  Ceres differentiates both poses through
// the functor (photometric_error.h:146-186); the normal equations only need their products, and those follow from the
// target's: J_hᵀJ_h = Adᵀ(J_tᵀJ_t)Ad, J_hᵀJ_t = −Adᵀ(J_tᵀJ_t), J_hᵀr = −Adᵀ(J_tᵀr), J_ρᵀJ_h = −(J_ρᵀJ_t)Ad — linear in
// the per-target sums, so applied once per (chunk, target) and once per block for the point data.  The matrix cores
// then form only the 8-column products of x = √w [tv tw jr r] (36 in the upper triangle, against 104 of the 14-column
// rows): per block the three 4×4 tiles (0,0), (0,1), (1,1) of xᵀx, K = 8 rows in two steps of v_mfma_f64_4x4x4_4b_f64
// (16 cycles each, against two 64-cycle v_mfma_f64_16x16x4f64).  Same chunk partials and point data as
// linearize_kernel (the 14-column kernel, kept for the geometric rows and as PBA_LIN_LEGACY's A/B reference).
// MFMA layout (tools/micro/mfma_f64_4x4_layout.hip, measured): lane l works in 4×4 block β = (l >> 2) & 3; A holds
// A_β[l & 3][l >> 4], B holds B_β[l >> 4][l & 3], the accumulator C_β[l >> 4][l & 3].
__host__ __device__ constexpr int upper8(int r, int c) { return r * 8 - r * (r - 1) / 2 + (c - r); }  // r ≤ c < 8

// PPL > 1 (9…32 px, C5's 21): lane k evaluates pixels k, k + 8, … in PPL passes (8 lanes per block, as the evaluation's
// photometric_block_kernel_multi: a chunk stays 32 blocks, the chunk partials those of 8 px); each pass's
// unweighted rows go through the matrix cores into per-block fp64 accumulators (the chain runs on across the passes) and
// the block's Huber weight, known after its last row, scales them (x̃ᵀx̃ = w·xᵀx).  LDS per wave: the tile blocks and a
// pass's rows side by side, the run product sets over the tile once the passes are done.
#ifndef PBA_LINADJ_WAVES
#define PBA_LINADJ_WAVES 5
#endif
// NT: threads per workgroup (NT / 8 blocks per chunk).  Measured at 8 px: 512 threads (64-block chunks: the phases,
// partial slots, assembly contributions and decision slots per chunk spread over twice the blocks) 71.1 → 76.6 µs for
// the linearisation against 12.1 → 10.9 for the assembly — the 8-wave barriers cost more than the halved chunk work.
// AFF (pba_gn_set_solve_affine): the rows' residual is r = (I − b_t) − E·(I_h − b_h) at the engine's affine state, held
// constant — block_affine once per block in the first memory round (the pair-table branch: host and target from the
// block's pair) and photometric_row<…, AFF>, the record path's formula and bits.  ∇I does not depend on (a, b): the
// Jacobian columns, the products and everything downstream are the same code.
template <int MODEL, int PPL, int NT, bool AFF = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(PPL == 1 ? 8 : PBA_LINADJ_WAVES, 8)))
void linearize_adj_kernel(const KernelArgs a, const LinArgs g) {
  constexpr int LPB = 8, BW = 64 / LPB, NW = NT / 64;
  constexpr int kRowS = 12;                  // floats per staged row (8 used): 8-lane groups of b128 stores hit 32 banks
  constexpr int NQ = 36;                     // products per run set (the 8 × 8 upper triangle)
  constexpr int kTileW = BW * (int)sizeof(TileBlock), kRowsW = 64 * kRowS * 4, kProdW = kChunkTargets * NQ * 8;
  // per wave — PPL = 1: [tile blocks, then the weighted rows over them | run product sets];
  //            PPL > 1: [tile blocks, then the run product sets over them | a pass's rows]
  constexpr int kRowsOff = PPL == 1 ? 0 : kTileW;
  constexpr int kProdOff = PPL == 1 ? (kTileW > kRowsW ? kTileW : kRowsW) : 0;
  constexpr int kArena = PPL == 1 ? kProdOff + kProdW : kTileW + kRowsW;
  static_assert(kProdW <= kTileW && kRowsW <= kTileW + 512, "regions");
  static_assert(kChunkTargets * 64 * 8 <= kRowsW, "phase data fits a rows region");
  static_assert(NT >= 64 * kChunkTargets && NT / LPB <= 64, "one thread per entry of the targets' 8 × 8 sums");
  __shared__ __attribute__((aligned(16))) unsigned char arena[NW][kArena];
  __shared__ double s_rt[kChunkTargets][12];  // R_th, t_th of each local target (the host is the chunk's)
  __shared__ double s_ad[kChunkTargets][36];  // Ad of each local target
  __shared__ int s_wlo[NW], s_wn[NW];
  __shared__ float s_bc[NT / LPB];
  __shared__ float2 s_pat[PPL == 1 ? 1 : LPB * PPL];
  const int chunk = logical_tile();
  const int lb = threadIdx.x / LPB;
  // one memory round: record, chunk descriptor and linearise record before either exit (see linearize_kernel)
  const int cc = min(chunk, g.n_chunks - 1);
  const int4 d = g.chunk_desc[cc];
  const int4 lr = g.lin_rec[(long long)cc * (NT / LPB) + lb];
  const LmView lv = lm_view(g.lm);
  asm volatile("" ::"v"(lr.x), "v"(lr.y), "v"(lr.z), "v"(lr.w), "s"(d.x), "s"(d.y), "s"(d.z), "s"(d.w));
  if (chunk >= g.n_chunks || lv.done != 0.0) return;
  const bool s1 = (lv.set != 0.0) != g.spare;
  double* const blk_schur = s1 ? g.blk_schur1 : g.blk_schur;
  double* const part_lin = s1 ? g.part_lin1 : g.part_lin;
  if (g.lin_set && chunk == 0 && threadIdx.x == 0) {  // (the λ-free elimination after this launch reads them)
    *g.lin_set = s1 ? 1 : 0;
    g.degen[s1 ? 1 : 0] = 0;
  }
  const int count = d.y, n_t = d.z, poff = d.w;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = threadIdx.x % LPB, wb = lb % BW;
  const bool live = lb < count;
  const int R = a.P;
  const int blk = lr.x, gpos = lr.w, lt = (int)((unsigned)lr.z >> 24);
  TileBlock* s_tb = reinterpret_cast<TileBlock*>(arena[wave]);
  float* sX = reinterpret_cast<float*>(arena[wave] + kRowsOff);  // the wave's 64 rows
  // the block's pair is in the linearise record: block_affine goes pair → keyframes' state without the block → pair load
  // (a dead slot repeats slot 0: a live block's pair); PPL > 1 parks E, b_h, b_t in LDS across the pass loop, read back
  // per pass like the tile (three registers fewer across the row: the 17–32-px pinhole forms spilled them)
  __shared__ float s_af[AFF && PPL > 1 ? NT / LPB : 1][3];
  Affine af = {1.0f, 0.0f, 0.0f};
  if constexpr (AFF) af = block_affine(a, blk, lr.z & 0xffffff);
  // lane l: 4×4 block β — tiles (0,0), (0,1), (1,1) of xᵀx, and β = 3 repeating (0,1) unused — operand columns
  // ca / cb, product (pr_, pc_)
  const int beta = (lane >> 2) & 3, i4 = lane & 3, kq = lane >> 4;
  const int I = beta == 2 ? 1 : 0, J = beta == 0 ? 0 : 1;
  const int ca = 4 * I + i4, cb = 4 * J + i4;
  auto ops = [&](int b, float* o) {  // block b's operands from the staged rows: A, B of K steps 0 and 1
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const float* xr = sX + (8 * b + 4 * st + kq) * kRowS;
      o[2 * st] = xr[ca];
      o[2 * st + 1] = xr[cb];
    }
  };
  auto save_rt = [&]() {  // R_th, t_th of the block's target from the first block of each target in the wave, for
                          // the phases below and (pair_rt) the point elimination's W_h
    const int prev = __shfl(lt, (lane - LPB) & 63, 64);
    if (live && (wb == 0 || prev != lt)) {
      const PairRec& pr = s_tb[wb].pr;
      double* prt = (s1 ? g.pair_rt1 : g.pair_rt) + (long long)(lr.z & 0xffffff) * 12;
      s_rt[lt][k] = prt[k] = pr.R[k];
      if (k < 4) s_rt[lt][8 + k] = prt[8 + k] = k == 0 ? pr.R[8] : pr.t[k - 1];
    }
  };
  int ok;
  float bcost;
  double accb[BW];  // the blocks' products (PPL > 1: unweighted over the passes, then weighted)
  if constexpr (PPL == 1) {
    const bool act = live && k < R;
    const float2 off = pattern_at<LPB>(a, k);
    const float Ih = act ? a.host_int[(long long)lr.y * R + k] : 0.0f;
    stage_tile_pp<LPB>(a, s_tb, wb, k, make_int2(lr.y, lr.z & 0xffffff));
    asm volatile("" ::"v"(Ih));
    __syncthreads();
#ifdef PBA_ABL_ROW  // ablation builds (tools/build_variant.sh): timing of the parts, results are garbage
    Row row;
    row.r = Ih + (float)s_tb[wb].pr.R[k] + off.x;
    row.jr = row.r;
    row.tv = Vec3{row.r, row.r, row.r};
    row.tw = row.tv;
#else
    const Row row =  // (hv, hw unused: not formed)
        photometric_row<MODEL, true, TileBlock, false, false, AFF>(a, s_tb[wb], off, Ih, nullptr, nullptr, &af);
#endif
    save_rt();
    ok = group_all<LPB>(act ? row.ok : 1);
    const float s = group_sum<LPB>(act && ok ? row.r * row.r : 0.0f);
    const float w = ok ? huber_weight(s, a.huber) : 0.0f;
    bcost = ok ? huber_cost(s, a.huber) : 0.0f;
    const bool use = act && ok;
    const float sw = use ? sqrtf(w) : 0.0f;
    auto wx = [&](float v) { return use ? sw * v : 0.0f; };
    float4* xr = reinterpret_cast<float4*>(sX + lane * kRowS);  // (over the wave's tile blocks, read above)
    xr[0] = make_float4(wx(row.tv.x), wx(row.tv.y), wx(row.tv.z), wx(row.tw.x));
    xr[1] = make_float4(wx(row.tw.y), wx(row.tw.z), wx(row.jr), wx(row.r));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    if ((int)threadIdx.x < LPB * PPL) s_pat[threadIdx.x] = pattern_at<LPB * PPL>(a, threadIdx.x);
    float Ih[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
      const int px = k + LPB * j;
      Ih[j] = live && px < R ? a.host_int[(long long)lr.y * R + px] : 0.0f;
    }
    stage_tile_pp<LPB>(a, s_tb, wb, k, make_int2(lr.y, lr.z & 0xffffff));
#pragma unroll
    for (int j = 0; j < PPL; ++j) asm volatile("" ::"v"(Ih[j]));
    if constexpr (AFF) {
      if (k == 0) {
        s_af[lb][0] = af.E;
        s_af[lb][1] = af.bh;
        s_af[lb][2] = af.bt;
      }
    }
    __syncthreads();
    save_rt();
#pragma unroll
    for (int b = 0; b < BW; ++b) accb[b] = 0.0;
    int okl = 1;
    float s = 0.0f;
#pragma unroll 1
    for (int j = 0; j < PPL; ++j) {
      const int px = k + LPB * j;
      const bool act = live && px < R;
      float ih = Ih[0];
#pragma unroll
      for (int q = 1; q < PPL; ++q) ih = j == q ? Ih[q] : ih;
      asm volatile("" ::: "memory");  // the tile is read from LDS per pass (see photometric_block_kernel_multi)
#ifdef PBA_ABL_ROW
      Row row;
      row.ok = 1;
      row.r = ih + (float)s_tb[wb].pr.R[k] + s_pat[act ? px : 0].x;
      row.jr = row.r;
      row.tv = Vec3{row.r, row.r, row.r};
      row.tw = row.tv;
#else
      Affine afl = af;
      if constexpr (AFF) afl = Affine{s_af[lb][0], s_af[lb][1], s_af[lb][2]};
      const Row row = photometric_row<MODEL, true, TileBlock, false, false, AFF>(a, s_tb[wb], s_pat[act ? px : 0], ih,
                                                                                 nullptr, nullptr, &afl);
#endif
      const bool use = act && row.ok;
      okl &= act ? row.ok : 1;
      s += use ? row.r * row.r : 0.0f;
      auto xv = [&](float v) { return use ? v : 0.0f; };  // selects: a row that is not ok may hold inf / NaN
      float4* xr = reinterpret_cast<float4*>(sX + lane * kRowS);
      xr[0] = make_float4(xv(row.tv.x), xv(row.tv.y), xv(row.tv.z), xv(row.tw.x));
      xr[1] = make_float4(xv(row.tw.y), xv(row.tw.z), xv(row.jr), xv(row.r));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#ifndef PBA_ABL_MFMA
#pragma unroll
      for (int b = 0; b < BW; ++b) {
        float o[4];
        ops(b, o);
#pragma unroll
        for (int st = 0; st < 2; ++st)
          accb[b] = __builtin_amdgcn_mfma_f64_4x4x4f64((double)o[2 * st], (double)o[2 * st + 1], accb[b], 0, 0, 0);
      }
#endif
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // this pass's reads before the next pass's row stores
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    ok = group_all<LPB>(okl);
    s = group_sum<LPB>(s);
    const float w = ok ? huber_weight(s, a.huber) : 0.0f;
    bcost = ok ? huber_cost(s, a.huber) : 0.0f;
#pragma unroll
    for (int b = 0; b < BW; ++b)
      accb[b] *= (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), b * LPB));
  }
  if (k == 0) s_bc[lb] = live && ok ? bcost : -1.0f;  // read after the barrier below
  const int nbw = min(max(count - wave * BW, 0), BW);
  {
    const int pr_ = 4 * I + kq, pc_ = 4 * J + i4;
    const int pslot = beta < 3 && pr_ <= pc_ ? upper8(pr_, pc_) : -1;
    // the point data: column 6 (jr) of tiles (0,1) and (1,1) — W_t[0..3] and W_t[4..5], H_ρρ, g_ρ — at its blk_schur
    // position [H_ρρ, g_ρ, W_t(6)]
    const int ppos = i4 != 2 || beta == 0 || beta == 3 ? -1 : (beta == 1 ? 2 + kq : (kq < 2 ? 6 + kq : kq - 2));
    double* sP = reinterpret_cast<double*>(arena[wave] + kProdOff);
    const int lo = __builtin_amdgcn_readfirstlane(lt);
    if constexpr (PPL == 1) {
      // every block's products first — the two-step chains of four blocks at a time in flight together — then the
      // stores: the matrix-core latency is paid once per four blocks, and the point-data and run-set stores each run
      // under one exec mask instead of one per block
#pragma unroll
      for (int h = 0; h < BW; h += 4) {
        float o[4][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) ops(h + b, o[b]);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          double acc = 0.0;
#pragma unroll
          for (int st = 0; st < 2; ++st)
            acc = __builtin_amdgcn_mfma_f64_4x4x4f64((double)o[b][2 * st], (double)o[b][2 * st + 1], acc, 0, 0, 0);
          accb[h + b] = acc;
        }
      }
    }
    int gpb[BW];  // (read in uniform control flow: a readlane of a lane the exec mask excludes reads a dead register)
#pragma unroll
    for (int b = 0; b < BW; ++b) gpb[b] = __builtin_amdgcn_readlane(gpos, b * LPB);
    if (ppos >= 0) {
#pragma unroll
      for (int b = 0; b < BW; ++b)
        if (b < nbw) blk_schur[(long long)gpb[b] * kPd + ppos] = accb[b];
    }
    double tacc = 0.0;
    int cur = lo;
#pragma unroll
    for (int b = 0; b < BW; ++b) {
      if (b < nbw) {
        const int ltb = __builtin_amdgcn_readlane(lt, b * LPB);
        if (ltb != cur) {
          if (pslot >= 0) sP[(cur - lo) * NQ + pslot] = tacc;
          tacc = 0.0;
          cur = ltb;
        }
        tacc += accb[b];
      }
    }
    if (nbw > 0 && pslot >= 0) sP[(cur - lo) * NQ + pslot] = tacc;
    if (lane == 0) {
      s_wlo[wave] = lo;
      s_wn[wave] = nbw > 0 ? cur - lo + 1 : 0;
    }
  }
#ifdef PBA_ABL_PHASE
  if (n_t > 0) return;
#endif
  __syncthreads();
  // Phase A: the chunk's product sums per local target j, as full 8 × 8 matrices (one thread per entry; the sets of j
  // over the waves in order), and Ad_j from R_th, t_th.  Over wave 0's rows.
  double* sT = reinterpret_cast<double*>(arena[0] + kRowsOff);  // [j][8][8]
  double* sN = reinterpret_cast<double*>(arena[1] + kRowsOff);  // [j][6][6]: H_tt,j·Ad_j
  {
    const int t = threadIdx.x, j = t >> 6, r = (t >> 3) & 7, c = t & 7;
    if (j < n_t && t < 64 * kChunkTargets) {
      const int u = upper8(min(r, c), max(r, c));
      double acc = 0.0;
#pragma unroll
      for (int w_ = 0; w_ < NW; ++w_) {
        const int wl = s_wlo[w_], wn = s_wn[w_];
        if (j >= wl && j < wl + wn) acc += reinterpret_cast<const double*>(arena[w_] + kProdOff)[(j - wl) * NQ + u];
      }
      sT[t] = acc;
    }
    if (t < 36 * n_t) {  // Ad = [[R, [t]×R], [0, R]]; ([t]×R)[q][c] = t[q+1] R[q+2][c] − t[q+2] R[q+1][c] (indices mod 3)
      const int jj = t / 36, e = t - 36 * jj, q = e / 6, p = e - 6 * q;
      const double* rt = s_rt[jj];
      double v = 0.0;
      if (q < 3 && p < 3) {
        v = rt[3 * q + p];
      } else if (q >= 3 && p >= 3) {
        v = rt[3 * (q - 3) + (p - 3)];
      } else if (q < 3) {
        const int c = p - 3, q1 = q == 2 ? 0 : q + 1, q2 = q == 0 ? 2 : q - 1;
        v = rt[9 + q1] * rt[3 * q2 + c] - rt[9 + q2] * rt[3 * q1 + c];
      }
      s_ad[jj][e] = v;
    }
  }
  __syncthreads();
  // Phase B: N_j = H_tt,j·Ad_j; the target outputs — H_ht = −AdᵀH_tt, H_tt, g_t — and g_h = −Σ_j Ad_jᵀ g_t,j
  const int nout = SLOT_LIN_BASE + SLOT_LIN_T * n_t;
  for (int o = threadIdx.x; o < nout; o += NT) {
    if (o < 36) {
      const int r = o / 6, c = o - 6 * (o / 6);
      for (int j = 0; j < n_t; ++j) {
        double v = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) v += sT[64 * j + 8 * r + p] * s_ad[j][6 * p + c];
        sN[36 * j + o] = v;
      }
      continue;
    }
    double v = 0.0;
    if (o < 42) {
      const int r = o - 36;
      for (int j = 0; j < n_t; ++j)
#pragma unroll
        for (int q = 0; q < 6; ++q) v -= s_ad[j][6 * q + r] * sT[64 * j + 8 * q + 7];
    } else {
      const int j = (o - 42) / SLOT_LIN_T, q = (o - 42) - SLOT_LIN_T * j;
      if (q < 36) {
        const int r = q / 6, c = q - 6 * (q / 6);
#pragma unroll
        for (int p = 0; p < 6; ++p) v -= s_ad[j][6 * p + r] * sT[64 * j + 8 * p + c];
      } else if (q < 72) {
        const int r = (q - 36) / 6, c = (q - 36) % 6;
        v = sT[64 * j + 8 * r + c];
      } else {
        v = sT[64 * j + 8 * (q - 72) + 7];
      }
    }
    part_lin[(long long)poff + o] = v;
  }
  __syncthreads();
  if (threadIdx.x < 36) {  // Phase C: H_hh[r][c] = Σ_j Σ_q Ad_j[q][r] N_j[q][c], (r, c) and (c, r) from one sum
    const int o = threadIdx.x, r0 = o / 6, c0 = o - 6 * (o / 6), r = min(r0, c0), c = max(r0, c0);
    double v = 0.0;
    for (int j = 0; j < n_t; ++j)
#pragma unroll
      for (int q = 0; q < 6; ++q) v += s_ad[j][6 * q + r] * sN[36 * j + 6 * q + c];
    part_lin[(long long)poff + o] = v;
  }
  if (live && k == 0) {
    a.valid[blk] = (uint8_t)ok;
    a.cost[blk] = bcost;
  }
  if (g.wg_red && wave == 0) {  // the chunk's (Σ cost, Σ valid): lane b takes block b, xor butterflies (fixed order)
    const float x = lane < count ? s_bc[lane] : -1.0f;
    double cs = x >= 0.0f ? (double)x : 0.0, vs = x >= 0.0f ? 1.0 : 0.0;
    for (int m = 32; m >= 1; m >>= 1) {
      cs += __shfl_xor(cs, m, 64);
      vs += __shfl_xor(vs, m, 64);
    }
    if (lane == 0) {
      g.wg_red[2 * chunk] = cs;
      g.wg_red[2 * chunk + 1] = vs;
    }
  }
}

template <int KIND, int MODEL>  // photometric: MODEL = camera model + 4 · interpolator
void launch_linearize(pba_engine* e, const KernelArgs& ka, const LinArgs& la) {
  const int grid = la.n_chunks;
  if constexpr (KIND == PBA_RESIDUAL_PHOTOMETRIC) {
    if (e->affine) {  // the solve at the engine's affine state (ensure_prepared: pba_gn_set_solve_affine is on)
      switch (e->gn.ppl) {
        case 1: linearize_adj_kernel<MODEL, 1, kBlockThreads, true><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
        case 2: linearize_adj_kernel<MODEL, 2, kBlockThreads, true><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
        case 3: linearize_adj_kernel<MODEL, 3, kBlockThreads, true><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
        default: linearize_adj_kernel<MODEL, 4, kBlockThreads, true><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
      }
    }
    switch (e->gn.ppl) {  // 9…32 px: 8 lanes per block, ⌈P/8⌉ rows per lane
      case 1: break;
      case 2: linearize_adj_kernel<MODEL, 2, kBlockThreads><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
      case 3: linearize_adj_kernel<MODEL, 3, kBlockThreads><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
      default: linearize_adj_kernel<MODEL, 4, kBlockThreads><<<grid, kBlockThreads, 0, e->stream>>>(ka, la); return;
    }
    // the 14-column products of the same rows: the A/B reference of the test build (PBA_TEST_HOOKS, PBA_LIN_LEGACY)
    if (e->gn.lin_legacy) linearize_kernel<KIND, MODEL, 8><<<grid, kBlockThreads, 0, e->stream>>>(ka, la);
    else linearize_adj_kernel<MODEL, 1, kBlockThreads><<<grid, kBlockThreads, 0, e->stream>>>(ka, la);
  } else {
    linearize_kernel<KIND, MODEL, 4><<<grid, kBlockThreads, 0, e->stream>>>(ka, la);
  }
}

}  // namespace

namespace pba {
namespace detail {

void launch_linearize_photometric(pba_engine* e, const KernelArgs& ka, const LinArgs& la) {
  dispatch_pm(e, [&](auto pm) { launch_linearize<PBA_RESIDUAL_PHOTOMETRIC, decltype(pm)::value>(e, ka, la); });
}

void launch_linearize_geometric(pba_engine* e, const KernelArgs& ka, const LinArgs& la) {
  switch (e->opt.camera_model) {
    case PBA_CAMERA_PINHOLE: launch_linearize<PBA_RESIDUAL_GEOMETRIC, CAM_PINHOLE>(e, ka, la); break;
    case PBA_CAMERA_DOUBLE_SPHERE: launch_linearize<PBA_RESIDUAL_GEOMETRIC, CAM_DS>(e, ka, la); break;
    case PBA_CAMERA_EUCM: launch_linearize<PBA_RESIDUAL_GEOMETRIC, CAM_EUCM>(e, ka, la); break;
    default: launch_linearize<PBA_RESIDUAL_GEOMETRIC, CAM_KB4>(e, ka, la); break;
  }
}

}  // namespace detail
}  // namespace pba
