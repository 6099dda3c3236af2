// pba_affine.hip — the brightness solve at fixed poses and inverse distances (include/pba.h pba_affine_*,
// pba_solve_affine): photometric engines with pba_set_affine_brightness.
//
// With h the block's host, t its target, E = exp(a_t − a_h), c_k = I_h,k − b_h and r_k the affine residual, the
// brightness Jacobian of a row is J_ab_host = [E·c_k, E], J_ab_target = [−E·c_k, −1]: a block's whole contribution to
// the (a, b) normal equations is Σc², Σc, Σc·r, Σr over its rows, its Huber weight w = ρ′(Σr²) (Ceres' Corrector with
// ρ″ ≤ 0: J̃ = √ρ′ J, r̃ = √ρ′ r, corrector.cc:42-110) and E:
//   H_hh = w·E²·[[Σc², Σc], [Σc, P]]        H_tt = w·[[E²Σc², EΣc], [EΣc, P]]
//   H_ht = −w·[[E²Σc², EΣc], [E²Σc, E·P]]    g_h = w·E·[Σcr, Σr]    g_t = −w·[EΣcr, Σr]
// affine_moments_kernel evaluates the rows residual-only and writes one fp64 record per block; every sum across
// blocks is fp64 in the fixed order of the host-built lists (pba_affine_plan.h), no atomics; the system is a
// 2×2-block lower skyline, damped as Ceres' LM strategy does (levenberg_marquardt_strategy.cc) and factored by one
// wave (affine_factor_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pba_affine_plan.h"
#include "pba_host_lm.h"
#include "pba_internal.h"

using namespace pba;
using namespace pba::detail;

namespace {

constexpr int kRec = 8;    // doubles per block record: w, E, Σc², Σc, Σcr, Σr, cost, valid
constexpr int kPair = 16;  // doubles per pair record

// Lane = (block, pixel k) for P ≤ 8; 8 lanes per block with ⌈P/8⌉ rows per lane beyond (the cost kernels' layout; the
// row count is a launch scalar, so one instantiation per camera model × interpolator).  Fused-state prologue
// (a.poses) or the pair table, as stage_tile decides.  ρ′ and the block's validity are formed as the linearisation forms
// them: fp32 Σr² per lane over its rows, the DPP group sum, huber_weight.
template <int PM>
__global__ __launch_bounds__(kBlockThreads) void affine_moments_kernel(const KernelArgs a, double* __restrict__ rec,
                                                                      int ppl) {
  constexpr int LPB = 8, BPW = kBlockThreads / LPB;
  __shared__ __attribute__((aligned(16))) TileBlock s_tb[BPW];
  __shared__ float2 s_pat[PBA_MAX_PATTERN];
  const int P = a.P;
  const int blk0 = logical_tile() * BPW;
  const int lb = threadIdx.x / LPB, k = threadIdx.x % LPB;
  const int blk = blk0 + lb;
  const bool live = blk < a.n_blocks;
  const int bq = live ? blk : a.n_blocks - 1;  // a dead block evaluates the last block, masked below
  for (int i = threadIdx.x; i < P; i += kBlockThreads) s_pat[i] = make_float2(a.pattern[2 * i], a.pattern[2 * i + 1]);
  const int pt = stage_tile<LPB>(a, s_tb, lb, k, blk, live);
  const Affine af = block_affine(a, bq);
  __syncthreads();
  int okl = 1;
  float s = 0.0f;
  double c2 = 0.0, c1 = 0.0, cr = 0.0, r1 = 0.0;
  for (int j = 0; j < ppl; ++j) {
    const int px = k + LPB * j;
    const bool act = live && px < P;
    const float Ih = act ? a.host_int[(long long)pt * P + px] : 0.0f;
    const Row row = photometric_row<PM, false, TileBlock, false, false, true>(a, s_tb[lb], s_pat[act ? px : 0], Ih,
                                                                               nullptr, nullptr, &af);
    const bool use = act && row.ok;
    okl &= act ? row.ok : 1;
    s += use ? row.r * row.r : 0.0f;
    const double c = use ? (double)(Ih - af.bh) : 0.0, r = use ? (double)row.r : 0.0;  // (products of floats: exact)
    c2 += c * c;
    c1 += c;
    cr += c * r;
    r1 += r;
  }
  const int ok = group_all<LPB>(okl);
  s = group_sum<LPB>(s);
#pragma unroll
  for (int m = 1; m < LPB; m <<= 1) {  // xor butterflies over the block's lanes: a fixed order
    c2 += __shfl_xor(c2, m, 64);
    c1 += __shfl_xor(c1, m, 64);
    cr += __shfl_xor(cr, m, 64);
    r1 += __shfl_xor(r1, m, 64);
  }
  const float w = ok ? huber_weight(s, a.huber) : 0.0f;
  const float bc = ok ? huber_cost(s, a.huber) : 0.0f;
  if (live && k == 0) {
    double* o = rec + (long long)blk * kRec;
    o[0] = (double)w;
    o[1] = ok ? (double)af.E : 0.0;
    o[2] = ok ? c2 : 0.0;
    o[3] = ok ? c1 : 0.0;
    o[4] = ok ? cr : 0.0;
    o[5] = ok ? r1 : 0.0;
    o[6] = (double)bc;
    o[7] = ok ? 1.0 : 0.0;
  }
  if (a.wg_red) {
    const bool one = live && k == 0;
    wg_reduce2(one ? (double)bc : 0.0, one && ok ? 1.0 : 0.0, a.wg_red + 2 * logical_tile());
  }
}

// One thread per pair: its blocks' contributions in block order.
__global__ void affine_pair_kernel(const double* __restrict__ rec, const int* __restrict__ pair_ptr,
                                   const int* __restrict__ pair_blocks, double P, int n_pairs, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  double v[kPair];
#pragma unroll
  for (int i = 0; i < kPair; ++i) v[i] = 0.0;
  for (int q = pair_ptr[p]; q < pair_ptr[p + 1]; ++q) {
    const double* b = rec + (long long)pair_blocks[q] * kRec;
    const double w = b[0], E = b[1], c2 = b[2], c1 = b[3], cr = b[4], r1 = b[5];
    if (!(w > 0.0)) continue;
    const double E2 = E * E;
    v[0] += w * E2 * c2; v[1] += w * E2 * c1; v[2] += w * E2 * P;       // H_hh: [0 1; 1 2]
    v[3] += w * E2 * c2; v[4] += w * E * c1;  v[5] += w * P;            // H_tt: [3 4; 4 5]
    v[6] -= w * E2 * c2; v[7] -= w * E * c1;                            // H_ht rows (a_h, b_h) × columns (a_t, b_t)
    v[8] -= w * E2 * c1; v[9] -= w * E * P;
    v[10] += w * E * cr; v[11] += w * E * r1;                           // g_h
    v[12] -= w * E * cr; v[13] -= w * r1;                               // g_t
  }
#pragma unroll
  for (int i = 0; i < kPair; ++i) out[(long long)p * kPair + i] = v[i];
}

struct AsmArgsAb {
  const double* pair_rec;
  const int *frame_ptr, *frame_pairs, *first, *row, *off_ptr, *off_pairs;
  double *S0, *g;
  int n_frames, n_sky;
};

// Units [0, n_frames): keyframe i's diagonal block and gradient, its pairs as host, then as target.  Units
// [n_frames, n_frames + n_sky): skyline block s, off the diagonal, its pairs in order (H_ht, or its transpose where the
// pair's host is the block's column).  Undamped, nothing fixed yet (affine_damp_kernel).
__global__ void affine_assemble_kernel(const AsmArgsAb a) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < a.n_frames) {
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, g0 = 0.0, g1 = 0.0;
    for (int q = a.frame_ptr[u]; q < a.frame_ptr[u + 1]; ++q) {
      const int e = a.frame_pairs[q];
      const double* v = a.pair_rec + (long long)(e >> 1) * kPair;
      const int o = (e & 1) ? 3 : 0, og = (e & 1) ? 12 : 10;
      d0 += v[o]; d1 += v[o + 1]; d2 += v[o + 2];
      g0 += v[og]; g1 += v[og + 1];
    }
    double* S = a.S0 + 4 * (long long)(a.row[u] + (u - a.first[u]));
    S[0] = d0; S[1] = d1; S[2] = d1; S[3] = d2;
    a.g[2 * u] = g0;
    a.g[2 * u + 1] = g1;
  } else if (u < a.n_frames + a.n_sky) {
    const int s = u - a.n_frames;
    if (a.off_ptr[s] == a.off_ptr[s + 1]) {
      // (a diagonal block — written above — or an envelope block no pair fills; the diagonal ones are told apart by row)
      int lo = 0, hi = a.n_frames - 1;  // the block row of s: the last i with row[i] ≤ s
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.row[mid] <= s) lo = mid; else hi = mid - 1;
      }
      if (s - a.row[lo] + a.first[lo] == lo) return;
    }
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;  // rows: the block row's (a, b); columns: the block column's
    for (int q = a.off_ptr[s]; q < a.off_ptr[s + 1]; ++q) {
      const int e = a.off_pairs[q];
      const double* v = a.pair_rec + (long long)(e >> 1) * kPair + 6;
      if (e & 1) { m0 += v[0]; m1 += v[2]; m2 += v[1]; m3 += v[3]; }  // host = column: H_htᵀ
      else { m0 += v[0]; m1 += v[1]; m2 += v[2]; m3 += v[3]; }
    }
    double* S = a.S0 + 4 * (long long)s;
    S[0] = m0; S[1] = m1; S[2] = m2; S[3] = m3;
  }
}

// constant keyframes: the requested ones and those without a valid block (a zero diagonal: w > 0, E > 0 and P > 0
// make S0's (b, b) entry positive as soon as one block is valid)
__device__ __forceinline__ bool ab_constant(const double* S0, const int* first, const int* row, const uint8_t* fixed, int i) {
  return fixed[i] != 0 || !(S0[4 * (long long)(row[i] + (i - first[i])) + 3] > 0.0);
}

// L ← S0 + λ·clamp(diag S0, 1e-6, 1e32) with identity rows and columns for the constant keyframes; one thread per
// skyline block (the block row found by bisection).
__global__ void affine_damp_kernel(const double* __restrict__ S0, const int* __restrict__ first,
                                   const int* __restrict__ row, const uint8_t* __restrict__ fixed, int n_frames, int n_sky,
                                   double lambda, double* __restrict__ L) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sky) return;
  int lo = 0, hi = n_frames - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row[mid] <= s) lo = mid; else hi = mid - 1;
  }
  const int i = lo, j = first[i] + (s - row[i]);
  const bool ci = ab_constant(S0, first, row, fixed, i), cj = ab_constant(S0, first, row, fixed, j);
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = S0[4 * (long long)s + q];
  if (i == j) {
    if (ci) {
      v[0] = 1.0; v[1] = 0.0; v[2] = 0.0; v[3] = 1.0;
    } else {
      v[0] += lambda * fmin(fmax(v[0], 1e-6), 1e32);
      v[3] += lambda * fmin(fmax(v[3], 1e-6), 1e32);
    }
  } else if (ci || cj) {
    v[0] = v[1] = v[2] = v[3] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) L[4 * (long long)s + q] = v[q];
}

struct FactorArgs {
  double* L;          // damped skyline, factored in place (lower Cholesky factor, 2×2 blocks row-major)
  const double* S0;   // undamped (for D and the constant keyframes)
  const double* g;
  const int *first, *row;
  const uint8_t* fixed;
  double* x;          // step δ (2 per keyframe)
  double* out;        // status, model decrease ½(λ δᵀDδ − gᵀδ), max|δ|, δᵀδ
  const double* ab;   // state, ab_new ← ab + δ
  double* ab_new;
  double lambda;
  int n_frames;
};

// Scalar entry (r, c), c ≤ r, of the skyline: block row r / 2, block column c / 2.
__device__ __forceinline__ long long sky_at(const int* first, const int* row, int r, int c) {
  const int i = r >> 1, j = c >> 1;
  return 4 * (long long)(row[i] + (j - first[i])) + 2 * (r & 1) + (c & 1);
}

// One wave: row-by-row (left-looking) Cholesky of the skyline in place, the dot products over the lanes with xor
// butterflies (a fixed order: bitwise reproducible), then forward and backward substitution of −g, the candidate state
// and the model decrease.  The current row lives in LDS (dynamic: the widest row), the finished rows in global memory.
// status 1 and no candidate when a pivot is not positive (or not finite).
__global__ __launch_bounds__(64) void affine_factor_kernel(const FactorArgs a) {
  extern __shared__ double s_row[];  // max_row doubles
  const int lane = threadIdx.x, n = 2 * a.n_frames;
  auto wsum = [](double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
  };
  auto sync = []() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  int bad = 0;
  for (int r = 0; r < n && !bad; ++r) {
    const int fr = 2 * a.first[r >> 1];  // first scalar column of row r
    for (int c = fr + lane; c <= r; c += 64) s_row[c - fr] = a.L[sky_at(a.first, a.row, r, c)];
    sync();
    for (int c = fr; c <= r; ++c) {
      const int fc = 2 * a.first[c >> 1], lo = max(fr, fc);
      double acc = 0.0;
      for (int q = lo + lane; q < c; q += 64)  // (row r itself is final only in LDS)
        acc += s_row[q - fr] * (c == r ? s_row[q - fr] : a.L[sky_at(a.first, a.row, c, q)]);
      acc = wsum(acc);
      const double v = s_row[c - fr] - acc;
      double l;
      if (c == r) {
        if (!(v > 0.0) || !isfinite(v)) {
          bad = 1;
          break;
        }
        l = sqrt(v);
      } else {
        l = v / a.L[sky_at(a.first, a.row, c, c)];
      }
      sync();  // every lane has read s_row[c − fr] before lane 0 replaces it
      if (lane == 0) s_row[c - fr] = l;
      sync();
    }
    if (bad) break;
    for (int c = fr + lane; c <= r; c += 64) a.L[sky_at(a.first, a.row, r, c)] = s_row[c - fr];
    sync();
  }
  if (bad) {
    if (lane == 0) {
      a.out[0] = 1.0;
      a.out[1] = a.out[2] = a.out[3] = 0.0;
    }
    return;
  }
  // forward: L y = −g (constant keyframes: zero right-hand side), y in x
  for (int r = 0; r < n; ++r) {
    const int fr = 2 * a.first[r >> 1];
    double acc = 0.0;
    for (int q = fr + lane; q < r; q += 64) acc += a.L[sky_at(a.first, a.row, r, q)] * a.x[q];
    acc = wsum(acc);
    if (lane == 0) {
      const bool cst = ab_constant(a.S0, a.first, a.row, a.fixed, r >> 1);
      a.x[r] = ((cst ? 0.0 : -a.g[r]) - acc) / a.L[sky_at(a.first, a.row, r, r)];
    }
    sync();
  }
  // backward: Lᵀ δ = y, column-oriented
  for (int r = n - 1; r >= 0; --r) {
    const int fr = 2 * a.first[r >> 1];
    const double xr = a.x[r] / a.L[sky_at(a.first, a.row, r, r)];
    sync();  // every lane has read x[r]
    if (lane == 0) a.x[r] = xr;
    for (int q = fr + lane; q < r; q += 64) a.x[q] -= a.L[sky_at(a.first, a.row, r, q)] * xr;
    sync();
  }
  // candidate, model decrease ½(λ δᵀDδ − gᵀδ) with D = clamp(diag S0) over the free keyframes, step norms
  double dD = 0.0, gd = 0.0, mx = 0.0, dd = 0.0;
  for (int r = lane; r < n; r += 64) {
    const bool cst = ab_constant(a.S0, a.first, a.row, a.fixed, r >> 1);
    const double d = cst ? 0.0 : a.x[r];
    if (cst) a.x[r] = 0.0;
    a.ab_new[r] = a.ab[r] + d;
    const int i = r >> 1;
    const double diag = a.S0[4 * (long long)(a.row[i] + (i - a.first[i])) + 3 * (r & 1)];
    dD += cst ? 0.0 : d * d * fmin(fmax(diag, 1e-6), 1e32);
    gd += cst ? 0.0 : a.g[r] * d;
    mx = fmax(mx, fabs(d));
    dd += d * d;
  }
  dD = wsum(dD);
  gd = wsum(gd);
  dd = wsum(dd);
  for (int m = 32; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m, 64));
  if (lane == 0) {
    a.out[0] = 0.0;
    a.out[1] = 0.5 * (a.lambda * dD - gd);
    a.out[2] = mx;
    a.out[3] = dd;
  }
}

int ready(pba_engine* e) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC || !e->affine)
    return fail(PBA_ERR_INVALID_ARGUMENT, "the brightness solve needs a photometric engine with pba_set_affine_brightness");
  // its kernels read 18-column brightness columns and project with the cameras: not the 26-column engine's residual
  if (int rc = solve_refuses_both(e)) return rc;
  if (e->n_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  if (!e->state_set) return fail(PBA_ERR_NOT_READY, "pba_set_state first");
  if (!e->have_images || e->P <= 0) return fail(PBA_ERR_NOT_READY, "images/pattern missing");
  if (int rc = check_device(e)) return rc;
  AffineSolve& A = e->aff;
  if (!A.planned) {
    AffinePlanInput in;
    in.n_frames = e->n_frames;
    in.n_pairs = e->n_pairs;
    in.n_blocks = e->n_blocks;
    in.pair_host = e->pair_host_h.data();
    in.pair_target = e->pair_target_h.data();
    in.block_pair = e->pair_of_h.data();
    AffinePlan P;
    if (!build_affine_plan(in, P)) return fail(PBA_ERR_INVALID_ARGUMENT, "inconsistent pairs");
    PBA_HIP(A.pair_ptr.upload(P.pair_ptr, e->stream));
    PBA_HIP(A.pair_blocks.upload(P.pair_blocks, e->stream));
    PBA_HIP(A.frame_ptr.upload(P.frame_ptr, e->stream));
    PBA_HIP(A.frame_pairs.upload(P.frame_pairs, e->stream));
    PBA_HIP(A.first.upload(P.first, e->stream));
    PBA_HIP(A.row.upload(P.row, e->stream));
    PBA_HIP(A.off_ptr.upload(P.off_ptr, e->stream));
    PBA_HIP(A.off_pairs.upload(P.off_pairs, e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));  // (the plan's vectors die with this scope)
    A.n_sky = P.n_sky;
    A.max_row = P.max_row;
    A.first_h = P.first;
    A.row_h = P.row;
    const size_t nf = e->n_frames;
    PBA_HIP(A.rec.resize((size_t)e->n_blocks * kRec));
    PBA_HIP(A.pair_rec.resize((size_t)std::max(e->n_pairs, 1) * kPair));
    PBA_HIP(A.S0.resize(4 * (size_t)A.n_sky));
    PBA_HIP(A.L.resize(4 * (size_t)A.n_sky));
    PBA_HIP(A.g.resize(2 * nf));
    PBA_HIP(A.x.resize(2 * nf));
    PBA_HIP(A.ab_new.resize(2 * nf));
    PBA_HIP(A.out.resize(4));
    PBA_HIP(A.red.resize(2 * ((size_t)e->n_blocks / 16 + 2)));
    A.planned = true;
    A.linearized = A.have_step = false;
  }
  std::vector<uint8_t> f = A.fixed_h;
  f.resize(e->n_frames, 0);
  if (A.fixed.n < f.size() || !A.linearized) {  // (uploaded before every linearisation: a few bytes per keyframe)
    PBA_HIP(A.fixed.upload(f, e->stream));
    PBA_HIP(hipStreamSynchronize(e->stream));
  }
  return PBA_OK;
}

int linearize_ab(pba_engine* e, double* cost) {
  AffineSolve& A = e->aff;
  KernelArgs ka = make_kernel_args(e, e->pairs.p, e->rho.p);
  ka.poses = e->poses.p;  // the fused-state prologue, as the public evaluations
  ka.wg_red = A.red.p;
  const int grid = (int)(((long long)e->n_blocks * 8 + kBlockThreads - 1) / kBlockThreads);
  dispatch_pm(e, [&](auto pm) {
    affine_moments_kernel<decltype(pm)::value><<<grid, kBlockThreads, 0, e->stream>>>(ka, A.rec.p, (e->P + 7) / 8);
  });
  PBA_HIP(hipGetLastError());
  if (e->n_pairs > 0)
    affine_pair_kernel<<<(e->n_pairs + 255) / 256, 256, 0, e->stream>>>(A.rec.p, A.pair_ptr.p, A.pair_blocks.p, (double)e->P,
                                                                        e->n_pairs, A.pair_rec.p);
  AsmArgsAb aa{A.pair_rec.p, A.frame_ptr.p, A.frame_pairs.p, A.first.p, A.row.p, A.off_ptr.p, A.off_pairs.p,
               A.S0.p, A.g.p, e->n_frames, A.n_sky};
  affine_assemble_kernel<<<(e->n_frames + A.n_sky + 255) / 256, 256, 0, e->stream>>>(aa);
  PBA_HIP(hipGetLastError());
  A.linearized = true;
  A.have_step = false;
  double c = 0.0;
  if (int rc = sum_red(e, A.red.p, grid, &c, nullptr)) return rc;
  if (cost) *cost = c;
  return PBA_OK;
}

int step_ab(pba_engine* e, double lambda, double* model, int* status, double* max_step, double* sq_step) {
  AffineSolve& A = e->aff;
  affine_damp_kernel<<<(A.n_sky + 255) / 256, 256, 0, e->stream>>>(A.S0.p, A.first.p, A.row.p, A.fixed.p, e->n_frames,
                                                                  A.n_sky, lambda, A.L.p);
  FactorArgs fa{A.L.p, A.S0.p, A.g.p, A.first.p, A.row.p, A.fixed.p, A.x.p, A.out.p, e->affine_state.p, A.ab_new.p,
                lambda, e->n_frames};
  affine_factor_kernel<<<1, 64, sizeof(double) * (size_t)std::max(A.max_row, 2), e->stream>>>(fa);
  PBA_HIP(hipGetLastError());
  double o[4];
  PBA_HIP(hipMemcpyAsync(o, A.out.p, sizeof(o), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  const int st = o[0] != 0.0 ? 1 : 0;
  A.have_step = st == 0;
  if (status) *status = st;
  if (model) *model = o[1];
  if (max_step) *max_step = o[2];
  if (sq_step) *sq_step = o[3];
  return PBA_OK;
}

int candidate_cost_ab(pba_engine* e, double* cost) {
  int slots = 0;
  if (int rc = launch_cost_only(e, e->pairs.p, e->rho.p, e->aff.red.p, &slots, e->poses.p, nullptr, nullptr, e->aff.ab_new.p))
    return rc;
  return sum_red(e, e->aff.red.p, slots, cost, nullptr);
}

int accept_ab(pba_engine* e) {
  PBA_HIP(hipMemcpyAsync(e->affine_state.p, e->aff.ab_new.p, sizeof(double) * 2 * (size_t)e->n_frames,
                         hipMemcpyDeviceToDevice, e->stream));
  e->aff.linearized = e->aff.have_step = false;
  e->joint.linearized = false;
  e->evaluated = false;
  e->res_fresh = false;
  return PBA_OK;
}

// max |g| and ‖x‖ over the free (a, b): the norms of the LM loop
int free_norms(pba_engine* e, double* gmax, double* xnorm) {
  AffineSolve& A = e->aff;
  const size_t nf = e->n_frames;
  std::vector<double> g(2 * nf), ab(2 * nf), S((size_t)4 * A.n_sky);
  PBA_HIP(hipMemcpyAsync(g.data(), A.g.p, sizeof(double) * g.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipMemcpyAsync(ab.data(), e->affine_state.p, sizeof(double) * ab.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipMemcpyAsync(S.data(), A.S0.p, sizeof(double) * S.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  double gm = 0.0, xx = 0.0;
  for (size_t i = 0; i < nf; ++i) {
    const bool fixed = i < A.fixed_h.size() && A.fixed_h[i];
    if (fixed || !(S[4 * (size_t)(A.row_h[i] + ((int)i - A.first_h[i])) + 3] > 0.0)) continue;
    for (int q = 0; q < 2; ++q) {
      gm = std::max(gm, std::fabs(g[2 * i + q]));
      xx += ab[2 * i + q] * ab[2 * i + q];
    }
  }
  *gmax = gm;
  *xnorm = std::sqrt(xx);
  return PBA_OK;
}

}  // namespace

extern "C" {

int pba_set_fixed_affine_frames(pba_engine* e, int32_t n, const int32_t* frames) {
  if (!e || n < 0 || (n > 0 && !frames)) return fail(PBA_ERR_INVALID_ARGUMENT, "bad fixed-frame arguments");
  if (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC || !e->affine)
    return fail(PBA_ERR_INVALID_ARGUMENT, "the brightness solve needs a photometric engine with pba_set_affine_brightness");
  if (e->n_frames <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_frames first");
  std::vector<uint8_t> f(e->n_frames, 0);
  for (int i = 0; i < n; ++i) {
    if (frames[i] < 0 || frames[i] >= e->n_frames) return fail(PBA_ERR_INVALID_ARGUMENT, "fixed frame out of range");
    f[frames[i]] = 1;
  }
  e->aff.fixed_h = f;
  e->aff.linearized = e->aff.have_step = false;
  e->joint.linearized = false;
  return PBA_OK;
}

int pba_affine_linearize(pba_engine* e, double* cost) {
  if (int rc = ready(e)) return rc;
  return linearize_ab(e, cost);
}

int pba_affine_system_size(pba_engine* e, int32_t* n) {
  if (int rc = ready(e)) return rc;
  if (!n) return fail(PBA_ERR_INVALID_ARGUMENT, "null size");
  *n = 2 * e->n_frames;
  return PBA_OK;
}

int pba_affine_get_system(pba_engine* e, double* H_dense, double* g) {
  if (int rc = ready(e)) return rc;
  AffineSolve& A = e->aff;
  if (!A.linearized) return fail(PBA_ERR_NOT_READY, "pba_affine_linearize first");
  const int nf = e->n_frames;
  const size_t n = 2 * (size_t)nf;
  std::vector<double> S((size_t)4 * A.n_sky), gh(n);
  PBA_HIP(hipMemcpyAsync(S.data(), A.S0.p, sizeof(double) * S.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipMemcpyAsync(gh.data(), A.g.p, sizeof(double) * n, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  std::vector<uint8_t> cst(nf);
  for (int i = 0; i < nf; ++i)
    cst[i] = (i < (int)A.fixed_h.size() && A.fixed_h[i]) || !(S[4 * (size_t)(A.row_h[i] + (i - A.first_h[i])) + 3] > 0.0);
  if (H_dense)  // (identity rows and columns for the constant keyframes)
    skyline_to_dense<2>(S, A.first_h, A.row_h, nf, false, [&](int i, int j, int r, int c, double v) {
      return cst[i] || cst[j] ? (i == j && r == c ? 1.0 : 0.0) : v;
    }, H_dense);
  if (g)
    for (size_t i = 0; i < n; ++i) g[i] = cst[i / 2] ? 0.0 : gh[i];
  return PBA_OK;
}

int pba_affine_step(pba_engine* e, double lambda, double* model_decrease, int32_t* solver_status) {
  if (int rc = ready(e)) return rc;
  if (!(lambda >= 0.0)) return fail(PBA_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
  if (!e->aff.linearized) return fail(PBA_ERR_NOT_READY, "pba_affine_linearize first");
  int st = 0;
  const int rc = step_ab(e, lambda, model_decrease, &st, nullptr, nullptr);
  if (solver_status) *solver_status = st;
  return rc;
}

int pba_affine_get_step(pba_engine* e, double* d_ab) {
  if (int rc = ready(e)) return rc;
  if (!d_ab) return fail(PBA_ERR_INVALID_ARGUMENT, "null step");
  if (!e->aff.have_step) return fail(PBA_ERR_NOT_READY, "pba_affine_step first");
  PBA_HIP(hipMemcpyAsync(d_ab, e->aff.x.p, sizeof(double) * 2 * (size_t)e->n_frames, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_affine_candidate_cost(pba_engine* e, double* cost) {
  if (int rc = ready(e)) return rc;
  if (!cost) return fail(PBA_ERR_INVALID_ARGUMENT, "null cost");
  if (!e->aff.have_step) return fail(PBA_ERR_NOT_READY, "pba_affine_step first");
  return candidate_cost_ab(e, cost);
}

int pba_affine_accept(pba_engine* e) {
  if (int rc = ready(e)) return rc;
  if (!e->aff.have_step) return fail(PBA_ERR_NOT_READY, "pba_affine_step first");
  return accept_ab(e);
}

// The host-driven trust-region loop (pba_host_lm.h); norms over the free (a, b).
int pba_solve_affine(pba_engine* e, const pba_solver_options* o, pba_solver_summary* sum) {
  if (int rc = ready(e)) return rc;
  HostLmStages stages{
      [&](double* cost, double* gmax, double* x_norm) {
        if (int rc = linearize_ab(e, cost)) return rc;
        return free_norms(e, gmax, x_norm);
      },
      [&](double lambda, int* status, double* model, double* sq_step) {
        return step_ab(e, lambda, model, status, nullptr, sq_step);
      },
      [&](double* cost) { return candidate_cost_ab(e, cost); },
      [&]() { return accept_ab(e); }};
  return host_lm(o, stages, e->gn.history, sum);
}

}  // extern "C"
