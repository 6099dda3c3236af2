// pba_record.h — the photometric record: its formats, its column layout and the staging of one pixel row.
//
// A block's record over its P pattern pixels is [r | J_host (P×6) | J_target (P×6) | J_ρ | tail]; the tail is the
// format's: none (fp32, PBA_RECORD_F16), the row scales e (PBA_RECORD_F16_SCALED), J_intr (P×8, free intrinsics),
// J_ab_host | J_ab_target (P×2 each, affine brightness) or J_intr followed by the two brightness blocks (both).  The
// block kernels (pba_evaluate.hip) stage their records in LDS through the functions below; the decodes
// (decode_records_kernel, pba_get_records) read the layout from here too.
#pragma once

#include <type_traits>

#include "pba_internal.h"
#include "pba_wave_slab.h"

// The storage tags sit in an unnamed namespace like the kernels they parameterise (a kernel's name carries its tag).
namespace {

// Storage tag of PBA_RECORD_F16_SCALED: halves with one power-of-two scale per pixel row, 15 halves per row
// ([r | J_host | J_target | J_rho | e], pba.h).  RecFormat<T>: what a kernel stores (S) and a record's columns per row.
// Storage tag of the fp32 records with free target intrinsics (pba_set_optimize_intrinsics): 22 floats per row,
// [r | J_host | J_target | J_rho | J_intr (P×8)].
// Storage tag of the fp32 records with affine brightness (pba_set_affine_brightness): 18 floats per row,
// [r | J_host | J_target | J_rho | J_ab_host (P×2) | J_ab_target (P×2)].
// Storage tag of the fp32 records with both (pba_set_intrinsics_with_affine): 26 floats per row,
// [r | J_host | J_target | J_rho | J_intr (P×8) | J_ab_host (P×2) | J_ab_target (P×2)].
struct ScaledF16 {};
struct IntrF32 {};
struct AffineF32 {};
struct IntrAffineF32 {};
template <class Stored, int Cols, bool Scaled = false, bool Intr = false, bool Affine = false>
struct RecLayout {
  using S = Stored;
  static constexpr int kCols = Cols;
  static constexpr bool kScaled = Scaled, kIntr = Intr, kAffine = Affine;
};
template <class T>
struct RecFormat : RecLayout<T, 14> {};
template <>
struct RecFormat<ScaledF16> : RecLayout<_Float16, 15, true> {};
template <>
struct RecFormat<IntrF32> : RecLayout<float, 22, false, true> {};
template <>
struct RecFormat<AffineF32> : RecLayout<float, 18, false, false, true> {};
template <>
struct RecFormat<IntrAffineF32> : RecLayout<float, 26, false, true, true> {};

// every format's entry in the table the host check of the per-wave stores walks (pba_wave_slab.h)
template <class T>
constexpr bool slab_entry_is(int i) {
  return pba::detail::kSlabFormats[i].cols == RecFormat<T>::kCols &&
         pba::detail::kSlabFormats[i].ssize == (int)sizeof(typename RecFormat<T>::S);
}
static_assert(slab_entry_is<float>(0) && slab_entry_is<_Float16>(1) && slab_entry_is<ScaledF16>(2) &&
                  slab_entry_is<IntrF32>(3) && slab_entry_is<AffineF32>(4) && slab_entry_is<IntrAffineF32>(5),
              "pba_wave_slab.h: kSlabFormats");

}  // namespace

namespace pba {
namespace detail {

// Column offsets of a block's record, in stored values, for a pattern of P pixels.  Pixel px has r at col_r + px, its
// J_host and J_target rows at col_jhost + 6·px and col_jtarget + 6·px, J_ρ at col_jrho + px and its tail entries from
// col_tail.  The first col_tail(P) = 14·P columns are every format's, and what a half record decodes to.
__host__ __device__ __forceinline__ constexpr int col_r(int) { return 0; }
__host__ __device__ __forceinline__ constexpr int col_jhost(int P) { return P; }
__host__ __device__ __forceinline__ constexpr int col_jtarget(int P) { return 7 * P; }
__host__ __device__ __forceinline__ constexpr int col_jrho(int P) { return 13 * P; }
__host__ __device__ __forceinline__ constexpr int col_tail(int P) { return 14 * P; }
// the affine tail: J_ab_host (P×2), then J_ab_target (P×2); INTR (the format's kIntr): behind J_intr (P×8 from
// col_tail) in the format that has both — columns 14·P and 16·P of the 18-column record, 22·P and 24·P of the 26-column one
template <bool INTR = false>
__host__ __device__ __forceinline__ constexpr int col_jab_host(int P) {
  if constexpr (INTR) return col_tail(P) + 8 * P;
  else return col_tail(P);
}
template <bool INTR = false>
__host__ __device__ __forceinline__ constexpr int col_jab_target(int P) {
  if constexpr (INTR) return col_tail(P) + 10 * P;
  else return col_tail(P) + 2 * P;
}

// The pixel row whose scale e applies to column c of the decoded record (PBA_RECORD_F16_SCALED: a Jacobian entry of
// pixel row k is stored divided by e[k], at col_tail + k); −1 for the residual columns, which are not scaled.
__host__ __device__ __forceinline__ constexpr int scale_row_of(int c, int P) {
  return c < col_jhost(P) ? -1 : c < col_jrho(P) ? ((c - col_jhost(P)) % (6 * P)) / 6 : c - col_jrho(P);
}

// A record value in the engine's format.  fp16 saturates at ±65504 (the half range) instead of rounding to ±inf: at
// full resolution a strong edge's rotation Jacobian ∇I·∂π/∂p·[b]× reaches ~1e5 intensity units per radian (measured
// up to 9.0e4 on the C5-style problem), so those entries are clamped (pba.h, PBA_RECORD_F16).
template <class T>
__device__ __forceinline__ T rec_val(float v) { return (T)v; }
template <>
__device__ __forceinline__ _Float16 rec_val<_Float16>(float v) {
  // (fmed3 would map NaN to −65504: a NaN stays NaN)
  return (_Float16)(isnan(v) ? v : __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f));
}

// Row px of J_ab_host = [E·(I_h − b_h), E] and J_ab_target = [−E·(I_h − b_h), −1] (2 floats each at col_jab_host + 2·px
// and col_jab_target + 2·px of the block's staged record), g = E·(I_h − b_h): two 8-B LDS writes.  A block's record is
// 72·P bytes and the rows start 56·P + 8·px and 64·P + 8·px into it: 8-B aligned at every P, odd ones included.
// INTR (the format's kIntr): the rows sit behind J_intr — a 104·P-byte record, the rows 88·P + 8·px and 96·P + 8·px into
// it, 8-B aligned at every P as well.
// ok = false: the zero rows of an invalid block.
template <bool INTR = false>
__device__ __forceinline__ void stage_affine(float* s_rec, int P, int px, float g, float E, bool ok) {
  reinterpret_cast<float2*>(s_rec + col_jab_host<INTR>(P))[px] = ok ? make_float2(g, E) : make_float2(0.0f, 0.0f);
  reinterpret_cast<float2*>(s_rec + col_jab_target<INTR>(P))[px] = ok ? make_float2(-g, -1.0f) : make_float2(0.0f, 0.0f);
}

// Row px of J_intr (8 floats at col_tail + 8·px of the block's staged record): two 16-B LDS writes when the row is 16-B
// aligned — a block's record is 88·P bytes (104·P with the brightness blocks behind it: a multiple of 16 for the same P)
// and the row starts 56·P + 32·px into it, so for even P — else four 8-B ones.
__device__ __forceinline__ void stage_intr(float* s_rec, int P, int px, const float (&ji)[8]) {
  float* d = s_rec + col_tail(P) + 8 * px;
  if ((P & 1) == 0) {
    reinterpret_cast<f32x4*>(d)[0] = f32x4{ji[0], ji[1], ji[2], ji[3]};
    reinterpret_cast<f32x4*>(d)[1] = f32x4{ji[4], ji[5], ji[6], ji[7]};
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<float2*>(d)[q] = make_float2(ji[2 * q], ji[2 * q + 1]);
  }
}

// Store a workgroup's contiguous record slab (LDS → global): 16-B non-temporal stores when the slab is 16-B
// aligned, 4-B or 2-B stores otherwise (odd patterns in fp16).
// wt (wave-uniform, KernelArgs::slab_wt): non-temporal write-through stores (`nt sc1`) — for launches of at most one
// wave of workgroups (a 1/8 shard of C4: 8.29 → 8.07-8.15 µs, nothing left dirty in L2 for the kernel's end), never for
// a full C4 launch (44.9 → 46.2 µs), DESIGN.md §3.
// NTH threads share the slab, thread tid of them calling: the workgroup (the default), or one wave storing its own
// run of records (NTH = 64, tid = its lane: photometric_block_kernel, pba_wave_slab.h).
template <class T, int NTH = kBlockThreads>
__device__ __forceinline__ void store_slab(const unsigned char* src, unsigned char* dst, int bytes, int wt = 0,
                                           int tid = threadIdx.x) {
  constexpr int kBlockThreads = NTH;
  if ((((uintptr_t)dst | (unsigned)bytes) & 15) == 0) {
    // non-temporal 16-B stores (write-through sc1 stores measured 49 → 71 µs for this kernel; per-lane stores
    // straight from registers, without the LDS slab, 49 → 104 µs: DESIGN.md §3)
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
    if (wt) {
      for (int i = tid; i < (bytes >> 4); i += kBlockThreads)
        asm volatile("global_store_dwordx4 %0, %1, off nt sc1" ::"v"(d4 + i), "v"(s4[i]) : "memory");
    } else {
      for (int i = tid; i < (bytes >> 4); i += kBlockThreads) __builtin_nontemporal_store(s4[i], d4 + i);
    }
  } else if (sizeof(T) == 4 || (((uintptr_t)dst | (unsigned)bytes) & 3) == 0) {
    const float* s1 = reinterpret_cast<const float*>(src);
    float* d1 = reinterpret_cast<float*>(dst);
#pragma unroll 1
    for (int i = tid; i < (bytes >> 2); i += kBlockThreads) __builtin_nontemporal_store(s1[i], d1 + i);
  } else {
    const _Float16* s1 = reinterpret_cast<const _Float16*>(src);
    _Float16* d1 = reinterpret_cast<_Float16*>(dst);
#pragma unroll 1
    for (int i = tid; i < (bytes >> 1); i += kBlockThreads) d1[i] = s1[i];
  }
}

typedef float rec_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 rec_h2 __attribute__((ext_vector_type(2)));

// Row px of a half record into its LDS stage: c = {r, J_rho}, 3 × J_host pairs, 3 × J_target pairs.  The 6-value rows
// as 4-byte LDS writes where they are 4-byte aligned (LDS issue is what the 21-px kernel waits on: SQ_WAIT_INST_LDS
// ≈ 0.26 of wave time): 3 per row when `even` (the J_host row starts on a 4-byte boundary), else 1 + 2 + 1 with the
// inner pairs re-packed.
__device__ __forceinline__ void stage_halves(_Float16* s_rec, int P, int px, const rec_h2 (&c)[7], bool even) {
  _Float16* h = s_rec + col_jhost(P) + 6 * px;
  _Float16* t = s_rec + col_jtarget(P) + 6 * px;
  s_rec[col_r(P) + px] = c[0].x;
  s_rec[col_jrho(P) + px] = c[0].y;
  if (even) {
    rec_h2* h4 = reinterpret_cast<rec_h2*>(h);
    rec_h2* t4 = reinterpret_cast<rec_h2*>(t);
    h4[0] = c[1]; h4[1] = c[2]; h4[2] = c[3];
    t4[0] = c[4]; t4[1] = c[5]; t4[2] = c[6];
  } else {
    rec_h2* h4 = reinterpret_cast<rec_h2*>(h + 1);
    rec_h2* t4 = reinterpret_cast<rec_h2*>(t + 1);
    h[0] = c[1].x; h4[0] = (rec_h2){c[1].y, c[2].x}; h4[1] = (rec_h2){c[2].y, c[3].x}; h[5] = c[3].y;
    t[0] = c[4].x; t4[0] = (rec_h2){c[4].y, c[5].x}; t4[1] = (rec_h2){c[5].y, c[6].x}; t[5] = c[6].y;
  }
}

// Row px of a PBA_RECORD_F16_SCALED record (pba.h), by the lane that evaluated it: with m the largest magnitude of the
// row's 13 Jacobian values, e = 1 for m < 65520 (every value rounds to a finite half: the row is stored as
// PBA_RECORD_F16 stores it), else e = 2^(⌊log₂ m⌋ − 14) ≤ 2¹⁵, which puts the scaled maximum into [16384, 32768).  The
// multiplication by 1/e is exact, so the one rounding is the half conversion.  Beyond 65504·2¹⁵ the scaled values
// saturate at ±65504.  The residual is not scaled.  s_rec is block lb's record in the 4-byte aligned stage (15·P halves per
// block: an odd P puts every other block on a 2-byte boundary).
__device__ __forceinline__ void stage_row_scaled(_Float16* s_rec, int lb, int P, int px, const Row& row, bool act) {
  const float j[13] = {row.jr, row.hv.x, row.hv.y, row.hv.z, row.hw.x, row.hw.y, row.hw.z,
                       row.tv.x, row.tv.y, row.tv.z, row.tw.x, row.tw.y, row.tw.z};
  float m = 0.0f;  // (a NaN drops out of the max and stays NaN in the record)
#pragma unroll
  for (int q = 0; q < 13; ++q) m = fmaxf(m, fabsf(j[q]));
  int ex = 0;  // e = 2^ex
  if (m >= 65520.0f) ex = min((int)((__float_as_uint(m) >> 23) & 0xffu) - (127 + 14), 15);  // (m = +inf: the cap)
  const float inv = __uint_as_float((unsigned)(127 - ex) << 23);
  // the residual saturates as PBA_RECORD_F16's does (|r| ≤ 255 for 8-bit images)
  const float r = isnan(row.r) ? row.r : __builtin_amdgcn_fmed3f(row.r, -65504.0f, 65504.0f);
  rec_h2 c[7];
  c[0] = __builtin_convertvector((rec_f2){r, j[0] * inv}, rec_h2);
#pragma unroll
  for (int q = 1; q < 7; ++q) c[q] = __builtin_convertvector((rec_f2){j[2 * q - 1] * inv, j[2 * q] * inv}, rec_h2);
  if (ex == 15) {  // the largest scale: a value beyond the format's range rounded to ±inf and saturates
    auto sat = [](_Float16 h) -> _Float16 {
      return __builtin_isinf(h) ? (h > (_Float16)0 ? (_Float16)65504.0f : (_Float16)-65504.0f) : h;
    };
    c[0].y = sat(c[0].y);
#pragma unroll
    for (int q = 1; q < 7; ++q) c[q] = (rec_h2){sat(c[q].x), sat(c[q].y)};
  }
  if (act) {
    stage_halves(s_rec, P, px, c, ((lb + 1) & P & 1) == 0);  // J_host row at half (15·lb + 1)·P + 6·px of the stage
    reinterpret_cast<unsigned short*>(s_rec)[col_tail(P) + px] = (unsigned short)((15 + ex) << 10);  // 2^ex as a half
  }
}

// Row px of a block's staged record (r | J_host row | J_target row | J_rho), one value at a time (rec_val), by the lane
// that evaluated it.  The fp32 form of stage_row, and what the 8-lane kernel (photometric_block_kernel) stages every
// format but the scaled one with, its half records included: staged through stage_row<_Float16> a stored half of its
// P = 8 records changed.
template <class T>
__device__ __forceinline__ void stage_row_each(T* s_rec, int P, int px, const Row& row) {
  T* h = s_rec + col_jhost(P) + 6 * px;
  T* t = s_rec + col_jtarget(P) + 6 * px;
  s_rec[col_r(P) + px] = rec_val<T>(row.r);
  h[0] = rec_val<T>(row.hv.x); h[1] = rec_val<T>(row.hv.y); h[2] = rec_val<T>(row.hv.z);
  h[3] = rec_val<T>(row.hw.x); h[4] = rec_val<T>(row.hw.y); h[5] = rec_val<T>(row.hw.z);
  t[0] = rec_val<T>(row.tv.x); t[1] = rec_val<T>(row.tv.y); t[2] = rec_val<T>(row.tv.z);
  t[3] = rec_val<T>(row.tw.x); t[4] = rec_val<T>(row.tw.y); t[5] = rec_val<T>(row.tw.z);
  s_rec[col_jrho(P) + px] = rec_val<T>(row.jr);
}

// Row px of a block's staged record (r | J_host row | J_target row | J_rho; T = float or _Float16), written by the lane
// that evaluated it when act.  Every lane of the wave calls it (the fp16 form's saturation test is a ballot).
template <class T>
__device__ __forceinline__ void stage_row(T* s_rec, int P, int px, const Row& row, bool act) {
  if constexpr (std::is_same<T, _Float16>::value) {
    // fp16 records: the 14 values in 7 packed round-to-nearest conversions (v_cvt_pk_f16_f32) instead of a
    // NaN-preserving clamp + conversion each; a value beyond the half range rounds to ±inf there, which rec_val
    // saturates to ±65504 — applied afterwards, only when some lane of the wave has one (a ballot)
    typedef rec_f2 f2;
    typedef rec_h2 h2;
    const float v[14] = {row.r, row.jr, row.hv.x, row.hv.y, row.hv.z, row.hw.x, row.hw.y, row.hw.z,
                         row.tv.x, row.tv.y, row.tv.z, row.tw.x, row.tw.y, row.tw.z};
    h2 c[7];
    // a value rounds to ±inf in half precision iff |v| ≥ 65520: one max over the 14 magnitudes (v_max3 with abs
    // modifiers; a NaN drops out of the max and stays NaN) instead of a class test per converted half
    float m = 0.0f;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      c[q] = __builtin_convertvector((f2){v[2 * q], v[2 * q + 1]}, h2);
      m = fmaxf(m, fmaxf(fabsf(v[2 * q]), fabsf(v[2 * q + 1])));
    }
    const bool big = m >= 65520.0f;
    if (__ballot(act && big) != 0) {
      auto sat = [](_Float16 h) -> _Float16 {
        return __builtin_isinf(h) ? (h > (_Float16)0 ? (_Float16)65504.0f : (_Float16)-65504.0f) : h;
      };
#pragma unroll
      for (int q = 0; q < 7; ++q) c[q] = (h2){sat(c[q].x), sat(c[q].y)};
    }
    // (14·P halves per block: the J_host row starts on a 4-byte boundary for even P)
    if (act) stage_halves(s_rec, P, px, c, (P & 1) == 0);
  } else if (act) {
    stage_row_each(s_rec, P, px, row);
  }
}

}  // namespace detail
}  // namespace pba
