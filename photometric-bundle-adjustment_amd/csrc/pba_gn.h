// pba_gn.h — what the Gauss-Newton device units share: pba_gn.hip (elimination, assembly, update), pba_gn_lm.hip (the LM
// driver; its interface with pba_gn.hip is pba_gn_lm.h), pba_gn_linearize.hip (the linearisation), pba_gn_intr.hip (free
// intrinsics; its own interface is pba_gn_intr.h) and pba_gn_solve_cr.hip (v4f64; the solvers' own interface is
// pba_gn_solve.h).  The layout constants that the host-only symbolic analysis (pba_gn_plan.cpp) shares with them come
// from pba_gn_plan.h, the LM record's fields from pba_gn_lm_record.h (no HIP either).
// The pipeline of a trial is described in pba_gn.hip.
#pragma once

#include "pba_gn_lm_record.h"
#include "pba_gn_plan.h"
#include "pba_internal.h"

namespace pba {
namespace detail {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int kPd = 8;            // point data per GN block: [H_ρρ, g_ρ, W_t(6)] (blk_schur)
// (SLOT_LIN_*, kChunkTargets, SCHUR_PTS, SCHUR_W, C_*: pba_gn_plan.h, shared with the host-only plan unit)

// (the LM decision record's fields kLm* and done reasons kDone*: pba_gn_lm_record.h)
// The kernels always get a record: the device loop's, or — host-driven steps — GnData::lm_idle (not done, set 0, λ NaN
// = use the kernel's λ argument).  They read it with their first loads, never behind a branch of its own (a gate
// read before anything else cost the linearisation ~8 µs of serialised scalar round trips).
struct LmView {
  double done, set, lambda, accept;
};
__device__ __forceinline__ LmView lm_view(const double* lm) {
  return LmView{lm[kLmDone], lm[kLmSet], lm[kLmLambda], lm[kLmAccept]};
}
// λ of a kernel: the record's, or — NaN there, host-driven steps — the kernel's argument
__device__ __forceinline__ double lm_lambda(const LmView& v, double lambda) { return isnan(v.lambda) ? lambda : v.lambda; }

// Multi-GPU exchange: the tail of a row after its blocks (export_band_kernel, and the border rows of pba_gn_intr.hip)
constexpr int EX_TAIL = 24;  // g(6) | g_direct(6) | diag(A)(6) | observed | pad

struct LinArgs {
  const int4* lin_rec;      // chunk slot → {block, point, pair | local target slot << 24, GN position (blk_schur index)}
  double* blk_schur1;       // the second buffer set (device LM loop: the candidate's linearisation goes to the spare)
  double* part_lin1;
  double* wg_red;           // per-chunk (Σ cost, Σ valid) slots, or nullptr
  const int4* chunk_desc;   // first linearise position, count, n_targets, partial offset (slots)
  double* blk_schur;
  double* part_lin;
  int n_chunks;
  const double* lm;         // LM record: skip when the solve is done; spare: write the set the record does not hold
  bool spare;
  int* lin_set;             // or nullptr: the set written (workgroup 0 stores it, and clears degen[set])
  int* degen;
  double* pair_rt;          // per pair [R_th(9), t_th(3)] of the linearisation (set 0 / set 1): schur_chunk forms
  double* pair_rt1;         // W_h = −W_t·Ad from them
};

// pba_gn_linearize.hip: the linearisation's launch for the engine's camera model (and interpolator)
void launch_linearize_photometric(pba_engine* e, const KernelArgs& ka, const LinArgs& la);
void launch_linearize_geometric(pba_engine* e, const KernelArgs& ka, const LinArgs& la);

}  // namespace detail
}  // namespace pba
