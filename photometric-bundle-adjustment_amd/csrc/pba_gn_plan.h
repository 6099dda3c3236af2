// pba_gn_plan.h — the symbolic analysis of a Gauss-Newton problem (pba_gn_plan.cpp) as a pure host function: from the
// blocks' topology to every index structure the GN kernels read without checking — the GN block order, the linearise
// and Schur chunks with their slot offsets, the uint8 local indices, the pair slots, the skyline profile with its
// contribution lists, the free-intrinsics border lists and the point-aligned wave table.  No HIP: gn_prepare
// (pba_gn.hip) fills the input from the engine and uploads the vectors as they are; tests/cpp/gn_plan_check.cpp checks
// their invariants on the host (g++, AddressSanitizer + UndefinedBehaviorSanitizer).  The layout constants both sides
// need are here too.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace pba {
namespace detail {

#ifndef PBA_SCHUR_PTS
#define PBA_SCHUR_PTS 128
#endif
constexpr int SCHUR_PTS = PBA_SCHUR_PTS;  // points per Schur chunk (-DPBA_SCHUR_PTS: A/B builds)
constexpr int SCHUR_W = 2048;             // points × local poses per Schur chunk (LDS budget: dynamic, 48 B each)

constexpr int SLOT_LIN_BASE = 42;  // H_hh(36) + g_h(6)
constexpr int SLOT_LIN_T = 78;     // H_ht(36) + H_tt(36) + g_t(6)

// At most this many targets per linearise chunk (build_gn_plan cuts chunks there): a wave's blocks then hold ≤ 4 target
// runs, so its per-run product sets (fp64) fit the LDS the fp32 ones took for 8.
constexpr int kChunkTargets = 4;

// flags of a contribution {offset, flags}: the block is stored transposed / lies in the Schur partials (else linearise)
enum : int { C_TRANSPOSE = 1, C_SCHUR = 2 };

// The records that are int4, int2 and uchar2 on the device (pba_gn.hip asserts the sizes and uploads them as such).
struct PlanInt4 {
  int x, y, z, w;
};
struct PlanInt2 {
  int x, y;
};
struct PlanUchar2 {
  unsigned char x, y;
};

struct GnPlanInput {
  int n_frames, n_cams, n_pairs, n_points, n_blocks;
  const int* block_point_h;   // n_blocks
  const int* block_target_h;  // n_blocks
  const int* point_host_h;    // n_points
  const int* pair_of_h;       // n_blocks
  const int* pair_host_h;     // n_pairs
  const int* pair_target_h;   // n_pairs
  const int* frame_cam_h;     // n_frames
  const uint8_t* fixed_h;     // the requested constant frames, n_fixed ≤ n_frames of them (the rest: free)
  int n_fixed;
  int lpb, ppl, bpw;          // lanes per block, rows per lane, blocks per linearise workgroup
  int nc;                     // cameras with free intrinsics (0: none)
  bool test_pblk_walk;        // PBA_TEST_PBLK_WALK: every target entry of ib_pblk walks its point's blocks (−2)
  bool test_row_waves64;      // PBA_TEST_ROW_WAVES64: no point-aligned wave table
  bool skyline_global;        // PBA_SKYLINE_GLOBAL: no front plan (passed on to build_front_plan by gn_prepare)
};

// The vectors are named after the GnData buffers they fill and hold exactly what is uploaded (the placeholder element
// of a list that would be empty included).
struct GnPlan {
  std::vector<PlanInt4> lin_rec, chunk_desc;
  std::vector<int> pt_first, pt_nblk, pt_orig, pt_host, gn_target;
  std::vector<PlanInt4> pt_rec, pt_tgt;
  std::vector<PlanInt2> pt_fb;
  std::vector<PlanInt4> schur_desc, schur_aux, schur_lvp4;
  std::vector<PlanUchar2> schur_pairs;
  std::vector<uint8_t> blk_lv;
  std::vector<int> schur_lvp;
  // skyline profile: first column of each row, row offsets, last row of each column, the columns' row lists (what
  // build_front_plan takes: first, rowp, ccptr, ccrows)
  std::vector<int> sky_first, sky_row, sky_last, sky_colptr, sky_colrows;
  std::vector<int> sky_cptr, g_cptr, sky_blk_i, sky_blk_j, sky_diag, sky_off;
  std::vector<PlanInt2> sky_contrib, g_contrib;
  std::vector<uint8_t> fixed, observed, fixed_req;
  std::vector<PlanInt4> pair_rec;
  // free intrinsics (nc > 0; else empty)
  std::vector<PlanInt4> ib_rec, ir_wave;
  std::vector<int> ib_cam, ib_bptr, ib_blist, ib_pptr, ib_plist, ib_pblk;

  int n_chunks = 0, n_gn_points = 0, n_schur = 0, schur_rt_off = 0;
  size_t lin_slots = 0, schur_doubles = 0, schur_lds = 0;
  int n_sky = 0, n_sky_diag = 0, band = 0, nfs = 0, ir_waves = 0;
};

// PBA_OK, or PBA_ERR_INVALID_ARGUMENT with pba_last_error() set ("a point observes too many keyframes", "more than 2^24
// (host, target) pairs").
int build_gn_plan(const GnPlanInput& in, GnPlan& plan);

// The rows of each column's profile: column k → every i > k with first(i) ≤ k, in order (CSR).
void profile_columns(const std::vector<int>& first, std::vector<int>& ccptr, std::vector<int>& ccrows);
// A skyline profile from its rows' first columns: row offsets (rowp[n] blocks in all), the last row of each column, and
// profile_columns.
void skyline_profile(const std::vector<int>& first, std::vector<int>& rowp, std::vector<int>& last,
                     std::vector<int>& ccptr, std::vector<int>& ccrows);

}  // namespace detail
}  // namespace pba
