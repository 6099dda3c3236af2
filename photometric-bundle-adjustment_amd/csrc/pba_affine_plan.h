// pba_affine_plan.h — the host-only plan of the brightness solve (pba_affine.hip): which blocks, pairs and skyline
// blocks each sum of the (a, b) normal equations runs over, in a fixed order.  No device code, no engine: plain
// vectors in, plain vectors out (tests/cpp/affine_plan_check.cpp checks it stand-alone, under the sanitizers).
#pragma once

#include <vector>

namespace pba {
namespace detail {

struct AffinePlanInput {
  int n_frames = 0, n_pairs = 0, n_blocks = 0;
  const int* pair_host = nullptr;    // per pair
  const int* pair_target = nullptr;  // per pair
  const int* block_pair = nullptr;   // per block
};

// The system is 2·n_frames square, 2×2 blocks, lower skyline by block rows: row i holds the blocks (i, j),
// first[i] ≤ j ≤ i, at block offsets row[i] + (j − first[i]); first[i] is the smallest keyframe that shares a pair
// with i (the envelope of the pairs: Cholesky fills nothing outside it, loop closures included).
struct AffinePlan {
  std::vector<int> pair_ptr, pair_blocks;    // CSR: the blocks of each pair, ascending
  std::vector<int> frame_ptr, frame_pairs;   // CSR: per keyframe, pair · 2 + role (0: host, 1: target), hosts' pairs
                                             // first, each ascending
  std::vector<int> first, row;               // skyline profile (row has n_frames + 1 entries)
  std::vector<int> off_ptr, off_pairs;       // CSR per skyline block (the diagonal ones stay empty): pair · 2 + t,
                                             // t = 1 when the pair's host is the block's column (H_htᵀ goes in)
  int n_sky = 0;                             // skyline blocks
  int max_row = 0;                           // widest scalar row, 2 · max(i − first[i] + 1)
};

// false when an index is out of range (the plan is then unspecified)
bool build_affine_plan(const AffinePlanInput& in, AffinePlan& P);

}  // namespace detail
}  // namespace pba
