// pba_affine_plan.cpp — see pba_affine_plan.h.
#include "pba_affine_plan.h"

#include <algorithm>

#include "pba_plan_lists.h"

namespace pba {
namespace detail {

bool build_affine_plan(const AffinePlanInput& in, AffinePlan& P) {
  const int nf = in.n_frames, np = in.n_pairs, nb = in.n_blocks;
  if (nf <= 0 || np < 0 || nb < 0) return false;
  for (int p = 0; p < np; ++p)
    if (in.pair_host[p] < 0 || in.pair_host[p] >= nf || in.pair_target[p] < 0 || in.pair_target[p] >= nf) return false;
  for (int b = 0; b < nb; ++b)
    if (in.block_pair[b] < 0 || in.block_pair[b] >= np) return false;
  csr_group(np, nb, in.block_pair, P.pair_ptr, P.pair_blocks);
  frame_pair_lists(nf, np, in.pair_host, in.pair_target, P.frame_ptr, P.frame_pairs);
  // skyline profile
  P.first.resize(nf);
  for (int f = 0; f < nf; ++f) P.first[f] = f;
  for (int p = 0; p < np; ++p) {
    const int lo = std::min(in.pair_host[p], in.pair_target[p]), hi = std::max(in.pair_host[p], in.pair_target[p]);
    P.first[hi] = std::min(P.first[hi], lo);
  }
  P.row.assign(nf + 1, 0);
  P.max_row = 0;
  for (int f = 0; f < nf; ++f) {
    P.row[f + 1] = P.row[f] + (f - P.first[f] + 1);
    P.max_row = std::max(P.max_row, 2 * (f - P.first[f] + 1));
  }
  P.n_sky = P.row[nf];
  // a pair of a keyframe with itself has no off-diagonal part; a pair without blocks keeps its (empty) place
  off_diagonal_pair_lists(np, in.pair_host, in.pair_target, P.first, P.row,
                          [&](int p) { return in.pair_host[p] != in.pair_target[p]; }, P.off_ptr, P.off_pairs);
  return true;
}

}  // namespace detail
}  // namespace pba
