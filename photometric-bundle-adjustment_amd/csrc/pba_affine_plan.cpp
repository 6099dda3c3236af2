// pba_affine_plan.cpp — see pba_affine_plan.h.
#include "pba_affine_plan.h"

#include <algorithm>

namespace pba {
namespace detail {

bool build_affine_plan(const AffinePlanInput& in, AffinePlan& P) {
  const int nf = in.n_frames, np = in.n_pairs, nb = in.n_blocks;
  if (nf <= 0 || np < 0 || nb < 0) return false;
  for (int p = 0; p < np; ++p)
    if (in.pair_host[p] < 0 || in.pair_host[p] >= nf || in.pair_target[p] < 0 || in.pair_target[p] >= nf) return false;
  for (int b = 0; b < nb; ++b)
    if (in.block_pair[b] < 0 || in.block_pair[b] >= np) return false;
  // blocks of each pair (counting sort: ascending within a pair)
  P.pair_ptr.assign(np + 1, 0);
  for (int b = 0; b < nb; ++b) ++P.pair_ptr[in.block_pair[b] + 1];
  for (int p = 0; p < np; ++p) P.pair_ptr[p + 1] += P.pair_ptr[p];
  P.pair_blocks.resize(nb);
  {
    std::vector<int> at(P.pair_ptr.begin(), P.pair_ptr.end() - 1);
    for (int b = 0; b < nb; ++b) P.pair_blocks[at[in.block_pair[b]]++] = b;
  }
  // pairs of each keyframe: as host, then as target
  P.frame_ptr.assign(nf + 1, 0);
  for (int p = 0; p < np; ++p) {
    ++P.frame_ptr[in.pair_host[p] + 1];
    ++P.frame_ptr[in.pair_target[p] + 1];
  }
  for (int f = 0; f < nf; ++f) P.frame_ptr[f + 1] += P.frame_ptr[f];
  P.frame_pairs.resize(2 * (size_t)np);
  {
    std::vector<int> at(P.frame_ptr.begin(), P.frame_ptr.end() - 1);
    for (int p = 0; p < np; ++p) P.frame_pairs[at[in.pair_host[p]]++] = 2 * p;
    for (int p = 0; p < np; ++p) P.frame_pairs[at[in.pair_target[p]]++] = 2 * p + 1;
  }
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
  // pairs of each off-diagonal skyline block (a pair of a keyframe with itself has no off-diagonal part)
  P.off_ptr.assign(P.n_sky + 1, 0);
  auto sky = [&](int p) {
    const int h = in.pair_host[p], t = in.pair_target[p], hi = std::max(h, t), lo = std::min(h, t);
    return P.row[hi] + (lo - P.first[hi]);
  };
  for (int p = 0; p < np; ++p)
    if (in.pair_host[p] != in.pair_target[p]) ++P.off_ptr[sky(p) + 1];
  for (int s = 0; s < P.n_sky; ++s) P.off_ptr[s + 1] += P.off_ptr[s];
  P.off_pairs.resize(P.off_ptr[P.n_sky]);
  {
    std::vector<int> at(P.off_ptr.begin(), P.off_ptr.end() - 1);
    for (int p = 0; p < np; ++p)
      if (in.pair_host[p] != in.pair_target[p])
        P.off_pairs[at[sky(p)]++] = 2 * p + (in.pair_host[p] < in.pair_target[p] ? 1 : 0);
  }
  return true;
}

}  // namespace detail
}  // namespace pba
