// pba_plan_lists.h — the lists the brightness plan (pba_affine_plan.cpp) and the joint plan (pba_joint_plan.cpp) share:
// CSR lists in a fixed order, built by counting sorts.  Host only, plain vectors; static, so that the library exports
// nothing new.
#pragma once

#include <algorithm>
#include <vector>

namespace pba {
namespace detail {

// CSR pointers from the counts in ptr[1…]
static inline void csr_prefix(std::vector<int>& ptr) {
  for (size_t i = 0; i + 1 < ptr.size(); ++i) ptr[i + 1] += ptr[i];
}

// The items 0 … n − 1 grouped by key[i] in [0, n_keys), ascending within a key: the blocks of each pair, of each point.
static inline void csr_group(int n_keys, int n, const int* key, std::vector<int>& ptr, std::vector<int>& items) {
  ptr.assign(n_keys + 1, 0);
  for (int i = 0; i < n; ++i) ++ptr[key[i] + 1];
  csr_prefix(ptr);
  items.resize(n);
  std::vector<int> at(ptr.begin(), ptr.end() - 1);
  for (int i = 0; i < n; ++i) items[at[key[i]]++] = i;
}

// The pairs of each keyframe as pair · 2 + role (0: host, 1: target): the hosts' pairs first, each ascending.
static inline void frame_pair_lists(int n_frames, int n_pairs, const int* pair_host, const int* pair_target,
                                    std::vector<int>& ptr, std::vector<int>& pairs) {
  ptr.assign(n_frames + 1, 0);
  for (int p = 0; p < n_pairs; ++p) {
    ++ptr[pair_host[p] + 1];
    ++ptr[pair_target[p] + 1];
  }
  csr_prefix(ptr);
  pairs.resize(2 * (size_t)n_pairs);
  std::vector<int> at(ptr.begin(), ptr.end() - 1);
  for (int p = 0; p < n_pairs; ++p) pairs[at[pair_host[p]]++] = 2 * p;
  for (int p = 0; p < n_pairs; ++p) pairs[at[pair_target[p]]++] = 2 * p + 1;
}

// The pairs of each off-diagonal block of the lower skyline (first, row; row has n_frames + 1 entries), ascending, as
// pair · 2 + t, t = 1 when the pair's host is the block's column; the pairs p with takes_part(p), none of them a pair of
// a keyframe with itself.
template <class Pred>
static void off_diagonal_pair_lists(int n_pairs, const int* pair_host, const int* pair_target,
                                    const std::vector<int>& first, const std::vector<int>& row, Pred takes_part,
                                    std::vector<int>& ptr, std::vector<int>& pairs) {
  auto sky = [&](int p) {
    const int hi = std::max(pair_host[p], pair_target[p]), lo = std::min(pair_host[p], pair_target[p]);
    return row[hi] + (lo - first[hi]);
  };
  ptr.assign(row.back() + 1, 0);
  for (int p = 0; p < n_pairs; ++p)
    if (takes_part(p)) ++ptr[sky(p) + 1];
  csr_prefix(ptr);
  pairs.resize(ptr.back());
  std::vector<int> at(ptr.begin(), ptr.end() - 1);
  for (int p = 0; p < n_pairs; ++p)
    if (takes_part(p)) pairs[at[sky(p)]++] = 2 * p + (pair_host[p] < pair_target[p] ? 1 : 0);
}

}  // namespace detail
}  // namespace pba
