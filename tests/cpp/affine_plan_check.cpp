// Stand-alone checker of the brightness solve's host plan (csrc/pba_affine_plan.cpp): builds plans for a chain, a loop
// closure, reversed and repeated pairs, a self pair and pairs without blocks, and checks every list against a
// brute-force restatement.  Compiled with -fsanitize=address,undefined by tests/test_affine_plan.py and run as a program.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pba_affine_plan.h"

using pba::detail::AffinePlan;
using pba::detail::AffinePlanInput;
using pba::detail::build_affine_plan;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

static void check(int nf, const std::vector<int>& ph, const std::vector<int>& pt, const std::vector<int>& bp) {
  AffinePlanInput in;
  in.n_frames = nf;
  in.n_pairs = (int)ph.size();
  in.n_blocks = (int)bp.size();
  in.pair_host = ph.data();
  in.pair_target = pt.data();
  in.block_pair = bp.data();
  AffinePlan P;
  CHECK(build_affine_plan(in, P));
  const int np = in.n_pairs, nb = in.n_blocks;
  // blocks of each pair: exactly its blocks, ascending
  CHECK((int)P.pair_ptr.size() == np + 1 && P.pair_ptr[0] == 0 && P.pair_ptr[np] == nb && (int)P.pair_blocks.size() == nb);
  for (int p = 0; p < np; ++p) {
    std::vector<int> want;
    for (int b = 0; b < nb; ++b)
      if (bp[b] == p) want.push_back(b);
    CHECK(std::vector<int>(P.pair_blocks.begin() + P.pair_ptr[p], P.pair_blocks.begin() + P.pair_ptr[p + 1]) == want);
  }
  // pairs of each keyframe: as host ascending, then as target ascending
  CHECK((int)P.frame_ptr.size() == nf + 1 && P.frame_ptr[nf] == 2 * np);
  for (int f = 0; f < nf; ++f) {
    std::vector<int> want;
    for (int p = 0; p < np; ++p)
      if (ph[p] == f) want.push_back(2 * p);
    for (int p = 0; p < np; ++p)
      if (pt[p] == f) want.push_back(2 * p + 1);
    CHECK(std::vector<int>(P.frame_pairs.begin() + P.frame_ptr[f], P.frame_pairs.begin() + P.frame_ptr[f + 1]) == want);
  }
  // profile: the envelope of the pairs
  int n_sky = 0, max_row = 0;
  for (int f = 0; f < nf; ++f) {
    int first = f;
    for (int p = 0; p < np; ++p)
      if (std::max(ph[p], pt[p]) == f) first = std::min(first, std::min(ph[p], pt[p]));
    CHECK(P.first[f] == first && P.row[f] == n_sky);
    n_sky += f - first + 1;
    max_row = std::max(max_row, 2 * (f - first + 1));
  }
  CHECK(P.row[nf] == n_sky && P.n_sky == n_sky && P.max_row == max_row);
  // off-diagonal lists: every pair with host ≠ target once, in its block, ascending, with the transpose flag
  CHECK((int)P.off_ptr.size() == n_sky + 1);
  int seen = 0;
  for (int i = 0; i < nf; ++i)
    for (int j = P.first[i]; j <= i; ++j) {
      const int s = P.row[i] + (j - P.first[i]);
      std::vector<int> want;
      for (int p = 0; p < np; ++p)
        if (i != j && ((ph[p] == i && pt[p] == j) || (ph[p] == j && pt[p] == i))) want.push_back(2 * p + (ph[p] == j ? 1 : 0));
      CHECK(std::vector<int>(P.off_pairs.begin() + P.off_ptr[s], P.off_pairs.begin() + P.off_ptr[s + 1]) == want);
      seen += (int)want.size();
    }
  int off = 0;
  for (int p = 0; p < np; ++p) off += ph[p] != pt[p];
  CHECK(seen == off && (int)P.off_pairs.size() == off);
}

int main() {
  // a chain of K = 4 targets per host, as the synthetic problems
  {
    std::vector<int> ph, pt, bp;
    for (int h = 0; h < 6; ++h)
      for (int k = 1; k <= 4; ++k) { ph.push_back(h); pt.push_back(h + k); }
    for (int b = 0; b < 97; ++b) bp.push_back((b * 7) % (int)ph.size());
    check(10, ph, pt, bp);
  }
  // a loop closure (9 → 0), a reversed pair, a repeated pair, a self pair, a pair without blocks, an idle keyframe
  check(11, {0, 1, 9, 1, 0, 3, 5}, {1, 2, 0, 0, 1, 3, 4}, {0, 0, 2, 3, 4, 4, 1, 5, 2});
  // no pairs, no blocks
  check(3, {}, {}, {});
  // random problems
  std::mt19937 rng(5);
  for (int it = 0; it < 50; ++it) {
    const int nf = 1 + (int)(rng() % 12), np = (int)(rng() % 30), nb = np ? (int)(rng() % 200) : 0;
    std::vector<int> ph(np), pt(np), bp(nb);
    for (int p = 0; p < np; ++p) { ph[p] = (int)(rng() % nf); pt[p] = (int)(rng() % nf); }
    for (int b = 0; b < nb; ++b) bp[b] = (int)(rng() % np);
    check(nf, ph, pt, bp);
  }
  // out-of-range indices are refused
  {
    const int h[1] = {0}, t[1] = {3}, b[1] = {0};
    AffinePlanInput in;
    in.n_frames = 3; in.n_pairs = 1; in.n_blocks = 1; in.pair_host = h; in.pair_target = t; in.block_pair = b;
    AffinePlan P;
    CHECK(!build_affine_plan(in, P));
    const int t2[1] = {2}, b2[1] = {1};
    in.pair_target = t2; in.block_pair = b2;
    CHECK(!build_affine_plan(in, P));
  }
  std::puts("affine plan: ok");
  return 0;
}
