// Stand-alone checker of the joint solve's host plan (csrc/pba_joint_plan.cpp): builds plans for a chain, loop closures,
// an idle keyframe, points without blocks, a point that observes one keyframe twice and random problems, and checks every
// list against a brute-force restatement.  Compiled with -fsanitize=address,undefined by tests/test_joint_plan.py and
// run as a program.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include <string>

#include "pba_joint_plan.h"

namespace pba {
namespace detail {
thread_local std::string g_last_error;  // (pba_gn_plan.cpp's, for skyline_profile: defined in pba_engine.hip in the full library)
}  // namespace detail
}  // namespace pba

using pba::detail::build_joint_plan;
using pba::detail::JointPlan;
using pba::detail::JointPlanInput;
using pba::detail::JointTerm;

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      std::exit(1);                                                  \
    }                                                                \
  } while (0)

struct Problem {
  int nf = 0;
  std::vector<int> point_host, block_point, block_target;
  // the engine's pairs: distinct (host, target), sorted
  std::vector<int> pair_host, pair_target, block_pair;
  void pairs() {
    std::map<std::pair<int, int>, int> ids;
    for (size_t b = 0; b < block_point.size(); ++b) ids[{point_host[block_point[b]], block_target[b]}] = 0;
    pair_host.clear();
    pair_target.clear();
    for (auto& kv : ids) {
      kv.second = (int)pair_host.size();
      pair_host.push_back(kv.first.first);
      pair_target.push_back(kv.first.second);
    }
    block_pair.resize(block_point.size());
    for (size_t b = 0; b < block_point.size(); ++b) block_pair[b] = ids[{point_host[block_point[b]], block_target[b]}];
  }
  JointPlanInput input() const {
    JointPlanInput in;
    in.n_frames = nf;
    in.n_pairs = (int)pair_host.size();
    in.n_points = (int)point_host.size();
    in.n_blocks = (int)block_point.size();
    in.pair_host = pair_host.data();
    in.pair_target = pair_target.data();
    in.block_pair = block_pair.data();
    in.block_point = block_point.data();
    in.point_host = point_host.data();
    return in;
  }
};

template <class T>
static std::vector<T> slice(const std::vector<T>& v, int a, int b) {
  return std::vector<T>(v.begin() + a, v.begin() + b);
}

static long long check(Problem& pb) {
  pb.pairs();
  const JointPlanInput in = pb.input();
  JointPlan P;
  CHECK(build_joint_plan(in, P));
  const int nf = pb.nf, np = in.n_pairs, npt = in.n_points, nb = in.n_blocks;
  // blocks of each pair and of each point: exactly its blocks, ascending
  CHECK((int)P.pair_ptr.size() == np + 1 && P.pair_ptr[np] == nb && (int)P.pair_blocks.size() == nb);
  for (int p = 0; p < np; ++p) {
    std::vector<int> want;
    for (int b = 0; b < nb; ++b)
      if (pb.block_pair[b] == p) want.push_back(b);
    CHECK(slice(P.pair_blocks, P.pair_ptr[p], P.pair_ptr[p + 1]) == want);
  }
  CHECK((int)P.pt_ptr.size() == npt + 1 && P.pt_ptr[npt] == nb && (int)P.pt_blocks.size() == nb);
  for (int q = 0; q < npt; ++q) {
    std::vector<int> want;
    for (int b = 0; b < nb; ++b)
      if (pb.block_point[b] == q) want.push_back(b);
    CHECK(slice(P.pt_blocks, P.pt_ptr[q], P.pt_ptr[q + 1]) == want);
  }
  // pairs of each keyframe: as host ascending, then as target ascending
  CHECK((int)P.frame_ptr.size() == nf + 1 && P.frame_ptr[nf] == 2 * np);
  for (int f = 0; f < nf; ++f) {
    std::vector<int> want;
    for (int p = 0; p < np; ++p)
      if (pb.pair_host[p] == f) want.push_back(2 * p);
    for (int p = 0; p < np; ++p)
      if (pb.pair_target[p] == f) want.push_back(2 * p + 1);
    CHECK(slice(P.frame_pairs, P.frame_ptr[f], P.frame_ptr[f + 1]) == want);
  }
  // the keyframes of each point with blocks, and which keyframes share a point
  std::vector<std::vector<char>> share(nf, std::vector<char>(nf, 0));
  for (int q = 0; q < npt; ++q) {
    std::vector<int> fr;
    for (int b = 0; b < nb; ++b)
      if (pb.block_point[b] == q) fr.push_back(pb.block_target[b]);
    if (fr.empty()) continue;
    fr.push_back(pb.point_host[q]);
    for (int x : fr)
      for (int y : fr) share[x][y] = 1;
  }
  // profile: the envelope of the shared points, the last row of each column, the columns' row lists
  int n_sky = 0;
  CHECK((int)P.first.size() == nf && (int)P.row.size() == nf + 1 && (int)P.last.size() == nf);
  for (int i = 0; i < nf; ++i) {
    int first = i;
    for (int j = 0; j < i; ++j)
      if (share[i][j]) first = std::min(first, j);
    CHECK(P.first[i] == first && P.row[i] == n_sky);
    n_sky += i - first + 1;
  }
  CHECK(P.row[nf] == n_sky && P.n_sky == n_sky && (int)P.colptr.size() == nf + 1);
  for (int k = 0; k < nf; ++k) {
    std::vector<int> want;
    for (int i = k + 1; i < nf; ++i)
      if (P.first[i] <= k) want.push_back(i);
    CHECK(slice(P.colrows, P.colptr[k], P.colptr[k + 1]) == want);
    CHECK(P.last[k] == (want.empty() ? k : want.back()));
  }
  // entries: the host part ~q, then the point's blocks
  auto frame_of = [&](int e) { return e < 0 ? pb.point_host[~e] : pb.block_target[e]; };
  auto entries = [&](int q) {
    std::vector<int> ent;
    for (int b = 0; b < nb; ++b)
      if (pb.block_point[b] == q) ent.push_back(b);
    if (!ent.empty()) ent.insert(ent.begin(), ~q);
    return ent;
  };
  // direct and Schur lists of every skyline block
  CHECK((int)P.off_ptr.size() == n_sky + 1 && (int)P.term_ptr.size() == n_sky + 1);
  long long n_terms = 0, n_off = 0;
  for (int i = 0; i < nf; ++i)
    for (int j = P.first[i]; j <= i; ++j) {
      const int s = P.row[i] + (j - P.first[i]);
      std::vector<int> want;
      for (int p = 0; p < np; ++p)
        if (i != j && ((pb.pair_host[p] == i && pb.pair_target[p] == j) || (pb.pair_host[p] == j && pb.pair_target[p] == i)))
          want.push_back(2 * p + (pb.pair_host[p] == j ? 1 : 0));
      CHECK(slice(P.off_pairs, P.off_ptr[s], P.off_ptr[s + 1]) == want);
      n_off += (long long)want.size();
      std::vector<std::pair<int, int>> terms;
      for (int q = 0; q < npt; ++q) {
        const std::vector<int> ent = entries(q);
        for (int a : ent)
          for (int b : ent)
            if (frame_of(a) == i && frame_of(b) == j) terms.emplace_back(a, b);
      }
      CHECK(P.term_ptr[s + 1] - P.term_ptr[s] == (int)terms.size());
      for (size_t k = 0; k < terms.size(); ++k) {
        const JointTerm& t = P.terms[P.term_ptr[s] + k];
        CHECK(t.a == terms[k].first && t.b == terms[k].second);
      }
      n_terms += (long long)terms.size();
    }
  CHECK(n_off == np && (int)P.off_pairs.size() == np);  // (every pair here has a block)
  // no term falls outside the profile: the lists hold every ordered pair of entries with keyframe(a) ≥ keyframe(b)
  long long all = 0, n_ent = 0;
  for (int q = 0; q < npt; ++q) {
    const std::vector<int> ent = entries(q);
    n_ent += (long long)ent.size();
    for (int a : ent)
      for (int b : ent) all += frame_of(a) >= frame_of(b);
  }
  CHECK(n_terms == all && (long long)P.terms.size() == all);
  // entries of each keyframe, points ascending
  CHECK((int)P.fe_ptr.size() == nf + 1 && P.fe_ptr[nf] == n_ent && (long long)P.fe_entries.size() == n_ent);
  for (int f = 0; f < nf; ++f) {
    std::vector<int> want;
    for (int q = 0; q < npt; ++q)
      for (int e : entries(q))
        if (frame_of(e) == f) want.push_back(e);
    CHECK(slice(P.fe_entries, P.fe_ptr[f], P.fe_ptr[f + 1]) == want);
  }
  return n_terms;
}

int main() {
  long long terms = 0;
  // a chain of K = 4 targets per host, as the synthetic problems
  {
    Problem pb;
    pb.nf = 10;
    for (int q = 0; q < 40; ++q) {
      const int h = q % 6;
      pb.point_host.push_back(h);
      for (int k = 1; k <= 4; ++k)
        if ((q + k) % 5) { pb.block_point.push_back(q); pb.block_target.push_back(h + k); }
    }
    terms += check(pb);
  }
  // loop closures (a point hosted in 9 seen from 0), backward targets, a point seen twice from one keyframe, points
  // without blocks, an idle keyframe (5)
  {
    Problem pb;
    pb.nf = 11;
    pb.point_host = {0, 1, 9, 3, 4, 2, 10};
    pb.block_point = {0, 0, 1, 2, 2, 3, 3, 3, 6, 1};
    pb.block_target = {1, 2, 0, 0, 8, 2, 2, 4, 7, 3};
    terms += check(pb);
  }
  // one block
  {
    Problem pb;
    pb.nf = 2;
    pb.point_host = {1};
    pb.block_point = {0};
    pb.block_target = {0};
    terms += check(pb);
  }
  // random problems
  std::mt19937 rng(7);
  for (int it = 0; it < 60; ++it) {
    Problem pb;
    pb.nf = 2 + (int)(rng() % 12);
    const int npt = 1 + (int)(rng() % 25), nb = 1 + (int)(rng() % 90);
    for (int q = 0; q < npt; ++q) pb.point_host.push_back((int)(rng() % pb.nf));
    for (int b = 0; b < nb; ++b) {
      const int q = (int)(rng() % npt);
      int t = (int)(rng() % pb.nf);
      if (t == pb.point_host[q]) t = (t + 1) % pb.nf;
      pb.block_point.push_back(q);
      pb.block_target.push_back(t);
    }
    terms += check(pb);
  }
  // refused: an index out of range, a block whose pair does not have its point's host, a pair of a keyframe with itself
  {
    const int ph[2] = {0, 1}, pt[2] = {1, 2}, bpair[2] = {0, 1}, bpoint[2] = {0, 1}, host[2] = {0, 1};
    JointPlanInput in;
    in.n_frames = 3; in.n_pairs = 2; in.n_points = 2; in.n_blocks = 2;
    in.pair_host = ph; in.pair_target = pt; in.block_pair = bpair; in.block_point = bpoint; in.point_host = host;
    JointPlan P;
    CHECK(build_joint_plan(in, P));
    const int pt_bad[2] = {1, 3};
    in.pair_target = pt_bad;
    CHECK(!build_joint_plan(in, P));
    in.pair_target = pt;
    const int bpoint_bad[2] = {0, 2};
    in.block_point = bpoint_bad;
    CHECK(!build_joint_plan(in, P));
    const int bpoint_other[2] = {1, 1};  // block 0's pair is hosted by 0, its point by 1
    in.block_point = bpoint_other;
    CHECK(!build_joint_plan(in, P));
    in.block_point = bpoint;
    const int pt_self[2] = {0, 2};
    in.pair_target = pt_self;
    CHECK(!build_joint_plan(in, P));
  }
  std::printf("joint plan: ok (%lld Schur terms checked)\n", terms);
  return 0;
}
