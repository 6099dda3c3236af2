// Stand-alone checker of the multi-GPU joint exchange's host plan (csrc/pba_joint_plan.cpp build_joint_exchange): the
// band profile, the offsets and, per exchange block, the local skyline block whose lists fill it, against a brute-force
// restatement — for the six-keyframe structure of the tests (points hosted by keyframes 0 and 1), a loop-closed graph,
// a shard of it (points of some hosts only), a keyframe without pairs, K = the local band and K = n_frames − 1 and the
// values between, and the refused bands.  Compiled with -fsanitize=address,undefined by
// tests/test_joint_exchange_plan.py and run as a program.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pba_joint_plan.h"

namespace pba {
namespace detail {
thread_local std::string g_last_error;  // (pba_gn_plan.cpp's: defined in pba_engine.hip in the full library)
}  // namespace detail
}  // namespace pba

using namespace pba::detail;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

struct Problem {
  int nf = 0;
  std::vector<int> point_host, block_point, block_target, pair_host, pair_target, block_pair;
  void add_point(int host, const std::vector<int>& targets) {
    const int q = (int)point_host.size();
    point_host.push_back(host);
    for (int t : targets)
      if (t >= 0 && t < nf && t != host) {
        block_point.push_back(q);
        block_target.push_back(t);
      }
  }
  JointPlan plan() {
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
    JointPlan P;
    CHECK(build_joint_plan(in, P));
    return P;
  }
};

// every band the plan allows, and the two next to them that it must refuse
static long long check(Problem& pb) {
  const JointPlan P = pb.plan();
  const int nf = pb.nf;
  int band = 0;
  for (int i = 0; i < nf; ++i) band = std::max(band, i - P.first[i]);
  CHECK(joint_local_band(P.first) == band);
  JointExchangePlan X;
  CHECK(!build_joint_exchange(P.first, P.row, band - 1, X));
  CHECK(!build_joint_exchange(P.first, P.row, nf, X));
  long long blocks = 0;
  for (int K = band; K <= nf - 1; ++K) {
    JointExchangePlan Y;
    CHECK(build_joint_exchange(P.first, P.row, K, Y));
    CHECK(Y.K == K && Y.stride == 64LL * (K + 1) + kJointExTail && Y.scalar_off == Y.stride * nf);
    CHECK(Y.count == Y.scalar_off + kJointExScalars && (int)Y.src.size() == nf * (K + 1));
    // sources: exchange block (i, c) is column j = i − K + c; filled exactly where (i, j) lies in the local profile,
    // by that skyline block, and every local skyline block fills exactly one exchange block
    std::vector<int> used(P.n_sky, 0);
    for (int i = 0; i < nf; ++i)
      for (int c = 0; c <= K; ++c) {
        const int j = i - K + c, s = Y.src[(size_t)i * (K + 1) + c];
        const bool in_profile = j >= 0 && j >= P.first[i];
        CHECK((s >= 0) == in_profile);
        if (s >= 0) {
          CHECK(s == P.row[i] + (j - P.first[i]) && s < P.n_sky);
          ++used[s];
        }
      }
    for (int s = 0; s < P.n_sky; ++s) CHECK(used[s] == 1);
    // the band profile and its column lists
    int n_sky = 0;
    CHECK((int)Y.first.size() == nf && (int)Y.row.size() == nf + 1 && (int)Y.colptr.size() == nf + 1);
    for (int i = 0; i < nf; ++i) {
      CHECK(Y.first[i] == std::max(0, i - K) && Y.first[i] <= P.first[i] && Y.row[i] == n_sky);
      for (int j = Y.first[i]; j <= i; ++j) {
        CHECK(Y.sky_i[n_sky] == i && Y.sky_j[n_sky] == j);
        // … and where the import reads block (i, j): inside keyframe i's (K + 1) blocks
        CHECK(j - (i - K) >= 0 && j - (i - K) <= K);
        ++n_sky;
      }
    }
    CHECK(Y.row[nf] == n_sky && Y.n_sky == n_sky && (int)Y.sky_i.size() == n_sky && (int)Y.sky_j.size() == n_sky);
    for (int k = 0; k < nf; ++k) {
      std::vector<int> want;
      for (int i = k + 1; i < nf; ++i)
        if (std::max(0, i - K) <= k) want.push_back(i);
      CHECK(std::vector<int>(Y.colrows.begin() + Y.colptr[k], Y.colrows.begin() + Y.colptr[k + 1]) == want);
      CHECK(Y.last[k] == (want.empty() ? k : want.back()));
    }
    blocks += n_sky;
  }
  return blocks;
}

int main() {
  long long blocks = 0;
  {  // the six-keyframe structure: points hosted by keyframes 0 and 1, targets host + 1 … host + 4
    Problem pb;
    pb.nf = 6;
    for (int q = 0; q < 20; ++q) pb.add_point(q % 2, {q % 2 + 1, q % 2 + 2, q % 2 + 3, q % 2 + 4});
    blocks += check(pb);
    Problem r0;  // … and its first shard alone (host 0): keyframe 5 has no pair there
    r0.nf = 6;
    for (int q = 0; q < 10; ++q) r0.add_point(0, {1, 2, 3, 4});
    blocks += check(r0);
  }
  {  // a loop-closed two-way graph, whole and as the shard of the hosts 8 … 15
    for (int lo : {0, 8}) {
      Problem pb;
      pb.nf = 16;
      for (int q = 0; q < 64; ++q) {
        const int h = q % 16;
        if (h < lo) continue;
        const int s = q % 3 == 0 ? 1 : -1;
        pb.add_point(h, {h + s, h + 2 * s, h + 3 * s});
        if (h == 15) pb.add_point(h, {0, 14});  // the closure
      }
      blocks += check(pb);
    }
  }
  {  // a keyframe without pairs (4), and a single pair
    Problem pb;
    pb.nf = 9;
    for (int q = 0; q < 18; ++q)
      if (q % 9 != 4) pb.add_point(q % 9, {q % 9 == 3 ? 5 : q % 9 + 1, q % 9 == 5 ? 3 : q % 9 - 1});
    const JointPlan P = pb.plan();
    CHECK(P.frame_ptr[4] == P.frame_ptr[5]);
    blocks += check(pb);
    Problem one;
    one.nf = 2;
    one.add_point(1, {0});
    blocks += check(one);
  }
  std::printf("joint exchange plan: ok (%lld band blocks checked)\n", blocks);
  return 0;
}
