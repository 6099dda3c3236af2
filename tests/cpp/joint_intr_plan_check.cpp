// Stand-alone checker of the joint plan with free intrinsics (csrc/pba_joint_plan.cpp, JointPlanInput::n_cams > 0): the
// cameras' block rows, their entries, border lists and per-camera pair lists against a brute-force restatement, and the
// keyframes' part against the plan without cameras, vector for vector.  Problems: random ones built here, and those of
// the file given as the first argument (tests/test_joint_intr_plan.py writes the test problems' structure there):
//   n_problems, then per problem  n_frames n_cams n_points n_blocks | frame_cam | point_host | block_point | block_target.
// Compiled with -fsanitize=address,undefined and run as a program.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "pba_joint_plan.h"

namespace pba {
namespace detail {
thread_local std::string g_last_error;  // (pba_gn_plan.cpp's: defined in pba_engine.hip in the full library)
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
  int nf = 0, nc = 0;
  std::vector<int> frame_cam, point_host, block_point, block_target;
  std::vector<int> pair_host, pair_target, block_pair;  // the engine's pairs: distinct (host, target), sorted
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
  JointPlanInput input(bool cams) const {
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
    if (cams) {
      in.n_cams = nc;
      in.frame_cam = frame_cam.data();
    }
    return in;
  }
};

template <class T>
static std::vector<T> slice(const std::vector<T>& v, int a, int b) {
  return std::vector<T>(v.begin() + a, v.begin() + b);
}

static bool same_terms(const std::vector<JointTerm>& a, const std::vector<JointTerm>& b, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (a[k].a != b[k].a || a[k].b != b[k].b) return false;
  return true;
}

static long long check(Problem& pb) {
  pb.pairs();
  const JointPlanInput in = pb.input(true);
  JointPlan P, K;
  CHECK(build_joint_plan(in, P));
  CHECK(build_joint_plan(pb.input(false), K));
  const int nf = pb.nf, nc = pb.nc, N = nf + nc, np = in.n_pairs, npt = in.n_points, nb = in.n_blocks;
  // the keyframes' part is the plan without cameras
  CHECK(K.cam_ptr.empty() && K.cam_pairs.empty() && K.n_sky_kf == K.n_sky && P.n_sky_kf == K.n_sky);
  CHECK(P.pair_ptr == K.pair_ptr && P.pair_blocks == K.pair_blocks && P.frame_ptr == K.frame_ptr &&
        P.frame_pairs == K.frame_pairs && P.pt_ptr == K.pt_ptr && P.pt_blocks == K.pt_blocks);
  CHECK((int)P.first.size() == N && (int)P.row.size() == N + 1 && (int)P.last.size() == N && (int)P.colptr.size() == N + 1);
  CHECK(slice(P.first, 0, nf) == K.first && slice(P.row, 0, nf + 1) == K.row);
  CHECK((int)P.off_ptr.size() == P.n_sky + 1 && (int)P.term_ptr.size() == P.n_sky + 1 && (int)P.fe_ptr.size() == N + 1);
  CHECK(slice(P.off_ptr, 0, K.n_sky + 1) == K.off_ptr && slice(P.off_pairs, 0, (int)K.off_pairs.size()) == K.off_pairs);
  CHECK(slice(P.term_ptr, 0, K.n_sky + 1) == K.term_ptr && same_terms(P.terms, K.terms, K.terms.size()));
  // the profile: the cameras' rows start at 0
  int n_sky = K.n_sky;
  for (int c = 0; c < nc; ++c) {
    CHECK(P.first[nf + c] == 0 && P.row[nf + c] == n_sky);
    n_sky += nf + c + 1;
  }
  CHECK(P.row[N] == n_sky && P.n_sky == n_sky);
  for (int k = 0; k < N; ++k) {
    std::vector<int> want;
    for (int i = k + 1; i < N; ++i)
      if (P.first[i] <= k) want.push_back(i);
    CHECK(slice(P.colrows, P.colptr[k], P.colptr[k + 1]) == want);
    CHECK(P.last[k] == (want.empty() ? k : want.back()));
  }
  // the pairs of each camera: those with blocks whose target has it
  std::vector<int> n_of_pair(np, 0);
  for (int b = 0; b < nb; ++b) ++n_of_pair[pb.block_pair[b]];
  CHECK((int)P.cam_ptr.size() == nc + 1);
  for (int c = 0; c < nc; ++c) {
    std::vector<int> want;
    for (int p = 0; p < np; ++p)
      if (n_of_pair[p] > 0 && pb.frame_cam[pb.pair_target[p]] == c) want.push_back(p);
    CHECK(slice(P.cam_pairs, P.cam_ptr[c], P.cam_ptr[c + 1]) == want);
  }
  CHECK(P.cam_ptr[nc] == (int)P.cam_pairs.size());
  // entries: the host part ~q, the point's blocks, then their camera parts nb + b
  auto row_of = [&](int e) {
    return e < 0 ? pb.point_host[~e] : e < nb ? pb.block_target[e] : nf + pb.frame_cam[pb.block_target[e - nb]];
  };
  auto entries = [&](int q) {
    std::vector<int> ent;
    for (int b = 0; b < nb; ++b)
      if (pb.block_point[b] == q) ent.push_back(b);
    const size_t n = ent.size();
    for (size_t k = 0; k < n; ++k) ent.push_back(nb + ent[k]);
    if (!ent.empty()) ent.insert(ent.begin(), ~q);
    return ent;
  };
  std::vector<std::vector<int>> ent(npt);
  for (int q = 0; q < npt; ++q) ent[q] = entries(q);
  // every block's terms and every row's entries in one pass over the points (points ascending, a then b in the point's
  // entry order), kept per block / per row
  std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> terms_of;
  std::vector<std::vector<int>> on_row(N);
  for (int q = 0; q < npt; ++q)
    for (int a : ent[q]) {
      on_row[row_of(a)].push_back(a);
      for (int b : ent[q])
        if (row_of(a) >= row_of(b)) terms_of[{row_of(a), row_of(b)}].emplace_back(a, b);
    }
  long long n_terms = 0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      if (j < P.first[i]) {  // no term falls outside the profile
        CHECK(terms_of.count({i, j}) == 0);
        continue;
      }
      const int s = P.row[i] + (j - P.first[i]);
      if (i >= nf) {  // a camera's row: the border lists
        std::vector<int> want;
        for (int p = 0; p < np && j < nf; ++p) {
          if (n_of_pair[p] == 0 || pb.frame_cam[pb.pair_target[p]] != i - nf) continue;
          if (pb.pair_host[p] == j) want.push_back(2 * p);
          if (pb.pair_target[p] == j) want.push_back(2 * p + 1);
        }
        CHECK(slice(P.off_pairs, P.off_ptr[s], P.off_ptr[s + 1]) == want);
      }
      const std::vector<std::pair<int, int>>& terms = terms_of[{i, j}];
      CHECK(P.term_ptr[s + 1] - P.term_ptr[s] == (int)terms.size());
      for (size_t k = 0; k < terms.size(); ++k) {
        const JointTerm& t = P.terms[P.term_ptr[s] + k];
        CHECK(t.a == terms[k].first && t.b == terms[k].second);
      }
      n_terms += (long long)terms.size();
    }
  CHECK(P.off_ptr[P.n_sky] == (int)P.off_pairs.size());
  long long all = 0, n_ent = 0;
  for (int q = 0; q < npt; ++q) {
    n_ent += (long long)ent[q].size();
    for (int a : ent[q])
      for (int b : ent[q]) all += row_of(a) >= row_of(b);
  }
  CHECK(n_terms == all && (long long)P.terms.size() == all);
  CHECK(P.fe_ptr[N] == n_ent && (long long)P.fe_entries.size() == n_ent);
  for (int f = 0; f < N; ++f) CHECK(slice(P.fe_entries, P.fe_ptr[f], P.fe_ptr[f + 1]) == on_row[f]);
  return n_terms;
}

static int read_int(std::FILE* f) {
  int v = 0;
  CHECK(std::fscanf(f, "%d", &v) == 1);
  return v;
}

int main(int argc, char** argv) {
  long long terms = 0;
  int n_file = 0;
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "r");
    CHECK(f != nullptr);
    n_file = read_int(f);
    for (int k = 0; k < n_file; ++k) {
      Problem pb;
      pb.nf = read_int(f);
      pb.nc = read_int(f);
      const int npt = read_int(f), nb = read_int(f);
      CHECK(pb.nf > 0 && pb.nc > 0 && npt >= 0 && nb >= 0);
      for (int i = 0; i < pb.nf; ++i) pb.frame_cam.push_back(read_int(f));
      for (int i = 0; i < npt; ++i) pb.point_host.push_back(read_int(f));
      for (int i = 0; i < nb; ++i) pb.block_point.push_back(read_int(f));
      for (int i = 0; i < nb; ++i) pb.block_target.push_back(read_int(f));
      terms += check(pb);
    }
    std::fclose(f);
  }
  // random problems: 1–3 cameras, cameras no keyframe has, points without blocks, idle keyframes
  std::mt19937 rng(11);
  for (int it = 0; it < 40; ++it) {
    Problem pb;
    pb.nf = 2 + (int)(rng() % 10);
    pb.nc = 1 + (int)(rng() % 3);
    const int npt = 1 + (int)(rng() % 20), nb = 1 + (int)(rng() % 70);
    for (int i = 0; i < pb.nf; ++i) pb.frame_cam.push_back((int)(rng() % pb.nc));
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
  // refused: a keyframe's camera out of range, no frame_cam
  {
    Problem pb;
    pb.nf = 3;
    pb.nc = 2;
    pb.frame_cam = {0, 1, 2};
    pb.point_host = {0};
    pb.block_point = {0};
    pb.block_target = {1};
    pb.pairs();
    JointPlan P;
    CHECK(!build_joint_plan(pb.input(true), P));
    JointPlanInput in = pb.input(true);
    in.frame_cam = nullptr;
    CHECK(!build_joint_plan(in, P));
    pb.frame_cam = {0, 1, 1};
    CHECK(build_joint_plan(pb.input(true), P));
  }
  std::printf("joint intrinsics plan: ok (%d problems from the file, %lld Schur terms checked)\n", n_file, terms);
  return 0;
}
