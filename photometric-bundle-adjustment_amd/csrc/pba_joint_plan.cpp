// pba_joint_plan.cpp — see pba_joint_plan.h.
#include "pba_joint_plan.h"

#include <algorithm>

#include "pba_gn_plan.h"
#include "pba_plan_lists.h"

namespace pba {
namespace detail {

bool build_joint_plan(const JointPlanInput& in, JointPlan& P) {
  const int nf = in.n_frames, np = in.n_pairs, npt = in.n_points, nb = in.n_blocks;
  const int nc = in.n_cams, N = nf + (nc > 0 ? nc : 0);  // block rows: keyframes, then cameras
  if (nf <= 0 || np < 0 || npt < 0 || nb < 0 || nc < 0) return false;
  for (int f = 0; nc > 0 && f < nf; ++f)
    if (!in.frame_cam || in.frame_cam[f] < 0 || in.frame_cam[f] >= nc) return false;
  for (int p = 0; p < np; ++p) {
    if (in.pair_host[p] < 0 || in.pair_host[p] >= nf || in.pair_target[p] < 0 || in.pair_target[p] >= nf) return false;
    if (in.pair_host[p] == in.pair_target[p]) return false;
  }
  for (int q = 0; q < npt; ++q)
    if (in.point_host[q] < 0 || in.point_host[q] >= nf) return false;
  for (int b = 0; b < nb; ++b) {
    if (in.block_pair[b] < 0 || in.block_pair[b] >= np || in.block_point[b] < 0 || in.block_point[b] >= npt) return false;
    if (in.pair_host[in.block_pair[b]] != in.point_host[in.block_point[b]]) return false;
  }
  csr_group(np, nb, in.block_pair, P.pair_ptr, P.pair_blocks);
  csr_group(npt, nb, in.block_point, P.pt_ptr, P.pt_blocks);
  frame_pair_lists(nf, np, in.pair_host, in.pair_target, P.frame_ptr, P.frame_pairs);
  auto target_of = [&](int b) { return in.pair_target[in.block_pair[b]]; };
  // skyline profile: every two keyframes of one point share a block of the reduced system
  P.first.assign(N, 0);  // (a camera's row starts at keyframe 0)
  for (int f = 0; f < nf; ++f) P.first[f] = f;
  for (int q = 0; q < npt; ++q) {
    if (P.pt_ptr[q] == P.pt_ptr[q + 1]) continue;
    int lo = in.point_host[q];
    for (int k = P.pt_ptr[q]; k < P.pt_ptr[q + 1]; ++k) lo = std::min(lo, target_of(P.pt_blocks[k]));
    P.first[in.point_host[q]] = std::min(P.first[in.point_host[q]], lo);
    for (int k = P.pt_ptr[q]; k < P.pt_ptr[q + 1]; ++k) {
      const int t = target_of(P.pt_blocks[k]);
      P.first[t] = std::min(P.first[t], lo);
    }
  }
  skyline_profile(P.first, P.row, P.last, P.colptr, P.colrows);
  P.n_sky = P.row[N];
  P.n_sky_kf = P.row[nf];
  auto sky = [&](int i, int j) { return P.row[i] + (j - P.first[i]); };  // i ≥ j ≥ first[i]
  // (self pairs are refused above; a pair without blocks lies in no point's span, so it takes no part)
  auto has_blocks = [&](int p) { return P.pair_ptr[p] < P.pair_ptr[p + 1]; };
  off_diagonal_pair_lists(np, in.pair_host, in.pair_target, P.first, std::vector<int>(P.row.begin(), P.row.begin() + nf + 1),
                          has_blocks, P.off_ptr, P.off_pairs);
  P.cam_ptr.clear();
  P.cam_pairs.clear();
  if (nc > 0) {
    // per camera its pairs; per border block (n_frames + c, j) the pairs of c that touch j — the rows in order, so the
    // lists continue the keyframes' CSR
    std::vector<int> pair_cam(np);
    for (int p = 0; p < np; ++p) pair_cam[p] = has_blocks(p) ? in.frame_cam[in.pair_target[p]] : -1;
    P.cam_ptr.assign(nc + 1, 0);
    for (int p = 0; p < np; ++p)
      if (pair_cam[p] >= 0) ++P.cam_ptr[pair_cam[p] + 1];
    csr_prefix(P.cam_ptr);
    P.cam_pairs.resize(P.cam_ptr[nc]);
    std::vector<int> at(P.cam_ptr.begin(), P.cam_ptr.end() - 1);
    for (int p = 0; p < np; ++p)
      if (pair_cam[p] >= 0) P.cam_pairs[at[pair_cam[p]]++] = p;
    P.off_ptr.resize(P.n_sky + 1);
    std::vector<std::vector<int>> per(nf);
    for (int c = 0; c < nc; ++c) {
      for (auto& v : per) v.clear();
      for (int k = P.cam_ptr[c]; k < P.cam_ptr[c + 1]; ++k) {
        const int p = P.cam_pairs[k];
        per[in.pair_host[p]].push_back(2 * p);
        per[in.pair_target[p]].push_back(2 * p + 1);
      }
      for (int j = 0; j < N; ++j) {
        const int s = sky(nf + c, j);
        if (j < nf) P.off_pairs.insert(P.off_pairs.end(), per[j].begin(), per[j].end());
        P.off_ptr[s + 1] = (int)P.off_pairs.size();
        if (j == nf + c) break;
      }
    }
  }
  // Schur terms per skyline block and entries per keyframe: two passes over the points' entries (count, fill)
  // (the block row of an entry: a keyframe, or n_frames + the camera of a camera part)
  auto frame_of = [&](int e) {
    return e < 0 ? in.point_host[~e] : e < nb ? target_of(e) : nf + in.frame_cam[target_of(e - nb)];
  };
  P.term_ptr.assign(P.n_sky + 1, 0);
  P.fe_ptr.assign(N + 1, 0);
  std::vector<int> at_t, at_f;
  std::vector<int> ent;
  for (int pass = 0; pass < 2; ++pass) {
    for (int q = 0; q < npt; ++q) {
      if (P.pt_ptr[q] == P.pt_ptr[q + 1]) continue;
      ent.clear();
      ent.push_back(~q);
      for (int k = P.pt_ptr[q]; k < P.pt_ptr[q + 1]; ++k) ent.push_back(P.pt_blocks[k]);
      for (int k = P.pt_ptr[q]; nc > 0 && k < P.pt_ptr[q + 1]; ++k) ent.push_back(nb + P.pt_blocks[k]);
      for (int a : ent) {
        const int fa = frame_of(a);
        if (pass == 0) ++P.fe_ptr[fa + 1];
        else P.fe_entries[at_f[fa]++] = a;
        for (int b : ent) {
          const int fb = frame_of(b);
          if (fa < fb) continue;
          const int s = sky(fa, fb);
          if (pass == 0) ++P.term_ptr[s + 1];
          else P.terms[at_t[s]++] = JointTerm{a, b};
        }
      }
    }
    if (pass == 0) {
      csr_prefix(P.term_ptr);
      csr_prefix(P.fe_ptr);
      P.terms.resize(P.term_ptr[P.n_sky]);
      P.fe_entries.resize(P.fe_ptr[N]);
      at_t.assign(P.term_ptr.begin(), P.term_ptr.end() - 1);
      at_f.assign(P.fe_ptr.begin(), P.fe_ptr.end() - 1);
    }
  }
  return true;
}

int joint_local_band(const std::vector<int>& first) {
  int band = 0;
  for (int i = 0; i < (int)first.size(); ++i) band = std::max(band, i - first[i]);
  return band;
}

bool build_joint_exchange(const std::vector<int>& first, const std::vector<int>& row, int K, JointExchangePlan& X) {
  const int nf = (int)first.size();
  if (nf <= 0 || (int)row.size() != nf + 1 || K < joint_local_band(first) || K > nf - 1) return false;
  X.K = K;
  X.stride = (long long)(K + 1) * 64 + kJointExTail;
  X.scalar_off = X.stride * nf;
  X.count = X.scalar_off + kJointExScalars;
  X.src.assign((size_t)nf * (K + 1), -1);
  X.first.resize(nf);
  for (int i = 0; i < nf; ++i) {
    X.first[i] = std::max(0, i - K);
    for (int j = first[i]; j <= i; ++j) X.src[(size_t)i * (K + 1) + (j - (i - K))] = row[i] + (j - first[i]);
  }
  skyline_profile(X.first, X.row, X.last, X.colptr, X.colrows);
  X.n_sky = X.row[nf];
  X.sky_i.resize(X.n_sky);
  X.sky_j.resize(X.n_sky);
  for (int i = 0; i < nf; ++i)
    for (int j = X.first[i]; j <= i; ++j) {
      X.sky_i[X.row[i] + (j - X.first[i])] = i;
      X.sky_j[X.row[i] + (j - X.first[i])] = j;
    }
  return true;
}

}  // namespace detail
}  // namespace pba
