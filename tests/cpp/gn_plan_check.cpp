// Driver of tests/test_gn_plan.py: the invariants of the Gauss-Newton symbolic analysis (build_gn_plan, pba_gn_plan.cpp)
// — the index structures the GN kernels read without checking — on small topologies from a fixed LCG.  Host-only: built
// by g++ with AddressSanitizer + UndefinedBehaviorSanitizer together with pba_gn_plan.cpp.  Prints one JSON line (per
// case the counts and an FNV-1a hash of every plan vector) and exits non-zero on the first violated invariant.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "pba.h"
#include "pba_gn_plan.h"
#include "pba_host.h"

namespace pba {
namespace detail {
thread_local std::string g_last_error;  // defined in pba_engine.hip in the full library
}
}  // namespace pba

using namespace pba::detail;

#ifndef GN_PLAN_FN  // (a stand-in with the same signature can be checked by the same driver)
#define GN_PLAN_FN build_gn_plan
#else
int GN_PLAN_FN(const GnPlanInput& in, GnPlan& plan);
#endif

namespace {

const char* g_case = "";
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      fprintf(stderr, "case %s: line %d: violated: %s\n", g_case, __LINE__, #cond);  \
      exit(1);                                                                       \
    }                                                                                \
  } while (0)

struct Lcg {
  uint64_t s;
  int next(int n) {  // uniform in [0, n)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (int)((s >> 33) % (uint64_t)n);
  }
};

struct Topo {
  int nf = 0, n_cams = 0;
  std::vector<int> frame_cam, point_host, block_point, block_target, pair_of, pair_host, pair_target;
  std::vector<uint8_t> fixed;
  std::map<std::pair<int, int>, int> pair_idx;
  int add_point(int host) {
    point_host.push_back(host);
    return (int)point_host.size() - 1;
  }
  void add_block(int point, int target) {
    const std::pair<int, int> key{point_host[point], target};
    auto it = pair_idx.find(key);
    if (it == pair_idx.end()) {
      it = pair_idx.emplace(key, (int)pair_host.size()).first;
      pair_host.push_back(key.first);
      pair_target.push_back(target);
    }
    block_point.push_back(point);
    block_target.push_back(target);
    pair_of.push_back(it->second);
  }
  // a point of `host` with k distinct random targets among the frames [0, nt) other than its host
  void random_point(Lcg& r, int host, int k, int nt) {
    const int p = add_point(host);
    std::vector<int> ts;
    while ((int)ts.size() < k) {
      const int t = r.next(nt);
      if (t != host && std::find(ts.begin(), ts.end(), t) == ts.end()) ts.push_back(t);
    }
    for (int t : ts) add_block(p, t);
  }
};

struct Opts {
  int lpb = 4, nc = 0;
  bool walk = false, row_waves64 = false;
};

GnPlanInput make_input(const Topo& t, const Opts& o) {
  GnPlanInput in{};
  in.n_frames = t.nf;
  in.n_cams = t.n_cams;
  in.n_pairs = (int)t.pair_host.size();
  in.n_points = (int)t.point_host.size();
  in.n_blocks = (int)t.block_point.size();
  in.block_point_h = t.block_point.data();
  in.block_target_h = t.block_target.data();
  in.point_host_h = t.point_host.data();
  in.pair_of_h = t.pair_of.data();
  in.pair_host_h = t.pair_host.data();
  in.pair_target_h = t.pair_target.data();
  in.frame_cam_h = t.frame_cam.data();
  in.fixed_h = t.fixed.data();
  in.n_fixed = (int)t.fixed.size();
  in.lpb = o.lpb;
  in.ppl = 1;
  in.bpw = 256 / o.lpb;  // kBlockThreads / lpb
  in.nc = o.nc;
  in.test_pblk_walk = o.walk;
  in.test_row_waves64 = o.row_waves64;
  in.skyline_global = false;
  return in;
}

struct Counts {
  int chunks = 0, target_cuts = 0, schur = 0, noncanon = 0, sky = 0, border = 0, ir_waves = 0;
};

// ---- GN order, GN points, linearise chunks -----------------------------------------------------
// Returns the GN order (GN position → block), recovered from lin_rec.
std::vector<int> check_linearise(const GnPlanInput& in, const GnPlan& P, Counts& n) {
  const int nb = in.n_blocks;
  CHECK(P.n_chunks == (int)P.chunk_desc.size() && P.n_chunks > 0);
  CHECK(P.lin_rec.size() == (size_t)P.n_chunks * in.bpw);
  std::vector<int> order(nb, -1);
  std::vector<char> seen_block(nb, 0);
  size_t off = 0;
  int next = 0;
  for (int c = 0; c < P.n_chunks; ++c) {
    const PlanInt4 d = P.chunk_desc[c];
    CHECK(d.x == next && d.y >= 1 && d.y <= in.bpw && d.z >= 1 && d.z <= kChunkTargets && d.w == (int)off);
    std::vector<int> slot_target(d.z, -1);
    int host = -1;
    for (int s = 0; s < in.bpw; ++s) {
      const PlanInt4 r = P.lin_rec[(size_t)c * in.bpw + s];
      if (s >= d.y) {  // padding: the chunk's first record again
        const PlanInt4 r0 = P.lin_rec[(size_t)c * in.bpw];
        CHECK(r.x == r0.x && r.y == r0.y && r.z == r0.z && r.w == r0.w);
        continue;
      }
      CHECK(r.x >= 0 && r.x < nb && !seen_block[r.x]);
      seen_block[r.x] = 1;
      CHECK(r.w >= 0 && r.w < nb && order[r.w] < 0);  // lin_rec.w: a permutation of the GN positions
      order[r.w] = r.x;
      CHECK(r.y == in.block_point_h[r.x] && (r.z & 0xffffff) == in.pair_of_h[r.x]);
      const int h = in.point_host_h[r.y], slot = (int)((unsigned)r.z >> 24), t = in.block_target_h[r.x];
      CHECK(host < 0 || host == h);  // one host
      host = h;
      CHECK(slot < d.z && (slot_target[slot] < 0 || slot_target[slot] == t));  // the slot names the block's target
      slot_target[slot] = t;
    }
    for (int a = 0; a < d.z; ++a) {
      CHECK(slot_target[a] >= 0);
      for (int b = 0; b < a; ++b) CHECK(slot_target[a] != slot_target[b]);  // d.z distinct targets
    }
    if (d.z == kChunkTargets && d.y < in.bpw && c + 1 < P.n_chunks) {  // cut at kChunkTargets: the host goes on
      const PlanInt4 r1 = P.lin_rec[(size_t)(c + 1) * in.bpw];
      if (in.point_host_h[r1.y] == host) ++n.target_cuts;
    }
    next += d.y;
    off += SLOT_LIN_BASE + SLOT_LIN_T * d.z;
  }
  CHECK(next == nb && P.lin_slots == off);
  // the GN order: a permutation of the blocks (above), non-decreasing in (host, point, target)
  CHECK((int)P.gn_target.size() == nb);
  for (int g = 0; g < nb; ++g) {
    const int b = order[g], p = in.block_point_h[b];
    CHECK(P.gn_target[g] == in.block_target_h[b]);
    if (g == 0) continue;
    const int b0 = order[g - 1], p0 = in.block_point_h[b0];
    const int k0[3] = {in.point_host_h[p0], p0, in.block_target_h[b0]}, k1[3] = {in.point_host_h[p], p, in.block_target_h[b]};
    CHECK(std::lexicographical_compare(k0, k0 + 3, k1, k1 + 3) || std::equal(k0, k0 + 3, k1));
  }
  n.chunks = P.n_chunks;
  return order;
}

void check_points(const GnPlanInput& in, const GnPlan& P, const std::vector<int>& order) {
  const int ngp = P.n_gn_points;
  CHECK(ngp > 0 && (int)P.pt_first.size() == ngp && (int)P.pt_nblk.size() == ngp && (int)P.pt_orig.size() == ngp);
  CHECK((int)P.pt_host.size() == ngp && (int)P.pt_rec.size() == ngp && (int)P.pt_tgt.size() == ngp);
  CHECK(P.pt_first[0] == 0);
  for (int q = 0; q < ngp; ++q) {
    CHECK(P.pt_nblk[q] >= 1);
    CHECK(P.pt_first[q] + P.pt_nblk[q] == (q + 1 < ngp ? P.pt_first[q + 1] : in.n_blocks));
    CHECK(P.pt_orig[q] >= 0 && P.pt_orig[q] < in.n_points && P.pt_host[q] == in.point_host_h[P.pt_orig[q]]);
    CHECK(q == 0 || P.pt_orig[q] != P.pt_orig[q - 1]);
    for (int g = P.pt_first[q]; g < P.pt_first[q] + P.pt_nblk[q]; ++g) CHECK(in.block_point_h[order[g]] == P.pt_orig[q]);
    const PlanInt4 r = P.pt_rec[q], t = P.pt_tgt[q];
    CHECK(r.x == P.pt_first[q] && r.y == P.pt_nblk[q] && r.z == P.pt_host[q] && r.w == P.pt_orig[q]);
    const int t4[4] = {t.x, t.y, t.z, t.w};
    for (int u = 0; u < 4; ++u) CHECK(t4[u] == (u < P.pt_nblk[q] ? P.gn_target[P.pt_first[q] + u] : 0));
  }
  CHECK((int)P.pair_rec.size() == std::max(in.n_pairs, 1));
  for (int q = 0; q < in.n_pairs; ++q) {
    const PlanInt4 r = P.pair_rec[q];
    CHECK(r.x == in.pair_host_h[q] && r.y == in.pair_target_h[q] && r.z == in.frame_cam_h[r.x] && r.w == in.frame_cam_h[r.y]);
  }
}

// ---- Schur chunks ------------------------------------------------------------------------------
// Returns per chunk the frame of each local pose.
std::vector<std::vector<int>> check_schur(const GnPlanInput& in, const GnPlan& P, const std::vector<int>& order,
                                          std::vector<std::vector<char>>& pair_used, Counts& n) {
  const int ngp = P.n_gn_points, ns = P.n_schur;
  CHECK(ns > 0 && (int)P.schur_desc.size() == ns && (int)P.schur_aux.size() == ns && (int)P.schur_lvp4.size() == ns);
  CHECK((int)P.blk_lv.size() == in.n_blocks && P.pt_fb.size() == (size_t)ns * SCHUR_PTS);
  std::vector<std::vector<int>> frames(ns);
  pair_used.assign(ns, {});
  size_t off = 0, lds = 0;
  int next = 0, pair_off = 0, lvp_off = 0, max_nv = 1;
  for (int c = 0; c < ns; ++c) {
    const PlanInt4 d = P.schur_desc[c], ax = P.schur_aux[c];
    const int npts = d.y, nv = d.z;
    CHECK(d.x == next && npts >= 1 && npts <= SCHUR_PTS && nv >= 1 && nv <= 255 && d.w == (int)off);
    CHECK(npts == 1 || npts * nv <= SCHUR_W);
    std::vector<int>& fr = frames[c];
    fr.assign(nv, -1);
    fr[0] = P.pt_host[d.x];
    std::vector<int> lpair(nv, -1);
    std::vector<char> used(nv * nv, 0);
    int nblk = 0;
    for (int q = d.x; q < d.x + npts; ++q) {
      CHECK(P.pt_host[q] == fr[0]);  // one host
      const PlanInt2 fb = P.pt_fb[(size_t)c * SCHUR_PTS + (q - d.x)];
      CHECK(fb.x == P.pt_first[q] && fb.y == P.pt_nblk[q]);
      std::vector<int> lv{0};
      for (int g = P.pt_first[q]; g < P.pt_first[q] + P.pt_nblk[q]; ++g, ++nblk) {
        const int l = P.blk_lv[g];
        CHECK(l < nv && (fr[l] < 0 || fr[l] == P.gn_target[g]));  // blk_lv names gn_target
        fr[l] = P.gn_target[g];
        const int pr = in.pair_of_h[order[g]];
        CHECK(lpair[l] < 0 || lpair[l] == pr);
        lpair[l] = pr;
        lv.push_back(l);
      }
      for (int x : lv)
        for (int y : lv) used[std::min(x, y) * nv + std::max(x, y)] = 1;
    }
    for (int q = npts; q < SCHUR_PTS; ++q) {
      const PlanInt2 fb = P.pt_fb[(size_t)c * SCHUR_PTS + q];
      CHECK(fb.x == 0 && fb.y == 0);
    }
    for (int a = 0; a < nv; ++a) {
      CHECK(fr[a] >= 0);
      for (int b = 0; b < a; ++b) CHECK(fr[a] != fr[b]);  // nv distinct frames
    }
    // the pair list: a ≤ b, strictly increasing; every pair when canonical, else exactly the used ones
    CHECK(ax.x == pair_off && ax.z == lvp_off && ax.w == nblk);
    CHECK(ax.x + ax.y <= (int)P.schur_pairs.size());
    const bool canon = 6 * nv + 1 <= 32;
    if (!canon) ++n.noncanon;
    std::vector<char> listed(nv * nv, 0);
    for (int u = 0; u < ax.y; ++u) {
      const PlanUchar2 pr = P.schur_pairs[ax.x + u];
      CHECK(pr.x <= pr.y && pr.y < nv);
      if (u) {
        const PlanUchar2 p0 = P.schur_pairs[ax.x + u - 1];
        CHECK(p0.x < pr.x || (p0.x == pr.x && p0.y < pr.y));
      }
      listed[pr.x * nv + pr.y] = 1;
      pair_used[c].push_back(used[pr.x * nv + pr.y]);
    }
    for (int a = 0; a < nv; ++a)
      for (int b = a; b < nv; ++b) CHECK(listed[a * nv + b] == (canon ? 1 : used[a * nv + b]));
    // the local targets' pairs
    CHECK(ax.z + nv - 1 <= (int)P.schur_lvp.size());
    const PlanInt4 l4 = P.schur_lvp4[c];
    const int l4v[4] = {l4.x, l4.y, l4.z, l4.w};
    for (int l = 1; l < nv; ++l) {
      const int pr = P.schur_lvp[ax.z + l - 1];
      CHECK(pr == lpair[l] && in.pair_host_h[pr] == fr[0] && in.pair_target_h[pr] == fr[l]);
    }
    for (int l = 0; l < 4; ++l) CHECK(l4v[l] == (l < nv - 1 ? P.schur_lvp[ax.z + l] : 0));
    next += npts;
    pair_off += ax.y;
    lvp_off += nv - 1;
    off += 36 * (size_t)ax.y + 6 * nv;
    lds = std::max(lds, sizeof(double) * 6 * (size_t)npts * nv);
    max_nv = std::max(max_nv, nv);
  }
  CHECK(next == ngp && P.schur_doubles == off && (int)P.schur_pairs.size() == pair_off);
  CHECK((int)P.schur_lvp.size() == std::max(lvp_off, 1));
  CHECK(P.schur_rt_off == 12 * (max_nv - 1) && P.schur_lds == lds + sizeof(double) * P.schur_rt_off);
  n.schur = ns;
  return frames;
}

// ---- skyline profile and contribution lists ----------------------------------------------------
void check_profile(const GnPlanInput& in, const GnPlan& P) {
  const int nf = in.n_frames, nfs = nf + 2 * in.nc;
  CHECK(P.nfs == nfs && (int)P.sky_first.size() == nfs && (int)P.sky_row.size() == nfs + 1);
  CHECK((int)P.sky_last.size() == nfs && (int)P.sky_colptr.size() == nfs + 1);
  const std::vector<int>&first = P.sky_first, &rowp = P.sky_row;
  int band = 0;
  CHECK(rowp[0] == 0);
  for (int i = 0; i < nfs; ++i) {
    CHECK(first[i] >= 0 && first[i] <= i && (i < nf || first[i] == 0));
    CHECK(rowp[i + 1] == rowp[i] + (i - first[i] + 1));
    if (i < nf) band = std::max(band, i - first[i]);
  }
  CHECK(P.n_sky == rowp[nfs] && P.band == band);
  CHECK((int)P.sky_blk_i.size() == P.n_sky && (int)P.sky_blk_j.size() == P.n_sky);
  std::vector<int> diag, offd;
  for (int i = 0, s = 0; i < nfs; ++i)
    for (int j = first[i]; j <= i; ++j, ++s) {
      CHECK(P.sky_blk_i[s] == i && P.sky_blk_j[s] == j);
      (i == j ? diag : offd).push_back(s);
    }
  CHECK(P.n_sky_diag == nfs && diag == P.sky_diag);
  CHECK(P.sky_off == (offd.empty() ? std::vector<int>{0} : offd));
  int ncol = 0;
  for (int k = 0; k < nfs; ++k) {
    int last = k;
    CHECK(P.sky_colptr[k] == ncol);
    for (int i = k + 1; i < nfs; ++i)
      if (first[i] <= k) {
        last = i;
        CHECK(ncol < (int)P.sky_colrows.size() && P.sky_colrows[ncol] == i);
        ++ncol;
      }
    CHECK(P.sky_last[k] == last);
  }
  CHECK(P.sky_colptr[nfs] == ncol && (int)P.sky_colrows.size() == std::max(ncol, 1));
}

void check_contributions(const GnPlanInput& in, const GnPlan& P, const std::vector<std::vector<int>>& sframes,
                         const std::vector<std::vector<char>>& pair_used) {
  const int nf = in.n_frames, nfs = P.nfs;
  // every produced partial: (offset, C_SCHUR bit) → the frames (rows, columns) of its source orientation; g: its frame
  std::map<std::pair<int, int>, std::pair<int, int>> hsrc;
  std::map<std::pair<int, int>, int> gsrc;
  for (int c = 0; c < P.n_chunks; ++c) {
    const PlanInt4 d = P.chunk_desc[c];
    const int h = in.point_host_h[P.lin_rec[(size_t)c * in.bpw].y];
    hsrc[{d.w, 0}] = {h, h};
    gsrc[{d.w + 36, 0}] = h;
    std::vector<int> tg(d.z);
    for (int s = 0; s < d.y; ++s) {
      const PlanInt4 r = P.lin_rec[(size_t)c * in.bpw + s];
      tg[(unsigned)r.z >> 24] = in.block_target_h[r.x];
    }
    for (int j = 0; j < d.z; ++j) {
      const int bo = d.w + SLOT_LIN_BASE + SLOT_LIN_T * j;
      hsrc[{bo, 0}] = {h, tg[j]};
      hsrc[{bo + 36, 0}] = {tg[j], tg[j]};
      gsrc[{bo + 72, 0}] = tg[j];
    }
  }
  for (int s = 0; s < P.n_schur; ++s) {
    const PlanInt4 d = P.schur_desc[s], ax = P.schur_aux[s];
    for (int u = 0; u < ax.y; ++u) {
      const PlanUchar2 pr = P.schur_pairs[ax.x + u];
      if (pair_used[s][u]) hsrc[{d.w + 36 * u, C_SCHUR}] = {sframes[s][pr.x], sframes[s][pr.y]};
    }
    for (int a = 0; a < d.z; ++a) gsrc[{d.w + 36 * ax.y + 6 * a, C_SCHUR}] = sframes[s][a];
  }
  // … is consumed exactly once, in the block of its frames, transposed exactly when its rows < its columns
  CHECK((int)P.sky_cptr.size() == P.n_sky + 1 && P.sky_cptr[0] == 0);
  CHECK(P.sky_cptr[P.n_sky] == (int)hsrc.size() && (int)P.sky_contrib.size() == std::max((int)hsrc.size(), 1));
  for (int s = 0; s < P.n_sky; ++s) {
    CHECK(P.sky_cptr[s] <= P.sky_cptr[s + 1]);
    const int i = P.sky_blk_i[s], j = P.sky_blk_j[s];
    for (int k = P.sky_cptr[s]; k < P.sky_cptr[s + 1]; ++k) {
      const PlanInt2 cn = P.sky_contrib[k];
      CHECK((cn.y & ~(C_TRANSPOSE | C_SCHUR)) == 0);
      auto it = hsrc.find({cn.x, cn.y & C_SCHUR});
      CHECK(it != hsrc.end());
      const int fa = it->second.first, fb = it->second.second;
      CHECK(((cn.y & C_TRANSPOSE) != 0) == (fa < fb));
      CHECK(i == std::max(fa, fb) && j == std::min(fa, fb) && P.sky_first[i] <= j && j <= i);
      hsrc.erase(it);
    }
  }
  CHECK(hsrc.empty());
  CHECK((int)P.g_cptr.size() == nfs + 1 && P.g_cptr[0] == 0);
  CHECK(P.g_cptr[nfs] == (int)gsrc.size() && (int)P.g_contrib.size() == std::max((int)gsrc.size(), 1));
  for (int i = 0; i < nfs; ++i) {
    CHECK(P.g_cptr[i] <= P.g_cptr[i + 1] && (i < nf || P.g_cptr[i] == P.g_cptr[i + 1]));
    for (int k = P.g_cptr[i]; k < P.g_cptr[i + 1]; ++k) {
      const PlanInt2 cn = P.g_contrib[k];
      CHECK((cn.y & ~C_SCHUR) == 0);
      auto it = gsrc.find({cn.x, cn.y});
      CHECK(it != gsrc.end() && it->second == i);
      gsrc.erase(it);
    }
  }
  CHECK(gsrc.empty());
}

void check_fixed(const GnPlanInput& in, const GnPlan& P) {
  const int nf = in.n_frames, nc = in.nc;
  std::vector<char> observed(nf, 0), cam_target(std::max(nc, 1), 0);
  for (int b = 0; b < in.n_blocks; ++b) {
    observed[in.point_host_h[in.block_point_h[b]]] = 1;
    observed[in.block_target_h[b]] = 1;
    if (nc) cam_target[in.frame_cam_h[in.block_target_h[b]]] = 1;
  }
  CHECK((int)P.fixed.size() == P.nfs && (int)P.observed.size() == nf && (int)P.fixed_req.size() == nf);
  for (int i = 0; i < nf; ++i) {
    const bool req = i < in.n_fixed && in.fixed_h[i];
    CHECK(P.observed[i] == observed[i] && P.fixed_req[i] == req && P.fixed[i] == (req || !observed[i]));
  }
  for (int c = 0; c < nc; ++c) CHECK(P.fixed[nf + 2 * c] == !cam_target[c] && P.fixed[nf + 2 * c + 1] == !cam_target[c]);
}

// ---- free intrinsics: border lists and wave table ----------------------------------------------
void check_border(const GnPlanInput& in, const GnPlan& P, const std::vector<int>& order, bool walk, Counts& n) {
  const int nb = in.n_blocks, nf = in.n_frames, nc = in.nc, nu = nf + nc, ngp = P.n_gn_points;
  CHECK((int)P.ib_rec.size() == nb && (int)P.ib_cam.size() == nb);
  for (int g = 0; g < nb; ++g) {
    const PlanInt4 r = P.ib_rec[g];
    CHECK(r.x == order[g] && r.y == in.block_point_h[r.x] && r.z == in.point_host_h[r.y] && r.w == in.block_target_h[r.x]);
    CHECK(P.ib_cam[g] == in.frame_cam_h[r.w] && P.ib_cam[g] < nc);
  }
  CHECK((int)P.ib_bptr.size() == nc * nu + 1 && (int)P.ib_pptr.size() == nc * nu + 1);
  CHECK(P.ib_bptr[0] == 0 && P.ib_pptr[0] == 0 && P.ib_plist.size() == P.ib_pblk.size());
  CHECK((int)P.ib_blist.size() == std::max(P.ib_bptr[nc * nu], 1) && (int)P.ib_plist.size() == std::max(P.ib_pptr[nc * nu], 1));
  for (int c = 0; c < nc; ++c)
    for (int u = 0; u < nu; ++u) {
      const int L = c * nu + u;
      CHECK(P.ib_bptr[L] <= P.ib_bptr[L + 1] && P.ib_pptr[L] <= P.ib_pptr[L + 1]);
      int expect = 0;  // the list is complete: every block of camera c that touches u, once per way it touches
      for (int g = 0; g < nb; ++g)
        if (P.ib_cam[g] == c)
          expect += u < nf ? (P.ib_rec[g].z == u) + (P.ib_rec[g].w == u) : (u - nf == c);
      CHECK(P.ib_bptr[L + 1] - P.ib_bptr[L] == expect);
      for (int k = P.ib_bptr[L]; k < P.ib_bptr[L + 1]; ++k) {
        const int g = P.ib_blist[k] & 0x7fffffff;
        const bool hosted = P.ib_blist[k] < 0;  // bit 31
        CHECK(g < nb && P.ib_cam[g] == c);
        if (u < nf) CHECK(hosted ? P.ib_rec[g].z == u : P.ib_rec[g].w == u);
        else CHECK(!hosted && u - nf == c);
        if (u < nf && P.ib_rec[g].z == u && P.ib_rec[g].w != u) CHECK(hosted);
      }
      for (int k = P.ib_pptr[L]; k < P.ib_pptr[L + 1]; ++k) {
        const int q = P.ib_plist[k];
        CHECK(q >= 0 && q < ngp);
        bool has_c = false, cam_u = false;
        int n_u = 0, blk_u = -1;
        for (int g = P.pt_first[q]; g < P.pt_first[q] + P.pt_nblk[q]; ++g) {
          has_c = has_c || P.ib_cam[g] == c;
          cam_u = cam_u || (u >= nf && P.ib_cam[g] == u - nf);
          if (P.gn_target[g] == u) {
            ++n_u;
            blk_u = g;
          }
        }
        const bool hosts = u < nf && P.pt_host[q] == u;
        CHECK(has_c && (hosts || n_u > 0 || cam_u));
        if (u >= nf || hosts) CHECK(P.ib_pblk[k] == -1);
        else CHECK(P.ib_pblk[k] == (n_u == 1 && !walk ? blk_u : -2));
      }
    }
  n.border = P.ib_bptr[nc * nu] + P.ib_pptr[nc * nu];
}

void check_waves(const GnPlanInput& in, const GnPlan& P, bool row_waves64, Counts& n) {
  bool long_point = false;
  for (int q = 0; q < P.n_gn_points; ++q) long_point = long_point || P.pt_nblk[q] > 64;
  CHECK((P.ir_waves == 0) == (long_point || row_waves64));
  CHECK((int)P.ir_wave.size() == P.ir_waves);
  int next = 0, q = 0;
  for (int w = 0; w < P.ir_waves; ++w) {
    const PlanInt4 r = P.ir_wave[w];
    CHECK(r.x == next && r.y >= 1 && r.y <= 64 && r.z == q && r.w == 0);
    int end = r.x;  // whole points only
    while (q < P.n_gn_points && end < r.x + r.y) end += P.pt_nblk[q++];
    CHECK(end == r.x + r.y);
    next = end;
  }
  if (P.ir_waves) CHECK(next == in.n_blocks && q == P.n_gn_points);
  n.ir_waves = P.ir_waves;
}

// ---- hashes and cases --------------------------------------------------------------------------
template <class T>
uint64_t fnv(const std::vector<T>& v) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

void print_hashes(const GnPlan& P) {
#define H(name) printf("%s\"" #name "\": \"%016llx\"", sep, (unsigned long long)fnv(P.name)), sep = ", "
  const char* sep = "";
  H(lin_rec); H(chunk_desc); H(pt_first); H(pt_nblk); H(pt_orig); H(pt_host); H(gn_target); H(pt_rec); H(pt_tgt); H(pt_fb);
  H(schur_desc); H(schur_aux); H(schur_lvp4); H(schur_pairs); H(blk_lv); H(schur_lvp);
  H(sky_first); H(sky_row); H(sky_last); H(sky_colptr); H(sky_colrows); H(sky_cptr); H(g_cptr); H(sky_blk_i); H(sky_blk_j);
  H(sky_diag); H(sky_off); H(sky_contrib); H(g_contrib); H(fixed); H(observed); H(fixed_req); H(pair_rec);
  H(ib_rec); H(ir_wave); H(ib_cam); H(ib_bptr); H(ib_blist); H(ib_pptr); H(ib_plist); H(ib_pblk);
#undef H
}

bool g_first_case = true;
Counts run_case(const char* name, const Topo& t, const Opts& o) {
  g_case = name;
  const GnPlanInput in = make_input(t, o);
  GnPlan P;
  CHECK(GN_PLAN_FN(in, P) == PBA_OK);
  Counts n;
  const std::vector<int> order = check_linearise(in, P, n);
  check_points(in, P, order);
  std::vector<std::vector<char>> pair_used;
  const std::vector<std::vector<int>> sframes = check_schur(in, P, order, pair_used, n);
  check_profile(in, P);
  check_contributions(in, P, sframes, pair_used);
  check_fixed(in, P);
  n.sky = P.n_sky;
  if (o.nc) {
    check_border(in, P, order, o.walk, n);
    check_waves(in, P, o.row_waves64, n);
  } else {
    CHECK(P.ib_rec.empty() && P.ib_blist.empty() && P.ir_wave.empty() && P.ir_waves == 0);
  }
  printf("%s\"%s\": {\"chunks\": %d, \"target_cuts\": %d, \"schur\": %d, \"noncanon\": %d, \"sky\": %d, \"border\": %d, "
         "\"ir_waves\": %d, \"hash\": {",
         g_first_case ? "" : ", ", name, n.chunks, n.target_cuts, n.schur, n.noncanon, n.sky, n.border, n.ir_waves);
  print_hashes(P);
  printf("}}");
  g_first_case = false;
  return n;
}

Topo frames(int nf, int n_cams) {
  Topo t;
  t.nf = nf;
  t.n_cams = n_cams;
  for (int f = 0; f < nf; ++f) t.frame_cam.push_back(f % n_cams);
  return t;
}

Topo topo_a() {  // 6 frames, 2 cameras, 40 points of 1–4 targets; frame 0 requested constant (a list shorter than nf)
  Lcg r{1};
  Topo t = frames(6, 2);
  for (int p = 0; p < 40; ++p) t.random_point(r, r.next(6), 1 + r.next(4), 6);
  t.fixed = {1, 0, 0};
  return t;
}
Topo topo_c() {  // one host with 300 points (Schur chunks cut at SCHUR_PTS), and a few elsewhere
  Lcg r{3};
  Topo t = frames(5, 1);
  for (int p = 0; p < 300; ++p) t.random_point(r, 0, 1 + r.next(3), 5);
  for (int p = 0; p < 7; ++p) t.random_point(r, 1 + r.next(4), 1 + r.next(2), 5);
  return t;
}
Topo topo_d() {  // host 0's 12 points observe the 9 targets 1 … 9: 10 local poses, 12 blocks per target
  Lcg r{4};
  Topo t = frames(10, 2);
  for (int p = 0; p < 12; ++p) {
    const int q = t.add_point(0);
    for (int f = 1; f <= 9; ++f) t.add_block(q, f);
  }
  for (int p = 0; p < 5; ++p) t.random_point(r, 1 + r.next(9), 1 + r.next(3), 10);
  return t;
}
Topo topo_e() {  // 72 frames, one point of 70 blocks, 20 points of 2: 110 blocks (mod 256 in 1 … 192)
  Lcg r{5};
  Topo t = frames(72, 1);
  const int q = t.add_point(3);
  for (int f = 0, k = 0; k < 70; ++f)
    if (f != 3) {
      t.add_block(q, f);
      ++k;
    }
  for (int p = 0; p < 20; ++p) t.random_point(r, r.next(72), 2, 72);
  return t;
}
Topo topo_f() {  // frame 5 untouched; camera 2 (frames 4, 5) never a target's camera: frame 4 only hosts
  Lcg r{6};
  Topo t = frames(6, 3);
  t.frame_cam = {0, 1, 0, 1, 2, 2};
  for (int p = 0; p < 25; ++p) t.random_point(r, r.next(5), 1 + r.next(3), 4);
  t.random_point(r, 4, 2, 4);
  const int q = t.add_point(0);  // two blocks of one point target keyframe 1: ib_pblk −2 (walk the point's blocks)
  t.add_block(q, 1);
  t.add_block(q, 2);
  t.add_block(q, 1);
  return t;
}

}  // namespace

int main() {
  printf("{");
  const Topo a = topo_a(), c = topo_c(), d = topo_d(), e = topo_e(), f = topo_f();
  Opts o4, o8, b, g;
  o8.lpb = 8;
  b.nc = 2;
  g.nc = 2;
  g.walk = g.row_waves64 = true;
  run_case("a", a, o4);
  run_case("a_lpb8", a, o8);  // (i): bpw = 64 and 32
  run_case("b", a, b);
  const Counts nc_ = run_case("c", c, o4);
  run_case("c_lpb8", c, o8);
  const Counts nd = run_case("d", d, o4);
  run_case("d_lpb8", d, o8);
  Opts oe;
  oe.nc = 1;
  g_case = "e";
  CHECK(e.block_point.size() % 256 >= 1 && e.block_point.size() % 256 <= 192);
  const Counts ne = run_case("e", e, oe);
  Opts of;
  of.nc = 3;
  run_case("f", f, of);
  const Counts ng = run_case("g", a, g);
  g_case = "counts";
  CHECK(nc_.schur >= 3 && nd.noncanon >= 1 && nd.target_cuts >= 1 && ne.ir_waves == 0 && ng.ir_waves == 0);
  {  // (h) a point observed by 256 keyframes (its host and 255 targets): an error, not a plan
    g_case = "h";
    Topo t = frames(256, 1);
    const int q = t.add_point(0);
    for (int f2 = 1; f2 < 256; ++f2) t.add_block(q, f2);
    const GnPlanInput in = make_input(t, o4);
    GnPlan P;
    CHECK(GN_PLAN_FN(in, P) == PBA_ERR_INVALID_ARGUMENT);
    CHECK(g_last_error == "a point observes too many keyframes");
    printf(", \"h\": {\"error\": \"%s\"}", g_last_error.c_str());
  }
  printf("}\n");
  return 0;
}
