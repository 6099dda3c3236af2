// pba_gn_plan.cpp — the symbolic analysis of a Gauss-Newton problem (pba_gn_plan.h): GN block order, chunks, slot
// layouts, skyline profile, contribution lists and the free-intrinsics border lists.  Host-only (pba_host.h, no HIP).
#include "pba_gn_plan.h"

#include <algorithm>
#include <map>
#include <numeric>
#include <utility>

#include "pba.h"
#include "pba_host.h"

namespace pba {
namespace detail {

namespace {

// What the stages hand on to each other besides the plan's own vectors.
struct Work {
  std::vector<int> order;  // GN position → block
  std::vector<int> lpos;   // linearise position → GN position
  std::vector<uint8_t> blt;  // linearise position → local target slot in its chunk
  std::vector<std::vector<int>> chunk_targets;
  std::vector<int> chunk_host;
  std::vector<std::vector<int>> schur_poses;
  std::vector<std::vector<std::pair<int, int>>> schur_used;
  std::vector<std::vector<char>> schur_used_flag;
};

// GN order (host, point, target), and the linearise order: each host's GN range regrouped by target (stable), so a
// chunk's blocks of one target are consecutive (one matrix-core chain per target run in linearize_kernel)
void order_blocks(const GnPlanInput& in, Work& W, GnPlan& P) {
  const int nb = in.n_blocks;
  const int* ph = in.point_host_h;
  W.order.resize(nb);
  std::iota(W.order.begin(), W.order.end(), 0);
  std::stable_sort(W.order.begin(), W.order.end(), [&](int a, int b) {
    const int pa_ = in.block_point_h[a], pb_ = in.block_point_h[b];
    if (ph[pa_] != ph[pb_]) return ph[pa_] < ph[pb_];
    if (pa_ != pb_) return pa_ < pb_;
    return in.block_target_h[a] < in.block_target_h[b];
  });
  std::vector<int>& gtgt = P.gn_target;
  gtgt.resize(nb);
  for (int i = 0; i < nb; ++i) gtgt[i] = in.block_target_h[W.order[i]];
  W.lpos.resize(nb);
  std::iota(W.lpos.begin(), W.lpos.end(), 0);
  for (int i = 0; i < nb;) {
    const int h = ph[in.block_point_h[W.order[i]]];
    int j = i;
    while (j < nb && ph[in.block_point_h[W.order[j]]] == h) ++j;
    std::stable_sort(W.lpos.begin() + i, W.lpos.begin() + j, [&](int x, int y) { return gtgt[x] < gtgt[y]; });
    i = j;
  }
}

// linearise chunks, and their records: chunk slot → {block, point, pair | local target slot << 24, GN position}
void linearise_chunks(const GnPlanInput& in, Work& W, GnPlan& P) {
  const int nb = in.n_blocks;
  const int* ph = in.point_host_h;
  const std::vector<int>&order = W.order, &lpos = W.lpos, &gtgt = P.gn_target;
  std::vector<PlanInt4>& cdesc = P.chunk_desc;
  W.blt.resize(nb);
  size_t off = 0;
  for (int i = 0; i < nb;) {
    const int h = ph[in.block_point_h[order[lpos[i]]]];
    int j = i;
    std::vector<int> tg;
    while (j < nb && j - i < in.bpw && ph[in.block_point_h[order[lpos[j]]]] == h) {
      const int t = gtgt[lpos[j]];
      auto it = std::find(tg.begin(), tg.end(), t);
      if (it == tg.end() && (int)tg.size() == kChunkTargets) break;  // a chunk spans ≤ kChunkTargets targets
      W.blt[j] = (uint8_t)(it - tg.begin());
      if (it == tg.end()) tg.push_back(t);
      ++j;
    }
    cdesc.push_back(PlanInt4{i, j - i, (int)tg.size(), (int)off});
    off += SLOT_LIN_BASE + SLOT_LIN_T * tg.size();
    W.chunk_targets.push_back(tg);
    W.chunk_host.push_back(h);
    i = j;
  }
  P.lin_slots = off;
  P.n_chunks = (int)cdesc.size();
  P.lin_rec.resize((size_t)P.n_chunks * in.bpw);
  for (int c = 0; c < P.n_chunks; ++c)
    for (int s = 0; s < in.bpw; ++s) {
      const int i = cdesc[c].x + (s < cdesc[c].y ? s : 0), b = order[lpos[i]];
      P.lin_rec[(size_t)c * in.bpw + s] =
          PlanInt4{b, in.block_point_h[b], in.pair_of_h[b] | ((int)W.blt[i] << 24), lpos[i]};
    }
}

// GN points (the runs of one point in the GN order) and their records
void gn_points(const GnPlanInput& in, const Work& W, GnPlan& P) {
  const int nb = in.n_blocks;
  for (int i = 0; i < nb;) {
    const int p = in.block_point_h[W.order[i]];
    int j = i;
    while (j < nb && in.block_point_h[W.order[j]] == p) ++j;
    P.pt_first.push_back(i);
    P.pt_nblk.push_back(j - i);
    P.pt_orig.push_back(p);
    P.pt_host.push_back(in.point_host_h[p]);
    i = j;
  }
  const int ngp = (int)P.pt_first.size();
  P.n_gn_points = ngp;
  P.pt_rec.resize(ngp);
  P.pt_tgt.resize(ngp);
  for (int q = 0; q < ngp; ++q) {
    P.pt_rec[q] = PlanInt4{P.pt_first[q], P.pt_nblk[q], P.pt_host[q], P.pt_orig[q]};
    int t4[4] = {0, 0, 0, 0};
    for (int u = 0; u < 4 && u < P.pt_nblk[q]; ++u) t4[u] = P.gn_target[P.pt_first[q] + u];
    P.pt_tgt[q] = PlanInt4{t4[0], t4[1], t4[2], t4[3]};
  }
  P.pair_rec.assign(std::max(in.n_pairs, 1), PlanInt4{0, 0, 0, 0});
  for (int q = 0; q < in.n_pairs; ++q) {
    const int h = in.pair_host_h[q], t = in.pair_target_h[q];
    P.pair_rec[q] = PlanInt4{h, t, in.frame_cam_h[h], in.frame_cam_h[t]};
  }
}

// Schur chunks: ≤ SCHUR_PTS points of one host, their local poses (the host first), pair slots and partial offsets
int schur_chunks(const GnPlanInput& in, Work& W, GnPlan& P) {
  const int ngp = P.n_gn_points;
  const std::vector<int>&pfirst = P.pt_first, &pnblk = P.pt_nblk, &phost = P.pt_host, &gtgt = P.gn_target;
  std::vector<PlanInt4>&sdesc = P.schur_desc, &saux = P.schur_aux;
  std::vector<PlanUchar2>& spairs = P.schur_pairs;
  std::vector<int>& lvp = P.schur_lvp;
  std::vector<uint8_t>& blv = P.blk_lv;
  P.schur_lds = 0;
  int max_nv = 1;
  blv.assign(in.n_blocks, 0);
  size_t soff = 0;
  for (int p = 0; p < ngp;) {
    const int h = phost[p];
    std::vector<int> poses{h};
    int q = p;
    while (q < ngp && q - p < SCHUR_PTS && phost[q] == h) {
      std::vector<int> add;
      for (int b = pfirst[q]; b < pfirst[q] + pnblk[q]; ++b)
        if (std::find(poses.begin(), poses.end(), gtgt[b]) == poses.end() &&
            std::find(add.begin(), add.end(), gtgt[b]) == add.end())
          add.push_back(gtgt[b]);
      const int nv = (int)(poses.size() + add.size());
      if (q > p && ((q - p + 1) * nv > SCHUR_W || nv > 255)) break;
      if (nv > 255 || nv > SCHUR_W) return fail(PBA_ERR_INVALID_ARGUMENT, "a point observes too many keyframes");
      poses.insert(poses.end(), add.begin(), add.end());
      ++q;
    }
    const int nv = (int)poses.size();
    std::vector<char> used(nv * nv, 0);
    std::vector<int> lpair(nv, 0);  // the pair (host, poses[l]) of each local target
    for (int r = p; r < q; ++r) {
      std::vector<int> lv{0};
      for (int b = pfirst[r]; b < pfirst[r] + pnblk[r]; ++b) {
        const int l = (int)(std::find(poses.begin(), poses.end(), gtgt[b]) - poses.begin());
        blv[b] = (uint8_t)l;
        lpair[l] = in.pair_of_h[W.order[b]];
        lv.push_back(l);
      }
      for (int x : lv)
        for (int y : lv) used[std::min(x, y) * nv + std::max(x, y)] = 1;
    }
    // pair slots: the used pairs, or every pair (a ≤ b) in canonical order when the chunk takes the matrix-core path
    // of schur_kernel (≤ 5 local poses; unused pairs are zero blocks no contribution list references)
    const bool canon = nv * 6 + 1 <= 32;
    std::vector<std::pair<int, int>> up;
    std::vector<char> upu;
    for (int x = 0; x < nv; ++x)
      for (int y = x; y < nv; ++y)
        if (canon || used[x * nv + y]) {
          up.emplace_back(x, y);
          upu.push_back(used[x * nv + y]);
        }
    const int fb0 = pfirst[p], nbc = pfirst[q - 1] + pnblk[q - 1] - fb0;
    saux.push_back(PlanInt4{(int)spairs.size(), (int)up.size(), (int)lvp.size(), nbc});
    lvp.insert(lvp.end(), lpair.begin() + 1, lpair.end());
    max_nv = std::max(max_nv, nv);
    for (auto& pr : up) spairs.push_back(PlanUchar2{(unsigned char)pr.first, (unsigned char)pr.second});
    sdesc.push_back(PlanInt4{p, q - p, nv, (int)soff});
    P.schur_lds = std::max<size_t>(P.schur_lds, sizeof(double) * 6 * (size_t)(q - p) * nv);
    soff += 36 * up.size() + 6 * nv;
    W.schur_poses.push_back(poses);
    W.schur_used.push_back(up);
    W.schur_used_flag.push_back(upu);
    p = q;
  }
  P.schur_doubles = soff;
  P.schur_rt_off = 12 * (max_nv - 1);  // the chunks' target poses, then W (schur_chunk)
  P.schur_lds += sizeof(double) * P.schur_rt_off;
  P.n_schur = (int)sdesc.size();
  // chunk c's point p → {first GN block, block count} at c · SCHUR_PTS + p (schur_kernel reads it with its descriptor)
  P.pt_fb.assign((size_t)P.n_schur * SCHUR_PTS, PlanInt2{0, 0});
  for (int c = 0; c < P.n_schur; ++c)
    for (int q = 0; q < sdesc[c].y; ++q)
      P.pt_fb[(size_t)c * SCHUR_PTS + q] = PlanInt2{pfirst[sdesc[c].x + q], pnblk[sdesc[c].x + q]};
  P.schur_lvp4.assign(sdesc.size(), PlanInt4{0, 0, 0, 0});
  for (size_t c = 0; c < sdesc.size(); ++c) {
    int l4[4] = {0, 0, 0, 0};
    for (int l = 0; l < 4 && l < sdesc[c].z - 1; ++l) l4[l] = lvp[saux[c].z + l];
    P.schur_lvp4[c] = PlanInt4{l4[0], l4[1], l4[2], l4[3]};
  }
  if (P.schur_lvp4.empty()) P.schur_lvp4.push_back(PlanInt4{0, 0, 0, 0});
  if (lvp.empty()) lvp.push_back(0);
  return PBA_OK;
}

// reduced camera system structure: lower blocks (i ≥ j), the skyline profile over them and each block's / each frame's
// contribution list; the constant frames
void reduced_system(const GnPlanInput& in, const Work& W, GnPlan& P) {
  const int nf = in.n_frames, nc = in.nc, nfs = nf + 2 * nc;
  std::map<std::pair<int, int>, std::vector<PlanInt2>> contrib;
  std::vector<std::vector<PlanInt2>> gcon(nf);
  auto add = [&](int fa, int fb, int o, int flags) {  // contribution block in orientation (fa rows, fb cols)
    if (fa >= fb) contrib[{fa, fb}].push_back(PlanInt2{o, flags});
    else contrib[{fb, fa}].push_back(PlanInt2{o, flags | C_TRANSPOSE});
  };
  std::vector<uint8_t>& observed = P.observed;
  observed.assign(nf, 0);
  for (int c = 0; c < P.n_chunks; ++c) {
    const int h = W.chunk_host[c], o = P.chunk_desc[c].w;
    observed[h] = 1;
    add(h, h, o, 0);
    gcon[h].push_back(PlanInt2{o + 36, 0});
    for (size_t j = 0; j < W.chunk_targets[c].size(); ++j) {
      const int t = W.chunk_targets[c][j], bo = o + SLOT_LIN_BASE + SLOT_LIN_T * (int)j;
      observed[t] = 1;
      add(h, t, bo, 0);
      add(t, t, bo + 36, 0);
      gcon[t].push_back(PlanInt2{bo + 72, 0});
    }
  }
  for (int s = 0; s < P.n_schur; ++s) {
    const auto& poses = W.schur_poses[s];
    const int o = P.schur_desc[s].w;
    for (size_t u = 0; u < W.schur_used[s].size(); ++u) {
      if (!W.schur_used_flag[s][u]) continue;
      const int fa = poses[W.schur_used[s][u].first], fb = poses[W.schur_used[s][u].second];
      add(fa, fb, o + 36 * (int)u, C_SCHUR);
    }
    for (size_t a = 0; a < poses.size(); ++a)
      gcon[poses[a]].push_back(PlanInt2{o + 36 * (int)W.schur_used[s].size() + 6 * (int)a, C_SCHUR});
  }
  // free intrinsics (geometric): two system frames per camera after the keyframes, a dense border (profile from 0)
  P.nfs = nfs;
  for (int i = 0; i < nfs; ++i) contrib[{i, i}];  // every diagonal block exists
  std::vector<int>&first = P.sky_first, &rowp = P.sky_row;
  first.resize(nfs);
  for (int i = 0; i < nfs; ++i) first[i] = i < nf ? i : 0;
  for (auto& kv : contrib) first[kv.first.first] = std::min(first[kv.first.first], kv.first.second);
  skyline_profile(first, rowp, P.sky_last, P.sky_colptr, P.sky_colrows);
  P.n_sky = rowp[nfs];
  P.band = 0;  // over the keyframes (the free-intrinsics border rows start at frame 0)
  for (int i = 0; i < nf; ++i) P.band = std::max(P.band, i - first[i]);
  std::vector<int>&cptr = P.sky_cptr, &bi = P.sky_blk_i, &bj = P.sky_blk_j;
  cptr.assign(P.n_sky + 1, 0);
  bi.resize(P.n_sky);
  bj.resize(P.n_sky);
  std::vector<std::vector<PlanInt2>> per(P.n_sky);
  for (int i = 0; i < nfs; ++i)
    for (int j = first[i]; j <= i; ++j) {
      const int s = rowp[i] + (j - first[i]);
      bi[s] = i;
      bj[s] = j;
    }
  for (auto& kv : contrib) {
    const int s = rowp[kv.first.first] + (kv.first.second - first[kv.first.first]);
    per[s] = kv.second;
  }
  std::vector<PlanInt2>&flat = P.sky_contrib, &gflat = P.g_contrib;
  for (int s = 0; s < P.n_sky; ++s) {
    cptr[s] = (int)flat.size();
    flat.insert(flat.end(), per[s].begin(), per[s].end());
  }
  cptr[P.n_sky] = (int)flat.size();
  P.g_cptr.resize(nfs + 1);
  for (int i = 0; i < nfs; ++i) {
    P.g_cptr[i] = (int)gflat.size();
    if (i < nf) gflat.insert(gflat.end(), gcon[i].begin(), gcon[i].end());
  }
  P.g_cptr[nfs] = (int)gflat.size();
  if (flat.empty()) flat.push_back(PlanInt2{0, 0});
  if (gflat.empty()) gflat.push_back(PlanInt2{0, 0});
  for (int q = 0; q < (int)bi.size(); ++q) (bi[q] == bj[q] ? P.sky_diag : P.sky_off).push_back(q);
  P.n_sky_diag = (int)P.sky_diag.size();
  if (P.sky_diag.empty()) P.sky_diag.push_back(0);
  if (P.sky_off.empty()) P.sky_off.push_back(0);
  // constant frames: requested + never observed (a camera whose intrinsics no block projects with: border_lists)
  P.fixed.assign(nfs, 0);
  for (int i = 0; i < nf; ++i) P.fixed[i] = (i < in.n_fixed && in.fixed_h[i]) || !observed[i];
  P.fixed_req.assign(nf, 0);
  for (int i = 0; i < nf && i < in.n_fixed; ++i) P.fixed_req[i] = in.fixed_h[i];
}

// the border's CSR lists: unit pair (camera c, unit u), u < nf keyframe u, u ≥ nf camera u − nf; direct terms from
// the blocks whose target camera is c and that touch u (host or target u; u = c: every block of camera c), Schur
// terms from the points with a block of camera c that touch u (a block of keyframe u / of camera u − nf)
void border_lists(const GnPlanInput& in, const Work& W, GnPlan& P) {
  const int nb = in.n_blocks, nf = in.n_frames, nc = in.nc, ngp = P.n_gn_points;
  const int* ph = in.point_host_h;
  const std::vector<int>&pfirst = P.pt_first, &pnblk = P.pt_nblk, &phost = P.pt_host, &gtgt = P.gn_target;
  const int nu = nf + nc;
  std::vector<std::vector<int>> bl((size_t)nc * nu), pl((size_t)nc * nu), pk((size_t)nc * nu);
  const bool walk = in.test_pblk_walk;  // (tests: every target entry walks its point's blocks)
  std::vector<int>& bcam = P.ib_cam;
  bcam.resize(nb);
  P.ib_rec.resize(nb);
  std::vector<char> cam_seen(nc, 0);
  for (int gb = 0; gb < nb; ++gb) {
    const int b = W.order[gb], pt = in.block_point_h[b], h = ph[pt], t = in.block_target_h[b], c = in.frame_cam_h[t];
    bcam[gb] = c;
    P.ib_rec[gb] = PlanInt4{b, pt, h, t};
    cam_seen[c] = 1;
    bl[(size_t)c * nu + h].push_back((int)((unsigned)gb | 0x80000000u));  // (bit 31: the unit hosts the block)
    bl[(size_t)c * nu + t].push_back(gb);
    bl[(size_t)c * nu + nf + c].push_back(gb);
  }
  for (int q = 0; q < ngp; ++q) {
    std::vector<int> cams, units{phost[q]};
    for (int gb = pfirst[q]; gb < pfirst[q] + pnblk[q]; ++gb) {
      if (std::find(cams.begin(), cams.end(), bcam[gb]) == cams.end()) cams.push_back(bcam[gb]);
      if (std::find(units.begin(), units.end(), gtgt[gb]) == units.end()) units.push_back(gtgt[gb]);
    }
    for (int c : cams) units.push_back(nf + c);
    for (int c : cams)
      for (int u : units) {
        pl[(size_t)c * nu + u].push_back(q);
        // the border kernel's Schur term for keyframe u: −1 u hosts the point, else its one block targeting u
        int by = -1;
        if (u < nf && u != phost[q]) {
          int n_u = 0;
          for (int gb = pfirst[q]; gb < pfirst[q] + pnblk[q]; ++gb)
            if (gtgt[gb] == u) {
              by = gb;
              ++n_u;
            }
          if (n_u != 1 || walk) by = -2;
        }
        pk[(size_t)c * nu + u].push_back(by);
      }
  }
  std::vector<int>&bp = P.ib_bptr, &bflat = P.ib_blist, &pp = P.ib_pptr, &pflat = P.ib_plist, &pkflat = P.ib_pblk;
  bp.assign(1, 0);
  pp.assign(1, 0);
  for (size_t L = 0; L < bl.size(); ++L) {
    bflat.insert(bflat.end(), bl[L].begin(), bl[L].end());
    bp.push_back((int)bflat.size());
    pflat.insert(pflat.end(), pl[L].begin(), pl[L].end());
    pkflat.insert(pkflat.end(), pk[L].begin(), pk[L].end());
    pp.push_back((int)pflat.size());
  }
  if (bflat.empty()) bflat.push_back(0);
  if (pflat.empty()) pflat.push_back(0);
  if (pkflat.empty()) pkflat.push_back(-1);
  for (int c = 0; c < nc; ++c) P.fixed[nf + 2 * c] = P.fixed[nf + 2 * c + 1] = !cam_seen[c];
}

// point-aligned waves for intr_rows_kernel (whole points of ≤ 64 blocks each; a longer point: consecutive waves and
// the separate point sums of intr_pw_kernel — ir_waves = 0, no table)
void wave_table(const GnPlanInput& in, GnPlan& P) {
  const int nb = in.n_blocks, ngp = P.n_gn_points;
  const std::vector<int>&pfirst = P.pt_first, &pnblk = P.pt_nblk;
  std::vector<PlanInt4>& wt = P.ir_wave;
  bool fits = true;
  for (int q = 0; q < ngp && fits; ++q) {
    if (pnblk[q] > 64) fits = false;
    else if (wt.empty() || wt.back().y + pnblk[q] > 64) wt.push_back(PlanInt4{pfirst[q], pnblk[q], q, 0});
    else wt.back().y += pnblk[q];
  }
  // (the GN points cover the GN blocks in order: pfirst[q + 1] = pfirst[q] + pnblk[q], checked here)
  for (int q = 0; q + 1 < ngp && fits; ++q) fits = pfirst[q + 1] == pfirst[q] + pnblk[q];
  fits = fits && ngp > 0 && pfirst[0] == 0 && pfirst[ngp - 1] + pnblk[ngp - 1] == nb;
  if (in.test_row_waves64) fits = false;  // (tests: the 64-block waves + intr_pw_kernel path)
  P.ir_waves = fits ? (int)wt.size() : 0;
  if (!fits) wt.clear();
}

}  // namespace

void profile_columns(const std::vector<int>& first, std::vector<int>& ccptr, std::vector<int>& ccrows) {
  const int n = (int)first.size();
  std::vector<std::vector<int>> col(n);
  for (int i = 0; i < n; ++i)
    for (int k = first[i]; k < i; ++k) col[k].push_back(i);
  ccptr.assign(n + 1, 0);
  ccrows.clear();
  for (int k = 0; k < n; ++k) {
    ccptr[k + 1] = ccptr[k] + (int)col[k].size();
    ccrows.insert(ccrows.end(), col[k].begin(), col[k].end());
  }
  if (ccrows.empty()) ccrows.push_back(0);
}

void skyline_profile(const std::vector<int>& first, std::vector<int>& rowp, std::vector<int>& last,
                     std::vector<int>& ccptr, std::vector<int>& ccrows) {
  const int n = (int)first.size();
  rowp.assign(n + 1, 0);
  for (int i = 0; i < n; ++i) rowp[i + 1] = rowp[i] + (i - first[i] + 1);
  last.resize(n);
  for (int k = 0; k < n; ++k) last[k] = k;
  for (int i = 0; i < n; ++i)
    for (int k = first[i]; k < i; ++k) last[k] = std::max(last[k], i);
  profile_columns(first, ccptr, ccrows);
}

int build_gn_plan(const GnPlanInput& in, GnPlan& P) {
  P = GnPlan{};
  Work W;
  order_blocks(in, W, P);
  linearise_chunks(in, W, P);
  gn_points(in, W, P);
  if (int rc = schur_chunks(in, W, P)) return rc;
  reduced_system(in, W, P);
  if (in.nc) {
    border_lists(in, W, P);
    wave_table(in, P);
  }
  if (in.n_pairs >= (1 << 24)) return fail(PBA_ERR_INVALID_ARGUMENT, "more than 2^24 (host, target) pairs");
  return PBA_OK;
}

}  // namespace detail
}  // namespace pba
