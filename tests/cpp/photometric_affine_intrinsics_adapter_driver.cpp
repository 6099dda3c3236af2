// Drives include/pba_ceres.h's photometric cost with a free target-intrinsics block and affine brightness blocks,
// GpuPhotometricAffineIntrinsicsCost<8> = SizedCostFunction<8, 7, 7, 1, 8, 2, 2>, the way Ceres' ProgramEvaluator/
// ResidualBlock would (program_evaluator.h:157-237, residual_block.cc:69-158): a GpuEvaluator that was given the cameras'
// intrinsics blocks and one (a, b) block per keyframe, PrepareForEvaluation, then per block CostFunction::Evaluate with
// the parameter pointers (T_w_host, T_w_target, ρ, intr_target, ab_host, ab_target), then J_local = J_global ·
// LocalParameterization::ComputeJacobian for the two poses.
//   usage: photometric_affine_intrinsics_adapter_driver <problem.bin> <intrinsics.bin> <affine.bin> <out.bin>
//   problem layout: tests/golden/make_golden.py (photometric, P = 8); intrinsics.bin: 8·n_cams doubles, the intrinsics
//   blocks' values; affine.bin: 2·n_frames doubles, the (a, b) blocks' values.
//   out.bin: f64 records[n_blocks·26·8] ([r | J_host | J_target | J_rho | J_intr | J_ab_host | J_ab_target], tangent pose
//            Jacobians), u8 valid[n_blocks],
//            f64 records[n_blocks·14·8] of a second pass with jacobians[3] == [4] == [5] == nullptr, u8 valid[n_blocks],
//            i32 {an evaluator with the (a, b) blocks only: Evaluate with jacobians[3] returned false and
//                 refused_intrinsics() (and not refused_affine()),
//                 an evaluator with the intrinsics blocks only: Evaluate with jacobians[5] returned false and
//                 refused_affine() (and not refused_intrinsics()),
//                 an evaluator with neither: Evaluate with jacobians[3..5] == nullptr returned true for a valid block,
//                 nothing refused}
#include <array>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "pba_ceres.h"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}

constexpr int P = 8;
using Cost = pba_ceres::GpuPhotometricAffineIntrinsicsCost<P>;

int main(int argc, char** argv) {
  if (argc < 5) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto hdr = rd<int32_t>(f, 9);
  const int kind = hdr[0], model = hdr[1], nf = hdr[2], np = hdr[3], nb = hdr[4], nc = hdr[5], W = hdr[6], H = hdr[7];
  if (kind != 0 || hdr[8] != P) { fprintf(stderr, "driver is built for photometric problems with P = 8\n"); return 3; }
  const auto intr = rd<double>(f, 8 * nc);
  const auto frame_cam = rd<int32_t>(f, nf);
  const auto images = rd<uint8_t>(f, (size_t)nf * W * H);
  const auto pattern = rd<float>(f, 2 * P);
  const auto point_host = rd<int32_t>(f, np);
  const auto u_ref = rd<double>(f, 2 * np);
  const auto host_int = rd<float>(f, (size_t)P * np);
  const auto block_point = rd<int32_t>(f, nb);
  const auto block_target = rd<int32_t>(f, nb);
  auto poses_flat = rd<double>(f, 7 * nf);
  auto rho = rd<double>(f, np);
  fclose(f);
  f = fopen(argv[2], "rb");
  if (!f) return 2;
  auto kstate = rd<double>(f, 8 * nc);  // the intrinsics blocks, user memory Ceres would optimise in place
  fclose(f);
  f = fopen(argv[3], "rb");
  if (!f) return 2;
  auto state = rd<double>(f, 2 * nf);  // the (a, b) blocks
  fclose(f);

  auto make_engine = [&]() {
    pba_options opt{0, kind, model, 0.0f};
    pba_engine* e = nullptr;
    pba_ceres::check(pba_create(&opt, &e), "pba_create");
    pba_ceres::check(pba_set_cameras(e, nc, intr.data()), "cameras");
    pba_ceres::check(pba_set_frames(e, nf, frame_cam.data(), W, H, images.data()), "frames");
    pba_ceres::check(pba_set_pattern(e, P, pattern.data()), "pattern");
    pba_ceres::check(pba_set_points(e, np, point_host.data(), u_ref.data(), host_int.data()), "points");
    pba_ceres::check(pba_set_blocks(e, nb, block_point.data(), block_target.data(), nullptr), "blocks");
    return e;
  };
  std::vector<std::array<double, 7>> T(nf);
  for (int i = 0; i < nf; ++i)
    for (int q = 0; q < 7; ++q) T[i][q] = poses_flat[7 * i + q];
  std::vector<double*> pose_ptr(nf), rho_ptr(np), k_ptr(nc), ab_ptr(nf);
  for (int i = 0; i < nf; ++i) pose_ptr[i] = T[i].data();
  for (int p = 0; p < np; ++p) rho_ptr[p] = &rho[p];
  for (int c = 0; c < nc; ++c) k_ptr[c] = &kstate[8 * c];
  for (int i = 0; i < nf; ++i) ab_ptr[i] = &state[2 * i];
  std::vector<double> Pf(42 * (size_t)nf);
  for (int i = 0; i < nf; ++i) pba_ceres::se3_plus_jacobian(T[i].data(), &Pf[42 * i]);
  auto params_of = [&](int b, const double** params) {
    const int p = block_point[b], h = point_host[p], t = block_target[b];
    params[0] = T[h].data(); params[1] = T[t].data(); params[2] = &rho[p];
    params[3] = k_ptr[frame_cam[t]]; params[4] = ab_ptr[h]; params[5] = ab_ptr[t];
  };

  pba_engine* e = make_engine();
  std::vector<double> out26((size_t)nb * 26 * P, 0.0), out14((size_t)nb * 14 * P, 0.0);
  std::vector<uint8_t> valid26(nb, 0), valid14(nb, 0);
  {
    pba_ceres::GpuEvaluator ev(e, pose_ptr, rho_ptr, k_ptr, pba_ceres::PoseJacobian::kReferenceSE3, ab_ptr);
    if (pba_record_floats(e) != 26 * P || pba_record_bytes(e) != 104 * P) return 6;
    std::vector<std::unique_ptr<ceres::CostFunction>> cfs;
    for (int b = 0; b < nb; ++b) cfs.emplace_back(new Cost(&ev, b, point_host[block_point[b]], block_target[b]));
    if (cfs[0]->num_residuals() != P || cfs[0]->parameter_block_sizes() != std::vector<int32_t>{7, 7, 1, 8, 2, 2}) return 4;
    ev.PrepareForEvaluation(true, true);
    std::vector<double> J0(P * 7), J1(P * 7), J2(P), J3(P * 8), J4(P * 2), J5(P * 2), r(P);
    for (int pass = 0; pass < 2; ++pass) {  // 0: all six Jacobians; 1: the three new blocks constant (null Jacobians)
      const int rec = pass == 0 ? 26 * P : 14 * P;
      std::vector<double>& out = pass == 0 ? out26 : out14;
      for (int b = 0; b < nb; ++b) {
        const int h = point_host[block_point[b]], t = block_target[b];
        const double* params[6];
        params_of(b, params);
        double* jac[6] = {J0.data(), J1.data(), J2.data(), pass == 0 ? J3.data() : nullptr,
                          pass == 0 ? J4.data() : nullptr, pass == 0 ? J5.data() : nullptr};
        if (!cfs[b]->Evaluate(params, r.data(), jac)) continue;
        (pass == 0 ? valid26 : valid14)[b] = 1;
        double* o = &out[(size_t)b * rec];
        const double* Ph = &Pf[42 * h];
        const double* Pt = &Pf[42 * t];
        for (int k = 0; k < P; ++k) {
          o[k] = r[k];
          for (int c = 0; c < 6; ++c) {  // J_local = J_global · P   (residual_block.cc:136-158)
            double sh = 0, st = 0;
            for (int g = 0; g < 7; ++g) {
              sh += J0[k * 7 + g] * Ph[g * 6 + c];
              st += J1[k * 7 + g] * Pt[g * 6 + c];
            }
            o[P + 6 * k + c] = sh;
            o[7 * P + 6 * k + c] = st;
          }
          o[13 * P + k] = J2[k];
          if (pass == 0) {
            for (int c = 0; c < 8; ++c) o[14 * P + 8 * k + c] = J3[8 * k + c];
            for (int c = 0; c < 2; ++c) {
              o[22 * P + 2 * k + c] = J4[2 * k + c];
              o[24 * P + 2 * k + c] = J5[2 * k + c];
            }
          }
        }
      }
    }
  }
  pba_destroy(e);

  // evaluators that were not given the matching blocks refuse a Jacobian request for one of them, and only that
  int32_t flags[3] = {0, 0, 0};
  int b = 0;
  while (b < nb && !valid26[b]) ++b;
  if (b == nb) return 5;
  const double* params[6];
  params_of(b, params);
  std::vector<double> J0(P * 7), J1(P * 7), J2(P), J3(P * 8), J5(P * 2), r(P);
  for (int which = 0; which < 3; ++which) {
    e = make_engine();
    {
      pba_ceres::GpuEvaluator ev(e, pose_ptr, rho_ptr, which == 1 ? k_ptr : std::vector<double*>{},
                                 pba_ceres::PoseJacobian::kReferenceSE3, which == 0 ? ab_ptr : std::vector<double*>{});
      ev.PrepareForEvaluation(true, true);
      Cost cf(&ev, b, point_host[block_point[b]], block_target[b]);
      if (which == 0) {
        double* jac[6] = {J0.data(), J1.data(), J2.data(), J3.data(), nullptr, nullptr};
        flags[0] = !cf.Evaluate(params, r.data(), jac) && ev.refused_intrinsics() && !ev.refused_affine();
      } else if (which == 1) {
        double* jac[6] = {J0.data(), J1.data(), J2.data(), nullptr, nullptr, J5.data()};
        flags[1] = !cf.Evaluate(params, r.data(), jac) && ev.refused_affine() && !ev.refused_intrinsics();
      } else {
        double* jac[6] = {J0.data(), J1.data(), J2.data(), nullptr, nullptr, nullptr};
        flags[2] = cf.Evaluate(params, r.data(), jac) && !ev.refused_affine() && !ev.refused_intrinsics();
      }
    }
    pba_destroy(e);
  }

  FILE* g = fopen(argv[4], "wb");
  if (!g) return 2;
  fwrite(out26.data(), sizeof(double), out26.size(), g);
  fwrite(valid26.data(), 1, valid26.size(), g);
  fwrite(out14.data(), sizeof(double), out14.size(), g);
  fwrite(valid14.data(), 1, valid14.size(), g);
  fwrite(flags, sizeof(int32_t), 3, g);
  fclose(g);
  return 0;
}
