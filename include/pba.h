/* include/pba.h — C ABI of the MI355X photometric bundle-adjustment residual/Jacobian engine.
 *
 * This is the drop-in boundary for the reference's hot path.  In the reference every residual block is
 * a separate Ceres AutoDiffCostFunction evaluated on CPU threads:
 *
 *   map_utils.h:347-375      problem build: one AutoDiffCostFunction<Functor,2,7,7,1,8> + HuberLoss per
 *                            (landmark, non-anchor observation); parameters (T_w_host, T_w_target, ρ, intr)
 *   reprojection.h:83-112    BundleAdjustmentReprojectionCostFunctor::operator()  (geometric residual)
 *   photometric_error.h:139-182  PhotometricError<8>::operator()                 (photometric residual)
 *   program_evaluator.h:139-258  ProgramEvaluator::Evaluate — the per-block ParallelFor this replaces
 *   residual_block.cc:69-198     ResidualBlock::Evaluate   — J_local = J_global · P(7×6)
 *   evaluation_callback.h:63-76  EvaluationCallback::PrepareForEvaluation — where pba_evaluate is called
 *
 * One engine evaluates ALL blocks of a problem in one launch on one GPU.  Conventions:
 *   pose        Sophus SE3d storage [qx qy qz qw tx ty tz], camera-to-world T_w_c (common_types.h:174-179)
 *   tangent     δ = [υ(3), ω(3)], right update T·exp(δ)  (local_parameterization_se3.hpp:43-50)
 *   point       anchored at its host keyframe; inverse DISTANCE ρ along the unit bearing of u_ref
 *               (common_types.h:205-217; reprojection.h:105-108)
 *   intrinsics  8-vector [fx fy cx cy p1 p2 p3 p4] (camera_models.h:50); model shared by all cameras,
 *               host camera model used for the target too (reprojection.h:99-100)
 *   block       (point, target keyframe); host = the point's host keyframe
 *   residuals   geometric: r = u_obs − π_t(T_w_t⁻¹ T_w_h b/ρ)                    (R = 2)
 *               photometric: r_k = I_t(π_t(R_th b_k + ρ t_th)) − I_h,k, k < P      (R = P)
 *               bilinear (default) or Ceres' bicubic interpolation of the u8 target image (pba_set_interpolator),
 *               Grid2D edge clamp
 *   record      per block, R×14 floats: [ r(R) | J_host(R×6) | J_target(R×6) | J_rho(R) ], row-major,
 *               tangent-space (= Ceres' J_global·P of residual_block.cc:136-158), NOT robustified
 *               (the loss stays with the caller, residual_block.cc:161-196).
 *   valid       per block 1/0; 0 when a projection leaves the camera's domain or a value is non-finite;
 *               the record is then all zeros (a Ceres adapter returns false for such a block,
 *               matching residual_block.cc:113-131).
 *
 * Memory: every pointer argument is a HOST pointer unless the function name ends in _device.  The engine
 * owns its device buffers; the caller owns its host buffers.  One engine per GPU; calls on one engine
 * must be serialised by the caller (thread-compatible, not thread-safe).  All functions return PBA_OK
 * (0) or a negative status; pba_last_error() describes the most recent failure of the calling thread.
 */
#ifndef PBA_H_
#define PBA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBA_OK 0
#define PBA_ERR_INVALID_ARGUMENT (-1)
#define PBA_ERR_DEVICE (-2)          /* HIP runtime error (no device, launch failure, …) */
#define PBA_ERR_OUT_OF_MEMORY (-3)
#define PBA_ERR_NOT_READY (-4)       /* a set_* call required by this call has not been made */

#define PBA_RESIDUAL_PHOTOMETRIC 0
#define PBA_RESIDUAL_GEOMETRIC 1

#define PBA_CAMERA_PINHOLE 0        /* camera_models.h:48-114  */
#define PBA_CAMERA_DOUBLE_SPHERE 1  /* camera_models.h:198-284 */
#define PBA_CAMERA_EUCM 2           /* camera_models.h:116-196 */
#define PBA_CAMERA_KB4 3            /* camera_models.h:286-421 (Kannala-Brandt, 4 distortion terms) */

#define PBA_MAX_PATTERN 32

typedef struct pba_engine pba_engine;

typedef struct pba_options {
  int32_t device;         /* HIP device ordinal */
  int32_t residual_kind;  /* PBA_RESIDUAL_* */
  int32_t camera_model;   /* PBA_CAMERA_* */
  float huber_width;      /* a of HuberLoss(a) for the per-block cost (loss_function.cc:48-62); <= 0: squared */
} pba_options;

/* Lifecycle ------------------------------------------------------------------------------------- */
int pba_create(const pba_options* options, pba_engine** out_engine);
int pba_destroy(pba_engine* engine);
const char* pba_status_string(int status);
const char* pba_last_error(void);
int pba_version(void);  /* 100·major + minor */

/* Problem description (BundleAdjustment problem build, map_utils.h:322-375) ---------------------- */
/* intrinsics: 8·n_cams doubles */
int pba_set_cameras(pba_engine* engine, int32_t n_cams, const double* intrinsics);
/* frame_cam[n_frames]: camera index of every keyframe; images: n_frames·height·width u8, row-major,
 * required for photometric engines (may be NULL for geometric ones). */
int pba_set_frames(pba_engine* engine, int32_t n_frames, const int32_t* frame_cam, int32_t width,
                   int32_t height, const uint8_t* images);
/* same, with the images already in device memory (copied device-to-device on the engine stream) */
int pba_set_frames_device(pba_engine* engine, int32_t n_frames, const int32_t* frame_cam, int32_t width,
                          int32_t height, const uint8_t* d_images);
/* residual pattern: P (du, dv) pairs, P <= PBA_MAX_PATTERN (photometric only) */
int pba_set_pattern(pba_engine* engine, int32_t P, const float* offsets);
/* points: host keyframe, u_ref (2 doubles, pixel in the host image), host_intensity (P floats,
 * photometric only — the I_h,k of photometric_error.h:179; NULL: sampled on the device from the host keyframe's
 * image at u_ref + pattern offset, with the engine's interpolator; a later pba_set_interpolator samples them again). */
int pba_set_points(pba_engine* engine, int32_t n_points, const int32_t* host_frame, const double* u_ref,
                   const float* host_intensity);
/* blocks: point index and target keyframe per block; u_obs (2 doubles per block) for geometric engines.
 * target != host(point) is required. */
int pba_set_blocks(pba_engine* engine, int32_t n_blocks, const int32_t* block_point,
                   const int32_t* block_target, const double* u_obs);

/* Evaluation (EvaluationCallback::PrepareForEvaluation → one launch) ----------------------------- */
/* poses: 7·n_frames doubles; inv_dist: n_points doubles (host memory; copied to the device) */
int pba_set_state(pba_engine* engine, const double* poses, const double* inv_dist);
int pba_set_state_device(pba_engine* engine, const double* d_poses, const double* d_inv_dist);
/* Enqueue the evaluation of every block on the engine's stream.  want_jacobians = 0 writes only the
 * residual part of each record (Ceres' residual-only evaluation, trust_region_minimizer.cc:761-779). */
int pba_evaluate(pba_engine* engine, int32_t want_jacobians);
/* Evaluate at a device-resident state and adopt it (afterwards it is the engine's state, as after
 * pba_set_state_device): Ceres' Evaluator::Evaluate(state, …) (program_evaluator.h:139-258), which reads the
 * parameter state straight from the caller's array.  Photometric engines do it in ONE launch — each block forms
 * its relative pose from the poses in its prologue and the launch copies the state — so no pair-table or copy
 * launch precedes the evaluation.  d_poses / d_inv_dist must stay valid until the launch has run. */
int pba_evaluate_state_device(pba_engine* engine, const double* d_poses, const double* d_inv_dist,
                              int32_t want_jacobians);
/* n evaluations back to back — state i = (d_poses[i], d_inv_dist[i]), each as pba_evaluate_state_device (one launch
 * that adopts it), enqueued by one call: a caller stepping through candidate states (a line search, a benchmark's
 * steps) pays the host-side launch cost in C instead of per foreign-function call.  Replaces n calls of
 * Evaluator::Evaluate (program_evaluator.h:139-258); the records hold the last state's evaluation. */
int pba_evaluate_states_device(pba_engine* engine, int32_t n, const double* const* d_poses,
                               const double* const* d_inv_dist, int32_t want_jacobians);
int pba_synchronize(pba_engine* engine);

/* Results ---------------------------------------------------------------------------------------- */
/* values per record as pba_get_records returns them: 14·R, or — with pba_set_optimize_intrinsics, on geometric and
 * photometric engines alike — 22·R: [ r(R) | J_host(R×6) | J_target(R×6) | J_rho(R) | J_intr(R×8) ], or — with
 * pba_set_affine_brightness — 18·R: [ … | J_rho(R) | J_ab_host(R×2) | J_ab_target(R×2) ], or — with both, which
 * pba_set_intrinsics_with_affine allows — 26·R: [ … | J_rho(R) | J_intr(R×8) | J_ab_host(R×2) | J_ab_target(R×2) ] */
int pba_record_floats(const pba_engine* engine);
/* Record storage format (photometric engines): PBA_RECORD_F32 (default) or PBA_RECORD_F16 — IEEE half records,
 * half the HBM write traffic (config C5's "fp16 residuals"; evaluation stays fp64 warp + fp32 chain, rounding
 * only at the store: ≤ 2⁻¹¹ relative per value; values beyond the half range saturate at ±65504 — at full
 * resolution a strong edge's rotation Jacobian can exceed it; the on-device GN path never reads records, it
 * accumulates JᵀJ from fp32 rows).  pba_get_records returns floats either way;
 * pba_device_records' pointer then addresses 14·R halves per block.
 * PBA_RECORD_F16_SCALED — half records that keep the Jacobians PBA_RECORD_F16 clamps: 15·R halves per block,
 *   [ r(R) | J_host(R×6) | J_target(R×6) | J_rho(R) | e(R) ]
 * the first 14·R laid out as PBA_RECORD_F16, then one scale per pixel row k (a row = the 13 Jacobian values of pattern
 * pixel k: 6 + 6 + 1); the true value of a Jacobian entry of row k is stored · e[k].  e[k] is a power of two stored as a
 * half: with m the largest magnitude of the row's 13 fp32 values, e = 1 when m < 65520 (every value rounds to a finite
 * half; the row is stored exactly as PBA_RECORD_F16 stores it), else e = 2^(⌊log₂ m⌋ − 14), at most 2¹⁵ — the scaled
 * row maximum then lies in [16384, 32768).  Scaling by 1/e is exact, so the one rounding is the half conversion:
 * ≤ 2⁻¹¹ relative per value (absolute 2⁻²⁴·e where the scaled value is a subnormal half).  Range: values beyond
 * 65504·2¹⁵ ≈ 2.1e9 saturate at that bound.  Residuals are stored unscaled (|r| ≤ 255 for 8-bit images).  An invalid
 * block stores 15·R zero halves; a residual-only evaluation writes only r, at the 15·R stride.  The format serves the
 * same consumers as PBA_RECORD_F16 (AutoDiffCostFunction's Jacobian blocks of photometric_error.h:139-182 as read by
 * ResidualBlock::Evaluate, residual_block.cc:69-158) at 30 instead of 28 bytes per row, 56 for fp32.  pba_get_records
 * decodes on the host ((float)half · (float)e, exact), pba_decode_records_device on the device. */
#define PBA_RECORD_F32 0
#define PBA_RECORD_F16 1
#define PBA_RECORD_F16_SCALED 2
int pba_set_record_format(pba_engine* engine, int32_t format);
int pba_record_format(const pba_engine* engine);
/* device bytes per record as stored: 4·pba_record_floats (PBA_RECORD_F32), 28·R (PBA_RECORD_F16) or 30·R
 * (PBA_RECORD_F16_SCALED).  pba_record_floats stays 14·R in the half formats: it describes what pba_get_records returns.
 * With pba_set_optimize_intrinsics the records are fp32 only: 88·R bytes; with pba_set_affine_brightness 72·R; with
 * both (pba_set_intrinsics_with_affine) 104·R. */
int pba_record_bytes(const pba_engine* engine);
/* Target-intrinsics Jacobian (geometric and photometric engines; BundleAdjustmentOptions::optimize_intrinsics,
 * map_utils.h:339-345):
 * the reference functor takes the TARGET camera's intrinsics as its 4th parameter block (sIntr_c2, reprojection.h:83-86,
 * :108) and unprojects the host pixel with the intrinsics captured at problem build (ref_intrinsics, :93-98; Ceres never
 * writes user memory during a solve without an evaluation callback, so those stay at their initial values).  Enabled,
 * every projection uses the intrinsics state (pba_set_intrinsics_state, 8·n_cams doubles; initially the cameras'),
 * host unprojection keeps the pba_set_cameras values, and each record grows by J_intr (R×8, row-major) after J_rho:
 * 22·R values.
 * Photometric engines: the bearing b_k and a device-sampled I_h,k keep the cameras' values; the domain test, π in
 * r_k = I_t(π_state(p̃_k)) − I_h,k and the chain ∇I·∂π/∂p̃ of J_host, J_target and J_rho use the state of the TARGET
 * keyframe's camera; row k of J_intr is [∂I/∂u ∂I/∂v]·∂π/∂k (2×8) at p̃_k (no minus sign, unlike the geometric
 * r = u_obs − π), with exact zeros in the columns of parameters the model does not use.  An invalid block stores 22·R
 * zeros, a residual-only evaluation writes r at the 22·R stride.  At pyramid level l the target projects with the
 * level-l image of the state (fx/2^l, fy/2^l, (c + 0.5)/2^l − 0.5, distortion unchanged) while J_intr stays the
 * derivative with respect to the level-0 state — the block a caller such as Ceres holds — so its columns 0-3 carry the
 * factor 2^−l; pba_set_intrinsics_state and pba_get_intrinsics speak of the level-0 state at every level.  The records
 * are fp32 only: with free intrinsics pba_set_record_format refuses the half formats, and with a half format active
 * this call refuses (PBA_ERR_INVALID_ARGUMENT either way; J_intr's distortion columns reach ~2.5e4 and a 21-value row
 * scale is a design of its own).  By default the on-device Gauss-Newton does not take photometric free intrinsics:
 * every pba_gn_* entry point, pba_solve, pba_solve_pyramid and pba_solve_distributed(_comm) returns
 * PBA_ERR_INVALID_ARGUMENT instead of solving with the intrinsics held fixed, and the consumer is an outer solver over
 * the records (include/pba_ceres.h, GpuPhotometricIntrinsicsCost).  pba_gn_set_solve_intrinsics (below) opts the
 * single-GPU entry points in: the state's 8 intrinsics per camera then join the reduced camera system as on a geometric
 * engine (its border formed from 160-double moment records of the P-row blocks), pba_gn_accept and every
 * solve that accepted a step leave the solved level-0 state in pba_get_intrinsics, and pba_solve_pyramid carries it
 * across the levels.  The multi-GPU entry points (pba_gn_step_export/import, pba_solve_distributed(_comm)) refuse
 * photometric free intrinsics either way.
 * Geometric engines: the on-device Gauss-Newton (pba_gn_*, pba_solve) then optimises the intrinsics too: each camera's 8
 * intrinsics are 12 unknowns of the reduced camera system after the keyframes' (two 6-dim blocks, the last four pads
 * with identity rows), a dense border of the skyline system (SPARSE_SCHUR keeps the intrinsics blocks among the f-blocks,
 * schur_complement_solver.cc:138-146); k ← k + δk, Ceres' LM diagonal over them too.  The multi-GPU entry points
 * exchange the border rows too (pba_gn_exchange_size). */
int pba_set_optimize_intrinsics(pba_engine* engine, int32_t enable);
/* Photometric engines with pba_set_optimize_intrinsics: let the on-device Gauss-Newton (pba_gn_linearize/step/
 * candidate_cost/accept, pba_solve, pba_solve_pyramid) optimise the intrinsics state too — the arrow system of the
 * geometric engines.  Default 0: those entry points refuse as before.  Geometric engines: PBA_OK, no effect (their
 * solve always takes free intrinsics). */
int pba_gn_set_solve_intrinsics(pba_engine* engine, int32_t enable);
int pba_set_intrinsics_state(pba_engine* engine, const double* intrinsics);
/* the intrinsics state (8·n_cams doubles: the free intrinsics with pba_set_optimize_intrinsics, else the cameras') */
int pba_get_intrinsics(pba_engine* engine, double* intrinsics);
/* Affine brightness per keyframe (photometric engines; the transform [a, b] of Engel et al.'s direct sparse odometry
 * that PhotometricError<8> names as left out, photometric_error.h:61-63).  Every keyframe f has two parameters
 * (a_f, b_f), held by the engine as the affine state [a_0 b_0 a_1 b_1 …] of 2·n_frames doubles.  Enabled, with h the
 * block's host keyframe, t its target and E = exp(a_t − a_h),
 *   r_k = (I_t(π(p̃_k)) − b_t) − E·(I_h,k − b_h)                                   k < R
 * and each record grows by four columns per pixel row after J_rho, 18·R values (72·R bytes, fp32 only):
 *   [ r(R) | J_host(R×6) | J_target(R×6) | J_rho(R) | J_ab_host(R×2) | J_ab_target(R×2) ]
 *   row k:  J_ab_host   = [ ∂r/∂a_h, ∂r/∂b_h ] = [ +E·(I_h,k − b_h), +E ]
 *           J_ab_target = [ ∂r/∂a_t, ∂r/∂b_t ] = [ −E·(I_h,k − b_h), −1 ]
 * J_host, J_target and J_rho are unchanged (∇I_t does not depend on (a, b)); the records stay unrobustified and the
 * per-block Huber cost (pba_get_block_costs, pba_get_cost) is taken on the new r.  a_t − a_h and its exponential are
 * formed in fp64 from the state once per block; E, b_h, b_t are floats from there on, and at a = b = 0 the residual is
 * I − I_h bit for bit.  Validity is unchanged (projection domain, finite values): a non-finite a or b of a block's host
 * or target makes the block invalid, its record 18·R zeros; a residual-only evaluation writes r at the 18·R stride.
 * (a, b) are shared by all pyramid levels (the 2×2 mean is linear in intensity: no level factor).  Every read-back
 * path serves the 18·R records (pba_get_records, _raw, _async / pba_wait_records, pba_get_residuals,
 * pba_device_records, pba_decode_records_device).
 * pba_set_affine_brightness: enabling sets the state to zeros, disabling restores the 14·R records.  Refused with
 * PBA_ERR_INVALID_ARGUMENT, the engine left as it was: on a geometric engine; with a half record format active (and
 * pba_set_record_format then refuses the half formats: the brightness columns have no half layout); together with
 * pba_set_optimize_intrinsics, whichever comes second, unless pba_set_intrinsics_with_affine (below) has opted in to
 * the 26-column record.  While it is enabled, and
 * unless pba_gn_set_solve_affine (below) opts in, every on-device Gauss-Newton entry point (pba_gn_*, pba_solve,
 * pba_solve_pyramid, pba_gn_step_export/import, pba_solve_distributed(_comm)) returns PBA_ERR_INVALID_ARGUMENT instead
 * of solving with a = b = 0.  The consumer of the brightness columns is an outer solver over the records
 * (include/pba_ceres.h, GpuPhotometricAffineCost).
 * pba_set_affine_state / _device (host / device memory) and pba_get_affine_state move the 2·n_frames doubles;
 * PBA_ERR_NOT_READY before pba_set_frames or without pba_set_affine_brightness.  pba_set_frames* resets the state to
 * zeros.  pba_evaluate_state(s)_device keep taking poses and inverse distances only: the affine state is the engine's,
 * as the intrinsics state is. */
int pba_set_affine_brightness(pba_engine* engine, int32_t enable);
int pba_set_affine_state(pba_engine* engine, const double* ab);
int pba_set_affine_state_device(pba_engine* engine, const double* d_ab);
int pba_get_affine_state(pba_engine* engine, double* ab);
/* Free intrinsics together with affine brightness (photometric engines): the records of the full photometric problem —
 * poses, inverse distances, intrinsics (BundleAdjustmentOptions::optimize_intrinsics, map_utils.h:339-345) and (a, b) —
 * for an outer solver (include/pba_ceres.h, GpuPhotometricAffineIntrinsicsCost).
 * Default 0: pba_set_optimize_intrinsics and pba_set_affine_brightness refuse each other as described above.  With
 * enable = 1 each accepts the other, in either order; the switch alone changes no record, size or evaluation.  With
 * both on, pba_record_floats = 26·R and pba_record_bytes = 104·R (fp32 only):
 *   [ r(R) | J_host(R×6) | J_target(R×6) | J_rho(R) | J_intr(R×8) | J_ab_host(R×2) | J_ab_target(R×2) ]
 *   r_k = (I_t(π_state(p̃_k)) − b_t) − E·(I_h,k − b_h): the target projects with the intrinsics state, the host
 *   unprojects with the cameras' values, E = exp(a_t − a_h) in fp64 once per block;
 *   J_intr row k = ∇I_t·∂π/∂k, exact zeros for parameters the model does not use (∇I_t does not depend on (a, b));
 *   J_ab_host row k = [ E·(I_h,k − b_h), E ],  J_ab_target row k = [ −E·(I_h,k − b_h), −1 ].
 * Turning one of the two off gives the other's 22·R or 18·R record back.  Everything else is as with one switch:
 * validity (and a non-finite a, pose or intrinsics-state value — one that leaves π not finite — makes the blocks it
 * touches invalid), 26·R zeros for an invalid block, the per-block Huber cost on the new r, a residual-only evaluation writing
 * r at the 26·R stride, pba_set_frames* zeroing (a, b), the intrinsics state starting at the cameras' values, J_intr
 * with respect to the level-0 state at every pyramid level and no level factor on (a, b); every read-back path serves
 * the 26·R records (pba_get_records, _raw, _async / pba_wait_records, pba_get_residuals, pba_device_records,
 * pba_decode_records_device), and pba_set_record_format keeps refusing the half formats while either switch is on.
 * With both on, every on-device solve entry point returns PBA_ERR_INVALID_ARGUMENT and changes nothing, whatever
 * pba_gn_set_solve_intrinsics and pba_gn_set_solve_affine say: pba_gn_*, pba_solve, pba_solve_pyramid,
 * pba_gn_step_export/import, pba_solve_distributed(_comm), pba_affine_*, pba_solve_affine, pba_joint_*,
 * pba_solve_joint, pba_joint_step_export/import and pba_solve_joint_distributed.  One solve runs the full problem:
 * under pba_joint_set_solve_intrinsics (below) pba_joint_linearize / step / get_reduced_system / get_step /
 * get_intrinsics_step / candidate_cost / accept and pba_solve_joint free the intrinsics too.  With or without that
 * switch the rest keeps refusing: pba_joint_band / exchange_size / step_export / step_import,
 * pba_solve_joint_distributed, pba_gn_*, pba_solve, pba_solve_pyramid, the multi-GPU Gauss-Newton, pba_affine_* and
 * pba_solve_affine.
 * PBA_ERR_INVALID_ARGUMENT, the engine left as it was: on a geometric engine; for enable = 1 with a half record format
 * active; for enable = 0 while both switches are on (turn one off first). */
int pba_set_intrinsics_with_affine(pba_engine* engine, int32_t enable);
/* Photometric engines with pba_set_affine_brightness: enable = 1 makes the single-GPU on-device solve
 * (pba_gn_linearize/step/candidate_cost/accept, pba_gn_get_reduced_system/get_step, pba_solve, pba_solve_pyramid) run
 * with the residual above at the engine's affine state, which those calls hold constant — Ceres'
 * SetParameterBlockConstant on the (a, b) blocks (problem.h:306): poses and inverse distances are solved, the state
 * is left bit for bit as it was.  ∇I_t does not depend on (a, b), so J_host, J_target and J_rho are the plain solve's
 * and at the zero state every result is the plain engine's bit for bit.  (a, b) are shared by the pyramid levels.
 * A linearisation or candidate formed before pba_set_affine_state* is stale afterwards, as after pba_set_state.
 * Default 0: those entry points refuse as before.  PBA_ERR_INVALID_ARGUMENT, nothing changed, on an engine without
 * pba_set_affine_brightness; disabling affine brightness clears the switch.  The multi-GPU entry points
 * (pba_gn_step_export/import, pba_solve_distributed(_comm)) refuse either way. */
int pba_gn_set_solve_affine(pba_engine* engine, int32_t enable);
/* The brightness solve at fixed poses and inverse distances (photometric engines with pba_set_affine_brightness; no
 * opt-in: the entry points are new).  Exactly a Ceres solve of the (a, b) blocks with the pose and inverse-distance
 * blocks constant (Problem::SetParameterBlockConstant, problem.h:306), with the pose solve's rules: per-block Huber
 * through the Corrector (corrector.cc:42-110, ρ'' ≤ 0: J̃ = √ρ' J, r̃ = √ρ' r), cost Σ ½ρ(‖r‖²), damping
 * (H + λ·clamp(diag H, 1e-6, 1e32)) δ = −g (levenberg_marquardt_strategy.cc), model decrease ½(λ δᵀDδ − gᵀδ), identity
 * rows for the keyframes of pba_set_fixed_affine_frames (default none) and for keyframes without a valid block (δ = 0
 * there).  The system is 2·n_frames square, unknowns [a_0 b_0 a_1 b_1 …]; every sum is fp64 in a fixed order, so results
 * are bitwise reproducible.  pba_affine_get_system: the undamped system dense (row-major) and g, constant rows as
 * identity / zero — testing and inspection.  pba_affine_step: solver_status ≠ 0 and no candidate when the damped system
 * is not positive definite.  pba_affine_accept: affine state ← candidate.  pba_solve_affine: Ceres' trust-region loop
 * (trust_region_minimizer.cc:67-136) driven from the host, norms over the free (a, b); fills the summary (the device
 * phase times stay 0) and the trajectory pba_solver_iterations serves.  Alternated with pba_solve under
 * pba_gn_set_solve_affine the two give a photometric BA with brightness on the device.
 * PBA_ERR_INVALID_ARGUMENT on a geometric engine or without pba_set_affine_brightness, and for a fixed keyframe out of
 * range (nothing changed); PBA_ERR_NOT_READY for a call before the one it follows (step before linearize, …). */
int pba_set_fixed_affine_frames(pba_engine* engine, int32_t n, const int32_t* frames);
int pba_affine_linearize(pba_engine* engine, double* cost);  /* cost may be NULL */
int pba_affine_system_size(pba_engine* engine, int32_t* n);  /* 2·n_frames */
int pba_affine_get_system(pba_engine* engine, double* H_dense, double* g);
int pba_affine_step(pba_engine* engine, double lambda, double* model_decrease, int32_t* solver_status);
int pba_affine_get_step(pba_engine* engine, double* d_ab);
int pba_affine_candidate_cost(pba_engine* engine, double* cost);
int pba_affine_accept(pba_engine* engine);
/* The joint solve of poses, inverse distances and brightness (photometric engines with pba_set_affine_brightness; no
 * opt-in: the entry points are new, and pba_gn_* and pba_affine_* behave as before).  Exactly a Ceres solve with every
 * parameter block of the 18·P record free: 8 unknowns per keyframe, [δpose (6, right update T·exp δ) | δa δb], and one δρ
 * per point, with the pose solve's rules — per-block Huber through the Corrector (corrector.cc:42-110, ρ'' ≤ 0:
 * J̃ = √ρ' J, r̃ = √ρ' r; w = ρ'(Σr²) in the linearisation's own float arithmetic, a block out exactly when the other
 * solves count it invalid), cost Σ ½ρ(‖r‖²), damping (H + λ·clamp(diag H, 1e-6, 1e32)) δ = −g
 * (levenberg_marquardt_strategy.cc), the ρ eliminated into the 8·n_frames reduced system S δ_kf = −g_S
 * (schur_complement_solver.cc), δρ = −(g_ρ + Wᵀδ_kf)/H'_ρρ, model decrease ½(λ δᵀDδ − gᵀδ) over all free unknowns,
 * candidate T·exp(δpose), ρ + δρ, (a, b) + (δa, δb).
 * Constants (Problem::SetParameterBlockConstant, problem.h:306) get identity rows, a zero gradient and a zero step, the
 * two halves of a keyframe independently: its pose when it is in pba_set_fixed_frames or has no valid block; its (a, b)
 * when it is in pba_set_fixed_affine_frames (the brightness solve's call, reused), has no valid block, or has a
 * non-finite a or b.  AT LEAST ONE KEYFRAME'S (a, b) MUST BE CONSTANT: adding a common offset to every a, or any
 * consistent shift of the b's, leaves every residual unchanged, so with none fixed the undamped reduced system is
 * singular (measured smallest eigenvalue −5e-8, against 0.76 with keyframe 0 fixed); with λ > 0 the system is definite
 * either way.  pba_joint_step: solver_status ≠ 0 and no candidate when the damped reduced system is not positive
 * definite, as pba_gn_step.
 * pba_joint_get_reduced_system: the last step's system, dense (row-major, n = pba_joint_system_size = 8·n_frames), damped,
 * constants as identity / 0, and g_S — testing and inspection.  pba_joint_get_step: δ of the keyframes (8·n_frames) and
 * δρ (n_points); either may be NULL.  pba_joint_accept: poses, ρ and affine state ← candidate.
 * Every sum is fp64 in a fixed order, so results are bitwise reproducible.  They work at the engine's current pyramid
 * level; (a, b) carry no level factor.  One GPU; over several: pba_joint_step_export / import and
 * pba_solve_joint_distributed, below the multi-GPU Gauss-Newton.
 * pba_solve_joint: Ceres' trust-region loop (trust_region_minimizer.cc:67-136) driven from the host as pba_solve_affine
 * is, norms over the free poses (ambient [q | t]), the ρ of points with blocks and the free (a, b); a candidate with
 * fewer valid blocks than the current state counts as a failed evaluation (pba_solve's rule); fills the summary (the
 * device phase times stay 0) and the trajectory pba_solver_iterations serves.
 * Stale: pba_set_state*, pba_set_affine_state*, pba_set_fixed_frames, pba_set_fixed_affine_frames, pba_set_level,
 * pba_joint_accept, pba_affine_accept and pba_gn_accept (pba_solve, pba_solve_affine) leave a joint linearisation stale:
 * step, candidate cost, accept and the getters then return PBA_ERR_NOT_READY until pba_joint_linearize.
 * PBA_ERR_INVALID_ARGUMENT, nothing changed, on a geometric engine or without pba_set_affine_brightness (so never with
 * half records), and with free intrinsics unless pba_joint_set_solve_intrinsics, below, lets the solve free them too;
 * PBA_ERR_NOT_READY for a call before the one it
 * follows (step before linearize; candidate cost, accept and the getters before a step that succeeded). */
int pba_joint_linearize(pba_engine* engine, double* cost);  /* cost may be NULL */
int pba_joint_system_size(pba_engine* engine, int32_t* n);  /* 8·n_frames (+ 8·n_cams: pba_joint_set_solve_intrinsics) */
int pba_joint_step(pba_engine* engine, double lambda, double* model_decrease, int32_t* solver_status);
int pba_joint_get_reduced_system(pba_engine* engine, double* S_dense, double* g);
int pba_joint_get_step(pba_engine* engine, double* d_keyframes, double* d_inv_dist);
int pba_joint_candidate_cost(pba_engine* engine, double* cost);
int pba_joint_accept(pba_engine* engine);
/* The joint solve with free intrinsics: the full photometric problem — poses, inverse distances, (a, b) and the target
 * cameras' intrinsics (BundleAdjustmentOptions::optimize_intrinsics, map_utils.h:339-345) — in one solve.  Photometric
 * engines with both pba_set_optimize_intrinsics and pba_set_affine_brightness on (pba_set_intrinsics_with_affine).
 * Default 0: pba_joint_* and pba_solve_joint refuse such an engine as before.  With enable = 1 they run with the rows
 * of the 26·P record: unknowns 8 per keyframe [δpose | δa δb], then 8 per camera δk — with respect to the level-0
 * intrinsics state, a plain parameter block, k + δk — then one δρ per point.  The rules are the joint solve's
 * throughout: the Corrector weight in the linearisation's own float arithmetic, the damping
 * (H + λ·clamp(diag H, 1e-6, 1e32)) δ = −g over the intrinsics too (a parameter the camera model does not use has a
 * zero row and column, the pivot λ·1e-6, a zero gradient and a zero step), the model decrease over all free unknowns,
 * the candidate T·exp(δ), ρ + δρ, (a, b) + δ, k + δk.  A block whose projection with the intrinsics state is not finite
 * is invalid, as in the 26·P evaluation.
 * pba_joint_system_size becomes 8·(n_frames + n_cams), keyframes first; pba_joint_get_reduced_system is dense at that
 * size; pba_joint_get_step keeps its two arguments and their sizes, and pba_joint_get_intrinsics_step returns the
 * cameras' 8·n_cams (PBA_ERR_INVALID_ARGUMENT without the switch, PBA_ERR_NOT_READY as pba_joint_get_step).
 * Constants: a camera that no valid block targets gets identity rows, a zero gradient and a zero step; the keyframes'
 * two halves as above, and at least one keyframe's (a, b) must be constant as above.
 * pba_joint_accept also moves the intrinsics state to the candidate: pba_get_intrinsics then returns the solved level-0
 * state, as after every pba_solve_joint that accepted a step.  pba_set_intrinsics_state leaves a joint linearisation
 * stale, like pba_set_affine_state.  At pyramid level l the solve works on that level: J_intr's columns 0–3 carry 2^−l
 * and the level's image of the state moves by 2^−l·δk in entries 0–3 and by δk in the distortion.
 * pba_solve_joint: the step norm, the state norm and the gradient max norm include the intrinsics of the cameras that
 * have a valid block (of the level-0 state; all 8 entries).
 * The switch is not one of the two pba_gn_set_solve_* opt-ins, which make no difference to it.
 * PBA_ERR_INVALID_ARGUMENT, nothing changed: enable = 1 on a geometric engine, or unless both
 * pba_set_optimize_intrinsics and pba_set_affine_brightness are on; turning either of them off clears the switch. */
int pba_joint_set_solve_intrinsics(pba_engine* engine, int32_t enable);
int pba_joint_get_intrinsics_step(pba_engine* engine, double* d_intrinsics);  /* 8·n_cams */
/* Image interpolator of the photometric residual (and of the device-sampled I_h,k): PBA_INTERP_BILINEAR (default,
 * the north star's) or PBA_INTERP_BICUBIC — Ceres' BiCubicInterpolator over Grid2D<uint8_t, 1>
 * (cubic_interpolation.h:252-344, edge clamp :403-414), the interpolator of PhotometricError<8>
 * (photometric_error.h:84): with PBA_CAMERA_EUCM the engine then evaluates that functor's residual exactly.
 * Applies to every evaluation and Gauss-Newton entry point. */
#define PBA_INTERP_BILINEAR 0
#define PBA_INTERP_BICUBIC 1
int pba_set_interpolator(pba_engine* engine, int32_t interpolator);
int pba_interpolator(const pba_engine* engine);
/* The interpolator at n positions uv (2 doubles each, (column, row) pixels, any value: outside the image the edge is
 * clamped as Grid2D does) of one frame of the active level: out = 3 floats per position [I, ∂I/∂u, ∂I/∂v]
 * (BiCubicInterpolator::Evaluate(r = v, c = u) returns f, dfdr = ∂I/∂v, dfdc = ∂I/∂u).  Synchronises. */
int pba_sample_image(pba_engine* engine, int32_t frame, int32_t n, const double* uv, float* out);
int pba_num_blocks(const pba_engine* engine);
int pba_num_points(const pba_engine* engine);
int pba_num_frames(const pba_engine* engine);
int pba_residuals_per_block(const pba_engine* engine);
/* records: n_blocks·record_floats floats; valid: n_blocks bytes (either may be NULL).  Synchronises. */
int pba_get_records(pba_engine* engine, float* records, uint8_t* valid);
/* the record array as stored (no decoding): n_blocks·pba_record_bytes bytes into dst, `bytes` = dst's capacity —
 * fp32 values, halves, or the 15·R-half records of PBA_RECORD_F16_SCALED.  Synchronises. */
int pba_get_records_raw(pba_engine* engine, void* dst, size_t bytes);
/* residuals only: n_blocks·R floats (the first R values of every record, one strided DMA copy instead of the
 * whole record — what a residual-only evaluation needs, trust_region_minimizer.cc:761-779); valid may be NULL.
 * Synchronises. */
int pba_get_residuals(pba_engine* engine, float* residuals, uint8_t* valid);
/* Asynchronous read-back in chunks (fp32 records only: PBA_RECORD_F16 and PBA_RECORD_F16_SCALED are refused): enqueues the copies of records and validity into caller-owned
 * page-locked memory behind the evaluation, chunk_blocks blocks per copy, and returns at once; pba_wait_records returns
 * once the chunk holding `block` has arrived.  Thread-safe for concurrent waiters (Ceres' evaluator threads), so the
 * per-block CostFunction::Evaluate work overlaps the transfer of later chunks (program_evaluator.h:187-258). */
int pba_get_records_async(pba_engine* engine, float* records, uint8_t* valid, int32_t chunk_blocks);
int pba_wait_records(pba_engine* engine, int32_t block);
/* page-locked host memory for the read-back buffers of an adapter (records / residuals then arrive by DMA at
 * full PCIe rate instead of being staged through a driver buffer) */
int pba_host_alloc(size_t bytes, void** ptr);
int pba_host_free(void* ptr);
/* per-block cost ½ρ(‖r‖²) with the engine's Huber width (0 for invalid blocks) */
int pba_get_block_costs(pba_engine* engine, float* costs);
/* Σ block costs, summed in double on the host; n_valid may be NULL */
int pba_get_cost(pba_engine* engine, double* total_cost, int32_t* n_valid);

/* Device-side access for in-process consumers (zero copy) ----------------------------------------- */
/* hipStream_t the engine enqueues on (may be replaced with pba_set_stream; NULL = engine's own) */
int pba_set_stream(pba_engine* engine, void* hip_stream);
int pba_get_stream(pba_engine* engine, void** hip_stream);
/* d_records addresses the records as stored, pba_record_bytes per block: floats, 14·R halves (PBA_RECORD_F16) or the
 * 15·R halves [r | J_host | J_target | J_rho | e] of PBA_RECORD_F16_SCALED */
int pba_device_records(pba_engine* engine, float** d_records, uint8_t** d_valid, float** d_costs);
/* Expand the engine's records, in any format, to n_blocks·pba_record_floats fp32 values at d_out (device memory; 16-B
 * stores when it is 16-B aligned, 4-B stores otherwise): a copy for PBA_RECORD_F32, half → float for PBA_RECORD_F16, (float)half · (float)e for
 * PBA_RECORD_F16_SCALED — the values pba_get_records returns.  Enqueued on the engine's stream, for in-process
 * consumers of pba_device_records that want the fp32 Jacobian blocks of residual_block.cc:69-158. */
int pba_decode_records_device(pba_engine* engine, float* d_out);

/* Kernel timing: when enabled, every pba_evaluate brackets its residual/Jacobian block kernel with
 * hipEvents on the engine stream; pba_get_kernel_timing synchronises, returns the summed device time of
 * the block kernel (ms) and the launch count since the last call, and resets. */
int pba_enable_kernel_timing(pba_engine* engine, int32_t enable);
int pba_get_kernel_timing(pba_engine* engine, double* total_ms, int32_t* launches);

/* On-device Gauss-Newton / Levenberg-Marquardt --------------------------------
 * Replaces the solver side of ceres::Solve for this problem (map_utils.h:378-383: LM, SPARSE_SCHUR): the
 * normal equations JᵀJ / Jᵀr are accumulated on the device with the Huber corrector of
 * residual_block.cc:161-196, the inverse distances are eliminated (Schur complement; the <2,1,6>
 * structure of schur_complement_solver.cc:138-146), and the reduced camera system is factorised on the
 * device (block-skyline Cholesky, fp64).  Damping follows levenberg_marquardt_strategy.cc: (H + λ·D)δ = −g
 * with D = diag(JᵀJ) clamped to [1e-6, 1e32], λ = 1/trust-region radius. */
/* Termination as Ceres' TerminationType (types.h): CONVERGENCE on a tolerance or the minimum trust region radius,
 * NO_CONVERGENCE (here MAX_ITERATIONS) after max_iterations, FAILURE after max_num_consecutive_invalid_steps invalid
 * steps; stop_reason says which test ended the solve (trust_region_minimizer.cc, in its order of evaluation):
 *   gradient tolerance   max |x − (x ⊞ −∇)| ≤ gradient_tolerance at an accepted state (or the initial one), :668-684
 *   parameter tolerance  |x − x_candidate| ≤ parameter_tolerance (|x| + parameter_tolerance) for a valid step, with
 *                        |x| = −1 until the first accepted step (x_norm_, :185 / :814), :706-726
 *   function tolerance   |cost − candidate cost| ≤ function_tolerance · cost for a valid step, :729-748
 *   (neither candidate is applied) — norms in the ambient parameter space of the non-constant parameter blocks
 *   (poses as Sophus [q | t], inverse distances).  A candidate that leaves a block invalid which is valid at the current
 *   state has infinite cost (Ceres' failed Evaluate, :771-778). */
#define PBA_TERMINATION_CONVERGENCE 0
#define PBA_TERMINATION_MAX_ITERATIONS 1
#define PBA_TERMINATION_FAILURE 2

#define PBA_STOP_MAX_ITERATIONS 0
#define PBA_STOP_FUNCTION_TOLERANCE 1
#define PBA_STOP_PARAMETER_TOLERANCE 2
#define PBA_STOP_GRADIENT_TOLERANCE 3
#define PBA_STOP_MIN_TRUST_REGION_RADIUS 4
#define PBA_STOP_INVALID_STEPS 5

typedef struct pba_solver_options {
  int32_t max_iterations;                     /* BundleAdjustmentOptions::max_num_iterations (20, map_utils.h:318) */
  int32_t max_num_consecutive_invalid_steps;  /* Ceres default 5 (<= 0: 5) */
  double initial_trust_region_radius;         /* Ceres default 1e4 */
  double function_tolerance;                  /* Ceres default 1e-6 */
  double parameter_tolerance;                 /* Ceres default 1e-8 */
  double min_relative_decrease;               /* Ceres default 1e-3 */
  double gradient_tolerance;                  /* Ceres default 1e-10 */
  double max_trust_region_radius;             /* Ceres default 1e16 */
  double min_trust_region_radius;             /* Ceres default 1e-32 */
} pba_solver_options;

typedef struct pba_solver_summary {
  int32_t iterations;                   /* trials, the one that met a function / parameter tolerance included */
  int32_t successful_steps, unsuccessful_steps, termination;
  double initial_cost, final_cost;      /* Σ ½ρ(‖r‖²) */
  /* total_ms: host wall clock of the whole solve.  The parts: pba_solve — device time between stream events, only
   * with pba_set_solver_timing(engine, 1) (the events cost the GPU a few µs of idle time each, so they are off by
   * default and the parts are then 0): solve_ms = Schur complement + reduced solve + candidate state, linearize_ms =
   * the linearisation at each candidate (which is also its cost; plus the initial one), cost_ms = the decision; pba_solve_distributed — host wall clock of each phase, collectives included. */
  double total_ms, linearize_ms, solve_ms, cost_ms;
  double gradient_max_norm;             /* at the last state whose gradient was evaluated; pba_solve_distributed(_comm):
                                         * rank-local — max(the global pose part, this rank's points) */
  int32_t stop_reason, pad_;            /* PBA_STOP_* */
} pba_solver_summary;
/* per-phase device timing of pba_solve (linearize_ms / solve_ms / cost_ms of the summary); default off */
int pba_set_solver_timing(pba_engine* engine, int32_t enable);

/* One entry of the last solve's trajectory — Ceres' Solver::Summary::iterations (IterationSummary, iteration_callback.h;
 * filled as trust_region_minimizer.cc does): entry 0 is the initial state (successful, cost = the initial cost, radius =
 * the initial radius); then one entry per trial Ceres would push — accepted, rejected, invalid (:476-483) or ending on the
 * minimum trust-region radius — but not the trial that met the parameter / function tolerance or the invalid-step limit
 * (Minimize returns before FinalizeIteration, :110-115, :453-466).  cost: accepted — the new state's; rejected — the
 * candidate's (:124); invalid — the current state's.  trust_region_radius: after this iteration's update (:327).
 * gradient_max_norm: at the state the iteration ended in (a rejected step keeps the previous one, :130); after a
 * distributed solve it is rank-local (the global pose part, this rank's points), where Ceres reports the global value. */
typedef struct pba_iteration_summary {
  int32_t iteration, step_is_successful, step_is_valid, pad_;
  double cost, cost_change, relative_decrease, trust_region_radius, step_norm, gradient_max_norm;
} pba_iteration_summary;
/* copies min(capacity, entries) entries of the last pba_solve / pba_solve_distributed(_comm) into out (may be NULL with
 * capacity 0) and the number of entries into count; replaces reading Solver::Summary::iterations (map_utils.h:384-392) */
int pba_solver_iterations(const pba_engine* engine, int32_t capacity, pba_iteration_summary* out, int32_t* count);
/* the brightness solve's LM loop (see pba_affine_linearize above) */
int pba_solve_affine(pba_engine* engine, const pba_solver_options* options, pba_solver_summary* summary);
/* the joint solve's LM loop (see pba_joint_linearize above) */
int pba_solve_joint(pba_engine* engine, const pba_solver_options* options, pba_solver_summary* summary);

/* constant parameter blocks (Problem::SetParameterBlockConstant, map_utils.h:334-336) */
int pba_set_fixed_frames(pba_engine* engine, int32_t n, const int32_t* frames);
/* Jacobian evaluation at the current state + normal-equation pieces; cost may be NULL */
int pba_gn_linearize(pba_engine* engine, double* cost);
/* Schur complement for damping lambda, reduced-system solve, candidate state; solver_status ≠ 0 when the
 * reduced system was not positive definite (the candidate is then not formed) */
int pba_gn_step(pba_engine* engine, double lambda, double* model_decrease, int32_t* solver_status);
int pba_gn_candidate_cost(pba_engine* engine, double* cost);
int pba_gn_accept(pba_engine* engine);   /* state ← candidate */
/* full LM loop (trust_region_minimizer.cc semantics); options may be NULL (Ceres defaults, 20 iterations).
 * A candidate counts as a failed evaluation (cost DBL_MAX, trust_region_minimizer.cc:771-778) when it has fewer valid
 * blocks than the current state — exactly Ceres' rule when every block is valid at the current state (the normal case:
 * an invalid block has no residual for Ceres either); from a state that already has invalid blocks, a block turning
 * valid can mask another turning invalid. */
int pba_solve(pba_engine* engine, const pba_solver_options* options, pba_solver_summary* summary);
/* read back the state (7·n_frames poses, n_points inverse distances) */
int pba_get_state(pba_engine* engine, double* poses, double* inv_dist);
/* testing/inspection: reduced camera system as a dense n² matrix, n = pba_gn_system_size (6·n_frames, + 12 per camera
 * with free intrinsics), and its right-hand side g (the solve is S δ = −g), and the last step (δ poses 6·n_frames, δρ
 * n_points) */
int pba_gn_system_size(pba_engine* engine, int32_t* n);
int pba_gn_get_reduced_system(pba_engine* engine, double* S_dense, double* g);
int pba_gn_get_step(pba_engine* engine, double* d_poses, double* d_inv_dist);

/* Multi-GPU Gauss-Newton ------------------------------------------------------------
 * One engine per GPU.  Every engine holds ALL keyframes (global frame indices, identical poses) and the
 * points hosted by its shard of keyframes with all their blocks, so the inverse distances are eliminated
 * locally (a point's blocks never leave its host's rank).  The only exchange is the sum of the per-rank
 * reduced camera systems: rank r contributes S_r = A_r − B_r (C_r + λD_C)⁻¹ B_rᵀ, its gradients and the
 * undamped pose diagonal; after the all-reduce every rank adds λ·clamp(diag), applies the constant frames
 * and solves the same system (block cyclic reduction / band Cholesky), then back-substitutes its own points.
 *
 * The exchange buffer is a DEVICE array of pba_gn_exchange_size doubles, banded with K ∈ {4, 8, 16} block
 * rows, K ≥ max over ranks of pba_gn_band: per frame i, (K+1) 6×6 blocks (block c = column i−K+c, row
 * major) followed by 24 doubles [g(6) | g_direct(6) | diag(A)(6) | observed | 0…]; with free intrinsics
 * (pba_set_optimize_intrinsics) then the 2·n_cams border rows of nfs = n_frames + 2·n_cams frames: per row, nfs 6×6
 * blocks (block y = column y; those right of the diagonal unused) and the same 24-double tail (observed = a camera this
 * rank observes) — the summed system is then solved as a skyline with its active front in LDS; then 16 scalar
 * slots. */
int pba_gn_band(pba_engine* engine, int32_t* band);   /* local reduced-system bandwidth (block rows) */
int pba_gn_exchange_size(pba_engine* engine, int32_t band, int64_t* count);
/* after pba_gn_linearize: point elimination for lambda + this rank's partial system into d_exchange */
int pba_gn_step_export(pba_engine* engine, double lambda, int32_t band, double* d_exchange);
/* d_exchange holds the sum over ranks: damping, constant frames, solve, candidate state.  model_pose is the
 * pose part of the LM model decrease (identical on every rank), model_points this rank's point part. */
int pba_gn_step_import(pba_engine* engine, double lambda, int32_t band, const double* d_exchange,
                       double* model_pose, double* model_points, int32_t* solver_status);
/* pba_solve over all ranks, steered by the device LM record as on one GPU: per trial, the banded partial systems
 * (and border rows; count = pba_gn_exchange_size − 16 doubles) and then 16 scalars are summed over the ranks: the point part (model
 * decrease, candidate cost and valid blocks, step and state norms, points above the gradient tolerance) from every
 * rank, and — with a pba_comm — the pose part and the reduced solve's status from rank 0 alone, so every rank takes the
 * same decision on the device from bit-identical inputs.  Two collectives per trial (trial i + 1's damping, hence its point elimination, depends
 * on trial i's decision).
 *
 * The collective is either a host callback — the in-place sum over all ranks of count doubles at d_buf (device memory
 * of this engine's GPU), called after the engine's stream has drained and complete when it returns — or a pba_comm,
 * whose sums are enqueued on the engine's stream (the host then enqueues trial i + 1 before trial i's decision is
 * known, as pba_solve does). */
typedef int (*pba_allreduce_fn)(void* user, double* d_buf, int64_t count);
/* This engine's rank in the host-callback collective of pba_solve_distributed (a pba_comm knows its own): rank 0 then
 * contributes the pose part and the solve status to the scalar sum as with a pba_comm; −1 (the default) leaves every
 * rank deciding from its own, bit-identical, copy. */
int pba_gn_set_rank(pba_engine* engine, int32_t rank);
int pba_solve_distributed(pba_engine* engine, const pba_solver_options* options, int32_t band, double* d_exchange,
                          pba_allreduce_fn allreduce, void* user, pba_solver_summary* summary);
/* Communicators.  RCCL (one process per GPU, over xGMI): rank 0 gets a 128-byte id from pba_comm_unique_id and shares
 * it (e.g. with torch.distributed.broadcast); every rank calls pba_comm_init (collective).  librccl.so.1 is opened at
 * run time.  In-process group (tests / one-GPU rehearsal): pba_comm_init_local(n, device, comms) fills comms[0..n) for n
 * engines on one device driven by n host threads; sums in rank order through events.  pba_comm_allreduce enqueues the
 * in-place sum of count doubles at d_buf on hip_stream (every rank, same order). */
typedef struct pba_comm pba_comm;
int pba_comm_unique_id(void* id128);
int pba_comm_init(const void* id128, int32_t n_ranks, int32_t rank, int32_t device, pba_comm** out_comm);
int pba_comm_init_local(int32_t n_ranks, int32_t device, pba_comm** out_comms);
int pba_comm_destroy(pba_comm* comm);
int pba_comm_rank(const pba_comm* comm);
int pba_comm_size(const pba_comm* comm);
int pba_comm_allreduce(pba_comm* comm, double* d_buf, int64_t count, void* hip_stream);
/* pba_solve_distributed over a communicator, with an exchange buffer owned by the engine */
int pba_solve_distributed_comm(pba_engine* engine, const pba_solver_options* options, int32_t band, pba_comm* comm,
                               pba_solver_summary* summary);

/* Multi-GPU joint solve of poses, inverse distances and (a, b) -------------------------------------------
 * The arrangement above for the joint solve (pba_joint_linearize): every engine holds ALL keyframes (global indices,
 * identical poses and identical affine state) and the points hosted by its shard of keyframes with all their blocks, so
 * the inverse distances are eliminated locally.  Rank r contributes its undamped keyframe system with its points
 * eliminated at λ, S_r = A_r − B_r (C_r + λ·clamp(C_r))⁻¹ B_rᵀ, its Schur gradient, its direct gradient, its undamped
 * direct diagonal and, per keyframe, the number of valid blocks on it.  Damping and constants come AFTER the sum,
 * because a rank cannot decide them (a keyframe without a valid block on this rank may have one on another): every rank
 * adds λ·clamp(diag, 1e-6, 1e32) on the free diagonal, makes a keyframe's pose constant when it is in
 * pba_set_fixed_frames or its summed count is 0, its (a, b) constant when it is in pba_set_fixed_affine_frames, its
 * summed count is 0 or its a or b is not finite, solves the same system, back-substitutes its own δρ and forms its
 * candidate.
 *
 * The exchange buffer is a DEVICE array of pba_joint_exchange_size doubles, banded with K block rows, any K with
 * max over ranks of pba_joint_band ≤ K ≤ n_frames − 1 (the summed system is solved as a skyline over the band's
 * profile): per keyframe i, (K+1) row-major 8×8 blocks (block c = column i−K+c; blocks left of column 0 and blocks
 * outside the rank's own profile are zeros), followed by 32 doubles [g_S(8) | g_direct(8) | diag(8) | valid blocks on
 * the keyframe | 0…]; after all keyframes, 16 scalar slots.  An export writes every double of the buffer (the scalar
 * slots as zeros), in fp64 sums of a fixed order: two exports of one linearisation are bit-identical, and two ranks
 * importing the same buffer get the same keyframe step bit for bit.
 *
 * pba_joint_step_export: after pba_joint_linearize, the point elimination for lambda and this rank's contribution.
 * pba_joint_step_import: d_exchange holds the sum over the ranks of exports at the same lambda and band — damping,
 * constants, solve, this rank's δρ and candidate.  model_keyframes is the keyframes' part of the model decrease
 * (identical on every rank, to be counted once), model_points this rank's points'.  After an import
 * pba_joint_get_reduced_system and pba_joint_get_step serve the summed damped system and the step, and
 * pba_joint_candidate_cost (this rank's blocks) and pba_joint_accept work as after pba_joint_step.
 * pba_solve_joint_distributed: pba_solve_joint over all ranks with the host-callback collective of
 * pba_solve_distributed (the joint loop is host-driven; there is no pba_comm variant).  Per linearisation the scalar
 * slots are summed once (cost, valid blocks, ‖x‖² of this rank's points, this rank's groups of 256 points with a
 * gradient entry above the tolerance); per trial the system (pba_joint_exchange_size − 16 doubles), then the scalar
 * slots (the points' part of the model decrease, the candidate's cost and valid blocks, ‖δ‖² and ‖x‖² of this rank's
 * points).  The keyframes' parts are computed by every rank from the same summed buffer and counted once, so every
 * rank decides from bit-identical numbers and no decision is exchanged.  Summary, trajectory, the rule for a candidate
 * with fewer valid blocks (over all ranks) and staleness as pba_solve_joint.  gradient_max_norm is rank-local:
 * max(the keyframes' part, this rank's points), the keyframes' part being that of the last summed system (a
 * linearisation's own only after its first trial); the gradient-tolerance stop uses the summed count, and where that
 * is 0 one more sum of the system (exported at λ = 0) gives the linearisation's own keyframe part.
 * PBA_ERR_INVALID_ARGUMENT: an engine pba_joint_linearize refuses, a band below pba_joint_band or above n_frames − 1,
 * a null buffer or callback.  PBA_ERR_NOT_READY: an export before pba_joint_linearize, an import before an export of
 * this linearisation at the same lambda and band, and an engine without blocks — the caller chooses keyframe ranges
 * that leave at least one block on every rank. */
int pba_joint_band(pba_engine* engine, int32_t* band);   /* local bandwidth of the 8×8-block system, block rows */
int pba_joint_exchange_size(pba_engine* engine, int32_t band, int64_t* count);   /* doubles */
int pba_joint_step_export(pba_engine* engine, double lambda, int32_t band, double* d_exchange);
int pba_joint_step_import(pba_engine* engine, double lambda, int32_t band, const double* d_exchange,
                          double* model_keyframes, double* model_points, int32_t* solver_status);
int pba_solve_joint_distributed(pba_engine* engine, const pba_solver_options* options, int32_t band, double* d_exchange,
                                pba_allreduce_fn allreduce, void* user, pba_solver_summary* summary);

/* Image pyramid / coarse-to-fine ------------------------------------------
 * pba_build_pyramid builds levels 1 … n−1 on the device from the current frames, cameras and points (DSO
 * convention): level l+1 pixel = round(mean of a 2×2 level-l block), W_{l+1} = ⌊W_l/2⌋; camera fx_l = fx/2^l,
 * c_l = (c + 0.5)/2^l − 0.5 (distortion unchanged); u_ref_l likewise; the same pattern offsets; I_h,k re-sampled
 * from the host's level-l image.  pba_set_level selects the level every evaluation / Gauss-Newton entry point
 * runs on (state and problem structure are shared by all levels).  Any pba_set_cameras/frames/pattern/points
 * call returns to level 0 and drops the pyramid.  Photometric engines only. */
#define PBA_MAX_LEVELS 8
int pba_build_pyramid(pba_engine* engine, int32_t n_levels);
int pba_num_levels(const pba_engine* engine);
int pba_set_level(pba_engine* engine, int32_t level);
int pba_get_level(const pba_engine* engine, int32_t* level, int32_t* width, int32_t* height);
/* the active level's I_h,k (n_points·P floats) */
int pba_get_host_intensities(pba_engine* engine, float* host_intensity);
/* pba_solve on levels n−1 … 0 (coarse to fine); the summary sums iterations/timings, initial cost of the
 * coarsest level, final cost at level 0 */
int pba_solve_pyramid(pba_engine* engine, const pba_solver_options* options, pba_solver_summary* summary);

/* Reprojections and outlier flags after a bundle-adjustment pass -------------------
 * pba_compute_projections replaces compute_projections() + set_outlier_flags() of src/sfm.cpp:1928-2008 for
 * any list of observations (inlier and outlier obs; the anchor's own observation included, as the reference
 * does): with the engine's current state, per observation i of point p in frame f
 *   p_c = T_w_f⁻¹ · T_w_host(p) · (normalize(π_host⁻¹(u_ref(p))) / ρ_p)   (Landmark::get_p, common_types.h:205-217)
 *   reprojected = π_f(p_c), error = ‖obs_uv − reprojected‖, and for inlier observations the flags below
 *   (thresholds: sfm.cpp:254-261 defaults 3 px, 40 px, 0.1 m, 0.05 m when th == NULL).
 * fp64 throughout, at pyramid level 0.  All pointers are host pointers; obs_is_outlier, reprojected, point_c,
 * error, flags may be NULL. */
#define PBA_OUTLIER_NONE 0u
#define PBA_OUTLIER_REPROJECTION_HUGE 1u     /* error > huge threshold       (common_types.h:279) */
#define PBA_OUTLIER_REPROJECTION_NORMAL 2u   /* error > normal threshold     (common_types.h:281) */
#define PBA_OUTLIER_CAMERA_DISTANCE 4u       /* ‖p_c‖ < distance threshold    (common_types.h:283) */
#define PBA_OUTLIER_Z_COORDINATE 8u          /* p_c.z < z threshold           (common_types.h:285) */

typedef struct pba_outlier_thresholds {
  double reprojection_error_normal_px;  /* reprojection_error_outlier_threshold_normal_pixel (3.0)  */
  double reprojection_error_huge_px;    /* reprojection_error_outlier_threshold_huge_pixel (40.0)   */
  double camera_center_distance_m;      /* camera_center_distance_outlier_threshold_meter (0.1)     */
  double z_coordinate_m;                /* z_coordinate_outlier_threshold_meter (0.05)              */
} pba_outlier_thresholds;

int pba_compute_projections(pba_engine* engine, int32_t n_obs, const int32_t* obs_point, const int32_t* obs_frame,
                            const double* obs_uv, const uint8_t* obs_is_outlier, const pba_outlier_thresholds* th,
                            double* reprojected, double* point_c, double* error, uint32_t* flags);
/* remove_outlier_landmarks (sfm.cpp:2028-2114): remove[p] = 1 for points to drop.  Each point's inlier
 * observations are visited in frame-index order (= FrameCamId order when frames are indexed that way, as
 * pba_map_load does) and the first decisive flag wins; the normal-error flag removes a point only when no
 * observation anywhere carries another flag.  counts (may be NULL): [huge, normal, camera distance, z,
 * any_severe].  Host-only (no device needed). */
int pba_outlier_landmarks(int32_t n_points, int32_t n_obs, const int32_t* obs_point, const int32_t* obs_frame,
                          const uint32_t* flags, const uint8_t* obs_is_outlier, uint8_t* remove, int32_t* counts);

/* Problem loader from the reference's files ----------------------------------------
 * map.cereal (save_map_file, map_utils.h:58-86: cereal binary archive of corners, matches, tracks, outlier
 * tracks, cameras, landmarks; serializers serialization.h:155-205) + opt_calib.json (cereal JSON of the
 * Calibration, serialization.h:115-143; the DoubleSphere LoadCalibration form is accepted too), turned into
 * the arrays of pba_set_cameras/frames/points/blocks exactly as bundle_adjustment builds its problem
 * (map_utils.h:322-375): frames = map cameras in FrameCamId order (frame_cam = cam_id), points = landmarks in
 * TrackId order anchored at their smallest observing FrameCamId (u_ref = that corner, ρ = inv_depth),
 * blocks = the other observations (u_obs = their corners).  Host-only; the getters copy into caller arrays
 * sized from pba_map_info (any pointer may be NULL). */
typedef struct pba_map pba_map;
typedef struct pba_map_info {
  int32_t n_frames, n_points, n_blocks, n_cams;
  int32_t camera_model;      /* PBA_CAMERA_* shared by all cameras */
  int32_t n_outlier_obs;     /* Landmark::outlier_obs entries */
  int32_t width, height;     /* from the calibration (0 when absent) */
} pba_map_info;
int pba_map_load(const char* map_path, const char* calib_path, pba_map** out_map);
int pba_map_destroy(pba_map* map);
int pba_map_get_info(const pba_map* map, pba_map_info* info);
/* intrinsics 8·n_cams [fx fy cx cy p1 p2 p3 p4]; T_i_c 7·n_cams (Sophus storage) */
int pba_map_get_cameras(const pba_map* map, double* intrinsics, double* T_i_c);
/* FrameCamId.frame_id, cam_id (= camera index) and T_w_c per frame */
int pba_map_get_frames(const pba_map* map, int64_t* frame_id, int32_t* frame_cam, double* poses);
int pba_map_get_points(const pba_map* map, int64_t* track_id, int32_t* host_frame, double* u_ref, double* inv_dist);
int pba_map_get_blocks(const pba_map* map, int32_t* block_point, int32_t* block_target, double* u_obs);
int pba_map_get_outlier_obs(const pba_map* map, int32_t* point, int32_t* frame, double* uv);

#ifdef __cplusplus
}
#endif

#endif /* PBA_H_ */
