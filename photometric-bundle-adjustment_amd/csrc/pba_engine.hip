// pba_engine.hip — the C ABI (include/pba.h) of the photometric BA residual/Jacobian engine and the engine's state:
// problem upload (image tiling, pair table, state) and read-back.  The evaluation itself — the block kernels and their
// launches — is pba_evaluate.hip; the record layout both sides read is pba_record.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pba_internal.h"
#include "pba_record.h"

using namespace pba;
using namespace pba::detail;

namespace pba {
namespace detail {
thread_local std::string g_last_error;
}  // namespace detail
}  // namespace pba

namespace {

// ------------------------------------------------------------------------------------------------
// Pair table: relative poses in fp64 (form_pair, pba_internal.h)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void make_pair(const double* __restrict__ poses, const int* __restrict__ pair_host,
                                          const int* __restrict__ pair_target, const int* __restrict__ frame_cam,
                                          const double* __restrict__ cams, const double* __restrict__ cams_t,
                                          PairRec* __restrict__ pairs, int i) {
  PairRec r;
  form_pair(poses, frame_cam, cams, cams_t, pair_host[i], pair_target[i], r);
  pairs[i] = r;
}

__global__ void pair_kernel(const double* __restrict__ poses, const int* __restrict__ pair_host,
                            const int* __restrict__ pair_target, const int* __restrict__ frame_cam,
                            const double* __restrict__ cams, const double* __restrict__ cams_t,
                            PairRec* __restrict__ pairs, int n_pairs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pairs) make_pair(poses, pair_host, pair_target, frame_cam, cams, cams_t, pairs, i);
}

// State upload fused with the pair kernel (one launch instead of two copies + pair_kernel): workgroups
// [0, pair_wgs) form the relative poses straight from the caller's pose array, the rest copy the poses and
// inverse distances into the engine's state buffers (16 B per lane, grid-stride).
__global__ void state_kernel(const double* __restrict__ src_poses, const double* __restrict__ src_rho,
                             double* __restrict__ poses, double* __restrict__ rho, int n_pose_d, int n_points,
                             const int* __restrict__ pair_host, const int* __restrict__ pair_target,
                             const int* __restrict__ frame_cam, const double* __restrict__ cams,
                             PairRec* __restrict__ pairs, int n_pairs, int pair_wgs) {
  if ((int)blockIdx.x < pair_wgs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pairs) make_pair(src_poses, pair_host, pair_target, frame_cam, cams, cams, pairs, i);
    return;
  }
  const long long stride = (long long)(gridDim.x - pair_wgs) * blockDim.x;
  const long long i0 = (long long)(blockIdx.x - pair_wgs) * blockDim.x + threadIdx.x;
  for (long long i = i0; i < n_pose_d; i += stride) poses[i] = src_poses[i];
  for (long long i = i0; i < n_points; i += stride) rho[i] = src_rho[i];
}

// ------------------------------------------------------------------------------------------------
// Image relayout: row-major u8 frames → 16×8 tiles with the edge-replicating apron (pba_device.h).  One lane per
// 16-texel tile row of the padded frame; texels beyond the padded frame are zero and never read.
// ------------------------------------------------------------------------------------------------
// Device → page-locked host copy by a kernel (the host buffer is mapped into the device's address space): 16-B
// stores over the bus when both ends are 16-B aligned, bytes otherwise.  Enqueued like any launch, so the host never
// waits inside the call — hipMemcpyAsync into the same buffers returned only when the data had arrived (C4 sample:
// 2.4 ms per Jacobian read-back spent inside the enqueue, tools/probe/c2_probe.py).
__global__ void host_copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long bytes) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
    const long long n16 = bytes >> 4;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (long long i = i0; i < n16; i += stride) d4[i] = s4[i];
    for (long long i = (n16 << 4) + i0; i < bytes; i += stride) dst[i] = src[i];
  } else {
    for (long long i = i0; i < bytes; i += stride) dst[i] = src[i];
  }
}

__global__ void tile_images_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                   int tiles_x, int tiles_y, long long n_rows) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  // i enumerates (frame, tile, row-in-tile) in destination order → 16-B coalesced stores
  const int r = (int)(i & 7);
  const long long tile = i >> 3;
  const long long tiles_per_frame = (long long)tiles_x * tiles_y;
  const long long f = tile / tiles_per_frame;
  const int t = (int)(tile - f * tiles_per_frame);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int yp = ty * kTileH + r, xp0 = tx * kTileW;
  const int y = min(max(yp - kImgPad, 0), H - 1);
  union { uint8_t b[16]; uint4 v; } row;
  const uint8_t* s = src + f * W * (long long)H + (long long)y * W;
  const bool yin = yp < H + 2 * kImgPad;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int xp = xp0 + j;
    row.b[j] = (yin && xp < W + 2 * kImgPad) ? s[min(max(xp - kImgPad, 0), W - 1)] : (uint8_t)0;
  }
  reinterpret_cast<uint4*>(dst)[i] = row.v;
}

}  // namespace

namespace pba {
namespace detail {

void launch_pairs(pba_engine* e, const double* poses, PairRec* pairs) {
  // a photometric pair's target part is the intrinsics state's (the geometric kernels read the state themselves and
  // keep the cameras in the table, as the Gauss-Newton kernels expect)
  const bool state = e->opt_intr && e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC;
  pair_kernel<<<(e->n_pairs + 255) / 256, 256, 0, e->stream>>>(poses, e->pair_host.p, e->pair_target.p, e->frame_cam.p,
                                                               e->intr_d.p, state ? e->intr_state_d.p : e->intr_d.p,
                                                               pairs, e->n_pairs);
}

}  // namespace detail
}  // namespace pba

extern "C" {

int pba_version(void) { return 104; }

const char* pba_status_string(int s) {
  switch (s) {
    case PBA_OK: return "ok";
    case PBA_ERR_INVALID_ARGUMENT: return "invalid argument";
    case PBA_ERR_DEVICE: return "device error";
    case PBA_ERR_OUT_OF_MEMORY: return "out of device memory";
    case PBA_ERR_NOT_READY: return "not ready (missing set_* call)";
    default: return "unknown status";
  }
}

const char* pba_last_error(void) { return g_last_error.c_str(); }

int pba_create(const pba_options* o, pba_engine** out) {
  if (!o || !out) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (o->residual_kind != PBA_RESIDUAL_PHOTOMETRIC && o->residual_kind != PBA_RESIDUAL_GEOMETRIC)
    return fail(PBA_ERR_INVALID_ARGUMENT, "unknown residual kind");
  if (o->camera_model < PBA_CAMERA_PINHOLE || o->camera_model > PBA_CAMERA_KB4)
    return fail(PBA_ERR_INVALID_ARGUMENT, "unknown camera model");
  int n = 0;
  hipError_t err = hipGetDeviceCount(&n);
  if (err != hipSuccess || n <= 0) return fail(PBA_ERR_DEVICE, "no HIP device available");
  if (o->device < 0 || o->device >= n) return fail(PBA_ERR_INVALID_ARGUMENT, "device ordinal out of range");
  PBA_HIP(hipSetDevice(o->device));
  pba_engine* e = new pba_engine();
  e->opt = *o;
  err = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking);
  if (err != hipSuccess) {
    delete e;
    return fail(PBA_ERR_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(err));
  }
  e->stream = e->own_stream;
  *out = e;
  return PBA_OK;
}

int pba_destroy(pba_engine* e) {
  if (!e) return PBA_OK;
  (void)hipSetDevice(e->opt.device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  e->intr.release(); e->intr_d.release(); e->frame_cam.release(); e->images.release(); e->u_ref.release(); e->host_int.release(); e->point_host_d.release();
  e->block_point.release(); e->block_pair.release(); e->block_pp.release(); e->u_obs.release(); e->pair_host.release();
  e->pair_target.release(); e->block_rec.release(); e->pairs.release(); e->poses.release(); e->rho.release(); e->out.release();
  e->cost.release(); e->valid.release(); e->affine_state.release();
  for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->chunk_ev) (void)hipEventDestroy(ev);
  if (e->res_ev) (void)hipEventDestroy(e->res_ev);
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  delete e;
  return PBA_OK;
}

int pba_set_stream(pba_engine* e, void* s) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  e->stream = s ? static_cast<hipStream_t>(s) : e->own_stream;
  return PBA_OK;
}

int pba_get_stream(pba_engine* e, void** s) {
  if (!e || !s) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  *s = e->stream;
  return PBA_OK;
}

// Camera tables from 8·n intrinsics: fp32 [fx fy cx cy p1..p4] (Jacobian chain) and the fp64 records (kCamD doubles
// each, pba_device.h) [fx fy cx cy p1..p4 | cx cy 1/fx 1/fy p1..p4], uploaded to f / d on the engine stream.
static int upload_cameras(pba_engine* e, int n_cams, const double* intrinsics, DevBuf<float>& f, DevBuf<double>& d) {
  std::vector<float> hf(8 * (size_t)n_cams);
  for (size_t i = 0; i < hf.size(); ++i) hf[i] = (float)intrinsics[i];
  for (int c = 0; c < n_cams; ++c)
    if (!(hf[8 * c] != 0.0f && hf[8 * c + 1] != 0.0f)) return fail(PBA_ERR_INVALID_ARGUMENT, "zero focal length");
  std::vector<double> hd((size_t)kCamD * n_cams, 0.0);
  for (int c = 0; c < n_cams; ++c) {
    const double* k = intrinsics + 8 * c;
    double* r = hd.data() + (size_t)kCamD * c;
    for (int j = 0; j < 8; ++j) r[j] = k[j];
    r[8] = k[2]; r[9] = k[3]; r[10] = 1.0 / k[0]; r[11] = 1.0 / k[1];
    for (int j = 4; j < 8; ++j) r[8 + j] = k[j];
  }
  PBA_HIP(f.resize(hf.size()));
  PBA_HIP(d.resize(hd.size()));
  PBA_HIP(hipMemcpyAsync(f.p, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipMemcpyAsync(d.p, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_set_cameras(pba_engine* e, int32_t n_cams, const double* intrinsics) {
  if (!e || n_cams <= 0 || n_cams > 32767 || !intrinsics) return fail(PBA_ERR_INVALID_ARGUMENT, "bad camera arguments");
  if (int rc = check_device(e)) return rc;
  reset_pyramid(e);
  if (int rc = upload_cameras(e, n_cams, intrinsics, e->intr, e->intr_d)) return rc;
  e->n_cams = n_cams;
  e->cams_h.assign(intrinsics, intrinsics + 8 * (size_t)n_cams);
  if (e->opt_intr) {
    e->intr_state_h = e->cams_h;
    return upload_intrinsics_state(e);
  }
  return PBA_OK;
}

}  // extern "C"

namespace pba {
namespace detail {

// intr_state / intr_state_d from the level-0 state intr_state_h: at pyramid level l the target projects with the
// level-l image of the state, fx/2^l, fy/2^l, c_l = (c + 0.5)/2^l − 0.5, distortion unchanged (pba_pyramid.hip).
int upload_intrinsics_state(pba_engine* e) {
  if (int rc = check_device(e)) return rc;  // (reset_pyramid reaches this from calls that touch no device otherwise)
  std::vector<double> k = e->intr_state_h;
  const double s = std::ldexp(1.0, -e->level);
  if (e->level > 0)
    for (int c = 0; c < e->n_cams; ++c) {
      double* r = k.data() + 8 * (size_t)c;
      r[0] *= s; r[1] *= s; r[2] = (r[2] + 0.5) * s - 0.5; r[3] = (r[3] + 0.5) * s - 0.5;
    }
  e->joint.linearized = false;  // (a joint linearisation with free intrinsics was formed at the old state)
  return upload_cameras(e, e->n_cams, k.data(), e->intr_state, e->intr_state_d);
}

// The inverse: level-0 fx = fx_l·2^l, c = (c_l + 0.5)·2^l − 0.5 (photometric engines keep the level-0 state on the host).
int download_intrinsics_state(pba_engine* e) {
  if (!e->opt_intr || e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC || e->n_cams <= 0) return PBA_OK;
  std::vector<double> k((size_t)kCamD * e->n_cams);
  PBA_HIP(hipMemcpyAsync(k.data(), e->intr_state_d.p, sizeof(double) * k.size(), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  const double s = std::ldexp(1.0, e->level);
  e->intr_state_h.resize(8 * (size_t)e->n_cams);
  for (int c = 0; c < e->n_cams; ++c) {
    const double* r = k.data() + (size_t)kCamD * c;
    double* o = e->intr_state_h.data() + 8 * (size_t)c;
    for (int j = 0; j < 8; ++j) o[j] = r[j];
    if (e->level > 0) {
      o[0] = r[0] * s; o[1] = r[1] * s; o[2] = (r[2] + 0.5) * s - 0.5; o[3] = (r[3] + 0.5) * s - 0.5;
    }
  }
  return PBA_OK;
}

}  // namespace detail
}  // namespace pba

extern "C" {

int pba_set_optimize_intrinsics(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (enable && e->record_format != PBA_RECORD_F32)
    return fail(PBA_ERR_INVALID_ARGUMENT, "free intrinsics need PBA_RECORD_F32 records (J_intr has no half format)");
  if (enable && e->affine && !e->intr_with_affine)
    return fail(PBA_ERR_INVALID_ARGUMENT,
                "free intrinsics and affine brightness are not combined without pba_set_intrinsics_with_affine");
  if (enable && e->n_cams <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_cameras first");
  if (int rc = check_device(e)) return rc;
  const bool on = enable != 0;
  if (on && !e->opt_intr) {  // the state starts at the cameras' (level-0) intrinsics
    e->intr_state_h = e->cams_h;
    if (int rc = upload_intrinsics_state(e)) return rc;
  }
  e->opt_intr = on;
  if (!on) e->joint_solve_intr = false;  // (pba_joint_set_solve_intrinsics needs both switches: asked for again)
  e->joint.linearized = false;           // (the joint solve's unknowns and rows change with the switch)
  e->evaluated = false;
  e->res_fresh = false;
  e->pairs_fresh = false;  // (a photometric pair's target part is the state's)
  e->gn.prepared = false;  // the reduced camera system gains / loses its intrinsics border
  if (e->n_blocks > 0) PBA_HIP(e->out.resize((size_t)e->n_blocks * e->rec_floats()));
  return PBA_OK;
}

// The affine state [a_0 b_0 a_1 b_1 …] at zeros (pba_set_affine_brightness, pba_set_frames*).
static int zero_affine_state(pba_engine* e) {
  if (e->n_frames <= 0) return PBA_OK;
  PBA_HIP(e->affine_state.resize(2 * (size_t)e->n_frames));
  PBA_HIP(hipMemsetAsync(e->affine_state.p, 0, sizeof(double) * 2 * (size_t)e->n_frames, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_set_affine_brightness(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC)
    return fail(PBA_ERR_INVALID_ARGUMENT, "affine brightness is photometric only");
  if (enable && e->record_format != PBA_RECORD_F32)
    return fail(PBA_ERR_INVALID_ARGUMENT, "affine brightness needs PBA_RECORD_F32 records (no half format)");
  if (enable && e->opt_intr && !e->intr_with_affine)
    return fail(PBA_ERR_INVALID_ARGUMENT,
                "affine brightness and free intrinsics are not combined without pba_set_intrinsics_with_affine");
  if (int rc = check_device(e)) return rc;
  const bool on = enable != 0;
  if (on)
    if (int rc = zero_affine_state(e)) return rc;
  e->affine = on;
  if (!on) e->gn_solve_affine = false;  // (the switch belongs to the affine engine: asked for again when it comes back)
  if (!on) e->joint_solve_intr = false;
  e->evaluated = false;
  e->res_fresh = false;
  if (e->n_blocks > 0) PBA_HIP(e->out.resize((size_t)e->n_blocks * e->rec_floats()));
  return PBA_OK;
}

// The opt-in that lets pba_set_optimize_intrinsics and pba_set_affine_brightness accept each other, in either order
// (26-column records [… | J_intr | J_ab_host | J_ab_target], pba_record.h).  Off, the default, the two refuse each other
// as they did before it existed.  The switch alone changes no record, size or evaluation.
int pba_set_intrinsics_with_affine(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC)
    return fail(PBA_ERR_INVALID_ARGUMENT, "free intrinsics with affine brightness is photometric only");
  if (enable && e->record_format != PBA_RECORD_F32)
    return fail(PBA_ERR_INVALID_ARGUMENT, "free intrinsics with affine brightness needs PBA_RECORD_F32 records");
  if (!enable && e->opt_intr && e->affine)
    return fail(PBA_ERR_INVALID_ARGUMENT, "both switches are on: turn one of them off first");
  e->intr_with_affine = enable != 0;
  return PBA_OK;
}

static int affine_state_ready(pba_engine* e, const void* p) {
  if (!e || !p) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (e->n_frames <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_frames first");
  if (!e->affine) return fail(PBA_ERR_NOT_READY, "pba_set_affine_brightness first");
  return check_device(e);
}

int pba_set_affine_state(pba_engine* e, const double* ab) {
  if (int rc = affine_state_ready(e, ab)) return rc;
  PBA_HIP(hipMemcpyAsync(e->affine_state.p, ab, sizeof(double) * 2 * (size_t)e->n_frames, hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));  // (the caller's memory is free to change on return)
  e->joint.linearized = false;
  return PBA_OK;
}

int pba_set_affine_state_device(pba_engine* e, const double* d_ab) {
  if (int rc = affine_state_ready(e, d_ab)) return rc;
  PBA_HIP(hipMemcpyAsync(e->affine_state.p, d_ab, sizeof(double) * 2 * (size_t)e->n_frames, hipMemcpyDeviceToDevice, e->stream));
  e->joint.linearized = false;
  return PBA_OK;
}

int pba_get_affine_state(pba_engine* e, double* ab) {
  if (int rc = affine_state_ready(e, ab)) return rc;
  PBA_HIP(hipMemcpyAsync(ab, e->affine_state.p, sizeof(double) * 2 * (size_t)e->n_frames, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_gn_set_solve_intrinsics(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC) return PBA_OK;  // (a geometric solve always frees them)
  const bool on = enable != 0;
  if (on != e->gn_solve_intr) e->gn.prepared = false;  // the reduced camera system gains / loses its intrinsics border
  e->gn_solve_intr = on;
  return PBA_OK;
}

int pba_gn_set_solve_affine(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (enable && !e->affine)
    return fail(PBA_ERR_INVALID_ARGUMENT, "pba_gn_set_solve_affine needs pba_set_affine_brightness");
  e->gn_solve_affine = enable != 0;  // (the GN structure does not depend on it: the same reduced camera system)
  return PBA_OK;
}

int pba_get_intrinsics(pba_engine* e, double* intrinsics) {
  if (!e || !intrinsics) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (e->n_cams <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_cameras first");
  if (e->opt_intr && e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC) {  // the level-0 state, whatever level is active
    std::copy(e->intr_state_h.begin(), e->intr_state_h.end(), intrinsics);
    return PBA_OK;
  }
  if (int rc = check_device(e)) return rc;
  std::vector<double> k((size_t)kCamD * e->n_cams);
  PBA_HIP(hipMemcpyAsync(k.data(), e->opt_intr ? e->intr_state_d.p : e->intr_d.p, sizeof(double) * k.size(),
                         hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  for (int c = 0; c < e->n_cams; ++c)
    for (int j = 0; j < 8; ++j) intrinsics[8 * c + j] = k[(size_t)kCamD * c + j];
  return PBA_OK;
}

int pba_set_intrinsics_state(pba_engine* e, const double* intrinsics) {
  if (!e || !intrinsics) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (!e->opt_intr) return fail(PBA_ERR_NOT_READY, "pba_set_optimize_intrinsics first");
  if (int rc = check_device(e)) return rc;
  for (int c = 0; c < e->n_cams; ++c)
    if (!((float)intrinsics[8 * c] != 0.0f && (float)intrinsics[8 * c + 1] != 0.0f))
      return fail(PBA_ERR_INVALID_ARGUMENT, "zero focal length");
  e->intr_state_h.assign(intrinsics, intrinsics + 8 * (size_t)e->n_cams);
  e->pairs_fresh = e->pairs_fresh && e->opt.residual_kind == PBA_RESIDUAL_GEOMETRIC;
  return upload_intrinsics_state(e);
}

// Per-block {point, host, target, host_cam << 16 | target_cam} for the fused-state prologue (pba_internal.h
// stage_tile); rebuilt whenever blocks or frame cameras change.  Blocks that no longer fit the frames/points
// are dropped (pba_set_blocks again).
static int upload_block_records(pba_engine* e) {
  const size_t nb = e->block_point_h.size();
  if (nb == 0 || e->n_blocks <= 0) return PBA_OK;
  std::vector<int4> rec(nb);
  const int nf = (int)e->frame_cam_h.size(), np = (int)e->point_host_h.size();
  for (size_t b = 0; b < nb; ++b) {
    const int p = e->block_point_h[b], t = e->block_target_h[b];
    const int h = p < np ? e->point_host_h[p] : nf;
    if (h >= nf || t >= nf) {
      e->n_blocks = 0;
      e->block_point_h.clear();
      e->block_target_h.clear();
      return PBA_OK;
    }
    rec[b] = make_int4(p, h, t, (e->frame_cam_h[h] << 16) | e->frame_cam_h[t]);
  }
  PBA_HIP(e->block_rec.upload(rec, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

static int set_frames_impl(pba_engine* e, int32_t n_frames, const int32_t* frame_cam, int32_t width,
                           int32_t height, const uint8_t* images, hipMemcpyKind kind) {
  if (!e || n_frames <= 0 || !frame_cam) return fail(PBA_ERR_INVALID_ARGUMENT, "bad frame arguments");
  if (e->n_cams <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_cameras first");
  for (int i = 0; i < n_frames; ++i)
    if (frame_cam[i] < 0 || frame_cam[i] >= e->n_cams) return fail(PBA_ERR_INVALID_ARGUMENT, "frame_cam out of range");
  const bool photometric = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC;
  if (photometric && (!images || width <= 1 || height <= 1))
    return fail(PBA_ERR_INVALID_ARGUMENT, "photometric engines need images of at least 2x2");
  if (photometric && (long long)width * height > (1LL << 31))
    return fail(PBA_ERR_INVALID_ARGUMENT, "image too large");
  if (int rc = check_device(e)) return rc;
  reset_pyramid(e);
  PBA_HIP(e->frame_cam.resize(n_frames));
  PBA_HIP(hipMemcpyAsync(e->frame_cam.p, frame_cam, n_frames * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (images) {
    // frames arrive row-major (the reference's cv::Mat / pangolin image rows) and are re-tiled once on the
    // device; host input is staged through a transient device buffer.
    const size_t bytes = (size_t)n_frames * width * height;
    const int tx = tiles_x_of(width), ty = (height + 2 * kImgPad + kTileH - 1) / kTileH;
    PBA_HIP(e->images.resize((size_t)n_frames * tiled_frame_bytes(width, height)));
    const uint8_t* src = images;
    DevBuf<uint8_t> staging;
    if (kind == hipMemcpyHostToDevice) {
      PBA_HIP(staging.resize(bytes));
      PBA_HIP(hipMemcpyAsync(staging.p, images, bytes, kind, e->stream));
      src = staging.p;
    }
    const long long n_rows = (long long)n_frames * tx * ty * kTileH;
    tile_images_kernel<<<(unsigned)((n_rows + 255) / 256), 256, 0, e->stream>>>(src, e->images.p, width, height,
                                                                               tx, ty, n_rows);
    PBA_HIP(hipGetLastError());
    PBA_HIP(hipStreamSynchronize(e->stream));
    staging.release();
    e->have_images = true;
  }
  PBA_HIP(hipStreamSynchronize(e->stream));
  e->frame_cam_h.assign(frame_cam, frame_cam + n_frames);
  e->pairs_fresh = false;
  e->gn.prepared = false;  // the GN structure (frame count, the pairs' camera records) is re-analysed on next use
  e->aff.planned = false;
  e->aff.fixed_h.clear();
  e->aff.linearized = e->aff.have_step = false;
  e->joint.planned = e->joint.linearized = false;
  e->n_frames = n_frames;
  e->width = width;
  e->height = height;
  if (e->affine)  // a new set of keyframes starts at a = b = 0
    if (int rc = zero_affine_state(e)) return rc;
  return upload_block_records(e);
}

int pba_set_frames(pba_engine* e, int32_t n_frames, const int32_t* frame_cam, int32_t width, int32_t height,
                   const uint8_t* images) {
  return set_frames_impl(e, n_frames, frame_cam, width, height, images, hipMemcpyHostToDevice);
}

int pba_set_frames_device(pba_engine* e, int32_t n_frames, const int32_t* frame_cam, int32_t width,
                          int32_t height, const uint8_t* d_images) {
  return set_frames_impl(e, n_frames, frame_cam, width, height, d_images, hipMemcpyDeviceToDevice);
}

int pba_set_pattern(pba_engine* e, int32_t P, const float* offsets) {
  if (!e || P <= 0 || P > PBA_MAX_PATTERN || !offsets) return fail(PBA_ERR_INVALID_ARGUMENT, "bad pattern");
  reset_pyramid(e);
  e->pattern_h.assign(offsets, offsets + 2 * P);
  e->P = P;
  e->evaluated = false;  // the records and contiguous residuals of the last evaluation were sized for the old P
  e->res_fresh = false;
  return PBA_OK;
}

int pba_set_points(pba_engine* e, int32_t n_points, const int32_t* host_frame, const double* u_ref,
                   const float* host_intensity) {
  if (!e || n_points <= 0 || !host_frame || !u_ref) return fail(PBA_ERR_INVALID_ARGUMENT, "bad point arguments");
  if (e->n_frames <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_frames first");
  const bool photometric = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC;
  if (photometric && e->P <= 0) return fail(PBA_ERR_NOT_READY, "photometric points need pba_set_pattern first");
  if (photometric && !host_intensity && !e->have_images)
    return fail(PBA_ERR_NOT_READY, "sampling host intensities needs the frames' images");
  for (int i = 0; i < n_points; ++i)
    if (host_frame[i] < 0 || host_frame[i] >= e->n_frames) return fail(PBA_ERR_INVALID_ARGUMENT, "host frame out of range");
  if (int rc = check_device(e)) return rc;
  reset_pyramid(e);
  PBA_HIP(e->u_ref.resize(n_points));
  PBA_HIP(hipMemcpyAsync(e->u_ref.p, u_ref, n_points * sizeof(double2), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(e->point_host_d.resize(n_points));
  PBA_HIP(hipMemcpyAsync(e->point_host_d.p, host_frame, n_points * sizeof(int), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(e->rho.resize(n_points));
  e->n_points = n_points;
  if (photometric) {
    PBA_HIP(e->host_int.resize((size_t)n_points * e->P));
    if (host_intensity) {
      PBA_HIP(hipMemcpyAsync(e->host_int.p, host_intensity, (size_t)n_points * e->P * sizeof(float),
                             hipMemcpyHostToDevice, e->stream));
    } else if (int rc = sample_host_intensities(e, e->u_ref.p, e->host_int.p)) {  // I_h,k from the host image
      return rc;
    }
    e->host_int_sampled = host_intensity == nullptr;
  }
  PBA_HIP(hipStreamSynchronize(e->stream));
  e->point_host_h.assign(host_frame, host_frame + n_points);
  e->state_set = false;
  e->joint.planned = e->joint.linearized = false;
  return PBA_OK;
}

int pba_set_blocks(pba_engine* e, int32_t n_blocks, const int32_t* block_point, const int32_t* block_target,
                   const double* u_obs) {
  if (!e || n_blocks <= 0 || !block_point || !block_target) return fail(PBA_ERR_INVALID_ARGUMENT, "bad block arguments");
  if (e->n_points <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_points first");
  const bool geometric = e->opt.residual_kind == PBA_RESIDUAL_GEOMETRIC;
  if (geometric && !u_obs) return fail(PBA_ERR_INVALID_ARGUMENT, "geometric blocks need u_obs");
  const long long rec = e->rec_floats();
  if ((long long)n_blocks * rec >= (1LL << 40)) return fail(PBA_ERR_INVALID_ARGUMENT, "problem too large");
  // distinct (host, target) pairs, in first-seen order
  std::vector<int> pair_of(n_blocks), ph, pt;
  std::vector<long long> keys;
  {
    std::vector<std::pair<long long, int>> seen;
    seen.reserve(n_blocks);
    for (int b = 0; b < n_blocks; ++b) {
      const int p = block_point[b], t = block_target[b];
      if (p < 0 || p >= e->n_points) return fail(PBA_ERR_INVALID_ARGUMENT, "block point out of range");
      if (t < 0 || t >= e->n_frames) return fail(PBA_ERR_INVALID_ARGUMENT, "block target out of range");
      const int h = e->point_host_h[p];
      if (h == t) return fail(PBA_ERR_INVALID_ARGUMENT, "block target equals the point's host");
      seen.emplace_back((long long)h * e->n_frames + t, b);
    }
    std::sort(seen.begin(), seen.end());
    for (size_t i = 0; i < seen.size(); ++i) {
      if (i == 0 || seen[i].first != seen[i - 1].first) {
        ph.push_back((int)(seen[i].first / e->n_frames));
        pt.push_back((int)(seen[i].first % e->n_frames));
      }
      pair_of[seen[i].second] = (int)ph.size() - 1;
    }
  }
  if (int rc = check_device(e)) return rc;
  const int np = (int)ph.size();
  PBA_HIP(e->block_point.resize(n_blocks));
  PBA_HIP(e->block_pair.resize(n_blocks));
  PBA_HIP(e->pair_host.resize(np));
  PBA_HIP(e->pair_target.resize(np));
  PBA_HIP(e->pairs.resize((size_t)np));
  PBA_HIP(hipMemcpyAsync(e->block_point.p, block_point, n_blocks * sizeof(int), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipMemcpyAsync(e->block_pair.p, pair_of.data(), n_blocks * sizeof(int), hipMemcpyHostToDevice, e->stream));
  std::vector<int2> pp(n_blocks);
  for (int b = 0; b < n_blocks; ++b) pp[b] = make_int2(block_point[b], pair_of[b]);
  PBA_HIP(e->block_pp.upload(pp, e->stream));
  PBA_HIP(hipMemcpyAsync(e->pair_host.p, ph.data(), np * sizeof(int), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipMemcpyAsync(e->pair_target.p, pt.data(), np * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (geometric) {
    PBA_HIP(e->u_obs.resize(n_blocks));
    PBA_HIP(hipMemcpyAsync(e->u_obs.p, u_obs, n_blocks * sizeof(double2), hipMemcpyHostToDevice, e->stream));
  }
  PBA_HIP(e->out.resize((size_t)n_blocks * rec));
  PBA_HIP(e->cost.resize(n_blocks));
  PBA_HIP(e->valid.resize(n_blocks));
  PBA_HIP(hipStreamSynchronize(e->stream));
  e->n_blocks = n_blocks;
  e->n_pairs = np;
  e->evaluated = false;
  e->res_fresh = false;
  e->chunk_blocks = 0;
  e->n_chunks_async = 0;
  e->chunks_arrived.store(0);
  e->pairs_fresh = false;
  e->block_point_h.assign(block_point, block_point + n_blocks);
  e->block_target_h.assign(block_target, block_target + n_blocks);
  e->pair_of_h = std::move(pair_of);
  e->pair_host_h = std::move(ph);
  e->pair_target_h = std::move(pt);
  e->gn.prepared = false;
  e->aff.planned = false;
  e->aff.linearized = e->aff.have_step = false;
  e->joint.planned = e->joint.linearized = false;
  return upload_block_records(e);
}

int pba_set_state(pba_engine* e, const double* poses, const double* inv_dist) {
  if (!e || !poses || !inv_dist) return fail(PBA_ERR_INVALID_ARGUMENT, "null state");
  if (e->n_points <= 0 || e->n_frames <= 0) return fail(PBA_ERR_NOT_READY, "problem not set");
  if (int rc = check_device(e)) return rc;
  PBA_HIP(e->poses.resize(7 * (size_t)e->n_frames));
  PBA_HIP(hipMemcpyAsync(e->poses.p, poses, 7 * (size_t)e->n_frames * sizeof(double), hipMemcpyHostToDevice, e->stream));
  PBA_HIP(hipMemcpyAsync(e->rho.p, inv_dist, (size_t)e->n_points * sizeof(double), hipMemcpyHostToDevice, e->stream));
  e->state_set = true;
  e->pairs_fresh = false;
  e->joint.linearized = false;
  return PBA_OK;
}

int pba_set_state_device(pba_engine* e, const double* d_poses, const double* d_inv_dist) {
  if (!e || !d_poses || !d_inv_dist) return fail(PBA_ERR_INVALID_ARGUMENT, "null state");
  if (e->n_points <= 0 || e->n_frames <= 0) return fail(PBA_ERR_NOT_READY, "problem not set");
  if (int rc = check_device(e)) return rc;
  PBA_HIP(e->poses.resize(7 * (size_t)e->n_frames));
  const int n_pose_d = 7 * e->n_frames;
  // the photometric evaluation forms its pairs itself (fused state); the table serves the geometric kernels
  const bool table = e->n_blocks > 0 && e->opt.residual_kind == PBA_RESIDUAL_GEOMETRIC;
  const int pair_wgs = table ? (e->n_pairs + 255) / 256 : 0;
  const int copy_wgs = std::min(1024, (std::max(n_pose_d, e->n_points) + 255) / 256);
  state_kernel<<<pair_wgs + copy_wgs, 256, 0, e->stream>>>(d_poses, d_inv_dist, e->poses.p, e->rho.p, n_pose_d,
                                                           e->n_points, e->pair_host.p, e->pair_target.p,
                                                           e->frame_cam.p, e->intr_d.p, e->pairs.p, e->n_pairs,
                                                           pair_wgs);
  PBA_HIP(hipGetLastError());
  e->state_set = true;
  e->pairs_fresh = table;
  e->joint.linearized = false;
  return PBA_OK;
}

namespace {

// One evaluation launch at state (poses, rho); with `adopt`, the same launch copies that state into the engine's
// buffers (it then is the engine's state, as after pba_set_state_device).
int evaluate_at(pba_engine* e, const double* poses, const double* rho, bool adopt, bool jac) {
  const bool photometric = e->opt.residual_kind == PBA_RESIDUAL_PHOTOMETRIC;
  if (photometric && (!e->have_images || e->P <= 0)) return fail(PBA_ERR_NOT_READY, "images/pattern missing");
  if (int rc = check_device(e)) return rc;
  KernelArgs ka;
  if (photometric) {
    // every photometric launch runs 8 lanes per block (photometric_block_kernel / _multi, launch_blocks)
    const long long lanes = (long long)e->n_blocks * 8;
    if (adopt && lanes < std::max<long long>(7LL * e->n_frames, e->n_points)) {
      if (int rc = pba_set_state_device(e, poses, rho)) return rc;  // more state than lanes: copy first
      poses = e->poses.p;
      rho = e->rho.p;
      adopt = false;
    }
    if (test_hook("PBA_TEST_PAIR_TABLE")) {
      // test build: the block kernels' pair-table prologue (stage_tile, a.poses == nullptr), which no launch of a
      // photometric engine takes otherwise — every evaluation and every cost-only launch is at a fused state.  The
      // state is copied first, the table formed from it, and the launch reads the table.
      if (adopt) {
        if (int rc = pba_set_state_device(e, poses, rho)) return rc;
        poses = e->poses.p;
        rho = e->rho.p;
        adopt = false;
      }
      launch_pairs(e, poses, e->pairs.p);
      e->pairs_fresh = false;
      ka = make_kernel_args(e, e->pairs.p, rho);
    } else {
      ka = make_kernel_args(e, nullptr, rho);
      ka.poses = poses;
    }
    if (adopt) {
      PBA_HIP(e->poses.resize(7 * (size_t)e->n_frames));
      ka.adopt_poses = e->poses.p;
      ka.adopt_rho = e->rho.p;
      e->state_set = true;
      e->pairs_fresh = false;
    }
  } else {
    if (adopt) {
      if (int rc = pba_set_state_device(e, poses, rho)) return rc;
    } else if (!e->pairs_fresh) {
      launch_pairs(e, e->poses.p, e->pairs.p);
    }
    e->pairs_fresh = true;
    ka = make_kernel_args(e, e->pairs.p, e->rho.p);
  }
  hipEvent_t ev_stop = nullptr;
  if (e->timing) {
    while (e->ev_pool.size() < e->ev_used + 2) {
      hipEvent_t ev;
      // timing-only events: no system-scope fence (no L2 writeback of the records inside the bracket)
      PBA_HIP(hipEventCreateWithFlags(&ev, hipEventDisableSystemFence));
      e->ev_pool.push_back(ev);
    }
    PBA_HIP(hipEventRecord(e->ev_pool[e->ev_used], e->stream));
    ev_stop = e->ev_pool[e->ev_used + 1];
    e->ev_used += 2;
  }
  if (!jac) {
    PBA_HIP(e->res.resize((size_t)e->n_blocks * e->R()));
    ka.res_out = e->res.p;
  }
  launch_mode(e, ka, jac ? 1 : 0);
  PBA_HIP(hipGetLastError());
  if (ev_stop) PBA_HIP(hipEventRecord(ev_stop, e->stream));
  e->evaluated = true;
  e->res_fresh = !jac;
  // a new evaluation invalidates an earlier asynchronous read-back (pba_wait_records then fails instead of returning)
  e->chunk_blocks = 0;
  e->n_chunks_async = 0;
  e->chunks_arrived.store(0);
  return PBA_OK;
}

}  // namespace

int pba_evaluate(pba_engine* e, int32_t want_jacobians) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (e->n_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  if (!e->state_set) return fail(PBA_ERR_NOT_READY, "pba_set_state first");
  return evaluate_at(e, e->poses.p, e->rho.p, false, want_jacobians != 0);
}

int pba_evaluate_state_device(pba_engine* e, const double* d_poses, const double* d_inv_dist, int32_t want_jacobians) {
  if (!e || !d_poses || !d_inv_dist) return fail(PBA_ERR_INVALID_ARGUMENT, "null state");
  if (e->n_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  return evaluate_at(e, d_poses, d_inv_dist, true, want_jacobians != 0);
}

int pba_evaluate_states_device(pba_engine* e, int32_t n, const double* const* d_poses, const double* const* d_inv_dist,
                               int32_t want_jacobians) {
  if (!e || n < 0 || (n > 0 && (!d_poses || !d_inv_dist))) return fail(PBA_ERR_INVALID_ARGUMENT, "null states");
  if (e->n_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_set_blocks first");
  for (int i = 0; i < n; ++i) {
    if (!d_poses[i] || !d_inv_dist[i]) return fail(PBA_ERR_INVALID_ARGUMENT, "null state");
    if (int rc = evaluate_at(e, d_poses[i], d_inv_dist[i], true, want_jacobians != 0)) return rc;
  }
  return PBA_OK;
}

int pba_enable_kernel_timing(pba_engine* e, int32_t enable) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  e->timing = enable != 0;
  return PBA_OK;
}

int pba_get_kernel_timing(pba_engine* e, double* total_ms, int32_t* launches) {
  if (!e || !total_ms) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (int rc = check_device(e)) return rc;
  PBA_HIP(hipStreamSynchronize(e->stream));
  double tot = 0;
  for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
    float ms = 0;
    PBA_HIP(hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]));
    tot += ms;
  }
  *total_ms = tot;
  if (launches) *launches = (int32_t)(e->ev_used / 2);
  e->ev_used = 0;
  return PBA_OK;
}

int pba_synchronize(pba_engine* e) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (int rc = check_device(e)) return rc;
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_record_floats(const pba_engine* e) { return e ? e->rec_floats() : 0; }

int pba_set_record_format(pba_engine* e, int32_t format) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (format != PBA_RECORD_F32 && format != PBA_RECORD_F16 && format != PBA_RECORD_F16_SCALED)
    return fail(PBA_ERR_INVALID_ARGUMENT, "unknown record format");
  if (format != PBA_RECORD_F32 && e->opt.residual_kind != PBA_RESIDUAL_PHOTOMETRIC)
    return fail(PBA_ERR_INVALID_ARGUMENT, "fp16 records are photometric only");
  if (format != PBA_RECORD_F32 && e->opt_intr)
    return fail(PBA_ERR_INVALID_ARGUMENT, "free intrinsics need PBA_RECORD_F32 records (J_intr has no half format)");
  if (format != PBA_RECORD_F32 && e->affine)
    return fail(PBA_ERR_INVALID_ARGUMENT, "affine brightness needs PBA_RECORD_F32 records (no half format)");
  e->record_format = format;
  e->evaluated = false;
  e->res_fresh = false;
  return PBA_OK;
}

int pba_record_format(const pba_engine* e) { return e ? e->record_format : PBA_RECORD_F32; }
int pba_record_bytes(const pba_engine* e) { return e ? e->rec_bytes() : 0; }
int pba_residuals_per_block(const pba_engine* e) { return e ? e->R() : 0; }
int pba_num_blocks(const pba_engine* e) { return e ? e->n_blocks : 0; }
int pba_num_points(const pba_engine* e) { return e ? e->n_points : 0; }
int pba_num_frames(const pba_engine* e) { return e ? e->n_frames : 0; }

int pba_get_records(pba_engine* e, float* records, uint8_t* valid) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (!e->evaluated) return fail(PBA_ERR_NOT_READY, "pba_evaluate first");
  if (int rc = check_device(e)) return rc;
  const size_t n = (size_t)e->n_blocks * e->rec_floats();
  const bool scaled = e->record_format == PBA_RECORD_F16_SCALED;
  std::vector<_Float16> half;
  if (records && e->record_format != PBA_RECORD_F32) {
    half.resize((size_t)e->n_blocks * e->rec_bytes() / sizeof(_Float16));
    PBA_HIP(hipMemcpyAsync(half.data(), e->out.p, half.size() * sizeof(_Float16), hipMemcpyDeviceToHost, e->stream));
  } else if (records) {
    PBA_HIP(hipMemcpyAsync(records, e->out.p, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  }
  if (valid) PBA_HIP(hipMemcpyAsync(valid, e->valid.p, e->n_blocks, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  if (scaled && records) {  // a Jacobian entry of pixel row k is stored divided by e[k] (as decode_records_kernel)
    const int R = e->R();
    for (size_t b = 0; b < (size_t)e->n_blocks; ++b) {
      const _Float16* s = half.data() + b * (RecFormat<ScaledF16>::kCols * R);
      float* d = records + b * col_tail(R);
      for (int c = 0; c < col_tail(R); ++c) {
        const int row = scale_row_of(c, R);
        d[c] = row < 0 ? (float)s[c] : (float)s[c] * (float)s[col_tail(R) + row];
      }
    }
  } else {
    for (size_t i = 0; i < half.size(); ++i) records[i] = (float)half[i];
  }
  return PBA_OK;
}

int pba_get_records_raw(pba_engine* e, void* dst, size_t bytes) {
  if (!e || !dst) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (!e->evaluated) return fail(PBA_ERR_NOT_READY, "pba_evaluate first");
  const size_t n = (size_t)e->n_blocks * e->rec_bytes();
  if (bytes < n) return fail(PBA_ERR_INVALID_ARGUMENT, "buffer smaller than n_blocks * pba_record_bytes");
  if (int rc = check_device(e)) return rc;
  PBA_HIP(hipMemcpyAsync(dst, e->out.p, n, hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

// Wait for an event by polling it (its completion signal lives in host memory) before falling back to a blocking
// wait: the read-backs of the Ceres adapter sit inside Ceres' evaluation timer, and a blocking wait's wake-up came late
// when the process's cgroup CPU quota was saturated by Ceres' own threads (C2 residual-only evaluations measured
// 0.7-1.8 ms box to box for the same work).  The poll is bounded in time (kEventSpinUs; a C2 read-back chunk arrives
// within ~0.1 ms), so a long wait — or several of Ceres' threads waiting at once — blocks instead of spinning on the
// quota Ceres' own threads need.
constexpr double kEventSpinUs = 200.0;
static hipError_t wait_event(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned i = 0;; ++i) {
    const hipError_t q = hipEventQuery(ev);
    if (q != hipErrorNotReady) return q;
    __builtin_ia32_pause();
    if ((i & 63u) == 63u &&
        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > kEventSpinUs)
      break;
  }
  return hipEventSynchronize(ev);
}

// Enqueue a device → host copy: by host_copy_kernel when the destination is page-locked memory mapped for the device
// (pba_host_alloc), else hipMemcpyAsync.
// The device address of a page-locked host buffer (the base of its allocation: an interior pointer is not found), or
// nullptr for other memory.
static void* mapped_device_ptr(void* host) {
  void* dd = nullptr;
  if (hipHostGetDevicePointer(&dd, host, 0) != hipSuccess) {
    (void)hipGetLastError();  // (not a mapped host allocation: clear the query's error)
    return nullptr;
  }
  return dd;
}

// dd: dst's device address (mapped_device_ptr of its allocation, plus the offset), or nullptr.
static int enqueue_to_host(pba_engine* e, void* dst, void* dd, const void* src, size_t bytes) {
  if (!bytes) return PBA_OK;
  if (dd) {
    const long long n16 = (long long)((bytes + 15) >> 4);
    const int grid = (int)std::min<long long>(1024, std::max<long long>(1, (n16 + 255) / 256));
    host_copy_kernel<<<grid, 256, 0, e->stream>>>(static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dd),
                                                  (long long)bytes);
    PBA_HIP(hipGetLastError());
    return PBA_OK;
  }
  PBA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  return PBA_OK;
}

// Chunked asynchronous read-back for the Ceres adapter: the copies go out on the engine stream behind the evaluation,
// an event after each chunk; a caller waiting for one block only waits for its chunk, so Ceres' per-block work
// (CostFunction::Evaluate, the Jacobian writer) overlaps the PCIe transfer of the later chunks.
int pba_get_records_async(pba_engine* e, float* records, uint8_t* valid, int32_t chunk_blocks) {
  if (!e || !records || !valid || chunk_blocks <= 0) return fail(PBA_ERR_INVALID_ARGUMENT, "bad async read-back arguments");
  if (!e->evaluated) return fail(PBA_ERR_NOT_READY, "pba_evaluate first");
  if (e->record_format != PBA_RECORD_F32) return fail(PBA_ERR_INVALID_ARGUMENT, "asynchronous read-back: fp32 records only");
  if (int rc = check_device(e)) return rc;
  const long long nb = e->n_blocks, rf = e->rec_floats();
  const int nc = (int)((nb + chunk_blocks - 1) / chunk_blocks);
  while ((int)e->chunk_ev.size() < nc) {
    hipEvent_t ev;
    PBA_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e->chunk_ev.push_back(ev);
  }
  e->chunk_blocks = chunk_blocks;
  e->n_chunks_async = nc;
  e->chunks_arrived.store(0);
  // the validity flags of every block in one copy ahead of the record chunks (a copy per chunk of chunk_blocks bytes was
  // small enough for the runtime to complete it on the host, which made every chunk's enqueue wait for the transfers
  // before it: the whole read-back then ran inside this call, 2.5 ms of the C4 sample's evaluation)
  float* rd = static_cast<float*>(mapped_device_ptr(records));
  if (int rc = enqueue_to_host(e, valid, mapped_device_ptr(valid), e->valid.p, (size_t)nb)) return rc;
  for (int c = 0; c < nc; ++c) {
    const long long b0 = (long long)c * chunk_blocks, n = std::min<long long>(chunk_blocks, nb - b0);
    if (int rc = enqueue_to_host(e, records + b0 * rf, rd ? rd + b0 * rf : nullptr, e->out.p + b0 * rf,
                                 sizeof(float) * (size_t)(n * rf)))
      return rc;
    PBA_HIP(hipEventRecord(e->chunk_ev[c], e->stream));
  }
  return PBA_OK;
}

int pba_wait_records(pba_engine* e, int32_t block) {
  if (!e || block < 0 || block >= e->n_blocks) return fail(PBA_ERR_INVALID_ARGUMENT, "bad wait arguments");
  // no read-back in flight for the current evaluation (pba_evaluate / pba_set_blocks reset it), or one that does not
  // cover this block: fail rather than report stale records as arrived
  if (e->chunk_blocks <= 0) return fail(PBA_ERR_NOT_READY, "pba_get_records_async first");
  const int c = block / e->chunk_blocks;
  if (c >= e->n_chunks_async || c >= (int)e->chunk_ev.size()) return fail(PBA_ERR_NOT_READY, "block not in the read-back");
  if (c < e->chunks_arrived.load(std::memory_order_acquire)) return PBA_OK;
  PBA_HIP(wait_event(e->chunk_ev[c]));  // chunks arrive in stream order: every chunk ≤ c is in
  int seen = e->chunks_arrived.load(std::memory_order_relaxed);
  while (seen < c + 1 && !e->chunks_arrived.compare_exchange_weak(seen, c + 1, std::memory_order_release)) {
  }
  return PBA_OK;
}

int pba_get_residuals(pba_engine* e, float* residuals, uint8_t* valid) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (!e->evaluated) return fail(PBA_ERR_NOT_READY, "pba_evaluate first");
  if (int rc = check_device(e)) return rc;
  const size_t R = (size_t)e->R(), nb = (size_t)e->n_blocks, RF = (size_t)e->rec_floats();
  std::vector<_Float16> half;
  if (residuals && nb && e->res_fresh && e->res.n >= nb * R) {
    // a residual-only evaluation also wrote its residuals contiguously: one plain device-to-host copy
    if (int rc = enqueue_to_host(e, residuals, mapped_device_ptr(residuals), e->res.p, nb * R * sizeof(float))) return rc;
  } else if (residuals && nb) {
    // the first R values of every record (14R values; 15R halves for PBA_RECORD_F16_SCALED, whose residuals are
    // unscaled): one pitched device-to-host copy
    if (e->record_format != PBA_RECORD_F32) {
      half.resize(nb * R);
      PBA_HIP(hipMemcpy2DAsync(half.data(), R * sizeof(_Float16), e->out.p, (size_t)e->rec_bytes(),
                               R * sizeof(_Float16), nb, hipMemcpyDeviceToHost, e->stream));
    } else {
      PBA_HIP(hipMemcpy2DAsync(residuals, R * sizeof(float), e->out.p, RF * sizeof(float), R * sizeof(float), nb,
                               hipMemcpyDeviceToHost, e->stream));
    }
  }
  if (valid)
    if (int rc = enqueue_to_host(e, valid, mapped_device_ptr(valid), e->valid.p, nb)) return rc;
  if (!e->res_ev) PBA_HIP(hipEventCreateWithFlags(&e->res_ev, hipEventDisableTiming));
  PBA_HIP(hipEventRecord(e->res_ev, e->stream));
  PBA_HIP(wait_event(e->res_ev));
  for (size_t i = 0; i < half.size(); ++i) residuals[i] = (float)half[i];
  return PBA_OK;
}

int pba_host_alloc(size_t bytes, void** ptr) {
  if (!ptr) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  *ptr = nullptr;
  // mapped into the device's address space: the read-backs into it are copy kernels (enqueue_to_host), not
  // hipMemcpyAsync, which returned only once a device-to-host copy had arrived
  PBA_HIP(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocMapped | hipHostMallocPortable));
  // touch every page from the device now: the first device access to fresh page-locked memory maps it into the GPU's
  // page tables (tools/micro/d2h_enqueue: 18.5 ms for 45 MB, against 0.9 ms per later 45-MB read-back) — setup work that
  // otherwise lands inside the first evaluation Ceres times
  void* dd = nullptr;
  if (bytes && hipHostGetDevicePointer(&dd, *ptr, 0) == hipSuccess && dd) {
    PBA_HIP(hipMemsetAsync(dd, 0, bytes, nullptr));
    PBA_HIP(hipStreamSynchronize(nullptr));
  }
  (void)hipGetLastError();
  return PBA_OK;
}

int pba_host_free(void* ptr) {
  if (ptr) PBA_HIP(hipHostFree(ptr));
  return PBA_OK;
}

int pba_get_block_costs(pba_engine* e, float* costs) {
  if (!e || !costs) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (!e->evaluated) return fail(PBA_ERR_NOT_READY, "pba_evaluate first");
  if (int rc = check_device(e)) return rc;
  PBA_HIP(hipMemcpyAsync(costs, e->cost.p, e->n_blocks * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  PBA_HIP(hipStreamSynchronize(e->stream));
  return PBA_OK;
}

int pba_get_cost(pba_engine* e, double* total, int32_t* n_valid) {
  if (!e || !total) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  std::vector<float> c(e->n_blocks);
  std::vector<uint8_t> v(e->n_blocks);
  if (int rc = pba_get_block_costs(e, c.data())) return rc;
  PBA_HIP(hipMemcpy(v.data(), e->valid.p, e->n_blocks, hipMemcpyDeviceToHost));
  double s = 0;
  int nv = 0;
  for (int i = 0; i < e->n_blocks; ++i) {
    s += c[i];
    nv += v[i];
  }
  *total = s;
  if (n_valid) *n_valid = nv;
  return PBA_OK;
}

int pba_device_records(pba_engine* e, float** d_records, uint8_t** d_valid, float** d_costs) {
  if (!e) return fail(PBA_ERR_INVALID_ARGUMENT, "null engine");
  if (d_records) *d_records = e->out.p;
  if (d_valid) *d_valid = e->valid.p;
  if (d_costs) *d_costs = e->cost.p;
  return PBA_OK;
}

int pba_decode_records_device(pba_engine* e, float* d_out) {
  if (!e || !d_out) return fail(PBA_ERR_INVALID_ARGUMENT, "null argument");
  if (!e->evaluated) return fail(PBA_ERR_NOT_READY, "pba_evaluate first");
  if (int rc = check_device(e)) return rc;
  return launch_decode_records(e, d_out);
}

}  // extern "C"
