// pba_joint_plan.h — the host-only plan of the joint solve of poses, inverse distances and brightness (pba_joint.hip):
// which blocks, pairs, points and Schur terms each sum of the reduced system runs over, in a fixed order, and the
// system's profile.  No device code, no engine: plain vectors in, plain vectors out (tests/cpp/joint_plan_check.cpp
// checks it stand-alone, under the sanitizers).
#pragma once

#include <vector>

namespace pba {
namespace detail {

struct JointPlanInput {
  int n_frames = 0, n_pairs = 0, n_points = 0, n_blocks = 0;
  const int* pair_host = nullptr;    // per pair
  const int* pair_target = nullptr;  // per pair
  const int* block_pair = nullptr;   // per block
  const int* block_point = nullptr;  // per block
  const int* point_host = nullptr;   // per point
  // Free intrinsics (pba_joint_set_solve_intrinsics): the cameras are unknowns too.  n_cams = 0: the plan is the
  // keyframes' alone, vector for vector what it was without these two fields.
  int n_cams = 0;
  const int* frame_cam = nullptr;    // per keyframe (read when n_cams > 0)
};

// An ENTRY is one 8-vector W = Σ w J_kfᵀ J_ρ of a point p: e ≥ 0 is block e's target part W_t (its keyframe: the
// block's target), e < 0 the point ~e's host part W_h summed over its blocks (its keyframe: the point's host).  A
// point's entries in order: the host part, then its blocks ascending.
// With n_cams > 0 every block has a third entry, e = n_blocks + b: block b's camera part W_c = Σ w J_intrᵀ J_ρ on block
// row n_frames + cam(target of b).  They come last in the point's order: the host part, the blocks' target parts
// ascending, then the blocks' camera parts ascending.
struct JointTerm {
  int a, b;  // entries of one point: −W_a W_bᵀ / H'_ρρ goes into the block (keyframe of a, keyframe of b)
};

// The reduced system is 8·n_frames square, 8×8 blocks, lower skyline by block rows: row i holds the blocks (i, j),
// first[i] ≤ j ≤ i, at block offsets row[i] + (j − first[i]).  first[i] is the smallest keyframe that shares a point
// with i (as host or target of one of the point's blocks): the pose system's profile (skyline_profile of
// pba_gn_plan.h), with the point elimination's fill and loop closures.
// With n_cams > 0 the system is 8·(n_frames + n_cams) square: camera c is block row n_frames + c with first = 0, a dense
// border under the keyframes' skyline (a camera shares points with most keyframes, so a tighter profile saves little;
// blocks no term reaches are zeros).  The keyframes' rows come first, so their blocks, lists and offsets are those of the
// plan without cameras; first, row, last, colptr, colrows, off_ptr, term_ptr and fe_ptr grow by the cameras' rows.
struct JointPlan {
  std::vector<int> pair_ptr, pair_blocks;    // CSR: the blocks of each pair, ascending
  std::vector<int> frame_ptr, frame_pairs;   // CSR: per keyframe, pair · 2 + role (0: host, 1: target), hosts' pairs
                                             // first, each ascending
  std::vector<int> pt_ptr, pt_blocks;        // CSR: the blocks of each point, ascending
  std::vector<int> first, row, last, colptr, colrows;  // skyline_profile (row has n_frames + 1 entries)
  std::vector<int> off_ptr, off_pairs;       // CSR per skyline block (the diagonal ones stay empty): pair · 2 + t,
                                             // t = 1 when the pair's host is the block's column (H_htᵀ goes in).
                                             // A camera's border block (n_frames + c, keyframe j): the pairs with blocks
                                             // whose target has camera c and that touch j, ascending, as pair · 2 + role
                                             // (0: j is the pair's host, 1: its target); camera × camera blocks: empty
  std::vector<int> cam_ptr, cam_pairs;       // CSR per camera: the pairs with blocks whose target has it, ascending (the
                                             // direct H_cc and g_c); empty vectors when n_cams = 0
  std::vector<int> term_ptr;                 // CSR per skyline block: its Schur terms, points ascending, then a, then b
  std::vector<JointTerm> terms;              //   in the point's entry order (block (i, j): keyframe(a) = i, keyframe(b) = j)
  std::vector<int> fe_ptr, fe_entries;       // CSR per block row (keyframes, then cameras): the entries on it, points
                                             // ascending, a point's in its entry order
  int n_sky = 0;                             // skyline blocks
  int n_sky_kf = 0;                          // … of the keyframes' rows (= n_sky when n_cams = 0)
};

// false when an index is out of range, a block's pair does not have its point's host as host, or a pair's target is
// its host, or a keyframe's camera is out of range (the plan is then unspecified)
bool build_joint_plan(const JointPlanInput& in, JointPlan& P);

// The exchange of the multi-GPU joint solve (pba.h pba_joint_step_export / import): every rank's reduced system goes
// into one banded layout of K block rows, any K with joint_local_band ≤ K ≤ n_frames − 1, and the sum over the ranks is
// factored over the band's own profile.
//   Layout (doubles): per keyframe i, (K + 1) row-major 8×8 blocks, block c = column i − K + c, then a tail of
//   kJointExTail doubles [g_S(8) | g_direct(8) | diag(8) | valid blocks on the keyframe | 0 …]: `stride` per keyframe;
//   after the keyframes kJointExScalars scalar slots at `scalar_off`; `count` in all.
//   src[i·(K + 1) + c]: the local skyline block (its direct and Schur lists are JointPlan's) that fills exchange block
//   (i, c), or −1 where the exchange block is zeros: left of column 0, or outside the local profile.
//   first … colrows, n_sky: the band profile first[i] = max(0, i − K) (skyline_profile), sky_i / sky_j its blocks'
//   keyframes.
constexpr int kJointExTail = 32;
constexpr int kJointExScalars = 16;
struct JointExchangePlan {
  int K = -1, n_sky = 0;
  long long stride = 0, scalar_off = 0, count = 0;
  std::vector<int> src;
  std::vector<int> first, row, last, colptr, colrows, sky_i, sky_j;
};

// the local bandwidth in block rows: max over i of i − first[i]
int joint_local_band(const std::vector<int>& first);
// first, row: a JointPlan's.  false (X unspecified) when K is below the local band or above n_frames − 1.
bool build_joint_exchange(const std::vector<int>& first, const std::vector<int>& row, int K, JointExchangePlan& X);

}  // namespace detail
}  // namespace pba
