// pba_gn_intr.h — the free-intrinsics stage of a Gauss-Newton trial (pba_gn_intr.hip) as pba_gn.hip sees it: its buffers
// and its launches.  Everything else of the stage (the row layout kIb*, kCamSplit, the kernels) is private to that unit.
#pragma once

#include "pba_internal.h"

namespace pba {
namespace detail {

// gn_prepare, nc_sys > 0: sizes the stage's buffers (rows, point sums, camera partials, candidate intrinsics) for the
// prepared problem (n_gn_points, nc_sys) and starts the candidate intrinsics as copies of the state.
int intr_prepare_buffers(pba_engine* e);

// The candidate intrinsics become the state, gated by the LM record lm (nullptr: always).
void launch_intr_accept(pba_engine* e, const double* lm);

// The last trial's accept (lm: the LM record, else none; accept = false: the point elimination's launch has applied
// it), then the blocks' contributions at the state: the weighted fp64 rows of a geometric engine, the moment records of a
// photometric one (intr_rows_photometric_kernel).
void enqueue_intr_rows(pba_engine* e, const double* lm, bool accept = true);

// The border rows of the reduced system into the skyline S — or, X ≠ nullptr, this rank's undamped border into the
// exchange buffer's border region (X points at it).
// arrow: the local solve is an arrow (arrow_solve follows with built = true): its level 0 is built in the same launch as
// the camera blocks.
void enqueue_border(pba_engine* e, double lambda, const double* lm, double* X, bool arrow = false);

}  // namespace detail
}  // namespace pba
