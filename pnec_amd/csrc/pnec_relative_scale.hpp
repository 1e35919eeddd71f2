// pnec_relative_scale.hpp -- launch interface of the relative-scale kernel (pnec_relative_scale.hip), shared with the ABI
// layer, and the device function that turns the two midpoint systems of one link into a baseline ratio.
//
// A track seen in frames A, B, C is correspondence j of the previous pair (A, B) and correspondence i of the current pair
// (B, C).  Both reconstructions have a baseline of 1 (t is a direction), and both give the track's distance from the
// shared camera B: depth2 of the previous pair (along u = R f2, from camera 2), depth1 of the current pair (along f1, from
// camera 1).  With r the TriSystem (pnec_triangulate.hpp) of j at the previous pose and c that of i at the current pose
//   ratio = (r.depth2 * sqrt(r.a11)) / (c.depth1 * sqrt(c.a00))       = |baseline_cur| / |baseline_prev|
// (the depths multiply bearings that are not assumed unit; the square roots make both terms metric distances).
//
// A link is USED iff r.front and c.front, both pass the parallax gate, and ratio is a positive finite number.
// Parallax gate: sin^2 psi = D / (a00 a11) against sin^2(min_parallax), written D >= sin2_min * (a00 a11) with D formed
// from two rounded products exactly as tri_depths forms it (no division, no arctangent).  ONLY IF min_parallax > 0 the
// gate also requires a10 > 0: sin^2 does not tell psi from pi - psi, and a parallax of 90 degrees or more is no track.
// With min_parallax = 0 neither test is made.  sin2_min is computed by the ABI layer on the host (2 for
// min_parallax >= pi/2, which no correspondence with a10 > 0 reaches).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnec_device.hpp"
#include "pnec_triangulate.hpp"   // tri_depths / TriSystem; through it pnec_pose_pass.hpp

namespace pnec_hip {

struct RelativeScaleArgs {
  // the current batch
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  const int64_t *offsets;        // [P+1] the batch's correspondence offsets (device)
  // the previous batch (may be the same buffers)
  const double *prev_data;
  const int64_t *prev_block_offset;
  const int32_t *prev_count;
  int64_t n_prev_pairs;
  const int64_t *prev_pair;      // [P]
  const int32_t *link;           // [sum N cur]
  const double *q, *t;           // [P,4], [P,3]
  const double *q_prev, *t_prev; // [n_prev_pairs,4], [n_prev_pairs,3]
  double sin2_min;               // sin^2(min_parallax)
  int32_t gate_a10;              // min_parallax > 0
  double *ratio;                 // [sum N cur] never NULL: the caller's out_ratio or the handle's workspace
  uint8_t *out_used;             // [sum N cur] or NULL
  double *out_scale;             // [P,3] or NULL
  int32_t *out_n_linked;         // [P] or NULL
  int32_t *out_n_used;           // [P] or NULL
};

// one block of `waves` wavefronts per pair of the current batch
hipError_t launch_relative_scale(int64_t n_pairs, int waves, const RelativeScaleArgs &a, hipStream_t stream);

// the parallax gate of one system (see the head of this file)
__device__ __forceinline__ bool rs_parallax_ok(const TriSystem &s, double sin2_min, bool gate_a10) {
  const double a0011 = __dmul_rn(s.a00, s.a11);
  const double D = __dsub_rn(a0011, __dmul_rn(s.a10, s.a10));
  return D >= __dmul_rn(sin2_min, a0011) && (!gate_a10 || s.a10 > 0.0);
}

// One link: c = the correspondence's system in the current pair, r = the linked correspondence's in the previous pair.
// Returns whether the link is used; ratio is NaN when it is not.
__device__ __forceinline__ bool relative_scale_link(const TriSystem &c, const TriSystem &r, double sin2_min, bool gate_a10,
                                                    double &ratio) {
  const double num = r.depth2 * sqrt(r.a11);
  const double den = c.depth1 * sqrt(c.a00);
  const double x = num / den;
  const bool used = c.front && r.front && rs_parallax_ok(c, sin2_min, gate_a10) && rs_parallax_ok(r, sin2_min, gate_a10) &&
                    x > 0.0 && finite_d(x);
  ratio = used ? x : __builtin_nan("");
  return used;
}

}  // namespace pnec_hip
