// pnec_essential_minimal.hpp -- launch interface of the minimal essential-matrix solvers (pnec_essential_minimal.hip),
// shared with the ABI layer.  include/pnec_hip.h (pnec_hip_essential_minimal) has the definitions: the null space of
// A'A by the eight-point's cyclic Jacobi, Nister's ten cubics / the seven-point's cubic, the real roots by a Sturm
// chain, a polish on the constraints themselves, and the eight-point's decomposition and choice once per solution.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pnec_hip {

struct EssentialMinimalArgs {
  const double *data;
  const int64_t *block_offset;
  const int32_t *count;
  int32_t algorithm;           // PNEC_HIP_EM_NISTER / PNEC_HIP_EM_SEVENPT
  int32_t flags;               // PNEC_HIP_EM_QUALITY_ALL
  // per pair; each may be NULL
  double *out_q;               // [P,4] xyzw
  double *out_t;               // [P,3] unit
  double *out_E;               // [P,9] the chosen solution
  double *out_singular;        // [P,3] of the chosen solution
  double *out_gap;             // [P]
  int32_t *out_n_solutions;    // [P]
  double *out_E_all;           // [P,10,9]
  double *out_quality;         // [P,10,4]
  int32_t *out_choice;         // [P]
  int32_t *out_status;         // [P]
};

// one block of one wavefront per pair
hipError_t launch_essential_minimal(int64_t n_pairs, const EssentialMinimalArgs &a, hipStream_t stream);

constexpr int kEmMaxSolutions = 10;
constexpr int kEmSampleNister = 8;     // the reference's sampleSize for NISTER: 5 + 3 (common.cc:352-373)
constexpr int kEmSampleSevenpt = 9;    // for SEVENPT: 7 + 2
constexpr int kEmBisections = 64;      // halvings of the interval between two doubles in their integer order: to one ulp
// Gauss-Newton steps on the ten cubics.  The start is the root of p(z) and the null vector of B(z); where two roots lie
// close together in z (in the basis the Jacobi happened to return: the solutions themselves may be far apart) the
// monomial p(z) places them to 1e-3 .. 5e-2 only, and two steps (the first build) left errors of up to 3e-7 in e on 4 of
// the 138 five-correspondence pairs the population tests compare.  e_(k+1) = C e_k^2 with C about 6 there: five steps
// reach the rounding from 5e-2.
constexpr int kEmPolishNister = 5;
constexpr int kEmPolishSevenpt = 2;    // Newton steps on det(W + aX): a cubic's roots start at one ulp

}  // namespace pnec_hip
