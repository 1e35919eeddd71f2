// relative_scale_link (pnec_amd/csrc/pnec_relative_scale.hpp), the per-link function of relative_scale_kernel, built for
// the HOST so that its arithmetic can be measured without a GPU (tests/test_relative_scale_cpu.py):
//   hipcc --offload-host-only -O2 -std=c++17 -fPIC -shared -mfma -Iinclude -Ipnec_amd/csrc \
//         tools/relative_scale_link_host.hip -o librs_link_host.so
// The header's functions are __device__; here __device__ is re-defined to host + device after hip_runtime.h has been
// read, and the two rounding intrinsics they call get host overloads that cannot be contracted into an FMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
__host__ inline double __dmul_rn(double a, double b) {
  volatile double r = a * b;
  return r;
}
__host__ inline double __dsub_rn(double a, double b) {
  volatile double r = a - b;
  return r;
}
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "pnec_relative_scale.hpp"

using namespace pnec_hip;

// fc / fp: [n,6] rows (f1 | f2) of the current correspondence and of the one it is linked to, one pose per side
extern "C" void rs_link_host(int64_t n, const double *fc, const double *qc, const double *tc, const double *fp,
                             const double *qp, const double *tp, double sin2_min, int gate_a10, double *ratio,
                             uint8_t *used) {
  double R[9], Rp[9], st, ct, cp, sp;
  pose_setup(qc, tc, R, st, ct, cp, sp);
  const double t[3] = {st * cp, st * sp, ct};
  pose_setup(qp, tp, Rp, st, ct, cp, sp);
  const double t2[3] = {st * cp, st * sp, ct};
  for (int64_t i = 0; i < n; ++i) {
    double f[6], g[6];
    for (int c = 0; c < 6; ++c) {
      f[c] = fc[6 * i + c];
      g[c] = fp[6 * i + c];
    }
    TriSystem cs, rs;
    tri_depths(f, R, t, cs);
    tri_depths(g, Rp, t2, rs);
    double x;
    used[i] = relative_scale_link(cs, rs, sin2_min, gate_a10 != 0, x) ? 1 : 0;
    ratio[i] = x;
  }
}
