// pnec_triangulate.hip -- triangulation of every correspondence at a pose the caller passes in, and the cheirality vote
// that fixes the sign of t.  One pass over the pair's resident SoA planes, a translation unit of its own (the solve /
// stream / front-stage objects do not see it).  pnec_triangulate.hpp has the definitions.
//
// Blocks, wavefronts, the pose, the plane loads and the output offset: pnec_pose_pass.hpp.  The six bearing planes are
// always read, the covariance planes only when the depth variance is wanted (wave-uniform).  Counts are popcounts of
// ballots; the
// parallax sum goes lane by lane, then through the tree of wave_reduce21 for accumulator 0 and the wavefronts' partials
// in wave order: no atomics, a slot's bits depend on its own pair and pose only.
//
// PNEC_HIP_TRI_ORIENT: the per-correspondence outputs are evaluated at t_oriented.  The vote has to be known before
// the first store, so when the flag is set AND a per-correspondence output is wanted, a first sweep over the six bearing
// planes takes the vote (depths only), the block agrees on the sign through LDS, and the second sweep -- the pass
// proper, whose loads now hit L2 -- runs at sign * t.  Every condition on the way to a barrier is uniform over the block.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_triangulate.hpp"

namespace pnec_hip {

template <int MODE>
__global__ __launch_bounds__(kCovMaxWaves *kWave) void triangulate_kernel(const TriangulateArgs a) {
  constexpr int NC = num_components(MODE);
  __shared__ int32_t vote[kCovMaxWaves][2];    // sweep 1: front | back
  __shared__ double part[kCovMaxWaves];        // sweep 2: parallax sum
  __shared__ int32_t parti[kCovMaxWaves][3];   // sweep 2: front | back | left out of the parallax mean

  const PoseSlot g = pose_slot(a.count, a.offsets, a.n_hyp);
  const int64_t s = g.s, ob = g.ob;
  const int lane = g.lane, wave = g.wave, n = g.n, stride = g.stride, W = g.W;
  // load_plane's 32-bit offsets: a 64-bit index per plane costs scalar registers that the output pointers and the
  // constants of the arctangent need
  const char *base = reinterpret_cast<const char *>(a.data + a.block_offset[g.p]);
  const unsigned plane_bytes = (unsigned)stride * 8u;

  // R stays in vector registers (every lane holds the same bits): the scalar file is full with the output pointers,
  // t and the constants of the arctangent, and nine more pairs there are spilled
  double R[9], t[3], st, ct, cp, sp;
  pose_setup(a.q + 4 * s, a.t + 3 * s, R, st, ct, cp, sp);
  st = to_sgpr(st);
  t[0] = to_sgpr(st * cp);   t[1] = to_sgpr(st * sp);   t[2] = to_sgpr(ct);

  const bool per_corr = a.out_point || a.out_depth1 || a.out_depth2 || a.out_parallax || a.out_depth1_var || a.out_front;
  const bool want_var = a.out_depth1_var != nullptr;
  const bool many = blockDim.x > kWave;   // (uniform: the launch's block size)

  // sweep 1: the vote at t as given, when the stores below depend on it
  int nf1 = 0, nb1 = 0;   // block-uniform after the exchange
  const bool two_sweeps = (a.flags & PNEC_HIP_TRI_ORIENT) && per_corr;
  if (two_sweeps) {
    if (wave < W) {
#pragma unroll 1
      for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
        double f[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) f[c] = load_plane(base, plane_bytes, c, i);
        TriSystem ts;
        tri_depths(f, R, t, ts);
        // (a padding slot is all zeros: D = 0, neither front nor back)
        nf1 += __popcll(__builtin_amdgcn_ballot_w64(ts.front));
        nb1 += __popcll(__builtin_amdgcn_ballot_w64(ts.back));
      }
    }
    if (many) {
      if (lane == 0 && wave < W) {
        vote[wave][0] = nf1;
        vote[wave][1] = nb1;
      }
      __syncthreads();
      nf1 = 0;
      nb1 = 0;
      for (int w = 0; w < W; ++w) {
        nf1 += vote[w][0];
        nb1 += vote[w][1];
      }
      nf1 = to_sgpr(nf1);
      nb1 = to_sgpr(nb1);
    }
    if (nf1 < nb1) {   // exact negations: the second sweep's values are those of a call at -t
      t[0] = -t[0];
      t[1] = -t[1];
      t[2] = -t[2];
    }
  }

  // sweep 2, the pass proper, at t (or at the oriented t)
  double psum = 0.0;
  int nf = 0, nb = 0, nout = 0;   // wave-uniform
  if (wave < W) {
#pragma unroll 1
    for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
      double d[NC];
#pragma unroll
      for (int c = 0; c < 6; ++c) d[c] = load_plane(base, plane_bytes, c, i);
#pragma unroll
      for (int c = 6; c < NC; ++c) d[c] = 0.0;
      if (want_var) {
#pragma unroll
        for (int c = 6; c < NC; ++c) d[c] = load_plane(base, plane_bytes, c, i);
      }
      TriCorr o;
      triangulate_corr<MODE>(d, R, t, want_var, o);
      const bool real = i < n;
      const bool skip = o.psi != o.psi;   // a NaN bearing (or a parallax that is no number): not in the mean
      psum += skip ? 0.0 : o.psi;         // (a padding slot has psi exactly 0)
      nf += __popcll(__builtin_amdgcn_ballot_w64(o.front));
      nb += __popcll(__builtin_amdgcn_ballot_w64(o.back));
      nout += __popcll(__builtin_amdgcn_ballot_w64(skip && real));
      if (real && per_corr) {
        const int64_t e = ob + i;
        if (a.out_point) {
          a.out_point[3 * e] = o.px;
          a.out_point[3 * e + 1] = o.py;
          a.out_point[3 * e + 2] = o.pz;
        }
        if (a.out_depth1) a.out_depth1[e] = o.depth1;
        if (a.out_depth2) a.out_depth2[e] = o.depth2;
        if (a.out_parallax) a.out_parallax[e] = o.psi;
        if (a.out_depth1_var) a.out_depth1_var[e] = o.var;
        if (a.out_front) a.out_front[e] = o.front ? 1 : 0;
      }
    }
  }
  double sum_psi = read_lane<0>(wave_reduce_acc0_row0(psum));
  // combine_waves' exchange written out: one double and three counts as one parked struct pad to 24 bytes a wavefront,
  // 32 bytes of LDS more than the two arrays
  if (many) {
    if (lane == 0 && wave > 0 && wave < W) {
      part[wave] = sum_psi;
      parti[wave][0] = nf;
      parti[wave][1] = nb;
      parti[wave][2] = nout;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // the five per-slot pointers are read from the kernel's arguments HERE, through a pointer the compiler cannot see
    // through: read at the top they would sit in ten scalar registers across both sweeps, which the pose, the output
    // pointers of the stores and the constants of the arctangent already fill
    const TriangulateArgs *ka = (const TriangulateArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    int32_t *const o_n_front = ka->out_n_front, *const o_n_back = ka->out_n_back, *const o_sign = ka->out_sign;
    double *const o_t = ka->out_t_oriented, *const o_mean = ka->out_parallax_mean;
    for (int w = 1; w < W; ++w) {
      sum_psi += part[w];
      nf += parti[w][0];
      nb += parti[w][1];
      nout += parti[w][2];
    }
    // the vote is relative to t as given: the first sweep's counts where there was one
    const int n_front = two_sweeps ? nf1 : nf;
    const int n_back = two_sweeps ? nb1 : nb;
    const int sign = n_front >= n_back ? 1 : -1;
    // t[] holds the oriented direction already if the first sweep turned it
    const double sg = (!two_sweeps && sign < 0) ? -1.0 : 1.0;
    if (o_n_front) o_n_front[s] = n_front;
    if (o_n_back) o_n_back[s] = n_back;
    if (o_sign) o_sign[s] = sign;
    if (o_t) {
      o_t[3 * s] = sg * t[0];
      o_t[3 * s + 1] = sg * t[1];
      o_t[3 * s + 2] = sg * t[2];
    }
    if (o_mean) {
      const int m = n - nout;
      o_mean[s] = m > 0 ? sum_psi / (double)m : 0.0;
    }
  }
}

template <int MODE>
struct TriangulateKernel {
  static constexpr auto run = &triangulate_kernel<MODE>;
};

hipError_t launch_triangulate(int mode, int64_t n_slots, int waves, const TriangulateArgs &a, hipStream_t stream) {
  return launch_by_mode<TriangulateKernel>(mode, n_slots, waves, a, stream);
}

}  // namespace pnec_hip
