// pnec_relative_scale.hip -- the ratio of a pair's baseline to the previous pair's, from the tracks the two pairs share,
// and three exact order statistics of the ratios (lower quartile, lower median, upper quartile).  A translation unit of
// its own; pnec_relative_scale.hpp has the definitions.
//
// Blocks, wavefronts, the poses and the plane loads: pnec_pose_pass.hpp, with one slot per pair of the current batch.  The
// current pair's six bearing planes are read coalesced; the six bearing values of the linked correspondence are gathered
// from the previous pair's planes (one 8-byte load per plane and lane, not coalesced: the link is a permutation).
//
// Pass 1 stores every ratio (NaN for a link that is not used) to a.ratio -- the caller's out_ratio or the handle's
// workspace -- and counts.  A pair may be of any size, so the selection reads the ratios back from there; a thread reads
// only what it wrote itself (same i), so the block needs no memory fence for them.
//
// Selection: positive finite doubles order as their 64-bit patterns, and every used ratio is one (an unused entry is a
// NaN, whose pattern lies above +inf's).  Eight rounds, most significant byte first.  Per round and rank the block builds
// a 256-bin histogram of the next byte over the candidates whose higher bytes equal the rank's prefix (LDS integer adds:
// the order does not matter to an integer sum; when a wavefront's candidates all have the same byte -- the rule for the
// exponent bytes -- one lane adds the popcount), every wavefront scans it (4 bins per lane, a shuffle prefix sum, a
// ballot) and extends the prefix by the byte whose bin holds the rank.  While the three prefixes are equal the ranks
// share one histogram.  After eight rounds a prefix IS the element of that rank.  Every wavefront reaches every barrier;
// m == 0, the number of histograms and the trip counts are uniform over the block.  No atomics on global memory.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_relative_scale.hpp"

namespace pnec_hip {

constexpr int kRsBins = 256;
constexpr unsigned long long kRsInfBits = 0x7ff0000000000000ull;

// inclusive prefix sum over the wavefront
__device__ __forceinline__ int rs_wave_scan(int x, int lane) {
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int v = __shfl_up(x, off, kWave);
    if (lane >= off) x += v;
  }
  return x;
}

__global__ __launch_bounds__(kCovMaxWaves *kWave) void relative_scale_kernel(const RelativeScaleArgs a) {
  __shared__ int32_t hist[3][kRsBins];
  __shared__ int32_t cnt[kCovMaxWaves][2];   // linked | used

  const PoseSlot slot = pose_slot(a.count, a.offsets, 1);
  const int64_t p = slot.p, e0 = slot.ob;
  const int tid = threadIdx.x;
  const int lane = slot.lane, wave = slot.wave, n = slot.n, stride = slot.stride, W = slot.W;
  // (the ABI layer refuses a batch whose largest pair has 4 GiB of planes or more, on either side)
  const char *base = reinterpret_cast<const char *>(a.data + a.block_offset[p]);
  const unsigned plane_bytes = (unsigned)stride * 8u;

  const int64_t pp = a.prev_pair[p];
  const bool has_prev = pp >= 0 && pp < a.n_prev_pairs;   // uniform over the block
  const int n_prev = has_prev ? a.prev_count[pp] : 0;
  const char *pbase = reinterpret_cast<const char *>(a.prev_data + (has_prev ? a.prev_block_offset[pp] : 0));
  const unsigned pplane_bytes = (unsigned)((n_prev + kWave - 1) & ~(kWave - 1)) * 8u;

  double R[9], t[3], Rp[9], tp[3], st, ct, cp, sp;
  pose_setup(a.q + 4 * p, a.t + 3 * p, R, st, ct, cp, sp);
  t[0] = st * cp;
  t[1] = st * sp;
  t[2] = ct;
  if (has_prev) {
    pose_setup(a.q_prev + 4 * pp, a.t_prev + 3 * pp, Rp, st, ct, cp, sp);
    tp[0] = st * cp;
    tp[1] = st * sp;
    tp[2] = ct;
  } else {   // (nothing is linked: any pose will do)
#pragma unroll
    for (int c = 0; c < 9; ++c) Rp[c] = (c % 4 == 0) ? 1.0 : 0.0;
    tp[0] = 0.0;
    tp[1] = 0.0;
    tp[2] = 1.0;
  }
  const double sin2_min = a.sin2_min;
  const bool gate_a10 = a.gate_a10 != 0;

  // pass 1: the ratios
  int nl = 0, nu = 0;   // wave-uniform
  if (wave < W) {
#pragma unroll 1
    for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
      const bool real = i < n;
      const int j = real ? a.link[e0 + i] : -1;
      const bool linked = real && j >= 0 && j < n_prev;   // (n_prev is 0 without a previous pair)
      double f[6], g[6];
#pragma unroll
      for (int c = 0; c < 6; ++c)
        f[c] = load_plane(base, plane_bytes, c, i);
#pragma unroll
      for (int c = 0; c < 6; ++c) g[c] = 0.0;
      if (linked) {
#pragma unroll
        for (int c = 0; c < 6; ++c)
          g[c] = load_plane(pbase, pplane_bytes, c, j);
      }
      TriSystem cs, rs;
      tri_depths(f, R, t, cs);
      tri_depths(g, Rp, tp, rs);   // (all zeros where not linked: D = 0, not front)
      double ratio;
      const bool used = relative_scale_link(cs, rs, sin2_min, gate_a10, ratio) && linked;
      if (!used) ratio = __builtin_nan("");
      nl += __popcll(__builtin_amdgcn_ballot_w64(linked));
      nu += __popcll(__builtin_amdgcn_ballot_w64(used));
      if (real) {
        a.ratio[e0 + i] = ratio;
        if (a.out_used) a.out_used[e0 + i] = used ? 1 : 0;
      }
    }
  }
  if (lane == 0) {
    cnt[wave][0] = nl;
    cnt[wave][1] = nu;
  }
  __syncthreads();
  int n_linked = 0, m = 0;
  const int waves = (int)(blockDim.x >> 6);
  for (int w = 0; w < waves; ++w) {
    n_linked += cnt[w][0];
    m += cnt[w][1];
  }
  n_linked = to_sgpr(n_linked);
  m = to_sgpr(m);

  // the three ranks ride the same rounds
  unsigned long long pre[3] = {0ull, 0ull, 0ull};
  int k[3] = {(m - 1) / 4, (m - 1) / 2, (int)((3ll * (m - 1)) / 4)};
  if (m > 0) {
#pragma unroll 1
    for (int d = 0; d < 8; ++d) {
      const int sh = 56 - 8 * d;
      const bool shared = pre[0] == pre[1] && pre[1] == pre[2];
      const int nh = shared ? 1 : 3;
      for (int x = tid; x < nh * kRsBins; x += (int)blockDim.x) (&hist[0][0])[x] = 0;
      __syncthreads();
      if (wave < W) {
#pragma unroll 1
        for (int i = wave * kWave + lane; i < stride; i += W * kWave) {
          const unsigned long long key = i < n ? (unsigned long long)__double_as_longlong(a.ratio[e0 + i]) : 0ull;
          const bool valid = key - 1ull < kRsInfBits - 1ull;   // 0 < key < +inf: a used ratio
          const int digit = (int)((key >> sh) & 0xffull);
          const unsigned long long top = (key >> sh) >> 8;      // the bytes above (0 in round 0)
          for (int h = 0; h < nh; ++h) {
            const bool match = valid && top == pre[h];
            const unsigned long long mm = __builtin_amdgcn_ballot_w64(match);
            if (mm != 0ull) {   // wave-uniform
              const int first = __shfl(digit, __builtin_ctzll(mm), kWave);
              const unsigned long long same = __builtin_amdgcn_ballot_w64(match && digit == first);
              if (same == mm) {
                if (lane == 0) atomicAdd(&hist[h][first], (int32_t)__popcll(mm));
              } else if (match) {
                atomicAdd(&hist[h][digit], 1);
              }
            }
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int32_t *hh = hist[shared ? 0 : r];
        const int c0 = hh[4 * lane], c1 = hh[4 * lane + 1], c2 = hh[4 * lane + 2], c3 = hh[4 * lane + 3];
        const int s = c0 + c1 + c2 + c3;
        const int incl = rs_wave_scan(s, lane);
        const unsigned long long over = __builtin_amdgcn_ballot_w64(incl > k[r]);
        // (the candidates of a prefix number more than its rank, so `over` is never empty; 63 keeps a wrong count harmless)
        const int L = over != 0ull ? (int)__builtin_ctzll(over) : kWave - 1;
        int rem = k[r] - __shfl(incl - s, L, kWave);
        const int b0 = __shfl(c0, L, kWave), b1 = __shfl(c1, L, kWave), b2 = __shfl(c2, L, kWave);
        int b = 0;
        if (rem >= b0) {
          rem -= b0;
          b = 1;
          if (rem >= b1) {
            rem -= b1;
            b = 2;
            if (rem >= b2) {
              rem -= b2;
              b = 3;
            }
          }
        }
        pre[r] = (pre[r] << 8) | (unsigned long long)(4 * L + b);
        k[r] = to_sgpr(rem);
      }
      __syncthreads();   // the histograms are zeroed again only after every wavefront has scanned them
    }
  }
  if (tid == 0) {
    if (a.out_n_linked) a.out_n_linked[p] = n_linked;
    if (a.out_n_used) a.out_n_used[p] = m;
    if (a.out_scale) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
        a.out_scale[3 * p + r] = m > 0 ? __longlong_as_double((long long)pre[r]) : __builtin_nan("");
    }
  }
}

hipError_t launch_relative_scale(int64_t n_pairs, int waves, const RelativeScaleArgs &a, hipStream_t stream) {
  const dim3 grid((unsigned)n_pairs), block((unsigned)(waves * kWave));
  hipLaunchKernelGGL(relative_scale_kernel, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
