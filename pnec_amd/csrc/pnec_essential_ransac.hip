// pnec_essential_ransac.hip -- the RANSAC forms of the essential-matrix baselines: five-point, seven-point and
// eight-point models on random samples, every correspondence scored against every model, opengv's sequential rule.  A
// translation unit of its own.  include/pnec_hip.h has the definitions; this file says how the wavefront is used.
//
// One block of one wavefront per pair, the rule taken literally: one attempt at a time.
//   sample    every lane runs the same draws on wave-uniform values (the hash of seed, pair, attempt, draw), so the S
//             indices live in scalar registers; lane j < S gathers row s_j of the six planes into LDS (six planes of
//             sixteen), where the phases below read the sample as if it were a pair of its own
//   sums      es_sums over the first m rows of the sample; a trace that is not finite ends the attempt here
//   model     em_model / ep_model of pnec_essential_model.hpp: the phases of the two non-RANSAC kernels, the quality of
//             every candidate over all S rows of the sample.  Lane 0 leaves the chosen (R, t, E, singular values) in LDS
//   score     the whole wavefront, 64 rows a step: es_term at the model (R and t by broadcast reads from LDS), a ballot
//             and a population count per step, always in the same order
//   rule      scalar: counters, the best count, k; a new best copies the 24 doubles of the model within LDS
// The pass that writes the mask is the scoring pass once more at the best model -- the same statements in the same loop
// (`last` below), so that the mask's sum cannot differ from the count that won.
// No atomics, plain vector stores; every barrier and every cross-lane operation is reached by the whole wavefront on
// wave-uniform conditions.  Every loop's trip count is wave-uniform: the draws (a function of scalars only), the rows
// (the pair's count), the attempts (each one raises `it` or `skipped`: at most 11 max_iterations + 1).
// Several wavefronts per pair with a round of attempts in flight would finish a pair sooner; one wavefront was chosen
// because its outputs are the sequential rule's by construction and because launches here have far more pairs than the
// chip has SIMDs.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_essential_model.hpp"
#include "pnec_essential_ransac.hpp"
#include "pnec_essential_shared.hpp"
#include "pnec_rng.hpp"

namespace pnec_hip {

namespace {

constexpr int kErModel = 24;   // R (9), t (3), E (9), singular values (3)

// the first S distinct indices min(floor(u n), n - 1), u = rng_uniform of pnec_rng.hpp, n >= S: static indices only,
// as ransac_sample_regs of pnec_frontend.hip
__device__ __forceinline__ void er_sample(unsigned long long seed, unsigned long long pid, unsigned long long attempt,
                                          int n, int S, int (&s)[kErMaxSample]) {
#pragma unroll
  for (int j = 0; j < kErMaxSample; ++j) s[j] = -1;
  int have = 0;
  unsigned long long draw = 0;
  while (have < S) {
    long long idx = (long long)(rng_uniform(seed, pid, attempt, draw++) * (double)n);
    if (idx >= n) idx = n - 1;
    const int id = to_sgpr((int)idx);
    bool dup = false;
#pragma unroll
    for (int j = 0; j < kErMaxSample; ++j) dup = dup || s[j] == id;   // (entries from `have` on are -1, id >= 0)
    if (!dup) {
#pragma unroll
      for (int j = 0; j < kErMaxSample; ++j) s[j] = (j == have) ? id : s[j];
      ++have;
    }
  }
}
// w^S by squaring, as the eigensolver RANSAC's pow_sample
__device__ __forceinline__ double er_pow(double w, int S) {
  double r = 1.0, b = w;
  for (int e = S; e > 0; e >>= 1) {
    if (e & 1) r *= b;
    b *= b;
  }
  return r;
}

}  // namespace

template <bool EIGHT>
__global__ __launch_bounds__(kWave) void essential_ransac_kernel(const EssentialRansacArgs a) {
  __shared__ double M[kEsRows * kEsDim];                           // A'A on top of its eigenvectors
  __shared__ double T[EIGHT ? 1 : 10 * 20];                        // em_model's arrays
  __shared__ double St[EIGHT ? 1 : 11 * 11];
  __shared__ double Es[EIGHT ? 1 : kEmMaxSolutions * 9];
  __shared__ double C[EIGHT ? 1 : kEmMaxSolutions * model::kCand];
  __shared__ double Rw[6 * kErRowStride];                          // the sample's rows, plane c at Rw[16 c]
  __shared__ double Cur[kErModel], Best[kErModel];                 // the attempt's model, the best one

  const int64_t pair = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = to_sgpr(a.count[pair]);
  const bool nister = a.algorithm == PNEC_HIP_EM_NISTER;
  const int m = EIGHT ? 8 : (nister ? 5 : 7);
  const int S = EIGHT ? kEpSample : (nister ? kEmSampleNister : kEmSampleSevenpt);
  const EsPair pr = {a.data + a.block_offset[pair], ((int64_t)n + kWave - 1) & ~(int64_t)(kWave - 1)};
  const EsPair sp = {Rw, kErRowStride};
  const unsigned long long pid = a.first_pair_id + (unsigned long long)pair;
  const int64_t aos0 = a.offsets[pair];
  const long long skip_limit = (long long)kErSkipFactor * a.max_iterations;
  const bool too_few = n < S;

  int it = 0, attempts = 0, best = -1, best_attempt = -1, count = 0;
  long long skipped = 0;
  double k = 1.0;
  bool stop = too_few;
  for (;;) {
    // `last`: the rule has ended, what remains is the mask at the best model
    const bool last = stop || !((double)it < k && skipped < skip_limit);
    if (last && best < 0) break;
    if (last && !a.out_inlier_mask) {   // nobody wants the mask: its sum is the count that won
      count = best;
      break;
    }
    __syncthreads();   // whatever the round before read from LDS has been read
    if (!last) {
      const unsigned long long attempt = (unsigned long long)attempts;
      ++attempts;
      int s[kErMaxSample];
      er_sample(a.seed, pid, attempt, n, S, s);
      {
        int mine = s[0];
#pragma unroll
        for (int j = 1; j < kErMaxSample; ++j) mine = lane == j ? s[j] : mine;
        if (lane < S) {
          double f[6];
          pr.load6(mine, f);
#pragma unroll
          for (int c = 0; c < 6; ++c) Rw[c * kErRowStride + lane] = f[c];
        }
      }
      __syncthreads();
      const double trace = es_sums(sp, m, lane, M);
      __syncthreads();
      bool have = finite_d(trace);
      if (have) {
        if constexpr (EIGHT) {
          int choice;
          double gap, quality[4], E[9], sing[3], Rc[9], tc[3];
          have = model::ep_model(sp, S, false, lane, M, trace, gap, choice, quality, E, sing, Rc, tc) == PNEC_HIP_EP_OK;
          if (have && lane == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) {
              Cur[j] = Rc[j];
              Cur[12 + j] = E[j];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              Cur[9 + j] = tc[j];
              Cur[21 + j] = sing[j];
            }
          }
        } else {
          const model::EmLds L = {M, T, St, Es, C};
          int n_sol, choice;
          double gap, quality, e[9];
          have = model::em_model(sp, S, nister, lane, L, trace, n_sol, gap, choice, quality, e) == PNEC_HIP_EM_OK;
          if (have && lane == 0) {
            double Rc[9], tc[3], Ec[9], sing[3];
            model::em_chosen(L, choice, Rc, tc, Ec, sing);
#pragma unroll
            for (int j = 0; j < 9; ++j) {
              Cur[j] = Rc[j];
              Cur[12 + j] = Ec[j];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              Cur[9 + j] = tc[j];
              Cur[21 + j] = sing[j];
            }
          }
        }
      }
      if (!have) {   // opengv's skip: no model, not an iteration
        ++skipped;
        continue;
      }
      __syncthreads();
    }

    // ---- the score of every row at the model; the last pass writes the mask ---------------------------------------------------
    const double *const src = last ? Best : Cur;
    double R[9], t[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = src[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = src[9 + j];
    int c = 0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += kWave) {
      const int i = i0 + lane;
      const bool in = i < n;
      double f[6];
      pr.load6(in ? i : n - 1, f);
      const bool inlier = in && es_term(f, R, t) < a.threshold;   // (a score that is not finite compares false)
      c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(inlier));
      if (last && a.out_inlier_mask && in) a.out_inlier_mask[aos0 + i] = inlier ? 1 : 0;
    }
    if (last) {
      count = c;
      break;
    }

    // ---- opengv::sac::Ransac::computeModel's bookkeeping ------------------------------------------------------------------------
    if (c > best) {
      best = c;
      best_attempt = attempts - 1;
      const double w = (double)c / (double)n;
      double p_no = 1.0 - er_pow(w, S);
      p_no = fmax(0x1p-52, p_no);
      p_no = fmin(1.0 - 0x1p-52, p_no);
      k = log(1.0 - kErProbability) / log(p_no);
      if (lane < kErModel) Best[lane] = Cur[lane];   // (read by the last pass, behind the barrier at the loop's head)
    }
    ++it;
    if (it > a.max_iterations) stop = true;
  }

  // ---- the outputs -------------------------------------------------------------------------------------------------------------
  const bool ok = best >= 0;
  if (!ok && a.out_inlier_mask) {
    for (int i = lane; i < n; i += kWave) a.out_inlier_mask[aos0 + i] = 0;
  }
  if (lane == 0) {
    const double nan = __builtin_nan("");
    double mdl[kErModel];
#pragma unroll
    for (int j = 0; j < kErModel; ++j) mdl[j] = ok ? Best[j] : nan;
    if (a.out_q) {
      double q[4] = {nan, nan, nan, nan};
      if (ok) {
        const double Rc[9] = {mdl[0], mdl[1], mdl[2], mdl[3], mdl[4], mdl[5], mdl[6], mdl[7], mdl[8]};
        es_quat(Rc, q);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) a.out_q[4 * pair + j] = q[j];
    }
    if (a.out_t) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.out_t[3 * pair + j] = mdl[9 + j];
    }
    if (a.out_E) {
#pragma unroll
      for (int j = 0; j < 9; ++j) a.out_E[9 * pair + j] = mdl[12 + j];
    }
    if (a.out_singular) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.out_singular[3 * pair + j] = mdl[21 + j];
    }
    if (a.out_inlier_count) a.out_inlier_count[pair] = ok ? count : 0;
    if (a.out_iterations) a.out_iterations[pair] = it;
    if (a.out_attempts) a.out_attempts[pair] = attempts;
    if (a.out_best_attempt) a.out_best_attempt[pair] = best_attempt;
    if (a.out_status) a.out_status[pair] = too_few ? PNEC_HIP_ER_TOO_FEW : (ok ? PNEC_HIP_ER_OK : PNEC_HIP_ER_NO_MODEL);
  }
}

hipError_t launch_essential_ransac(int64_t n_pairs, const EssentialRansacArgs &a, hipStream_t stream) {
  if (a.algorithm == PNEC_HIP_EM_EIGHTPT)
    hipLaunchKernelGGL(essential_ransac_kernel<true>, dim3((unsigned)n_pairs), dim3(kWave), 0, stream, a);
  else
    hipLaunchKernelGGL(essential_ransac_kernel<false>, dim3((unsigned)n_pairs), dim3(kWave), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
