// pnec_patch_store.hip -- stored patches: a slot per track that keeps the track's templates from the frame it was born
// in (pnec_hip_patch_store_add), and the tracker that reads its templates from there (pnec_hip_patch_track_stored);
// include/pnec_hip.h has the definitions, pnec_patch_store.hpp the layout of a slot and the rules of the assignment.  A
// translation unit of its own.
//
//   assign  one block per image.  The occupancy of the image's C local slots is a bit map in LDS: the carried rows set
//           their bits (an LDS OR: the map does not depend on the order), every lane counts the free bits of its
//           contiguous run of words, one block scan turns the counts into the number of free slots below each word, and
//           the i-th new row finds the i-th free slot by bisection of those numbers and a bit select.  No allocation, no
//           global atomic, nothing read back: the result is a function of the image's rows alone.  The blocks share the
//           padding rows among themselves.
//   build   16 lanes -- one DPP row -- per (row, level), so the levels of a new row run side by side; the template phase
//           of pnec_patch_track_kernel.inl, term by term, then plain stores of the four planes and the header words.  A
//           row of lanes whose (row, level) has nothing to build computes on its own row all the same and stores nothing,
//           so that every DPP move runs with all lanes active; a wavefront none of whose four rows of lanes has anything
//           to build leaves at once.
//   track   the third variant of pnec_patch_track_kernel.inl: the template phase replaced by loads.
#include <hip/hip_runtime.h>

#include "pnec_device.hpp"
#include "pnec_patch_store.hpp"

namespace pnec_hip {

__global__ __launch_bounds__(kStoreAssignBlock) void patch_store_assign_kernel(const PatchStoreAssignArgs a) {
  __shared__ uint32_t occupied[kStoreMapWords];
  __shared__ int32_t before[kStoreMapWords];
  __shared__ int32_t part[kStoreAssignBlock];
  const int t = threadIdx.x;
  const int64_t f = blockIdx.x, C = a.capacity;
  const int n_words = (int)((C + 31) / 32);   // (1 .. kStoreMapWords: the ABI layer has refused any other C)
  int64_t lo, c, take;
  store_counts(a.carried_offsets, a.offsets, a.n_rows, f, lo, c, take);   // (block-uniform)
  for (int w = t; w < n_words; w += kStoreAssignBlock) occupied[w] = 0u;
  __syncthreads();
  for (int64_t r = t; r < take; r += kStoreAssignBlock) {
    const int64_t v = store_local_slot(a.slot[lo + r], f, C);
    if (v >= 0) atomicOr(&occupied[v >> 5], 1u << (int)(v & 31));
  }
  __syncthreads();
  // lane t owns the words [t per, (t + 1) per)
  const int per = (n_words + kStoreAssignBlock - 1) / kStoreAssignBlock;
  const int w0 = t * per < n_words ? t * per : n_words, w1 = w0 + per < n_words ? w0 + per : n_words;
  int32_t mine = 0;
  for (int w = w0; w < w1; ++w) mine += store_popcount(store_free_word(occupied[w], w, C));
  int32_t x = mine;
  part[t] = x;
  __syncthreads();
  for (int s = 1; s < kStoreAssignBlock; s <<= 1) {
    const int32_t o = t >= s ? part[t - s] : 0;
    __syncthreads();
    x += o;
    part[t] = x;
    __syncthreads();
  }
  const int64_t n_free = part[kStoreAssignBlock - 1];
  int32_t run = x - mine;
  for (int w = w0; w < w1; ++w) {
    before[w] = run;
    run += store_popcount(store_free_word(occupied[w], w, C));
  }
  __syncthreads();
  const int64_t n_new = c - take;
  for (int64_t i = t; i < n_new; i += kStoreAssignBlock)
    a.slot[lo + take + i] = i < n_free ? (int32_t)(f * C + store_nth_free(occupied, before, n_words, C, i)) : -1;
  // padding: the rows at and beyond offsets[n_images], shared among the blocks
  int64_t end = a.offsets[a.n_images];
  end = end < 0 ? 0 : end;
  for (int64_t r = end + f * kStoreAssignBlock + t; r < a.n_rows; r += a.n_images * kStoreAssignBlock) a.slot[r] = -1;
}

hipError_t launch_patch_store_assign(const PatchStoreAssignArgs &a, hipStream_t stream) {
  if (a.n_images < 1 || a.n_images > 0x7fffffffLL || a.capacity < 1 || a.capacity > kStoreMaxCapacity)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(patch_store_assign_kernel, dim3((unsigned)a.n_images), dim3(kStoreAssignBlock), 0, stream, a);
  return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(kTrackBlock) void patch_store_build_kernel(const PatchStoreBuildArgs a) {
  PNEC_PATCH_NO_CONTRACT
  const int64_t g = ((int64_t)blockIdx.x * kTrackBlock + threadIdx.x) / kPatchLanes;
  const int j = threadIdx.x & (kPatchLanes - 1);
  const int64_t total = a.n_rows * a.n_levels;   // (>= 1: the ABI layer launches nothing otherwise)
  const bool live = g < total;
  const int64_t gg = live ? g : total - 1;
  const int64_t row = gg / a.n_levels;
  const int l = (int)(gg - row * a.n_levels);
  const int64_t f = tracks_image_of(a.offsets, a.n_images, row);
  int64_t lo, c, take;
  store_counts(a.carried_offsets, a.offsets, a.n_rows, f, lo, c, take);
  const int64_t slot_k = (int64_t)a.slot[row];
  const bool build = live && row >= lo + take && row < lo + c && slot_k >= 0 && slot_k < a.n_slots;
  if (__builtin_amdgcn_ballot_w64(build) == 0ull) return;

  double patx[kPatchSlots], paty[kPatchSlots];
  bool has[kPatchSlots];
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    const int i = j + kPatchLanes * s;
    has[s] = i < a.n_pattern;
    patx[s] = has[s] ? a.pattern[2 * i] : 0.0;
    paty[s] = has[s] ? a.pattern[2 * i + 1] : 0.0;
  }
  const double tpx = a.tmpl_pts[2 * row], tpy = a.tmpl_pts[2 * row + 1];
  const int32_t wl = a.w >> l, hl = a.h >> l;
  const double scale = (double)(1 << l);
  // ---- the template of this level: the template phase of pnec_patch_track_kernel.inl, term by term
  const T *timg = reinterpret_cast<const T *>(a.cur.level[l]) + f * (int64_t)hl * a.cur.pitch[l];
  const int64_t tpitch = a.cur.pitch[l];
  const double qx = tpx / scale, qy = tpy / scale;
  double data[kPatchSlots], K[kPatchSlots][3];
  bool tvalid[kPatchSlots];
  double d[kPatchSlots], gx[kPatchSlots], gy[kPatchSlots];
  double S = 0.0, Gx = 0.0, Gy = 0.0;
  int cnt = 0;
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    tvalid[s] = false;
    d[s] = 0.0;
    gx[s] = 0.0;
    gy[s] = 0.0;
    if (has[s]) tvalid[s] = patch_point(timg, tpitch, wl, hl, qx + patx[s], qy + paty[s], d[s], gx[s], gy[s]);
    S += d[s];
    Gx += gx[s];
    Gy += gy[s];
    cnt += tvalid[s] ? 1 : 0;
  }
  S = row_allreduce_sum(S);
  Gx = row_allreduce_sum(Gx);
  Gy = row_allreduce_sum(Gy);
  const int n = track_row_sum_i(cnt);
  const double nd = (double)n;
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double gpx[kPatchSlots], gpy[kPatchSlots];
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    gpx[s] = tvalid[s] ? patch_normalised_gradient(nd, gx[s], S, Gx, d[s]) : 0.0;
    gpy[s] = tvalid[s] ? patch_normalised_gradient(nd, gy[s], S, Gy, d[s]) : 0.0;
    patch_accumulate(gpx[s], gpy[s], patx[s], paty[s], H);
  }
#pragma unroll
  for (int c6 = 0; c6 < 6; ++c6) H[c6] = row_allreduce_sum(H[c6]);
  double Hi[6];
  const int tstat = patch_inverse3(n, S, H, Hi);
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    data[s] = track_normalised_value(nd, d[s], S);
    track_gain(Hi, gpx[s], gpy[s], patx[s], paty[s], K[s]);
  }
  // the validity of the 64 pattern points as two words of 32 bits: lane j holds bits j and 16 + j of each, and a sum of
  // distinct bits is their union
  const uint32_t v_lo = (uint32_t)track_row_sum_i((int)(((tvalid[0] ? 1u : 0u) << j) | ((tvalid[1] ? 1u : 0u) << (16 + j))));
  const uint32_t v_hi = (uint32_t)track_row_sum_i((int)(((tvalid[2] ? 1u : 0u) << j) | ((tvalid[3] ? 1u : 0u) << (16 + j))));
  if (!build) return;   // (no lane exchange follows)

  double *const words = a.store + slot_k * store_slot_doubles(a.n_levels);
  double *const plane = words + kStoreHeader + l * kStoreLevel;
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    const int i = j + kPatchLanes * s;
    plane[i] = data[s];
    plane[kStorePlane + i] = K[s][0];
    plane[2 * kStorePlane + i] = K[s][1];
    plane[3 * kStorePlane + i] = K[s][2];
  }
  if (j == 0) {
    reinterpret_cast<int64_t *>(words)[kStoreWordStatus + l] = (int64_t)tstat;
    reinterpret_cast<uint64_t *>(words)[kStoreWordValid + l] = ((uint64_t)v_hi << 32) | (uint64_t)v_lo;
  }
  if (l == 0) {
    // the level-0 sums the covariance epilogue needs, and zeros in the words no level owns
    if (j == 0) reinterpret_cast<int64_t *>(words)[kStoreWordN] = (int64_t)n;
    if (j == 1) words[kStoreWordS] = S;
    if (j >= 2 && j < 8) words[j] = j == 2 ? H[0] : (j == 3 ? H[1] : (j == 4 ? H[2] : (j == 5 ? H[3] : (j == 6 ? H[4] : H[5]))));
    if (j >= 8) reinterpret_cast<int64_t *>(words)[kStoreWordZero + (j - 8)] = 0;
    if (j >= a.n_levels && j < PNEC_HIP_TRACK_MAX_LEVELS) {
      reinterpret_cast<int64_t *>(words)[kStoreWordStatus + j] = 0;
      reinterpret_cast<int64_t *>(words)[kStoreWordValid + j] = 0;
    }
  }
}

hipError_t launch_patch_store_build(int pixel_type, const PatchStoreBuildArgs &a, hipStream_t stream) {
  if (a.n_rows < 1 || a.n_levels < 1 || a.n_levels > PNEC_HIP_TRACK_MAX_LEVELS || !a.store || !a.slot || a.n_slots < 1)
    return hipErrorInvalidValue;
  const int64_t blocks = (a.n_rows * a.n_levels * kPatchLanes + kTrackBlock - 1) / kTrackBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block((unsigned)kTrackBlock);
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8: hipLaunchKernelGGL(patch_store_build_kernel<uint8_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_U16: hipLaunchKernelGGL(patch_store_build_kernel<uint16_t>, grid, block, 0, stream, a); break;
    case PNEC_HIP_PIXEL_F32: hipLaunchKernelGGL(patch_store_build_kernel<float>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(kTrackBlock) void patch_track_stored_kernel(const PatchTrackArgs a, const double *store,
                                                                         const int64_t n_slots, const int32_t *slot) {
#define PNEC_TRACK_STORED
#include "pnec_patch_track_kernel.inl"
#undef PNEC_TRACK_STORED
}

hipError_t launch_patch_track_stored(int pixel_type, const PatchTrackArgs &a, const double *store, int64_t n_slots,
                                     const int32_t *slot, hipStream_t stream) {
  const int64_t blocks = (a.n_points * kPatchLanes + kTrackBlock - 1) / kTrackBlock;
  if (blocks > 0x7fffffffLL || !store || !slot || n_slots < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block((unsigned)kTrackBlock);
  switch (pixel_type) {
    case PNEC_HIP_PIXEL_U8:
      hipLaunchKernelGGL(patch_track_stored_kernel<uint8_t>, grid, block, 0, stream, a, store, n_slots, slot);
      break;
    case PNEC_HIP_PIXEL_U16:
      hipLaunchKernelGGL(patch_track_stored_kernel<uint16_t>, grid, block, 0, stream, a, store, n_slots, slot);
      break;
    case PNEC_HIP_PIXEL_F32:
      hipLaunchKernelGGL(patch_track_stored_kernel<float>, grid, block, 0, stream, a, store, n_slots, slot);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace pnec_hip
