// pnec_detect.hip -- keypoint detection: grid FAST-9 corners, up to four per cell (pnec_hip_detect_keypoints;
// include/pnec_hip.h has the definition, pnec_detect.hpp the arithmetic).  A translation unit of its own.
//
// Six steps in stream order, no allocation, no atomics, nothing read back:
//   mark    out_cell <- 0, then one lane per current point stores -1 into its cell (every writer stores the same value).
//   search  one wavefront per (image, cell), four per block.  The cell's G x G bytes go to LDS (row loads; the high byte of
//           a 16-bit pixel), lanes stride over the (G-6)^2 interior pixels and write m into a second byte map, then test
//           the 3 x 3 strict maximum and the bounds rule and keep their four best keys sorted in registers; K rounds of a
//           wavefront-wide maximum pick the winners, the winner's lane drops its key each round.  out_cell <- the count
//           packed with the best key (detect_pack).  Occupied cells do nothing.
//   count   one wavefront per image sums the counts of its cells into out_offsets[f + 1].
//   scan    one block turns out_offsets into the exclusive scan over images.
//   emit    one wavefront per (image, cell) with points: its position is out_offsets[f] plus the counts of the image's
//           cells before it; a cell with one point is unpacked, a cell with more is searched again.  Plain stores to the
//           final position: nothing beyond out_offsets[n_images] is touched.
//   finish  out_cell <- the count.
// Why emit searches again for K > 1 instead of reading fixed slots: the caller's arrays must stay untouched beyond
// out_offsets[n_images], which is not known before the scan, and a DEVICE-space call may neither allocate nor wait -- so
// there is no place for [image, cell, rank] slots.  One key fits beside the count in out_cell's 32 bits, four do not.
//
// Every cross-lane move and every barrier runs with all lanes of all four wavefronts active: a wavefront without work
// (past the last cell, occupied, empty) keeps walking with `active` false.  LDS holds nothing outside the wavefront's
// own two maps; __syncthreads orders a wavefront's LDS writes before its other lanes' reads.
#include <hip/hip_runtime.h>

#include "pnec_detect.hpp"

namespace pnec_hip {

constexpr int kDetectWaves = 4;
constexpr int kDetectBlock = kDetectWaves * kDetectLanes;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)x, s, kDetectLanes);
    x = o > x ? o : x;
  }
  return x;
}

__device__ __forceinline__ int wave_sum_i32(int x) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, kDetectLanes);
  return x;
}

__device__ __forceinline__ int map_bytes(int grid) { return (grid * grid + 15) & ~15; }

// The search of one cell by one wavefront.  Called by every wavefront of the block (it holds barriers); `active` false
// does no memory access.  win[r] is the key of rank r or 0, the same in every lane.
template <typename T>
__device__ __forceinline__ void search_cell(const DetectArgs &a, bool active, int64_t f, int c, uint8_t *cell,
                                            uint8_t *mm, uint32_t (&win)[kDetectMaxPerCell]) {
  const int lane = threadIdx.x & (kDetectLanes - 1);
  const int G = a.grid, GG = G * G, GI = G - 2 * kDetectBorder, GII = GI * GI;
  const uint32_t inv = detect_inverse(G), inv_i = detect_inverse(GI);
  const int cx = c / a.ny, cy = c - cx * a.ny;
  const int X0 = a.x_start + cx * G, Y0 = a.y_start + cy * G;
  if (active) {
    const T *img = reinterpret_cast<const T *>(a.images) + (f * (int64_t)a.h + Y0) * a.pitch + X0;
    for (int i = lane; i < GG; i += kDetectLanes) {
      const int y = detect_div(i, inv), x = i - y * G;
      cell[i] = detect_pixel(img[(int64_t)y * a.pitch + x]);
      mm[i] = 0;
    }
  }
  __syncthreads();
  if (active) {
    for (int j = lane; j < GII; j += kDetectLanes) {
      const int yy = detect_div(j, inv_i);
      const int idx = (yy + kDetectBorder) * G + (j - yy * GI) + kDetectBorder;
      mm[idx] = (uint8_t)detect_measure(cell + idx, G, a.thr);
    }
  }
  __syncthreads();
  uint32_t k[4] = {0u, 0u, 0u, 0u};
  if (active) {
    for (int j = lane; j < GII; j += kDetectLanes) {
      const int yy = detect_div(j, inv_i), xx = j - yy * GI;
      const int y = yy + kDetectBorder, x = xx + kDetectBorder, idx = y * G + x;
      if (detect_is_peak(mm, idx, G, a.thr) && detect_in_bounds(X0 + x, Y0 + y, a.w, a.h, a.edge))
        detect_insert(detect_key(mm[idx], idx), k);
    }
  }
#pragma unroll
  for (int r = 0; r < kDetectMaxPerCell; ++r) {
    win[r] = 0u;
    if (r < a.per_cell) {   // (uniform)
      const uint32_t best = wave_max_u32(k[0]);
      win[r] = best;
      if (best != 0u && k[0] == best) {   // keys are distinct: one lane
        k[0] = k[1];
        k[1] = k[2];
        k[2] = k[3];
        k[3] = 0u;
      }
    }
  }
  __syncthreads();   // (the maps may be written again by a later call in the same kernel: none today)
}

__global__ __launch_bounds__(256) void detect_mark_kernel(const DetectArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_cur) return;
  // the image of point i: the last f in [0, F-1] with cur_offsets[f] <= i (clamped to the images there are)
  int64_t lo = 0, hi = a.n_images - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (a.cur_offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int c = detect_point_cell(a.cur_pts[2 * i], a.cur_pts[2 * i + 1], a.x_start, a.y_start, a.nx, a.ny, a.grid);
  if (c >= 0) a.out_cell[lo * ((int64_t)a.nx * a.ny) + c] = -1;
}

template <typename T>
__global__ __launch_bounds__(kDetectBlock) void detect_search_kernel(const DetectArgs a, const int marked) {
  extern __shared__ uint8_t lds[];
  const int wave = threadIdx.x / kDetectLanes, lane = threadIdx.x & (kDetectLanes - 1);
  const int n_cells = a.nx * a.ny;
  const int64_t u = (int64_t)blockIdx.x * kDetectWaves + wave, n_units = a.n_images * n_cells;
  const bool inside = u < n_units;
  const int64_t f = inside ? u / n_cells : 0;
  const int c = inside ? (int)(u - f * n_cells) : 0;
  const bool active = inside && !(marked && a.out_cell[u] < 0);
  uint8_t *cell = lds + wave * 2 * map_bytes(a.grid), *mm = cell + map_bytes(a.grid);
  uint32_t win[kDetectMaxPerCell];
  search_cell<T>(a, active, f, c, cell, mm, win);
  int count = 0;
#pragma unroll
  for (int r = 0; r < kDetectMaxPerCell; ++r) count += win[r] != 0u ? 1 : 0;
  if (active && lane == 0) a.out_cell[u] = detect_pack(count, win[0]);
}

__global__ __launch_bounds__(kDetectBlock) void detect_count_kernel(const DetectArgs a) {
  const int wave = threadIdx.x / kDetectLanes, lane = threadIdx.x & (kDetectLanes - 1);
  const int n_cells = a.nx * a.ny;
  const int64_t f = (int64_t)blockIdx.x * kDetectWaves + wave;
  const bool inside = f < a.n_images;
  int sum = 0;
  if (inside)
    for (int c = lane; c < n_cells; c += kDetectLanes) sum += detect_packed_count(a.out_cell[f * n_cells + c]);
  sum = wave_sum_i32(sum);
  if (inside && lane == 0) a.out_offsets[f + 1] = sum;
}

// out_offsets[1 .. F] hold the images' counts: the running sum in place, 256 images at a time, and out_offsets[0] = 0
__global__ __launch_bounds__(256) void detect_scan_kernel(const DetectArgs a) {
  __shared__ int64_t part[256];
  int64_t carry = 0;
  for (int64_t base = 0; base < a.n_images; base += 256) {
    const int64_t f = base + threadIdx.x;
    int64_t v = f < a.n_images ? a.out_offsets[f + 1] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      const int64_t o = (int)threadIdx.x >= s ? part[threadIdx.x - s] : 0;
      __syncthreads();
      v += o;
      part[threadIdx.x] = v;
      __syncthreads();
    }
    if (f < a.n_images) a.out_offsets[f + 1] = carry + v;
    carry += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.out_offsets[0] = 0;
}

template <typename T>
__global__ __launch_bounds__(kDetectBlock) void detect_emit_kernel(const DetectArgs a) {
  extern __shared__ uint8_t lds[];
  const int wave = threadIdx.x / kDetectLanes, lane = threadIdx.x & (kDetectLanes - 1);
  const int n_cells = a.nx * a.ny;
  const int64_t u = (int64_t)blockIdx.x * kDetectWaves + wave, n_units = a.n_images * n_cells;
  const bool inside = u < n_units;
  const int64_t f = inside ? u / n_cells : 0;
  const int c = inside ? (int)(u - f * n_cells) : 0;
  const int32_t packed = inside ? a.out_cell[u] : 0;
  const int count = detect_packed_count(packed);
  // the points of the image's cells before this one
  int before = 0;
  if (count > 0)
    for (int i = lane; i < c; i += kDetectLanes) before += detect_packed_count(a.out_cell[f * n_cells + i]);
  before = wave_sum_i32(before);
  uint32_t win[kDetectMaxPerCell] = {detect_packed_key(packed), 0u, 0u, 0u};
  const bool again = count > 1;
  if (__syncthreads_or(again ? 1 : 0)) {   // (block-uniform: search_cell holds barriers)
    uint8_t *cell = lds + wave * 2 * map_bytes(a.grid), *mm = cell + map_bytes(a.grid);
    uint32_t w2[kDetectMaxPerCell];
    search_cell<T>(a, again, f, c, cell, mm, w2);
    if (again) {
#pragma unroll
      for (int r = 0; r < kDetectMaxPerCell; ++r) win[r] = w2[r];
    }
  }
  if (lane < count) {   // count <= 4: lane r stores rank r
    const uint32_t key = lane == 0 ? win[0] : (lane == 1 ? win[1] : (lane == 2 ? win[2] : win[3]));
    const int idx = detect_key_index(key);
    const int y = detect_div(idx, detect_inverse(a.grid)), x = idx - y * a.grid;
    const int cx = c / a.ny, cy = c - cx * a.ny;
    const int64_t at = a.out_offsets[f] + before + lane;
    a.out_pts[2 * at] = (double)(a.x_start + cx * a.grid + x);
    a.out_pts[2 * at + 1] = (double)(a.y_start + cy * a.grid + y);
    if (a.out_score) a.out_score[at] = detect_key_m(key) - 1;
    if (a.out_cell_index) a.out_cell_index[at] = c;
  }
}

__global__ __launch_bounds__(256) void detect_finish_kernel(const DetectArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_images * ((int64_t)a.nx * a.ny)) return;
  const int32_t v = a.out_cell[i];
  if (v > 0) a.out_cell[i] = detect_packed_count(v);
}

hipError_t launch_detect_keypoints(int pixel_type, const DetectArgs &a, hipStream_t stream) {
  const int64_t n_units = a.n_images * ((int64_t)a.nx * a.ny);
  const int64_t unit_blocks = (n_units + kDetectWaves - 1) / kDetectWaves, flat_blocks = (n_units + 255) / 256;
  const int64_t image_blocks = (a.n_images + kDetectWaves - 1) / kDetectWaves, cur_blocks = (a.n_cur + 255) / 256;
  if (unit_blocks > 0x7fffffffLL || cur_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (pixel_type != PNEC_HIP_PIXEL_U8 && pixel_type != PNEC_HIP_PIXEL_U16) return hipErrorInvalidValue;
  const int marked = a.cur_offsets && a.cur_pts && a.n_cur > 0 ? 1 : 0;
  const size_t lds_bytes = (size_t)kDetectWaves * 2 * (size_t)((a.grid * a.grid + 15) & ~15);
  const dim3 units((unsigned)unit_blocks), wide((unsigned)kDetectBlock);
  if (marked) {
    hipError_t e = hipMemsetAsync(a.out_cell, 0, sizeof(int32_t) * (size_t)n_units, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(detect_mark_kernel, dim3((unsigned)cur_blocks), dim3(256), 0, stream, a);
  }
  if (pixel_type == PNEC_HIP_PIXEL_U8)
    hipLaunchKernelGGL(detect_search_kernel<uint8_t>, units, wide, lds_bytes, stream, a, marked);
  else
    hipLaunchKernelGGL(detect_search_kernel<uint16_t>, units, wide, lds_bytes, stream, a, marked);
  hipLaunchKernelGGL(detect_count_kernel, dim3((unsigned)image_blocks), wide, 0, stream, a);
  hipLaunchKernelGGL(detect_scan_kernel, dim3(1), dim3(256), 0, stream, a);
  if (pixel_type == PNEC_HIP_PIXEL_U8)
    hipLaunchKernelGGL(detect_emit_kernel<uint8_t>, units, wide, lds_bytes, stream, a);
  else
    hipLaunchKernelGGL(detect_emit_kernel<uint16_t>, units, wide, lds_bytes, stream, a);
  hipLaunchKernelGGL(detect_finish_kernel, dim3((unsigned)flat_blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace pnec_hip
