// pnec_detect.hpp -- keypoint detection (pnec_hip_detect_keypoints): launch interface of pnec_detect.hip, shared with the
// ABI layer, and the integer arithmetic of the detector -- the cell grid, the FAST-9 corner measure on a cell held as
// G x G bytes, the 3 x 3 strict maximum, the bounds rule, the selection key and its sorted insertion -- written so that it
// also compiles for the host (tools/detect_host.cc runs it under the address sanitizer on images and cells without slack
// before any device does).  include/pnec_hip.h has the definition.
#pragma once

#include <cstdint>

#include "pnec_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNEC_DETECT_HD __host__ __device__ __forceinline__
#else
#define PNEC_DETECT_HD inline
#endif

namespace pnec_hip {

constexpr int kDetectMinGrid = 8, kDetectMaxGrid = 64, kDetectMaxPerCell = 4, kDetectMaxThreshold = 254;
constexpr int kDetectBorder = 3;   // the ring's radius: pixels this close to a cell's border are never corners
constexpr int kDetectLanes = 64;   // one wavefront per (image, cell)

// i / d for 0 <= i < 4096 and 2 <= d <= 64 without a division: (i * inv) >> 20 with inv = ceil(2^20 / d).  The error of
// the product is below i / 2^20 < 1 / 256 < 1 / d, so the floor is exact (tools/detect_host.cc checks every pair).
PNEC_DETECT_HD uint32_t detect_inverse(int d) { return ((1u << 20) + (uint32_t)d - 1u) / (uint32_t)d; }
PNEC_DETECT_HD int detect_div(int i, uint32_t inv) { return (int)(((uint32_t)i * inv) >> 20); }

// the 8-bit value of a pixel: U8 as it is, U16 by its high byte (the reference's quantisation of its 16-bit pyramid)
PNEC_DETECT_HD uint8_t detect_pixel(uint8_t v) { return v; }
PNEC_DETECT_HD uint8_t detect_pixel(uint16_t v) { return (uint8_t)(v >> 8); }

// The cell a current point marks: cx * ny + cy, or -1 when it lies outside the grid (or is NaN: every comparison with a
// NaN is false).  Inside, the quotient is below nx: (nx G - ulp) / G is further from nx than half a unit in its last place.
PNEC_DETECT_HD int detect_point_cell(double px, double py, int x_start, int y_start, int nx, int ny, int grid) {
  const double x0 = (double)x_start, y0 = (double)y_start, g = (double)grid;
  if (!(px >= x0 && px < x0 + (double)nx * g && py >= y0 && py < y0 + (double)ny * g)) return -1;
  int cx = (int)((px - x0) / g), cy = (int)((py - y0) / g);
  cx = cx > nx - 1 ? nx - 1 : cx;   // (never taken; keeps the store inside out_cell whatever the rounding)
  cy = cy > ny - 1 ? ny - 1 : cy;
  return cx * ny + cy;
}

// m(p) of the pixel at `p` inside a cell stored with `grid` bytes per row; p is at least 3 pixels from every border of
// the cell.  Returns 0 instead of m when both |I_0 - I| and |I_8 - I| are <= thr: every arc of 9 holds ring pixel 0 or
// 8, so then m <= thr, the pixel is no candidate, and as a neighbour it loses against every candidate (whose m > thr)
// either way.  The minimum over 9 contiguous ring pixels is built by doubling: windows of 2, 4, 8, then one more.
PNEC_DETECT_HD int detect_measure(const uint8_t *p, int grid, int thr) {
  const int I = p[0];
  const int d0 = (int)p[-3 * grid] - I, d8 = (int)p[3 * grid] - I;
  if ((d0 < 0 ? -d0 : d0) <= thr && (d8 < 0 ? -d8 : d8) <= thr) return 0;
  int d[16];
  d[0] = d0;
  d[1] = (int)p[-3 * grid + 1] - I;
  d[2] = (int)p[-2 * grid + 2] - I;
  d[3] = (int)p[-grid + 3] - I;
  d[4] = (int)p[3] - I;
  d[5] = (int)p[grid + 3] - I;
  d[6] = (int)p[2 * grid + 2] - I;
  d[7] = (int)p[3 * grid + 1] - I;
  d[8] = d8;
  d[9] = (int)p[3 * grid - 1] - I;
  d[10] = (int)p[2 * grid - 2] - I;
  d[11] = (int)p[grid - 3] - I;
  d[12] = (int)p[-3] - I;
  d[13] = (int)p[-grid - 3] - I;
  d[14] = (int)p[-2 * grid - 2] - I;
  d[15] = (int)p[-grid * 3 - 1] - I;
  int lo2[16], hi2[16], lo4[16], hi4[16];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 16; ++k) {
    const int a = d[k], b = d[(k + 1) & 15];
    lo2[k] = a < b ? a : b;
    hi2[k] = a > b ? a : b;
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 16; ++k) {
    const int a = lo2[k], b = lo2[(k + 2) & 15], c = hi2[k], e = hi2[(k + 2) & 15];
    lo4[k] = a < b ? a : b;
    hi4[k] = c > e ? c : e;
  }
  int m = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 16; ++k) {
    int lo = lo4[k] < lo4[(k + 4) & 15] ? lo4[k] : lo4[(k + 4) & 15];   // min of d[k .. k+7]
    int hi = hi4[k] > hi4[(k + 4) & 15] ? hi4[k] : hi4[(k + 4) & 15];   // max of d[k .. k+7]
    const int last = d[(k + 8) & 15];
    lo = lo < last ? lo : last;   // brighter arc: min (I_k - I)
    hi = hi > last ? hi : last;   // darker arc: min (I - I_k) = -max (I_k - I)
    m = lo > m ? lo : m;
    m = -hi > m ? -hi : m;
  }
  return m;
}

// Is the interior pixel at raster index idx of the cell's measure map a strict 3 x 3 maximum above thr?
PNEC_DETECT_HD bool detect_is_peak(const uint8_t *mm, int idx, int grid, int thr) {
  const int m = mm[idx];
  if (m <= thr) return false;
  return m > mm[idx - grid - 1] && m > mm[idx - grid] && m > mm[idx - grid + 1] && m > mm[idx - 1] && m > mm[idx + 1] &&
         m > mm[idx + grid - 1] && m > mm[idx + grid] && m > mm[idx + grid + 1];
}

// basalt's InBounds on the image position
PNEC_DETECT_HD bool detect_in_bounds(int x, int y, int w, int h, int edge) {
  return x >= edge && x < w - edge - 1 && y >= edge && y < h - edge - 1;
}

// The selection key of a candidate: larger m first, then the smaller raster index (ascending y, then x).  m >= 1, so a
// key is never 0, which stands for "none".  grid <= 64 keeps the raster index inside 12 bits.
PNEC_DETECT_HD uint32_t detect_key(int m, int idx) { return ((uint32_t)m << 12) | (uint32_t)(4095 - idx); }
PNEC_DETECT_HD int detect_key_m(uint32_t key) { return (int)(key >> 12); }
PNEC_DETECT_HD int detect_key_index(uint32_t key) { return 4095 - (int)(key & 4095u); }

// keeps the four largest keys, k[0] >= k[1] >= k[2] >= k[3]
PNEC_DETECT_HD void detect_insert(uint32_t key, uint32_t (&k)[4]) {
  if (key <= k[3]) return;
  k[3] = key;
  if (k[3] > k[2]) { const uint32_t t = k[2]; k[2] = k[3]; k[3] = t; }
  if (k[2] > k[1]) { const uint32_t t = k[1]; k[1] = k[2]; k[2] = t; }
  if (k[1] > k[0]) { const uint32_t t = k[0]; k[0] = k[1]; k[1] = t; }
}

// What the first pass leaves in out_cell for a searched cell until the last kernel replaces it with the count: the
// count in the low three bits and the best key above them (20 bits), so a cell with one point is emitted without being
// searched again.  0 is an empty cell, -1 an occupied one, before and after.
PNEC_DETECT_HD int32_t detect_pack(int count, uint32_t best) { return count > 0 ? (int32_t)((best << 3) | (uint32_t)count) : 0; }
PNEC_DETECT_HD int detect_packed_count(int32_t v) { return v > 0 ? (v & 7) : 0; }
PNEC_DETECT_HD uint32_t detect_packed_key(int32_t v) { return (uint32_t)v >> 3; }

struct DetectArgs {
  const void *images;
  int32_t w, h;
  int64_t pitch, n_images;
  int32_t grid, per_cell, thr, edge;
  int32_t nx, ny, x_start, y_start;
  const int64_t *cur_offsets;
  const double *cur_pts;
  int64_t n_cur;
  int32_t *out_cell;
  int64_t *out_offsets;
  double *out_pts;
  int32_t *out_score, *out_cell_index;
};

#if defined(__HIPCC__)
// mark, search, count, scan, emit, finish: six kernels in stream order on `stream` (pnec_detect.hip)
hipError_t launch_detect_keypoints(int pixel_type, const DetectArgs &a, hipStream_t stream);
#endif

}  // namespace pnec_hip
