// pnec_tracks.hpp -- the bookkeeping of tracks across frames (pnec_hip_tracks_retain, pnec_hip_tracks_append): launch
// interface of pnec_tracks.hip, shared with the ABI layer, and everything in it that is arithmetic or control flow -- the
// retention rule, the saturating age, the clamped row ranges, the ballot rank, the capacity split, the image of an output
// row, the padding values -- written so that it also compiles for the host (tools/tracks_host.cc replays the kernels'
// control flow with it under the address sanitizer, on arrays without slack, before any device does).
// include/pnec_hip.h has the definition.
#pragma once

#include <cstdint>

#include "pnec_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNEC_TRACKS_HD __host__ __device__ __forceinline__
#else
#define PNEC_TRACKS_HD inline
#endif

namespace pnec_hip {

constexpr int kTracksLanes = 64;   // one wavefront per image in retain's count and emit
constexpr int kTracksWaves = 4;
constexpr int kTracksBlock = kTracksWaves * kTracksLanes;
constexpr int64_t kTracksPadId = -1, kTracksPadSrc = -1;
constexpr int32_t kTracksPadInt = 0;

// A quiet NaN built from its bits, so that the host and the device write the same word into padding.
PNEC_TRACKS_HD double tracks_nan() {
  union {
    uint64_t u;
    double d;
  } v;
  v.u = 0x7ff8000000000000ull;
  return v.d;
}

// rows [lo, hi) of image f, forced into 0 <= lo <= hi <= n_rows whatever the offsets hold (DEVICE space checks nothing)
PNEC_TRACKS_HD void tracks_range(const int64_t *offsets, int64_t f, int64_t n_rows, int64_t &lo, int64_t &hi) {
  lo = 0;
  hi = 0;
  if (!offsets) return;
  lo = offsets[f];
  hi = offsets[f + 1];
  lo = lo < 0 ? 0 : (lo > n_rows ? n_rows : lo);
  hi = hi < lo ? lo : (hi > n_rows ? n_rows : hi);
}

// the retention rule of a row that lies inside its image's range
PNEC_TRACKS_HD bool tracks_keep(int64_t id, int32_t status, int32_t age, int32_t max_age) {
  return id >= 0 && status == PNEC_HIP_TRACK_OK && (max_age == 0 || (int64_t)age + 1 <= (int64_t)max_age);
}

PNEC_TRACKS_HD int32_t tracks_next_age(int32_t age) { return age == INT32_MAX ? INT32_MAX : age + 1; }

// how many lanes below `lane` hold a true predicate
PNEC_TRACKS_HD int tracks_rank(uint64_t ballot, int lane) {
  const uint64_t below = ballot & ((1ull << lane) - 1ull);   // lane in 0 .. 63: the shift is defined
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(below);
#else
  return __builtin_popcountll(below);
#endif
}
PNEC_TRACKS_HD int tracks_popcount(uint64_t ballot) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(ballot);
#else
  return __builtin_popcountll(ballot);
#endif
}

// append: of a set rows and d detections an image with room for C rows keeps the first take_a and the first take_d
PNEC_TRACKS_HD void tracks_take(int64_t a, int64_t d, int64_t C, int64_t &take_a, int64_t &take_d) {
  take_a = a < C ? a : C;
  const int64_t room = C - take_a;
  take_d = d < room ? d : room;
}

// the image of output row i: the last f in [0, F - 1] with offsets[f] <= i (offsets non-decreasing, offsets[0] = 0)
PNEC_TRACKS_HD int64_t tracks_image_of(const int64_t *offsets, int64_t F, int64_t i) {
  int64_t lo = 0, hi = F - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct TrackSetIn {
  const int64_t *offsets;     // [n_images + 1]; NULL: no set (append's first frame)
  int64_t n_rows;
  const int64_t *id;          // [n_rows]
  const int32_t *tmpl_image;  // [n_rows]
  const double *tmpl_pts;     // [n_rows, 2]
  const int32_t *age;         // [n_rows]
  const double *pts;          // [n_rows, 2]
  const double *angle;        // [n_rows]    (append only)
  const double *cov;          // [n_rows, 3] or NULL
};

struct TrackSetOut {
  int64_t *offsets;
  int64_t *id;
  int32_t *tmpl_image;
  double *tmpl_pts;
  int32_t *age;
  double *pts;
  double *angle;
  double *cov;                // or NULL
};

struct TracksRetainArgs {
  int64_t n_images;
  TrackSetIn in;
  const double *trk_pts;      // [n_rows, 2]
  const double *trk_angle;    // [n_rows]
  const double *trk_cov;      // [n_rows, 3] or NULL
  const int32_t *trk_status;  // [n_rows]
  int32_t max_age;
  TrackSetOut out;            // n_rows rows
  double *out_prev_pts;       // [n_rows, 2] or NULL
  double *out_prev_cov;       // [n_rows, 3] or NULL
  int64_t *out_src;           // [n_rows]    or NULL
};

struct TracksAppendArgs {
  int64_t n_images;
  TrackSetIn in;
  const int64_t *det_offsets; // [n_images + 1]
  int64_t n_det;
  const double *det_pts;      // [n_det, 2]
  const double *det_cov;      // [n_det, 3] or NULL
  int32_t tmpl_image_base;
  int64_t capacity;           // per image
  int64_t *next_id;           // [n_images], read by emit, written by the last kernel
  int64_t n_out;
  TrackSetOut out;            // n_out rows
  int64_t *out_dropped;       // [n_images] or NULL
};

// the padding row (both calls) and the two kinds of rows append writes: the same statements on the host and the device
PNEC_TRACKS_HD void tracks_pad_row(const TrackSetOut &o, int64_t at) {
  const double nan = tracks_nan();
  o.id[at] = kTracksPadId;
  o.tmpl_image[at] = kTracksPadInt;
  o.tmpl_pts[2 * at] = nan;
  o.tmpl_pts[2 * at + 1] = nan;
  o.age[at] = kTracksPadInt;
  o.pts[2 * at] = nan;
  o.pts[2 * at + 1] = nan;
  o.angle[at] = nan;
  if (o.cov) {
    o.cov[3 * at] = nan;
    o.cov[3 * at + 1] = nan;
    o.cov[3 * at + 2] = nan;
  }
}

PNEC_TRACKS_HD void tracks_pad_retained(const TracksRetainArgs &a, int64_t at) {
  const double nan = tracks_nan();
  tracks_pad_row(a.out, at);
  if (a.out_prev_pts) {
    a.out_prev_pts[2 * at] = nan;
    a.out_prev_pts[2 * at + 1] = nan;
  }
  if (a.out_prev_cov) {
    a.out_prev_cov[3 * at] = nan;
    a.out_prev_cov[3 * at + 1] = nan;
    a.out_prev_cov[3 * at + 2] = nan;
  }
  if (a.out_src) a.out_src[at] = kTracksPadSrc;
}

// retain: input row k goes to output row at
PNEC_TRACKS_HD void tracks_retain_row(const TracksRetainArgs &a, int64_t k, int64_t at) {
  a.out.id[at] = a.in.id[k];
  a.out.tmpl_image[at] = a.in.tmpl_image[k];
  a.out.tmpl_pts[2 * at] = a.in.tmpl_pts[2 * k];
  a.out.tmpl_pts[2 * at + 1] = a.in.tmpl_pts[2 * k + 1];
  a.out.age[at] = tracks_next_age(a.in.age[k]);
  a.out.pts[2 * at] = a.trk_pts[2 * k];
  a.out.pts[2 * at + 1] = a.trk_pts[2 * k + 1];
  a.out.angle[at] = a.trk_angle[k];
  if (a.out.cov) {
    a.out.cov[3 * at] = a.trk_cov[3 * k];
    a.out.cov[3 * at + 1] = a.trk_cov[3 * k + 1];
    a.out.cov[3 * at + 2] = a.trk_cov[3 * k + 2];
  }
  if (a.out_prev_pts) {
    a.out_prev_pts[2 * at] = a.in.pts[2 * k];
    a.out_prev_pts[2 * at + 1] = a.in.pts[2 * k + 1];
  }
  if (a.out_prev_cov) {
    a.out_prev_cov[3 * at] = a.in.cov[3 * k];
    a.out_prev_cov[3 * at + 1] = a.in.cov[3 * k + 1];
    a.out_prev_cov[3 * at + 2] = a.in.cov[3 * k + 2];
  }
  if (a.out_src) a.out_src[at] = k;
}

// append: the counts of image f from the two offset arrays
PNEC_TRACKS_HD void tracks_append_counts(const TracksAppendArgs &a, int64_t f, int64_t &lo_a, int64_t &lo_d,
                                         int64_t &n_a, int64_t &n_d, int64_t &take_a, int64_t &take_d) {
  int64_t hi_a, hi_d;
  tracks_range(a.in.offsets, f, a.in.n_rows, lo_a, hi_a);
  tracks_range(a.det_offsets, f, a.n_det, lo_d, hi_d);
  n_a = hi_a - lo_a;
  n_d = hi_d - lo_d;
  tracks_take(n_a, n_d, a.capacity, take_a, take_d);
}

// append: output row i (< n_out), out.offsets already scanned
PNEC_TRACKS_HD void tracks_append_row(const TracksAppendArgs &a, int64_t i) {
  const int64_t F = a.n_images;
  if (i >= a.out.offsets[F]) {
    tracks_pad_row(a.out, i);
    return;
  }
  const int64_t f = tracks_image_of(a.out.offsets, F, i);
  const int64_t j = i - a.out.offsets[f];
  int64_t lo_a, lo_d, n_a, n_d, take_a, take_d;
  tracks_append_counts(a, f, lo_a, lo_d, n_a, n_d, take_a, take_d);
  const double nan = tracks_nan();
  if (j < take_a) {
    const int64_t k = lo_a + j;
    a.out.id[i] = a.in.id[k];
    a.out.tmpl_image[i] = a.in.tmpl_image[k];
    a.out.tmpl_pts[2 * i] = a.in.tmpl_pts[2 * k];
    a.out.tmpl_pts[2 * i + 1] = a.in.tmpl_pts[2 * k + 1];
    a.out.age[i] = a.in.age[k];
    a.out.pts[2 * i] = a.in.pts[2 * k];
    a.out.pts[2 * i + 1] = a.in.pts[2 * k + 1];
    a.out.angle[i] = a.in.angle[k];
    if (a.out.cov) {
      a.out.cov[3 * i] = a.in.cov ? a.in.cov[3 * k] : nan;
      a.out.cov[3 * i + 1] = a.in.cov ? a.in.cov[3 * k + 1] : nan;
      a.out.cov[3 * i + 2] = a.in.cov ? a.in.cov[3 * k + 2] : nan;
    }
  } else {
    const int64_t r = j - take_a, k = lo_d + r;
    const double x = a.det_pts[2 * k], y = a.det_pts[2 * k + 1];
    a.out.id[i] = a.next_id[f] + r;
    a.out.tmpl_image[i] = a.tmpl_image_base + (int32_t)f;
    a.out.tmpl_pts[2 * i] = x;
    a.out.tmpl_pts[2 * i + 1] = y;
    a.out.age[i] = 0;
    a.out.pts[2 * i] = x;
    a.out.pts[2 * i + 1] = y;
    a.out.angle[i] = 0.0;
    if (a.out.cov) {
      a.out.cov[3 * i] = a.det_cov ? a.det_cov[3 * k] : nan;
      a.out.cov[3 * i + 1] = a.det_cov ? a.det_cov[3 * k + 1] : nan;
      a.out.cov[3 * i + 2] = a.det_cov ? a.det_cov[3 * k + 2] : nan;
    }
  }
}

#if defined(__HIPCC__)
// (shared by pnec_tracks.hip and pnec_keyframe.hip: one block of 256 lanes)
// v[1 .. F] hold per-image counts (count(f) for f < F): the running sum in place, 256 images at a time, and v[0] = 0
template <typename Count>
__device__ __forceinline__ void tracks_block_scan(int64_t *v, int64_t F, Count count) {
  __shared__ int64_t part[256];
  int64_t carry = 0;
  for (int64_t base = 0; base < F; base += 256) {
    const int64_t f = base + threadIdx.x;
    int64_t x = f < F ? count(f) : 0;
    part[threadIdx.x] = x;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      const int64_t o = (int)threadIdx.x >= s ? part[threadIdx.x - s] : 0;
      __syncthreads();
      x += o;
      part[threadIdx.x] = x;
      __syncthreads();
    }
    if (f < F) v[f + 1] = carry + x;
    carry += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) v[0] = 0;
}

// four launches: count, scan, emit, pad
hipError_t launch_tracks_retain(const TracksRetainArgs &a, hipStream_t stream);
// three launches: scan (with out_dropped), emit, next_id
hipError_t launch_tracks_append(const TracksAppendArgs &a, hipStream_t stream);
#endif

}  // namespace pnec_hip
