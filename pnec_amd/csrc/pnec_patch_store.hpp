// pnec_patch_store.hpp -- stored patches (pnec_hip_patch_store_slot_bytes, pnec_hip_patch_store_add,
// pnec_hip_patch_track_stored): launch interface of pnec_patch_store.hip, shared with the ABI layer, the layout of a slot,
// and the rules of the slot assignment -- the counts of an image, a carried row's local slot, the free bits of a word of
// the occupancy map, the word and the bit of the i-th free slot -- written so that they also compile for the host
// (tools/patch_store_host.cc replays the assignment's control flow with them under the address sanitizer, on arrays
// without slack, before any device does).  include/pnec_hip.h has the definition.
#pragma once

#include <cstdint>

#include "pnec_patch_track.hpp"
#include "pnec_tracks.hpp"

namespace pnec_hip {

// ---- a slot: kStoreHeader + n_levels * kStoreLevel doubles (64-bit words)
//   word 0          int64   n   of the level-0 template (valid points)
//   word 1          double  S   of the level-0 template
//   words 2 .. 7    double  H[6] of the level-0 template (00 01 02 11 12 22)
//   words 8 + l     int64   level l's template status (patch_inverse3's return), l < 8
//   words 16 + l    uint64  level l's validity: bit i is pattern point i's
//   words 24 .. 31  0
//   level l's planes start at word kStoreHeader + l * kStoreLevel: four planes of kStorePlane doubles, element i of a
//   plane is pattern point i's -- the normalised value, then the three components of the gain.
// With the store aligned to 256 bytes every plane starts on a 128-byte line, and the 16 lanes of a track, lane j reading
// elements j + 16 s, read 128 contiguous bytes per plane and s.
constexpr int kStoreHeader = 32;
constexpr int kStorePlane = 64;
constexpr int kStorePlanes = 4;
constexpr int kStoreLevel = kStorePlanes * kStorePlane;
constexpr int kStoreWordN = 0, kStoreWordS = 1, kStoreWordH = 2, kStoreWordStatus = 8, kStoreWordValid = 16,
              kStoreWordZero = 24;
// the assignment keeps an image's occupancy map and its running count of free slots in LDS: one bit and 1/32 of an
// int32 per local slot
constexpr int64_t kStoreMaxCapacity = 65536;
constexpr int kStoreMapWords = (int)(kStoreMaxCapacity / 32);
constexpr int kStoreAssignBlock = 256;

PNEC_TRACKS_HD int64_t store_slot_doubles(int32_t n_levels) {
  return (int64_t)kStoreHeader + (int64_t)n_levels * kStoreLevel;
}

struct PatchStoreAssignArgs {
  int64_t n_images;
  const int64_t *carried_offsets;   // [n_images + 1] or NULL: nothing is carried
  const int64_t *offsets;           // [n_images + 1]
  int64_t n_rows;
  int32_t *slot;                    // [n_rows], read (carried rows) and written (new rows, padding)
  int64_t capacity;                 // C, 1 .. kStoreMaxCapacity, n_images * C fits int32
};

// image f: its rows [lo, lo + c), the first `take` of them carried
PNEC_TRACKS_HD void store_counts(const int64_t *carried_offsets, const int64_t *offsets, int64_t n_rows, int64_t f,
                                 int64_t &lo, int64_t &c, int64_t &take) {
  int64_t hi;
  tracks_range(offsets, f, n_rows, lo, hi);
  c = hi - lo;
  int64_t n_a = 0;
  if (carried_offsets) n_a = carried_offsets[f + 1] - carried_offsets[f];
  n_a = n_a < 0 ? 0 : n_a;
  take = n_a < c ? n_a : c;
}

// a carried row's local slot, -1 when its value is not a slot of image f
PNEC_TRACKS_HD int64_t store_local_slot(int32_t value, int64_t f, int64_t C) {
  const int64_t v = (int64_t)value - f * C;
  return v >= 0 && v < C ? v : -1;
}

// the free local slots among 32 w .. 32 w + 31, as bits: not occupied and below C
PNEC_TRACKS_HD uint32_t store_free_word(uint32_t occupied, int64_t w, int64_t C) {
  const int64_t left = C - 32 * w;
  const uint32_t below = left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : ((1u << (int)left) - 1u));
  return ~occupied & below;
}

PNEC_TRACKS_HD int store_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

// the position of the r-th set bit of `bits` (r counted from 0, r < popcount(bits))
PNEC_TRACKS_HD int store_select_bit(uint32_t bits, int r) {
  int at = 0;
  for (int width = 16; width >= 1; width >>= 1) {
    const uint32_t low = (bits >> at) & ((1u << width) - 1u);
    const int n = store_popcount(low);
    if (r >= n) {
      r -= n;
      at += width;
    }
  }
  return at;
}

// the local slot of the i-th free one (i counted from 0, i < the number of free slots): before[w] free slots lie in the
// words below w, n_words >= 1
PNEC_TRACKS_HD int64_t store_nth_free(const uint32_t *occupied, const int32_t *before, int n_words, int64_t C,
                                      int64_t i) {
  int lo = 0, hi = n_words - 1;   // the last word with before[w] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)before[mid] <= i) lo = mid; else hi = mid - 1;
  }
  // (words without a free bit share their `before` with the next one: the last of them that qualifies has the bit)
  const uint32_t bits = store_free_word(occupied[lo], lo, C);
  return 32 * (int64_t)lo + store_select_bit(bits, (int)(i - before[lo]));
}

#if defined(__HIPCC__)
struct PatchStoreBuildArgs {
  TrackPyramid cur;                 // the frame the new rows were detected in
  int32_t n_levels;
  int32_t w, h;                     // of level 0
  int64_t n_images;
  const int64_t *carried_offsets;   // [n_images + 1] or NULL
  const int64_t *offsets;           // [n_images + 1]
  int64_t n_rows;
  const double *tmpl_pts;           // [n_rows, 2]
  const int32_t *slot;              // [n_rows], assigned
  const double *pattern;            // [n_pattern, 2]
  int32_t n_pattern;
  double *store;                    // [n_slots, store_slot_doubles(n_levels)]
  int64_t n_slots;
};

// one block per image
hipError_t launch_patch_store_assign(const PatchStoreAssignArgs &a, hipStream_t stream);
// 16 lanes per (row, level)
hipError_t launch_patch_store_build(int pixel_type, const PatchStoreBuildArgs &a, hipStream_t stream);
// pnec_hip_patch_track's kernel with the templates of keypoint k read from slot[k] of the store (a.tmpl is not used)
hipError_t launch_patch_track_stored(int pixel_type, const PatchTrackArgs &a, const double *store, int64_t n_slots,
                                     const int32_t *slot, hipStream_t stream);
#endif

}  // namespace pnec_hip
