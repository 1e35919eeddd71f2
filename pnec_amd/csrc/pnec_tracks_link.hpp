// pnec_tracks_link.hpp -- the join of two track sets on their ids (pnec_hip_tracks_link): launch interface of
// pnec_tracks_link.hip, shared with the ABI layer, and the whole of a row's work -- its image, the two cuts, the
// bisection -- written so that it also compiles for the host.  include/pnec_hip.h has the definition.
#pragma once

#include <cstdint>

#include "pnec_tracks.hpp"

namespace pnec_hip {

constexpr int kTracksLinkBlock = 256;   // the row kernel: one lane per row of the current set
constexpr int32_t kTracksNoLink = -1;

struct TracksLinkArgs {
  int64_t n_images;
  const int64_t *cur_offsets;    // [n_images + 1]
  int64_t n_cur;
  const int64_t *cur_id;         // [n_cur]
  const int64_t *prev_offsets;   // [n_images + 1]
  int64_t n_prev;
  const int64_t *prev_id;        // [n_prev]
  int32_t *out_link;             // [n_cur]
  int32_t *out_n_linked;         // [n_images] or NULL
};

// the lower bound of `id` among the Lp ids from prev_id[plo] on, by the bisection of the definition; the row within the
// previous image where that entry holds `id`, else -1.  Every read lies in [plo, plo + Lp).
PNEC_TRACKS_HD int32_t tracks_link_find(const int64_t *prev_id, int64_t plo, int64_t Lp, int64_t id) {
  if (id < 0) return kTracksNoLink;
  int64_t a = 0, b = Lp;
  while (a < b) {
    const int64_t m = a + (b - a) / 2;
    if (prev_id[plo + m] < id) a = m + 1; else b = m;
  }
  return a < Lp && prev_id[plo + a] == id ? (int32_t)a : kTracksNoLink;
}

// row k (< n_cur) of the current set: its image is the last f whose cut first row is not beyond k (the images that share
// that first row and come before it are empty); a row outside that image's range -- at or beyond the cut
// cur_offsets[n_images], or in a gap that only unchecked offsets can leave -- is padding.
PNEC_TRACKS_HD int32_t tracks_link_row(const TracksLinkArgs &a, int64_t k) {
  int64_t f = 0, above = a.n_images;
  while (above - f > 1) {
    const int64_t mid = f + (above - f) / 2;
    const int64_t first = a.cur_offsets[mid];
    if ((first < 0 ? 0 : first) <= k) f = mid; else above = mid;   // (k < n_cur: the upper clamp decides nothing)
  }
  int64_t lo, hi, plo, phi;
  tracks_range(a.cur_offsets, f, a.n_cur, lo, hi);
  if (k < lo || k >= hi) return kTracksNoLink;
  tracks_range(a.prev_offsets, f, a.n_prev, plo, phi);
  return tracks_link_find(a.prev_id, plo, phi - plo, a.cur_id[k]);
}

#if defined(__HIPCC__)
// two launches: the rows (one lane each), then the counts (one wavefront per image); n_cur >= 1
hipError_t launch_tracks_link(const TracksLinkArgs &a, hipStream_t stream);
#endif

}  // namespace pnec_hip
