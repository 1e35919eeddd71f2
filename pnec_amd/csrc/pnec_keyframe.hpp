// pnec_keyframe.hpp -- keyframe pairs (pnec_hip_tracks_keyframe): launch interface of pnec_keyframe.hip, shared with the
// ABI layer, and every rule of the call -- the match predicate, the displacement of a match, the order of the sum, the
// accept rule, the saturating span, `take`, the next-state row, the pair row and the padding values -- written so that it
// also compiles for the host (tools/keyframe_host.cc replays the kernels' control flow with it under the address
// sanitizer, on arrays without slack, before any device does).  include/pnec_hip.h has the definition.
#pragma once

#include <cmath>
#include <cstdint>

#include "pnec_tracks.hpp"

namespace pnec_hip {

constexpr int64_t kKeyframePadRow = -1;

struct KeyframeArgs {
  int64_t n_images;
  // the retained set B (offsets NULL: the first-frame form, n_rows = 0)
  const int64_t *offsets;      // [n_images + 1]
  int64_t n_rows;
  const double *pts;           // [n_rows, 2]
  const double *cov;           // [n_rows, 3] or NULL
  const int64_t *src;          // [n_rows] the row of the state
  // the refilled set A'
  const int64_t *new_offsets;  // [n_images + 1]
  int64_t n_new;
  const double *new_pts;       // [n_new, 2]
  const double *new_cov;       // [n_new, 3] or NULL
  // the state
  int64_t n_key_rows;
  const double *key_pts;       // [n_key_rows, 2]
  const double *key_cov;       // [n_key_rows, 3] or NULL
  const int32_t *span;         // [n_images]
  double min_displacement;
  int32_t max_span;
  // the pairs: n_rows rows
  int64_t *out_offsets;        // [n_images + 1]
  double *out_key_pts, *out_pts;   // [n_rows, 2]
  double *out_cov, *out_key_cov;   // [n_rows, 3] or NULL
  int64_t *out_row;            // [n_rows]
  uint8_t *out_accepted;       // [n_images] or NULL
  double *out_mean;            // [n_images] or NULL
  int32_t *out_n_matches;      // [n_images] or NULL
  // the next state: n_new rows
  double *next_key_pts;        // [n_new, 2]
  double *next_key_cov;        // [n_new, 3] or NULL
  int32_t *next_span;          // [n_images]; 0 <=> the image was accepted: what the later launches read
};

PNEC_TRACKS_HD bool keyframe_finite(double x) { return x - x == 0.0; }   // (false for NaN and the infinities)

// is retained row k (inside its image's range) a match?  `d` gets its displacement
PNEC_TRACKS_HD bool keyframe_match(const KeyframeArgs &a, int64_t k, double &d) {
  d = 0.0;
  const int64_t s = a.src[k];
  if (s < 0 || s >= a.n_key_rows) return false;
  const double kx = a.key_pts[2 * s], ky = a.key_pts[2 * s + 1], x = a.pts[2 * k], y = a.pts[2 * k + 1];
  if (!(keyframe_finite(kx) && keyframe_finite(ky) && keyframe_finite(x) && keyframe_finite(y))) return false;
  const double dx = x - kx, dy = y - ky;
  d = sqrt(dx * dx + dy * dy);
  return true;
}

// The order of the sum.  Lane l of 64 adds the displacements of the matches among rows lo + l, lo + l + 64, ... in that
// order, from +0.0; then six tree steps s = 32, 16, 8, 4, 2, 1: v[l] += v[l + s] (a lane with l + s > 63 adds its own
// value: it is never read again); the sum is v[0].  This is one step of that tree for lane `lane` of `v` before the step.
PNEC_TRACKS_HD double keyframe_tree_step(double own, double other) { return own + other; }
PNEC_TRACKS_HD int keyframe_tree_peer(int lane, int s) { return lane + s < kTracksLanes ? lane + s : lane; }

PNEC_TRACKS_HD double keyframe_mean(double sum, int64_t n_matches) {
  return n_matches > 0 ? sum / (double)n_matches : tracks_nan();
}

// a negative span counts as 0
PNEC_TRACKS_HD int32_t keyframe_span(int32_t span) { return span < 0 ? 0 : span; }

// the reference's comparison (a NaN mean is accepted), or the cap on the pair's span
PNEC_TRACKS_HD bool keyframe_accept(double mean, int32_t span, double min_displacement, int32_t max_span) {
  return !(mean < min_displacement) || (int64_t)keyframe_span(span) + 1 >= (int64_t)max_span;
}

// >= 1 for a skipped image
PNEC_TRACKS_HD int32_t keyframe_next_span(bool accepted, int32_t span) {
  const int32_t s = keyframe_span(span);
  return accepted ? 0 : (s == INT32_MAX ? INT32_MAX : s + 1);
}

// count's last statements for image f with n matches whose displacements sum to `sum`
PNEC_TRACKS_HD void keyframe_decide(const KeyframeArgs &a, int64_t f, int64_t n, double sum) {
  const bool first = !a.offsets;
  const int32_t span = (first || !a.span) ? 0 : a.span[f];
  const double mean = keyframe_mean(sum, n);
  const bool accepted = first || keyframe_accept(mean, span, a.min_displacement, a.max_span);
  a.out_offsets[f + 1] = accepted ? n : 0;
  a.next_span[f] = keyframe_next_span(accepted, span);
  if (a.out_n_matches) a.out_n_matches[f] = (int32_t)n;
  if (a.out_mean) a.out_mean[f] = mean;
  if (a.out_accepted) a.out_accepted[f] = accepted ? 1 : 0;
}

PNEC_TRACKS_HD bool keyframe_accepted(const KeyframeArgs &a, int64_t f) { return a.next_span[f] == 0; }

// emit: retained row k, a match, goes to pair row at
PNEC_TRACKS_HD void keyframe_pair_row(const KeyframeArgs &a, int64_t k, int64_t at) {
  const int64_t s = a.src[k];
  a.out_key_pts[2 * at] = a.key_pts[2 * s];
  a.out_key_pts[2 * at + 1] = a.key_pts[2 * s + 1];
  a.out_pts[2 * at] = a.pts[2 * k];
  a.out_pts[2 * at + 1] = a.pts[2 * k + 1];
  if (a.out_cov) {
    a.out_cov[3 * at] = a.cov[3 * k];
    a.out_cov[3 * at + 1] = a.cov[3 * k + 1];
    a.out_cov[3 * at + 2] = a.cov[3 * k + 2];
  }
  if (a.out_key_cov) {
    a.out_key_cov[3 * at] = a.key_cov[3 * s];
    a.out_key_cov[3 * at + 1] = a.key_cov[3 * s + 1];
    a.out_key_cov[3 * at + 2] = a.key_cov[3 * s + 2];
  }
  a.out_row[at] = k;
}

PNEC_TRACKS_HD void keyframe_pad_pair(const KeyframeArgs &a, int64_t at) {
  const double nan = tracks_nan();
  a.out_key_pts[2 * at] = nan;
  a.out_key_pts[2 * at + 1] = nan;
  a.out_pts[2 * at] = nan;
  a.out_pts[2 * at + 1] = nan;
  if (a.out_cov) {
    a.out_cov[3 * at] = nan;
    a.out_cov[3 * at + 1] = nan;
    a.out_cov[3 * at + 2] = nan;
  }
  if (a.out_key_cov) {
    a.out_key_cov[3 * at] = nan;
    a.out_key_cov[3 * at + 1] = nan;
    a.out_key_cov[3 * at + 2] = nan;
  }
  a.out_row[at] = kKeyframePadRow;
}

// how many rows of image f the two sets share: append's take_a for every capacity
PNEC_TRACKS_HD int64_t keyframe_take(int64_t count_b, int64_t count_new) { return count_b < count_new ? count_b : count_new; }

// the next state's row i (< n_new): next_span and nothing else of this call's outputs is read
PNEC_TRACKS_HD void keyframe_state_row(const KeyframeArgs &a, int64_t i) {
  const double nan = tracks_nan();
  double x = nan, y = nan, c0 = nan, c1 = nan, c2 = nan;
  const int64_t f = tracks_image_of(a.new_offsets, a.n_images, i);
  int64_t lo, hi;
  tracks_range(a.new_offsets, f, a.n_new, lo, hi);
  if (i >= lo && i < hi) {   // (else: a row at or beyond new_offsets[n_images])
    if (keyframe_accepted(a, f)) {
      x = a.new_pts[2 * i];
      y = a.new_pts[2 * i + 1];
      if (a.new_cov) {
        c0 = a.new_cov[3 * i];
        c1 = a.new_cov[3 * i + 1];
        c2 = a.new_cov[3 * i + 2];
      }
    } else {
      int64_t lo_b, hi_b;
      tracks_range(a.offsets, f, a.n_rows, lo_b, hi_b);
      const int64_t l = i - lo;
      if (l < keyframe_take(hi_b - lo_b, hi - lo)) {
        const int64_t s = a.src[lo_b + l];
        if (s >= 0 && s < a.n_key_rows) {
          x = a.key_pts[2 * s];
          y = a.key_pts[2 * s + 1];
          if (a.key_cov) {
            c0 = a.key_cov[3 * s];
            c1 = a.key_cov[3 * s + 1];
            c2 = a.key_cov[3 * s + 2];
          }
        }
      }
    }
  }
  a.next_key_pts[2 * i] = x;
  a.next_key_pts[2 * i + 1] = y;
  if (a.next_key_cov) {
    a.next_key_cov[3 * i] = c0;
    a.next_key_cov[3 * i + 1] = c1;
    a.next_key_cov[3 * i + 2] = c2;
  }
}

#if defined(__HIPCC__)
// four launches: count, scan, emit, state + pad
hipError_t launch_tracks_keyframe(const KeyframeArgs &a, hipStream_t stream);
#endif

}  // namespace pnec_hip
