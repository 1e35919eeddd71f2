// call_arrays_host.cc -- the counting of CallArrays (pnec_amd/csrc/pnec_internal.hpp) checked on the host: the lists of
// the entry points of pnec_capi.hip / pnec_pipeline.hip replayed through CallPlan (pnec_call_plan.hpp, no HIP) at small
// sizes.  For every list and every choice of its optional arrays:
//   * the regions of each buffer follow one another in the order of the list without gap or overlap, end at the total, and
//     hold what is copied into or out of them (offsets and lengths count whole items of the buffer, so everything is
//     8-byte aligned among the doubles and 4-byte aligned among the ints);
//   * with every optional array given the totals are the ones the entry point used to write out by hand
//     (stage.reserve(...) before CallArrays), and with some omitted they are never larger;
//   * an output marked kKeep has room without a caller's array, and one marked kPreload travels up exactly when given.
// Built with -fsanitize=address,undefined by tests/test_call_arrays_cpu.py.  Prints one line per list; exit status 1 on
// the first list that fails.
#include <cstdio>
#include <functional>
#include <string>

#include "pnec_call_plan.hpp"

using pnec_hip::CallPlan;
using pnec_hip::kKeep;
using pnec_hip::kPreload;

namespace {

int g_failures = 0;
void expect(bool ok, const std::string &list, const char *what) {
  if (ok) return;
  std::printf("FAIL %s: %s\n", list.c_str(), what);
  ++g_failures;
}

// One replay: the arrays a caller may leave out are numbered in the order of the list; bit k of `given` says whether
// the k-th is there.  Required arrays are always there.
struct List {
  CallPlan plan;
  unsigned given;
  int n_optional = 0;
  struct Note {
    size_t entry;
    bool present;
    unsigned flags;
    bool output;
  };
  std::vector<Note> notes;
  explicit List(unsigned given_) : given(given_) {}
  bool opt() { return (given >> n_optional++) & 1u; }
  void in(bool present, int64_t n, size_t item) {
    plan.in(present, n, item);
    notes.push_back({plan.entries.size() - 1, present, 0, false});
  }
  void out(bool present, int64_t n, size_t item, unsigned flags = 0) {
    plan.out(present, n, item, flags);
    notes.push_back({plan.entries.size() - 1, present, flags, true});
  }
  void scratch(int64_t n, size_t item) { plan.scratch(n, item); }
};

void check_layout(const std::string &name, const List &l) {
  int64_t next[2] = {0, 0};
  for (const CallPlan::Entry &e : l.plan.entries) {
    const int64_t unit = e.ints ? 4 : 8;
    expect(e.offset == next[e.ints], name, "a region does not start where the one before it ends");
    expect(e.items >= 0, name, "a region of negative length");
    expect(e.room || e.items == 0, name, "an array without room takes room");
    expect(!(e.up || e.back) || e.room, name, "a copy without room");
    expect(!(e.up || e.back) || (int64_t)e.bytes <= e.items * unit, name, "a copy larger than its region");
    next[e.ints] = e.offset + e.items;
  }
  expect(next[0] == l.plan.doubles, name, "the doubles total is not the end of the last region");
  expect(next[1] == l.plan.ints, name, "the ints total is not the end of the last region");
  for (const List::Note &n : l.notes) {
    const CallPlan::Entry &e = l.plan.entries[n.entry];
    if (!n.output) {
      expect(e.room == n.present, name, "an input has room exactly when it is given");
      expect(e.up == (n.present && e.bytes > 0) && !e.back, name, "an input travels up, once, when given");
    } else {
      expect(e.room == (n.present || (n.flags & kKeep)), name, "an output has room when given or kept");
      expect(e.back == (n.present && e.bytes > 0), name, "an output comes back exactly when given");
      expect(e.up == (n.present && (n.flags & kPreload) && e.bytes > 0), name, "only a given preloaded output travels up");
    }
  }
}

// replay(l) builds the list; (doubles, ints) is the hand-written total of the entry point's former stage.reserve(...)
void run(const std::string &name, const std::function<void(List &)> &replay, int64_t doubles, int64_t ints) {
  const int before = g_failures;
  List probe(~0u);
  replay(probe);
  const int n_opt = probe.n_optional;
  check_layout(name, probe);
  expect(probe.plan.doubles == doubles, name, "doubles total with every array given differs from the former formula");
  expect(probe.plan.ints == ints, name, "ints total with every array given differs from the former formula");
  for (unsigned given = 0; given < (1u << n_opt); ++given) {
    List l(given);
    replay(l);
    check_layout(name, l);
    expect(l.n_optional == n_opt, name, "the list's length depends on what is given");
    expect(l.plan.doubles <= doubles && l.plan.ints <= ints, name, "totals above the former formula");
  }
  std::printf("%s %s: %d optional arrays, doubles %lld (formula %lld), ints %lld (formula %lld)\n",
              g_failures == before ? "ok  " : "FAIL", name.c_str(), n_opt, (long long)probe.plan.doubles, (long long)doubles,
              (long long)probe.plan.ints, (long long)ints);
}

int64_t image_block_bytes(int64_t elem, int64_t n_images, int64_t rows, int64_t pitch, int64_t width) {
  return elem * ((n_images * rows - 1) * pitch + width);
}
int64_t d8(int64_t bytes) { return (bytes + 7) / 8; }

std::string tag(const char *name, std::initializer_list<int64_t> sizes) {
  std::string s = name;
  char sep = '(';
  for (int64_t v : sizes) {
    s += sep + std::to_string(v);
    sep = ',';
  }
  return s + ")";
}

// ---- the batch entry points: P pairs of n correspondences each, n_hyp poses per pair -------------------------------
void batch_lists(int64_t P, int64_t n_hyp, int64_t n) {
  const int64_t S = P * n_hyp, M = P * n * n_hyp, C = P * n;

  run(tag("solve", {P, n_hyp}), [&](List &l) {
    l.in(true, 4 * P, 8);          // init_q
    l.in(l.opt(), 3 * P, 8);       // init_t
    l.in(l.opt(), 3 * S, 8);       // hyp_t
    l.out(l.opt(), 4 * S, 8, kKeep);
    l.out(l.opt(), 3 * S, 8, kKeep);
    l.out(l.opt(), S, 8, kKeep);
    l.out(l.opt(), S, 4, kKeep);
    l.out(l.opt(), S, 4, kKeep);
  }, 7 * P + 11 * S, 2 * S);

  if (n_hyp == 1) {
    run(tag("cost_function", {P}), [&](List &l) {
      l.in(true, 4 * P, 8);
      l.in(true, 3 * P, 8);
      l.out(true, P, 8);
    }, 8 * P, 0);

    run(tag("front_stage", {P}), [&](List &l) {
      l.in(true, 4 * P, 8);
      l.in(l.opt(), 3 * P, 8);     // init_t: NULL for the unweighted stage
      l.out(true, 4 * P, 8);
      l.out(true, 3 * P, 8);
    }, 14 * P, 0);

    // the former total, (11 P, 2 P), left the mask out: it had a block of C bytes of its own, now a region of the staging
    run(tag("ransac_eigensolver", {P, C}), [&](List &l) {
      l.in(true, 4 * P, 8);
      l.out(true, 4 * P, 8);
      l.out(true, 3 * P, 8);
      l.out(l.opt(), C, 1);        // inlier mask
      l.out(l.opt(), P, 4, kKeep);
      l.out(l.opt(), P, 4, kKeep);
    }, 11 * P + d8(C), 2 * P);

    // the former total, (28 P, 2 P), had a second block of P ints (`its`) that nothing used
    run(tag("solve_pipeline", {P}), [&](List &l) {
      l.in(true, 4 * P, 8);
      l.in(true, 3 * P, 8);
      l.scratch(4 * P, 8);         // es_q, es_t, w_q, w_t
      l.scratch(3 * P, 8);
      l.scratch(4 * P, 8);
      l.scratch(3 * P, 8);
      l.out(true, 4 * P, 8);
      l.out(true, 3 * P, 8);
      l.scratch(P, 4);             // inlier counts
    }, 28 * P, 2 * P - P);

    // (outputs only: the call reads nothing but the batch)
    run(tag("eight_point", {P}), [&](List &l) {
      l.out(l.opt(), 4 * P, 8);    // q
      l.out(l.opt(), 3 * P, 8);    // t
      l.out(l.opt(), 9 * P, 8);    // E
      l.out(l.opt(), 3 * P, 8);    // singular
      l.out(l.opt(), P, 8);        // gap
      l.out(l.opt(), 4 * P, 8);    // quality
      l.out(l.opt(), P, 4);        // choice
      l.out(l.opt(), P, 4);        // status
    }, 24 * P, 2 * P);

    run(tag("essential_minimal", {P}), [&](List &l) {
      l.out(l.opt(), 4 * P, 8);    // q
      l.out(l.opt(), 3 * P, 8);    // t
      l.out(l.opt(), 9 * P, 8);    // E
      l.out(l.opt(), 3 * P, 8);    // singular
      l.out(l.opt(), P, 8);        // gap
      l.out(l.opt(), P, 4);        // n_solutions
      l.out(l.opt(), 90 * P, 8);   // E_all
      l.out(l.opt(), 40 * P, 8);   // quality
      l.out(l.opt(), P, 4);        // choice
      l.out(l.opt(), P, 4);        // status
    }, 150 * P, 3 * P);

    run(tag("essential_ransac", {P, C}), [&](List &l) {
      l.out(l.opt(), 4 * P, 8);    // q
      l.out(l.opt(), 3 * P, 8);    // t
      l.out(l.opt(), 9 * P, 8);    // E
      l.out(l.opt(), 3 * P, 8);    // singular
      l.out(l.opt(), C, 1);        // inlier mask
      l.out(l.opt(), P, 4);        // inlier count
      l.out(l.opt(), P, 4);        // iterations
      l.out(l.opt(), P, 4);        // attempts
      l.out(l.opt(), P, 4);        // best attempt
      l.out(l.opt(), P, 4);        // status
    }, 19 * P + d8(C), 5 * P);

    // pairs of the previous batch: one more than of this one, so that the two counts cannot be mixed up unnoticed
    const int64_t Pp = P + 1;
    run(tag("relative_scale", {P, Pp, C}), [&](List &l) {
      l.in(true, 4 * P, 8);
      l.in(true, 3 * P, 8);
      l.in(true, 4 * Pp, 8);
      l.in(true, 3 * Pp, 8);
      l.in(true, P, 8);            // prev_pair (int64)
      l.out(l.opt(), 3 * P, 8);
      l.out(l.opt(), C, 8, kKeep); // ratios
      l.out(l.opt(), C, 1);
      l.in(true, C, 4);            // link
      l.out(l.opt(), P, 4);
      l.out(l.opt(), P, 4);
    }, 11 * P + 7 * Pp + C + d8(C), C + 2 * P);
  }

  run(tag("pose_covariance", {P, n_hyp}), [&](List &l) {
    l.in(true, 4 * S, 8);
    l.in(true, 3 * S, 8);
    l.out(l.opt(), 36 * S, 8);
    l.out(l.opt(), 15 * S, 8);
    l.out(l.opt(), 5 * S, 8);
    l.out(l.opt(), S, 8);
    l.out(l.opt(), S, 4);
  }, 64 * S, S);

  run(tag("residuals", {P, n_hyp, M}), [&](List &l) {
    l.in(true, 4 * S, 8);
    l.in(true, 3 * S, 8);
    l.out(l.opt(), S, 8);
    l.out(l.opt(), S, 8);
    l.out(l.opt(), S, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 1);
    l.out(l.opt(), S, 4);
  }, 10 * S + 2 * M + (M + 7) / 8, S);

  // (no former formula: the call was written with CallArrays; the total is the sum of its documented array lengths)
  run(tag("pose_sensitivity", {P, n_hyp, M}), [&](List &l) {
    l.in(true, 4 * S, 8);
    l.in(true, 3 * S, 8);
    l.in(true, 6 * S, 8);          // grad_pose
    l.out(l.opt(), 5 * S, 8);      // lambda
    l.out(l.opt(), 15 * S, 8);     // hessian
    l.out(l.opt(), 5 * S, 8);      // grad
    l.out(l.opt(), 5 * S, 8);      // newton
    l.out(l.opt(), 3 * M, 8);      // grad_bvs1
    l.out(l.opt(), 3 * M, 8);      // grad_bvs2
    l.out(l.opt(), 9 * M, 8);      // grad_covs
    l.out(l.opt(), 9 * M, 8);      // grad_covs_host
    l.out(l.opt(), S, 4);
  }, 43 * S + 24 * M, S);

  run(tag("triangulate", {P, n_hyp, M}), [&](List &l) {
    l.in(true, 4 * S, 8);
    l.in(true, 3 * S, 8);
    l.out(l.opt(), 3 * S, 8);
    l.out(l.opt(), S, 8);
    l.out(l.opt(), 3 * M, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 1);
    l.out(l.opt(), S, 4);
    l.out(l.opt(), S, 4);
    l.out(l.opt(), S, 4);
  }, 11 * S + 7 * M + (M + 7) / 8, 3 * S);
}

// ---- the image entry points: F images of h x w pixels of `elem` bytes, rows `pitch` elements apart ------------------
void image_lists(int64_t F, int64_t elem, int64_t n_points) {
  const int64_t h = 37, w = 41, pitch = 43, n_pattern = 5, M = n_points;
  const int64_t image_bytes = image_block_bytes(elem, F, h, pitch, w);

  run(tag("patch_covariance", {F, elem, M}), [&](List &l) {
    l.in(true, image_bytes, 1);
    l.in(true, F + 1, 8);          // offsets (int64)
    l.in(true, 2 * M, 8);
    l.in(true, 2 * n_pattern, 8);
    l.in(l.opt(), M, 8);           // angle
    l.out(l.opt(), 3 * M, 8);
    l.out(l.opt(), 6 * M, 8);
    l.out(l.opt(), M, 8);
    l.out(l.opt(), M, 4);
    l.out(l.opt(), M, 4);
  }, (image_bytes + 7) / 8 + (F + 1) + 13 * M + 2 * n_pattern, 2 * M);

  const int64_t pitch_out = 23;
  const int64_t out_bytes = image_block_bytes(elem, F, h / 2, pitch_out, w / 2);
  run(tag("image_pyramid_level", {F, elem}), [&](List &l) {
    l.in(true, image_bytes, 1);
    l.out(true, out_bytes, 1, kPreload);
  }, (image_bytes + 7) / 8 + (out_bytes + 7) / 8, 0);

  for (int n_levels : {1, 3})
    for (bool share_prev : {true, false}) {
      auto level_bytes = [&](int lv, int64_t p) { return image_block_bytes(elem, F, h >> lv, p, w >> lv); };
      int64_t pitches[3] = {pitch, 21, 11};
      int64_t pixels8 = 0;
      for (int lv = 0; lv < n_levels; ++lv) {
        pixels8 += (level_bytes(lv, pitches[lv]) + 7) / 8 + (level_bytes(lv, pitches[lv] + 1) + 7) / 8;
        if (!share_prev) pixels8 += (level_bytes(lv, pitches[lv] + 2) + 7) / 8;
      }
      run(tag("patch_track", {F, elem, M, n_levels, share_prev}), [&](List &l) {
        for (int lv = 0; lv < n_levels; ++lv) {
          l.in(true, level_bytes(lv, pitches[lv]), 1);                       // tmpl
          l.in(true, level_bytes(lv, pitches[lv] + 1), 1);                   // next
          if (!share_prev) l.in(true, level_bytes(lv, pitches[lv] + 2), 1);  // prev, unless it is tmpl's level
        }
        l.in(true, F + 1, 8);
        l.in(true, 2 * M, 8);
        l.in(l.opt(), 2 * M, 8);   // init_pts
        l.in(l.opt(), M, 8);       // init_angle
        l.in(true, 2 * n_pattern, 8);
        l.out(l.opt(), 2 * M, 8);
        l.out(l.opt(), M, 8);
        l.out(l.opt(), 3 * M, 8);
        l.out(l.opt(), M, 8);
        l.out(l.opt(), M, 4);
        l.out(l.opt(), M, 4);
      }, pixels8 + (F + 1) + 12 * M + 2 * n_pattern, 2 * M);
    }

  if (elem <= 2) {
    const int64_t grid = 8, per_cell = 2, n_cells = (w / grid) * (h / grid), cap = F * n_cells * per_cell;
    for (bool have_cur : {false, true}) {
      const int64_t Cn = have_cur ? 3 : 0;
      run(tag("detect_keypoints", {F, elem, have_cur}), [&](List &l) {
        l.in(true, image_bytes, 1);
        l.in(have_cur, F + 1, 8);  // cur_offsets and cur_pts: both or neither
        l.in(have_cur, 2 * Cn, 8);
        l.out(true, F * n_cells, 4);
        l.out(true, F + 1, 8);     // out_offsets (int64)
        l.out(true, 2 * cap, 8, kPreload);
        l.out(l.opt(), cap, 4, kPreload);
        l.out(l.opt(), cap, 4, kPreload);
      }, (image_bytes + 7) / 8 + (have_cur ? F + 1 + 2 * Cn : 0) + (F + 1) + 2 * cap, F * n_cells + 2 * cap);
    }
  }

  // the indexed tracker: pnec_hip_patch_track's list with a template stack of Ft images per level, never shared with
  // prev, and the index array
  for (int n_levels : {1, 3}) {
    const int64_t Ft = 2 * F + 1;
    auto level_bytes = [&](int lv, int64_t p, int64_t n) { return image_block_bytes(elem, n, h >> lv, p, w >> lv); };
    int64_t pitches[3] = {pitch, 21, 11};
    int64_t pixels8 = 0;
    for (int lv = 0; lv < n_levels; ++lv)
      pixels8 += (level_bytes(lv, pitches[lv], Ft) + 7) / 8 + (level_bytes(lv, pitches[lv] + 1, F) + 7) / 8 +
                 (level_bytes(lv, pitches[lv] + 2, F) + 7) / 8;
    run(tag("patch_track_indexed", {F, elem, M, n_levels}), [&](List &l) {
      for (int lv = 0; lv < n_levels; ++lv) {
        l.in(true, level_bytes(lv, pitches[lv], Ft), 1);      // tmpl: the stack
        l.in(true, level_bytes(lv, pitches[lv] + 1, F), 1);   // next
        l.in(true, level_bytes(lv, pitches[lv] + 2, F), 1);   // prev
      }
      l.in(true, F + 1, 8);
      l.in(true, 2 * M, 8);
      l.in(l.opt(), 2 * M, 8);   // init_pts
      l.in(l.opt(), M, 8);       // init_angle
      l.in(true, M, 4);          // tmpl_image
      l.in(true, 2 * n_pattern, 8);
      l.out(l.opt(), 2 * M, 8);
      l.out(l.opt(), M, 8);
      l.out(l.opt(), 3 * M, 8);
      l.out(l.opt(), M, 8);
      l.out(l.opt(), M, 4);
      l.out(l.opt(), M, 4);
    }, pixels8 + (F + 1) + 12 * M + 2 * n_pattern, 3 * M);
  }

  // the bookkeeping of tracks (no images): a set of N rows, D detections, O output rows
  if (elem == 1) {
    const int64_t N = M, D = M + 2, O = M + 5;
    run(tag("tracks_retain", {F, N}), [&](List &l) {
      l.in(true, F + 1, 8);      // offsets
      l.in(true, N, 8);          // id
      l.in(true, N, 4);          // tmpl_image
      l.in(true, 2 * N, 8);      // tmpl_pts
      l.in(true, N, 4);          // age
      l.in(true, 2 * N, 8);      // pts
      l.in(l.opt(), 3 * N, 8);   // cov
      l.in(true, 2 * N, 8);      // trk_pts
      l.in(true, N, 8);          // trk_angle
      l.in(l.opt(), 3 * N, 8);   // trk_cov
      l.in(true, N, 4);          // trk_status
      l.out(true, F + 1, 8);
      l.out(true, N, 8);
      l.out(true, N, 4);
      l.out(true, 2 * N, 8);
      l.out(true, N, 4);
      l.out(true, 2 * N, 8);
      l.out(true, N, 8);
      l.out(l.opt(), 3 * N, 8);  // out_cov
      l.out(l.opt(), 2 * N, 8);  // out_prev_pts
      l.out(l.opt(), 3 * N, 8);  // out_prev_cov
      l.out(l.opt(), N, 8);      // out_src
    }, 2 * (F + 1) + 29 * N, 5 * N);
    for (bool have_set : {false, true}) {
      const int64_t Ns = have_set ? N : 0;
      run(tag("tracks_append", {F, Ns, D, O}), [&](List &l) {
        l.in(have_set, F + 1, 8);
        l.in(have_set, Ns, 8);
        l.in(have_set, Ns, 4);
        l.in(have_set, 2 * Ns, 8);
        l.in(have_set, Ns, 4);
        l.in(have_set, 2 * Ns, 8);
        l.in(have_set, Ns, 8);
        l.in(have_set && l.opt(), 3 * Ns, 8);   // cov
        l.in(true, F + 1, 8);      // det_offsets
        l.in(true, 2 * D, 8);
        l.in(l.opt(), 3 * D, 8);   // det_cov
        l.out(true, F, 8, kPreload);   // next_id
        l.out(true, F + 1, 8);
        l.out(true, O, 8);
        l.out(true, O, 4);
        l.out(true, 2 * O, 8);
        l.out(true, O, 4);
        l.out(true, 2 * O, 8);
        l.out(true, O, 8);
        l.out(l.opt(), 3 * O, 8);  // out_cov
        l.out(l.opt(), F, 8);      // out_dropped
      }, (have_set ? F + 1 + 9 * Ns : 0) + (F + 1) + 5 * D + F + (F + 1) + 9 * O + F, 2 * Ns + 2 * O);
    }
    // keypoint undistortion (no images, no batch): N rows; either frame may be left out, a covariance goes with its
    // points, and an output is there exactly when its input is
    run(tag("undistort_keypoints", {N}), [&](List &l) {
      const bool pts1 = l.opt(), pts2 = l.opt();
      const bool cov2 = l.opt() && pts2, cov1 = l.opt() && pts1;
      const bool status1 = l.opt() && pts1, status2 = l.opt() && pts2;
      l.in(pts1, 2 * N, 8);
      l.in(pts2, 2 * N, 8);
      l.in(cov2, 3 * N, 8);
      l.in(cov1, 3 * N, 8);
      l.in(true, 9, 8);          // camera
      l.out(pts1, 2 * N, 8);
      l.out(pts2, 2 * N, 8);
      l.out(cov2, 3 * N, 8);
      l.out(cov1, 3 * N, 8);
      l.out(status1, N, 1);
      l.out(status2, N, 1);
    }, 20 * N + 9 + 2 * d8(N), 0);
    // trajectory evaluation (no images, no batch): N rows in F sequences.  compose: the translation's arrays go with
    // rel_t; rows of no sequence are not written, so the outputs travel up first
    run(tag("trajectory_compose", {F, N}), [&](List &l) {
      const bool rel_t = l.opt();
      const bool scale = l.opt() && rel_t, q0 = l.opt(), p0 = l.opt() && rel_t, valid = l.opt();
      l.in(true, F + 1, 8);      // offsets
      l.in(true, 4 * N, 8);      // rel_q
      l.in(rel_t, 3 * N, 8);
      l.in(scale, N, 8);
      l.in(q0, 4 * F, 8);
      l.in(p0, 3 * F, 8);
      l.out(true, 4 * N, 8, kPreload);
      l.out(rel_t, 3 * N, 8, kPreload);
      l.out(valid, N, 1, kPreload);
    }, (F + 1) + 15 * N + 7 * F + d8(N), 0);
    // metrics: the positions go together, out_rt1 needs them
    run(tag("trajectory_metrics", {F, N}), [&](List &l) {
      const bool positions = l.opt(), angle1 = l.opt(), rt1 = l.opt() && positions;
      l.in(true, F + 1, 8);      // offsets
      l.in(true, 4 * N, 8);      // est_q
      l.in(true, 4 * N, 8);      // gt_q
      l.in(positions, 3 * N, 8);
      l.in(positions, 3 * N, 8);
      l.out(true, 5 * F, 8);     // out_metrics
      l.out(true, 4 * N, 8);     // out_err_q
      l.out(true, N, 8, kPreload);
      l.out(true, N, 8, kPreload);
      l.out(angle1, N, 8, kPreload);
      l.out(rt1, N, 8, kPreload);
    }, (F + 1) + 22 * N + 5 * F, 0);
    // the join of two sets on their ids: N current rows, D previous rows (another count, so that the two cannot be mixed up)
    run(tag("tracks_link", {F, N, D}), [&](List &l) {
      l.in(true, F + 1, 8);      // cur_offsets
      l.in(true, N, 8);          // cur_id
      l.in(true, F + 1, 8);      // prev_offsets
      l.in(true, D, 8);          // prev_id
      l.out(true, N, 4);         // out_link
      l.out(l.opt(), F, 4);      // out_n_linked
    }, 2 * (F + 1) + N + D, N + F);
    // one step of the running scale and pose of F sequences: n_used goes with scale3
    run(tag("trajectory_advance", {F}), [&](List &l) {
      const bool count = l.opt(), scale3 = l.opt(), n_used = l.opt() && scale3;
      l.in(true, 4 * F, 8);      // rel_q
      l.in(true, 3 * F, 8);      // rel_t
      l.in(count, F, 4);
      l.in(scale3, 3 * F, 8);
      l.in(n_used, F, 4);
      l.in(true, F, 8);          // s, q, p
      l.in(true, 4 * F, 8);
      l.in(true, 3 * F, 8);
      l.out(true, F, 8);         // next_s, next_q, next_p
      l.out(true, 4 * F, 8);
      l.out(true, 3 * F, 8);
      l.out(l.opt(), F, 4);      // out_status
    }, 26 * F, 3 * F);
  }
}

}  // namespace

int main() {
  for (int64_t P : {1, 3})
    for (int64_t n_hyp : {1, 2})
      for (int64_t n : {1, 5})     // correspondences per pair: P * n * n_hyp is 1 .. 30, mostly no multiple of 8
        batch_lists(P, n_hyp, n);
  for (int64_t F : {1, 3})
    for (int64_t elem : {1, 2, 4})
      for (int64_t n_points : {1, 13})
        image_lists(F, elem, n_points);
  if (g_failures) {
    std::printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("call arrays: every list counted\n");
  return 0;
}
