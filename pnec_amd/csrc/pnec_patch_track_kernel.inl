// pnec_patch_track_kernel.inl -- the body of the tracker's kernel (pnec_patch_track.hip), included once per variant with
// PNEC_TRACK_TMPL_IMAGE defined as the image of `a.tmpl` that keypoint k builds its templates in: `f`, the keypoint's own
// image, for pnec_hip_patch_track, and the clamped tmpl_image[k] for pnec_hip_patch_track_indexed.  Text, not a function
// template: the plain kernel must keep the machine code it had before the indexed one existed, and handing the kernel's
// argument block to a function by reference changed it (tools/isa_diff_kernels.py).
// A third variant, with PNEC_TRACK_STORED defined (pnec_patch_store.hip), builds no template: it loads what
// pnec_hip_patch_store_add kept of it from slot[k] of `store` (n_slots slots; pnec_patch_store.hpp has the layout), and a
// keypoint without a slot gets a template that is bad at every level.  The text of the other two is what it was.
  PNEC_PATCH_NO_CONTRACT
  const int64_t g = ((int64_t)blockIdx.x * kTrackBlock + threadIdx.x) / kPatchLanes;
  const int j = threadIdx.x & (kPatchLanes - 1);
  const bool live = g < a.n_points;
  const int64_t k = live ? g : a.n_points - 1;   // (n_points >= 1: the ABI layer launches nothing otherwise)

  // which image (pnec_patch_cov.hip's probe; the result is clamped to the images there are)
  const int64_t F = a.n_images;
  int64_t f = (int64_t)((double)k * (double)F / (double)a.n_points);
  f = f < 0 ? 0 : (f > F - 1 ? F - 1 : f);
  if (!(a.offsets[f] <= k && k < a.offsets[f + 1])) {
    int64_t lo = 0, hi = F - 1;   // the last f in [0, F-1] with offsets[f] <= k
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (a.offsets[mid] <= k) lo = mid; else hi = mid - 1;
    }
    f = lo;
  }

  double patx[kPatchSlots], paty[kPatchSlots];
  bool has[kPatchSlots];
#pragma unroll
  for (int s = 0; s < kPatchSlots; ++s) {
    const int i = j + kPatchLanes * s;
    has[s] = i < a.n_pattern;
    patx[s] = has[s] ? a.pattern[2 * i] : 0.0;
    paty[s] = has[s] ? a.pattern[2 * i + 1] : 0.0;
  }
  const double tpx = a.tmpl_pts[2 * k], tpy = a.tmpl_pts[2 * k + 1];
  const double ix0 = a.init_pts ? a.init_pts[2 * k] : tpx, iy0 = a.init_pts ? a.init_pts[2 * k + 1] : tpy;
  double tx = ix0 + a.shift_x, ty = iy0 + a.shift_y, theta = a.init_angle ? a.init_angle[k] : 0.0;
  double fx = tx, fy = ty, fth = theta;   // the forward result
  int status = PNEC_HIP_TRACK_OK, lost_level = -1;
  bool alive = true;
  int n0 = 0;                             // the level-0 template's sums: the covariance's
  double S0 = 0.0, H0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int half = a.n_pattern / 2;
  const int n_dirs = a.backward ? 2 : 1;
#if defined(PNEC_TRACK_STORED)
  const int64_t slot_k = (int64_t)slot[k];
  const bool has_slot = slot_k >= 0 && slot_k < n_slots;
  const double *const slot_words = store + (has_slot ? slot_k : 0) * store_slot_doubles(a.n_levels);
#endif

#pragma unroll 1
  for (int dir = 0; dir < n_dirs; ++dir) {
    const TrackPyramid &pyr = dir ? a.prev : a.next;
    if (dir && alive) {
      tx = tx - a.shift_x;
      ty = ty - a.shift_y;
    }
#pragma unroll 1
    for (int l = a.n_levels - 1; l >= 0; --l) {
      const int32_t wl = a.w >> l, hl = a.h >> l;
      const double scale = (double)(1 << l);
#if defined(PNEC_TRACK_STORED)
      // ---- the template of this level, as pnec_hip_patch_store_add left it: lane j's slot s is element j + 16 s
      double data[kPatchSlots], K[kPatchSlots][3];
      bool tvalid[kPatchSlots];
      {
        int tstat = PNEC_HIP_PATCH_EMPTY;
        uint64_t valid = 0ull;
        const double *const plane = slot_words + kStoreHeader + l * kStoreLevel;
#pragma unroll
        for (int s = 0; s < kPatchSlots; ++s) {
          data[s] = 0.0;
          K[s][0] = 0.0;
          K[s][1] = 0.0;
          K[s][2] = 0.0;
        }
        if (has_slot) {
          tstat = (int)reinterpret_cast<const int64_t *>(slot_words)[kStoreWordStatus + l];
          valid = reinterpret_cast<const uint64_t *>(slot_words)[kStoreWordValid + l];
#pragma unroll
          for (int s = 0; s < kPatchSlots; ++s) {
            const int i = j + kPatchLanes * s;
            data[s] = plane[i];
            K[s][0] = plane[kStorePlane + i];
            K[s][1] = plane[2 * kStorePlane + i];
            K[s][2] = plane[3 * kStorePlane + i];
          }
          if (l == 0) {
            n0 = (int)reinterpret_cast<const int64_t *>(slot_words)[kStoreWordN];
            S0 = slot_words[kStoreWordS];
#pragma unroll
            for (int c = 0; c < 6; ++c) H0[c] = slot_words[kStoreWordH + c];
          }
        }
#pragma unroll
        for (int s = 0; s < kPatchSlots; ++s) tvalid[s] = ((valid >> (j + kPatchLanes * s)) & 1ull) != 0ull;
        if (alive && tstat != PNEC_HIP_PATCH_OK) {
          alive = false;
          status = PNEC_HIP_TRACK_BAD_TEMPLATE;
          lost_level = l;
        }
      }
#else
      // ---- the template of this level: pnec_patch_cov.hip's two phases, term by term
      const T *timg = reinterpret_cast<const T *>(a.tmpl.level[l]) + PNEC_TRACK_TMPL_IMAGE * (int64_t)hl * a.tmpl.pitch[l];
      const int64_t tpitch = a.tmpl.pitch[l];
      const double qx = tpx / scale, qy = tpy / scale;
      double data[kPatchSlots], K[kPatchSlots][3];
      bool tvalid[kPatchSlots];
      {
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
        for (int c = 0; c < 6; ++c) H[c] = row_allreduce_sum(H[c]);
        double Hi[6];
        const int tstat = patch_inverse3(n, S, H, Hi);
#pragma unroll
        for (int s = 0; s < kPatchSlots; ++s) {
          data[s] = track_normalised_value(nd, d[s], S);
          track_gain(Hi, gpx[s], gpy[s], patx[s], paty[s], K[s]);
        }
        if (l == 0) {
          n0 = n;
          S0 = S;
#pragma unroll
          for (int c = 0; c < 6; ++c) H0[c] = H[c];
        }
        if (alive && tstat != PNEC_HIP_PATCH_OK) {
          alive = false;
          status = PNEC_HIP_TRACK_BAD_TEMPLATE;
          lost_level = l;
        }
      }
#endif
      // ---- the iterations of this level
      const T *img = reinterpret_cast<const T *>(pyr.level[l]) + f * (int64_t)hl * pyr.pitch[l];
      const int64_t pitch = pyr.pitch[l];
      const bool started = alive;
      double lx = tx / scale, ly = ty / scale;
#pragma unroll 1
      for (int it = 0; it < a.max_iterations; ++it) {
        if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
        double sn, cs;
        sincos_bounded(theta, sn, cs);
        double v[kPatchSlots];
        bool both[kPatchSlots];
        double S2 = 0.0;
        int cnt = 0;   // valid points in the low half, points valid here and in the template in the high half
#pragma unroll
        for (int s = 0; s < kPatchSlots; ++s) {
          double px, py;
          track_warp(cs, sn, lx, ly, patx[s], paty[s], px, py);
          v[s] = 0.0;
          bool val = false;
          if (has[s]) val = patch_value(img, pitch, wl, hl, px, py, v[s]);
          both[s] = val && tvalid[s];
          S2 += v[s];
          cnt += (val ? 1 : 0) + (both[s] ? 0x10000 : 0);
        }
        S2 = row_allreduce_sum(S2);
        cnt = track_row_sum_i(cnt);
        const int n2 = cnt & 0xffff, m = cnt >> 16;
        const bool ok = m > half && S2 > 0.0 && S2 <= 1.7976931348623157e308;
        const double n2d = (double)n2;
        double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < kPatchSlots; ++s) {
          const double r = both[s] ? track_normalised_value(n2d, v[s], S2) - data[s] : 0.0;
          track_accumulate(K[s], r, acc);
        }
        const double inc0 = -row_allreduce_sum(acc[0]), inc1 = -row_allreduce_sum(acc[1]);
        const double inc2 = -row_allreduce_sum(acc[2]);
        double sd, cd;
        sincos_bounded(inc2, sd, cd);
        double nx = lx, ny = ly, nth = theta;
        track_step(cs, sn, cd, sd, inc0, inc1, inc2, nx, ny, nth);
        const bool inside = track_in_bounds(wl, hl, nx, ny) && fabs(inc2) < 1.0e6 && fabs(nth) < 1.0e6;
        if (alive) {
          if (ok) {   // (a step from an unusable residual is not taken: the transform stays where it was)
            lx = nx;
            ly = ny;
            theta = nth;
          }
          if (!ok || !inside) {
            alive = false;
            status = dir ? PNEC_HIP_TRACK_LOST_BACKWARD : PNEC_HIP_TRACK_LOST_FORWARD;
            lost_level = l;
          }
        }
      }
      if (started) {
        tx = lx * scale;
        ty = ly * scale;
      }
      if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
    }
    if (dir == 0) {
      fx = tx;
      fy = ty;
      fth = theta;
    }
    if (__builtin_amdgcn_ballot_w64(alive) == 0ull) break;
  }

  const double nan = (double)NAN;
  double dist2 = nan;
  if (a.backward && alive) {
    const double ex = ix0 - tx, ey = iy0 - ty;
    const double ex2 = ex * ex, ey2 = ey * ey;
    dist2 = ex2 + ey2;
    if (!(dist2 < a.max_recovered_dist2)) status = PNEC_HIP_TRACK_RECOVERED_TOO_FAR;
  }
  double cs = 1.0, sn = 0.0;
  sincos_bounded(fth, sn, cs);
  double cov[3], Hs[6], mean;
  const int cstat = patch_epilogue(n0, S0, H0, a.scaling, cs, sn, cov, Hs, mean);
  if (status != PNEC_HIP_TRACK_OK || cstat != PNEC_HIP_PATCH_OK) {
    cov[0] = nan;
    cov[1] = nan;
    cov[2] = nan;
  }
  if (live) {
    if (a.out_pts && j < 2) a.out_pts[2 * k + j] = j == 0 ? fx : fy;
    if (a.out_cov && j < 3) a.out_cov[3 * k + j] = j == 0 ? cov[0] : (j == 1 ? cov[1] : cov[2]);
    if (j == 0) {
      if (a.out_angle) a.out_angle[k] = fth;
      if (a.out_dist2) a.out_dist2[k] = dist2;
      if (a.out_status) a.out_status[k] = status;
      if (a.out_lost_level) a.out_lost_level[k] = lost_level;
    }
  }
