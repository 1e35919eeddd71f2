// The patch tracker's and the pyramid's arithmetic (pnec_amd/csrc/pnec_patch_track.hpp and pnec_patch_cov.hpp) built for
// the HOST as a stand-alone program, so that an index error shows under the address sanitizer here and not as a fault on a
// device:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipnec_amd/csrc \
//       tools/patch_track_host.cc -o patch_track_host
//   patch_track_host track <job.bin> <out.bin>
//   patch_track_host pyr <u8|u16|f32> <height> <width> <pitch_in> <pitch_out> <in.bin> <out.bin>
// job.bin: 12 int64 -- pixel type (0 u8, 1 u16, 2 f32), F, h, w, L, M, P, max_iterations, flags, has_prev, has_init_pts,
// has_init_angle -- then 4 doubles (shift_x, shift_y, max_recovered_dist2, scaling), 3 x L int64 pitches (tmpl, prev,
// next), F + 1 int64 offsets, 2M doubles tmpl_pts, [2M init_pts], [M init_angle], 2P pattern, then the levels of tmpl,
// [prev,] next, level 0 first, each EXACTLY (F h_l - 1) pitch_l + w_l pixels.  Every level is read into a heap block of
// exactly that size: NO slack behind the last pixel and none in front of the first, so a read one pixel outside is a
// sanitizer report.  out.bin: M rows of 9 doubles -- pts (x, y) | angle | cov (xx, xy, yy) | dist2 | status | lost_level.
// The control flow and the order of every sum are the kernel's (pnec_patch_track.hip): point i in position i mod 16, a
// position's points in ascending i, then the row butterfly (j^1, j^2, 7-j per half, 15-j).  Sine and cosine come from
// libm here.  tests/test_patch_track_cpu.py builds it, runs it on every keypoint of the GPU tests' fixtures and compares
// the output with the numpy statement of the definition.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pnec_patch_track.hpp"

using namespace pnec_hip;

namespace {

struct Reader {
  FILE *f;
  explicit Reader(const char *path) : f(std::fopen(path, "rb")) {
    if (!f) {
      std::fprintf(stderr, "cannot open %s\n", path);
      std::exit(2);
    }
  }
  // `count` items in a heap block of exactly that size
  template <typename T>
  T *take(size_t count) {
    T *buf = static_cast<T *>(std::malloc(count ? count * sizeof(T) : 1));
    if (std::fread(buf, sizeof(T), count, f) != count) {
      std::fprintf(stderr, "the file ends early\n");
      std::exit(2);
    }
    return buf;
  }
  void done() {
    if (std::fgetc(f) != EOF) {
      std::fprintf(stderr, "the file holds more than it should\n");
      std::exit(2);
    }
    std::fclose(f);
  }
};

double row_sum(const double (&x)[kPatchLanes]) {
  double a[kPatchLanes], b[kPatchLanes];
  for (int j = 0; j < kPatchLanes; ++j) a[j] = x[j] + x[j ^ 1];
  for (int j = 0; j < kPatchLanes; ++j) b[j] = a[j] + a[j ^ 2];
  for (int j = 0; j < kPatchLanes; ++j) a[j] = b[j] + b[(j & 8) | (7 - (j & 7))];
  for (int j = 0; j < kPatchLanes; ++j) b[j] = a[j] + a[15 - j];
  return b[0];
}

struct Job {
  int64_t F, h, w, L, M, P, max_it, flags;
  double shift_x, shift_y, max_d2, scaling;
  int64_t *pitch[3];
  int64_t *offsets;
  double *tmpl_pts, *init_pts, *init_angle, *pattern;
  void *level[3][PNEC_HIP_TRACK_MAX_LEVELS];   // tmpl, prev, next
};

template <typename T>
void track(const Job &J, double *out) {
  const int P = (int)J.P, half = P / 2;
  const double nan = (double)NAN;
  for (int64_t k = 0; k < J.M; ++k) {
    int64_t f = 0;
    while (f < J.F - 1 && !(J.offsets[f] <= k && k < J.offsets[f + 1])) ++f;
    const double tpx = J.tmpl_pts[2 * k], tpy = J.tmpl_pts[2 * k + 1];
    const double ix0 = J.init_pts ? J.init_pts[2 * k] : tpx, iy0 = J.init_pts ? J.init_pts[2 * k + 1] : tpy;
    double tx = ix0 + J.shift_x, ty = iy0 + J.shift_y, theta = J.init_angle ? J.init_angle[k] : 0.0;
    double fx = tx, fy = ty, fth = theta;
    int status = PNEC_HIP_TRACK_OK, lost_level = -1;
    bool alive = true;
    int n0 = 0;
    double S0 = 0.0, H0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int n_dirs = (J.flags & PNEC_HIP_TRACK_NO_BACKWARD) ? 1 : 2;
    for (int dir = 0; dir < n_dirs && alive; ++dir) {
      const int which = dir ? 1 : 2;
      if (dir) {
        tx = tx - J.shift_x;
        ty = ty - J.shift_y;
      }
      for (int l = (int)J.L - 1; l >= 0 && alive; --l) {
        const int32_t wl = (int32_t)(J.w >> l), hl = (int32_t)(J.h >> l);
        const double scale = (double)(1 << l);
        const int64_t tpitch = J.pitch[0][l], pitch = J.pitch[which][l];
        const T *timg = static_cast<const T *>(J.level[0][l]) + f * (int64_t)hl * tpitch;
        const T *img = static_cast<const T *>(J.level[which][l]) + f * (int64_t)hl * pitch;
        const double qx = tpx / scale, qy = tpy / scale;
        double d[kPatchLanes][kPatchSlots], gx[kPatchLanes][kPatchSlots], gy[kPatchLanes][kPatchSlots];
        double patx[kPatchLanes][kPatchSlots], paty[kPatchLanes][kPatchSlots];
        bool tvalid[kPatchLanes][kPatchSlots], has[kPatchLanes][kPatchSlots];
        double lS[kPatchLanes], lGx[kPatchLanes], lGy[kPatchLanes];
        int n = 0;
        for (int j = 0; j < kPatchLanes; ++j) {
          lS[j] = lGx[j] = lGy[j] = 0.0;
          for (int s = 0; s < kPatchSlots; ++s) {
            const int i = j + kPatchLanes * s;
            has[j][s] = i < P;
            patx[j][s] = has[j][s] ? J.pattern[2 * i] : 0.0;
            paty[j][s] = has[j][s] ? J.pattern[2 * i + 1] : 0.0;
            tvalid[j][s] = false;
            d[j][s] = gx[j][s] = gy[j][s] = 0.0;
            if (has[j][s])
              tvalid[j][s] = patch_point(timg, tpitch, wl, hl, qx + patx[j][s], qy + paty[j][s], d[j][s], gx[j][s], gy[j][s]);
            lS[j] += d[j][s];
            lGx[j] += gx[j][s];
            lGy[j] += gy[j][s];
            n += tvalid[j][s] ? 1 : 0;
          }
        }
        const double S = row_sum(lS), Gx = row_sum(lGx), Gy = row_sum(lGy), nd = (double)n;
        double gpx[kPatchLanes][kPatchSlots], gpy[kPatchLanes][kPatchSlots], lH[6][kPatchLanes];
        for (int j = 0; j < kPatchLanes; ++j) {
          double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
          for (int s = 0; s < kPatchSlots; ++s) {
            gpx[j][s] = tvalid[j][s] ? patch_normalised_gradient(nd, gx[j][s], S, Gx, d[j][s]) : 0.0;
            gpy[j][s] = tvalid[j][s] ? patch_normalised_gradient(nd, gy[j][s], S, Gy, d[j][s]) : 0.0;
            patch_accumulate(gpx[j][s], gpy[j][s], patx[j][s], paty[j][s], H);
          }
          for (int c = 0; c < 6; ++c) lH[c][j] = H[c];
        }
        double H[6], Hi[6];
        for (int c = 0; c < 6; ++c) H[c] = row_sum(lH[c]);
        const int tstat = patch_inverse3(n, S, H, Hi);
        double data[kPatchLanes][kPatchSlots], K[kPatchLanes][kPatchSlots][3];
        for (int j = 0; j < kPatchLanes; ++j)
          for (int s = 0; s < kPatchSlots; ++s) {
            data[j][s] = track_normalised_value(nd, d[j][s], S);
            track_gain(Hi, gpx[j][s], gpy[j][s], patx[j][s], paty[j][s], K[j][s]);
          }
        if (l == 0) {
          n0 = n;
          S0 = S;
          for (int c = 0; c < 6; ++c) H0[c] = H[c];
        }
        if (tstat != PNEC_HIP_PATCH_OK) {
          alive = false;
          status = PNEC_HIP_TRACK_BAD_TEMPLATE;
          lost_level = l;
          break;
        }
        double lx = tx / scale, ly = ty / scale;
        for (int it = 0; it < (int)J.max_it && alive; ++it) {
          const double cs = cos(theta), sn = sin(theta);
          double v[kPatchLanes][kPatchSlots], lS2[kPatchLanes];
          bool both[kPatchLanes][kPatchSlots];
          int n2 = 0, m = 0;
          for (int j = 0; j < kPatchLanes; ++j) {
            lS2[j] = 0.0;
            for (int s = 0; s < kPatchSlots; ++s) {
              double px, py;
              track_warp(cs, sn, lx, ly, patx[j][s], paty[j][s], px, py);
              v[j][s] = 0.0;
              bool val = false;
              if (has[j][s]) val = patch_value(img, pitch, wl, hl, px, py, v[j][s]);
              both[j][s] = val && tvalid[j][s];
              lS2[j] += v[j][s];
              n2 += val ? 1 : 0;
              m += both[j][s] ? 1 : 0;
            }
          }
          const double S2 = row_sum(lS2);
          const bool ok = m > half && S2 > 0.0 && S2 <= 1.7976931348623157e308;
          double la[3][kPatchLanes];
          for (int j = 0; j < kPatchLanes; ++j) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int s = 0; s < kPatchSlots; ++s) {
              const double r = both[j][s] ? track_normalised_value((double)n2, v[j][s], S2) - data[j][s] : 0.0;
              track_accumulate(K[j][s], r, acc);
            }
            for (int c = 0; c < 3; ++c) la[c][j] = acc[c];
          }
          const double inc0 = -row_sum(la[0]), inc1 = -row_sum(la[1]), inc2 = -row_sum(la[2]);
          double nx = lx, ny = ly, nth = theta;
          track_step(cs, sn, cos(inc2), sin(inc2), inc0, inc1, inc2, nx, ny, nth);
          const bool inside = track_in_bounds(wl, hl, nx, ny) && fabs(inc2) < 1.0e6 && fabs(nth) < 1.0e6;
          if (ok) {
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
        tx = lx * scale;
        ty = ly * scale;
      }
      if (dir == 0) {
        fx = tx;
        fy = ty;
        fth = theta;
      }
    }
    double dist2 = nan;
    if (n_dirs == 2 && alive) {
      const double ex = ix0 - tx, ey = iy0 - ty;
      const double ex2 = ex * ex, ey2 = ey * ey;
      dist2 = ex2 + ey2;
      if (!(dist2 < J.max_d2)) status = PNEC_HIP_TRACK_RECOVERED_TOO_FAR;
    }
    double cov[3], Hs[6], mean;
    const int cstat = patch_epilogue(n0, S0, H0, J.scaling, cos(fth), sin(fth), cov, Hs, mean);
    if (status != PNEC_HIP_TRACK_OK || cstat != PNEC_HIP_PATCH_OK) cov[0] = cov[1] = cov[2] = nan;
    double *o = out + 9 * k;
    o[0] = fx;
    o[1] = fy;
    o[2] = fth;
    o[3] = cov[0];
    o[4] = cov[1];
    o[5] = cov[2];
    o[6] = dist2;
    o[7] = (double)status;
    o[8] = (double)lost_level;
  }
}

template <typename T>
size_t run_track(Reader &r, Job &J, double *out) {
  size_t pixels = 0;
  const bool has_prev = J.level[1][0] != nullptr;   // (a marker set by main)
  for (int y = 0; y < 3; ++y) {
    if (y == 1 && !has_prev) continue;
    for (int l = 0; l < (int)J.L; ++l) {
      const size_t count = (size_t)(J.F * (J.h >> l) - 1) * (size_t)J.pitch[y][l] + (size_t)(J.w >> l);
      J.level[y][l] = r.take<T>(count);
      pixels += count;
    }
  }
  r.done();
  if (!has_prev)
    for (int l = 0; l < (int)J.L; ++l) J.level[1][l] = J.level[0][l];
  track<T>(J, out);
  for (int y = 0; y < 3; ++y)
    for (int l = 0; l < (int)J.L; ++l)
      if (y != 1 || has_prev) std::free(J.level[y][l]);
  return pixels;
}

template <typename T>
int run_pyr(int32_t h, int32_t w, int64_t pin, int64_t pout, const char *in_path, const char *out_path) {
  const size_t n_in = (size_t)(h - 1) * (size_t)pin + (size_t)w, n_out = (size_t)(h / 2 - 1) * (size_t)pout + (size_t)(w / 2);
  Reader r(in_path);
  T *in = r.take<T>(n_in);
  r.done();
  T *out = static_cast<T *>(std::calloc(n_out, sizeof(T)));
  for (int32_t y = 0; y < h / 2; ++y)
    for (int32_t x = 0; x < w / 2; ++x) out[(int64_t)y * pout + x] = pyr_pixel(in, pin, w, h, x, y);
  FILE *f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(out, sizeof(T), n_out, f) != n_out) {
    std::fprintf(stderr, "cannot write %s\n", out_path);
    return 2;
  }
  std::fclose(f);
  std::free(in);
  std::free(out);
  std::printf("pyramid level: %zu pixels in, %zu out, without slack\n", n_in, n_out);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "pyr" && argc == 9) {
    const std::string type = argv[2];
    const int32_t h = std::atoi(argv[3]), w = std::atoi(argv[4]);
    const int64_t pin = std::atoll(argv[5]), pout = std::atoll(argv[6]);
    if (h < 4 || w < 4 || pin < w || pout < w / 2) {
      std::fprintf(stderr, "bad image shape\n");
      return 2;
    }
    if (type == "u8") return run_pyr<uint8_t>(h, w, pin, pout, argv[7], argv[8]);
    if (type == "u16") return run_pyr<uint16_t>(h, w, pin, pout, argv[7], argv[8]);
    if (type == "f32") return run_pyr<float>(h, w, pin, pout, argv[7], argv[8]);
    std::fprintf(stderr, "unknown pixel type %s\n", type.c_str());
    return 2;
  }
  if (mode != "track" || argc != 4) {
    std::fprintf(stderr, "usage: %s track <job.bin> <out.bin> | pyr <u8|u16|f32> <height> <width> <pitch_in> <pitch_out> "
                         "<in.bin> <out.bin>\n", argv[0]);
    return 2;
  }
  Reader r(argv[2]);
  int64_t *head = r.take<int64_t>(12);
  double *par = r.take<double>(4);
  Job J;
  std::memset(&J, 0, sizeof(J));
  const int64_t ptype = head[0];
  J.F = head[1], J.h = head[2], J.w = head[3], J.L = head[4], J.M = head[5], J.P = head[6], J.max_it = head[7];
  J.flags = head[8];
  const bool has_prev = head[9] != 0, has_init_pts = head[10] != 0, has_init_angle = head[11] != 0;
  if (J.F < 1 || J.L < 1 || J.L > PNEC_HIP_TRACK_MAX_LEVELS || J.M < 0 || J.P < 1 || J.P > PNEC_HIP_PATCH_MAX_POINTS ||
      (J.h >> (J.L - 1)) < 4 || (J.w >> (J.L - 1)) < 4) {
    std::fprintf(stderr, "bad job header\n");
    return 2;
  }
  J.shift_x = par[0], J.shift_y = par[1], J.max_d2 = par[2], J.scaling = par[3];
  for (int y = 0; y < 3; ++y) J.pitch[y] = r.take<int64_t>((size_t)J.L);
  for (int y = 0; y < 3; ++y)
    for (int l = 0; l < (int)J.L; ++l)
      if (J.pitch[y][l] < (J.w >> l)) {
        std::fprintf(stderr, "a pitch is below its level's width\n");
        return 2;
      }
  J.offsets = r.take<int64_t>((size_t)J.F + 1);
  J.tmpl_pts = r.take<double>(2 * (size_t)J.M);
  J.init_pts = has_init_pts ? r.take<double>(2 * (size_t)J.M) : nullptr;
  J.init_angle = has_init_angle ? r.take<double>((size_t)J.M) : nullptr;
  J.pattern = r.take<double>(2 * (size_t)J.P);
  static char marker;
  J.level[1][0] = has_prev ? &marker : nullptr;
  std::vector<double> out(9 * (size_t)J.M);
  size_t pixels = 0;
  if (ptype == PNEC_HIP_PIXEL_U8) pixels = run_track<uint8_t>(r, J, out.data());
  else if (ptype == PNEC_HIP_PIXEL_U16) pixels = run_track<uint16_t>(r, J, out.data());
  else if (ptype == PNEC_HIP_PIXEL_F32) pixels = run_track<float>(r, J, out.data());
  else {
    std::fprintf(stderr, "unknown pixel type\n");
    return 2;
  }
  FILE *f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  std::fclose(f);
  std::free(head);
  std::free(par);
  for (int y = 0; y < 3; ++y) std::free(J.pitch[y]);
  std::free(J.offsets);
  std::free(J.tmpl_pts);
  std::free(J.init_pts);
  std::free(J.init_angle);
  std::free(J.pattern);
  std::printf("%lld keypoints, %lld pattern points, %lld levels, %zu pixels without slack\n", (long long)J.M, (long long)J.P,
              (long long)J.L, pixels);
  return 0;
}
