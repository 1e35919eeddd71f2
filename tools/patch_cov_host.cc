// The patch-covariance kernel's arithmetic (pnec_amd/csrc/pnec_patch_cov.hpp: patch_point, patch_normalised_gradient,
// patch_accumulate, patch_epilogue) built for the HOST as a stand-alone program, so that an index error shows under the
// address sanitizer here and not as a fault on a device:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipnec_amd/csrc \
//       tools/patch_cov_host.cc -o patch_cov_host
//   patch_cov_host <u8|u16|f32> <height> <width> <pitch> <image.bin> <pts.bin> <pattern.bin> <scaling> <out.bin> [angle.bin]
// image.bin holds exactly (height - 1) * pitch + width pixels and is read into a heap block of exactly that size: NO
// slack behind the last pixel and none in front of the first, so a read one pixel outside is a sanitizer report.
// pts.bin: M x 2 doubles, pattern.bin: P x 2 doubles (P <= 64), angle.bin: M doubles.  out.bin: M rows of 12 doubles --
// cov (xx, xy, yy) | H * scaling (00 01 02 11 12 22) | mean | n_valid | status.  The sums run in the kernel's order:
// point i in position i mod 16, a position's points in ascending i, then the row butterfly (j^1, j^2, 7-j per half, 15-j).
// tests/test_patch_covariance_cpu.py builds it, runs it on every position of the GPU tests' edge case and compares the
// output with the numpy statement of the definition.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pnec_patch_cov.hpp"

using namespace pnec_hip;

namespace {

template <typename T>
T *read_exact(const char *path, size_t count) {
  FILE *f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  T *buf = static_cast<T *>(std::malloc(count * sizeof(T)));
  if (std::fread(buf, sizeof(T), count, f) != count || std::fgetc(f) != EOF) {
    std::fprintf(stderr, "%s does not hold exactly %zu items\n", path, count);
    std::exit(2);
  }
  std::fclose(f);
  return buf;
}

size_t file_doubles(const char *path) {
  FILE *f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fclose(f);
  return (size_t)bytes / sizeof(double);
}

// row_allreduce_sum's order (pnec_device.hpp): every position ends with the same sum; position 0's is returned
double row_sum(const double (&x)[kPatchLanes]) {
  double a[kPatchLanes], b[kPatchLanes];
  for (int j = 0; j < kPatchLanes; ++j) a[j] = x[j] + x[j ^ 1];
  for (int j = 0; j < kPatchLanes; ++j) b[j] = a[j] + a[j ^ 2];
  for (int j = 0; j < kPatchLanes; ++j) a[j] = b[j] + b[(j & 8) | (7 - (j & 7))];
  for (int j = 0; j < kPatchLanes; ++j) b[j] = a[j] + a[15 - j];
  return b[0];
}

template <typename T>
void run(const T *img, int32_t h, int32_t w, int64_t pitch, const double *pts, size_t M, const double *pat, int P,
         double scaling, const double *angle, double *out) {
  for (size_t k = 0; k < M; ++k) {
    double d[kPatchLanes][kPatchSlots], gx[kPatchLanes][kPatchSlots], gy[kPatchLanes][kPatchSlots];
    bool valid[kPatchLanes][kPatchSlots];
    double lS[kPatchLanes], lGx[kPatchLanes], lGy[kPatchLanes];
    int n = 0;
    for (int j = 0; j < kPatchLanes; ++j) {
      lS[j] = lGx[j] = lGy[j] = 0.0;
      for (int s = 0; s < kPatchSlots; ++s) {
        const int i = j + kPatchLanes * s;
        valid[j][s] = false;
        d[j][s] = gx[j][s] = gy[j][s] = 0.0;
        if (i < P)
          valid[j][s] = patch_point(img, pitch, w, h, pts[2 * k] + pat[2 * i], pts[2 * k + 1] + pat[2 * i + 1], d[j][s],
                                    gx[j][s], gy[j][s]);
        lS[j] += d[j][s];
        lGx[j] += gx[j][s];
        lGy[j] += gy[j][s];
        n += valid[j][s] ? 1 : 0;
      }
    }
    const double S = row_sum(lS), Gx = row_sum(lGx), Gy = row_sum(lGy);
    double lH[6][kPatchLanes];
    for (int j = 0; j < kPatchLanes; ++j) {
      double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int s = 0; s < kPatchSlots; ++s) {
        const int i = j + kPatchLanes * s;
        const double gpx = valid[j][s] ? patch_normalised_gradient((double)n, gx[j][s], S, Gx, d[j][s]) : 0.0;
        const double gpy = valid[j][s] ? patch_normalised_gradient((double)n, gy[j][s], S, Gy, d[j][s]) : 0.0;
        patch_accumulate(gpx, gpy, i < P ? pat[2 * i] : 0.0, i < P ? pat[2 * i + 1] : 0.0, H);
      }
      for (int c = 0; c < 6; ++c) lH[c][j] = H[c];
    }
    double H[6];
    for (int c = 0; c < 6; ++c) H[c] = row_sum(lH[c]);
    double cov[3], Hs[6], mean;
    const double cs = angle ? cos(angle[k]) : 1.0, sn = angle ? sin(angle[k]) : 0.0;
    const int status = patch_epilogue(n, S, H, scaling, cs, sn, cov, Hs, mean);
    double *o = out + 12 * k;
    for (int c = 0; c < 3; ++c) o[c] = cov[c];
    for (int c = 0; c < 6; ++c) o[3 + c] = Hs[c];
    o[9] = mean;
    o[10] = (double)n;
    o[11] = (double)status;
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 10 && argc != 11) {
    std::fprintf(stderr, "usage: %s <u8|u16|f32> <height> <width> <pitch> <image.bin> <pts.bin> <pattern.bin> <scaling> "
                         "<out.bin> [angle.bin]\n", argv[0]);
    return 2;
  }
  const std::string type = argv[1];
  const int32_t h = std::atoi(argv[2]), w = std::atoi(argv[3]);
  const int64_t pitch = std::atoll(argv[4]);
  if (h < 1 || w < 1 || pitch < w) {
    std::fprintf(stderr, "bad image shape\n");
    return 2;
  }
  const size_t pixels = (size_t)(h - 1) * (size_t)pitch + (size_t)w;
  const size_t M = file_doubles(argv[6]) / 2, P = file_doubles(argv[7]) / 2;
  if (P < 1 || P > PNEC_HIP_PATCH_MAX_POINTS) {
    std::fprintf(stderr, "pattern must hold 1 .. 64 points\n");
    return 2;
  }
  double *pts = read_exact<double>(argv[6], 2 * M), *pat = read_exact<double>(argv[7], 2 * P);
  double *angle = argc == 11 ? read_exact<double>(argv[10], M) : nullptr;
  const double scaling = std::atof(argv[8]);
  std::vector<double> out(12 * M);
  if (type == "u8") {
    uint8_t *img = read_exact<uint8_t>(argv[5], pixels);
    run(img, h, w, pitch, pts, M, pat, (int)P, scaling, angle, out.data());
    std::free(img);
  } else if (type == "u16") {
    uint16_t *img = read_exact<uint16_t>(argv[5], pixels);
    run(img, h, w, pitch, pts, M, pat, (int)P, scaling, angle, out.data());
    std::free(img);
  } else if (type == "f32") {
    float *img = read_exact<float>(argv[5], pixels);
    run(img, h, w, pitch, pts, M, pat, (int)P, scaling, angle, out.data());
    std::free(img);
  } else {
    std::fprintf(stderr, "unknown pixel type %s\n", type.c_str());
    return 2;
  }
  FILE *f = std::fopen(argv[9], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    std::fprintf(stderr, "cannot write %s\n", argv[9]);
    return 2;
  }
  std::fclose(f);
  std::free(pts);
  std::free(pat);
  std::free(angle);
  std::printf("%zu keypoints, %zu pattern points, %zu pixels without slack\n", M, P, pixels);
  return 0;
}
