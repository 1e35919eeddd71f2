// The keypoint detector's arithmetic (pnec_amd/csrc/pnec_detect.hpp) built for the HOST as a stand-alone program, so that
// an index error shows under the address sanitizer here and not as a fault on a device:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ipnec_amd/csrc \
//       tools/detect_host.cc -o detect_host
//   detect_host <job.bin> <out.bin>
// job.bin: 11 int64 -- pixel type (0 u8, 1 u16), F, h, w, pitch, G, K, T, E, n_cur, has_cur -- then, with has_cur, F + 1
// int64 cur_offsets and 2 n_cur doubles cur_pts, then the images, EXACTLY (F h - 1) pitch + w pixels.  The images are
// read into a heap block of exactly that size, and every cell's two byte maps are heap blocks of exactly G G bytes: NO
// slack, so a read one pixel outside the image or the cell is a sanitizer report.
// out.bin, all int64: N | out_cell F n_cells | out_offsets F + 1 | N rows of x, y, score, cell_index.
// The control flow is the kernels' (pnec_detect.hip): mark, search (64 lanes striding over the cell, four sorted keys per
// lane, K rounds of a maximum over the lanes with the winner's lane dropping its key), the packed count in out_cell,
// count, scan, emit (a cell with one point unpacked, a cell with more searched again), finish.  It also checks the
// division by multiplication for every divisor and index the kernels can meet.  tests/test_detect_keypoints_cpu.py builds
// it, runs it on the GPU tests' fixtures and compares the output with the numpy statement of the definition.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pnec_detect.hpp"

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

// search_cell of pnec_detect.hip for one (image, cell)
template <typename T>
void search_cell(const DetectArgs &a, int64_t f, int c, uint32_t (&win)[kDetectMaxPerCell]) {
  const int G = a.grid, GG = G * G, GI = G - 2 * kDetectBorder, GII = GI * GI;
  const uint32_t inv = detect_inverse(G), inv_i = detect_inverse(GI);
  const int cx = c / a.ny, cy = c - cx * a.ny;
  const int X0 = a.x_start + cx * G, Y0 = a.y_start + cy * G;
  uint8_t *cell = static_cast<uint8_t *>(std::malloc((size_t)GG)), *mm = static_cast<uint8_t *>(std::malloc((size_t)GG));
  const T *img = reinterpret_cast<const T *>(a.images) + (f * (int64_t)a.h + Y0) * a.pitch + X0;
  for (int lane = 0; lane < kDetectLanes; ++lane)
    for (int i = lane; i < GG; i += kDetectLanes) {
      const int y = detect_div(i, inv), x = i - y * G;
      cell[i] = detect_pixel(img[(int64_t)y * a.pitch + x]);
      mm[i] = 0;
    }
  for (int lane = 0; lane < kDetectLanes; ++lane)
    for (int j = lane; j < GII; j += kDetectLanes) {
      const int yy = detect_div(j, inv_i);
      const int idx = (yy + kDetectBorder) * G + (j - yy * GI) + kDetectBorder;
      mm[idx] = (uint8_t)detect_measure(cell + idx, G, a.thr);
    }
  uint32_t k[kDetectLanes][4];
  for (int lane = 0; lane < kDetectLanes; ++lane) {
    for (int r = 0; r < 4; ++r) k[lane][r] = 0u;
    for (int j = lane; j < GII; j += kDetectLanes) {
      const int yy = detect_div(j, inv_i), xx = j - yy * GI;
      const int y = yy + kDetectBorder, x = xx + kDetectBorder, idx = y * G + x;
      if (detect_is_peak(mm, idx, G, a.thr) && detect_in_bounds(X0 + x, Y0 + y, a.w, a.h, a.edge))
        detect_insert(detect_key(mm[idx], idx), k[lane]);
    }
  }
  for (int r = 0; r < kDetectMaxPerCell; ++r) {
    win[r] = 0u;
    if (r < a.per_cell) {
      uint32_t best = 0u;
      for (int lane = 0; lane < kDetectLanes; ++lane) best = k[lane][0] > best ? k[lane][0] : best;
      win[r] = best;
      for (int lane = 0; lane < kDetectLanes; ++lane)
        if (best != 0u && k[lane][0] == best) {
          k[lane][0] = k[lane][1];
          k[lane][1] = k[lane][2];
          k[lane][2] = k[lane][3];
          k[lane][3] = 0u;
        }
    }
  }
  std::free(cell);
  std::free(mm);
}

template <typename T>
void detect(const DetectArgs &a) {
  const int n_cells = a.nx * a.ny;
  const int64_t n_units = a.n_images * n_cells;
  const bool marked = a.cur_offsets && a.cur_pts && a.n_cur > 0;
  if (marked) {
    for (int64_t u = 0; u < n_units; ++u) a.out_cell[u] = 0;
    for (int64_t i = 0; i < a.n_cur; ++i) {
      int64_t lo = 0, hi = a.n_images - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (a.cur_offsets[mid] <= i) lo = mid; else hi = mid - 1;
      }
      const int c = detect_point_cell(a.cur_pts[2 * i], a.cur_pts[2 * i + 1], a.x_start, a.y_start, a.nx, a.ny, a.grid);
      if (c >= 0) a.out_cell[lo * n_cells + c] = -1;
    }
  }
  for (int64_t u = 0; u < n_units; ++u) {
    if (marked && a.out_cell[u] < 0) continue;
    uint32_t win[kDetectMaxPerCell];
    search_cell<T>(a, u / n_cells, (int)(u % n_cells), win);
    int count = 0;
    for (int r = 0; r < kDetectMaxPerCell; ++r) count += win[r] != 0u ? 1 : 0;
    a.out_cell[u] = detect_pack(count, win[0]);
  }
  for (int64_t f = 0; f < a.n_images; ++f) {
    int sum = 0;
    for (int c = 0; c < n_cells; ++c) sum += detect_packed_count(a.out_cell[f * n_cells + c]);
    a.out_offsets[f + 1] = sum;
  }
  for (int64_t f = 0; f < a.n_images; ++f) a.out_offsets[f + 1] += f > 0 ? a.out_offsets[f] : 0;
  a.out_offsets[0] = 0;
  for (int64_t u = 0; u < n_units; ++u) {
    const int64_t f = u / n_cells;
    const int c = (int)(u % n_cells);
    const int32_t packed = a.out_cell[u];
    const int count = detect_packed_count(packed);
    if (count == 0) continue;
    int before = 0;
    for (int i = 0; i < c; ++i) before += detect_packed_count(a.out_cell[f * n_cells + i]);
    uint32_t win[kDetectMaxPerCell] = {detect_packed_key(packed), 0u, 0u, 0u};
    if (count > 1) search_cell<T>(a, f, c, win);
    for (int lane = 0; lane < count; ++lane) {
      const uint32_t key = win[lane];
      const int idx = detect_key_index(key);
      const int y = detect_div(idx, detect_inverse(a.grid)), x = idx - y * a.grid;
      const int cx = c / a.ny, cy = c - cx * a.ny;
      const int64_t at = a.out_offsets[f] + before + lane;
      a.out_pts[2 * at] = (double)(a.x_start + cx * a.grid + x);
      a.out_pts[2 * at + 1] = (double)(a.y_start + cy * a.grid + y);
      a.out_score[at] = detect_key_m(key) - 1;
      a.out_cell_index[at] = c;
    }
  }
  for (int64_t u = 0; u < n_units; ++u)
    if (a.out_cell[u] > 0) a.out_cell[u] = detect_packed_count(a.out_cell[u]);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: detect_host <job.bin> <out.bin>\n");
    return 2;
  }
  // the division by multiplication, for every divisor and index of search_cell and of the emit step
  for (int d = kDetectMinGrid - 2 * kDetectBorder; d <= kDetectMaxGrid; ++d)
    for (int i = 0; i < kDetectMaxGrid * kDetectMaxGrid; ++i)
      if (detect_div(i, detect_inverse(d)) != i / d) {
        std::fprintf(stderr, "detect_div(%d, %d) is wrong\n", i, d);
        return 3;
      }
  Reader in(argv[1]);
  int64_t *hd = in.take<int64_t>(11);
  const int64_t ptype = hd[0], F = hd[1], h = hd[2], w = hd[3], pitch = hd[4], G = hd[5], K = hd[6], T = hd[7], E = hd[8],
                n_cur = hd[9], has_cur = hd[10];
  std::free(hd);
  if ((ptype != 0 && ptype != 1) || F < 1 || G < kDetectMinGrid || G > kDetectMaxGrid || h < G || w < G || pitch < w ||
      K < 1 || K > kDetectMaxPerCell || T < 0 || T > kDetectMaxThreshold || E < 0 || n_cur < 0) {
    std::fprintf(stderr, "bad job header\n");
    return 2;
  }
  DetectArgs a{};
  a.cur_offsets = has_cur ? in.take<int64_t>((size_t)F + 1) : nullptr;
  a.cur_pts = has_cur ? in.take<double>(2 * (size_t)n_cur) : nullptr;
  a.n_cur = has_cur ? n_cur : 0;
  const size_t pixels = (size_t)((F * h - 1) * pitch + w);
  a.images = ptype == 0 ? static_cast<void *>(in.take<uint8_t>(pixels)) : static_cast<void *>(in.take<uint16_t>(pixels));
  in.done();
  a.w = (int32_t)w;
  a.h = (int32_t)h;
  a.pitch = pitch;
  a.n_images = F;
  a.grid = (int32_t)G;
  a.per_cell = (int32_t)K;
  a.thr = (int32_t)T;
  a.edge = (int32_t)E;
  a.nx = (int32_t)(w / G);
  a.ny = (int32_t)(h / G);
  a.x_start = (int32_t)((w % G) / 2);
  a.y_start = (int32_t)((h % G) / 2);
  const int64_t n_cells = (int64_t)a.nx * a.ny, cap = F * n_cells * K;
  // outputs in heap blocks of exactly their size, filled with a value the detector never writes
  a.out_cell = static_cast<int32_t *>(std::malloc(sizeof(int32_t) * (size_t)(F * n_cells)));
  a.out_offsets = static_cast<int64_t *>(std::malloc(sizeof(int64_t) * (size_t)(F + 1)));
  a.out_pts = static_cast<double *>(std::malloc(sizeof(double) * 2 * (size_t)cap));
  a.out_score = static_cast<int32_t *>(std::malloc(sizeof(int32_t) * (size_t)cap));
  a.out_cell_index = static_cast<int32_t *>(std::malloc(sizeof(int32_t) * (size_t)cap));
  for (int64_t i = 0; i < F * n_cells; ++i) a.out_cell[i] = -77;
  for (int64_t i = 0; i < cap; ++i) {
    a.out_pts[2 * i] = a.out_pts[2 * i + 1] = -77.0;
    a.out_score[i] = a.out_cell_index[i] = -77;
  }
  if (ptype == 0) detect<uint8_t>(a); else detect<uint16_t>(a);
  const int64_t N = a.out_offsets[F];
  for (int64_t i = N; i < cap; ++i)
    if (a.out_pts[2 * i] != -77.0 || a.out_pts[2 * i + 1] != -77.0 || a.out_score[i] != -77 || a.out_cell_index[i] != -77) {
      std::fprintf(stderr, "entry %lld beyond the last point was written\n", (long long)i);
      return 3;
    }
  std::vector<int64_t> out;
  out.push_back(N);
  for (int64_t i = 0; i < F * n_cells; ++i) out.push_back(a.out_cell[i]);
  for (int64_t i = 0; i <= F; ++i) out.push_back(a.out_offsets[i]);
  for (int64_t i = 0; i < N; ++i) {
    out.push_back((int64_t)a.out_pts[2 * i]);
    out.push_back((int64_t)a.out_pts[2 * i + 1]);
    out.push_back(a.out_score[i]);
    out.push_back(a.out_cell_index[i]);
  }
  FILE *o = std::fopen(argv[2], "wb");
  if (!o || std::fwrite(out.data(), sizeof(int64_t), out.size(), o) != out.size()) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  std::fclose(o);
  std::printf("detect_host: %lld images, %lld cells each, %lld points; images and cell maps held without slack\n",
              (long long)F, (long long)n_cells, (long long)N);
  return 0;
}
