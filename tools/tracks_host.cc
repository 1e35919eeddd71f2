// tracks_host.cc -- pnec_tracks.hpp built for the host, and the control flow of pnec_tracks.hip's kernels replayed with
// it: blocks of four wavefronts of 64 lanes, the ballot of the retention rule and its ranks, the count, the block scan
// (256 lanes in lockstep, barrier by barrier) and the emit, then append's scan, one-lane-per-row emit and next_id pass.
// Every array is a heap block of exactly the size the ABI demands, so under -fsanitize=address,undefined any access beyond
// one is a report.  tests/test_tracks_cpu.py builds it, feeds it the GPU tests' cases and compares with numpy.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -Ipnec_amd/csrc tools/tracks_host.cc -o tracks_host
//   tracks_host job.bin out.bin
// job.bin: int64 [9] kind (0 retain, 1 append), F, n_rows, n_det, n_out, max_age, tmpl_image_base, capacity, flags
// (1 covariances wanted, 2 out_prev_pts, 4 out_src, 8 a set is given, 16 the set has cov, 32 det_cov), then the inputs in
// the ABI's order, absent ones left out.  out.bin: the outputs in the ABI's order, absent ones left out.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pnec_tracks.hpp"

using namespace pnec_hip;

namespace {

struct Reader {
  std::vector<char> buf;
  size_t at = 0;
  // a heap block of exactly n items (n = 0: a block of no bytes, still not NULL)
  template <typename T>
  T *take(int64_t n, std::vector<std::unique_ptr<char[]>> &keep) {
    const size_t bytes = sizeof(T) * (size_t)n;
    if (at + bytes > buf.size()) {
      std::fprintf(stderr, "job too short\n");
      std::exit(2);
    }
    keep.emplace_back(new char[bytes]);
    std::memcpy(keep.back().get(), buf.data() + at, bytes);
    at += bytes;
    return reinterpret_cast<T *>(keep.back().get());
  }
};

template <typename T>
T *fresh(int64_t n, std::vector<std::unique_ptr<char[]>> &keep) {
  keep.emplace_back(new char[sizeof(T) * (size_t)n]);
  std::memset(keep.back().get(), 0x5a, sizeof(T) * (size_t)n);
  return reinterpret_cast<T *>(keep.back().get());
}

template <typename T>
void put(std::FILE *f, const T *p, int64_t n) {
  if (p && n > 0) std::fwrite(p, sizeof(T), (size_t)n, f);
}

// tracks_block_scan: one block of 256 lanes; `count(f)` is read by the lane that then writes v[f + 1]
template <typename Count>
void block_scan(int64_t *v, int64_t F, Count count) {
  int64_t part[256], x[256];
  int64_t carry = 0;
  for (int64_t base = 0; base < F; base += 256) {
    for (int t = 0; t < 256; ++t) {
      const int64_t f = base + t;
      x[t] = f < F ? count(f) : 0;
      part[t] = x[t];
    }
    for (int s = 1; s < 256; s <<= 1) {
      int64_t o[256];
      for (int t = 0; t < 256; ++t) o[t] = t >= s ? part[t - s] : 0;   // (barrier)
      for (int t = 0; t < 256; ++t) {
        x[t] += o[t];
        part[t] = x[t];
      }
    }
    for (int t = 0; t < 256; ++t)
      if (base + t < F) v[base + t + 1] = carry + x[t];
    carry += part[255];
  }
  v[0] = 0;
}

void retain(const TracksRetainArgs &a) {
  const int64_t image_blocks = (a.n_images + kTracksWaves - 1) / kTracksWaves;
  // count
  for (int64_t b = 0; b < image_blocks; ++b)
    for (int wave = 0; wave < kTracksWaves; ++wave) {
      const int64_t f = b * kTracksWaves + wave;
      const bool inside = f < a.n_images;
      int64_t lo = 0, hi = 0;
      if (inside) tracks_range(a.in.offsets, f, a.in.n_rows, lo, hi);
      int64_t sum = 0;
      for (int64_t base = lo; base < hi; base += kTracksLanes) {
        uint64_t ballot = 0;
        for (int lane = 0; lane < kTracksLanes; ++lane) {
          const int64_t k = base + lane;
          const bool keep = k < hi && tracks_keep(a.in.id[k], a.trk_status[k], a.in.age[k], a.max_age);
          ballot |= (uint64_t)keep << lane;
        }
        sum += tracks_popcount(ballot);
      }
      if (inside) a.out.offsets[f + 1] = sum;
    }
  // scan
  block_scan(a.out.offsets, a.n_images, [&](int64_t f) { return a.out.offsets[f + 1]; });
  // emit
  for (int64_t b = 0; b < image_blocks; ++b)
    for (int wave = 0; wave < kTracksWaves; ++wave) {
      const int64_t f = b * kTracksWaves + wave;
      const bool inside = f < a.n_images;
      int64_t lo = 0, hi = 0;
      if (inside) tracks_range(a.in.offsets, f, a.in.n_rows, lo, hi);
      int64_t at0 = inside ? a.out.offsets[f] : 0;
      for (int64_t base = lo; base < hi; base += kTracksLanes) {
        bool keep[kTracksLanes];
        uint64_t ballot = 0;
        for (int lane = 0; lane < kTracksLanes; ++lane) {
          const int64_t k = base + lane;
          keep[lane] = k < hi && tracks_keep(a.in.id[k], a.trk_status[k], a.in.age[k], a.max_age);
          ballot |= (uint64_t)keep[lane] << lane;
        }
        for (int lane = 0; lane < kTracksLanes; ++lane) {
          const int64_t at = at0 + tracks_rank(ballot, lane);
          if (keep[lane] && at < a.in.n_rows) tracks_retain_row(a, base + lane, at);
        }
        at0 += tracks_popcount(ballot);
      }
    }
  // pad
  const int64_t row_blocks = (a.in.n_rows + 255) / 256;
  for (int64_t i = 0; i < row_blocks * 256; ++i) {
    if (i >= a.in.n_rows || i < a.out.offsets[a.n_images]) continue;
    tracks_pad_retained(a, i);
  }
}

void append(const TracksAppendArgs &a) {
  block_scan(a.out.offsets, a.n_images, [&](int64_t f) {
    int64_t lo_a, lo_d, n_a, n_d, take_a, take_d;
    tracks_append_counts(a, f, lo_a, lo_d, n_a, n_d, take_a, take_d);
    if (a.out_dropped) a.out_dropped[f] = (n_a - take_a) + (n_d - take_d);
    return take_a + take_d;
  });
  const int64_t row_blocks = (a.n_out + 255) / 256, image_blocks = (a.n_images + 255) / 256;
  for (int64_t i = 0; i < row_blocks * 256; ++i)
    if (i < a.n_out) tracks_append_row(a, i);
  for (int64_t f = 0; f < image_blocks * 256; ++f) {
    if (f >= a.n_images) continue;
    int64_t lo_a, lo_d, n_a, n_d, take_a, take_d;
    tracks_append_counts(a, f, lo_a, lo_d, n_a, n_d, take_a, take_d);
    a.next_id[f] += take_d;
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: tracks_host job.bin out.bin\n");
    return 2;
  }
  Reader r;
  {
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::fseek(f, 0, SEEK_END);
    r.buf.resize((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(r.buf.data(), 1, r.buf.size(), f) != r.buf.size()) return 2;
    std::fclose(f);
  }
  std::vector<std::unique_ptr<char[]>> keep;
  const int64_t *h = r.take<int64_t>(9, keep);
  const int64_t kind = h[0], F = h[1], N = h[2], D = h[3], O = h[4], flags = h[8];
  const bool cov = flags & 1;
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  if (kind == 0) {
    TracksRetainArgs a{};
    a.n_images = F;
    a.in.n_rows = N;
    a.max_age = (int32_t)h[5];
    a.in.offsets = r.take<int64_t>(F + 1, keep);
    a.in.id = r.take<int64_t>(N, keep);
    a.in.tmpl_image = r.take<int32_t>(N, keep);
    a.in.tmpl_pts = r.take<double>(2 * N, keep);
    a.in.age = r.take<int32_t>(N, keep);
    a.in.pts = r.take<double>(2 * N, keep);
    a.in.cov = cov ? r.take<double>(3 * N, keep) : nullptr;
    a.trk_pts = r.take<double>(2 * N, keep);
    a.trk_angle = r.take<double>(N, keep);
    a.trk_cov = cov ? r.take<double>(3 * N, keep) : nullptr;
    a.trk_status = r.take<int32_t>(N, keep);
    a.out.offsets = fresh<int64_t>(F + 1, keep);
    a.out.id = fresh<int64_t>(N, keep);
    a.out.tmpl_image = fresh<int32_t>(N, keep);
    a.out.tmpl_pts = fresh<double>(2 * N, keep);
    a.out.age = fresh<int32_t>(N, keep);
    a.out.pts = fresh<double>(2 * N, keep);
    a.out.angle = fresh<double>(N, keep);
    a.out.cov = cov ? fresh<double>(3 * N, keep) : nullptr;
    a.out_prev_pts = (flags & 2) ? fresh<double>(2 * N, keep) : nullptr;
    a.out_prev_cov = cov ? fresh<double>(3 * N, keep) : nullptr;
    a.out_src = (flags & 4) ? fresh<int64_t>(N, keep) : nullptr;
    retain(a);
    put(out, a.out.offsets, F + 1);
    put(out, a.out.id, N);
    put(out, a.out.tmpl_image, N);
    put(out, a.out.tmpl_pts, 2 * N);
    put(out, a.out.age, N);
    put(out, a.out.pts, 2 * N);
    put(out, a.out.angle, N);
    put(out, a.out.cov, 3 * N);
    put(out, a.out_prev_pts, 2 * N);
    put(out, a.out_prev_cov, 3 * N);
    put(out, a.out_src, N);
  } else {
    TracksAppendArgs a{};
    a.n_images = F;
    a.in.n_rows = N;
    a.n_det = D;
    a.n_out = O;
    a.tmpl_image_base = (int32_t)h[6];
    a.capacity = h[7];
    if (flags & 8) {
      a.in.offsets = r.take<int64_t>(F + 1, keep);
      a.in.id = r.take<int64_t>(N, keep);
      a.in.tmpl_image = r.take<int32_t>(N, keep);
      a.in.tmpl_pts = r.take<double>(2 * N, keep);
      a.in.age = r.take<int32_t>(N, keep);
      a.in.pts = r.take<double>(2 * N, keep);
      a.in.angle = r.take<double>(N, keep);
      a.in.cov = (flags & 16) ? r.take<double>(3 * N, keep) : nullptr;
    }
    a.det_offsets = r.take<int64_t>(F + 1, keep);
    a.det_pts = r.take<double>(2 * D, keep);
    a.det_cov = (flags & 32) ? r.take<double>(3 * D, keep) : nullptr;
    a.next_id = r.take<int64_t>(F, keep);
    a.out.offsets = fresh<int64_t>(F + 1, keep);
    a.out.id = fresh<int64_t>(O, keep);
    a.out.tmpl_image = fresh<int32_t>(O, keep);
    a.out.tmpl_pts = fresh<double>(2 * O, keep);
    a.out.age = fresh<int32_t>(O, keep);
    a.out.pts = fresh<double>(2 * O, keep);
    a.out.angle = fresh<double>(O, keep);
    a.out.cov = cov ? fresh<double>(3 * O, keep) : nullptr;
    a.out_dropped = fresh<int64_t>(F, keep);
    append(a);
    put(out, a.out.offsets, F + 1);
    put(out, a.out.id, O);
    put(out, a.out.tmpl_image, O);
    put(out, a.out.tmpl_pts, 2 * O);
    put(out, a.out.age, O);
    put(out, a.out.pts, 2 * O);
    put(out, a.out.angle, O);
    put(out, a.out.cov, 3 * O);
    put(out, a.next_id, F);
    put(out, a.out_dropped, F);
  }
  std::fclose(out);
  if (r.at != r.buf.size()) {
    std::fprintf(stderr, "job too long\n");
    return 2;
  }
  std::printf("every array a heap block without slack: %s done\n", kind == 0 ? "retain" : "append");
  return 0;
}
