// keyframe_host.cc -- pnec_keyframe.hpp built for the host, and the control flow of pnec_keyframe.hip's kernels replayed
// with it: blocks of four wavefronts of 64 lanes, the ballot of the match predicate and its ranks, the per-lane partial
// sums and the lane tree, the block scan (256 lanes in lockstep, barrier by barrier), the emit, and the one-lane-per-row
// state + pad pass.  Every array is a heap block of exactly the size the ABI demands, so under
// -fsanitize=address,undefined any access beyond one is a report.  tests/test_keyframe_cpu.py builds it, feeds it cases
// and compares with numpy.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -Ipnec_amd/csrc tools/keyframe_host.cc -o keyframe_host
//   keyframe_host job.bin out.bin
// job.bin: int64 [7] F, n_rows, n_new, n_key_rows, max_span, flags (1 covariances, 2 a retained set and a state are
// given), and the bits of the double min_displacement; then the inputs in the ABI's order, absent ones left out.
// out.bin: the outputs in the ABI's order, absent ones left out.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pnec_keyframe.hpp"

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

void keyframe(const KeyframeArgs &a) {
  const int64_t image_blocks = (a.n_images + kTracksWaves - 1) / kTracksWaves;
  // count
  for (int64_t b = 0; b < image_blocks; ++b)
    for (int wave = 0; wave < kTracksWaves; ++wave) {
      const int64_t f = b * kTracksWaves + wave;
      const bool inside = f < a.n_images;
      int64_t lo = 0, hi = 0;
      if (inside) tracks_range(a.offsets, f, a.n_rows, lo, hi);
      int64_t n = 0;
      double part[kTracksLanes];
      for (int lane = 0; lane < kTracksLanes; ++lane) part[lane] = 0.0;
      for (int64_t base = lo; base < hi; base += kTracksLanes) {
        uint64_t ballot = 0;
        for (int lane = 0; lane < kTracksLanes; ++lane) {
          const int64_t k = base + lane;
          double d = 0.0;
          const bool match = k < hi && keyframe_match(a, k, d);
          ballot |= (uint64_t)match << lane;
          if (match) part[lane] += d;
        }
        n += tracks_popcount(ballot);
      }
      for (int s = kTracksLanes / 2; s >= 1; s >>= 1) {
        double other[kTracksLanes];
        for (int lane = 0; lane < kTracksLanes; ++lane) other[lane] = part[keyframe_tree_peer(lane, s)];   // (exchange)
        for (int lane = 0; lane < kTracksLanes; ++lane) part[lane] = keyframe_tree_step(part[lane], other[lane]);
      }
      if (inside) keyframe_decide(a, f, n, part[0]);
    }
  // scan
  block_scan(a.out_offsets, a.n_images, [&](int64_t f) { return a.out_offsets[f + 1]; });
  // emit
  if (a.n_rows > 0)
    for (int64_t b = 0; b < image_blocks; ++b)
      for (int wave = 0; wave < kTracksWaves; ++wave) {
        const int64_t f = b * kTracksWaves + wave;
        const bool inside = f < a.n_images;
        int64_t lo = 0, hi = 0;
        if (inside && keyframe_accepted(a, f)) tracks_range(a.offsets, f, a.n_rows, lo, hi);
        int64_t at0 = inside ? a.out_offsets[f] : 0;
        for (int64_t base = lo; base < hi; base += kTracksLanes) {
          bool match[kTracksLanes];
          uint64_t ballot = 0;
          for (int lane = 0; lane < kTracksLanes; ++lane) {
            const int64_t k = base + lane;
            double d = 0.0;
            match[lane] = k < hi && keyframe_match(a, k, d);
            ballot |= (uint64_t)match[lane] << lane;
          }
          for (int lane = 0; lane < kTracksLanes; ++lane) {
            const int64_t at = at0 + tracks_rank(ballot, lane);
            if (match[lane] && at >= 0 && at < a.n_rows) keyframe_pair_row(a, base + lane, at);
          }
          at0 += tracks_popcount(ballot);
        }
      }
  // state + pad
  const int64_t rows = a.n_new > a.n_rows ? a.n_new : a.n_rows, row_blocks = (rows + 255) / 256;
  for (int64_t i = 0; i < row_blocks * 256; ++i) {
    if (i < a.n_new) keyframe_state_row(a, i);
    if (i < a.n_rows && i >= a.out_offsets[a.n_images]) keyframe_pad_pair(a, i);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: keyframe_host job.bin out.bin\n");
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
  const int64_t *h = r.take<int64_t>(7, keep);
  const int64_t F = h[0], N = h[1], A = h[2], S = h[3], flags = h[5];
  const bool cov = flags & 1, set = flags & 2;
  KeyframeArgs a{};
  a.n_images = F;
  a.n_rows = N;
  a.n_new = A;
  a.n_key_rows = set ? S : 0;
  a.max_span = (int32_t)h[4];
  std::memcpy(&a.min_displacement, &h[6], sizeof(double));
  if (set) {
    a.offsets = r.take<int64_t>(F + 1, keep);
    a.pts = r.take<double>(2 * N, keep);
    a.cov = cov ? r.take<double>(3 * N, keep) : nullptr;
    a.src = r.take<int64_t>(N, keep);
  }
  a.new_offsets = r.take<int64_t>(F + 1, keep);
  a.new_pts = r.take<double>(2 * A, keep);
  a.new_cov = cov ? r.take<double>(3 * A, keep) : nullptr;
  if (set) {
    a.key_pts = r.take<double>(2 * S, keep);
    a.key_cov = cov ? r.take<double>(3 * S, keep) : nullptr;
    a.span = r.take<int32_t>(F, keep);
  }
  a.out_offsets = fresh<int64_t>(F + 1, keep);
  a.out_key_pts = fresh<double>(2 * N, keep);
  a.out_pts = fresh<double>(2 * N, keep);
  a.out_cov = cov && set ? fresh<double>(3 * N, keep) : nullptr;
  a.out_key_cov = cov && set ? fresh<double>(3 * N, keep) : nullptr;
  a.out_row = fresh<int64_t>(N, keep);
  a.out_accepted = fresh<uint8_t>(F, keep);
  a.out_mean = fresh<double>(F, keep);
  a.out_n_matches = fresh<int32_t>(F, keep);
  a.next_key_pts = fresh<double>(2 * A, keep);
  a.next_key_cov = cov ? fresh<double>(3 * A, keep) : nullptr;
  a.next_span = fresh<int32_t>(F, keep);
  keyframe(a);
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  put(out, a.out_offsets, F + 1);
  put(out, a.out_key_pts, 2 * N);
  put(out, a.out_pts, 2 * N);
  put(out, a.out_cov, 3 * N);
  put(out, a.out_key_cov, 3 * N);
  put(out, a.out_row, N);
  put(out, a.out_accepted, F);
  put(out, a.out_mean, F);
  put(out, a.out_n_matches, F);
  put(out, a.next_key_pts, 2 * A);
  put(out, a.next_key_cov, 3 * A);
  put(out, a.next_span, F);
  std::fclose(out);
  if (r.at != r.buf.size()) {
    std::fprintf(stderr, "job too long\n");
    return 2;
  }
  std::printf("every array a heap block without slack: keyframe done\n");
  return 0;
}
