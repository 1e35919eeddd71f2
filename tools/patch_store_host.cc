// patch_store_host.cc -- pnec_patch_store.hpp built for the host, and the control flow of pnec_patch_store.hip's slot
// assignment replayed with it: one block of 256 lanes per image, barrier by barrier -- the occupancy map cleared, the
// carried rows' bits, every lane's count of free bits over its run of words, the block scan, the number of free slots
// below each word, the new rows' slots, the padding shared among the blocks.  Every array -- the two LDS arrays too, cut
// to the words the capacity needs -- is a heap block of exactly its size, so under -fsanitize=address,undefined any access
// beyond one is a report.  tests/test_patch_store_cpu.py builds it, feeds it the hand-worked vectors and boundary counts
// and compares with numpy.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -Ipnec_amd/csrc tools/patch_store_host.cc -o patch_store_host
//   patch_store_host job.bin out.bin
// job.bin: int64 [4] F, C, n_rows, carried (0 / 1), then carried_offsets int64 [F + 1] (if carried), offsets int64 [F + 1],
// slot int32 [n_rows].  out.bin: slot int32 [n_rows].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pnec_patch_store.hpp"

using namespace pnec_hip;

namespace {

template <typename T>
T *block(const char *src, int64_t n, std::vector<std::unique_ptr<char[]>> &keep) {
  const size_t bytes = sizeof(T) * (size_t)n;
  keep.emplace_back(new char[bytes]);
  if (src) std::memcpy(keep.back().get(), src, bytes);
  else std::memset(keep.back().get(), 0x5a, bytes);
  return reinterpret_cast<T *>(keep.back().get());
}

// patch_store_assign_kernel, block f
void assign_block(const PatchStoreAssignArgs &a, int64_t f) {
  constexpr int B = kStoreAssignBlock;
  std::vector<std::unique_ptr<char[]>> lds;
  const int64_t C = a.capacity;
  const int n_words = (int)((C + 31) / 32);
  uint32_t *occupied = block<uint32_t>(nullptr, n_words, lds);
  int32_t *before = block<int32_t>(nullptr, n_words, lds);
  int32_t *part = block<int32_t>(nullptr, B, lds);
  int64_t lo, c, take;
  store_counts(a.carried_offsets, a.offsets, a.n_rows, f, lo, c, take);
  for (int t = 0; t < B; ++t)
    for (int w = t; w < n_words; w += B) occupied[w] = 0u;
  // (barrier)
  for (int t = 0; t < B; ++t)
    for (int64_t r = t; r < take; r += B) {
      const int64_t v = store_local_slot(a.slot[lo + r], f, C);
      if (v >= 0) occupied[v >> 5] |= 1u << (int)(v & 31);
    }
  // (barrier)
  const int per = (n_words + B - 1) / B;
  int32_t mine[B], x[B];
  int w0[B], w1[B];
  for (int t = 0; t < B; ++t) {
    w0[t] = t * per < n_words ? t * per : n_words;
    w1[t] = w0[t] + per < n_words ? w0[t] + per : n_words;
    mine[t] = 0;
    for (int w = w0[t]; w < w1[t]; ++w) mine[t] += store_popcount(store_free_word(occupied[w], w, C));
    x[t] = mine[t];
    part[t] = x[t];
  }
  for (int s = 1; s < B; s <<= 1) {
    int32_t o[B];
    for (int t = 0; t < B; ++t) o[t] = t >= s ? part[t - s] : 0;   // (barrier)
    for (int t = 0; t < B; ++t) {
      x[t] += o[t];
      part[t] = x[t];
    }
  }
  const int64_t n_free = part[B - 1];
  for (int t = 0; t < B; ++t) {
    int32_t run = x[t] - mine[t];
    for (int w = w0[t]; w < w1[t]; ++w) {
      before[w] = run;
      run += store_popcount(store_free_word(occupied[w], w, C));
    }
  }
  // (barrier)
  const int64_t n_new = c - take;
  for (int t = 0; t < B; ++t)
    for (int64_t i = t; i < n_new; i += B)
      a.slot[lo + take + i] = i < n_free ? (int32_t)(f * C + store_nth_free(occupied, before, n_words, C, i)) : -1;
  int64_t end = a.offsets[a.n_images];
  end = end < 0 ? 0 : end;
  for (int t = 0; t < B; ++t)
    for (int64_t r = end + f * B + t; r < a.n_rows; r += a.n_images * B) a.slot[r] = -1;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: patch_store_host job.bin out.bin\n");
    return 2;
  }
  std::FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<char> buf;
  char chunk[65536];
  for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, in)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
  std::fclose(in);
  if (buf.size() < 32) return 2;
  int64_t head[4];
  std::memcpy(head, buf.data(), 32);
  const int64_t F = head[0], C = head[1], N = head[2];
  const bool carried = head[3] != 0;
  if (F < 1 || C < 1 || C > kStoreMaxCapacity || N < 0) return 2;
  const size_t want = 32 + (size_t)(carried ? 2 : 1) * 8 * (size_t)(F + 1) + 4 * (size_t)N;
  if (buf.size() != want) {
    std::fprintf(stderr, "job has %zu bytes, not %zu\n", buf.size(), want);
    return 2;
  }
  std::vector<std::unique_ptr<char[]>> keep;
  const char *at = buf.data() + 32;
  PatchStoreAssignArgs a{};
  a.n_images = F;
  a.capacity = C;
  a.n_rows = N;
  if (carried) {
    a.carried_offsets = block<int64_t>(at, F + 1, keep);
    at += 8 * (F + 1);
  }
  a.offsets = block<int64_t>(at, F + 1, keep);
  at += 8 * (F + 1);
  a.slot = block<int32_t>(at, N, keep);
  for (int64_t f = 0; f < F; ++f) assign_block(a, f);
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  if (N > 0) std::fwrite(a.slot, sizeof(int32_t), (size_t)N, out);
  std::fclose(out);
  std::printf("patch store: %lld images, capacity %lld, %lld rows assigned on heap blocks without slack\n", (long long)F,
              (long long)C, (long long)N);
  return 0;
}
