// pnec_call_plan.hpp -- where the arrays of one HOST-space call lie in the two staging buffers: the part of CallArrays
// (pnec_internal.hpp) that turns the list of a call's arrays into offsets and totals.  No HIP here: a host compiler
// builds it alone (tools/call_arrays_host.cc checks the counting under the sanitizers).
//   doubles and 64-bit integers share the doubles buffer; bytes live there too, in whole doubles; 32-bit integers have
//   the ints buffer.  Regions follow one another in the order of the list, so everything is 8-byte aligned in the
//   doubles buffer and 4-byte aligned in the ints buffer.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pnec_hip {

enum : unsigned {
  kKeep = 1u,     // an output the kernel writes whether or not the caller wants it: room also for a NULL pointer
  kPreload = 2u,  // an output whose caller-side content travels up first and comes back whole
};

struct CallPlan {
  struct Entry {
    bool ints;       // in the ints buffer (else the doubles buffer)
    bool room;       // it has a region (false: a NULL array, its field becomes nullptr)
    bool up, back;   // copied to the device before the launch / to the caller after it
    int64_t offset;  // first item of the region, in items of its buffer
    int64_t items;   // length of the region, in items of its buffer
    size_t bytes;    // what a copy moves
  };
  std::vector<Entry> entries;
  int64_t doubles = 0, ints = 0;  // the totals: what the two buffers must hold

  // n items of item_bytes (8, 4, or 1: bytes) each; `given`: the caller's pointer is not NULL
  const Entry &in(bool given, int64_t n, size_t item_bytes) {
    return add(item_bytes, n, given, given && n > 0, false);
  }
  const Entry &out(bool given, int64_t n, size_t item_bytes, unsigned flags = 0) {
    return add(item_bytes, n, given || (flags & kKeep), given && (flags & kPreload) && n > 0, given && n > 0);
  }
  // room the call's kernels use among themselves: nothing travels
  const Entry &scratch(int64_t n, size_t item_bytes) { return add(item_bytes, n, true, false, false); }

 private:
  const Entry &add(size_t item_bytes, int64_t n, bool room, bool up, bool back) {
    const bool ints = item_bytes == 4;
    int64_t &total = ints ? this->ints : doubles;
    const int64_t items = !room ? 0 : item_bytes == 1 ? (n + 7) / 8 : n;
    entries.push_back({ints, room, up, back, total, items, (size_t)n * item_bytes});
    total += items;
    return entries.back();
  }
};

}  // namespace pnec_hip
