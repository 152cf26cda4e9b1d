// The host arithmetic that cuts a batch into parts under a workspace cap, in plain C++ so that it can be compiled and
// checked without a GPU (tests/host_shims/part_cut_host.cpp, tests/test_part_cut_cpu.py).  The entries whose per-read
// store lies in a workspace (seed extension, event alignment, Viterbi decode, k-mer posteriors) all cut with it: it
// decides how much device memory is reserved and which reads share a launch.  Nothing here touches HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// off[0..n]: each read's first unit of a store; cap: units a part may take (>= 0).
// -> cut (0 = cut[0] < ... < cut.back() = n; n == 0 gives {0, 0}) and the units of the largest part (>= 1).
// A read joins the current part unless the part would then exceed cap; a read larger than cap on its own is a part of
// one.
inline int64_t cut_parts(const std::vector<int64_t> &off, int64_t cap, std::vector<int64_t> &cut) {
  const int64_t n = (int64_t)off.size() - 1;
  cut.assign(1, 0);
  int64_t need = 1;
  for (int64_t r = 0; r < n; r++) {
    const int64_t c0 = cut.back();
    if (r > c0 && off[r + 1] - off[c0] > cap) {
      need = need > off[r] - off[c0] ? need : off[r] - off[c0];
      cut.push_back(r);
    }
  }
  need = need > off[n] - off[cut.back()] ? need : off[n] - off[cut.back()];
  cut.push_back(n);
  return need;
}
