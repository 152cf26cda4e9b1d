// Host build of nadavca_amd/csrc/part_cut.h for tests/test_part_cut_cpu.py (g++ -O2 -shared): the cut of a batch into
// parts under a workspace cap that the seed-extension, event-alignment, decode and posterior entries run.
#include "../../nadavca_amd/csrc/part_cut.h"

// off: n + 1 values; cut: room for n + 2 values; n_cut: the number written -> the units of the largest part
extern "C" long long part_cut_host(const long long *off, long long n, long long cap, long long *cut,
                                   long long *n_cut) {
  const std::vector<int64_t> o(off, off + n + 1);
  std::vector<int64_t> c;
  const int64_t need = cut_parts(o, cap, c);
  for (size_t i = 0; i < c.size(); i++) cut[i] = c[i];
  *n_cut = (long long)c.size();
  return need;
}
