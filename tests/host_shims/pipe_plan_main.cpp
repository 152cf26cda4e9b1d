// Stand-alone run of nadavca_amd/csrc/pipe_plan.h for tests/test_pipe_plan_cpu.py, built there with
// -fsanitize=address,undefined: the edge table of the schedule test goes through the same header once more, in a
// program whose every buffer has exactly the size the header was promised.
// argv[1]: a text file, one case per line: n_reads n_chunks growth min_reads floor_bytes sig_off[0 .. n_reads]
// stdout: per case "count lo hi lo hi ...".  Exit status 0 unless a case is malformed or a property fails.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../nadavca_amd/csrc/pipe_plan.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "pipe_plan_main: %s (case %ld)\n", what, line);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: pipe_plan_main CASES", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the case file", 0);
  long line = 0;
  long long n_reads, n_chunks, min_reads, floor_bytes;
  double growth;
  while (fscanf(f, "%lld %lld %lf %lld %lld", &n_reads, &n_chunks, &growth, &min_reads, &floor_bytes) == 5) {
    line++;
    if (n_reads < 1) return fail("n_reads < 1", line);
    std::vector<int64_t> off((size_t)n_reads + 1);
    for (long long i = 0; i <= n_reads; i++) {
      long long v;
      if (fscanf(f, "%lld", &v) != 1) return fail("short offsets", line);
      off[(size_t)i] = v;
    }
    std::vector<int64_t> bounds(2 * pipe_plan::MAX_CHUNKS);
    const int64_t made = pipe_plan::chunk_schedule(off.data(), n_reads, n_chunks, growth, min_reads, floor_bytes,
                                                   bounds.data());
    if (made < 1 || made > pipe_plan::MAX_CHUNKS) return fail("chunk count out of range", line);
    printf("%lld", (long long)made);
    int64_t at_read = 0;
    for (int64_t c = 0; c < made; c++) {
      const int64_t lo = bounds[(size_t)(2 * c)], hi = bounds[(size_t)(2 * c + 1)];
      printf(" %lld %lld", (long long)lo, (long long)hi);
      if (lo != at_read || hi <= lo) return fail("chunks do not partition the reads", line);
      at_read = hi;
      // the chunk's pack, with the signal offsets standing for all five arrays: reference = the samples, no
      // context_before (an empty array), context_after and anchors one entry per read
      const int64_t n = hi - lo;
      size_t at[9];
      const size_t total = pipe_plan::pack_layout(n, off[(size_t)hi] - off[(size_t)lo], 0, n, n, at);
      char *buf = (char *)malloc(total);
      if (!buf) return fail("out of memory", line);
      const int64_t *src[5] = {off.data(), off.data(), off.data(), off.data(), off.data()};
      pipe_plan::rebase_offsets(src, lo, n, at, buf);
      for (int q = 0; q < 5; q++) {
        const int64_t *d = (const int64_t *)(buf + at[q]);
        for (int64_t i = 0; i <= n; i++)
          if (d[i] != off[(size_t)(lo + i)] - off[(size_t)lo]) {
            free(buf);
            return fail("rebased offsets differ", line);
          }
      }
      for (int q = 0; q < 9; q++)
        if (at[q] % 16 || at[q] >= total) {
          free(buf);
          return fail("an array lies outside the pack or is misaligned", line);
        }
      free(buf);
    }
    if (at_read != n_reads) return fail("chunks do not cover the reads", line);
    printf("\n");
  }
  fclose(f);
  return line > 0 ? 0 : fail("no cases", 0);
}
