// Stand-alone run of nadavca_amd/csrc/part_cut.h for tests/test_part_cut_cpu.py, built there with
// -fsanitize=address,undefined: the edge table of the cut test goes through the same header once more, in a program
// whose offsets have exactly the size the header was promised.
// argv[1]: a text file, one case per line: n cap off[0 .. n]
// stdout: per case "need count cut[0] cut[1] ...".  Exit status 0 unless a case is malformed or a property fails.
#include <stdio.h>

#include <vector>

#include "../../nadavca_amd/csrc/part_cut.h"

static int fail(const char *what, long line) {
  fprintf(stderr, "part_cut_main: %s (case %ld)\n", what, line);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: part_cut_main CASES", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the case file", 0);
  long line = 0;
  long long n, cap;
  while (fscanf(f, "%lld %lld", &n, &cap) == 2) {
    line++;
    if (n < 0 || cap < 0) return fail("n or cap below 0", line);
    std::vector<int64_t> off((size_t)n + 1);
    for (long long i = 0; i <= n; i++) {
      long long v;
      if (fscanf(f, "%lld", &v) != 1) return fail("short offsets", line);
      off[(size_t)i] = v;
    }
    std::vector<int64_t> cut;
    const int64_t need = cut_parts(off, cap, cut);
    if (cut.size() < 2 || cut.front() != 0 || cut.back() != n) return fail("the cut does not run from 0 to n", line);
    int64_t largest = 1;
    for (size_t c = 0; c + 1 < cut.size(); c++) {
      if (n > 0 && cut[c + 1] <= cut[c]) return fail("the cut does not ascend", line);
      const int64_t units = off[(size_t)cut[c + 1]] - off[(size_t)cut[c]];
      if (units > cap && cut[c + 1] - cut[c] != 1) return fail("a part of several reads exceeds the cap", line);
      if (units > largest) largest = units;
    }
    if (need != largest) return fail("need is not the largest part", line);
    printf("%lld %lld", (long long)need, (long long)cut.size());
    for (int64_t c : cut) printf(" %lld", (long long)c);
    printf("\n");
  }
  fclose(f);
  return line > 0 ? 0 : fail("no cases", 0);
}
