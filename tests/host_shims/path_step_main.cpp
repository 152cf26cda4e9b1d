// Stand-alone run of nadavca_amd/csrc/path_step.h for tests/test_path_step_cpu.py, built there with
// -fsanitize=address,undefined: the test's cases go through the header once more, in a program whose every buffer has
// exactly the size the cases need.
// argv[1]: a binary file: int64 n, then dv[n] (double), bestn[n] (double), Gin[n] (int32), G[n] (int32).
// stdout: "n differ xor" — the cases, those whose two forms differ, and the xor of (j + 1) * out[j] over all cases
// (path_step_host_run's words), which the test compares with the ctypes library's.
#include <stdio.h>

#include <vector>

#include "path_step_host.cpp"

static int fail(const char *what) {
  fprintf(stderr, "path_step_main: %s\n", what);
  return 1;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: path_step_main CASES");
  FILE *f = fopen(argv[1], "rb");
  if (!f) return fail("cannot open the case file");
  long long n = 0;
  if (fread(&n, sizeof n, 1, f) != 1 || n <= 0 || n > (1ll << 26)) return fail("bad header");
  std::vector<double> dv((size_t)n), bestn((size_t)n);
  std::vector<int32_t> Gin((size_t)n), G((size_t)n), out((size_t)n);
  if (fread(dv.data(), sizeof(double), (size_t)n, f) != (size_t)n || fread(bestn.data(), sizeof(double), (size_t)n, f) != (size_t)n ||
      fread(Gin.data(), sizeof(int32_t), (size_t)n, f) != (size_t)n || fread(G.data(), sizeof(int32_t), (size_t)n, f) != (size_t)n)
    return fail("short case file");
  fclose(f);
  const long long differ = path_step_host_run(n, dv.data(), Gin.data(), bestn.data(), G.data(), out.data());
  unsigned long long x = 0;
  for (long long j = 0; j < n; j++) x ^= (unsigned long long)(j + 1) * (unsigned long long)(uint32_t)out[(size_t)j];
  printf("%lld %lld %llu\n", n, differ, x);
  return 0;
}
