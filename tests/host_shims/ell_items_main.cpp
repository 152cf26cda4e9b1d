// Stand-alone run of nadavca_amd/csrc/ell_items.h for tests/test_ell_items_cpu.py, built there with
// -fsanitize=address,undefined: the test's cases go through the header once more, in a program whose every buffer has
// exactly the size the case needs.
// argv[1]: a text file, one case per line:
//   E R alphabet back fwd p d ni s[0 .. ni)
//   J R alphabet back fwd ns ref[0 .. R) pos[0 .. ns) base[0 .. ns)
// stdout: per case the integers ell_items_host_edit / ell_items_host_joint (ell_items_host.cpp) find, on one line.
#include <stdio.h>

#include <vector>

#include "ell_items_host.cpp"

static int fail(const char *what, long line) {
  fprintf(stderr, "ell_items_main: %s (case %ld)\n", what, line);
  return 1;
}

static bool read_ints(FILE *f, std::vector<int32_t> &v, long long n) {
  v.resize((size_t)n);
  for (long long i = 0; i < n; i++)
    if (fscanf(f, "%d", &v[(size_t)i]) != 1) return false;
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return fail("usage: ell_items_main CASES", 0);
  FILE *f = fopen(argv[1], "r");
  if (!f) return fail("cannot open the case file", 0);
  long line = 0;
  char kind;
  int R, alphabet, back, fwd;
  while (fscanf(f, " %c %d %d %d %d", &kind, &R, &alphabet, &back, &fwd) == 5) {
    line++;
    std::vector<long long> out;
    long long n;
    if (kind == 'E') {
      int p, d;
      long long ni;
      std::vector<int32_t> s;
      if (fscanf(f, "%d %d %lld", &p, &d, &ni) != 3 || ni < 0 || !read_ints(f, s, ni)) return fail("short edit", line);
      const long long R2 = R - (d > 0 ? d : 0) + ni;  // bases of the edited reference, if the edit is accepted
      out.resize(R2 > 0 ? (size_t)(11 + 4 * R2 + 4 * ELL_ITEMS_PAD) : 1);
      n = ell_items_host_edit(R, alphabet, back, fwd, p, d, s.data(), ni, out.data());
    } else if (kind == 'J') {
      long long ns;
      std::vector<int32_t> ref, pos, base;
      if (fscanf(f, "%lld", &ns) != 1 || ns < 0 || R < 0 || !read_ints(f, ref, R) || !read_ints(f, pos, ns) ||
          !read_ints(f, base, ns))
        return fail("short joint", line);
      out.resize((size_t)(8 + R + 2 * ELL_ITEMS_PAD));
      n = ell_items_host_joint(ref.data(), R, alphabet, back, fwd, pos.data(), base.data(), ns, out.data());
    } else {
      return fail("unknown kind of case", line);
    }
    if (n < 1 || (size_t)n > out.size()) return fail("output outside its buffer", line);
    for (long long i = 0; i < n; i++) printf(i ? " %lld" : "%lld", out[(size_t)i]);
    printf("\n");
  }
  fclose(f);
  return line > 0 ? 0 : fail("no cases", 0);
}
