// Stand-alone run of nadavca_amd/csrc/plan_key.h for tests/test_plan_key_cpu.py, built there with
// -fsanitize=address,undefined: the table of the test — an equal key matches; a key that differs in any single field,
// token 0 on either side and a cleared key do not — through the same header in a program of its own.
// Exit status 0 unless a row of the table comes out wrong.
#include <stdio.h>

#include <vector>

#include "plan_key_host.cpp"

static int fail(const char *what, int field) {
  fprintf(stderr, "plan_key_main: %s (field %d)\n", what, field);
  return 1;
}

int main() {
  std::vector<long long> base((size_t)PLAN_KEY_FIELDS);
  for (int q = 0; q < PLAN_KEY_FIELDS; q++) base[(size_t)q] = 1000 + 16 * q;  // all different, none 0
  base[4] = 1;                                                                // (transitions, rows_written: flags)
  base[5] = 0;
  if (!plan_key_host_matches(base.data(), base.data())) return fail("an equal key does not match", -1);
  for (int q = 0; q < PLAN_KEY_FIELDS; q++)
    for (int side = 0; side < 2; side++) {
      std::vector<long long> other(base);
      other[(size_t)q] = (q == 4 || q == 5) ? 1 - base[(size_t)q] : base[(size_t)q] + 1;
      const long long *held = side ? other.data() : base.data(), *want = side ? base.data() : other.data();
      if (plan_key_host_matches(held, want)) return fail("a key that differs in one field matches", q);
    }
  std::vector<long long> zero(base);
  zero[0] = 0;
  if (plan_key_host_matches(zero.data(), base.data()) || plan_key_host_matches(base.data(), zero.data()) ||
      plan_key_host_matches(zero.data(), zero.data()))
    return fail("token 0 matches", 0);
  if (plan_key_host_matches_cleared(base.data(), base.data())) return fail("a cleared key matches", -1);
  printf("plan_key_main: %d fields ok\n", PLAN_KEY_FIELDS);
  return 0;
}
