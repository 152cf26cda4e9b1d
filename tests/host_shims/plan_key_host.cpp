// Host build of nadavca_amd/csrc/plan_key.h for tests/test_plan_key_cpu.py (g++ -O2 -shared), and — included by
// plan_key_main.cpp — for the stand-alone sanitizer run: a key as a flat array of PLAN_KEY_FIELDS 64-bit values, in the
// order of the struct (token, model_id, bandwidth, mel, transitions, rows_written, n_reads, total_signal, total_ref,
// total_anchors, then the nine geometry addresses).
#include <stdint.h>

#include "../../nadavca_amd/csrc/plan_key.h"

enum { PLAN_KEY_FIELDS = 10 + plan_key::N_GEOM };

static plan_key::Key key_of(const long long *v) {
  plan_key::Key k;
  plan_key::clear(k);
  k.token = (uint64_t)v[0];
  k.model_id = (uint64_t)v[1];
  k.bandwidth = (int32_t)v[2];
  k.mel = (int32_t)v[3];
  k.transitions = (int32_t)v[4];
  k.rows_written = (int32_t)v[5];
  k.n_reads = v[6];
  k.total_signal = v[7];
  k.total_ref = v[8];
  k.total_anchors = v[9];
  for (int q = 0; q < plan_key::N_GEOM; q++) k.geom[q] = (const void *)(uintptr_t)v[10 + q];
  return k;
}

extern "C" int plan_key_host_fields(void) { return PLAN_KEY_FIELDS; }

// whether a call described by `want` may sweep from the plan held under `held`
extern "C" int plan_key_host_matches(const long long *held, const long long *want) {
  return plan_key::matches(key_of(held), key_of(want)) ? 1 : 0;
}

// the same after the held key was cleared
extern "C" int plan_key_host_matches_cleared(const long long *held, const long long *want) {
  plan_key::Key h = key_of(held);
  plan_key::clear(h);
  return plan_key::matches(h, key_of(want)) ? 1 : 0;
}
