// Which plan a context holds (api.hip): the key under which nvk_refine_alignment_batch_dev_keyed left the planner's
// results in the context's workspaces, and the comparison that lets a later call sweep from them without planning
// again.  In plain C++ so that it can be compiled and checked without a GPU (tests/host_shims/plan_key_host.cpp,
// tests/test_plan_key_cpu.py).  Nothing here touches HIP.
#pragma once
#include <stdint.h>

namespace plan_key {

enum { N_GEOM = 9 };

// Everything the planner's result is a function of.  The token IS the batch (include/nadavca_hip.h: one token, one
// immutable geometry); the pointers are a cheap cross-check and never the identity — an allocator hands the next batch
// of the same shape the same addresses.
struct Key {
  uint64_t token;     // 0: no plan is held / the caller asks for none
  uint64_t model_id;  // nvk_model::id, process-wide and never reused (a later model may get an earlier one's address)
  int32_t bandwidth, mel, transitions;
  int32_t rows_written;  // the plan was made with the row table (NADAVCA_ALIGN_KERNEL=1): such a plan serves only such calls
  int64_t n_reads, total_signal, total_ref, total_anchors;
  // sig_off, reference, ref_off, ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off (not signal: its samples, and
  // so where they lie, are no part of the plan)
  const void *geom[N_GEOM];
};

inline void clear(Key &k) {
  k.token = 0;
  k.model_id = 0;
  k.bandwidth = k.mel = k.transitions = k.rows_written = 0;
  k.n_reads = k.total_signal = k.total_ref = k.total_anchors = 0;
  for (int q = 0; q < N_GEOM; q++) k.geom[q] = nullptr;
}

// whether the plan held under `held` is the one a call described by `want` would make.  Token 0 on either side — a
// cleared key, or a caller without a token — never matches.
inline bool matches(const Key &held, const Key &want) {
  if (held.token == 0 || want.token == 0 || held.token != want.token) return false;
  if (held.model_id != want.model_id || held.bandwidth != want.bandwidth || held.mel != want.mel ||
      held.transitions != want.transitions || held.rows_written != want.rows_written)
    return false;
  if (held.n_reads != want.n_reads || held.total_signal != want.total_signal || held.total_ref != want.total_ref ||
      held.total_anchors != want.total_anchors)
    return false;
  for (int q = 0; q < N_GEOM; q++)
    if (held.geom[q] != want.geom[q]) return false;
  return true;
}

}  // namespace plan_key
