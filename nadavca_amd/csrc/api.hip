// C-ABI entry points of libnadavca_hip.so (declared in include/nadavca_hip.h).
// Host-side orchestration only: argument checks, workspace management, kernel launches.
// There is deliberately no CPU implementation of any operator in this library.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>
#include <vector>

#include "nvk_internal.h"

static thread_local char g_err[512] = "";

// process-wide serial numbers, never 0 and never handed out twice: batch tokens and model ids (plan_key.h)
static uint64_t next_serial() {
  static std::atomic<uint64_t> serial{0};
  uint64_t v;
  do v = serial.fetch_add(1, std::memory_order_relaxed) + 1; while (v == 0);
  return v;
}

extern "C" uint64_t nvk_plan_token_new(void) { return next_serial(); }

void nvk_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}

extern "C" const char *nvk_last_error(void) { return g_err; }

extern "C" int nvk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int nvk_alloc(void **p, size_t bytes, bool pinned, const char *what) {
  const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
  if (e == hipSuccess) return NVK_OK;
  *p = nullptr;
  (void)hipGetLastError();  // (handled here: the launch checks that follow must not see it)
  nvk_set_error("%s of %zu bytes (%s) failed: %s", pinned ? "hipHostMalloc" : "hipMalloc", bytes, what,
                hipGetErrorString(e));
  return NVK_ERR_NOMEM;
}

int nvk_grow(void **p, size_t *cap, size_t bytes, bool pinned, const char *what) {
  if (bytes <= *cap) return NVK_OK;
  if (*p) NVK_HIP(pinned ? hipHostFree(*p) : hipFree(*p));
  *p = nullptr;
  *cap = 0;
  size_t want = bytes + bytes / 8 + 4096;
  if (nvk_alloc(p, want, pinned, what)) {
    want = bytes;
    const int rc = nvk_alloc(p, want, pinned, what);
    if (rc) return rc;
  }
  *cap = want;
  return NVK_OK;
}

int nvk_ws_reserve(nvk_ctx *ctx, int which, size_t bytes) {
  if (bytes <= ctx->ws_bytes[which]) return NVK_OK;
  if (ctx->ws[which]) {
    NVK_HIP(hipStreamSynchronize(ctx->stream));
    NVK_HIP(hipStreamSynchronize(ctx->stream2));
  }
  // (a held plan lies in these blocks — WS_MISC: its totals, WS_ROWS: its row table — and goes with the one that moves)
  if (which == WS_META || which == WS_LANE_F || which == WS_LANE_R || which == WS_OFFS || which == WS_ORDER ||
      which == WS_STEPS || which == WS_MISC || which == WS_ROWS)
    plan_key::clear(ctx->plan_key);
  return nvk_grow(&ctx->ws[which], &ctx->ws_bytes[which], bytes, false, "workspace");
}

int64_t nvk_spill_cap(nvk_ctx *ctx, int which_ws) {
  if (ctx->ws_limit > 0) return ctx->ws_limit;  // nvk_ctx_set_workspace_limit
  // default: up to 60 % of what is free on the device beyond what this workspace already holds (long
  // reads: one read's spill is steps * 512 B, 170 MB for a 52 k-sample read with bandwidth 1000); a lane of
  // the pipelined host path (pipeline.hip) takes its share of that.  No floor beyond one read's worth: when
  // little is free (other tensors, another process on the GPU) the chunker serves fewer reads per launch,
  // and launch_align3 halves a chunk whose allocation still fails.
  const int share = ctx->spill_share > 1 ? ctx->spill_share : 1;
  int64_t cap = ((int64_t)48 << 30) / share;  // (if the runtime cannot say what is free)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
    cap = (int64_t)((double)(free_b + ctx->ws_bytes[which_ws]) * 0.6 / share);
  const int64_t floor_b = (int64_t)64 << 20;
  return cap > floor_b ? cap : floor_b;
}

TimerScope::TimerScope(nvk_ctx *c, int kid) : ctx(c), id(kid) {
  if (ctx->timing_on) (void)hipEventRecord(ctx->ev0, ctx->stream);
}
void TimerScope::stop() {
  if (ctx->timing_on && !stopped) (void)hipEventRecord(ctx->ev1, ctx->stream);
  stopped = true;
}
TimerScope::~TimerScope() {
  if (ctx->timing_on) {
    if (!stopped) (void)hipEventRecord(ctx->ev1, ctx->stream);
    (void)hipEventSynchronize(ctx->ev1);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) {
      ctx->k_ms[id] += (double)ms;
      ctx->k_launches[id] += 1;
    }
  }
}

extern "C" int nvk_ctx_create(int device, nvk_ctx **out) {
  if (!out) {
    nvk_set_error("nvk_ctx_create: out is NULL");
    return NVK_ERR_INVALID;
  }
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    nvk_set_error("no HIP device visible (this library has no CPU fallback)");
    return NVK_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= n) {
    nvk_set_error("device %d out of range (0..%d)", device, n - 1);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(device));
  nvk_ctx *c = new (std::nothrow) nvk_ctx();
  if (!c) {
    nvk_set_error("nvk_ctx_create: out of host memory");
    return NVK_ERR_NOMEM;
  }
  memset(c, 0, sizeof *c);
  c->device = device;
  c->meta_n = -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete c;
    nvk_set_error("hipGetDeviceProperties failed");
    return NVK_ERR_HIP;
  }
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // (nvk_ctx_destroy skips what was never created: every handle starts out null)
  if (hipStreamCreate(&c->stream) != hipSuccess || hipStreamCreate(&c->stream2) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
    nvk_ctx_destroy(c);
    nvk_set_error("stream/event creation failed");
    return NVK_ERR_HIP;
  }
  *out = c;
  return NVK_OK;
}

extern "C" void nvk_ctx_destroy(nvk_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  nvk_pipe_release(ctx);  // the lanes of the pipelined host path (threads, their contexts and staging)
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  for (int i = 0; i < WS_COUNT; i++)
    if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->h_plan) (void)hipHostFree(ctx->h_plan);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

extern "C" int nvk_ctx_synchronize(nvk_ctx *ctx) {
  if (!ctx) return NVK_ERR_INVALID;
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" void *nvk_ctx_stream(nvk_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int nvk_ctx_set_slots(nvk_ctx *ctx, int slots) {
  if (!ctx || slots < 0) return NVK_ERR_INVALID;
  ctx->slots_override = slots;
  return NVK_OK;
}

extern "C" int nvk_timing_enable(nvk_ctx *ctx, int on) {
  if (!ctx) return NVK_ERR_INVALID;
  ctx->timing_on = on ? 1 : 0;
  return NVK_OK;
}

extern "C" int nvk_timing_reset(nvk_ctx *ctx) {
  if (!ctx) return NVK_ERR_INVALID;
  for (int i = 0; i < NVK_K_COUNT; i++) {
    ctx->k_ms[i] = 0.0;
    ctx->k_launches[i] = 0;
  }
  return NVK_OK;
}

extern "C" int nvk_timing_read(nvk_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches) {
  if (!ctx || kernel_id < 0 || kernel_id >= NVK_K_COUNT) return NVK_ERR_INVALID;
  if (total_ms) *total_ms = ctx->k_ms[kernel_id];
  if (launches) *launches = ctx->k_launches[kernel_id];
  return NVK_OK;
}

extern "C" int nvk_last_batch_stats(nvk_ctx *ctx, int64_t *band_cells, int64_t *wave_steps,
                                    int64_t *spill_bytes) {
  if (!ctx) return NVK_ERR_INVALID;
  if (band_cells) *band_cells = ctx->last_cells;
  if (wave_steps) *wave_steps = ctx->last_steps;
  if (spill_bytes) *spill_bytes = ctx->last_spill_bytes;
  return NVK_OK;
}

extern "C" int nvk_last_retry_count(nvk_ctx *ctx, int64_t *n_reads) {
  if (!ctx || !n_reads) return NVK_ERR_INVALID;
  *n_reads = ctx->last_retries;
  return NVK_OK;
}

extern "C" int nvk_last_plan_reused(nvk_ctx *ctx, int *reused) {
  if (!ctx || !reused) return NVK_ERR_INVALID;
  *reused = ctx->plan_reused;
  return NVK_OK;
}

extern "C" int nvk_last_tie_count(nvk_ctx *ctx, int64_t *n_reads) {
  if (!ctx || !n_reads) return NVK_ERR_INVALID;
  *n_reads = ctx->last_ties;
  return NVK_OK;
}

extern "C" int nvk_last_tie_counts(nvk_ctx *ctx, int64_t *n_exact, int64_t *n_near, int64_t *n_ulp) {
  if (!ctx) return NVK_ERR_INVALID;
  if (n_exact) *n_exact = ctx->last_ties_exact;
  if (n_near) *n_near = ctx->last_ties_near;
  if (n_ulp) *n_ulp = ctx->last_ties_ulp;
  return NVK_OK;
}

extern "C" int nvk_last_tie_flags(nvk_ctx *ctx, int64_t n_reads, int32_t *out_flags) {
  if (!ctx || !out_flags || n_reads < 0) return NVK_ERR_INVALID;
  if (n_reads != ctx->ties_n) {
    nvk_set_error("nvk_last_tie_flags: the last refine_alignment batch had %lld reads, not %lld",
                  (long long)ctx->ties_n, (long long)n_reads);
    return NVK_ERR_INVALID;
  }
  if (n_reads == 0) return NVK_OK;
  if (ctx->ties_host) {
    memcpy(out_flags, ctx->ties_host, (size_t)n_reads * sizeof(int32_t));
    return NVK_OK;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  NVK_HIP(hipMemcpyAsync(out_flags, ctx->ws[WS_TIES], (size_t)n_reads * sizeof(int32_t), hipMemcpyDeviceToHost,
                         ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_last_launches(nvk_ctx *ctx, int cap, nvk_launch_rec *out, int *n_records) {
  if (!ctx || cap < 0 || (cap > 0 && !out)) return NVK_ERR_INVALID;
  const int kept = ctx->n_launches < NVK_LAUNCH_CAP ? ctx->n_launches : NVK_LAUNCH_CAP;
  for (int i = 0; i < kept && i < cap; i++) out[i] = ctx->launches[i];
  if (n_records) *n_records = ctx->n_launches;
  return NVK_OK;
}

extern "C" int nvk_last_read_skews(nvk_ctx *ctx, int64_t n_reads, int32_t *out_c, int32_t *out_cw) {
  if (!ctx || n_reads < 0) return NVK_ERR_INVALID;
  if (n_reads != ctx->meta_n) {
    nvk_set_error("nvk_last_read_skews: the reads planned last on this ctx by a device-pointer call are %lld, not %lld",
                  (long long)ctx->meta_n, (long long)n_reads);
    return NVK_ERR_INVALID;
  }
  if (n_reads == 0) return NVK_OK;
  std::vector<ReadMeta> h;
  try {
    h.resize((size_t)n_reads);
  } catch (const std::bad_alloc &) {
    nvk_set_error("out of host memory");
    return NVK_ERR_NOMEM;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  NVK_HIP(hipMemcpyAsync(h.data(), ctx->ws[WS_META], (size_t)n_reads * sizeof(ReadMeta), hipMemcpyDeviceToHost,
                         ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  for (int64_t i = 0; i < n_reads; i++) {
    if (out_c) out_c[i] = h[(size_t)i].c;
    if (out_cw) out_cw[i] = h[(size_t)i].cw;
  }
  return NVK_OK;
}

extern "C" int nvk_ctx_set_workspace_limit(nvk_ctx *ctx, int64_t bytes) {
  if (!ctx || bytes < 0) return NVK_ERR_INVALID;
  ctx->ws_limit = bytes;
  nvk_pipe_set_ws_limit(ctx, bytes);
  return NVK_OK;
}

// ---------------------------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------------------------
extern "C" int nvk_model_create(nvk_ctx *ctx, int k, int central_position, int alphabet_size,
                                const double *mean, const double *sigma, int64_t n,
                                nvk_model **out) {
  if (!ctx || !out || !mean || !sigma) {
    nvk_set_error("nvk_model_create: NULL argument");
    return NVK_ERR_INVALID;
  }
  *out = nullptr;
  if (k < 1 || k > 15 || alphabet_size < 2 || alphabet_size > 8 || central_position < 0 ||
      central_position >= k) {
    nvk_set_error("nvk_model_create: unsupported shape k=%d central=%d alphabet=%d", k,
                  central_position, alphabet_size);
    return NVK_ERR_INVALID;
  }
  int64_t want = 1;
  for (int i = 0; i < k; i++) want *= alphabet_size;
  if (n != want) {
    nvk_set_error("nvk_model_create: table has %lld rows, alphabet^k = %lld", (long long)n,
                  (long long)want);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  // additive / multiplicative constants exactly as kmer_model.cpp:9-12 spells them
  std::vector<double> ac, mc;
  try {
    ac.resize((size_t)n);
    mc.resize((size_t)n);
  } catch (const std::bad_alloc &) {
    nvk_set_error("nvk_model_create: out of host memory");
    return NVK_ERR_NOMEM;
  }
  for (int64_t i = 0; i < n; i++) {
    double s = sigma[i];
    ac[(size_t)i] = log(1 / sqrt(2 * M_PI * s * s));
    mc[(size_t)i] = 1 / (2 * s * s);
  }
  nvk_model *m = new (std::nothrow) nvk_model();
  if (!m) {
    nvk_set_error("nvk_model_create: out of host memory");
    return NVK_ERR_NOMEM;
  }
  memset(m, 0, sizeof *m);
  m->ctx = ctx;
  m->id = next_serial();  // (a destroyed model's plan dies with its id: no later model has it)
  size_t bytes = (size_t)n * sizeof(double);
  int rc;
  if ((rc = nvk_alloc((void **)&m->d_mean, bytes, false, "k-mer table")) ||
      (rc = nvk_alloc((void **)&m->d_ac, bytes, false, "k-mer table")) ||
      (rc = nvk_alloc((void **)&m->d_mc, bytes, false, "k-mer table"))) {
    nvk_model_destroy(m);
    return rc;
  }
  if (hipMemcpy(m->d_mean, mean, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->d_ac, ac.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->d_mc, mc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    nvk_set_error("nvk_model_create: copying the table to the device failed");
    nvk_model_destroy(m);
    return NVK_ERR_HIP;
  }
  m->dm.k = k;
  m->dm.central = central_position;
  m->dm.alphabet = alphabet_size;
  m->dm.n = n;
  m->dm.mean = m->d_mean;
  m->dm.ac = m->d_ac;
  m->dm.mc = m->d_mc;
  *out = m;
  return NVK_OK;
}

extern "C" void nvk_model_destroy(nvk_model *m) {
  if (!m) return;
  if (m->d_mean) (void)hipFree(m->d_mean);
  if (m->d_ac) (void)hipFree(m->d_ac);
  if (m->d_mc) (void)hipFree(m->d_mc);
  delete m;
}

extern "C" int nvk_model_info(const nvk_model *m, int *k, int *central_position,
                              int *alphabet_size) {
  if (!m) return NVK_ERR_INVALID;
  if (k) *k = m->dm.k;
  if (central_position) *central_position = m->dm.central;
  if (alphabet_size) *alphabet_size = m->dm.alphabet;
  return NVK_OK;
}

// ---------------------------------------------------------------------------------------------
// argument checks (nvk_internal.h) and helpers
// ---------------------------------------------------------------------------------------------
int check_offsets(const char *what, const int64_t *off, int64_t n) {
  if (!off) {
    nvk_set_error("%s offsets are NULL", what);
    return NVK_ERR_INVALID;
  }
  if (off[0] != 0) {
    nvk_set_error("%s offsets must start at 0", what);
    return NVK_ERR_INVALID;
  }
  for (int64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) {
      nvk_set_error("%s offsets decrease at read %lld", what, (long long)i);
      return NVK_ERR_INVALID;
    }
  return NVK_OK;
}

int nvk_fetch_offsets(nvk_ctx *ctx, const char *what, const int64_t *off, int64_t n, std::vector<int64_t> &h_off,
                      const char *total_name, int64_t total) {
  if (!off) return check_offsets(what, off, n);
  h_off.resize((size_t)n + 1);
  NVK_HIP(hipMemcpyAsync(h_off.data(), off, h_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  int rc = check_offsets(what, h_off.data(), n);
  if (rc) return rc;
  if (total_name && h_off[(size_t)n] != total) {
    nvk_set_error("%s offsets end at %lld, %s is %lld", what, (long long)h_off[(size_t)n], total_name,
                  (long long)total);
    return NVK_ERR_INVALID;
  }
  return NVK_OK;
}

int check_log_costs(const char *what, const char *names, std::initializer_list<double> v) {
  for (double c : v)
    if (!(c <= 0.0) || c * 0.0 != 0.0) {
      double x[4] = {0.0, 0.0, 0.0, 0.0};
      size_t i = 0;
      for (double d : v)
        if (i < 4) x[i++] = d;
      char text[192];
      snprintf(text, sizeof(text), names, x[0], x[1], x[2], x[3]);
      nvk_set_error("%s: %s is not a finite value <= 0", what, text);
      return NVK_ERR_INVALID;
    }
  return NVK_OK;
}

int check_common(nvk_model *model, int64_t n_reads, int bandwidth, int mel) {
  if (!model) {
    nvk_set_error("model handle is NULL");
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff) {
    nvk_set_error("n_reads %lld out of range", (long long)n_reads);
    return NVK_ERR_INVALID;
  }
  if (bandwidth < 0 || bandwidth > (1 << 28)) {
    nvk_set_error("bandwidth %d out of range", bandwidth);
    return NVK_ERR_INVALID;
  }
  if (mel < 0) {
    nvk_set_error("min_event_length %d is negative", mel);
    return NVK_ERR_INVALID;
  }
  return NVK_OK;
}

int check_site_samples(const char *what, nvk_ctx *ctx, int64_t n_rows_a, const int64_t *key_a, const double *val_a,
                       int64_t n_rows_b, const int64_t *key_b, const double *val_b, int64_t n_sites,
                       const int64_t *site_key) {
  if (!ctx || n_rows_a < 0 || n_rows_b < 0 || n_sites < 0) {
    nvk_set_error("%s: invalid argument (ctx, n_rows_a >= 0, n_rows_b >= 0, n_sites >= 0)", what);
    return NVK_ERR_INVALID;
  }
  if (n_sites > 0 && (!site_key || (n_rows_a > 0 && (!key_a || !val_a)) || (n_rows_b > 0 && (!key_b || !val_b)))) {
    nvk_set_error("%s: NULL site_key, or NULL key or values of a sample that has rows", what);
    return NVK_ERR_INVALID;
  }
  return NVK_OK;
}

int check_read_rows(const char *what, nvk_ctx *ctx, int64_t n_reads, int64_t total_ref, const int64_t *ref_off,
                    std::initializer_list<ReadRowsArray> arrays, bool *nothing_to_do) {
  *nothing_to_do = true;
  if (!ctx || n_reads < 0 || n_reads > 0x7fffffff || total_ref < 0) {
    nvk_set_error("%s: invalid argument", what);
    return NVK_ERR_INVALID;
  }
  if (n_reads == 0) {
    if (total_ref != 0) {
      nvk_set_error("%s: total_ref %lld with no reads", what, (long long)total_ref);
      return NVK_ERR_INVALID;
    }
    return NVK_OK;
  }
  bool offs = ref_off;
  for (const auto &x : arrays) offs = offs && x.off;
  if (!offs) {
    nvk_set_error("%s: offsets are NULL", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  int rc;
  if ((rc = nvk_fetch_offsets(ctx, "reference", ref_off, n_reads, off, "total_ref", total_ref))) return rc;
  for (const auto &x : arrays) {
    if ((rc = nvk_fetch_offsets(ctx, x.name, x.off, n_reads, off))) return rc;
    if (off[n_reads] > 0 && !x.data) {  // (a data array may be NULL only when its offsets end at 0)
      nvk_set_error("%s: %s is NULL", what, x.name);
      return NVK_ERR_INVALID;
    }
  }
  *nothing_to_do = total_ref == 0;
  return NVK_OK;
}

namespace {

// The prologue of the two device-pointer operators: their argument checks, the device, and the batch as
// BatchArgs.  An empty batch passes with nothing more to do.
int dev_batch(nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref, int64_t total_anchors,
              const double *signal, const int64_t *sig_off, const int32_t *reference, const int64_t *ref_off,
              const int32_t *ctx_before, const int64_t *cb_off, const int32_t *ctx_after, const int64_t *ca_off,
              const int32_t *anchors, const int64_t *anc_off, int bandwidth, int mel, const int32_t *out_status,
              BatchArgs &a) {
  int rc = check_common(model, n_reads, bandwidth, mel);
  if (rc) return rc;
  if (mel > 4) {
    nvk_set_error("min_event_length %d outside the compiled range 0..4", mel);
    return NVK_ERR_UNSUPPORTED;
  }
  if (total_signal < 0 || total_ref < 0 || total_anchors < 0 || !sig_off || !ref_off || !cb_off || !ca_off ||
      !anc_off || !out_status) {
    nvk_set_error("negative total or NULL offset/status pointer");
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(model->ctx->device));
  a = BatchArgs{n_reads, total_signal, total_ref, total_anchors, signal, sig_off, reference, ref_off,
                ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off, bandwidth, mel};
  return NVK_OK;
}

// What the planner hands back to the host, in one pinned block: the totals, then (refine_alignment) the reads'
// step counts in launch order.
struct PlanHost {
  PlanTotals tot;
  int32_t steps[1];  // [n_reads]
};

// plan a batch: metas, the lane records of kernels_align3, the launch order and the step counts in that order — and,
// with write_rows, the row table of the exact kernel — in ctx workspaces; ONE copy + synchronisation brings the
// totals and the step counts to the host (ctx->h_plan).  In two halves, so that the caller does the host work that
// does not depend on what the planner finds while the planner runs: plan_batch_queue reserves, launches — calling
// `meanwhile` as soon as the planner itself is queued (launch_plan) — and returns; plan_batch_wait queues the copy
// and waits for it.
int plan_batch_queue(nvk_model *model, const BatchArgs &a, int mode, int write_rows, const int **order,
                     const std::function<int()> *meanwhile) {
  nvk_ctx *ctx = model->ctx;
  int64_t n = a.n_reads;
  int64_t rows_total = (mode == PLAN_ALIGN_TRANS) ? 2 * a.total_ref : a.total_ref + n;
  int rc;
  plan_key::clear(ctx->plan_key);  // (the plan held so far is overwritten from here on)
  ctx->rows_current = 0;  // (whatever WS_ROWS holds belongs to an earlier batch from here on)
  ctx->meta_n = -1;       // (... and WS_META)
  if ((rc = nvk_ws_reserve(ctx, WS_META, (size_t)(n + 1) * sizeof(ReadMeta) + 64))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_ROWS, (size_t)(rows_total + 1) * sizeof(RowParam)))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_BANDTMP, (size_t)(2 * (a.total_ref + n) + 2) * 8))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_MISC, 256))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_LANE_F, (size_t)(rows_total + 1) * 48))) return rc;   // sizeof(Lane3), lane3.h
  if ((rc = nvk_ws_reserve(ctx, WS_LANE_R, (size_t)(rows_total + 1) * 48))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_OFFS, (size_t)(rows_total + 1) * sizeof(int32_t)))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_STEPS, (size_t)(n + 1) * sizeof(int32_t)))) return rc;
  // (launch_order's own, made here so that nothing is reserved once the planner is queued: it asks for the order and
  // its bucket counters, far less than a page)
  if ((rc = nvk_ws_reserve(ctx, WS_ORDER, (size_t)n * sizeof(int) + 4096))) return rc;
  if ((rc = nvk_grow(&ctx->h_plan, &ctx->h_plan_cap, sizeof(PlanHost) + (size_t)n * sizeof(int32_t), true,
                     "planner results")))
    return rc;
  PlanTotals *d_tot = nvk_plan_totals(ctx);
  rc = launch_plan(ctx, model->dm, a, mode, (ReadMeta *)ctx->ws[WS_META],
                   (RowParam *)ctx->ws[WS_ROWS], (unsigned long long *)ctx->ws[WS_BANDTMP], d_tot,
                   ctx->ws[WS_LANE_F], ctx->ws[WS_LANE_R], (int32_t *)ctx->ws[WS_OFFS], write_rows, meanwhile);
  if (rc) return rc;
  ctx->rows_current = write_rows ? 1 : 0;
  int *ord = nullptr;
  rc = launch_order(ctx, (const ReadMeta *)ctx->ws[WS_META], n, d_tot, &ord, (int32_t *)ctx->ws[WS_STEPS]);
  if (rc) return rc;
  *order = ord;
  return NVK_OK;
}

int plan_batch_wait(nvk_ctx *ctx, int64_t n, PlanTotals &tot, const int32_t **steps_sorted) {
  PlanHost *hp = (PlanHost *)ctx->h_plan;
  NVK_HIP(hipMemcpyAsync(&hp->tot, nvk_plan_totals(ctx), sizeof(PlanTotals), hipMemcpyDeviceToHost, ctx->stream));
  if (n) NVK_HIP(hipMemcpyAsync(hp->steps, ctx->ws[WS_STEPS], (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  tot = hp->tot;
  *steps_sorted = hp->steps;
  ctx->last_cells = (int64_t)tot.cells;
  ctx->last_steps = (int64_t)tot.steps;
  return NVK_OK;
}

// What plan_batch_queue + plan_batch_wait hand their caller, taken from the plan the ctx holds (ctx->plan_key matches
// the call): the planner's results are a function of the read geometry alone, the workspaces and the pinned block
// still hold them, so nothing is launched, copied or waited for.
void plan_batch_held(nvk_ctx *ctx, PlanTotals &tot, const int **order, const int32_t **steps_sorted) {
  const PlanHost *hp = (const PlanHost *)ctx->h_plan;
  tot = hp->tot;
  *steps_sorted = hp->steps;
  *order = (const int *)ctx->ws[WS_ORDER];
  ctx->last_cells = (int64_t)tot.cells;
  ctx->last_steps = (int64_t)tot.steps;
}

// The row table for a batch that was planned without it (plan_batch_queue, write_rows 0): the planner once more, with
// the table and without the lane records.  It rewrites the metas with the values they hold and leaves the totals, the
// launch order and out_status — by which the exact kernel picks its reads — alone.
int plan_rows_now(nvk_model *model, const BatchArgs &a, int mode) {
  nvk_ctx *ctx = model->ctx;
  if (ctx->rows_current) return NVK_OK;
  int rc = launch_plan(ctx, model->dm, a, mode, (ReadMeta *)ctx->ws[WS_META], (RowParam *)ctx->ws[WS_ROWS],
                       (unsigned long long *)ctx->ws[WS_BANDTMP], nullptr, nullptr, nullptr, nullptr, 1);
  if (rc) return rc;
  ctx->rows_current = 1;
  return NVK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// expected signal
// ---------------------------------------------------------------------------------------------
extern "C" int nvk_expected_signal_batch_dev(nvk_model *model, int64_t n_reads, int64_t total_ref,
                                             const int32_t *reference, const int64_t *ref_off,
                                             const int32_t *ctx_before, const int64_t *cb_off,
                                             const int32_t *ctx_after, const int64_t *ca_off,
                                             double *out) {
  int rc = check_common(model, n_reads, 0, 0);
  if (rc) return rc;
  nvk_ctx *ctx = model->ctx;
  NVK_HIP(hipSetDevice(ctx->device));
  rc = launch_expected(ctx, model->dm, n_reads, total_ref, reference, ref_off, ctx_before, cb_off,
                       ctx_after, ca_off, out);
  if (rc) return rc;
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_expected_signal_batch(nvk_model *model, int64_t n_reads,
                                         const int32_t *reference, const int64_t *ref_off,
                                         const int32_t *ctx_before, const int64_t *cb_off,
                                         const int32_t *ctx_after, const int64_t *ca_off,
                                         double *out) {
  int rc = check_common(model, n_reads, 0, 0);
  if (rc) return rc;
  nvk_ctx *ctx = model->ctx;
  NVK_HIP(hipSetDevice(ctx->device));
  if ((rc = check_offsets("reference", ref_off, n_reads))) return rc;
  if ((rc = check_offsets("context_before", cb_off, n_reads))) return rc;
  if ((rc = check_offsets("context_after", ca_off, n_reads))) return rc;
  hipStream_t s = ctx->stream;
  const size_t no = (size_t)(n_reads + 1) * sizeof(int64_t);
  const int64_t total_ref = ref_off[n_reads];
  NvkTmp d_ref, d_ref_off, d_cb, d_cb_off, d_ca, d_ca_off, d_out;
  if ((rc = d_ref.up(reference, (size_t)total_ref * 4, s))) return rc;
  if ((rc = d_ref_off.up(ref_off, no, s))) return rc;
  if ((rc = d_cb.up(ctx_before, (size_t)cb_off[n_reads] * 4, s))) return rc;
  if ((rc = d_cb_off.up(cb_off, no, s))) return rc;
  if ((rc = d_ca.up(ctx_after, (size_t)ca_off[n_reads] * 4, s))) return rc;
  if ((rc = d_ca_off.up(ca_off, no, s))) return rc;
  if ((rc = d_out.up(nullptr, (size_t)total_ref * 8, s))) return rc;
  rc = launch_expected(ctx, model->dm, n_reads, total_ref, (const int32_t *)d_ref.p, (const int64_t *)d_ref_off.p,
                       (const int32_t *)d_cb.p, (const int64_t *)d_cb_off.p, (const int32_t *)d_ca.p,
                       (const int64_t *)d_ca_off.p, (double *)d_out.p);
  if (rc) return rc;
  if (total_ref) NVK_HIP(hipMemcpyAsync(out, d_out.p, (size_t)total_ref * 8, hipMemcpyDeviceToHost, s));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

// ---------------------------------------------------------------------------------------------
// refine_alignment
// ---------------------------------------------------------------------------------------------
extern "C" int nvk_refine_alignment_batch_dev_keyed(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off, const int32_t *reference,
    const int64_t *ref_off, const int32_t *ctx_before, const int64_t *cb_off,
    const int32_t *ctx_after, const int64_t *ca_off, const int32_t *anchors,
    const int64_t *anc_off, int bandwidth, int min_event_length, int model_transitions,
    int32_t *out_events, int32_t *out_status, uint64_t plan_token) {
  BatchArgs a;
  int rc = dev_batch(model, n_reads, total_signal, total_ref, total_anchors, signal, sig_off, reference, ref_off,
                     ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off, bandwidth, min_event_length,
                     out_status, a);
  if (rc) return rc;
  nvk_launch_reset(model->ctx);
  model->ctx->plan_reused = 0;
  if (n_reads == 0) return rc;
  nvk_ctx *ctx = model->ctx;
  PlanTotals tot;
  // two implementations of the same operator with identical results (both parity-tested):
  //   default                  kernels_align3.hip (plain doubles, wave-uniform scale) with
  //                            kernels_align.hip as the exact fallback for reads it flags
  //   NADAVCA_ALIGN_KERNEL=1   kernels_align.hip only (mantissa+exponent per value)
  const char *force = getenv("NADAVCA_ALIGN_KERNEL");
  ctx->last_retries = 0;
  ctx->last_ties = ctx->last_ties_exact = ctx->last_ties_near = ctx->last_ties_ulp = 0;
  const int *order = nullptr;
  const int32_t *steps_sorted = nullptr;
  const bool exact_all = force && force[0] == '1';
  const int mode = model_transitions ? PLAN_ALIGN_TRANS : PLAN_ALIGN_PLAIN;
  // Everything up to plan_batch_wait is done before the planner is queued or while it runs: the reservations sized by
  // the batch alone first (one that grows drains the stream, which is empty here), then the planner — with the row
  // table only if the exact kernel serves the whole batch — and beside it the fills and the spill cap.  What is left
  // behind the wait is what the planner's totals and step counts decide.
  // WS_TIES: per-read tie bits, then 4 class counts, then the number of reads handed to the exact kernel
  if ((rc = nvk_ws_reserve(ctx, WS_TIES, (size_t)(n_reads + 8) * sizeof(int32_t)))) return rc;
  if (!exact_all && (rc = align3_reserve(ctx, n_reads))) return rc;
  int64_t spill_cap = 0;
  const std::function<int()> meanwhile = [&]() -> int {
    // (the fill covers d_retry; the kernels that write these words are queued behind it)
    NVK_HIP(hipMemsetAsync(ctx->ws[WS_TIES], 0, (size_t)(n_reads + 8) * sizeof(int32_t), ctx->stream));
    return exact_all ? NVK_OK : align3_prepare(ctx, &spill_cap);
  };
  // A batch planned before under the same token (include/nadavca_hip.h: one token, one immutable geometry) and still
  // held by the ctx is not planned again: the sweeps are queued with nothing asked of the device first.  Decided
  // behind the reservations above, which drop the key if they move a block the plan lies in.
  // NADAVCA_PLAN_REUSE=0 (read per call, like NADAVCA_ALIGN_KERNEL): plan every call.
  const char *reuse_env = getenv("NADAVCA_PLAN_REUSE");
  const plan_key::Key want = {plan_token, model->id, bandwidth, min_event_length, model_transitions ? 1 : 0,
                              exact_all ? 1 : 0, n_reads, total_signal, total_ref, total_anchors,
                              {sig_off, reference, ref_off, ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off}};
  if (!(reuse_env && reuse_env[0] == '0') && plan_key::matches(ctx->plan_key, want)) {
    if ((rc = meanwhile())) return rc;
    plan_batch_held(ctx, tot, &order, &steps_sorted);
    ctx->plan_reused = 1;
  } else {
    rc = plan_batch_queue(model, a, mode, exact_all ? 1 : 0, &order, &meanwhile);
    if (rc) return rc;
    if ((rc = plan_batch_wait(ctx, n_reads, tot, &steps_sorted))) return rc;
    if (plan_token) ctx->plan_key = want;
  }
  ctx->ties_n = n_reads;
  ctx->ties_host = nullptr;
  ctx->meta_n = n_reads;
  int32_t *d_ties = (int32_t *)ctx->ws[WS_TIES];
  int *d_retry = (int *)(d_ties + n_reads + 4);
  const ReadMeta *metas = (const ReadMeta *)ctx->ws[WS_META];
  const RowParam *rows = (const RowParam *)ctx->ws[WS_ROWS];
  // reads in which a path decision fell inside the tie margin (include/nadavca_hip.h) and — one copy, one
  // synchronisation for both — the reads the fast kernel handed to the exact one
  int32_t tail[5] = {0, 0, 0, 0, 0};
  auto fetch_counts = [&]() -> int {
    int rc2 = launch_count_flags(ctx, d_ties, n_reads, d_ties + n_reads);
    if (rc2) return rc2;
    NVK_HIP(hipMemcpyAsync(tail, d_ties + n_reads, sizeof tail, hipMemcpyDeviceToHost, ctx->stream));
    NVK_HIP(hipStreamSynchronize(ctx->stream));
    return NVK_OK;
  };
  if (!exact_all) {
    // fast path: plain doubles under a wave-uniform scale (bit-identical while in range);
    // reads it cannot serve come back flagged and are redone by the exact kernel below
    rc = launch_align3(ctx, a, model_transitions ? 1 : 0, metas, tot, order, steps_sorted, out_events, out_status,
                       d_retry, spill_cap);
    if (rc) return rc;
    if ((rc = fetch_counts())) return rc;
    ctx->last_retries = tail[4];
    if (tail[4] > 0) {
      // (rare: the row table is made for the whole batch now, not written for nobody on every batch)
      if ((rc = plan_rows_now(model, a, mode))) return rc;
      rc = launch_align_retry(ctx, a, model_transitions ? 1 : 0, metas, rows, tot, out_events,
                              out_status);
      if (rc) return rc;
      if ((rc = fetch_counts())) return rc;
    }
  } else {
    if ((rc = plan_rows_now(model, a, mode))) return rc;  // (planned with the table: nothing to do)
    rc = launch_align(ctx, a, model_transitions ? 1 : 0, metas, rows, tot, out_events, out_status);
    if (rc) return rc;
    if ((rc = fetch_counts())) return rc;
  }
  ctx->last_ties = tail[0];
  ctx->last_ties_exact = tail[1];
  ctx->last_ties_near = tail[2];
  ctx->last_ties_ulp = tail[3];
  return NVK_OK;
}

extern "C" int nvk_refine_alignment_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off, const int32_t *reference,
    const int64_t *ref_off, const int32_t *ctx_before, const int64_t *cb_off,
    const int32_t *ctx_after, const int64_t *ca_off, const int32_t *anchors,
    const int64_t *anc_off, int bandwidth, int min_event_length, int model_transitions,
    int32_t *out_events, int32_t *out_status) {
  // token 0: plans every call and leaves no plan behind
  return nvk_refine_alignment_batch_dev_keyed(model, n_reads, total_signal, total_ref, total_anchors, signal, sig_off,
                                              reference, ref_off, ctx_before, cb_off, ctx_after, ca_off, anchors,
                                              anc_off, bandwidth, min_event_length, model_transitions, out_events,
                                              out_status, 0);
}

// ---------------------------------------------------------------------------------------------
// estimate_log_likelihoods
// ---------------------------------------------------------------------------------------------
namespace {
// plan + launch of the full matrix (hyp.kind Full, into out_ll) or of listed hypotheses (into hyp.list.out_*)
int ell_run(nvk_model *model, const BatchArgs &a, int model_wobbling, double *out_ll, int32_t *out_status,
            const EllHyp &hyp) {
  int rc;
  const int64_t n_reads = a.n_reads, total_ref = a.total_ref;
  nvk_ctx *ctx = model->ctx;
  const int64_t n = n_reads, nrow = total_ref + n;
  nvk_launch_reset(ctx);  // (also: WS_META takes this batch's metas)
  plan_key::clear(ctx->plan_key);  // (... and WS_ORDER its order: a refine plan held so far is gone)
  if ((rc = nvk_ws_reserve(ctx, WS_META, (size_t)(n + 1) * sizeof(ReadMeta) + 64))) return rc;
  ctx->rows_current = 0;  // (WS_ROWS takes this operator's descriptors)
  if ((rc = nvk_ws_reserve(ctx, WS_ROWS, (size_t)(total_ref + 1) * sizeof(FusedParam)))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_ROWS2, (size_t)(total_ref + 1) * sizeof(FusedParam)))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_BP, (size_t)(3 * nrow + 16) * sizeof(int32_t)))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_BANDTMP, (size_t)(2 * nrow + 2) * 8))) return rc;
  if ((rc = nvk_ws_reserve(ctx, WS_MISC, 256))) return rc;
  EllPlan pl;
  pl.metas = (ReadMeta *)ctx->ws[WS_META];
  pl.fwd = (FusedParam *)ctx->ws[WS_ROWS];
  pl.rev = (FusedParam *)ctx->ws[WS_ROWS2];
  pl.bs = (int32_t *)ctx->ws[WS_BP];
  pl.be = pl.bs + nrow;
  pl.rowoff = pl.be + nrow;
  PlanTotals *d_tot = nvk_plan_totals(ctx);
  rc = launch_plan_ell(ctx, model->dm, a, model_wobbling ? 1 : 0, pl,
                       (unsigned long long *)ctx->ws[WS_BANDTMP], d_tot);
  if (rc) return rc;
  PlanTotals tot;
  NVK_HIP(hipMemcpyAsync(&tot, d_tot, sizeof(PlanTotals), hipMemcpyDeviceToHost, ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  ctx->last_cells = (int64_t)tot.cells;
  ctx->last_steps = (int64_t)tot.steps;
  ctx->meta_n = n;
  rc = launch_ell(ctx, model->dm, a, model_wobbling ? 1 : 0, pl, tot, out_ll, out_status, hyp);
  if (rc) return rc;
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
}  // namespace

extern "C" int nvk_estimate_log_likelihoods_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off, const int32_t *reference,
    const int64_t *ref_off, const int32_t *ctx_before, const int64_t *cb_off,
    const int32_t *ctx_after, const int64_t *ca_off, const int32_t *anchors,
    const int64_t *anc_off, int bandwidth, int min_event_length, int model_wobbling,
    double *out_ll, int32_t *out_status) {
  BatchArgs a;
  int rc = dev_batch(model, n_reads, total_signal, total_ref, total_anchors, signal, sig_off, reference, ref_off,
                     ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off, bandwidth, min_event_length,
                     out_status, a);
  if (rc) return rc;
  nvk_launch_reset(model->ctx);
  if (n_reads == 0) return rc;
  return ell_run(model, a, model_wobbling, out_ll, out_status, EllHyp{});
}

namespace {
// a read's hypothesis list is counted in an int by the kernel
int check_hyp_counts(const std::vector<int64_t> &h_off, int64_t n) {
  for (int64_t j = 0; j < n; j++)
    if (h_off[(size_t)j + 1] - h_off[(size_t)j] > 0x7fffffff) {
      nvk_set_error("read %lld lists more than 2^31 - 1 hypotheses", (long long)j);
      return NVK_ERR_INVALID;
    }
  return NVK_OK;
}

// the second level of a two-level list: hypothesis h owns off[h] .. off[h+1] of arrays of `total` entries
struct HypLevel {
  const char *what;        // "substitution", "insertion": the entries, as messages name them
  const char *total_name;  // the C argument that holds `total`
  int64_t total;
  const int64_t *off;
};

// What the listed-hypothesis entry points do after dev_batch, the same for every kind: the checks of the list (read j
// owns hyp.list.off[j] .. off[j+1] of its total_hyp hypotheses; `level`: their second level, or null) and the launch.
// lists_present: the kind's own arrays are there wherever their level's total is positive.
int hyp_run(nvk_model *model, const BatchArgs &a, int model_wobbling, int32_t *out_status, const EllHyp &hyp,
            const HypLevel *level, bool lists_present) {
  const int64_t total_hyp = hyp.list.total_hyp;
  nvk_launch_reset(model->ctx);
  if (total_hyp < 0 || !hyp.list.off || !hyp.list.out_total || (total_hyp > 0 && !hyp.list.out_hyp) ||
      (level && (level->total < 0 || !level->off)) || !lists_present) {
    if (level)
      nvk_set_error("negative total_hyp / %s or NULL hypothesis / %s / output pointer", level->total_name,
                    level->what);
    else
      nvk_set_error("negative total_hyp or NULL hypothesis / output pointer");
    return NVK_ERR_INVALID;
  }
  if (a.n_reads == 0) {
    if (level && (total_hyp != 0 || level->total != 0))
      nvk_set_error("hypothesis offsets end at 0, total_hyp is %lld and %s %lld", (long long)total_hyp,
                    level->total_name, (long long)level->total);
    else if (total_hyp != 0)
      nvk_set_error("hypothesis offsets end at 0, total_hyp is %lld", (long long)total_hyp);
    else
      return NVK_OK;
    return NVK_ERR_INVALID;
  }
  // the kernel walks every level of the list: each offsets array is checked here, on a host copy
  int rc;
  std::vector<int64_t> h_off;
  if ((rc = nvk_fetch_offsets(model->ctx, "hypothesis", hyp.list.off, a.n_reads, h_off, "total_hyp", total_hyp))) return rc;
  if ((rc = check_hyp_counts(h_off, a.n_reads))) return rc;
  if (level &&
      (rc = nvk_fetch_offsets(model->ctx, level->what, level->off, total_hyp, h_off, level->total_name, level->total)))
    return rc;
  return ell_run(model, a, model_wobbling, nullptr, out_status, hyp);
}
}  // namespace

extern "C" int nvk_estimate_hypotheses_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off, const int32_t *reference,
    const int64_t *ref_off, const int32_t *ctx_before, const int64_t *cb_off,
    const int32_t *ctx_after, const int64_t *ca_off, const int32_t *anchors,
    const int64_t *anc_off, int bandwidth, int min_event_length, int model_wobbling,
    int64_t total_hyp, const int64_t *hyp_off, const int32_t *hyp_pos, const int32_t *hyp_base,
    double *out_total, double *out_hyp, int32_t *out_status) {
  BatchArgs a;
  int rc = dev_batch(model, n_reads, total_signal, total_ref, total_anchors, signal, sig_off, reference, ref_off,
                     ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off, bandwidth, min_event_length,
                     out_status, a);
  if (rc) return rc;
  EllHyp hyp{EllKind::Listed, {hyp_off, out_total, out_hyp, total_hyp}};
  hyp.listed = {hyp_pos, hyp_base};
  return hyp_run(model, a, model_wobbling, out_status, hyp, nullptr, total_hyp <= 0 || (hyp_pos && hyp_base));
}

extern "C" int nvk_estimate_joint_hypotheses_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off, const int32_t *reference,
    const int64_t *ref_off, const int32_t *ctx_before, const int64_t *cb_off,
    const int32_t *ctx_after, const int64_t *ca_off, const int32_t *anchors,
    const int64_t *anc_off, int bandwidth, int min_event_length, int model_wobbling,
    int64_t total_hyp, const int64_t *hyp_off, int64_t total_sub, const int64_t *sub_off, const int32_t *sub_pos,
    const int32_t *sub_base, double *out_total, double *out_hyp, int32_t *out_status) {
  BatchArgs a;
  int rc = dev_batch(model, n_reads, total_signal, total_ref, total_anchors, signal, sig_off, reference, ref_off,
                     ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off, bandwidth, min_event_length,
                     out_status, a);
  if (rc) return rc;
  EllHyp hyp{EllKind::Joint, {hyp_off, out_total, out_hyp, total_hyp}};
  hyp.joint = {sub_off, sub_pos, sub_base};
  const HypLevel subs{"substitution", "total_sub", total_sub, sub_off};
  return hyp_run(model, a, model_wobbling, out_status, hyp, &subs, total_sub <= 0 || (sub_pos && sub_base));
}

extern "C" int nvk_estimate_edit_hypotheses_batch_dev(
    nvk_model *model, int64_t n_reads, int64_t total_signal, int64_t total_ref,
    int64_t total_anchors, const double *signal, const int64_t *sig_off, const int32_t *reference,
    const int64_t *ref_off, const int32_t *ctx_before, const int64_t *cb_off,
    const int32_t *ctx_after, const int64_t *ca_off, const int32_t *anchors,
    const int64_t *anc_off, int bandwidth, int min_event_length, int model_wobbling,
    int64_t total_hyp, const int64_t *hyp_off, const int32_t *edit_pos, const int32_t *edit_del, int64_t total_ins,
    const int64_t *ins_off, const int32_t *ins_base, double *out_total, double *out_hyp, int32_t *out_status) {
  BatchArgs a;
  int rc = dev_batch(model, n_reads, total_signal, total_ref, total_anchors, signal, sig_off, reference, ref_off,
                     ctx_before, cb_off, ctx_after, ca_off, anchors, anc_off, bandwidth, min_event_length,
                     out_status, a);
  if (rc) return rc;
  EllHyp hyp{EllKind::Edit, {hyp_off, out_total, out_hyp, total_hyp}};
  hyp.edit = {edit_pos, edit_del, ins_off, ins_base};
  const HypLevel letters{"insertion", "total_ins", total_ins, ins_off};
  return hyp_run(model, a, model_wobbling, out_status, hyp, &letters,
                 (total_hyp <= 0 || (edit_pos && edit_del)) && (total_ins <= 0 || ins_base));
}
