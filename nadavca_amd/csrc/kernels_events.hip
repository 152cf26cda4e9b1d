// Event detection for signal_map_batch (nadavca_amd/signal_map.py): where the level of a read's normalised signal
// jumps, and the mean level between two jumps.  The rules are those of include/nadavca_hip.h (nvk_event_flags_dev,
// nvk_event_levels_dev); the CPU restatement the tests hold these kernels to is tests/host_shims/events_host.cpp.
//
//   nvk_event_flags_dev    per sample, 1 where an event starts (a border), else 0
//   nvk_event_levels_dev   per event, its first sample, its length and its mean level; the caller takes the events'
//                          positions and the per-read counts from the flags with a nonzero / prefix sum
//
// Flags: one thread per sample of the batch's flat signal, EV_TILE samples per block.  A thread computes the statistic
// s of its own sample from the 2 w samples around it (ascending loops, as the contract writes them) and leaves it in
// LDS; the first 2 (w - 1) threads also compute the halo, w - 1 positions on each side of the tile.  The local-maximum
// test then reads 2 w - 1 values from LDS.  A position takes the read that owns it from a binary search over sig_off;
// s is 0 within w samples of a read's ends, and a border candidate lies at least w samples inside its read, so the
// window of the maximum test never leaves the read and the flat array of statistics serves every read at once.
//
// Levels: one thread per event, an ascending sum over its samples.  Events are a few samples long, so neighbouring
// threads read neighbouring lines; a small bandwidth-bound pass, not tuned.
#include <vector>

#include "nvk_internal.h"

namespace {

constexpr int EV_TILE = 256;
constexpr int EV_WMAX = 8;  // largest window compiled in

// s at flat position g (0 outside the signal): the read that owns g is found first
__device__ __forceinline__ double event_stat(const double *x, const int64_t *sig_off, int64_t n_reads, int64_t total,
                                             int64_t g, int w, double var_floor) {
  if (g < 0 || g >= total) return 0.0;
  const int64_t rd = owner_of(sig_off, n_reads, g);
  const int64_t i = g - sig_off[rd], n = sig_off[rd + 1] - sig_off[rd];
  if (i < w || i > n - w) return 0.0;
  const double *p = x + g;
  double sl = 0.0, sr = 0.0;
  for (int t = 0; t < w; t++) sl += p[t - w];
  for (int t = 0; t < w; t++) sr += p[t];
  const double ml = sl / (double)w, mr = sr / (double)w;
  double vl = 0.0, vr = 0.0;
  for (int t = 0; t < w; t++) {
    const double d = p[t - w] - ml;
    vl += d * d;
  }
  for (int t = 0; t < w; t++) {
    const double d = p[t] - mr;
    vr += d * d;
  }
  vl = vl / (double)w;
  vr = vr / (double)w;
  const double d = mr - ml;
  return ((double)w * (d * d)) / ((vl + vr) + var_floor);
}

__global__ __launch_bounds__(EV_TILE) void event_flags_kernel(int64_t n_reads, int64_t total, const double *x,
                                                              const int64_t *sig_off, int w, double threshold,
                                                              double var_floor, int32_t *out_flags) {
  __shared__ double s_stat[EV_TILE + 2 * (EV_WMAX - 1)];
  const int halo = w - 1;
  for (int64_t t0 = (int64_t)blockIdx.x * EV_TILE; t0 < total; t0 += (int64_t)gridDim.x * EV_TILE) {
    __syncthreads();  // (the previous tile's reads of s_stat)
    // slot u of s_stat holds position t0 - halo + u
    s_stat[halo + threadIdx.x] = event_stat(x, sig_off, n_reads, total, t0 + threadIdx.x, w, var_floor);
    if ((int)threadIdx.x < 2 * halo) {
      const int u = (int)threadIdx.x < halo ? (int)threadIdx.x : EV_TILE + (int)threadIdx.x;
      s_stat[u] = event_stat(x, sig_off, n_reads, total, t0 - halo + u, w, var_floor);
    }
    __syncthreads();
    const int64_t g = t0 + threadIdx.x;
    if (g < total) {
      const int c = halo + threadIdx.x;
      const double s = s_stat[c];
      bool border = s >= threshold;
      for (int u = 1; u <= halo; u++) border = border && s > s_stat[c - u] && s >= s_stat[c + u];
      const int64_t rd = owner_of(sig_off, n_reads, g);
      out_flags[g] = (g == sig_off[rd] || border) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(256) void event_levels_kernel(int64_t n_reads, int64_t total, const double *x,
                                                           const int64_t *sig_off, int64_t n_events,
                                                           const int64_t *ev_pos, int32_t *out_start,
                                                           int32_t *out_len, double *out_level) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_events; e += (int64_t)gridDim.x * 256) {
    int64_t a = ev_pos[e];
    a = a < 0 ? 0 : a >= total ? total - 1 : a;  // (positions are checked by the caller's flags; this keeps any in bounds)
    const int64_t rd = owner_of(sig_off, n_reads, a);
    int64_t b = e + 1 < n_events ? ev_pos[e + 1] : total;
    const int64_t end = sig_off[rd + 1];
    b = b > end ? end : b;
    double sum = 0.0;
    for (int64_t g = a; g < b; g++) sum += x[g];
    out_start[e] = (int32_t)(a - sig_off[rd]);
    out_len[e] = (int32_t)(b - a);
    out_level[e] = sum / (double)(b - a);
  }
}

constexpr int64_t EV_MAX_READ = 0x7fffffff;  // a sample's position inside its read is an int32

// the checks both entries share: sig_off is copied to the host and checked, and ends at total_signal
int events_check(const char *what, nvk_ctx *ctx, int64_t n_reads, int64_t total_signal, const double *signal,
                 const int64_t *sig_off) {
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_reads < 0 || n_reads > 0x7fffffff || total_signal < 0) {
    nvk_set_error("%s: n_reads %lld or total_signal %lld out of range", what, (long long)n_reads,
                  (long long)total_signal);
    return NVK_ERR_INVALID;
  }
  if (!sig_off || (total_signal > 0 && !signal)) {
    nvk_set_error("%s: NULL signal or offsets", what);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> off;
  int rc = nvk_fetch_offsets(ctx, "signal", sig_off, n_reads, off, "total_signal", total_signal);
  if (rc) return rc;
  for (int64_t r = 0; r < n_reads; r++)
    if (off[r + 1] - off[r] > EV_MAX_READ) {
      nvk_set_error("%s: read %lld has %lld samples, above %lld", what, (long long)r, (long long)(off[r + 1] - off[r]),
                    (long long)EV_MAX_READ);
      return NVK_ERR_INVALID;
    }
  return NVK_OK;
}

}  // namespace

extern "C" int nvk_event_flags_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_signal, const double *signal,
                                   const int64_t *sig_off, int window, double threshold, double var_floor,
                                   int32_t *out_flags) {
  int rc = events_check("nvk_event_flags_dev", ctx, n_reads, total_signal, signal, sig_off);
  if (rc) return rc;
  if (window > EV_WMAX) {
    nvk_set_error("nvk_event_flags_dev: window %d is above the compiled limit %d", window, EV_WMAX);
    return NVK_ERR_UNSUPPORTED;
  }
  if (window < 1 || !(threshold > 0.0) || !(var_floor > 0.0)) {
    nvk_set_error("nvk_event_flags_dev: window %d, threshold %g or var_floor %g out of range", window, threshold,
                  var_floor);
    return NVK_ERR_INVALID;
  }
  if (total_signal == 0) return NVK_OK;
  if (!out_flags) {
    nvk_set_error("nvk_event_flags_dev: out_flags is NULL");
    return NVK_ERR_INVALID;
  }
  hipLaunchKernelGGL(event_flags_kernel, dim3(grid_of(total_signal, EV_TILE)), dim3(EV_TILE), 0, ctx->stream, n_reads,
                     total_signal, signal, sig_off, window, threshold, var_floor, out_flags);
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}

extern "C" int nvk_event_levels_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_signal, const double *signal,
                                    const int64_t *sig_off, int64_t n_events, const int64_t *ev_pos,
                                    int32_t *out_start, int32_t *out_len, double *out_level) {
  int rc = events_check("nvk_event_levels_dev", ctx, n_reads, total_signal, signal, sig_off);
  if (rc) return rc;
  if (n_events < 0 || n_events > total_signal) {
    nvk_set_error("nvk_event_levels_dev: n_events %lld outside 0 .. total_signal %lld", (long long)n_events,
                  (long long)total_signal);
    return NVK_ERR_INVALID;
  }
  if (n_events == 0) return NVK_OK;
  if (!ev_pos || !out_start || !out_len || !out_level) {
    nvk_set_error("nvk_event_levels_dev: NULL event positions or output");
    return NVK_ERR_INVALID;
  }
  hipLaunchKernelGGL(event_levels_kernel, dim3(grid_of(n_events, 256)), dim3(256), 0, ctx->stream, n_reads,
                     total_signal, signal, sig_off, n_events, ev_pos, out_start, out_len, out_level);
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
