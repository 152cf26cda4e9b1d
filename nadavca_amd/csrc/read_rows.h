// The device side of a per-read row pass: what the kernels that walk a batch read by read and base by base share
// (mod_rows_kernel, site_rows_kernel, allele_rows_kernel; of kmer_event_kernel, which writes the loop out for its
// registers' sake, the conditions and the event clamp; the clamp also of event_means_kernel).
//
// Work split: ONE WAVE PER READ (grid-stride), its lanes over the read's bases 64 at a time.  A read's offsets, status,
// strand and start are wave-uniform (scalar loads, no per-thread binary search for the owner), and a read that did not
// align costs the wave no sample.  Lane l of a step takes base l, so at every step of a sample loop the wave's 64
// loads fall in one contiguous run of about 64 events' samples (10 samples, 80 B, per event in practice): each cache
// line it fetches serves the neighbouring lanes in the same and the following steps.  Events are 3 to 17 samples long,
// so lanes of a step finish at different times; that divergence is inherent to exact per-event sums and costs VALU
// issue slots, not bytes.  Idle lanes in a read's last step of 64 cost about 1/12 of a 400-base read.
//
// An event of more than 128 samples takes numpy's pairwise walk (npsum.h).  It is rare, and long_event_kernel serves
// it after the main pass, one thread per event, so that the main kernel's registers hold no walk state (the k-mer
// pass ran out of scalar registers with it).
#pragma once
#include "nvk_internal.h"

constexpr int ROWS_NT = 256;  // threads per block of a row pass: four reads

// the batch arrays a row pass may have; those its view does not ask for stay null
struct ReadArrays {
  const int64_t *ref_off;
  const int32_t *status;
  const int64_t *chunk_start;
  const int32_t *reverse;
  const double *signal;
  const int64_t *sig_off;
  const int32_t *ctx_before;
  const int64_t *cb_off;
  const int32_t *ctx_after;
  const int64_t *ca_off;
};
enum : unsigned { RV_SIGNAL = 1, RV_CONTEXTS = 2, RV_STRAND = 4 };  // what a view reads besides ref_off and status

// One read, wave-uniform.  Len: int where the C-ABI keeps a read's samples and bases below 2^31 and the kernel's
// registers are the better for it, else int64_t.
template <class Len>
struct ReadView {
  int64_t rd, r0;  // the read, its first base
  Len R;           // bases
  bool live;       // aligned: no status array, or NVK_READ_OK
  const double *x; // RV_SIGNAL: the samples,
  Len N;           //            their number
  const int32_t *cb, *ca;  // RV_CONTEXTS: the contexts,
  int B, A;                //              their lengths
  bool rev;        // RV_STRAND: reverse strand,
  int64_t start;   //            chunk_start
};

// per_read(view) for every read with bases, one wave per read
template <class Len, unsigned HAS, class PerRead>
__device__ __forceinline__ void for_each_read(const ReadArrays &a, int64_t n_reads, PerRead per_read) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t waves = (int64_t)gridDim.x * (ROWS_NT / 64);
  for (int64_t rd = (int64_t)blockIdx.x * (ROWS_NT / 64) + wave; rd < n_reads; rd += waves) {
    ReadView<Len> v = {};
    v.rd = rd;
    v.r0 = a.ref_off[rd];
    v.R = (Len)(a.ref_off[rd + 1] - v.r0);
    if (v.R <= 0) continue;
    v.live = !a.status || a.status[rd] == NVK_READ_OK;
    if constexpr (HAS & RV_SIGNAL) {
      v.x = a.signal + a.sig_off[rd];
      v.N = (Len)(a.sig_off[rd + 1] - a.sig_off[rd]);
    }
    if constexpr (HAS & RV_CONTEXTS) {
      v.cb = a.ctx_before + a.cb_off[rd];
      v.ca = a.ctx_after + a.ca_off[rd];
      v.B = (int)(a.cb_off[rd + 1] - a.cb_off[rd]);
      v.A = (int)(a.ca_off[rd + 1] - a.ca_off[rd]);
    }
    if constexpr (HAS & RV_STRAND) {
      v.rev = a.reverse[rd] != 0;
      v.start = a.chunk_start[rd];
    }
    per_read(v);
  }
}

// per_base(g) for the bases of the read that this lane takes: lane, lane + 64, ...
template <class Len, class PerBase>
__device__ __forceinline__ void for_each_base(const ReadView<Len> &v, PerBase per_base) {
  for (Len g = (Len)(threadIdx.x & 63); g < v.R; g += 64) per_base(g);
}

// event g of `events` as numpy slices a signal of N samples with it: x[s:e], both ends clamped to 0 .. N; the event
// is empty when e <= s
template <class T, class G>
__device__ __forceinline__ void event_span(const int32_t *events, G g, T N, T &s, T &e) {
  s = events[2 * g];
  e = events[2 * g + 1];
  s = s < 0 ? 0 : (s > N ? N : s);
  e = e < 0 ? 0 : (e > N ? N : e);
}

// base g of R counts when `trim` bases at either end do not
template <class Len>
__device__ __forceinline__ bool counted_base(Len g, Len R, int trim) { return g >= trim && g < R - trim; }

// the k-mer window of base g lies inside contexts | reference | contexts (B and A bases of context)
__device__ __forceinline__ bool window_inside(int g, int k, int central, int R, int B, int A) {
  const int p0 = g - central;  // first base of the window, reference-part coordinates
  return p0 >= -B && p0 + k - 1 < R + A;
}

// The second pass over the events of more than 128 samples: one thread per base, the owner read found by a binary
// search.  F, a functor struct of the caller's:
//   int64_t length(g)       the samples of base g's event as the main pass left them (key[g] >= 0)
//   void operator()(g, xs, n)   takes the event's n samples at xs and writes its values
template <class F>
__global__ __launch_bounds__(ROWS_NT) void long_event_kernel(int64_t n_reads, int64_t total_ref, const double *signal,
                                                             const int64_t *sig_off, const int32_t *events,
                                                             const int64_t *ref_off, const int64_t *key, F f) {
  for (int64_t g = (int64_t)blockIdx.x * ROWS_NT + threadIdx.x; g < total_ref; g += (int64_t)gridDim.x * ROWS_NT) {
    if (key[g] < 0) continue;
    const int64_t n = f.length(g);
    if (n <= 128) continue;
    const int64_t rd = owner_of(ref_off, n_reads, g);
    const int64_t N = sig_off[rd + 1] - sig_off[rd];
    int64_t s, e;
    event_span(events, g, N, s, e);
    f(g, signal + sig_off[rd] + s, n);
  }
}
