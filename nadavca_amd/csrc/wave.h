// Wave64 helpers shared by the kernels: the wave-local barrier, DPP moves of a neighbour's value, a wave-uniform
// value, butterfly reductions and inclusive scans over the 64 lanes.
#pragma once
#include <hip/hip_runtime.h>

// LDS traffic of a wave is executed in program order, so ordering between the lanes of ONE wave only needs the
// compiler not to reorder the accesses.  (__syncthreads() would also drain vmcnt, i.e. wait for the spill stores of
// every step.)
#define WAVE_SYNC()                                        \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
  } while (0)

// value of the previous lane (DPP row_shr:1 with bound_ctrl: the first lane of each 16-lane row reads 0)
__device__ __forceinline__ double dpp_shr1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x111, 0xf, 0xf, true);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x111, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// value of lane (l - 1) mod 64 (DPP wave_ror:1, GFX9)
__device__ __forceinline__ int dpp_ror1(int v) { return __builtin_amdgcn_mov_dpp(v, 0x13C, 0xf, 0xf, false); }
__device__ __forceinline__ double dpp_ror1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x13C, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x13C, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// value of lane (l + 1) mod 64 (DPP wave_rol:1, GFX9)
__device__ __forceinline__ double dpp_rol1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0x134, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, 0x134, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// a value that is the same in every lane, as one the compiler knows to be (loop bounds in scalar registers)
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)(uint64_t)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((int)(unsigned)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// reductions over the wave, the result in every lane
__device__ __forceinline__ int wave_max(int v) {
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
// wave_sum of N values at once, their butterflies interleaved (each value's additions in wave_sum's order)
template <int N>
__device__ __forceinline__ void wave_sum_n(double (&v)[N]) {
  for (int d = 32; d >= 1; d >>= 1) {
    double o[N];
#pragma unroll
    for (int a = 0; a < N; a++) o[a] = __shfl_xor(v[a], d, 64);
#pragma unroll
    for (int a = 0; a < N; a++) v[a] += o[a];
  }
}

// inclusive scan: lane l gets the sum of lanes 0 .. l
__device__ __forceinline__ int wave_scan_add(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// Inclusive scans (sum / maximum / minimum of lanes 0 .. l) on the DPP path: row shifts inside the 16-lane rows, then the two row broadcasts of GFX9
// (lane 15 of a row to the next row, lane 31 to the upper half).  No trip through the LDS crossbar, which is what a
// serial chain of scans waits for.  `ident`: the operation's neutral element, taken by lanes without a source.
#define WAVE_SCAN_DPP_STEP(ctrl, rows) v = op(v, __builtin_amdgcn_update_dpp(ident, v, ctrl, rows, 0xf, false))
template <class Op>
__device__ __forceinline__ int wave_scan_dpp(int v, const int ident, Op op) {
  WAVE_SCAN_DPP_STEP(0x111, 0xf);  // row_shr:1
  WAVE_SCAN_DPP_STEP(0x112, 0xf);  // row_shr:2
  WAVE_SCAN_DPP_STEP(0x114, 0xf);  // row_shr:4
  WAVE_SCAN_DPP_STEP(0x118, 0xf);  // row_shr:8
  WAVE_SCAN_DPP_STEP(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
  WAVE_SCAN_DPP_STEP(0x143, 0xc);  // row_bcast:31 into rows 2 and 3
  return v;
}
#undef WAVE_SCAN_DPP_STEP
__device__ __forceinline__ int wave_scan_add_dpp(int v) {
  return wave_scan_dpp(v, 0, [](int a, int b) { return a + b; });
}
__device__ __forceinline__ int wave_scan_max_dpp(int v) {
  return wave_scan_dpp(v, (int)0x80000000, [](int a, int b) { return max(a, b); });
}
__device__ __forceinline__ int wave_scan_min_dpp(int v) {
  return wave_scan_dpp(v, 0x7fffffff, [](int a, int b) { return min(a, b); });
}

// Maximum of the wave in a scalar register: the last lane of the DPP scan (six v_max_i32_dpp and one v_readlane_b32;
// the butterfly of wave_max is six ds_bpermute_b32, each waited for, on the chain of whoever calls it once per
// rescale period).  Needs all 64 lanes enabled, as every DPP read of a neighbour does; nvk_selftest_wave_max
// (include/nadavca_hip.h) runs this very function against a host maximum.
__device__ __forceinline__ int wave_max_i(int v) { return __builtin_amdgcn_readlane(wave_scan_max_dpp(v), 63); }
