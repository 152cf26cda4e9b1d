// Wave64 helpers shared by the kernels: the wave-local barrier, DPP moves of a neighbour's value, butterfly
// reductions and inclusive scans over the 64 lanes.
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

// inclusive scans: lane l gets the sum / maximum of lanes 0 .. l, or the minimum of lanes l .. 63
__device__ __forceinline__ int wave_scan_add(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
__device__ __forceinline__ int wave_scan_max(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    int o = __shfl_up(v, d, 64);
    if (lane >= d) v = max(v, o);
  }
  return v;
}
__device__ __forceinline__ int wave_scan_min_rev(int v, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    int o = __shfl_down(v, d, 64);
    if (lane + d < 64) v = min(v, o);
  }
  return v;
}
