// Self-test entries: helpers whose failure no result can show get a kernel of their own (include/nadavca_hip.h).
//
// wave_max_i (wave.h) feeds the sweeps' rescale decision (kernels_align3.hip).  A rescale by any common power of two
// is exact, so a wrong maximum changes no event: at worst it sends a read to the exact kernel.  No parity test can
// see it; this kernel hands the function rows of 64 values and returns what it says.
#include "nvk_internal.h"
#include "wave.h"

namespace {

// one wave per workgroup; wave w reduces in[w][0..63]
__global__ __launch_bounds__(64) void selftest_wave_max_kernel(const int32_t *in, int64_t n, int32_t *out) {
  const int lane = threadIdx.x;
  for (int64_t w = blockIdx.x; w < n; w += gridDim.x) {  // (uniform bounds: all 64 lanes stay enabled)
    const int mx = wave_max_i(in[w * 64 + lane]);
    if (lane == 0) out[w] = mx;
  }
}

}  // namespace

extern "C" int nvk_selftest_wave_max(nvk_ctx *ctx, const int32_t *in, int64_t n, int32_t *out) {
  if (!ctx || n < 0 || (n > 0 && (!in || !out))) {
    nvk_set_error("nvk_selftest_wave_max: invalid argument");
    return NVK_ERR_INVALID;
  }
  if (n == 0) return NVK_OK;
  NVK_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(selftest_wave_max_kernel, dim3(grid_of(n, 1)), dim3(64), 0, ctx->stream, in, n, out);
  NVK_HIP(hipGetLastError());
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  return NVK_OK;
}
