// The likelihood of every repeat count for count_repeats_batch(layers=n) (nadavca_amd/repeats.py): the forward sum of an
// item's events over all paths of the repeat's chain that go round its loop exactly c times, for every c < L at once.
// The rules are those of include/nadavca_hip.h (nvk_repeat_likelihoods_dev); the CPU restatement the tests hold this
// kernel to is tests/host_shims/repeatlik_host.cpp, which keeps the full (E, L, N) trellis.
//
// The Viterbi kernel (kernels_repeats.hip) carries the loop count inside the cell; a sum cannot, so the count is a
// second dimension of the trellis, the layer.  One workgroup per item.  Lane l of every wave owns the SPL consecutive
// states l SPL .. l SPL + SPL - 1 of the chain (SPL = 1, 2 or 4, rep_spl), and a wave holds LB consecutive layers of
// them in registers: 32 layers of one state, 16 of two, 16 of four; the workgroup is ceil(L / LB) waves, 4 or 8 at the
// most.  (32 cells per lane for SPL = 4 would be 8 layers and 16 waves, four per SIMD with 128 registers each, which
// the 64 + 16 + 24 registers of cells, sums and tables leave no room in; 16 layers run at two waves per SIMD.)
//
// A row is updated in place, layers descending and inside a layer the lane's states descending, so that every source
// is still the previous row's: the neighbours j - 1 and j - 2 at a lane's first states are the previous lane's last
// two, by DPP wave rotate; the loop's source P[c - 1][lp_from] is read from the lane that owns it, a wave-uniform lane
// and slot, before layer c - 1 is overwritten.  A lane evaluates b once per event for its SPL states and uses it in
// all its layers.  Between waves, per event each wave leaves two values in a double-buffered LDS slot -- its top
// layer's cell of state lp_from for the wave above, and the exponent of its largest value -- and one barrier per event
// separates that write from the next event's reads.  Only the maximum crosses lanes, as an integer exponent (of a
// positive double the exponent grows with the value, so the largest exponent is the exponent of the largest value):
// no sum depends on an order of lanes.  The z_c stay in the lane that owns state N - 1 (0 in the others).  Events are
// loaded 64 at a time and handed out by v_readlane.  No atomics, no workspace, no scratch.
#include <vector>

#include "kmer_hmm.h"
#include "nvk_internal.h"
#include "rep_chain.h"
#include "wave.h"

namespace {

constexpr double LIK_MIN_MOVE = 0x1p-10;   // max(w_stay, w_step) is at least this
constexpr int LIK_NO_EXP = -0x40000000;    // "the exponent" of a wave whose values are all 0

// the layers a wave holds
__host__ __device__ constexpr int lik_lb(int spl) { return spl == 1 ? 32 : 16; }

struct LikArgs {
  const int64_t *items;  // per item (chain, ev_lo, ev_hi)
  const double *level;
  const double *mu, *ac, *mc;  // the chains' states, chain c at st_off[c]
  const int64_t *st_off;
  const int32_t *chain_par;  // per chain (lp_from, lp_to, m1, m2)
  const int32_t *status_in;  // per item or null
  double w_stay, w_step, w_skip, w_trim;
  int L;
  double *out_z, *out_x;
  int32_t *out_status;
};

// v[slot] of lane l, both wave-uniform: every slot's value of that lane, then a choice among scalars (a choice among
// the lane's registers by a uniform slot becomes an indexed load, and the rows then live in scratch)
template <int SPL>
__device__ __forceinline__ double lik_read(const double (&v)[SPL], int slot, int l) {
  double r = rep_readlane(v[0], l);
#pragma unroll
  for (int s = 1; s < SPL; s++) {
    const double q = rep_readlane(v[s], l);
    r = slot == s ? q : r;
  }
  return r;
}

// SPL states per lane; a workgroup whose chain another instantiation serves leaves at once
template <int SPL>
__global__ __launch_bounds__(64 * (NVK_REP_MAX_LAYERS / lik_lb(SPL))) void repeat_lik_kernel(LikArgs a) {
  constexpr int LB = lik_lb(SPL), MAXW = NVK_REP_MAX_LAYERS / LB;
  __shared__ double up[2][MAXW];  // per event parity and wave: the cell of its top layer at state lp_from
  __shared__ int top[2][MAXW];    // ... and the exponent of its largest value
  __shared__ int some[MAXW];      // per wave: whether one of its z_c is above 0
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
  const int64_t it = blockIdx.x;
  const int64_t ch = a.items[3 * it];
  const int64_t s0 = a.st_off[ch];
  const int N = __builtin_amdgcn_readfirstlane((int)(a.st_off[ch + 1] - s0));
  if (rep_spl(N) != SPL) return;
  const int64_t e0 = a.items[3 * it + 1];
  const int E = __builtin_amdgcn_readfirstlane((int)(a.items[3 * it + 2] - e0));
  const int L = a.L;
  int status = a.status_in ? a.status_in[it] : 0;
  if (status == 0 && E == 0) status = NVK_REP_NO_EVENTS;
  if (status != 0) {   // (the whole workgroup: the barriers below are met by all or by none)
    if ((int)threadIdx.x < L) a.out_z[it * L + threadIdx.x] = 0.0;
    if (threadIdx.x == 0) {
      a.out_x[it] = 0.0;
      a.out_status[it] = status;
    }
    return;
  }
  const int32_t *par = a.chain_par + 4 * ch;
  const int lp_from = __builtin_amdgcn_readfirstlane(par[0]), lp_to = __builtin_amdgcn_readfirstlane(par[1]);
  const int from_lane = lp_from / SPL, from_slot = lp_from % SPL, end_lane = (N - 1) / SPL;
  const int c_base = wave * LB;   // the wave's first layer
  const double *lev = a.level + e0;
  const double w_stay = a.w_stay, w_step = a.w_step, w_skip = a.w_skip, w_trim = a.w_trim;

  double mu[SPL], ac[SPL], mc[SPL];
#pragma unroll
  for (int s = 0; s < SPL; s++) {
    const int j = lane * SPL + s;
    mu[s] = j < N ? a.mu[s0 + j] : 0.0;
    ac[s] = j < N ? a.ac[s0 + j] : 0.0;
    mc[s] = j < N ? a.mc[s0 + j] : 0.0;
  }
  // w_step where the lane's state is the loop's target, else 0: the loop's term as one product (0 * v is +0.0)
  double w_loop[SPL];
#pragma unroll
  for (int s = 0; s < SPL; s++) w_loop[s] = lane * SPL + s == lp_to ? w_step : 0.0;
  // b(i, j) of the lane's states for a level e; a state past the chain's end emits 0: its cells are 0 in every row
  const auto emit = [&](double e, double (&b)[SPL]) {
#pragma unroll
    for (int s = 0; s < SPL; s++) {
      const double em = post_exp(fmax(gauss_log(e, mu[s], ac[s], mc[s]), POST_EM_FLOOR));
      b[s] = lane * SPL + s < N ? em : 0.0;
    }
  };
  double cell[LB][SPL], z[LB];
#pragma unroll
  for (int c = 0; c < LB; c++) {
    z[c] = 0.0;   // (row 0: z_c = A(0, c, N-1) = 0, N - 1 is not state 0)
#pragma unroll
    for (int s = 0; s < SPL; s++) cell[c][s] = 0.0;
  }
  // row 0, and what row 1 reads of it: the one cell above 0 is (0, 0, 0)
  double mine = lane < E ? lev[lane] : 0.0;   // the events 64 at a time, one per lane
  {
    double b[SPL];
    emit(rep_readlane(mine, 0), b);
    if (wave == 0 && lane == 0) cell[0][0] = b[0];
    const int ex = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_frexp_exp(b[0]));
    if (lane == 0) {
      top[0][wave] = wave == 0 ? ex : LIK_NO_EXP;
      up[0][wave] = 0.0;
    }
    __syncthreads();
  }
  double o = 1.0;
  int64_t X = 0;
  for (int i = 1; i < E; i++) {
    if ((i & 63) == 0) mine = i + lane < E ? lev[i + lane] : 0.0;
    double b[SPL];
    emit(rep_readlane(mine, i & 63), b);
    const int par_in = (i - 1) & 1;
    int xw = top[par_in][0];
    for (int w = 1; w < nw; w++) xw = max(xw, top[par_in][w]);
    const int x = xw == LIK_NO_EXP ? 0 : xw;
    X += x;
    o = ldexp(o * w_trim, -x);
    const double below = wave > 0 ? up[par_in][wave > 0 ? wave - 1 : 0] : 0.0;
    double m = 0.0;   // the wave's largest value of the new row
#pragma unroll
    for (int c = LB - 1; c >= 0; c--) {
      // the loop's source: the previous row's layer c - 1 (the wave below's top layer for the wave's first)
      const double from = c >= 1 ? lik_read<SPL>(cell[c >= 1 ? c - 1 : 0], from_slot, from_lane) : below;
      // the previous lane's last two states of this layer
      double p1 = dpp_ror1(cell[c][SPL - 1]);
      double p2 = dpp_ror1(SPL >= 2 ? cell[c][SPL >= 2 ? SPL - 2 : 0] : p1);
      if (lane == 0) p1 = p2 = 0.0;
      if (SPL == 1 && lane == 1) p2 = 0.0;   // (lane 0's p1 before it was cut off)
      double fin = 0.0;   // the chain's last state, in the lane that owns it
#pragma unroll
      for (int s = SPL - 1; s >= 0; s--) {
        const double s1 = s >= 1 ? cell[c][s >= 1 ? s - 1 : 0] : p1;
        const double s2 = s >= 2 ? cell[c][s >= 2 ? s - 2 : 0] : s == 1 ? p1 : p2;
        // (a term that does not exist is +0.0, and v + 0.0 is v for every v >= 0: it is added or left out)
        double v = w_step * s1;
        v = v + w_loop[s] * from;
        v = v + w_stay * cell[c][s];
        v = v + w_skip * s2;
        v = ldexp(v, -x);
        if (c == 0 && s == 0 && wave == 0 && lane == 0) v = v + o;
        v = v * b[s];
        v = c_base + c < L ? v : 0.0;   // a path that would need layer L is dropped
        cell[c][s] = v;
        m = fmax(m, v);
        fin = lane * SPL + s == N - 1 ? v : fin;
      }
      z[c] = ldexp(z[c] * w_trim, -x) + fin;
      m = fmax(m, z[c]);
      // layer by layer: left to itself the scheduler starts the layers' rotates and readlanes together, and their
      // results take more registers than the rows
      __builtin_amdgcn_sched_barrier(0);
    }
    // for the next event: the exponent of the wave's largest value, and its top layer's loop source
    const int ex = wave_max_i(m > 0.0 ? __builtin_amdgcn_frexp_exp(m) : LIK_NO_EXP);
    const double mine_up = lik_read<SPL>(cell[LB - 1], from_slot, from_lane);
    if (lane == 0) {
      top[i & 1][wave] = ex;
      up[i & 1][wave] = mine_up;
    }
    __syncthreads();
  }
  bool nz = false;
#pragma unroll
  for (int c = 0; c < LB; c++)
    if (c_base + c < L && lane == end_lane) {
      a.out_z[it * L + c_base + c] = z[c];
      nz = nz || z[c] != 0.0;
    }
  if (lane == end_lane) some[wave] = nz;
  __syncthreads();
  if (threadIdx.x == 0) {
    int any = 0;
    for (int w = 0; w < nw; w++) any |= some[w];
    a.out_x[it] = (double)X;
    a.out_status[it] = any ? NVK_REP_OK : NVK_REP_NO_PATH;
  }
}

}  // namespace

extern "C" int nvk_repeat_likelihoods_dev(nvk_ctx *ctx, int64_t n_items, const int64_t *items, int64_t total_events,
                                          const double *level, int64_t n_chains, int64_t total_states,
                                          const double *mu, const double *ac, const double *mc, const int64_t *st_off,
                                          const int32_t *chain_par, double w_stay, double w_step, double w_skip,
                                          double w_trim, int layers, const int32_t *status_in, double *out_z,
                                          double *out_x, int32_t *out_status, double *out_ms) {
  const char *what = "nvk_repeat_likelihoods_dev";
  if (out_ms) *out_ms = 0.0;
  if (!ctx) {
    nvk_set_error("%s: ctx is NULL", what);
    return NVK_ERR_INVALID;
  }
  if (n_items < 0 || n_items > (1 << 30) || n_chains < 0 || n_chains > 0x7fffffff ||
      total_events < 0 || total_states < 0) {
    nvk_set_error("%s: n_items %lld, n_chains %lld, total_events %lld or total_states %lld out of range", what,
                  (long long)n_items, (long long)n_chains, (long long)total_events, (long long)total_states);
    return NVK_ERR_INVALID;
  }
  if (layers < 1) {
    nvk_set_error("%s: layers %d is below 1", what, layers);
    return NVK_ERR_INVALID;
  }
  if (layers > NVK_REP_MAX_LAYERS) {
    nvk_set_error("%s: layers %d is above %d", what, layers, (int)NVK_REP_MAX_LAYERS);
    return NVK_ERR_UNSUPPORTED;
  }
  const double weights[4] = {w_stay, w_step, w_skip, w_trim};
  for (double w : weights)
    if (!(w > 0.0 && w <= 1.0)) {
      nvk_set_error("%s: w_stay %g, w_step %g, w_skip %g or w_trim %g is not a finite value in (0, 1]", what, w_stay,
                    w_step, w_skip, w_trim);
      return NVK_ERR_INVALID;
    }
  if (!((w_stay > w_step ? w_stay : w_step) >= LIK_MIN_MOVE)) {
    nvk_set_error("%s: w_stay %g and w_step %g are both below 2^-10", what, w_stay, w_step);
    return NVK_ERR_INVALID;
  }
  if (n_items == 0) return NVK_OK;
  if (!items || !st_off || !chain_par || (total_events > 0 && !level) || !mu || !ac || !mc || !out_z || !out_x ||
      !out_status) {
    nvk_set_error("%s: NULL items, levels, offsets, chain tables or output", what);
    return NVK_ERR_INVALID;
  }
  bool used[5];   // by states per lane
  if (int rc = rep_check_batch(what, ctx, n_items, items, total_events, n_chains, total_states, st_off, chain_par, used))
    return rc;
  LikArgs a;
  a.items = items;
  a.level = level;
  a.mu = mu;
  a.ac = ac;
  a.mc = mc;
  a.st_off = st_off;
  a.chain_par = chain_par;
  a.status_in = status_in;
  a.w_stay = w_stay;
  a.w_step = w_step;
  a.w_skip = w_skip;
  a.w_trim = w_trim;
  a.L = layers;
  a.out_z = out_z;
  a.out_x = out_x;
  a.out_status = out_status;
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (out_ms) {
    for (hipEvent_t &e : ev) NVK_HIP(hipEventCreate(&e));
    NVK_HIP(hipEventRecord(ev[0], ctx->stream));
  }
  // one workgroup per item in every instantiation some item's chain needs, of as many waves as hold the layers: the
  // others' workgroups leave at once
  const dim3 grid((unsigned)n_items);
  const auto block = [&](int spl) { return dim3(64u * (unsigned)((layers + lik_lb(spl) - 1) / lik_lb(spl))); };
  if (used[1]) hipLaunchKernelGGL(repeat_lik_kernel<1>, grid, block(1), 0, ctx->stream, a);
  if (used[2]) hipLaunchKernelGGL(repeat_lik_kernel<2>, grid, block(2), 0, ctx->stream, a);
  if (used[4]) hipLaunchKernelGGL(repeat_lik_kernel<4>, grid, block(4), 0, ctx->stream, a);
  NVK_HIP(hipGetLastError());
  if (out_ms) NVK_HIP(hipEventRecord(ev[1], ctx->stream));
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  if (out_ms) {
    float ms = 0.f;
    NVK_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *out_ms = (double)ms;
    for (hipEvent_t e : ev) NVK_HIP(hipEventDestroy(e));
  }
  return NVK_OK;
}
