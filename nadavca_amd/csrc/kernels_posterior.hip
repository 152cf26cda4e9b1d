// Forward-backward over the 4^k k-mer states, and the three operators that stand on it: nvk_kmer_posterior_dev
// (decode_batch(qualities=True), nadavca_amd/decode.py: per event the posterior of each of the four letters at one
// position of the state), nvk_kmer_expectations_dev (decode_batch(fit=n): the E-step's sums per read) and
// nvk_kmer_state_moments_dev (estimate_decode_model, nadavca_amd/decode_train.py: per state the moments of the levels),
// each with the likelihood of a read's events summed over all paths.  The rules are those of include/nadavca_hip.h; the
// CPU restatement the tests hold these kernels to is tests/host_shims/kmer_fb_host.cpp, which keeps the full S x E
// matrices.
//
// All sweeps follow the Viterbi sweep of kernels_decode.hip: one workgroup per read, T = S / 16 threads (1, 4, 16, 64
// or 256 for k = 2..6), thread u owns the 16 consecutive states 16 u .. 16 u + 15, whose table entries stay in
// registers for the whole read, and one barrier per event.
//
// THE FORWARD SWEEP is the Viterbi sweep with sums where that one takes maxima: per event a thread reads the 16 skip
// predecessors c T + u and the four times four step predecessors a Q + 4 u + g of the previous row from LDS (two padded
// row buffers, as there), forms 16 emissions and writes its 16 values of A(i, .) to LDS and, as eight 16-byte pairs,
// to the row store in global memory.  The row is rescaled by the exponent of the previous row's largest value: every
// wave leaves its own largest value in LDS before the barrier, and every thread joins the waves' values after it.
//
// THE BACKWARD STEP (BackSweep below) is what the three sweeps that follow a forward sweep share, each a launch of its
// own.  B and W = B * b stay in registers; the successors factorise as the predecessors do (by a step
// (s mod Q) 4 + 0..3, by a skip (s mod T) 16 + 0..15), so the threads share only the sums G4 of four and G16 of sixteen
// consecutive W: before the event's barrier thread u publishes G4[4 u .. 4 u + 3] (already times w_step), G16[u]
// (times w_skip) and its wave's largest B; after it every thread reads 16 consecutive entries of each, joins the
// waves' largest B and advances its B to the event before.  What a sweep does with A * B between the two, and the
// order of its work inside an event, is its own and is described at its kernel.
//
// THE ROW STORE takes 8 * 4^k bytes per event (32 KB at k = 6), the rows of a read one after another from
// ev_off[r] - ev_off[r0] on, r0 the part's first read.  Inside a row the layout is the sweeps' own: state 16 u + 2 q + h
// lies at q 2 T + 2 u + h, so that one 16-byte access per lane covers 1 KB of consecutive memory per wave (with a
// thread's 16 values side by side every lane of an access would touch another 128-byte line).  The store is the seed
// aligner's traceback workspace, as the Viterbi store is; the host cuts a batch into parts whose rows fit the cap and
// runs the forward and the second sweep of a part before the next part's.
//
// No atomics, no scratch, no library exp or log: EXP is rint, the fma chain of xm::exp2_frac_horner and ldexp.  With
// -ffp-contract=off every value is the rounded operation the contract writes, on the device as on the host.
#include <algorithm>
#include <vector>

#include "kmer_hmm.h"
#include "nvk_internal.h"
#include "part_cut.h"
#include "xmath.h"

namespace {

constexpr double POST_MIN_MOVE = 0x1p-10;  // max(w_stay, w_step) is at least this

struct PostArgs : HmmIn {
  double w_stay, w_step, w_skip;
  double *out_marg, *out_z;
  int32_t *out_status;
  double *rows;  // the row store: the part's first read starts at double 0
  int r0;        // the part's first read
  int pos;
};

// Where the j-th of a thread's 16 values lies in a row of the store, from the thread's first pair on: the threads'
// pairs (j, j + 1) side by side, so that the 16-byte accesses of a wave's lanes are consecutive, 1 KB per instruction
template <int T>
__device__ __forceinline__ constexpr int post_store_at(int j) { return (j >> 1) * 2 * T + (j & 1); }

// b(i, s) for a level e
__device__ __forceinline__ double post_emission(double e, double mean, double ac, double mc) {
  return post_exp(fmax(gauss_log(e, mean, ac, mc), POST_EM_FLOOR));
}

// the butterfly of wave_sum over the W lanes of a workgroup's wave that hold a thread (W = min(T, 64))
// (N sums at once: per stage N shuffles, then N additions)
template <int W, int N>
__device__ __forceinline__ void post_wave_sum_n(double (&v)[N]) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) {
    double o[N];
#pragma unroll
    for (int x = 0; x < N; x++) o[x] = __shfl_xor(v[x], d, 64);
#pragma unroll
    for (int x = 0; x < N; x++) v[x] = v[x] + o[x];
  }
}
template <int W>
__device__ __forceinline__ double post_wave_sum(double v) {
  double one[1] = {v};
  post_wave_sum_n<W>(one);
  return one[0];
}
template <int W>
__device__ __forceinline__ double post_wave_max(double v) {
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
  return v;
}
// the waves' values of a sum over all states, joined: (g0 + g1) + (g2 + g3) for four waves
template <int NW>
__device__ __forceinline__ double post_join_sum(const double *g, int stride) {
  if (NW == 1) return g[0];
  return (g[0] + g[stride]) + (g[2 * stride] + g[3 * stride]);
}
template <int NW>
__device__ __forceinline__ double post_join_max(const double *g) {
  double m = g[0];
#pragma unroll
  for (int w = 1; w < NW; w++) m = fmax(m, g[w]);
  return m;
}

// What the sweeps of a read share: where the read and the thread's part of it lie, and the backward step.  The
// kernels keep their LDS buffers and hand in those of the event's parity: G4 and G16 (padded as rows are, holding
// w_step * G4 and w_skip * G16) and wave_top (per wave the largest B of the event).
template <int K>
struct BackSweep {
  static constexpr int S = KmerHmm<K>::S, T = KmerHmm<K>::T, Q = KmerHmm<K>::Q, W = KmerHmm<K>::W, NW = KmerHmm<K>::NW;
  static constexpr int G4_ROW = Q + (Q >> 4) * HMM_PAD + HMM_PAD, G16_ROW = T + (T >> 4) * HMM_PAD + HMM_PAD;
  int u, wave, E;
  int64_t rd, ev0;
  const double *lev;
  double *store;  // the read's rows, from the thread's first pair on
  // where the successors' sums of the thread's 16 states lie: s mod Q and s mod T are 16 consecutive entries from a
  // multiple of 16 on, or (Q or T below 16) the entries j mod Q, j mod T of the first block -- one address and
  // constant offsets, not 16 addresses in registers
  int q0, t0;
  double w_stay, w_step, w_skip;

  // -> the read's status: 0 if it is processed (the rest is filled in only then)
  __device__ __forceinline__ int begin(const PostArgs &a) {
    u = threadIdx.x;
    wave = u / W;
    rd = (int64_t)a.r0 + blockIdx.x;
    ev0 = a.ev_off[rd];
    E = (int)(a.ev_off[rd + 1] - ev0);
    const int status = hmm_status(a, rd, E);
    if (status != 0) return status;
    lev = a.level + ev0;
    w_stay = a.w_stay, w_step = a.w_step, w_skip = a.w_skip;
    store = a.rows + (ev0 - a.ev_off[a.r0]) * (int64_t)S + 2 * u;
    q0 = hmm_at((16 * u) & (Q - 1)), t0 = hmm_at((16 * u) & (T - 1));
    return 0;
  }

  // the thread's 16 values of A(i, .)
  __device__ __forceinline__ void load_row(int i, double (&av)[16]) const {
    const double *in = store + (int64_t)i * S;
#pragma unroll
    for (int j = 0; j < 16; j++) av[j] = in[post_store_at<T>(j)];
  }

  // Before the barrier of event i > 0, from B(i, .) and the level e of the event: the wave's largest B to wave_top,
  // W = B * b to Wv, the thread's sums to G4 and G16.  -> (EM) the largest em of the thread's 16 states
  template <bool EM>
  __device__ __forceinline__ double publish(const double (&B)[16], double e, const double (&mean)[16],
                                            const double (&ac)[16], const double (&mc)[16], double (&Wv)[16],
                                            double *G4, double *G16, double *wave_top) const {
    double top = B[0];
#pragma unroll
    for (int j = 1; j < 16; j++) top = fmax(top, B[j]);
    top = post_wave_max<W>(top);
    if ((u & (W - 1)) == 0) wave_top[wave] = top;
    double emx = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const double g = gauss_log(e, mean[j], ac[j], mc[j]);
      if (EM) emx = j == 0 ? g : fmax(emx, g);
      Wv[j] = B[j] * post_exp(fmax(g, POST_EM_FLOOR));
    }
    double g4[4];
#pragma unroll
    for (int g = 0; g < 4; g++) g4[g] = ((Wv[4 * g] + Wv[4 * g + 1]) + Wv[4 * g + 2]) + Wv[4 * g + 3];
    const double g16 = ((g4[0] + g4[1]) + g4[2]) + g4[3];
#pragma unroll
    for (int g = 0; g < 4; g++) G4[hmm_at(4 * u) + g] = w_step * g4[g];
    G16[hmm_at(u)] = w_skip * g16;
    return emx;
  }

  // After that barrier: B(i - 1, .), rescaled by the exponent of the largest B(i, .).  stay(j, w_stay * W[j]) sees the
  // stay term of every state
  template <class F>
  __device__ __forceinline__ void advance(double (&B)[16], const double (&Wv)[16], const double *G4, const double *G16,
                                          const double *wave_top, F &&stay) const {
    const int y = __builtin_amdgcn_frexp_exp(post_join_max<NW>(wave_top));
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const double st = w_stay * Wv[j];
      stay(j, st);
      B[j] = ldexp((G4[q0 + (j & (Q - 1))] + st) + G16[t0 + (j & (T - 1))], -y);
    }
  }
};

template <int K>
__global__ __launch_bounds__(KmerHmm<K>::T) void posterior_forward_kernel(PostArgs a) {
  constexpr int S = KmerHmm<K>::S, T = KmerHmm<K>::T, Q = KmerHmm<K>::Q, W = KmerHmm<K>::W, NW = KmerHmm<K>::NW;
  __shared__ __attribute__((aligned(16))) double row[2][KmerHmm<K>::ROW];
  __shared__ double wave_top[2][NW];  // per wave the largest value of the row it wrote
  __shared__ double wave_z[NW];
  BackSweep<K> bs;
  const int status = bs.begin(a);
  const int u = bs.u, wave = bs.wave, E = bs.E;
  const int64_t rd = bs.rd;
  if (status != 0) {
    if (u == 0) {
      a.out_status[rd] = status;
      a.out_z[2 * rd] = 0.0;
      a.out_z[2 * rd + 1] = 0.0;
    }
    return;
  }
  const double *lev = bs.lev;
  const double w_stay = bs.w_stay, w_step = bs.w_step, w_skip = bs.w_skip;
  double *store = bs.store;

  double A[16], mean[16], ac[16], mc[16];
  double e = lev[0];
  double top = 0.0;
  hmm_load_table(a, u, mean, ac, mc, [&](int j) {
    A[j] = post_emission(e, mean[j], ac[j], mc[j]);
    row[0][hmm_at(16 * u) + j] = A[j];
    store[post_store_at<T>(j)] = A[j];
    top = fmax(top, A[j]);
  });
  top = post_wave_max<W>(top);
  if ((u & (W - 1)) == 0) wave_top[0][wave] = top;
  __syncthreads();
  long long X = 0;
  for (int i = 1; i < E; i++) {
    const double *P = row[(i - 1) & 1];
    double *N = row[i & 1];
    e = lev[i];
    const int x = __builtin_amdgcn_frexp_exp(post_join_max<NW>(wave_top[(i - 1) & 1]));
    // skip: the 16 predecessors c T + u, shared by all the thread's states
    double sum16 = P[hmm_at(u)];
#pragma unroll
    for (int c = 1; c < 16; c++) sum16 = sum16 + P[hmm_at(c * T + u)];
    const double sk = w_skip * sum16;
    // step: per group g of four states the 4 predecessors a Q + 4 u + g
    double st[4];
#pragma unroll
    for (int g = 0; g < 4; g++) st[g] = P[hmm_at(4 * u) + g];
#pragma unroll
    for (int c = 1; c < 4; c++) {
#pragma unroll
      for (int g = 0; g < 4; g++) st[g] = st[g] + P[hmm_at(c * Q + 4 * u) + g];
    }
#pragma unroll
    for (int g = 0; g < 4; g++) st[g] = w_step * st[g];
    double *out = store + (int64_t)i * S;
    top = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const double t = (st[j >> 2] + w_stay * A[j]) + sk;
      A[j] = ldexp(t, -x) * post_emission(e, mean[j], ac[j], mc[j]);
      N[hmm_at(16 * u) + j] = A[j];
      out[post_store_at<T>(j)] = A[j];
      top = fmax(top, A[j]);
    }
    top = post_wave_max<W>(top);
    if ((u & (W - 1)) == 0) wave_top[i & 1][wave] = top;
    X += x;
    __syncthreads();
  }
  // Z: the thread's 16 values ascending, the butterfly over the wave, the waves joined
  double z = A[0];
#pragma unroll
  for (int j = 1; j < 16; j++) z = z + A[j];
  z = post_wave_sum<W>(z);
  if ((u & (W - 1)) == 0) wave_z[wave] = z;
  __syncthreads();
  if (u == 0) {
    a.out_status[rd] = NVK_DEC_OK;
    a.out_z[2 * rd] = post_join_sum<NW>(wave_z, 1);
    a.out_z[2 * rd + 1] = (double)X;
  }
}

// THE BACKWARD SWEEP (nvk_kmer_posterior_dev) forms the letter marginals.  It asks for its own 16 values of A(i, .)
// from the row store first, evaluates the emissions while they arrive, then forms the four class sums of A * B; the
// waves' class sums go to LDS before the event's barrier, and thread 0 joins them after it and writes the event's four
// marginals.
// (two waves per SIMD asked for: with the row in flight across the emissions the compiler otherwise takes 266 registers
// and one)
template <int K>
__global__ __launch_bounds__(KmerHmm<K>::T) __attribute__((amdgpu_waves_per_eu(2))) void
posterior_backward_kernel(PostArgs a) {
  using BS = BackSweep<K>;
  constexpr int W = BS::W, NW = BS::NW;
  __shared__ __attribute__((aligned(16))) double G4[2][BS::G4_ROW];    // w_step * G4
  __shared__ __attribute__((aligned(16))) double G16[2][BS::G16_ROW];  // w_skip * G16
  __shared__ double wave_top[2][NW];     // per wave the largest B of the event
  __shared__ double wave_cls[2][4][NW];  // per wave the four class sums of the event
  BS bs;
  if (bs.begin(a) != 0) return;
  const int u = bs.u;
  double *marg = a.out_marg + 4 * bs.ev0;
  // the letter at `pos`: the thread's 16 states differ in the last two letters only
  const int mode = a.pos == K - 1 ? 0 : a.pos == K - 2 ? 1 : 2;
  const int own = (a.pos < K - 2) ? ((16 * u) >> (2 * (K - 1 - a.pos))) & 3 : 0;  // mode 2: the letter of all 16

  double B[16], mean[16], ac[16], mc[16];
  hmm_load_table(a, u, mean, ac, mc, [&](int j) { B[j] = 1.0; });
  for (int i = bs.E - 1; i >= 0; i--) {
    const int p = i & 1;
    // (the event's row is asked for first and used last: the emissions below run while it arrives)
    double av[16], Wv[16];
    bs.load_row(i, av);
    if (i > 0) bs.template publish<false>(B, bs.lev[i], mean, ac, mc, Wv, G4[p], G16[p], wave_top[p]);
    double ab[16];
#pragma unroll
    for (int j = 0; j < 16; j++) ab[j] = av[j] * B[j];
    // the class sums of the thread's states, ascending inside a class
    double cls[4];
    if (mode == 0) {
#pragma unroll
      for (int x = 0; x < 4; x++) cls[x] = ((ab[x] + ab[4 + x]) + ab[8 + x]) + ab[12 + x];
    } else if (mode == 1) {
#pragma unroll
      for (int x = 0; x < 4; x++) cls[x] = ((ab[4 * x] + ab[4 * x + 1]) + ab[4 * x + 2]) + ab[4 * x + 3];
    } else {
      double all = ab[0];
#pragma unroll
      for (int j = 1; j < 16; j++) all = all + ab[j];
#pragma unroll
      for (int x = 0; x < 4; x++) cls[x] = (x == own) ? all : 0.0;
    }
    post_wave_sum_n<W>(cls);
    if ((u & (W - 1)) == 0) {
#pragma unroll
      for (int x = 0; x < 4; x++) wave_cls[p][x][bs.wave] = cls[x];
    }
    __syncthreads();
    if (u == 0) {
      double C[4];
#pragma unroll
      for (int x = 0; x < 4; x++) C[x] = post_join_sum<NW>(&wave_cls[p][x][0], 1);
      const double total = ((C[0] + C[1]) + C[2]) + C[3];
#pragma unroll
      for (int x = 0; x < 4; x++) marg[4 * (int64_t)i + x] = C[x] / total;
    }
    if (i > 0) bs.advance(B, Wv, G4[p], G16[p], wave_top[p], [](int, double) {});
  }
}

// THE COUNTS SWEEP (nvk_kmer_expectations_dev) forms the E-step's sums.  Per event it reduces seven sums over all
// states -- D and the three moment sums of A * B, and for the move i -> i + 1 the three numerators -- and the largest
// em of the event.  The move's terms of event i + 1 are still there when row i arrives: w_stay * W in SW, where the
// advance of iteration i + 1 left it, w_step * G4 and w_skip * G16 in the LDS buffers of the other parity, which the
// barrier of iteration i + 1 published and nobody writes before the barrier of iteration i.  The sums are formed
// before the emissions, which take the row's registers.  Thread 0 keeps the read's ten accumulators and takes every
// event's shares after its barrier, so the events enter descending; out_marg of PostArgs is out_stats here.
constexpr int CNT_SUMS = 7;  // D, m0, m1, m2, n_stay, n_step, n_skip

template <int K>
__global__ __launch_bounds__(KmerHmm<K>::T) __attribute__((amdgpu_waves_per_eu(2))) void
posterior_counts_kernel(PostArgs a) {
  using BS = BackSweep<K>;
  constexpr int S = BS::S, T = BS::T, Q = BS::Q, W = BS::W, NW = BS::NW;
  __shared__ __attribute__((aligned(16))) double G4[2][BS::G4_ROW];    // w_step * G4
  __shared__ __attribute__((aligned(16))) double G16[2][BS::G16_ROW];  // w_skip * G16
  __shared__ __attribute__((aligned(16))) double SW[S];  // w_stay * W, every thread's own 16 in the row store's layout
  __shared__ double wave_top[2][NW];            // per wave the largest B of the event
  __shared__ double wave_em[2][NW];             // per wave the largest em of the event
  __shared__ double wave_acc[2][CNT_SUMS][NW];  // per wave the seven sums of the event
  __shared__ double read_acc[10];               // the read's accumulators
  BS bs;
  if (bs.begin(a) != 0) return;
  const int u = bs.u, E = bs.E, q0 = bs.q0, t0 = bs.t0;

  double *sw = SW + 2 * u;
  double B[16], mean[16], ac[16], mc[16];
  hmm_load_table(a, u, mean, ac, mc, [&](int j) { B[j] = 1.0; });
  // (thread 0's alone, in LDS so that they cost no thread a register: M0, Mx, Mxx, Mm, Mxm, Mmm, N_stay, N_step,
  // N_skip, F)
  if (u == 0) {
#pragma unroll
    for (int x = 0; x < 10; x++) read_acc[x] = 0.0;
  }
  for (int i = E - 1; i >= 0; i--) {
    const int p = i & 1;
    double av[16];
    bs.load_row(i, av);
    double acc[CNT_SUMS];
    // the move i -> i + 1: W, w_step * G4 and w_skip * G16 of event i + 1
    if (i < E - 1) {
      const double *g4 = G4[p ^ 1], *g16 = G16[p ^ 1];
      acc[4] = av[0] * sw[post_store_at<T>(0)];
      acc[5] = av[0] * g4[q0];
      acc[6] = av[0] * g16[t0];
#pragma unroll
      for (int j = 1; j < 16; j++) {
        acc[4] = acc[4] + av[j] * sw[post_store_at<T>(j)];
        acc[5] = acc[5] + av[j] * g4[q0 + (j & (Q - 1))];
        acc[6] = acc[6] + av[j] * g16[t0 + (j & (T - 1))];
      }
    } else {
      acc[4] = acc[5] = acc[6] = 0.0;
    }
    // D and the moment sums of A * B, the thread's states ascending
    {
      const double ab = av[0] * B[0];
      const double t0 = ab * mc[0];
      const double t1 = t0 * mean[0];
      acc[0] = ab;
      acc[1] = t0;
      acc[2] = t1;
      acc[3] = t1 * mean[0];
    }
#pragma unroll
    for (int j = 1; j < 16; j++) {
      const double ab = av[j] * B[j];
      const double t0 = ab * mc[j];
      const double t1 = t0 * mean[j];
      acc[0] = acc[0] + ab;
      acc[1] = acc[1] + t0;
      acc[2] = acc[2] + t1;
      acc[3] = acc[3] + t1 * mean[j];
    }
    post_wave_sum_n<W>(acc);
    if ((u & (W - 1)) == 0) {
#pragma unroll
      for (int x = 0; x < CNT_SUMS; x++) wave_acc[p][x][bs.wave] = acc[x];
    }
    // (the row is done with: the emissions of the next backward step take its registers)
    const double e = bs.lev[i];
    double emx, Wv[16];
    if (i > 0) {
      emx = bs.template publish<true>(B, e, mean, ac, mc, Wv, G4[p], G16[p], wave_top[p]);
    } else {
      emx = gauss_log(e, mean[0], ac[0], mc[0]);
#pragma unroll
      for (int j = 1; j < 16; j++) emx = fmax(emx, gauss_log(e, mean[j], ac[j], mc[j]));
    }
    emx = post_wave_max<W>(emx);
    if ((u & (W - 1)) == 0) wave_em[p][bs.wave] = emx;
    __syncthreads();
    if (u == 0) {
      double C[CNT_SUMS];
#pragma unroll
      for (int x = 0; x < CNT_SUMS; x++) C[x] = post_join_sum<NW>(&wave_acc[p][x][0], 1);
      const double g0 = C[1] / C[0], g1 = C[2] / C[0], g2 = C[3] / C[0];
      read_acc[0] = read_acc[0] + g0;
      read_acc[1] = read_acc[1] + g0 * e;
      read_acc[2] = read_acc[2] + (g0 * e) * e;
      read_acc[3] = read_acc[3] + g1;
      read_acc[4] = read_acc[4] + g1 * e;
      read_acc[5] = read_acc[5] + g2;
      if (post_join_max<NW>(wave_em[p]) <= POST_EM_FLOOR) read_acc[9] = read_acc[9] + 1.0;
      if (i < E - 1) {
        const double total = (C[4] + C[5]) + C[6];
        read_acc[6] = read_acc[6] + C[4] / total;
        read_acc[7] = read_acc[7] + C[5] / total;
        read_acc[8] = read_acc[8] + C[6] / total;
      }
    }
    if (i > 0)
      bs.advance(B, Wv, G4[p], G16[p], wave_top[p], [&](int j, double stay) { sw[post_store_at<T>(j)] = stay; });
  }
  if (u == 0) {
    double *out = a.out_marg + 10 * bs.rd;
#pragma unroll
    for (int x = 0; x < 10; x++) out[x] = read_acc[x];
  }
}

// THE MOMENTS SWEEP (nvk_kmer_state_moments_dev) forms the per-state accumulation.  D needs the whole workgroup: the
// thread's 16 products A * B are formed before the barrier, their sum goes through the wave butterfly to LDS as the
// counts sweep's acc[0] does (so D has that sweep's bits), and after the barrier every thread joins the waves' values,
// forms 1 / D and updates the 48 accumulators of its 16 states.
//
// The accumulators, 3 S doubles (96 KB at k = 6), lie in LDS, every thread's own 16 of each moment in the row store's
// layout (pairs side by side, one 16-byte access per lane covering 1 KB per wave: no bank conflicts); nobody else
// touches them, so they need no barrier.  With G4 / G16 that is 119 KB at k = 6: one workgroup per CU, one wave per
// SIMD, and a lane may take up to 512 registers.  Nothing else runs on the CU to hide the row's latency behind, so the
// row of event i - 1 is asked for at the top of iteration i and used one iteration later.  `out_marg` of PostArgs is
// the part's slab buffer here: the workgroup of read r0 + b writes its 3 S sums to slab b, laid out [m][s].
template <int K>
__global__ __launch_bounds__(KmerHmm<K>::T) void posterior_moments_kernel(PostArgs a) {
  using BS = BackSweep<K>;
  constexpr int S = BS::S, T = BS::T, W = BS::W, NW = BS::NW;
  __shared__ __attribute__((aligned(16))) double G4[2][BS::G4_ROW];    // w_step * G4
  __shared__ __attribute__((aligned(16))) double G16[2][BS::G16_ROW];  // w_skip * G16
  __shared__ __attribute__((aligned(16))) double ACC[3][S];  // G0, G1, G2 in the row store's layout
  __shared__ double wave_top[2][NW];  // per wave the largest B of the event
  __shared__ double wave_d[2][NW];    // per wave the sum of A * B of the event
  BS bs;
  if (bs.begin(a) != 0) return;
  const int u = bs.u;
  double *acc = &ACC[0][0] + 2 * u;

  double B[16], mean[16], ac[16], mc[16], nx[16];
  hmm_load_table(a, u, mean, ac, mc, [&](int j) {
    B[j] = 1.0;
    nx[j] = bs.store[(int64_t)(bs.E - 1) * S + post_store_at<T>(j)];
  });
#pragma unroll
  for (int m = 0; m < 3; m++) {
#pragma unroll
    for (int j = 0; j < 16; j++) acc[m * S + post_store_at<T>(j)] = 0.0;
  }
  for (int i = bs.E - 1; i >= 0; i--) {
    const int p = i & 1;
    double av[16];
#pragma unroll
    for (int j = 0; j < 16; j++) av[j] = nx[j];
    if (i > 0) bs.load_row(i - 1, nx);
    const double e = bs.lev[i];
    double Wv[16];
    if (i > 0) bs.template publish<false>(B, e, mean, ac, mc, Wv, G4[p], G16[p], wave_top[p]);
    // the thread's 16 products, their sum ascending, the butterfly over the wave
    double ab[16];
#pragma unroll
    for (int j = 0; j < 16; j++) ab[j] = av[j] * B[j];
    double d = ab[0];
#pragma unroll
    for (int j = 1; j < 16; j++) d = d + ab[j];
    d = post_wave_sum<W>(d);
    if ((u & (W - 1)) == 0) wave_d[p][bs.wave] = d;
    __syncthreads();
    const double inv = 1.0 / post_join_sum<NW>(wave_d[p], 1);
#pragma unroll
    for (int j = 0; j < 16; j++) {
      double *at = acc + post_store_at<T>(j);
      const double g = ab[j] * inv;
      const double gx = g * e;
      at[0] = at[0] + g;
      at[S] = at[S] + gx;
      at[2 * S] = at[2 * S] + gx * e;
    }
    if (i > 0) bs.advance(B, Wv, G4[p], G16[p], wave_top[p], [](int, double) {});
  }
  double *slab = a.out_marg + (int64_t)blockIdx.x * (3 * S) + 16 * u;
#pragma unroll
  for (int m = 0; m < 3; m++) {
#pragma unroll
    for (int j = 0; j < 16; j++) slab[m * S + j] = acc[m * S + post_store_at<T>(j)];
  }
}

// The batch's totals, one thread per entry of [m][s]: the part's reads ascending, those the sweeps did not process
// left out, continuing the total the previous part left (zeroed on the stream at the start of the call).  One chain of
// additions per entry over the whole batch, so the cut into parts changes nothing.
__global__ __launch_bounds__(256) void state_moments_reduce_kernel(const double *slab, const int32_t *status, int r0,
                                                                   int n, int n3, double *tot) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= n3) return;
  double t = tot[x];
  for (int r = 0; r < n; r++)
    if (status[r0 + r] == NVK_DEC_OK) t = t + slab[(int64_t)r * n3 + x];
  tot[x] = t;
}

enum { SWEEP_FORWARD, SWEEP_BACKWARD, SWEEP_COUNTS, SWEEP_MOMENTS };

void launch_sweep(int sweep, int k, const PostArgs &a, int n, hipStream_t stream) {
  hmm_dispatch_k(k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    if (sweep == SWEEP_FORWARD)
      hipLaunchKernelGGL(posterior_forward_kernel<K>, dim3((unsigned)n), dim3(KmerHmm<K>::T), 0, stream, a);
    else if (sweep == SWEEP_BACKWARD)
      hipLaunchKernelGGL(posterior_backward_kernel<K>, dim3((unsigned)n), dim3(KmerHmm<K>::T), 0, stream, a);
    else if (sweep == SWEEP_COUNTS)
      hipLaunchKernelGGL(posterior_counts_kernel<K>, dim3((unsigned)n), dim3(KmerHmm<K>::T), 0, stream, a);
    else
      hipLaunchKernelGGL(posterior_moments_kernel<K>, dim3((unsigned)n), dim3(KmerHmm<K>::T), 0, stream, a);
  });
}

// what follows the forward sweep of a part
struct SecondSweep {
  int kernel;
  int n_ms;    // the launches of a part that are timed, the forward sweep included
  bool slabs;  // the sweep writes slabs to a workspace of its own and a reduce launch follows it
};

// the three entries: the forward sweep of a part, then `second` (the backward, the counts or the moments sweep) on its
// rows.  `out`: the marginals, the stats or the moments' totals.  The moments sweep leaves one slab of 3 S doubles per
// read of the part in a workspace of its own, which counts in the cut (a read takes its events and three more rows),
// and a third launch chains the slabs into `out`
int run_sweeps(const char *what, int second, nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
               const int64_t *ev_off, int k, int pos, const double *mean, const double *ac, const double *mc,
               double w_stay, double w_step, double w_skip, const int32_t *status_in, double *out, double *out_z,
               int32_t *out_status, int64_t *out_parts, double *out_ms) {
  if (out_parts) *out_parts = 0;
  const SecondSweep sw = second == SWEEP_MOMENTS ? SecondSweep{second, 3, true} : SecondSweep{second, 2, false};
  if (out_ms)
    for (int t = 0; t < sw.n_ms; t++) out_ms[t] = 0.0;
  int rc = hmm_check_entry(what, ctx, k, "pos", pos, n_reads, total_events, level, ev_off, mean, ac, mc);
  if (rc) return rc;
  const double weights[3] = {w_stay, w_step, w_skip};
  for (double w : weights)
    if (!(w > 0.0 && w <= 1.0)) {
      nvk_set_error("%s: w_stay %g, w_step %g or w_skip %g is not a finite value in (0, 1]", what, w_stay, w_step,
                    w_skip);
      return NVK_ERR_INVALID;
    }
  if (!((w_stay > w_step ? w_stay : w_step) >= POST_MIN_MOVE)) {
    nvk_set_error("%s: w_stay %g and w_step %g are both below 2^-10", what, w_stay, w_step);
    return NVK_ERR_INVALID;
  }
  NVK_HIP(hipSetDevice(ctx->device));
  std::vector<int64_t> eoff;
  if ((rc = nvk_fetch_offsets(ctx, "event", ev_off, n_reads, eoff, "total_events", total_events))) return rc;
  for (int64_t r = 0; r < n_reads; r++)
    if (eoff[r + 1] - eoff[r] > HMM_MAX_EVENTS) {
      nvk_set_error("%s: read %lld has %lld events, above %d", what, (long long)r, (long long)(eoff[r + 1] - eoff[r]),
                    HMM_MAX_EVENTS);
      return NVK_ERR_INVALID;
    }
  if (n_reads == 0) return NVK_OK;
  if (((total_events > 0 || sw.slabs) && !out) || !out_z || !out_status) {
    nvk_set_error("%s: NULL output", what);
    return NVK_ERR_INVALID;
  }
  // parts of reads whose rows fit the cap (a read larger than the cap on its own makes a part of one; a read the
  // kernels skip takes its rows all the same: its status is on the device).  A context without a limit stops at
  // 16 GiB: at k = 6 a read of 816 events takes 26.7 MB, so 4 GiB would hold 160 reads, fewer workgroups than the
  // device has CUs, and 16 GiB holds 640, two for every CU and more
  int64_t cap_b = nvk_spill_cap(ctx, WS_SEED_TB);
  if (ctx->ws_limit <= 0 && cap_b > ((int64_t)16 << 30)) cap_b = (int64_t)16 << 30;
  const int64_t S = (int64_t)1 << (2 * k);
  std::vector<int64_t> cut;
  int64_t need_rows = 1, need_slabs = 0;
  if (sw.slabs) {
    // a read's slab is three rows' worth: cut on events + 3 per read, then size the two workspaces from the cut
    std::vector<int64_t> uoff(eoff);
    for (int64_t r = 0; r <= n_reads; r++) uoff[(size_t)r] += 3 * r;
    cut_parts(uoff, cap_b / (8 * S), cut);
    for (size_t c = 0; c + 1 < cut.size(); c++) {
      need_rows = std::max(need_rows, eoff[(size_t)cut[c + 1]] - eoff[(size_t)cut[c]]);
      need_slabs = std::max(need_slabs, cut[c + 1] - cut[c]);
    }
    if ((rc = nvk_ws_reserve(ctx, WS_STATE_MOM, (size_t)need_slabs * 3 * (size_t)S * 8))) return rc;
    NVK_HIP(hipMemsetAsync(out, 0, 3 * (size_t)S * 8, ctx->stream));
  } else {
    need_rows = cut_parts(eoff, cap_b / (8 * S), cut);
  }
  // (the seed aligner's traceback workspace serves, as for the Viterbi store: they never run at once on a context)
  if ((rc = nvk_ws_reserve(ctx, WS_SEED_TB, (size_t)need_rows * (size_t)S * 8))) return rc;
  PostArgs a;
  (HmmIn &)a = HmmIn{level, ev_off, mean, ac, mc, status_in};
  a.w_stay = w_stay;
  a.w_step = w_step;
  a.w_skip = w_skip;
  a.out_marg = sw.slabs ? (double *)ctx->ws[WS_STATE_MOM] : out;
  a.out_z = out_z;
  a.out_status = out_status;
  a.rows = (double *)ctx->ws[WS_SEED_TB];
  a.pos = pos;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  if (out_ms)
    for (hipEvent_t &e : ev) NVK_HIP(hipEventCreate(&e));
  for (size_t c = 0; c + 1 < cut.size(); c++) {
    a.r0 = (int)cut[c];
    const int n = (int)(cut[c + 1] - cut[c]);
    if (out_ms) NVK_HIP(hipEventRecord(ev[0], ctx->stream));
    launch_sweep(SWEEP_FORWARD, k, a, n, ctx->stream);
    NVK_HIP(hipGetLastError());
    if (out_ms) NVK_HIP(hipEventRecord(ev[1], ctx->stream));
    launch_sweep(sw.kernel, k, a, n, ctx->stream);
    NVK_HIP(hipGetLastError());
    if (out_ms) NVK_HIP(hipEventRecord(ev[2], ctx->stream));
    if (sw.slabs) {
      const int n3 = 3 * (int)S;
      hipLaunchKernelGGL(state_moments_reduce_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, ctx->stream,
                         (const double *)a.out_marg, (const int32_t *)out_status, a.r0, n, n3, out);
      NVK_HIP(hipGetLastError());
    }
    if (out_ms) {
      if (sw.slabs) NVK_HIP(hipEventRecord(ev[3], ctx->stream));
      NVK_HIP(hipEventSynchronize(ev[sw.n_ms]));
      for (int t = 0; t < sw.n_ms; t++) {
        float ms = 0.f;
        NVK_HIP(hipEventElapsedTime(&ms, ev[t], ev[t + 1]));
        out_ms[t] += (double)ms;
      }
    }
  }
  NVK_HIP(hipStreamSynchronize(ctx->stream));
  if (out_ms)
    for (hipEvent_t e : ev) NVK_HIP(hipEventDestroy(e));
  if (out_parts) *out_parts = (int64_t)cut.size() - 1;
  return NVK_OK;
}

}  // namespace

extern "C" int nvk_kmer_posterior_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                                      const int64_t *ev_off, int k, int pos, const double *mean, const double *ac,
                                      const double *mc, double w_stay, double w_step, double w_skip,
                                      const int32_t *status_in, double *out_marg, double *out_z, int32_t *out_status,
                                      int64_t *out_parts, double *out_ms) {
  return run_sweeps("nvk_kmer_posterior_dev", SWEEP_BACKWARD, ctx, n_reads, total_events, level, ev_off, k, pos, mean,
                    ac, mc, w_stay, w_step, w_skip, status_in, out_marg, out_z, out_status, out_parts, out_ms);
}

extern "C" int nvk_kmer_expectations_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                                         const int64_t *ev_off, int k, const double *mean, const double *ac,
                                         const double *mc, double w_stay, double w_step, double w_skip,
                                         const int32_t *status_in, double *out_stats, double *out_z,
                                         int32_t *out_status, int64_t *out_parts, double *out_ms) {
  return run_sweeps("nvk_kmer_expectations_dev", SWEEP_COUNTS, ctx, n_reads, total_events, level, ev_off, k, 0, mean,
                    ac, mc, w_stay, w_step, w_skip, status_in, out_stats, out_z, out_status, out_parts, out_ms);
}

extern "C" int nvk_kmer_state_moments_dev(nvk_ctx *ctx, int64_t n_reads, int64_t total_events, const double *level,
                                          const int64_t *ev_off, int k, const double *mean, const double *ac,
                                          const double *mc, double w_stay, double w_step, double w_skip,
                                          const int32_t *status_in, double *out_moments, double *out_z,
                                          int32_t *out_status, int64_t *out_parts, double *out_ms) {
  return run_sweeps("nvk_kmer_state_moments_dev", SWEEP_MOMENTS, ctx, n_reads, total_events, level, ev_off, k, 0, mean,
                    ac, mc, w_stay, w_step, w_skip, status_in, out_moments, out_z, out_status, out_parts, out_ms);
}
