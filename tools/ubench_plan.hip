// The align planner alone (plan_kernel + plan_totals_kernel, csrc/kernels_plan.hip) on a synthetic batch.
//   ubench_plan time   LABEL [RLO RHI BW MEL TRANS WRITE_ROWS N DLO DHI]   HIP events, 10 launches after 3
//   ubench_plan digest LABEL [RLO RHI BW MEL TRANS WRITE_ROWS N DLO DHI]   one launch into zero-filled buffers, then
//       a 64-bit FNV-1a of each thing the planner writes (metas, lane_f, lane_r, lane_offs, the totals and, with
//       WRITE_ROWS 1, rows; none of the structs has padding).  Built against two versions of the kernel source, it
//       shows whether they write the same bytes.
// Reads of RLO..RHI bases, DLO..DHI samples per base, anchors on three bases in four (+-20 samples), a random 6-mer
// table; TRANS 1: transition rows.  The defaults are the shape of bench.py's cfg2_align: 360 440 150 2 1 0 10000 3 17.
// The kernels live in an anonymous namespace, so this file includes their source; the launchers in it need the
// library's other objects to link:
//   make -C nadavca_amd/csrc
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -w -Inadavca_amd/csrc -c tools/ubench_plan.hip -o tools/ubench_plan.o
//   hipcc --offload-arch=gfx950 tools/ubench_plan.o $(ls nadavca_amd/csrc/*.o | grep -v kernels_plan.o) -o tools/ubench_plan
// DESIGN.md 5.3's table of the kernel with parts switched off came from temporary edits of kernels_plan.hip (loop
// bounds forced to zero, stores behind a condition that never holds) timed with this driver; the edits were not kept.
#include "../nadavca_amd/csrc/kernels_plan.hip"
#include <vector>
#include <random>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
template <class T> static T *up(const std::vector<T> &v) { T *d = nullptr; if (hipMalloc(&d, v.size() * sizeof(T) + 64) != hipSuccess) return nullptr; hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); return d; }
static_assert(sizeof(ReadMeta) == 72 && sizeof(RowParam) == 48 && sizeof(Lane3) == 48 && sizeof(PlanTotals) == 40, "no padding");
// FNV-1a, 64 bit, of `bytes` bytes on the device
static int digest(const char *what, const void *dev, size_t bytes) {
  std::vector<unsigned char> h(bytes);
  CK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
  unsigned long long d = 0xcbf29ce484222325ull;
  for (unsigned char c : h) d = (d ^ c) * 0x100000001b3ull;
  printf(" %s %016llx", what, d);
  return 0;
}
int main(int argc, char **argv) {
  const bool dig = argc > 1 && !strcmp(argv[1], "digest");
  if (argc < 2 || (!dig && strcmp(argv[1], "time"))) { printf("usage: ubench_plan time|digest LABEL [RLO RHI BW MEL TRANS WRITE_ROWS N DLO DHI]\n"); return 1; }
  const char *label = argc > 2 ? argv[2] : "plan";
  auto arg = [&](int i, int dflt) { return argc > i ? atoi(argv[i]) : dflt; };
  const int rlo = arg(3, 360), rhi = arg(4, 440), bw = arg(5, 150), mel = arg(6, 2), trans = arg(7, 1);
  const int write_rows = arg(8, 0), n = arg(9, 10000), dlo = arg(10, 3), dhi = arg(11, 17), k = 6;
  if (rlo < 1 || rhi < rlo || bw < 0 || mel < 0 || n < 1 || dlo < 1 || dhi < dlo) { printf("bad shape\n"); return 1; }
  std::mt19937_64 rng(1);
  std::vector<int64_t> so{0}, ro{0}, ao{0}, bo{0}, co{0};
  std::vector<int32_t> ref, anc, cb, ca;
  for (int i = 0; i < n; i++) {
    int R = rlo + (int)(rng() % (rhi - rlo + 1));
    std::vector<int> st(R + 1); st[0] = bw;
    for (int j = 0; j < R; j++) st[j + 1] = st[j] + dlo + (int)(rng() % (dhi - dlo + 1));
    int N = st[R] + bw;
    for (int j = 0; j < R; j++) ref.push_back((int)(rng() % 4));
    int na = 0, prev = 0;
    for (int j = 0; j < R; j++) if (rng() % 4 != 0 || j == 0 || j == R - 1) { int s = st[j] + (int)(rng() % 41) - 20; if (s < prev) s = prev; if (s > N - 1) s = N - 1; prev = s; anc.push_back(s); anc.push_back(j); na++; }
    for (int j = 0; j < 2; j++) cb.push_back((int)(rng() % 4));
    for (int j = 0; j < 3; j++) ca.push_back((int)(rng() % 4));
    so.push_back(so.back() + N); ro.push_back(ro.back() + R); ao.push_back(ao.back() + na); bo.push_back(bo.back() + 2); co.push_back(co.back() + 3);
  }
  const int64_t tr = ro.back(), rows_total = trans ? 2 * tr : tr + n;
  const int mode = trans ? (int)PLAN_ALIGN_TRANS : (int)PLAN_ALIGN_PLAIN;
  std::vector<double> mean(4096), ac(4096), mc(4096);
  for (int i = 0; i < 4096; i++) { mean[i] = (double)(rng() % 100000) / 20000.0 - 2.5; ac[i] = -1.0 - (i % 7) * 0.1; mc[i] = 2.0 + (i % 5) * 0.3; }
  DeviceModel dm; dm.k = k; dm.central = 2; dm.alphabet = 4; dm.n = 4096; dm.mean = up(mean); dm.ac = up(ac); dm.mc = up(mc);
  BatchArgs a{n, so.back(), tr, ao.back(), nullptr, up(so), up(ref), up(ro), up(cb), up(bo), up(ca), up(co), up(anc), up(ao), bw, mel};
  ReadMeta *metas; RowParam *rows; unsigned long long *bandtmp; PlanTotals *tot; Lane3 *lf, *lr; int32_t *offs;
  const size_t b_metas = (size_t)n * sizeof(ReadMeta), b_rows = (size_t)rows_total * sizeof(RowParam);
  const size_t b_lane = (size_t)rows_total * sizeof(Lane3), b_offs = (size_t)rows_total * 4;
  CK(hipMalloc(&metas, b_metas + 128)); CK(hipMalloc(&rows, b_rows + 64));
  CK(hipMalloc(&bandtmp, (2 * (tr + n) + 2) * 8)); CK(hipMalloc(&tot, 256)); CK(hipMalloc(&lf, b_lane + 64));
  CK(hipMalloc(&lr, b_lane + 64)); CK(hipMalloc(&offs, b_offs + 64));
  CK(hipMemset(metas, 0, b_metas)); CK(hipMemset(rows, 0, b_rows)); CK(hipMemset(lf, 0, b_lane));
  CK(hipMemset(lr, 0, b_lane)); CK(hipMemset(offs, 0, b_offs));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float best = 1e9f, sum = 0;
  for (int it = 0; it < (dig ? 1 : 13); it++) {
    CK(hipMemset(tot, 0, sizeof(PlanTotals)));
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(plan_kernel, dim3(n), dim3(PLAN_T), 0, 0, dm, a, mode, log(0.01), ALIGN1_C_CAP, metas, rows, bandtmp, lf, lr, offs, write_rows);
    hipLaunchKernelGGL(plan_totals_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, metas, n, ALIGN1_C_CAP, tot);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (it >= 3) { sum += ms; best = ms < best ? ms : best; }
  }
  PlanTotals h; CK(hipMemcpy(&h, tot, sizeof h, hipMemcpyDeviceToHost));
  if (dig) {
    printf("%-28s", label);
    if (digest("metas", metas, b_metas) || digest("lane_f", lf, b_lane) || digest("lane_r", lr, b_lane) ||
        digest("lane_offs", offs, b_offs) || digest("totals", tot, sizeof(PlanTotals)) ||
        (write_rows && digest("rows", rows, b_rows)))
      return 2;
    printf("   (max_T %d max_c %d max_cw %d n_wide %d)\n", h.max_T, h.max_c, h.max_cw, h.n_wide);
  } else {
    printf("%-28s avg %.1f us  best %.1f us   (steps %llu cells %llu max_c %d n_wide %d)\n", label, sum / 10 * 1e3, best * 1e3, h.steps, h.cells, h.max_c, h.n_wide);
  }
  return 0;
}
