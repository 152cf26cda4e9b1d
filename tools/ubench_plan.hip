// Times the align planner alone (plan_kernel + plan_totals_kernel, csrc/kernels_plan.hip) on a batch shaped like
// bench.py's cfg2_align: 10 000 reads of 360-440 bases, 3-17 samples per base, anchors on three bases in four,
// bandwidth 150, min event length 2, transition rows, a random 6-mer table.  HIP events, 10 launches after 3.
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
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
template <class T> static T *up(const std::vector<T> &v) { T *d = nullptr; if (hipMalloc(&d, v.size() * sizeof(T) + 64) != hipSuccess) return nullptr; hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice); return d; }
int main(int argc, char **argv) {
  const int n = 10000, bw = 150, mel = 2, k = 6;
  const int write_rows = argc > 2 ? atoi(argv[2]) : 0;  // ubench_plan LABEL 1: with the row table of the exact kernel
  std::mt19937_64 rng(1);
  std::vector<int64_t> so{0}, ro{0}, ao{0}, bo{0}, co{0};
  std::vector<int32_t> ref, anc, cb, ca;
  for (int i = 0; i < n; i++) {
    int R = 360 + (int)(rng() % 81);
    std::vector<int> st(R + 1); st[0] = bw;
    for (int j = 0; j < R; j++) st[j + 1] = st[j] + 3 + (int)(rng() % 15);
    int N = st[R] + bw;
    for (int j = 0; j < R; j++) ref.push_back((int)(rng() % 4));
    int na = 0, prev = 0;
    for (int j = 0; j < R; j++) if (rng() % 4 != 0 || j == 0 || j == R - 1) { int s = st[j] + (int)(rng() % 41) - 20; if (s < prev) s = prev; if (s > N - 1) s = N - 1; prev = s; anc.push_back(s); anc.push_back(j); na++; }
    for (int j = 0; j < 2; j++) cb.push_back((int)(rng() % 4));
    for (int j = 0; j < 3; j++) ca.push_back((int)(rng() % 4));
    so.push_back(so.back() + N); ro.push_back(ro.back() + R); ao.push_back(ao.back() + na); bo.push_back(bo.back() + 2); co.push_back(co.back() + 3);
  }
  const int64_t tr = ro.back(), rows_total = 2 * tr;
  std::vector<double> mean(4096), ac(4096), mc(4096);
  for (int i = 0; i < 4096; i++) { mean[i] = (double)(rng() % 100000) / 20000.0 - 2.5; ac[i] = -1.0 - (i % 7) * 0.1; mc[i] = 2.0 + (i % 5) * 0.3; }
  DeviceModel dm; dm.k = k; dm.central = 2; dm.alphabet = 4; dm.n = 4096; dm.mean = up(mean); dm.ac = up(ac); dm.mc = up(mc);
  BatchArgs a{n, so.back(), tr, ao.back(), nullptr, up(so), up(ref), up(ro), up(cb), up(bo), up(ca), up(co), up(anc), up(ao), bw, mel};
  ReadMeta *metas; RowParam *rows; unsigned long long *bandtmp; PlanTotals *tot; Lane3 *lf, *lr; int32_t *offs;
  CK(hipMalloc(&metas, (n + 1) * sizeof(ReadMeta) + 64)); CK(hipMalloc(&rows, (rows_total + 1) * sizeof(RowParam)));
  CK(hipMalloc(&bandtmp, (2 * (tr + n) + 2) * 8)); CK(hipMalloc(&tot, 256)); CK(hipMalloc(&lf, (rows_total + 1) * 48));
  CK(hipMalloc(&lr, (rows_total + 1) * 48)); CK(hipMalloc(&offs, (rows_total + 1) * 4));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  float best = 1e9f, sum = 0;
  for (int it = 0; it < 13; it++) {
    CK(hipMemset(tot, 0, sizeof(PlanTotals)));
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(plan_kernel, dim3(n), dim3(PLAN_T), 0, 0, dm, a, (int)PLAN_ALIGN_TRANS, log(0.01), ALIGN1_C_CAP, metas, rows, bandtmp, lf, lr, offs, write_rows);
    hipLaunchKernelGGL(plan_totals_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, metas, n, ALIGN1_C_CAP, tot);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (it >= 3) { sum += ms; best = ms < best ? ms : best; }
  }
  PlanTotals h; CK(hipMemcpy(&h, tot, sizeof h, hipMemcpyDeviceToHost));
  printf("%-28s avg %.1f us  best %.1f us   (steps %llu cells %llu max_c %d n_wide %d)\n", argc > 1 ? argv[1] : "plan", sum / 10 * 1e3, best * 1e3, h.steps, h.cells, h.max_c, h.n_wide);
  return 0;
}
