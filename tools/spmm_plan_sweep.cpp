// Walks spmm_plan (get_amd/csrc/spmm_plan.h, the arithmetic of launch_spmm) over every shape class on the CPU and prints, per
// kernel kind, the largest dynamic LDS request and where it occurs.  launch_spmm refuses more than 64 KB instead of opting in;
// this is the evidence that no shape gets there.  Plain host C++:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/spmm_plan_sweep.cpp -o spmm_plan_sweep
#include "../get_amd/csrc/spmm_plan.h"
#include <stdio.h>

int main() {
  using namespace gh;
  static const char* const names[SPMM_NKINDS] = {"matrix pipe (bf16)", "edge list fp32", "edge list bf16", "bit walk bf16",
                                                 "bit walk float4", "bit walk scalar"};
  struct Max { size_t lds; int n, r, h, compact; long long shapes; } mx[SPMM_NKINDS] = {};
  long long bad = 0;
  // n: below / at the few-graph threshold (256) and the 24 KB slab cap's threshold (512), and the bench step's 960
  const int ns[] = {1, 255, 256, 511, 512, 960, 4096};
  for (int r = 1; r <= 256; ++r)
    for (int h = 1; h <= 4096; h += (h < 64 ? 1 : 4)) {      // 1 .. 63, then the multiples of 4
      for (int bf16 = 0; bf16 < 2; ++bf16)
        for (int v4 = 0; v4 < 2; ++v4) {
          if (v4 && h % 4) continue;
          if (bf16 && !v4) continue;      // launch_spmm refuses it
          for (int compact = 0; compact < 2; ++compact)
            for (int n : ns) {
              const SpmmPlan p = spmm_plan(n, r, h, bf16 != 0, v4 != 0, compact != 0);
              const int hv = h / (v4 ? 4 : 1);
              // every plan covers the row and has a grid: slabs x slab columns >= the row's columns
              const long long cols = p.kind == SPMM_MFMA_BF16 ? h : hv;
              if (p.grid_x == 0 || p.grid_y == 0 || p.slab <= 0 || p.seq < 1 || (long long)p.nslab * p.slab < cols) {
                if (bad++ < 10) printf("BAD PLAN n=%d r=%d h=%d bf16=%d v4=%d compact=%d\n", n, r, h, bf16, v4, compact);
              }
              Max& m = mx[p.kind];
              m.shapes++;
              if (p.lds > m.lds) { m.lds = p.lds; m.n = n; m.r = r; m.h = h; m.compact = compact; }
            }
        }
    }
  int over = 0;
  for (int k = 0; k < SPMM_NKINDS; ++k) {
    printf("%-20s %10lld plans  max dynamic LDS %6zu B  at n=%d r=%d h=%d%s\n", names[k], mx[k].shapes, mx[k].lds, mx[k].n, mx[k].r,
           mx[k].h, mx[k].compact ? " node-compact" : "");
    if (mx[k].lds > 64 * 1024) over = 1;
  }
  printf("%s\n", over ? "ABOVE 64 KB: an opt-in is needed" : "every plan stays at or below 65536 B");
  return (over || bad) ? 1 : 0;
}
