/* The argument checks of gj_immunity_step / gj_adjoint_immunity from plain C: every documented error comes back before any
 * device work, so this runs without a GPU - and under the host sanitizers, with the library's host code built the same way:
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC -shared -Xarch_host -fsanitize=address,undefined \
 *       -o /tmp/libgradjune_hip_asan.so gradabm-june_amd/csrc/gradjune_hip.hip
 *   hipcc -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude examples/immunity_args.c \
 *       -L/tmp -lgradjune_hip_asan -Wl,-rpath,/tmp -o /tmp/immunity_args && ASAN_OPTIONS=detect_leaks=0 /tmp/immunity_args
 */
#include <stdio.h>
#include <stdint.h>
#include "gradjune_hip.h"

#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { printf("FAIL %s: %d, expected %d\n", #call, rc_, (want)); bad = 1; } } while (0)

int main(void) {
  int bad = 0;
  gj_immunity_tables tab;
  for (int a = 0; a < 100; ++a) { tab.cap[a] = 0.8f; tab.keep[a] = 0.5f; }
  uint8_t cls[8] = {0}, flags[8] = {0};
  float stage[8] = {0}, nw[8] = {0}, susc[8] = {0}, inf[8] = {0}, g[8] = {0};
  int32_t band[8] = {0};
  int64_t count = 0, order[8] = {0}, seg[2] = {0, 8}, first[2] = {0, 1};
  int32_t chunk_group[1] = {0};
  double contrib[16], partial[2], sum_a[1], sum_b[1];
  gj_seed_plan plan = {8, 1, order, seg, first, chunk_group};

  EXPECT(gj_immunity_step(0, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL), GJ_OK);
  EXPECT(gj_immunity_step(-1, cls, &tab, stage, 0, nw, susc, inf, flags, NULL, &count, &count, NULL), GJ_E_RANGE);
  EXPECT(gj_immunity_step(8, cls, &tab, stage, -1, nw, susc, inf, flags, NULL, &count, &count, NULL), GJ_E_RANGE);
  EXPECT(gj_immunity_step(8, cls, &tab, stage, GJ_MAX_STAGES, nw, susc, inf, flags, NULL, NULL, NULL, NULL), GJ_E_RANGE);
  EXPECT(gj_immunity_step(8, NULL, &tab, stage, 0, nw, susc, inf, NULL, NULL, NULL, NULL, NULL), GJ_E_NULL);
  EXPECT(gj_immunity_step(8, cls, NULL, stage, 0, nw, susc, inf, NULL, NULL, NULL, NULL, NULL), GJ_E_NULL);
  EXPECT(gj_immunity_step(8, cls, &tab, NULL, 0, nw, susc, inf, NULL, NULL, NULL, NULL, NULL), GJ_E_NULL);
  EXPECT(gj_immunity_step(8, cls, &tab, stage, 0, NULL, NULL, inf, NULL, NULL, NULL, NULL, NULL), GJ_E_NULL);
  EXPECT(gj_immunity_step(8, cls, &tab, stage, 0, NULL, susc, NULL, NULL, NULL, NULL, NULL, NULL), GJ_E_NULL);

  EXPECT(gj_adjoint_immunity(-1, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_RANGE);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 0, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_RANGE);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, GJ_MAX_GROUPS + 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_RANGE);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, NULL, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, NULL, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, NULL, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, NULL, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, NULL, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, NULL, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, NULL, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, NULL, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, NULL, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, NULL, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  plan.n_sorted = 9;                                         /* more sorted agents than agents */
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_RANGE);
  plan.n_sorted = 8; plan.n_chunks = 3;                      /* more chunks than the sizes allow */
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_RANGE);
  plan.n_chunks = 1; plan.order = NULL;
  EXPECT(gj_adjoint_immunity(8, flags, cls, &tab, susc, g, g, band, 1, &plan, contrib, partial, sum_a, sum_b, g, g, g, NULL), GJ_E_NULL);
  printf(bad ? "argument checks: FAILED\n" : "argument checks: ok\n");
  return bad;
}
