/* The argument checks of gj_testing_step / gj_adjoint_testing from plain C: every documented error comes back before any
 * device work, so this runs without a GPU - and under the host sanitizers, with the library's host code built the same way:
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC -shared -Xarch_host -fsanitize=address,undefined \
 *       -o /tmp/libgradjune_hip_asan.so gradabm-june_amd/csrc/gradjune_hip.hip
 *   hipcc -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude examples/testing_args.c \
 *       -L/tmp -lgradjune_hip_asan -Wl,-rpath,/tmp -o /tmp/testing_args && ASAN_OPTIONS=detect_leaks=0 /tmp/testing_args
 */
#include <stdio.h>
#include <stdint.h>
#include "gradjune_hip.h"

#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { printf("FAIL %s: %d, expected %d\n", #call, rc_, (want)); bad = 1; } } while (0)
#define STREAM (1ull << 58)
/* the launch with one argument at a time replaced */
#define STEP(n, cls, tab, stage, time, now, stream, offset, dec, res, pos, iso, conf, q) \
  gj_testing_step(n, cls, tab, stage, time, 4.0f, 1, now, 1e30f, 10.0f, 1.0f, 7, stream, STREAM | (1ull << 57), offset, \
                  dec, res, pos, iso, conf, NULL, q, flags, counts, NULL)
#define ADJ(n, fl, stage, band, B, plan, contrib, partial, out) \
  gj_adjoint_testing(n, fl, stage, g, g, band, B, plan, contrib, partial, out, g, g, NULL)

int main(void) {
  int bad = 0;
  gj_testing_tables tab;
  for (int a = 0; a < 100; ++a) tab.probability[a] = 0.5f;
  for (int k = 0; k < GJ_TESTING_MAX_DELAYS; ++k) { tab.delay_cum[k] = 1.0f; tab.delay_days[k] = (float)k; }
  tab.n_delays = 3;
  tab._pad = 0;
  uint8_t cls[8] = {0}, flags[8] = {0};
  uint32_t dec[8] = {0};
  float stage[8] = {0}, t[8] = {0}, res[8] = {0}, pos[8] = {0}, iso[8] = {0}, conf[8] = {0}, q[8] = {0}, g[8] = {0};
  int32_t band[8] = {0};
  int64_t counts[2] = {0, 0}, order[8] = {0}, seg[2] = {0, 8}, first[2] = {0, 1};
  int32_t chunk_group[1] = {0};
  double contrib[8], partial[1], out[1];
  gj_seed_plan plan = {8, 1, order, seg, first, chunk_group};

  EXPECT(STEP(0, NULL, &tab, NULL, NULL, 1.0f, STREAM, 0, NULL, NULL, NULL, NULL, NULL, NULL), GJ_OK);
  EXPECT(STEP(-1, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, -4, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  EXPECT(STEP(8, cls, &tab, stage, t, -1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  EXPECT(STEP(8, cls, &tab, stage, t, 0.0f / 0.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM | 1, 0, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  EXPECT(STEP(8, cls, NULL, stage, t, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_NULL);
  tab.n_delays = 0;
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  tab.n_delays = GJ_TESTING_MAX_DELAYS + 1;
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_RANGE);
  tab.n_delays = 3;
  EXPECT(STEP(8, NULL, &tab, stage, t, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, NULL, t, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, stage, NULL, 1.0f, STREAM, 0, dec, res, pos, iso, conf, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, NULL, res, pos, iso, conf, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, NULL, pos, iso, conf, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, res, NULL, iso, conf, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, res, pos, iso, NULL, q), GJ_E_NULL);
  EXPECT(STEP(8, cls, &tab, stage, t, 1.0f, STREAM, 0, dec, res, pos, NULL, conf, q), GJ_E_NULL);      /* a mask without isolate_until */

  EXPECT(ADJ(-1, flags, stage, band, 1, &plan, contrib, partial, out), GJ_E_RANGE);
  EXPECT(ADJ(8, flags, stage, band, 0, &plan, contrib, partial, out), GJ_E_RANGE);
  EXPECT(ADJ(8, flags, stage, band, GJ_MAX_GROUPS + 1, &plan, contrib, partial, out), GJ_E_RANGE);
  EXPECT(ADJ(8, flags, stage, band, 1, &plan, contrib, partial, NULL), GJ_E_NULL);
  EXPECT(ADJ(8, flags, stage, band, 1, NULL, contrib, partial, out), GJ_E_NULL);
  EXPECT(ADJ(8, NULL, stage, band, 1, &plan, contrib, partial, out), GJ_E_NULL);
  EXPECT(ADJ(8, flags, NULL, band, 1, &plan, contrib, partial, out), GJ_E_NULL);
  EXPECT(ADJ(8, flags, stage, NULL, 1, &plan, contrib, partial, out), GJ_E_NULL);
  EXPECT(ADJ(8, flags, stage, band, 1, &plan, NULL, partial, out), GJ_E_NULL);
  EXPECT(ADJ(8, flags, stage, band, 1, &plan, contrib, NULL, out), GJ_E_NULL);
  plan.n_sorted = 9;                                         /* more sorted agents than agents */
  EXPECT(ADJ(8, flags, stage, band, 1, &plan, contrib, partial, out), GJ_E_RANGE);
  plan.n_sorted = 8; plan.n_chunks = 3;                      /* more chunks than the sizes allow */
  EXPECT(ADJ(8, flags, stage, band, 1, &plan, contrib, partial, out), GJ_E_RANGE);
  plan.n_chunks = 1; plan.order = NULL;
  EXPECT(ADJ(8, flags, stage, band, 1, &plan, contrib, partial, out), GJ_E_NULL);
  printf(bad ? "argument checks: FAILED\n" : "argument checks: ok\n");
  return bad;
}
