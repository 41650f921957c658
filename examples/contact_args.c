/* The argument checks of gj_contact_mark / gj_contact_mask from plain C: every documented error comes back before any
 * device work, so this runs without a GPU - and under the host sanitizers, with the library's host code built the same way:
 *
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC -shared -Xarch_host -fsanitize=address,undefined \
 *       -o /tmp/libgradjune_hip_asan.so gradabm-june_amd/csrc/gradjune_hip.hip
 *   hipcc -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude examples/contact_args.c \
 *       -L/tmp -lgradjune_hip_asan -Wl,-rpath,/tmp -o /tmp/contact_args && ASAN_OPTIONS=detect_leaks=0 /tmp/contact_args
 */
#include <math.h>
#include <stdio.h>
#include <stdint.h>
#include "gradjune_hip.h"

#define EXPECT(call, want) do { int rc_ = (call); if (rc_ != (want)) { printf("FAIL %s: %d, expected %d\n", #call, rc_, (want)); bad = 1; } } while (0)

int main(void) {
  int bad = 0;
  int32_t rowptr[2] = {0, 0}, venue[1] = {0};
  uint32_t until[1] = {0}, err = 0;
  float stage[1] = {1.0f}, q[1] = {0.0f};
  gj_contact_set sets[GJ_MAX_SETS + 1];
  for (int s = 0; s <= GJ_MAX_SETS; ++s) {
    sets[s].a_rowptr = rowptr; sets[s].a_venue = venue; sets[s].until = until; sets[s].n_venues = 1; sets[s].release = 15.0f;
  }
  EXPECT(gj_contact_mark(-1, stage, 4.0f, sets, 1, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, 0, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, GJ_MAX_SETS + 1, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mark(1, stage, 4.0f, NULL, 1, &err, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, 1, NULL, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mark(1, NULL, 4.0f, sets, 1, &err, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mark(0, NULL, 4.0f, sets, GJ_MAX_SETS, &err, NULL), GJ_OK);
  sets[1].release = -1.0f;
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, 2, &err, NULL), GJ_E_RANGE);
  sets[1].release = NAN;
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, 2, &err, NULL), GJ_E_RANGE);
  sets[1].release = 15.0f; sets[1].n_venues = -1;
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, 2, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 2, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_RANGE);
  sets[1].n_venues = (int64_t)1 << 31;
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 2, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_RANGE);
  sets[1].n_venues = 1; sets[1].until = NULL;
  EXPECT(gj_contact_mark(1, stage, 4.0f, sets, 2, &err, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 2, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_NULL);
  sets[1].until = until;
  EXPECT(gj_contact_mask(-1, stage, 4.0f, sets, 1, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 1, 1.0f, 1.0f, 1, 2, -4, q, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 13, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_RANGE);
  EXPECT(gj_contact_mask(1, stage, 4.0f, NULL, 1, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 1, 1.0f, 1.0f, 1, 2, 0, NULL, &err, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mask(1, NULL, 4.0f, sets, 1, 1.0f, 1.0f, 1, 2, 0, q, &err, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mask(1, stage, 4.0f, sets, 1, 1.0f, 1.0f, 1, 2, 0, q, NULL, NULL), GJ_E_NULL);
  EXPECT(gj_contact_mask(0, NULL, 4.0f, sets, GJ_MAX_SETS, 1.0f, 1.0f, 1, 2, 0, NULL, &err, NULL), GJ_OK);
  printf(bad ? "argument checks: FAILED\n" : "argument checks: ok\n");
  return bad;
}
