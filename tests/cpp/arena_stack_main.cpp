// The arena's bump stack (csrc/lgs_arena.h) on the CPU: every case prints its name; the first failed check ends the program with 1.
#include <stdio.h>
#include <stdlib.h>

#include "lgs_arena.h"

using lgs::ArenaStack;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static void full_block_fails_cleanly() {
  ArenaStack a;
  a.reset(1024);
  size_t off[5] = {7, 7, 7, 7, 7};
  for (int i = 0; i < 4; ++i) CHECK(a.take(256, &off[i]) && off[i] == (size_t)i * 256);
  CHECK(a.used() == 1024);
  CHECK(!a.take(1, &off[4]));                      // full: refused, nothing moved
  CHECK(off[4] == 7 && a.used() == 1024 && a.peak() == 1024);
  a.release(off[3]);
  CHECK(a.used() == 768);
  CHECK(!a.take(257, &off[4]) && off[4] == 7 && a.used() == 768);   // rounds to 512: does not fit
  CHECK(a.take(256, &off[4]) && off[4] == 768);
  ArenaStack none;                                  // no block at all
  CHECK(!none.take(1, &off[0]) && none.used() == 0 && none.peak() == 0);
  puts("full block fails cleanly");
}

static void allocation_order_pops_at_the_last_release() {
  ArenaStack a;
  a.reset(4096);
  size_t off[4];
  for (int i = 0; i < 4; ++i) CHECK(a.take(512, &off[i]));
  for (int i = 0; i < 3; ++i) {
    a.release(off[i]);
    CHECK(a.used() == 2048);
  }
  a.release(off[3]);
  CHECK(a.used() == 0);
  puts("allocation order pops at the last release");
}

static void reverse_order_pops_each_time() {
  ArenaStack a;
  a.reset(4096);
  size_t off[4];
  for (int i = 0; i < 4; ++i) CHECK(a.take(512, &off[i]));
  for (int i = 3; i >= 0; --i) {
    a.release(off[i]);
    CHECK(a.used() == (size_t)i * 512);
  }
  puts("reverse order pops each time");
}

static void hole_under_a_live_block() {
  ArenaStack a;
  a.reset(4096);
  size_t tmp, keep, next;
  CHECK(a.take(1024, &tmp) && a.take(256, &keep));
  a.release(tmp);                                   // a released block under a live one: the hole stays
  CHECK(a.used() == 1280);
  CHECK(a.take(256, &next) && next == 1280);        // and is not handed out again
  a.release(next);
  CHECK(a.used() == 1280);
  a.release(keep);                                  // the live one goes: both are reclaimed
  CHECK(a.used() == 0);
  CHECK(a.take(256, &next) && next == 0);
  puts("hole under a live block");
}

static void unknown_offset_is_ignored() {
  ArenaStack a;
  a.reset(4096);
  size_t x, y;
  CHECK(a.take(256, &x) && a.take(256, &y));
  a.release(128);
  a.release(512);
  a.release(1u << 20);
  CHECK(a.used() == 512);
  a.release(y);
  a.release(y);                                     // twice: the second finds nothing
  CHECK(a.used() == 256);
  ArenaStack none;
  none.release(0);
  CHECK(none.used() == 0);
  puts("unknown offset is ignored");
}

static void peak_is_the_high_water_mark() {
  ArenaStack a;
  a.reset(8192);
  size_t x, y, z;
  CHECK(a.peak() == 0);
  CHECK(a.take(1024, &x) && a.take(2048, &y));
  CHECK(a.peak() == 3072);
  a.release(y);
  CHECK(a.used() == 1024 && a.peak() == 3072);
  CHECK(a.take(512, &z) && a.peak() == 3072);
  CHECK(a.take(2048, &y) && a.peak() == 3584);
  a.release(y); a.release(z); a.release(x);
  CHECK(a.used() == 0 && a.peak() == 3584);
  a.reset(8192);                                    // a new block starts over
  CHECK(a.peak() == 0 && a.capacity() == 8192);
  puts("peak is the high-water mark");
}

static void sizes_round_up_to_256() {
  CHECK(ArenaStack::rounded(0) == 0 && ArenaStack::rounded(1) == 256 && ArenaStack::rounded(256) == 256 && ArenaStack::rounded(257) == 512);
  ArenaStack a;
  a.reset(4096);
  size_t off[4];
  CHECK(a.take(1, &off[0]) && a.take(255, &off[1]) && a.take(256, &off[2]) && a.take(300, &off[3]));
  CHECK(off[0] == 0 && off[1] == 256 && off[2] == 512 && off[3] == 768 && a.used() == 1280);
  puts("sizes round up to 256");
}

int main() {
  full_block_fails_cleanly();
  allocation_order_pops_at_the_last_release();
  reverse_order_pops_each_time();
  hole_under_a_live_block();
  unknown_offset_is_ignored();
  peak_is_the_high_water_mark();
  sizes_round_up_to_256();
  puts("arena stack ok: 7 cases");
  return 0;
}
