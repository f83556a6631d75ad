// The host side of csrc/lgs_idioms.h on the CPU: searches, ordered keys, workspace layouts.  Every case prints its name; the first
// failed check ends the program with 1.
#include <float.h>
#include <limits.h>
#include <limits>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lgs_idioms.h"

using namespace lgs;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      exit(1);                                                               \
    }                                                                        \
  } while (0)

static void lower_and_upper_bound() {
  const int64_t t7[7] = {1, 3, 3, 3, 5, 8, 8}, t2[2] = {4, 4}, t1[1] = {7};
  const int64_t *t0 = nullptr;                                     // no element: never read
  // 7 elements with duplicates: below all, equal to an element, between two, above all
  const int64_t k7[8] = {0, 1, 2, 3, 4, 5, 8, 9};
  const int lb7[8] = {0, 0, 1, 1, 4, 4, 5, 7}, ub7[8] = {0, 1, 1, 4, 4, 5, 7, 7};
  for (int i = 0; i < 8; ++i) {
    CHECK(lower_bound(t7, 0, 7, k7[i]) == lb7[i]);
    CHECK(upper_bound(t7, 0, 7, k7[i]) == ub7[i]);
    CHECK(lower_bound(t7, (int64_t)0, (int64_t)7, k7[i]) == (int64_t)lb7[i]);      // the other index type
    CHECK(upper_bound(t7, (int64_t)0, (int64_t)7, k7[i]) == (int64_t)ub7[i]);
  }
  CHECK(lower_bound(t7, 2, 5, (int64_t)3) == 2 && lower_bound(t7, 2, 5, (int64_t)9) == 5);      // a sub-range: answers stay inside it
  CHECK(upper_bound(t7, 2, 5, (int64_t)3) == 4 && upper_bound(t7, 2, 5, (int64_t)0) == 2);
  CHECK(lower_bound(t2, 0, 2, (int64_t)3) == 0 && lower_bound(t2, 0, 2, (int64_t)4) == 0 && lower_bound(t2, 0, 2, (int64_t)5) == 2);
  CHECK(upper_bound(t2, 0, 2, (int64_t)3) == 0 && upper_bound(t2, 0, 2, (int64_t)4) == 2 && upper_bound(t2, 0, 2, (int64_t)5) == 2);
  CHECK(lower_bound(t1, 0, 1, (int64_t)6) == 0 && lower_bound(t1, 0, 1, (int64_t)7) == 0 && lower_bound(t1, 0, 1, (int64_t)8) == 1);
  CHECK(upper_bound(t1, 0, 1, (int64_t)6) == 0 && upper_bound(t1, 0, 1, (int64_t)7) == 1 && upper_bound(t1, 0, 1, (int64_t)8) == 1);
  CHECK(lower_bound(t0, 0, 0, (int64_t)5) == 0 && upper_bound(t0, 0, 0, (int64_t)5) == 0);
  // an element type narrower than the key (the proposal offsets of the instance evaluation: int32 ends, an int64 member index)
  const int32_t ends[4] = {0, 5, 5, 9};
  CHECK(upper_bound(ends, 0, 4, (int64_t)0) == 1 && upper_bound(ends, 0, 4, (int64_t)4) == 1 && upper_bound(ends, 0, 4, (int64_t)5) == 3 &&
        upper_bound(ends, 0, 4, (int64_t)9) == 4);
  puts("lower_bound and upper_bound");
}

static void last_not_above_with_empty_records() {
  // seven records over 12 rows: 0 empty (leading), 1 = [0, 3), 2 and 3 empty (middle), 4 = [3, 9), 5 = [9, 12), 6 empty (trailing)
  const int64_t starts[7] = {0, 0, 3, 3, 3, 9, 12};
  const int record_of_row[12] = {1, 1, 1, 4, 4, 4, 4, 4, 4, 5, 5, 5};
  const int strides[3] = {1, 4, 6}, cols[3] = {0, 1, 3};          // the scene offsets; the paste's slot table (column 1); six columns, column 3
  for (int v = 0; v < 3; ++v) {
    int64_t table[7 * 6];
    for (int j = 0; j < 7 * 6; ++j) table[j] = (j % 2) ? -1000 : 1000;      // the other columns are not looked at
    for (int t = 0; t < 7; ++t) table[strides[v] * t + cols[v]] = starts[t];
    for (int64_t i = 0; i < 12; ++i) CHECK(last_not_above(table + cols[v], strides[v], 7, i) == record_of_row[i]);
    CHECK(last_not_above(table + cols[v], strides[v], 7, (int64_t)12) == 6);      // one past the rows: the last record
    CHECK(last_not_above(table + cols[v], strides[v], 7, (int64_t)-1) == 0);      // below every start
    CHECK(last_not_above(table + cols[v], strides[v], 1, (int64_t)5) == 0);
    CHECK(last_not_above(table + cols[v], strides[v], 2, (int64_t)0) == 1);       // {0, 0}: the empty record 0 loses
    CHECK(last_not_above(table + cols[v], strides[v], 0, (int64_t)0) == 0);       // no record: nothing is read
  }
  const int64_t two[2] = {0, 5};
  CHECK(last_not_above(two, 1, 2, (int64_t)4) == 0 && last_not_above(two, 1, 2, (int64_t)5) == 1);
  puts("last_not_above with empty records");
}

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof(u));
  return u;
}

static void ordered_keys() {
  const float inf = std::numeric_limits<float>::infinity(), den = std::numeric_limits<float>::denorm_min();
  const float f[10] = {-inf, -FLT_MAX, -1.0f, -den, -0.0f, 0.0f, den, 1.0f, FLT_MAX, inf};
  for (int i = 0; i < 10; ++i) {
    if (i > 0) CHECK(ord_key(f[i - 1]) < ord_key(f[i]));           // strictly: -0 lies in front of +0 in the plain map
    CHECK(bits_of(ord_key_inv(ord_key(f[i]))) == bits_of(f[i]));
    CHECK(ord_key_of_bits(bits_of(f[i])) == ord_key(f[i]));
  }
  CHECK(ord_key(inf) == 0xFF800000u && ord_key(-inf) == 0x007FFFFFu);      // the neutral elements lgs_augment.hip starts its bounds from
  const int32_t v[5] = {INT_MIN, -1, 0, 1, INT_MAX};
  for (int i = 0; i < 5; ++i) {
    if (i > 0) CHECK(ikey(v[i - 1]) < ikey(v[i]));
    CHECK(ikey_inv(ikey(v[i])) == v[i]);
  }
  CHECK(ikey(INT_MIN) == 0u && ikey(INT_MAX) == 0xFFFFFFFFu);
  puts("ordered keys");
}

static void layout_take() {
  Layout l;
  CHECK(l.total() == 0);
  CHECK(l.take(1) == 0 && l.total() == 256);
  CHECK(l.take(256) == 256 && l.total() == 512);
  CHECK(l.take(257) == 512 && l.total() == 1024);
  CHECK(l.take(0) == 1024 && l.total() == 1024);                  // an empty region takes nothing
  CHECK(l.take(1000) == 1024 && l.total() == 2048);
  CHECK(align256(0) == 0 && align256(255) == 256 && align256(256) == 256 && align256((1ll << 40) + 1) == (1ll << 40) + 256);
  char base[16];
  CHECK(reinterpret_cast<char *>(Layout::at<int32_t>(base, 8)) == base + 8);
  puts("Layout::take rounds to 256");
}

struct Region { int64_t off, bytes; };
// regions in the order of the workspace: the first at 0, each 256-aligned and ending before the next begins, the last inside total
static void check_regions(const Region *r, int n, int64_t total) {
  CHECK(r[0].off == 0);
  for (int i = 0; i < n; ++i) {
    CHECK(r[i].off % 256 == 0 && r[i].bytes >= 0);
    CHECK(r[i].off + r[i].bytes <= (i + 1 < n ? r[i + 1].off : total));
  }
  CHECK(total % 256 == 0);
}

static void operator_layouts() {
  // each: an empty argument set, the smallest non-empty one, odd sizes.  The totals are the closed formulas the *_workspace_bytes
  // functions returned before the layouts existed, typed as they stood.
  {
    const int64_t ns[3] = {0, 1, 1000}, tmps[3] = {0, 1, 12345};
    const int cs[3] = {1, 1, 13};
    for (int v = 0; v < 3; ++v) {
      const int64_t n = ns[v], tmp = tmps[v];
      const int c = cs[v];
      const ApWs w = ap_layout(n, c, tmp);
      CHECK(w.total == align256(tmp) + 3 * align256(8 * (n + 1)) + 2 * align256(4 * (n + 1)) + 2 * align256(4 * (c + 1)) + 256);
      const Region r[8] = {{w.tmp, tmp}, {w.keys, 8 * n}, {w.skeys, 8 * n}, {w.rowstat, 8 * n}, {w.cnt, 4 * n}, {w.pfx, 4 * n},
                           {w.off, 4 * (c + 1)}, {w.mn, 4 * c}};
      check_regions(r, 8, w.total);
      CHECK(w.terms == w.keys);                                   // the terms reuse the unsorted keys
    }
  }
  {
    const int64_t ns[3] = {0, 1, 1000}, tmps[3] = {0, 1, 4097};
    for (int v = 0; v < 3; ++v) {
      const int64_t n = ns[v], tb = tmps[v];
      const ClusterWs w = cluster_layout(n, tb);
      CHECK(w.total == align256((int64_t)tb) + 2 * align256(8 * (n + 1)) + 4 * align256(4 * (n + 1)) + 512);
      const Region r[8] = {{w.tmp, tb}, {w.keys, 8 * n}, {w.skeys, 8 * n}, {w.vals, 4 * n}, {w.svals, 4 * n}, {w.parent, 4 * n},
                           {w.size, 4 * n}, {w.scal, 8}};
      check_regions(r, 8, w.total);
    }
  }
  {
    CHECK(inst_table_size(1) == 2 && inst_table_size(37) == 128 && inst_table_size(4096) == 8192);
    CHECK(inst_pieces(0, 0) == 1 && inst_pieces(1, 1) == 3 && inst_pieces(1000, 13) == 15 && inst_pieces(1025, 0) == 3);
    const int64_t ms[3] = {0, 1, 1000}, ts[3] = {2, 2, 128}, pcs[3] = {1, 3, 15};
    const int ps[3] = {0, 1, 13}, caps[3] = {1, 1, 37};
    for (int v = 0; v < 3; ++v) {
      const int64_t t = ts[v], pieces = pcs[v];
      const InstOverlapWs w = inst_overlap_layout(ms[v], ps[v], caps[v]);
      CHECK(w.total == align256(8 * t) + align256(4 * t) + 256 + align256(4 * pieces) + align256(8 * pieces));
      const Region r[5] = {{w.t_key, 8 * t}, {w.t_cnt, 4 * t}, {w.n_slots, 4}, {w.part_max, 4 * pieces}, {w.part_sum, 8 * pieces}};
      check_regions(r, 5, w.total);
      CHECK(w.zeroed == w.part_max);                              // the table and the counter are cleared, the partials are not
    }
  }
  {
    const int bs[3] = {0, 1, 3};
    const int64_t cells[3] = {27, 27, 1001};
    for (int v = 0; v < 3; ++v) {
      const int b = bs[v];
      const int64_t max_cells = cells[v];
      const ElasticWs w = elastic_layout(b, max_cells);
      CHECK(w.total == 2 * align256((int64_t)b * max_cells * 3 * (int64_t)sizeof(float)));
      const Region r[2] = {{w.noise, b * max_cells * 12}, {w.field, b * max_cells * 12}};
      check_regions(r, 2, w.total);
    }
  }
  {
    CHECK(table_cap(0) == 64 && table_cap(32) == 64 && table_cap(33) == 128 && table_cap(1000) == 2048);
    const int bs[3] = {1, 1, 3}, slots[3] = {0, 1, 13};
    const int64_t rows[3] = {0, 1, 1000}, cells[3] = {1, 1, 1001}, caps[3] = {64, 64, 2048};
    for (int v = 0; v < 3; ++v) {
      const int b = bs[v];
      const int64_t s1 = slots[v] > 1 ? slots[v] : 1, r1 = rows[v] > 1 ? rows[v] : 1, cap = caps[v], mc = cells[v];
      const PasteWs w = paste_layout(b, slots[v], rows[v], mc);
      CHECK(w.cap == cap);
      CHECK(w.total == align256(8 * (b + 1)) + align256(4 * 6 * b) + align256(4 * 32) + align256(64 * s1) + align256(4 * 4 * s1) +
                           align256(8 * cap) + align256(4 * cap) + align256(4 * r1) + align256(4 * 4 * r1) + align256(4 * b * mc));
      const Region r[10] = {{w.off, 8 * (b + 1)}, {w.bounds, 24 * b}, {w.flags, 128}, {w.stats, 64 * s1}, {w.place, 16 * s1},
                            {w.hkeys, 8 * cap}, {w.hmin, 4 * cap}, {w.hslot, 4 * r1}, {w.ivox, 16 * r1}, {w.maps, 4 * b * mc}};
      check_regions(r, 10, w.total);
    }
  }
  puts("operator layouts keep their totals and order");
}

int main() {
  lower_and_upper_bound();
  last_not_above_with_empty_records();
  ordered_keys();
  layout_take();
  operator_layouts();
  puts("idioms ok: 5 cases");
  return 0;
}
