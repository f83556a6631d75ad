// lgs_tuning.hip -- ONE table of the engine's tuning / debugging knobs, and the per-launch-site dispatch counters.
//
// Every knob used to be a `static const ... getenv(...)` next to its launch site (20 of them by round 3).  They now live in
// the table below: name, default, what it does.  A knob's initial value comes from the environment variable LGS_<NAME> (read
// once, at the first query), lgs_tuning_set() changes it at run time (the parity tests use that, e.g. to send a 70 k-row
// layer through the kernel that production only picks above 200 k rows), lgs_tuning_describe() prints the table.
//
// Dispatch counters: every kernel launch of the engine goes through LGS_KLAUNCH (lgs_common.h), which bumps a counter keyed
// by the launch site's kernel expression + the template bindings of the enclosing function.  tests/ read them to assert that
// every kernel instantiation the benchmarked steps dispatch is also dispatched by a parity test (round 3 shipped a hot
// kernel that no test reached because of a size gate).
#include <atomic>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lgs_common.h"

namespace lgs {

namespace {
struct Knob { Tune id; const char *name; int64_t def; const char *doc; };
// in the order of enum Tune (lgs_common.h): every row names its enumerator, init_knobs() refuses a table whose row i is not knob i
const Knob kKnobs[T_COUNT] = {
    {T_WW_MIN_ROWS, "WW_MIN_ROWS", 200000, "k_wgrad_wide (per-offset GEMM over compacted pair lists) is used for 3^3 weight gradients with >= 256 x 256 "
                            "channels on maps of at least this many positions; below, k_wgrad_ps wins (81 k rows, 256->256: 0.82 vs 0.31 ms)"},
    {T_WW_RANGE, "WW_RANGE", 16384, "positions per k_wgrad_wide workgroup range (multiple of 256; 8192 overflows the partial-tile cap, 65536: 8.6 vs 7.5 ms)"},
    {T_WGRAD_WIDE, "WGRAD_WIDE", 1, "0 = never use k_wgrad_wide (A/B)"},
    {T_BN_FUSED, "BN_FUSED", 1, "0 = BatchNorm always as three launches (column sums, fold, apply) instead of the persistent grid-barrier kernels; "
                    "required when several processes time-share one GPU"},
    {T_BN_FUSED_MAX_MB, "BN_FUSED_MAX_MB", 24, "layers above this size use the three-launch BatchNorm (they are bandwidth-bound; the 4096-workgroup apply streams faster)"},
    {T_BN_FUSED_FWD_MAX_MB, "BN_FUSED_FWD_MAX_MB", 0, "the same bound for the FORWARD direction alone; 0 = the forward is always three launches.  Round 4: with the host "
                               "no longer the bound the one-launch forward loses at every size (8-scene step 27.93 vs 28.15 ms, one scene 10.17 vs "
                               "10.30; stand-alone 20 MB: 22.8 vs 33.0 us), the one-launch BACKWARD still wins (16.4 vs 16.8 ms of backward)"},
    {T_BN_FUSED_BLOCKS, "BN_FUSED_BLOCKS", 0, "workgroups of the fused BatchNorm kernels; 0 = min(256, co-resident workgroups of the device)"},
    {T_PS_CUS, "PS_CUS", 20, "CUs per XCD that k_wgrad_ps fills (of 32): the compute stream keeps CUs of its own next to the CU-owning weight gradient"},
    {T_PS_WIDE3, "PS_WIDE3", 1, "k_wgrad_ps: three-block stationary slices for >= 256-channel layers (0 = two-block)"},
    {T_WGRAD_PS, "WGRAD_PS", 1, "0 = force the round-1 pair-list weight gradient (k_wgrad_bf16) everywhere (debugging)"},
    {T_MASK_WINDOW, "MASK_WINDOW", 16384, "3^3 maps: positions per window inside which rows are re-sorted by their 27-bit neighbour mask (1024 .. 65536 swept)"},
    {T_CONV_SPLIT, "CONV_SPLIT", 1, "0 = no slot split (3 x 9 offsets into fp32 partial images) for under-filled coarse-level 3^3 launches"},
    {T_SMALL_CFG, "SMALL_CFG", 0, "k_conv_gather tile for maps < 65536 positions: 0 = automatic (id 8), 5 / 9 / 10 / 11 = the other measured shapes"},
    {T_WIDE_GC64, "WIDE_GC64", 1, "k_conv_wide: 64-channel stages per reduction group"},
    {T_ARENA_DBG, "ARENA_DBG", 0, "print coordinate-manager arena allocations to stderr"},
    {T_CONV_WIDE, "CONV_WIDE", 1, "0 = >= 256-output-channel layers stay on k_conv_gather's 8-wave tile (id 16) instead of k_conv_wide (A/B)"},
    {T_MASK_ORDER, "MASK_ORDER", 0, "3^3 maps: sort code of the neighbourhood mask inside a window: 0 the mask, 1 corners > edges > faces, 2 faces > edges > corners, 3 popcount-major"},
    {T_BN_FOLD, "BN_FOLD", 1, "1 = BatchNorm layers up to BN_FOLD_MAX_MB run as TWO launches per direction: column sums into <= BN_FOLD_PARTS partial rows, "
                   "then an apply kernel whose workgroups fold the partial rows themselves (no fold launch, no grid barrier); 0 = the round-4 "
                   "policies (grid-barrier kernel backward, three launches forward)"},
    {T_BN_FOLD_MAX_MB, "BN_FOLD_MAX_MB", 6, "layers above this size keep the round-4 policies.  Stand-alone (tools/dbg/bn_small.py, bf16): 2.6 MB 15.2 / 21.1 us forward / backward against 16.1 / 29.0 (three launches / grid barriers), 5 MB 17.8 / 26.0 against 16.0 / 27.6; at 10 - 20 MB the wider 512-row reduction wins (22 / 37 - 59 against 16 - 23 / 32 - 46)"},
    {T_BN_FOLD_PARTS, "BN_FOLD_PARTS", 64, "partial rows of the two-launch BatchNorm (<= 64): fewer = a shorter fold in every apply workgroup, more = a wider reduction"},
    {T_BN_FOLD_GRID, "BN_FOLD_GRID", 256, "apply workgroups of the two-launch BatchNorm (each folds the partial rows redundantly)"},
    {T_FP32_SPLIT, "FP32_SPLIT", 1, "fp32 tensors: 1 = convolution forward / dgrad multiply on the bf16 matrix pipe with exactly split operands (x = hi + mid + lo, "
                      "six bf16 products accumulated in fp32: error below 2^-22 |x||w|, 2.7 x the MFMA rate of v_mfma_f32_32x32x2_f32); "
                      "0 = the exact-fp32 MFMA instance"},
    {T_BLOCK_WGRAD_LATE, "BLOCK_WGRAD_LATE", 0, "A/B: 1 = lgs_block_backward forks the FIRST convolution's weight gradient after the block's last dgrad instead of "
                            "beside it (the 96->128 dgrad of block8.0 runs 2.1 x its stand-alone time next to k_wgrad_ps 128->96)"},
    {T_WGRAD_F32_LDS, "WGRAD_F32_LDS", 2, "fp32 weight gradients: 2 = rows staged through LDS as three exactly-split bf16 planes, six bf16 MFMAs per 16 pairs "
                                          "(k_wgrad_f32s_lds; dropped terms < 2^-24 |x g|, fp32 accumulate).  Stand-alone it wins at >= 96 input channels only "
                                          "(96 -> 96: 3.06 vs 3.38 ms; 32 -> 32: 1.06 vs 0.84), in the STEP it wins everywhere: 82.4 - 82.9 vs 86.1 - 86.7 ms -- it "
                                          "holds the matrix pipe 2.7 x shorter than the exact-fp32 MFMA and the convolutions on the other stream get it "
                                          "(round 6); 3 = split only where it also wins stand-alone (83.5 - 83.7 ms); 1 = exact-fp32 MFMA on staged rows "
                                          "(k_wgrad_f32_lds; bit-identical to 0); 0 = k_wgrad_f32 (one 4-byte load per lane and MFMA operand)"},
    {T_WIDE_SCHED, "WIDE_SCHED", 0, "k_conv_wide: where the two waves of a SIMD issue the next stage's LDS-DMA between their four row blocks.  0 = "
                                    "weights first / gathers after block 1 (round 3); 1 = gathers first, weights after block 1; 2 = gathers first, "
                                    "weights after block 0; 3 = gathers first, weights after block 2; 4 = both first (round 2's schedule)"},
    {T_HEAD_TILE, "HEAD_TILE", 0, "1x1 layers with 5 - 7 output blocks on the big maps (the 200-class head): 0 = one 128-position tile spans all output "
                                  "channels (the feature matrix is streamed once; 7 x 16 accumulator registers per wave), 1 = the generic 4-block tile "
                                  "(two column tiles, features read twice, 3 waves per SIMD)"},
    {T_POINTWISE, "POINTWISE", 1, "bf16 1x1 stride-1 convolutions (and their dgrads) on maps of >= 65536 positions with <= 224 output channels run on "
                                  "k_pointwise (persistent streaming GEMM, lgs_pointwise.hip) instead of k_conv_gather's identity-map tiles where that wins (5 - 7 output "
                                  "blocks, or > 128 reduction channels into 3 blocks: the 200-class head and its dgrad); 2 = every shape it serves; 0 = off (A/B)"},
    {T_INSTANCE_NORM, "INSTANCE_NORM", 1, "MinkowskiInstanceNorm on HIP tensors: 1 = the per-scene kernels of lgs_instnorm.hip (two passes per direction, no host "
                                          "synchronisation, reproducible); 0 = the torch lines the CPU path uses (index_add_ on fp32 copies, one .item() per "
                                          "call) -- read at call time: for timing the old path in the same process and for switching the kernels off in the field"},
    {T_METRICS_BLOCKS, "METRICS_BLOCKS", 8192, "most workgroups of a k_seg_metrics launch (lgs_metrics.hip); each walks tiles blockIdx.x, + gridDim.x, ... and adds its "
                                               "LDS table of (label, pred) counts to the confusion matrix once at its end, so a cell costs at most this many "
                                               "global atomics per call.  1.2 M x 200 bf16, no prob, uniform / 90 %-on-one-cell labels: 2048 373 / 273 us (two "
                                               "uneven rounds of resident workgroups), 4096 284 / 228, 8192 242 / 220, 16384 231 / 264, one tile per workgroup "
                                               "234 / 497 (37 500 adds on one address); small values let a test walk many tiles per workgroup on a few thousand rows"},
    {T_SUPCON_FUSED, "SUPCON_FUSED", 1, "PointSupConLoss on HIP tensors: 1 = the kernels of lgs_supcon.hip (k_supcon_sample, k_supcon_fwd, k_supcon_bwd: (1 + P + K) row "
                                        "reads per point, no [N, P + K, C] tensor); 0 = the torch gather path CPU tensors take (index gathers, normalise, mean) and "
                                        "the torch restatement of the sampler -- read at call time: for timing the two next to each other and for switching "
                                        "the kernels off in the field"},
    {T_BN_PAIR, "BN_PAIR", 1, "BatchNorm passes shared inside a residual block (paths `three` and `fold`; A/B): 1 = lgs_bn_backward masks dy ONCE when it "
                              "also returns the residual gradient (the reduce launch writes the masked gradient, the apply reads it back: 7 tensor "
                              "passes instead of 8), and lgs_bn_forward_pair / lgs_bn_backward_pair run the two norms of a downsample block on shared "
                              "reads (5 instead of 7 passes forward, 10 instead of 13 backward, 3 launches instead of 6); 0 = the single calls, dy "
                              "masked in both launches.  Bit-identical either way"},
    {T_MAP_WINDOW_SORT, "MAP_WINDOW_SORT", 1, "3^3 maps, the window mask sort (A/B): 1 = k_window_sort, one workgroup per MASK_WINDOW positions sorts (mask code, index in "
                                              "window) in LDS with a bitonic network, one launch per view; 0 = 64-bit keys (window, code) through rocPRIM's radix "
                                              "sort over the whole map (13 launches per view).  A window that is no power of two in 1024 .. 16384 takes the radix "
                                              "sort either way.  The permutation is identical"},
    {T_MAP_BLOCK_DIR, "MAP_BLOCK_DIR", 1, "3^3 maps, neighbour lookup (A/B): 1 = a directory with one entry per occupied 4 x 4 x 4 block of cells {block id, first "
                                          "sorted position, 64-bit occupancy}; a probe is one entry and a popcount; 0 = the open-addressing hash with one slot "
                                          "per voxel (>= 2 n slots of 12 bytes).  The tables are identical"},
    {T_MAP_PERMUTE_LDS, "MAP_PERMUTE_LDS", 1, "3^3 maps, the row permutation after the window sort (A/B): 1 = k_permute_map3_lds, one workgroup per (MASK_WINDOW "
                                              "positions, group of offsets) stages the window's segment of every offset row in LDS with 16-byte loads and "
                                              "gathers from there; 0 = k_permute_map3, 27 four-byte gathers per position from global memory.  A window "
                                              "above 32768 positions or no multiple of 256 takes k_permute_map3 either way.  The tables are identical.  "
                                              "Five maps of the 8-scene batch: 352 -> 90 us, all maps 1.86 -> 1.61 ms (profiles/map_stream.txt)"},
    {T_MAP_PERMUTE_GROUP, "MAP_PERMUTE_GROUP", 0, "k_permute_map3_lds: offsets per workgroup (the grid against the re-reads of the permutation).  0 = as many as "
                                                  "leave 640 workgroups (8-scene batch: 3 at level 0, 1 on the coarser maps); 1 .. 27 = that many on every "
                                                  "map; above 27 = as 0 with that many workgroups as the aim.  All maps: 1.61 ms at 0, 1, 2, 3 and at 320 / "
                                                  "1280 workgroups, 1.62 at 5, 1.65 at 9 -- flat wherever level 0 has at least ~600 workgroups"},
    {T_MAP_OWN_SORTS, "MAP_OWN_SORTS", 1, "2^3 stride-2 maps, grouping the fine rows by child index (A/B): 1 = a stable 8-way partition in three launches "
                                          "(k_child_hist per-workgroup counts, k_child_prefix one workgroup, k_child_scatter writes the grouped view "
                                          "itself); 0 = k_child_keys, rocPRIM's radix sort on 3 key bits, k_group_offsets, k_build_map2_fine.  The "
                                          "tables are identical.  Four maps of the 8-scene batch: 378 us in 57 launches -> 130 us in 12, all maps "
                                          "1.86 -> 1.61 ms (profiles/map_stream.txt)"},
    {T_MAP_CHILD_ROUNDS, "MAP_CHILD_ROUNDS", 0, "k_child_hist / k_child_scatter: rounds of 256 positions per workgroup (two barriers and a dependent load each).  "
                                                "0 = as many as leave 512 workgroups, between 1 and 16 (8-scene batch: 9 at level 0, 2 at level 1, 1 below); "
                                                "1 .. 16 = that many on every map (tests walk several rounds on small maps with it)"},
    {T_CONV_SLAB_TRIM, "CONV_SLAB_TRIM", 1, "k_conv_gather, bf16 tiles 0 / 1 / 2 / 7 with one reduction group of <= 8 chunks (A/B): 1 = the weight slabs the kernel fetches "
                                            "and stages hold real chunks only (nc below the image's slab length sc: one slab of nc; otherwise the largest "
                                            "divisor of nc below sc; tile 7 with 3 chunks: one slab of 3), the zero chunks the packed image pads an offset "
                                            "with are never loaded; 2 = as 1 with tile 7's 3 chunks as three 1-chunk slabs; 0 = whole image slabs.  Same "
                                            "chunks, same order, same MFMAs: bit-identical (profiles/conv_zero_loads.txt)"},
    {T_CONV_ROW_TRIM, "CONV_ROW_TRIM", 1, "k_conv_gather tile 0 on rows of one 16-byte piece (conv0's 3 colour channels padded to 8; needs CONV_SLAB_TRIM): 1 = only "
                                          "the first of a chunk's two gathers is issued, the fragment of the second piece is a zero register; 0 = both "
                                          "(the second is out of range in every lane).  Bit-identical"},
    {T_NEAREST_MAX_RING, "NEAREST_MAX_RING", 2, "lgs_manager_nearest: the last ring of cells (Chebyshev distance from the query's home cell) that k_nearest_ring searches "
                                                "through the map's lookup table before a query goes to the exact scan of its scene's keys (k_nearest_scan).  The "
                                                "answer is the same at every value (tests/test_gpu_nearest.py).  3.6 M points inside the occupied cells of the 8-scene, "
                                                "1.2 M-voxel batch, block directory, voxel corners / centres as sites: 1 = 1.056 / 0.514 ms with 0.025 % / 0 of the "
                                                "queries left to the scan, 2 = 0.611 / 0.514 ms with none, 4 = the same as 2 (tools/microbench.py nearest)"},
    {T_INST_EVAL_FUSED, "INST_EVAL_FUSED", 1, "insteval.instance_overlaps and Clustering.get_proposals on HIP tensors: 1 = the kernels of lgs_insteval.hip (one gather "
                                              "and one table probe per proposal member, an LDS histogram per piece of a proposal); 0 = the torch lines CPU tensors "
                                              "take (torch.unique over the ids, one bincount over (proposal, id) pairs, torch.max / mean per proposal) -- read at call "
                                              "time.  The integer tables and the max confidences are equal (tests/test_gpu_insteval.py)"},
    {T_CONV_LEAN_EPI, "CONV_LEAN_EPI", 1, "k_conv_gather, bf16 (A/B): 1 = a launch that writes no BatchNorm statistics (every dgrad, every forward without "
                                          "`partial`) runs the instance built without the statistics epilogue, whose registers every instance used to be sized "
                                          "for (tile 7: 204 -> 137 / 147 on its 2- and 3-chunk walks, three workgroups per CU instead of two, the 3-chunk walk with one weight slab in LDS); a launch with "
                                          "`partial` runs the instance with it.  Tile 7 takes its lean instances only on a grid of more than 512 workgroups "
                                          "(two per CU hold the rest; 256 -> 256 at level 3 measured 1 % slower on them); 2 = as 1 on every grid (tests reach "
                                          "the instances on small maps with it).  0 = every launch runs the instance with the epilogue, the kernel as it was "
                                          "before the split.  Same chunks, same order, same MFMAs, same stores: bit-identical "
                                          "(profiles/conv_lean_epilogue.txt, tests/test_gpu_conv_lean_epilogue.py)"},
};
std::atomic<int64_t> g_val[T_COUNT];
std::once_flag g_once;

void init_knobs() {
  for (int i = 0; i < T_COUNT; ++i) {
    if ((int)kKnobs[i].id != i) {     // a knob added to the enum and the table in different places (round 5 shipped one for an hour)
      fprintf(stderr, "lgs_engine: tuning table row %d is %s but enum Tune says otherwise -- fix csrc/lgs_tuning.hip\n", i, kKnobs[i].name);
      abort();
    }
    const std::string env = std::string("LGS_") + kKnobs[i].name;
    const char *e = getenv(env.c_str());
    g_val[i].store(e ? atoll(e) : kKnobs[i].def, std::memory_order_relaxed);
  }
}
int find_knob(const char *name) {
  if (!name) return -1;
  if (!strncmp(name, "LGS_", 4)) name += 4;
  for (int i = 0; i < T_COUNT; ++i)
    if (!strcmp(name, kKnobs[i].name)) return i;
  return -1;
}

// ---- dispatch counters
constexpr int kMaxSites = 1024;
struct Site { std::string name; std::atomic<int64_t> hits{0}; };
Site g_sites[kMaxSites];
int g_nsites = 0;
std::mutex g_site_mu;

std::string squeeze(const char *s) {   // drop blanks and the outer parentheses hipLaunchKernelGGL needs around template commas
  std::string o;
  for (; *s; ++s)
    if (*s != ' ' && *s != '\t' && *s != '\n') o.push_back(*s);
  while (o.size() >= 2 && o.front() == '(' && o.back() == ')') o = o.substr(1, o.size() - 2);
  return o;
}
}  // namespace

int64_t tune(Tune t) {
  std::call_once(g_once, init_knobs);
  return g_val[t].load(std::memory_order_relaxed);
}

std::string dispatch_site_name(const char *kernel_text, const char *pretty_function) {
  std::string name = squeeze(kernel_text);
  // template bindings of the enclosing function, e.g. "[T = unsigned short, KIND = 0]" (clang's __PRETTY_FUNCTION__)
  if (pretty_function) {
    const char *b = strrchr(pretty_function, '[');
    if (b && strchr(b, '=')) name += " " + squeeze(b);
  }
  return name;
}

int dispatch_site(const char *kernel_text, const char *pretty_function) {
  const std::string name = dispatch_site_name(kernel_text, pretty_function);
  std::lock_guard<std::mutex> lk(g_site_mu);
  for (int i = 0; i < g_nsites; ++i)
    if (g_sites[i].name == name) return i;
  if (g_nsites >= kMaxSites) return kMaxSites - 1;
  g_sites[g_nsites].name = name;
  return g_nsites++;
}

void dispatch_hit(int site) { g_sites[site].hits.fetch_add(1, std::memory_order_relaxed); }

}  // namespace lgs

extern "C" {

int lgs_tuning_set(const char *name, int64_t value) {
  std::call_once(lgs::g_once, lgs::init_knobs);
  const int i = lgs::find_knob(name);
  LGS_REQUIRE(i >= 0, std::string("lgs_tuning_set: unknown knob '") + (name ? name : "(null)") + "'");
  lgs::g_val[i].store(value, std::memory_order_relaxed);
  return 0;
}

int lgs_tuning_get(const char *name, int64_t *value) {
  std::call_once(lgs::g_once, lgs::init_knobs);
  const int i = lgs::find_knob(name);
  LGS_REQUIRE(i >= 0 && value, std::string("lgs_tuning_get: unknown knob '") + (name ? name : "(null)") + "'");
  *value = lgs::g_val[i].load(std::memory_order_relaxed);
  return 0;
}

// "NAME\tdefault\tvalue\tdoc\n" per knob; returns the bytes needed (incl. the terminating NUL); writes at most cap bytes
int64_t lgs_tuning_describe(char *buf, int64_t cap) {
  std::call_once(lgs::g_once, lgs::init_knobs);
  std::string s;
  for (int i = 0; i < lgs::T_COUNT; ++i)
    s += std::string(lgs::kKnobs[i].name) + "\t" + std::to_string(lgs::kKnobs[i].def) + "\t" +
         std::to_string(lgs::g_val[i].load()) + "\t" + lgs::kKnobs[i].doc + "\n";
  if (buf && cap > 0) {
    const int64_t n = std::min<int64_t>(cap - 1, (int64_t)s.size());
    memcpy(buf, s.data(), (size_t)n);
    buf[n] = 0;
  }
  return (int64_t)s.size() + 1;
}

// "count\tsite\n" per launch site that was hit since the last reset; same size protocol as lgs_tuning_describe
int64_t lgs_debug_dispatch_counts(char *buf, int64_t cap, int reset) {
  std::string s;
  {
    std::lock_guard<std::mutex> lk(lgs::g_site_mu);
    for (int i = 0; i < lgs::g_nsites; ++i) {
      const int64_t h = reset ? lgs::g_sites[i].hits.exchange(0) : lgs::g_sites[i].hits.load();
      if (h > 0) s += std::to_string(h) + "\t" + lgs::g_sites[i].name + "\n";
    }
  }
  if (buf && cap > 0) {
    const int64_t n = std::min<int64_t>(cap - 1, (int64_t)s.size());
    memcpy(buf, s.data(), (size_t)n);
    buf[n] = 0;
  }
  return (int64_t)s.size() + 1;
}

}  // extern "C"
