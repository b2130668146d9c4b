// host_variants.h -- the kernel-variant tables, and setup_trace: where the intersect kernel reads the tree
// from and its persistent grid.
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_context.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

namespace {

// Kernel variants: the one place where run-time choices become template arguments.  Every launch, occupancy
// query and attribute call takes its kernel from these tables as a typed pointer (a wrong argument struct stays
// a compile error); a new tree route or template flag is a new table entry and nothing else.
//
// The GPU test that reaches each entry (H / B: the hybrid / bare walk, short_stack 1 / 0):
//   k_trace, count off: TREE_WIDE, PACKED, LDS, LDS16 / LDS16G, H and B -- test_soup_cast_equals_oracle (rootleaf8200
//     "tree_global", syn20000, "tree_format" 32, "tree_format" 16); LDS16G, LDS16S, H and B -- test_cast_equals_oracle
//     (ico7, ico7-margin); in renders test_tuning_knobs_keep_parity, test_derived_box_tree_in_lds
//   k_trace, count on: TREE_WIDE, PACKED, LDS, LDS16, H and B -- test_soup_counters_on_every_route; LDS, H also
//     test_counters_match_oracle; LDS16G, LDS16S, H -- test_counters_on_the_cluster_routes (B: no test)
//   k_shade: compact + sort -- test_iteration2_sort_order (H), test_bit_exact_vs_oracle dragon_96_bare (B); compact
//     alone -- test_fused_shading_equals_scan_scatter (H); neither -- test_bit_exact_vs_oracle dragon_64_nocompact
//     (H); sort alone -- test_brute_force_bit_exact_vs_oracle sphere_48_brute_nocompact (H); B, those three --
//     test_geom_render_equals_oracle ("shade_fused" 0 and compaction 0 with short_stack 0, iterations 1 and 2)
//   k_shade_fused_b: STAGE -- every default render (H), dragon_96_bare (B); not STAGE (a scene of more than
//     ORDERED_GEOMS geoms or STAGE_MATS materials) -- test_geom_render_equals_oracle nine, mats33, mats64 (H and B);
//     k_shade_fused: H + STAGE -- test_tuning_knobs_keep_parity "shade_batch"; the other three --
//     test_geom_render_equals_oracle "shade_batch" 0 (tilted, nested, glass: STAGE; nine, mats33, mats64: not)
//   k_brute: count on -- test_brute_force_counters_match_oracle (use_bbox 0, 1); off --
//     test_brute_force_bit_exact_vs_oracle (both); k_cast_resolve: H and B -- test_cast_equals_oracle
//   k_adapt_geoms_b: every case of tests/test_gpu_adaptive.py but one; k_adapt_rays_b: its brute_sphere case
//     (enable_kd = 0); k_adapt_flags: false -- the same tests, true -- test_selftest_active_list_equals_numpy
struct TraceKernel {
  void (*fn)(TraceArgs);
  int block;
};
template <bool H, bool C, int M>
constexpr TraceKernel trace_variant() {
  return {k_trace<H, C, M>, trace_block<M>()};
}
#define TRACE_MODES(H, C)                                                                                         \
  {trace_variant<H, C, TREE_WIDE>(),  trace_variant<H, C, TREE_PACKED>(), trace_variant<H, C, TREE_LDS>(),        \
   trace_variant<H, C, TREE_LDS16>(), trace_variant<H, C, TREE_LDS16G>(), trace_variant<H, C, TREE_LDS16S>()}
// (mode: a TreeMode, the enum's values in order)
TraceKernel trace_kernel(bool hybrid, bool count, int mode) {
  static const TraceKernel table[2][2][6] = {{TRACE_MODES(false, false), TRACE_MODES(false, true)},
                                             {TRACE_MODES(true, false), TRACE_MODES(true, true)}};
  return table[hybrid][count][mode];
}
#undef TRACE_MODES

// The shading kernels compute the hit point with the offset of the traversal that found it: 1e-4 for the hybrid
// walk and the brute-force kernel, 1e-5 for traverseKDbare.
bool hybrid_shading(const kdpt_ctx* c) { return c->opt.short_stack || c->brute; }

using ShadeKernel = void (*)(ShadeArgs);
ShadeKernel shade_kernel(bool hybrid, bool compact, bool sort) {
  static const ShadeKernel table[2][2][2] = {{{k_shade<false, false, false>, k_shade<false, false, true>},
                                              {k_shade<false, true, false>, k_shade<false, true, true>}},
                                             {{k_shade<true, false, false>, k_shade<true, false, true>},
                                              {k_shade<true, true, false>, k_shade<true, true, true>}}};
  return table[hybrid][compact][sort];
}
// stage: the scene's geoms and materials fit the fused kernels' LDS copy
using FusedKernel = void (*)(ShadeArgs, FuseArgs);
FusedKernel shade_fused_kernel(bool hybrid, bool stage) {
  static const FusedKernel table[2][2] = {{k_shade_fused<false, false>, k_shade_fused<false, true>},
                                          {k_shade_fused<true, false>, k_shade_fused<true, true>}};
  return table[hybrid][stage];
}
using FusedBatchKernel = void (*)(ShadeBatch);
FusedBatchKernel shade_fused_batch_kernel(bool hybrid, bool stage) {
  static const FusedBatchKernel table[2][2] = {{k_shade_fused_b<false, false>, k_shade_fused_b<false, true>},
                                               {k_shade_fused_b<true, false>, k_shade_fused_b<true, true>}};
  return table[hybrid][stage];
}
// the fused kernels' STAGE argument: the scene's geoms and materials fit their LDS copy
bool shade_staged(const kdpt_ctx* c) {
  return c->S.num_geoms + c->S.num_boxes <= ORDERED_GEOMS && c->S.num_materials <= STAGE_MATS;
}
using BruteKernel = void (*)(BruteArgs);
BruteKernel brute_kernel(bool use_bbox, bool count) {
  static const BruteKernel table[2][2] = {{k_brute<false, false>, k_brute<false, true>},
                                          {k_brute<true, false>, k_brute<true, true>}};
  return table[use_bbox][count];
}

// The workgroups of the route's intersect kernel that fit a CU with `lds` bytes of tree: the fewest over the
// four (hybrid, count) variants, so that one grid serves whichever of them a launch picks.
int trace_blocks_per_cu(int mode, size_t lds, int* blocks) {
  int best = 0;
  for (int hyb = 0; hyb < 2; hyb++)
    for (int cnt = 0; cnt < 2; cnt++) {
      const TraceKernel k = trace_kernel(hyb, cnt, mode);
      int b = 0;
      if (lds > 0)
        HIP_TRY(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k.fn, k.block, lds));
      if (best == 0 || b < best) best = b;
    }
  *blocks = best;
  return KDPT_OK;
}

// Pick where the intersect kernel reads the tree from, and its persistent grid: in LDS when it fits (the
// "tree_format" knob limits the LDS records to one size) -- the candidate that keeps the most intersect waves
// on a CU wins, ties in the order below.
int setup_trace(kdpt_ctx* c) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, c->device));
  const size_t lds_max = prop.sharedMemPerBlock > 0 ? prop.sharedMemPerBlock : 65536;
  // (the counting kernel's per-wave WaveProf too: the tree must fit next to either kernel's static part)
  const size_t per_wave = sizeof(WaveLeafLDS) + sizeof(WaveProf);
  const size_t cl_bytes = 32 * (size_t)c->S.num_clusters;
  struct Cand { int mode; size_t lds; };
  std::vector<Cand> cands;
  // (in order of preference at equal occupancy: the 32-byte records need no box bookkeeping on the walk, which
  // costs the derived form 6 % on dragon_5; the derived form is what fits the C5 icosphere's tree)
  if (!c->force_global_tree) {
    if (c->S.pnodes && c->tree_format != 16) {
      const size_t t32 = 32 * (size_t)c->S.num_nodes + cl_bytes, st32 = per_wave * (TRACE_BLOCK / 64);
      if (st32 + t32 <= lds_max) cands.push_back({TREE_LDS, t32});
    }
    if (c->S.dnodes && c->tree_format != 32) {
      const size_t t16 = 16 * (size_t)c->S.num_nodes, st16 = per_wave * (TRACE_BLOCK16 / 64);
      if (st16 + t16 + cl_bytes <= lds_max) cands.push_back({TREE_LDS16, t16 + cl_bytes});
      // (leaving room for a fused-shading workgroup's LDS beside the intersect workgroup)
      const size_t sp_bytes = 16 * (size_t)c->S.num_supers;
      // (not when the one-level cull is the masked exact one: the supers' margins are not rigorous for it)
      if (c->S.snodes && c->super_cull && !c->S.cl_mask && st16 + t16 + sp_bytes + SHADE_LDS_RESERVE <= lds_max)
        cands.push_back({TREE_LDS16S, t16 + sp_bytes});
      if (st16 + t16 <= lds_max) cands.push_back({TREE_LDS16G, t16});
    }
  }
  c->tree_mode = c->S.pnodes ? TREE_PACKED : TREE_WIDE;
  c->tree_lds = 0;
  int blocks = 0, best_waves = 0, rc = KDPT_OK;
  for (const Cand& k : cands) {
    int b = 0;
    if ((rc = trace_blocks_per_cu(k.mode, k.lds, &b))) return rc;
    const int waves = b * trace_kernel(false, false, k.mode).block / 64;
    if (b > 0 && waves > best_waves) {
      best_waves = waves;
      blocks = b;
      c->tree_mode = k.mode;
      c->tree_lds = k.lds;
    }
  }
  if (c->tree_lds == 0 && (rc = trace_blocks_per_cu(c->tree_mode, 0, &blocks))) return rc;
  if (blocks < 1) return fail(KDPT_ERR_UNSUPPORTED, "intersect kernel does not fit on a CU");
  c->trace_grid = blocks * prop.multiProcessorCount;
  c->full_trace_grid = c->trace_grid;
  return KDPT_OK;
}

// setup_trace again after a knob that can change the route; a "trace_grid_frac" share of the grid is kept.
int resetup_trace(kdpt_ctx* c) {
  const double frac = (double)c->trace_grid / std::max(1, c->full_trace_grid);
  int rc = setup_trace(c);
  if (rc) return rc;
  if (c->grid_env) c->trace_grid = std::max(1, (int)(c->full_trace_grid * frac));
  return KDPT_OK;
}

}  // namespace
