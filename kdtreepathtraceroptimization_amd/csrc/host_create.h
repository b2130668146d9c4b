// host_create.h -- kdpt_create (upload of what kdpt_scene_prep.h prepared), kdpt_set_options, the tuning knobs
// (kdpt_set_tuning), the cull margins and the masked cull's direction masks (build_masks).
//
// A host section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after host_variants.h.  Host code only: no kernel is defined here (the kernels_*.h sections hold them), and
// tests/test_stream_discipline.py and tests/test_resource_ownership.py read every host section.
#pragma once

namespace {

// The scene's cull margins (kdpt_clusters.h cluster_margin) into the context and its DevScene; fixed: one
// direction-free coefficient for every level (tuning "cull_margin" / "cluster_cull" = 0, which passes inf).
void set_cull(kdpt_ctx* c, const CullMargin& cm) {
  c->cull = cm;
  c->S.cl_margin = cm.K;
  c->S.cl_margin_lo = cm.K_lo;
  c->S.cull_a = cm.a;
  c->S.cull_b = cm.b;
  c->S.cull_c = cm.c;
}
void fix_cull(kdpt_ctx* c, float K) {
  c->S.cl_margin = c->S.cl_margin_lo = K;
}
// The one-level route's cull: the exact masked one when the scene has masks and the knobs leave the scene's
// margins in place, else the margin-only cull.
void apply_cull_route(kdpt_ctx* c) {
  c->S.cl_mask = (c->cull_exact && c->cull_scene) ? c->masks.dev.get() : nullptr;
  c->S.mask_n = c->masks.n;
  c->S.cl_tn = c->masks.tn.get();
}

// The direction masks of the scene's clusters at resolution n (cube-map cells per face edge), built on the device (k_build_masks) from the per-entry records and the bucket directions the host
// computes (kdpt_clusters.h mask_entries / mask_buckets; tests/test_gpu_parity.py checks the cells against the
// host builder).  A rebuild (knobs "cull_mask_n", "cull_fast_k") frees the previous table once the new one is
// filled; a failed one changes nothing in the context.
int build_masks(kdpt_ctx* c, int n) {
  const auto t0 = std::chrono::steady_clock::now();
  const ClusterSet& cs = *c->masks.cs;
  const int ncl = (int)cs.info.size(), nb = 6 * n * n;
  // the intersect kernel indexes the table with 32 bits (kdpt_trace_phase.h, S.cl_mask[bucket * num_clusters + c]): a
  // resolution whose table has 2^32 cells or more is refused here, before anything is freed or allocated
  if (n < 1 || (unsigned long long)nb * (unsigned long long)ncl >= (1ull << 32))
    return fail(KDPT_ERR_ARG, "direction masks: 6 n^2 num_clusters must be below 2^32 (n = " + std::to_string(n) +
                                  ", " + std::to_string(ncl) + " clusters: n <= " +
                                  std::to_string((int)std::sqrt((double)((1ull << 32) - 1) / (6.0 * std::max(1, ncl)))) +
                                  ")");
  const float Kf = c->cull.K;
  MaskEntries me;
  mask_entries(cs, Kf, me);
  std::vector<double> bd;
  mask_buckets(n, bd);
  const size_t ne = 64 * (size_t)ncl;
  std::vector<double> ent(5 * ne);
  for (size_t k = 0; k < ne; k++) {
    ent[k] = me.nx[k];
    ent[ne + k] = me.ny[k];
    ent[2 * ne + k] = me.nz[k];
    ent[3 * ne + k] = me.beta[k];
    ent[4 * ne + k] = me.dthr[k];
  }
  // The new table is the context's only once it is filled: until then masks.dev, masks.n and S.cl_mask keep
  // describing the previous one, which a failure below leaves in place.
  DeviceBuf<unsigned long long> dm;
  DeviceBuf<double> d_ent, d_bd;
  DeviceBuf<float> d_krig;
  // (the uploads on the context's stream, ahead of the kernel; pageable sources are staged before each call
  // returns, and the stream is drained before the temporaries go)
  hipError_t e;
  if ((e = dm.alloc((size_t)nb * ncl)) != hipSuccess || (e = d_ent.alloc(ent.size())) != hipSuccess ||
      (e = d_krig.alloc(me.krig.size())) != hipSuccess || (e = d_bd.alloc(bd.size())) != hipSuccess ||
      (e = hipMemcpyAsync(d_ent.get(), ent.data(), ent.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) !=
          hipSuccess ||
      (e = hipMemcpyAsync(d_krig.get(), me.krig.data(), me.krig.size() * sizeof(float), hipMemcpyHostToDevice,
                          c->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(d_bd.get(), bd.data(), bd.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) !=
          hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return hip_fail("mask build: device buffers", e);
  }
  hipLaunchKernelGGL(k_build_masks, dim3(ncl, (nb + 255) / 256), dim3(256), 0, c->stream, d_ent.get(), d_krig.get(),
                     d_bd.get(), ncl, nb, Kf, dm.get());
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  if (e1 != hipSuccess || e2 != hipSuccess) return hip_fail("k_build_masks", e1 != hipSuccess ? e1 : e2);
  if (!c->masks.tn) {
    std::vector<float4> tn;
    build_entry_normals(cs, tn);
    DeviceBuf<float4> d_tn;
    if ((e = d_tn.alloc(tn.size())) != hipSuccess) return hip_fail("hipMalloc", e);
    if (!tn.empty()) HIP_TRY(hipMemcpy(d_tn.get(), tn.data(), tn.size() * sizeof(float4), hipMemcpyHostToDevice));
    c->masks.tn = std::move(d_tn);
  }
  // the swap: the previous table is freed before the call returns (the stream was drained above)
  c->masks.dev = std::move(dm);
  c->masks.n = n;
  c->masks.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  apply_cull_route(c);
  return KDPT_OK;
}

// The "reduce_spin_us" knob of a context, or the process default of the contexts created later.
int set_reduce_spin(double* spin_us, double value) {
  if (!(value >= 0.0 && value <= 1e6)) return fail(KDPT_ERR_ARG, "reduce_spin_us must be in [0, 1e6]");
  *spin_us = value;
  return KDPT_OK;
}

}  // namespace

extern "C" {

void kdpt_default_options(kdpt_options* o) { default_options(o); }

int kdpt_create(const kdpt_scene* sc, const kdpt_options* opt, int device, kdpt_ctx** out) {
  const auto t_create = std::chrono::steady_clock::now();
  if (!sc || !out) return fail(KDPT_ERR_ARG, "null scene/out");
  *out = nullptr;
  // every argument and scene error is reported here, before any device work (kdpt_scene_prep.h)
  PreparedScene p;
  {
    std::string err;
    const int prc = prepare_scene(sc, opt, g_cluster_chord, &p, &err);
    if (prc) return fail(prc, err);
  }
  const kdpt_options& o = p.opt;
  std::unique_ptr<kdpt_ctx, int (*)(kdpt_ctx*)> owner(new kdpt_ctx(), kdpt_destroy);  // (gone at an early return)
  kdpt_ctx* const c = owner.get();
  c->shade_oob = p.shade_oob;
  c->device = device;
  c->opt = o;
  c->cam = sc->camera;
  c->traceDepth = sc->traceDepth;
  c->W = sc->camera.resolution[0];
  c->H = sc->camera.resolution[1];
  c->npix = c->W * c->H;
  c->ntiles = (c->npix + TILE - 1) / TILE;
  c->cap = o.bounce_cap;
  c->nkeys = std::max(1, sc->num_materials);
  int rc;
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return hip_fail("hipSetDevice", e);
  c->cu_mask_streams = g_cu_mask_streams;
  if ((rc = create_stream(c, &c->stream))) return rc;
  if ((e = c->pipe.entry_ev.create_untimed()) != hipSuccess) return hip_fail("hipEventCreateWithFlags", e);
  // the prepared arrays onto the device, straight into the DevScene fields that point at them
  auto up = [&](auto* field, const auto& v) { return dupload(c, field, v); };
  DevScene& S = c->S;
  if ((rc = up(&S.geoms, p.geoms)) || (rc = up(&S.materials, p.materials))) return rc;
  S.num_geoms = p.num_geoms;
  S.num_boxes = p.num_boxes;
  c->viz = p.viz;
  S.num_materials = sc->num_materials;
  S.has_obj = (p.kd || p.brute) ? 1 : 0;
  S.num_nodes = p.num_nodes;
  S.root = 0;
  S.n0_left = p.n0_left;
  S.n0_right = p.n0_right;
  S.n1_left = p.n1_left;
  S.n1_right = p.n1_right;
  S.rlo = p.rlo;
  S.rhi = p.rhi;
  S.gc = p.gc;
  S.gh = p.gh;
  set_cull(c, p.cull);
  if ((p.kd || p.brute) &&
      ((rc = up(&S.tv0, p.tri.tv0)) || (rc = up(&S.te1, p.tri.te1)) || (rc = up(&S.te2, p.tri.te2)) ||
       (rc = up(&S.tn0, p.tri.tn0)) || (rc = up(&S.tn1, p.tri.tn1)) || (rc = up(&S.tn2, p.tri.tn2))))
    return rc;
  if (p.kd) {
    const ClusterSet& cs = p.clusters;
    // (the packed, derived and super-cluster node records exist only where the tree is eligible: null otherwise)
    if ((rc = up(&S.nodes, p.nodes)) || (rc = up(&S.obj_material_offsets, p.obj_material_offsets)) ||
        (!p.pnodes.empty() && (rc = up(&S.pnodes, p.pnodes))) || (!p.dnodes.empty() && (rc = up(&S.dnodes, p.dnodes))) ||
        (!p.snodes.empty() && (rc = up(&S.snodes, p.snodes))) ||
        (rc = up(&S.leaf_cl, cs.leaf_cl)) || (rc = up(&S.cl_info, cs.info)) || (rc = up(&S.cl_lo, cs.lo)) ||
        (rc = up(&S.cl_hi, cs.hi)) || (rc = up(&S.c_v0, cs.cv0)) || (rc = up(&S.c_e1, cs.ce1)) ||
        (rc = up(&S.c_e2, cs.ce2)) || (rc = up(&S.sup, cs.sup)) || (rc = up(&S.cl_n, cs.nrm)) ||
        (rc = up(&S.cl_u, cs.obb_u)) || (rc = up(&S.cl_v, cs.obb_v)) || (rc = up(&S.cl_w, cs.obb_w)) ||
        (rc = up(&S.sup_n, cs.sup_n)) || (rc = up(&S.sup_b, cs.sup_b)))
      return rc;
    S.num_clusters = (int)cs.info.size();
    S.cl_counts = p.cl_counts;
    S.num_supers = p.num_supers;
    S.cl_slab = 1;
    S.cl_obb = 1;
    S.flat_obb = 1;
    S.sup_slab = 1;
    // the masked one-level cull's direction masks, for the fast margin the box levels use
    if (p.wants_masks) {
      c->masks.cs.reset(new ClusterSet(std::move(p.clusters)));
      if ((rc = build_masks(c, dir_mask_resolution(S.num_clusters)))) return rc;
    }
  } else if (p.brute) {
    if ((rc = up(&c->bf.shapes, p.shapes)) || (rc = up(&c->bf.chunk_lo, p.chunk_lo)) ||
        (rc = up(&c->bf.chunk_hi, p.chunk_hi)))
      return rc;
    c->bf.num_shapes = (int)p.shapes.size();
    c->brute = true;
    c->bf.chunk_k_min = HUGE_VALF;
    for (const float4& q : p.chunk_lo) c->bf.chunk_k_min = std::min(c->bf.chunk_k_min, q.w);
  }
  if (o.external_image) {
    c->image = o.external_image;  // (the caller's: not owned)
  } else if ((rc = dalloc(c, &c->image, 3 * (size_t)c->npix))) {
    return rc;
  }
  if ((rc = dalloc(c, &c->counters, 1)) || (rc = dalloc(c, &c->total_segments, 1)) ||
      (rc = dalloc(c, &c->trace_total, 3)))
    return rc;
  if ((rc = alloc_iter(c, &c->solo, c->stream, false))) return rc;
  // (the one-at-a-time launches and the ray queries report into the solo state's fault word; a pipelined
  // launch gets its own states' words, launch_batch)
  c->S.fault = c->solo.fault;
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0)
      c->wall_khz = khz;
  }
  // The product reads no environment variables: every route is the tested default unless a caller
  // changes it explicitly with kdpt_set_tuning (A/B experiments, the three-kernel compaction test).
  c->S.trace_mode = 0;
  // leave the node phase early once at most early_walk lanes still walk and at least early_leaf wait on a
  // leaf (the walkers resume after the leaf phase; first A/B at 32 / 24: 3 390 -> 3 540 Mrays/s; 0 / 65 =
  // never)
  // re-swept after the flattened leaf phase made leaf phases cheaper (32 / 24 before: 4 505-4 530 -> 4 659-4 704
  // Mrays/s, k_trace launch 0.85 -> 0.80 ms), and again with round 5's exact cull (24 -> 16: C3 5 747-5 756 ->
  // 5 798-5 802, C5 4 487 -> 4 544; 8 / 12 / 20 / 32 below 16, early_leaf 8 / 24 neutral; profiles/r05_ab_log.md)
  c->S.early_walk = 16;
  c->S.early_leaf = 1;
  if ((rc = setup_trace(c))) return rc;
  c->S.trip_limit = 8 * std::max(c->S.num_nodes, 1) + 64;
  // the scene's uploads (hipMemcpy) complete before any kernel of the context's non-blocking streams
  if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail("hipDeviceSynchronize", e);
  if ((rc = kdpt_reset(c))) return rc;
  c->frames.reduce_spin_us = g_reduce_spin_us;
  c->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create).count();
  *out = owner.release();
  return KDPT_OK;
}

int kdpt_set_options(kdpt_ctx* c, const kdpt_options* o) {
  if (!c || !o) return fail(KDPT_ERR_ARG, "null arg");
  const kdpt_options& p = c->opt;
  // these select what is uploaded or how much is allocated: a new context is needed
  if (o->enable_kd != p.enable_kd || o->viz_kd != p.viz_kd || o->use_bbox != p.use_bbox ||
      (o->bounce_cap > 0 ? o->bounce_cap : 8) != c->cap || o->block_size != p.block_size ||
      o->external_image != p.external_image)
    return fail(KDPT_ERR_UNSUPPORTED, "enable_kd, viz_kd, use_bbox, bounce_cap, block_size and external_image "
                                      "are fixed at kdpt_create");
  HIP_TRY(hipSetDevice(c->device));
  if (!c->pipe.groups.empty()) {  // iterations in flight keep the options they were enqueued with
    int rc = kdpt_synchronize(c);
    if (rc) return rc;
  }
  kdpt_options& d = c->opt;
  d.focal_length = o->focal_length;
  d.dof_angle = o->dof_angle;
  d.softness = o->softness;
  d.cacherays = o->cacherays;
  d.antialias = o->antialias;
  d.enable_sss = o->enable_sss;
  d.testing_mode = o->testing_mode;
  d.compaction = o->compaction;
  d.short_stack = o->short_stack;
  return KDPT_OK;
}

int kdpt_set_tuning(kdpt_ctx* c, const char* name, double value) {
  const std::string k(name ? name : "");
  if (!c && k == "reduce_spin_us") return set_reduce_spin(&g_reduce_spin_us, value);  // of contexts created later
  if (!c && k == "cu_mask_streams") {  // ... the kind of their batch / reduce streams
    g_cu_mask_streams = value != 0.0;
    return KDPT_OK;
  }
  if (!c && k == "cluster_chord") {  // ... and their big-leaf cluster grouping
    if (!(value >= -1.0 && value <= 4.0)) return fail(KDPT_ERR_ARG, "cluster_chord must be in [-1, 4]");
    g_cluster_chord = value;
    return KDPT_OK;
  }
  if (!name) return fail(KDPT_ERR_ARG, "kdpt_set_tuning: null name");
  if (!c) return fail(KDPT_ERR_ARG, "kdpt_set_tuning: null ctx, and no process-wide tuning knob is called " + k);
  if (k == "cast_chunk") {  // kdpt_cast_rays' chunk; its buffers are remade by the next call
    if (!(value >= 64.0 && value <= (double)(1 << 26))) return fail(KDPT_ERR_ARG, "cast_chunk must be in 64 .. 2^26");
    c->cast.chunk = (int)value;
    return KDPT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  c->den.b = {};  // kdpt_denoise's buffers (nothing is queued on them): its next call remakes them
  c->tmp.s = {};  // ... and kdpt_denoise_temporal's history with them
  // queued iterations finish first: setup_trace and build_masks free and reallocate device memory their
  // kernels read.  The pipeline's states hold no knobs; they are still dropped, as include/kdpt.h documents
  // (the next kdpt_trace_iterations remakes them).
  if (!c->pipe.groups.empty()) {
    int rc = kdpt_synchronize(c);
    if (rc) return rc;
    c->pipe.drop_groups();
  }
  const int v = (int)value;
  bool route = false;  // the knob can change the intersect kernel's route: setup_trace again
  bool cull = false;   // ... and before that, which one-level cull it runs
  if (k == "shade_fused") {
    c->no_fuse = v == 0;
  } else if (k == "early_walk") {
    c->S.early_walk = v;
  } else if (k == "early_leaf") {
    c->S.early_leaf = v;
  } else if (k == "shade_batch") {
    c->shade_batch = v != 0;
  } else if (k == "gen_geoms") {
    c->gen_geoms = v != 0;
  } else if (k == "chunk_width0" || k == "chunk_width1" || k == "chunk_width2") {
    c->chunk_width[k.back() - '0'] = std::min(64, std::max(1, v));
  } else if (k == "trace_grid_frac") {
    if (!(value > 0.0 && value <= 1.0)) return fail(KDPT_ERR_ARG, "trace_grid_frac must be in (0, 1]");
    c->trace_grid = std::max(1, (int)(c->full_trace_grid * value));
    c->grid_env = value < 1.0;
  } else if (k == "cluster_obb") {
    c->S.cl_obb = v != 0;
  } else if (k == "flat_obb") {
    c->S.flat_obb = v != 0;
  } else if (k == "super_slab") {
    c->S.sup_slab = v != 0;
  } else if (k == "cluster_slab") {
    c->S.cl_slab = v != 0;
  } else if (k == "tree_format") {
    if (v != 0 && v != 16 && v != 32) return fail(KDPT_ERR_ARG, "tree_format must be 0 (best), 16 or 32");
    c->tree_format = v;
    route = true;
  } else if (k == "super_cull") {
    c->super_cull = v != 0;
    route = true;
  } else if (k == "tree_global") {
    c->force_global_tree = v != 0;
    route = true;
  } else if (k == "cluster_cull") {
    // 0: no cluster / chunk cull at all (every big-leaf cluster swept: exact by construction, whatever the
    // scene's margin); 1: the scene's margins (and masks)
    c->cull_scene = v != 0;
    if (v != 0) set_cull(c, c->cull);
    else fix_cull(c, __builtin_inff());
    cull = true;
  } else if (k == "cull_margin") {
    // > 0: one fixed margin coefficient for every level (no masks: not exact in general); 0: the scene's
    if (!(value >= 0.0)) return fail(KDPT_ERR_ARG, "cull_margin must be >= 0 (0: the scene's)");
    c->cull_scene = value == 0.0;
    if (value > 0.0) fix_cull(c, (float)value);
    else set_cull(c, c->cull);
    cull = true;
  } else if (k == "cull_exact") {
    // 0: the fast-margin one-level cull instead of the masked exact one (A/B; not exact for such scenes)
    c->cull_exact = v != 0;
    cull = true;
  } else if (k == "cull_fast_k") {
    // the masked cull's box coefficient (default CULL_MARGIN_MASKED), its direction masks rebuilt for it: a
    // wider box sweeps more clusters, a narrower one leaves more danger triangles to decide
    if (!(value > 0.0 && value < 1.0)) return fail(KDPT_ERR_ARG, "cull_fast_k must be in (0, 1)");
    if (!c->masks.cs) return fail(KDPT_ERR_ARG, "cull_fast_k: this scene has no direction masks");
    const CullMargin before = c->cull;
    c->cull.K = c->cull.K_lo = (float)value;
    if (c->cull_scene) set_cull(c, c->cull);
    int rc = build_masks(c, c->masks.n);
    if (rc) {  // the masks are still the old coefficient's: so is the margin again
      c->cull = before;
      if (c->cull_scene) set_cull(c, before);
      return rc;
    }
    cull = true;
  } else if (k == "cull_mask_n") {
    if (v < 1 || v > 512) return fail(KDPT_ERR_ARG, "cull_mask_n must be in 1 .. 512");
    if (!c->masks.cs) return fail(KDPT_ERR_ARG, "cull_mask_n: this scene has no direction masks");
    int rc = build_masks(c, v);
    if (rc) return rc;
    cull = true;
  } else if (k == "profile_batches") {
    c->profile_batches = v != 0;
    c->profile_steps = v >= 2;
  } else if (k == "sync_debug") {
    c->sync_debug = v != 0;
  } else if (k == "reduce_spin_us") {
    return set_reduce_spin(&c->frames.reduce_spin_us, value);
  } else {
    return fail(KDPT_ERR_ARG, "unknown tuning knob " + k);
  }
  // (the route may change with the cull too: no super-cluster route under the masked cull)
  if (cull) apply_cull_route(c);
  return (cull || route) ? resetup_trace(c) : KDPT_OK;
}

}  // extern "C"
