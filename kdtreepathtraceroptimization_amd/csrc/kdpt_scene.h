// kdpt_scene.h -- the gfx950 data layout the kernels and the host walk read: materials, analytic geoms, the
// scene record (SoA float4 nodes / triangles, clusters, cull tables) and the ray.
#pragma once

#include "kdpt_math.h"

namespace kdpt {

// Per-material record, read by divergent lanes.
struct DevMaterial {
  float color[3];
  float spec_exponent;
  float spec_color[3];
  float hasReflective;
  float hasRefractive;
  float indexOfRefraction;
  float emittance;
  float transmittance[3];
  float fresnel_R0;  // glm::pow((1-ior)/(1+ior), 2.0f), precomputed (folds to r*r)
  float pad_[3];
};

struct DevGeom {
  int type;
  int materialid;
  int pad_[2];
  float transform[16];
  float inverseTransform[16];
  float invTranspose[16];
  // world-space bounds of the unit cube / sphere under `transform`, enlarged by a margin, and in wlo[3] the
  // Chebyshev distance from them within which a ray origin may rely on them (geom_may_hit, below)
  float wlo[4], whi[4];
};

struct DevScene {
  const DevGeom* geoms;
  int num_geoms;
  int num_boxes;  // viz_kd: the KD node boxes, stored after the analytic geoms in `geoms`
  const DevMaterial* materials;
  int num_materials;
  int has_obj;
  int num_nodes;
  int root;
  // nodes: 64-byte records [4*i .. 4*i+3] = {minx,miny,minz,maxx}, {maxy,maxz,left,right},
  // {parent,triStart,triSize,axis}, padding; held as integer words (floats as their bits) so
  // that no float move can canonicalise the -1 links
  const int4* nodes;
  const int4* pnodes;  // the same tree as 32-byte NodesPacked records, or null when ineligible
  const int4* dnodes;  // ... and as 16-byte NodesDerived records (boxes derived on the walk), or null
  // triangles: v0 (w = mtlIdx bits), e1 = v1-v0, e2 = v2-v0 (exactly glm's e1/e2)
  const float4* tv0;
  const float4* te1;
  const float4* te2;
  const float4* tn0;
  const float4* tn1;
  const float4* tn2;
  const int* obj_material_offsets;
  // children of nodes[0] and nodes[1] for the hybrid skip line (-1 when absent)
  int n0_left, n0_right, n1_left, n1_right;
  // big leaves (>= BIG_LEAF triangles) as clusters of <= 64 triangles in Morton order, each with its
  // box: leaf_cl[node] = {first cluster, count} (count 0: not big); cl_lo/cl_hi boxes; cl_info =
  // {first triangle, size}; cluster-order copies of v0/e1/e2 with the original index in e1.w, each
  // cluster padded to CLUSTER entries (cluster c = entries [CLUSTER c, CLUSTER (c + 1)); padding: zeros, index -1)
  const int2* leaf_cl;
  int num_clusters;
  // 1 when some big leaf has more clusters than ceil(size / CLUSTER) (normal-cone grouping: balanced runs per
  // cone), so the kernels read each leaf's count from leaf_cl instead of deriving it from the leaf's size
  int cl_counts;
  const float4* cl_lo;
  const float4* cl_hi;
  const int2* cl_info;
  // super-clusters: a big leaf's clusters in runs of SUPER (consecutive in Morton order), as 16-byte records:
  // the box in half precision rounded outward (lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16) and
  // first cluster << 5 | (count - 1); snodes = the NodesDerived records with a big leaf's first super instead
  // of its first cluster (TREE_LDS16S: records and supers in LDS, the two-level cull), or null
  const int4* sup;
  int num_supers;
  // per super-cluster: the unit normal of its triangles' summed area vectors and the largest chord to their
  // unit normals (sup_n = (n, chord)), and the slab [sup_b.x, sup_b.y] of n . (q - c) holding them (c: the
  // centre of the half-precision box); the first cull level tests survivors of the box against it with the
  // direction-dependent margin when sup_slab is set (knob "super_slab")
  const float4* sup_n;
  const float4* sup_b;
  int sup_slab;
  // per cluster: the unit normal of its triangles' summed area vectors (xyz); every point q of its triangles
  // has n . (q - c) in [cl_lo.w, cl_hi.w], c = 0.5f * (lo + hi) (bounds rounded outward); n = 0: no slab.
  // The two-level cull tests the line against this slab as well as the box (knob "cluster_slab")
  const float4* cl_n;
  int cl_slab;
  // ... and the patch's extent along two unit directions u, v in its plane (u: the principal axis of its
  // vertices projected on the plane, v = n x u): cl_u = (u, min u.(q - c)), cl_v = (v, min v.(q - c)),
  // cl_w = (max u.(q - c), max v.(q - c), -, -), bounds rounded outward; with the slab an oriented box the
  // second cull level tests when cl_obb is set (knob "cluster_obb")
  const float4* cl_u;
  const float4* cl_v;
  const float4* cl_w;
  int cl_obb;
  // the one-level route (TREE_LDS / LDS16 / LDS16G...) also tests its box survivors against the cluster's
  // oriented box from HBM (knob "flat_obb")
  int flat_obb;
  // the cull's margin coefficients (kdpt_clusters.h cluster_margin): cl_margin for the box-only tests;
  // the slab level uses cull_margin_dir(): max(cl_margin_lo, min(cl_margin, cull_a / g + cull_c)),
  // g = |n . d| - cl_n.w - cull_b
  float cl_margin, cl_margin_lo, cull_a, cull_b, cull_c;
  // the exact one-level cull (kdpt_clusters.h build_dir_masks): per cluster c and direction bucket b,
  // cl_mask[b * num_clusters + c] = the danger mask over the cluster's 64 entries (bucket-major: a ray's
  // pairs, consecutive clusters of one leaf in one bucket, share cache lines); null: the fast-margin cull
  // (tuning "cull_exact" = 0) or no one-level cull at all
  const unsigned long long* cl_mask;  // [6 mask_n^2][num_clusters] danger masks
  int mask_n;                          // cube-map cells per face edge (dir_bucket)
  // per cluster entry: the triangle's unit normal (float) and 17.5 u rho (the exact cull's per-triangle
  // bound); w = -1: never passes (padding, small degenerate), w = +inf: may pass for any direction
  const float4* cl_tn;
  const int4* snodes;
  const float4* c_v0;
  const float4* c_e1;
  const float4* c_e2;
  float4 rlo, rhi;  // the KD root's box: prep_ray's first traversal step, the derived boxes' start
  // the ray origins for which every analytic geom's bounds hold (geoms_hold_for): the box of centre gc and
  // half-sizes gh; a negative half-size: none
  float4 gc, gh;
  int trace_mode;   // 1 class+octant, 2 octant, 3 class (experiments)
  int early_walk, early_leaf;  // leaf phase starts when <= early_walk lanes walk and >= early_leaf wait
  int trip_limit;  // bound on node steps per ray (a valid tree needs < 4 per node)
  int* fault;      // set to 1 when a ray exceeds trip_limit (never for a validated tree)
};

struct Ray {
  f3 origin, direction;
  bool isinside;
  float sdepth;
};

}  // namespace kdpt
