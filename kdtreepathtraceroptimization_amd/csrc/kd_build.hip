// kd_build.hip -- the reference's host KD-tree build (Scene::loadObj's KD section, src/scene.cpp:866-968:
// KDtree(triangles) -> rootNode->updateBbox() -> split(13) -> cacheTriangles_ / cacheNodesBare) on the GPU,
// byte-identical to it (and to csrc/scene_host.cpp's host restatement).
//
// The reference builds depth-first and numbers nodes in pre-order (a file-static counter incremented as
// each child is created, left subtree before right).  Here the tree is built level by level, breadth first,
// with one pass over all (node, triangle) pairs of a level per kernel:
//   k_side      per pair: does the triangle go left (mins[axis] < centre + 0.0001) / right
//               (maxs[axis] >= centre - 0.0001)?  (KDnode.cpp:177-186, the comparisons in double)
//   scans       of the two flags over the level's pairs (pairs are grouped by node, in the node's
//               triangle order, so a node's side counts are differences of the scans)
//   k_decide    per node: split when it has > 2 triangles, its level <= maxdepth and neither side takes
//               every triangle (KDnode.cpp:160-193); else it is a leaf and keeps its triangles
//   scans       of the per-node split flags / children's pair counts / leaf sizes
//   k_children  per split node: both children (box = the parent's with maxs[axis] (left) or mins[axis]
//               (right) set to the parent's centre, centre recomputed, splitPos, axis; KDnode.cpp:195-246)
//   k_scatter   per pair: into the left and/or right child's pair list, STABLY (the reference's
//               leftSide/rightSide keep the parent's order), or into the leaf store
// After the last level, subtree sizes (bottom-up) give every node its pre-order ID (ID(left) = ID + 1,
// ID(right) = ID + 1 + size(left)), the leaves' triangle lists are laid out in ID order (cacheTriangles_,
// src/scene.cpp:409-459; duplicates included) and NodeBare[] is written in ID order (cacheNodesBare,
// :905-932).  The root box (KDnode::updateBbox, KDnode.cpp:112-149) is a first-occurrence min/max over the
// triangles' bounds -- the reference's `a > b ? b : a` fold keeps the earliest of equal values (+0 / -0)
// -- plus the 0.001 pad, which does not refresh the centre.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kdpt.h"
#include "kd_build.h"
#define KDPT_HIP_STAGE "device KD build: "  // what this file's HIP_TRY messages begin with
#include "kdpt_error.h"
#include "kdpt_owned.h"

namespace {

using kdpt::Arena;
using kdpt::DeviceBuf;

constexpr int BLK = 256;
inline int blocks(long long n) { return (int)std::max(1ll, (n + BLK - 1) / BLK); }

// Triangle::computeBounds (KDnode.h:216-225): the nested ternaries, component by component
__device__ inline float tmin3(float a, float b, float c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
__device__ inline float tmax3(float a, float b, float c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

__global__ void k_tri_bounds(const float* __restrict__ v9, int n, float4* __restrict__ lo, float4* __restrict__ hi) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  const float* v = v9 + 9 * (size_t)i;  // x1 y1 z1 x2 y2 z2 x3 y3 z3
  lo[i] = make_float4(tmin3(v[0], v[3], v[6]), tmin3(v[1], v[4], v[7]), tmin3(v[2], v[5], v[8]), 0.0f);
  hi[i] = make_float4(tmax3(v[0], v[3], v[6]), tmax3(v[1], v[4], v[7]), tmax3(v[2], v[5], v[8]), 0.0f);
}

// Order-preserving 32-bit key of a float with +0 and -0 equal (they compare equal in the reference's fold).
__device__ inline uint32_t fkey(float f) {
  uint32_t u = __float_as_uint(f);
  if (f == 0.0f) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Root box: per component the FIRST triangle (in order) holding the minimum (maximum): min over
// (key << 32 | index) resp. max over (key << 32 | ~index).  NaNs never win (the fold's comparisons are
// false for them) unless triangle 0 holds one, which the host handles.
__global__ void k_root_keys(const float4* __restrict__ lo, const float4* __restrict__ hi, int n,
                            unsigned long long* keys) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  unsigned long long kmin[3] = {~0ull, ~0ull, ~0ull}, kmax[3] = {0ull, 0ull, 0ull};
  if (i < n) {
    const float4 a = lo[i], b = hi[i];
    const float la[3] = {a.x, a.y, a.z}, hb[3] = {b.x, b.y, b.z};
    for (int c = 0; c < 3; c++) {
      if (la[c] == la[c]) kmin[c] = ((unsigned long long)fkey(la[c]) << 32) | (uint32_t)i;
      if (hb[c] == hb[c]) kmax[c] = ((unsigned long long)fkey(hb[c]) << 32) | (uint32_t)~(uint32_t)i;
    }
  }
  for (int c = 0; c < 3; c++) {
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long om = __shfl_xor(kmin[c], off), ox = __shfl_xor(kmax[c], off);
      kmin[c] = om < kmin[c] ? om : kmin[c];
      kmax[c] = ox > kmax[c] ? ox : kmax[c];
    }
  }
  if ((threadIdx.x & 63) == 0) {
    for (int c = 0; c < 3; c++) {
      atomicMin(&keys[c], kmin[c]);
      atomicMax(&keys[3 + c], kmax[c]);
    }
  }
}

struct LevelArgs {
  int level, ax, maxdepth;
  int lvl_begin, nlvl;  // this level's nodes: global BFS indices [lvl_begin, lvl_begin + nlvl)
  long long npairs;
};

// Node store (global BFS index): box, centre, links, build results.
struct Nodes {
  float4 *lo, *hi, *ctr;   // box mins / maxs / centre (w unused)
  int* parent;
  int* left;
  int* right;
  int* axis;
  float* split_pos;
  int* pstart;             // this node's pair range in the level's pair list (its level only)
  int* pcnt;
  int* leaf_start;         // leaves: range in the leaf store; -1 for split nodes
  int* leaf_cnt;
  int* size;               // subtree size (nodes)
  int* id;                 // pre-order ID
};

__global__ void k_side(LevelArgs L, const int* __restrict__ ptri, const int* __restrict__ pnode, Nodes N,
                       const float4* __restrict__ tlo, const float4* __restrict__ thi, int* __restrict__ fl,
                       int* __restrict__ fr) {
  const long long p = (long long)blockIdx.x * BLK + threadIdx.x;
  if (p >= L.npairs) {
    if (p == L.npairs) fl[p] = fr[p] = 0;  // the scans' total slot
    return;
  }
  const int t = ptri[p], k = pnode[p];
  const float4 c4 = N.ctr[k], a = tlo[t], b = thi[t];
  const float c = L.ax == 0 ? c4.x : (L.ax == 1 ? c4.y : c4.z);
  const float mn = L.ax == 0 ? a.x : (L.ax == 1 ? a.y : a.z);
  const float mx = L.ax == 0 ? b.x : (L.ax == 1 ? b.y : b.z);
  fl[p] = ((double)mn < (double)c + 0.0001) ? 1 : 0;
  fr[p] = ((double)mx >= (double)c - 0.0001) ? 1 : 0;
}

__global__ void k_decide(LevelArgs L, Nodes N, const int* __restrict__ sl, const int* __restrict__ sr,
                         int* __restrict__ nsplit, int* __restrict__ npair_next, int* __restrict__ nleaf,
                         int* __restrict__ cl, int* __restrict__ cr) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= L.nlvl) {
    if (i == L.nlvl) nsplit[i] = npair_next[i] = nleaf[i] = 0;
    return;
  }
  const int k = L.lvl_begin + i;
  const int s = N.pstart[k], num = N.pcnt[k];
  const int l = sl[s + num] - sl[s], r = sr[s + num] - sr[s];
  const bool split = num > 2 && L.level <= L.maxdepth && l != num && r != num;
  nsplit[i] = split ? 1 : 0;
  npair_next[i] = split ? l + r : 0;
  nleaf[i] = split ? 0 : num;
  cl[i] = l;
  cr[i] = r;
}

__device__ inline void set_comp(float4& v, int ax, float x) {
  if (ax == 0) v.x = x; else if (ax == 1) v.y = x; else v.z = x;
}
__device__ inline float comp4(const float4& v, int ax) { return ax == 0 ? v.x : (ax == 1 ? v.y : v.z); }
// BoundingBox::updateCentroid (KDnode.h:279-285): (mins + maxs) in float, / 2.0 in double
__device__ inline float4 centroid(const float4& lo, const float4& hi) {
  return make_float4((float)((double)(lo.x + hi.x) / 2.0), (float)((double)(lo.y + hi.y) / 2.0),
                     (float)((double)(lo.z + hi.z) / 2.0), 0.0f);
}

__global__ void k_children(LevelArgs L, Nodes N, const int* __restrict__ nsplit_ex, const int* __restrict__ npair_ex,
                           const int* __restrict__ nleaf_ex, const int* __restrict__ nsplit_in,
                           const int* __restrict__ cl, const int* __restrict__ cr, int leaf_base) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= L.nlvl) return;
  const int k = L.lvl_begin + i;
  if (!nsplit_in[i]) {  // a leaf: keeps its triangles (triIdStart / triIdSize are set when laid out)
    N.left[k] = N.right[k] = -1;
    N.leaf_start[k] = leaf_base + nleaf_ex[i];
    N.leaf_cnt[k] = N.pcnt[k];
    return;
  }
  const int next_begin = L.lvl_begin + L.nlvl;
  const int lk = next_begin + 2 * nsplit_ex[i], rk = lk + 1;
  N.left[k] = lk;
  N.right[k] = rk;
  N.leaf_start[k] = -1;
  N.leaf_cnt[k] = 0;
  const float4 plo = N.lo[k], phi = N.hi[k], pc = N.ctr[k];
  const int ax = L.ax, cax = (ax + 1) % 3;
  {  // left: setBounds(parent) then maxs[axis] = parent centre; splitPos = parent maxs[axis]
    float4 lo = plo, hi = phi;
    set_comp(hi, ax, comp4(pc, ax));
    N.lo[lk] = lo;
    N.hi[lk] = hi;
    N.ctr[lk] = centroid(lo, hi);
    N.split_pos[lk] = comp4(phi, ax);
    N.axis[lk] = cax;
    N.parent[lk] = k;
    N.pstart[lk] = npair_ex[i];
    N.pcnt[lk] = cl[i];
  }
  {  // right: mins[axis] = parent centre; splitPos = parent mins[axis]
    float4 lo = plo, hi = phi;
    set_comp(lo, ax, comp4(pc, ax));
    N.lo[rk] = lo;
    N.hi[rk] = hi;
    N.ctr[rk] = centroid(lo, hi);
    N.split_pos[rk] = comp4(plo, ax);
    N.axis[rk] = cax;
    N.parent[rk] = k;
    N.pstart[rk] = npair_ex[i] + cl[i];
    N.pcnt[rk] = cr[i];
  }
}

__global__ void k_scatter(LevelArgs L, Nodes N, const int* __restrict__ ptri, const int* __restrict__ pnode,
                          const int* __restrict__ fl, const int* __restrict__ fr, const int* __restrict__ sl,
                          const int* __restrict__ sr, const int* __restrict__ nsplit_in, int* __restrict__ ntri,
                          int* __restrict__ nnode, int* __restrict__ leaf_tri, int* __restrict__ leaf_node) {
  const long long p = (long long)blockIdx.x * BLK + threadIdx.x;
  if (p >= L.npairs) return;
  const int t = ptri[p], k = pnode[p], i = k - L.lvl_begin;
  const int s = N.pstart[k];
  if (nsplit_in[i]) {
    const int lk = N.left[k], rk = N.right[k];
    if (fl[p]) {
      const int q = N.pstart[lk] + (sl[p] - sl[s]);
      ntri[q] = t;
      nnode[q] = lk;
    }
    if (fr[p]) {
      const int q = N.pstart[rk] + (sr[p] - sr[s]);
      ntri[q] = t;
      nnode[q] = rk;
    }
  } else {
    const int q = N.leaf_start[k] + (int)(p - s);
    leaf_tri[q] = t;
    leaf_node[q] = k;
  }
}

__global__ void k_sizes(Nodes N, int begin, int count) {  // one level, deepest first
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= count) return;
  const int k = begin + i;
  const int l = N.left[k], r = N.right[k];
  N.size[k] = 1 + (l >= 0 ? N.size[l] : 0) + (r >= 0 ? N.size[r] : 0);
}

__global__ void k_ids(Nodes N, int begin, int count) {  // one level, root first; ID[root] set before
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i >= count) return;
  const int k = begin + i;
  const int l = N.left[k], r = N.right[k];
  if (l >= 0) N.id[l] = N.id[k] + 1;
  if (r >= 0) N.id[r] = N.id[k] + 1 + (l >= 0 ? N.size[l] : 0);
}

__global__ void k_leaf_sizes_by_id(Nodes N, int nnodes, int* __restrict__ by_id) {
  const int k = blockIdx.x * BLK + threadIdx.x;
  if (k > nnodes) return;
  if (k == nnodes) {
    by_id[k] = 0;
    return;
  }
  by_id[N.id[k]] = N.leaf_cnt[k];
}

__global__ void k_write_nodes(Nodes N, int nnodes, const int* __restrict__ tstart_by_id,
                              kdpt_node_bare* __restrict__ out) {
  const int k = blockIdx.x * BLK + threadIdx.x;
  if (k >= nnodes) return;
  const int id = N.id[k];
  kdpt_node_bare o;
  o.axis = N.axis[k];
  o.splitPos = N.split_pos[k];
  const float4 lo = N.lo[k], hi = N.hi[k];
  o.mins[0] = lo.x; o.mins[1] = lo.y; o.mins[2] = lo.z;
  o.maxs[0] = hi.x; o.maxs[1] = hi.y; o.maxs[2] = hi.z;
  o.ID = id;
  o.parentID = N.parent[k] >= 0 ? N.id[N.parent[k]] : -1;
  o.leftID = N.left[k] >= 0 ? N.id[N.left[k]] : -1;
  o.rightID = N.right[k] >= 0 ? N.id[N.right[k]] : -1;
  const int cnt = N.leaf_cnt[k];
  o.triIdStart = cnt > 0 ? tstart_by_id[id] : -1;
  o.triIdSize = cnt > 0 ? cnt : -1;
  o.tmin = 0.0f;
  o.tmax = 0.0f;
  out[id] = o;
}

__global__ void k_write_tris(Nodes N, long long nleafpairs, const int* __restrict__ leaf_tri,
                             const int* __restrict__ leaf_node, const int* __restrict__ tstart_by_id,
                             const float* __restrict__ v9, const float* __restrict__ n9, const int* __restrict__ mtl,
                             kdpt_tri_bare* __restrict__ out) {
  const long long q = (long long)blockIdx.x * BLK + threadIdx.x;
  if (q >= nleafpairs) return;
  const int k = leaf_node[q], t = leaf_tri[q];
  const int pos = tstart_by_id[N.id[k]] + (int)(q - N.leaf_start[k]);
  const float* v = v9 + 9 * (size_t)t;
  const float* n = n9 + 9 * (size_t)t;
  kdpt_tri_bare o;
  o.x1 = v[0]; o.y1 = v[1]; o.z1 = v[2];
  o.x2 = v[3]; o.y2 = v[4]; o.z2 = v[5];
  o.x3 = v[6]; o.y3 = v[7]; o.z3 = v[8];
  o.nx1 = n[0]; o.ny1 = n[1]; o.nz1 = n[2];
  o.nx2 = n[3]; o.ny2 = n[4]; o.nz2 = n[5];
  o.nx3 = n[6]; o.ny3 = n[7]; o.nz3 = n[8];
  o.mtlIdx = mtl[t];
  out[pos] = o;
}

__global__ void k_iota(int* a, int n) {
  const int i = blockIdx.x * BLK + threadIdx.x;
  if (i < n) a[i] = i;
}

// ---------------------------------------------------------------- host side
// Helpers that wrap HIP calls return hipError_t and are called under HIP_TRY, whose message names the call;
// the stages of the build return the library's int status.

// (An Arena, kdpt_owned.h, owns what lives as long as the build; the stores that grow own theirs: BufferGroup.)
struct Scanner {
  void* tmp = nullptr;
  size_t bytes = 0;
  hipStream_t st;
  Arena* arena;
  hipError_t exclusive(const int* in, int* out, long long n) {  // n items (the last one the total slot)
    size_t need = 0;
    hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, (int)n, st);
    if (e != hipSuccess) return e;
    if (need > bytes) {
      if ((e = arena->alloc((char**)&tmp, need)) != hipSuccess) return e;
      bytes = need;
    }
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)n, st);
  }
};

// The device buffers sized by one capacity (cap + extra elements each).  A buffer is named once, where it is
// added; allocation and growth are loops over the list, so no buffer can be left at the old size.  The group owns
// the buffers; the build reads them through the pointers it named (`view`), which follow every reallocation.
struct BufferGroup {
  struct Buf {
    void** view;
    size_t elem;
    int extra;
    DeviceBuf<char> own;
    size_t bytes(long long cap) const { return (size_t)(cap + extra) * elem; }
  };
  long long cap = 0;
  std::vector<Buf> bufs;
  template <typename... T>
  void add(int extra, T**... p) {
    (bufs.push_back(Buf{(void**)p, sizeof(T), extra, {}}), ...);
  }
  hipError_t alloc_all(long long capacity) {
    cap = capacity;
    for (Buf& b : bufs) {
      if (hipError_t e = b.own.alloc(b.bytes(cap))) return e;
      *b.view = b.own.get();
    }
    return hipSuccess;
  }
  // Every buffer's contents move to a buffer of the new capacity.  Each old buffer is freed once its own copy
  // has run, so the peak device memory is the new capacity plus one old buffer, not the sum of every size.
  hipError_t grow(hipStream_t st, long long new_cap) {
    for (Buf& b : bufs) {
      DeviceBuf<char> q;
      hipError_t e = q.alloc(b.bytes(new_cap));
      if (e == hipSuccess) e = hipMemcpyAsync(q.get(), b.own.get(), b.bytes(cap), hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return e;
      b.own = std::move(q);
      *b.view = b.own.get();
    }
    cap = new_cap;
    return hipSuccess;
  }
};

// One build, handed from stage to stage.  The groups hold the addresses of its pointers: it is not copied.
struct Build {
  const float *v9, *n9;
  const int* mtl;
  const int ntri, maxdepth;
  const hipStream_t st;
  Arena& A;
  Scanner scan{nullptr, 0, st, &A};
  float *d_v9, *d_n9;  // the triangles and their bounds
  int* d_mtl;
  float4 *d_tlo, *d_thi;
  float4 rlo, rhi, rctr;  // the root's box and centre
  Nodes N{};
  int *cl, *cr, *nsplit, *npair, *nleaf, *nsplit_ex, *npair_ex, *nleaf_ex;  // a level's nodes: counts, scans
  int *ptri[2], *pnode[2];  // (triangle, node) pairs: level l's in [l & 1], the next level's in the other
  int *fl, *fr, *sl, *sr;             // a level's pairs: side flags and their scans
  int *leaf_tri, *leaf_node;          // leaf store
  BufferGroup nodes, pairs, leaves;
  std::vector<int> lvl_begin{0}, lvl_count{1};
  long long leaf_total = 0;
  int nnodes = 1;

  Build(const float* v9_, const float* n9_, const int* mtl_, int ntri_in, int maxdepth_, hipStream_t st_, Arena& A_)
      : v9(v9_), n9(n9_), mtl(mtl_), ntri(ntri_in), maxdepth(maxdepth_), st(st_), A(A_) {
    nodes.add(0, &N.lo, &N.hi, &N.ctr, &N.parent, &N.left, &N.right, &N.axis, &N.split_pos, &N.pstart, &N.pcnt,
              &N.leaf_start, &N.leaf_cnt, &N.size, &N.id, &cl, &cr);
    nodes.add(1, &nsplit, &npair, &nleaf, &nsplit_ex, &npair_ex, &nleaf_ex);  // scans: a total slot each
    pairs.add(0, &ptri[0], &pnode[0], &ptri[1], &pnode[1]);
    pairs.add(1, &fl, &fr, &sl, &sr);
    leaves.add(0, &leaf_tri, &leaf_node);
  }
  Build(const Build&) = delete;
};

int upload_stage(Build& B) {
  const size_t n = (size_t)B.ntri;
  HIP_TRY(B.A.alloc(&B.d_v9, 9 * n));
  HIP_TRY(B.A.alloc(&B.d_n9, 9 * n));
  HIP_TRY(B.A.alloc(&B.d_mtl, n));
  HIP_TRY(B.A.alloc(&B.d_tlo, n));
  HIP_TRY(B.A.alloc(&B.d_thi, n));
  HIP_TRY(hipMemcpyAsync(B.d_v9, B.v9, 36 * n, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(B.d_n9, B.n9, 36 * n, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(B.d_mtl, B.mtl, 4 * n, hipMemcpyHostToDevice, B.st));
  hipLaunchKernelGGL(k_tri_bounds, dim3(blocks(B.ntri)), dim3(BLK), 0, B.st, B.d_v9, B.ntri, B.d_tlo, B.d_thi);
  HIP_TRY(hipGetLastError());
  return KDPT_OK;
}

// Root box (KDnode::updateBbox): first-occurrence min / max, then the pad (centre not refreshed).
int root_box_stage(Build& B) {
  unsigned long long* d_keys;
  HIP_TRY(B.A.alloc(&d_keys, 6));
  const unsigned long long init[6] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull};
  HIP_TRY(hipMemcpyAsync(d_keys, init, sizeof init, hipMemcpyHostToDevice, B.st));
  hipLaunchKernelGGL(k_root_keys, dim3(blocks(B.ntri)), dim3(BLK), 0, B.st, B.d_tlo, B.d_thi, B.ntri, d_keys);
  HIP_TRY(hipGetLastError());
  unsigned long long keys[6];
  float4 ext[6];  // per component the bounds that hold its minimum [0..2] and its maximum [3..5]
  HIP_TRY(hipMemcpyAsync(keys, d_keys, sizeof keys, hipMemcpyDeviceToHost, B.st));
  HIP_TRY(hipMemcpyAsync(&ext[0], B.d_tlo, sizeof ext[0], hipMemcpyDeviceToHost, B.st));
  HIP_TRY(hipMemcpyAsync(&ext[3], B.d_thi, sizeof ext[3], hipMemcpyDeviceToHost, B.st));
  HIP_TRY(hipStreamSynchronize(B.st));
  ext[1] = ext[2] = ext[0];
  ext[4] = ext[5] = ext[3];
  for (int k = 0; k < 6; k++) {
    // the fold starts from triangle 0 and replaces only on a strict improvement: a NaN at triangle 0 stays;
    // otherwise the first triangle holding the extreme value
    const float4 t0 = ext[k];
    const float v0 = k % 3 == 0 ? t0.x : (k % 3 == 1 ? t0.y : t0.z);
    const uint32_t t = k < 3 ? (uint32_t)keys[k] : ~(uint32_t)keys[k];
    if (v0 != v0 || keys[k] == init[k] || t == 0) continue;
    if (t >= (uint32_t)B.ntri)
      return kdpt::fail(KDPT_ERR_HIP, "device KD build: root box: the key reduction names triangle " +
                                          std::to_string(t) + " of " + std::to_string(B.ntri));
    HIP_TRY(hipMemcpyAsync(&ext[k], (k < 3 ? B.d_tlo : B.d_thi) + t, sizeof ext[k], hipMemcpyDeviceToHost, B.st));
  }
  HIP_TRY(hipStreamSynchronize(B.st));
  float rmin[3], rmax[3], ctr[3];
  for (int c = 0; c < 3; c++) {
    rmin[c] = c == 0 ? ext[c].x : (c == 1 ? ext[c].y : ext[c].z);
    rmax[c] = c == 0 ? ext[3 + c].x : (c == 1 ? ext[3 + c].y : ext[3 + c].z);
    ctr[c] = (float)((double)(rmin[c] + rmax[c]) / 2.0);  // before the pad
  }
  const float pad = (float)0.001;
  B.rlo = make_float4(rmin[0] - pad, rmin[1] - pad, rmin[2] - pad, 0.0f);
  B.rhi = make_float4(rmax[0] + pad, rmax[1] + pad, rmax[2] + pad, 0.0f);
  B.rctr = make_float4(ctr[0], ctr[1], ctr[2], 0.0f);
  return KDPT_OK;
}

// The node store, the pair lists and the leaf store at their initial capacities, and the root in them.
int init_store(Build& B) {
  const int ntri = B.ntri;
  // every split makes two non-empty children and levels stop past maxdepth: < 2^(maxdepth + 2) nodes
  HIP_TRY(B.nodes.alloc_all(
      std::max<long long>(1024, std::min<long long>(4ll * ntri + 16, 1ll << std::min(B.maxdepth + 2, 20)))));
  HIP_TRY(B.pairs.alloc_all(std::max<long long>(3 * (long long)ntri, 1024)));
  HIP_TRY(B.leaves.alloc_all(std::max<long long>(3 * (long long)ntri, 1024)));
  // root: KDnode defaults (axis 0, splitPos 0, parent -1), all triangles in file order
  const int m1 = -1, z = 0;
  const float zf = 0.0f;
  const Nodes& N = B.N;
  HIP_TRY(hipMemcpyAsync(N.lo, &B.rlo, sizeof B.rlo, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.hi, &B.rhi, sizeof B.rhi, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.ctr, &B.rctr, sizeof B.rctr, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.parent, &m1, 4, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.axis, &z, 4, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.split_pos, &zf, 4, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.pstart, &z, 4, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.pcnt, &ntri, 4, hipMemcpyHostToDevice, B.st));
  HIP_TRY(hipMemcpyAsync(N.id, &z, 4, hipMemcpyHostToDevice, B.st));
  hipLaunchKernelGGL(k_iota, dim3(blocks(ntri)), dim3(BLK), 0, B.st, B.ptri[0], ntri);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(B.pnode[0], 0, 4 * (size_t)ntri, B.st));
  return KDPT_OK;
}

// The level loop, breadth first.  A level's node count and pair count are known before its children are made, so
// the stores grow inside the loop (capacity doubling): the level's flags and scans are already in place, only
// the next level's outputs need the larger capacity (rare: the initial capacities cover the reference meshes).
int levels_stage(Build& B) {
  if (int rc = init_store(B)) return rc;
  const hipStream_t st = B.st;
  long long npairs = B.ntri;
  for (int level = 0;; level++) {
    const int nl = B.lvl_count.back(), lb = B.lvl_begin.back();
    if (nl == 0) break;
    LevelArgs L{level, level % 3, B.maxdepth, lb, nl, npairs};
    const int cur = level & 1;
    hipLaunchKernelGGL(k_side, dim3(blocks(npairs + 1)), dim3(BLK), 0, st, L, B.ptri[cur], B.pnode[cur], B.N, B.d_tlo,
                       B.d_thi, B.fl, B.fr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(B.scan.exclusive(B.fl, B.sl, npairs + 1));
    HIP_TRY(B.scan.exclusive(B.fr, B.sr, npairs + 1));
    hipLaunchKernelGGL(k_decide, dim3(blocks(nl + 1)), dim3(BLK), 0, st, L, B.N, B.sl, B.sr, B.nsplit, B.npair, B.nleaf,
                       B.cl, B.cr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(B.scan.exclusive(B.nsplit, B.nsplit_ex, nl + 1));
    HIP_TRY(B.scan.exclusive(B.npair, B.npair_ex, nl + 1));
    HIP_TRY(B.scan.exclusive(B.nleaf, B.nleaf_ex, nl + 1));
    int tot[3];
    HIP_TRY(hipMemcpyAsync(&tot[0], B.nsplit_ex + nl, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tot[1], B.npair_ex + nl, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&tot[2], B.nleaf_ex + nl, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const long long nnodes_next = B.nnodes + 2ll * tot[0], npairs_next = tot[1], nleaf_next = B.leaf_total + tot[2];
    if (nnodes_next > B.nodes.cap) HIP_TRY(B.nodes.grow(st, std::max(2 * B.nodes.cap, nnodes_next + 16)));
    if (npairs_next > B.pairs.cap) HIP_TRY(B.pairs.grow(st, std::max(2 * B.pairs.cap, npairs_next + 16)));
    if (nleaf_next > B.leaves.cap) HIP_TRY(B.leaves.grow(st, std::max(2 * B.leaves.cap, nleaf_next + 16)));
    hipLaunchKernelGGL(k_children, dim3(blocks(nl)), dim3(BLK), 0, st, L, B.N, B.nsplit_ex, B.npair_ex, B.nleaf_ex,
                       B.nsplit, B.cl, B.cr, (int)B.leaf_total);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_scatter, dim3(blocks(npairs)), dim3(BLK), 0, st, L, B.N, B.ptri[cur], B.pnode[cur], B.fl, B.fr,
                       B.sl, B.sr, B.nsplit, B.ptri[cur ^ 1], B.pnode[cur ^ 1], B.leaf_tri, B.leaf_node);
    HIP_TRY(hipGetLastError());
    npairs = npairs_next;
    B.leaf_total = nleaf_next;
    B.lvl_begin.push_back(lb + nl);
    B.lvl_count.push_back(2 * tot[0]);
    B.nnodes = (int)nnodes_next;
  }
  return KDPT_OK;
}

// Pre-order IDs: subtree sizes bottom-up, then IDs top-down.
int preorder_stage(Build& B) {
  const int nlev = (int)B.lvl_count.size();
  for (int l = nlev - 1; l >= 0; l--) {
    if (B.lvl_count[l] == 0) continue;
    hipLaunchKernelGGL(k_sizes, dim3(blocks(B.lvl_count[l])), dim3(BLK), 0, B.st, B.N, B.lvl_begin[l], B.lvl_count[l]);
    HIP_TRY(hipGetLastError());
  }
  for (int l = 0; l < nlev; l++) {
    if (B.lvl_count[l] == 0) continue;
    hipLaunchKernelGGL(k_ids, dim3(blocks(B.lvl_count[l])), dim3(BLK), 0, B.st, B.N, B.lvl_begin[l], B.lvl_count[l]);
    HIP_TRY(hipGetLastError());
  }
  return KDPT_OK;
}

// The leaves' triangles in ID order, then the NodeBare / TriBare arrays and their read-back.
int emit_stage(Build& B, std::vector<kdpt_node_bare>& nodes_out, std::vector<kdpt_tri_bare>& tris_out) {
  const int nnodes = B.nnodes;
  const long long leaf_total = B.leaf_total;
  int *by_id, *tstart;
  HIP_TRY(B.A.alloc(&by_id, (size_t)nnodes + 1));
  HIP_TRY(B.A.alloc(&tstart, (size_t)nnodes + 1));
  hipLaunchKernelGGL(k_leaf_sizes_by_id, dim3(blocks(nnodes + 1)), dim3(BLK), 0, B.st, B.N, nnodes, by_id);
  HIP_TRY(hipGetLastError());
  HIP_TRY(B.scan.exclusive(by_id, tstart, nnodes + 1));
  kdpt_node_bare* d_nodes;
  kdpt_tri_bare* d_tris;
  HIP_TRY(B.A.alloc(&d_nodes, (size_t)nnodes));
  HIP_TRY(B.A.alloc(&d_tris, (size_t)leaf_total));
  hipLaunchKernelGGL(k_write_nodes, dim3(blocks(nnodes)), dim3(BLK), 0, B.st, B.N, nnodes, tstart, d_nodes);
  if (leaf_total > 0)
    hipLaunchKernelGGL(k_write_tris, dim3(blocks(leaf_total)), dim3(BLK), 0, B.st, B.N, leaf_total, B.leaf_tri,
                       B.leaf_node, tstart, B.d_v9, B.d_n9, B.d_mtl, d_tris);
  HIP_TRY(hipGetLastError());
  nodes_out.resize(nnodes);
  tris_out.resize((size_t)leaf_total);
  HIP_TRY(hipMemcpyAsync(nodes_out.data(), d_nodes, sizeof(kdpt_node_bare) * (size_t)nnodes, hipMemcpyDeviceToHost,
                         B.st));
  if (leaf_total > 0)
    HIP_TRY(hipMemcpyAsync(tris_out.data(), d_tris, sizeof(kdpt_tri_bare) * (size_t)leaf_total, hipMemcpyDeviceToHost,
                           B.st));
  HIP_TRY(hipStreamSynchronize(B.st));
  return KDPT_OK;
}

}  // namespace

namespace kdpt_host {

int build_kd_device(const float* v9, const float* n9, const int* mtl, int ntri, int maxdepth, int device,
                    std::vector<kdpt_node_bare>& nodes_out, std::vector<kdpt_tri_bare>& tris_out, double* ms) {
  nodes_out.clear();
  tris_out.clear();
  if (ntri <= 0) return KDPT_OK;
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(device));
  kdpt::Stream st;  // (destroyed after the build's buffers)
  HIP_TRY(st.create());
  Arena A;
  Build B(v9, n9, mtl, ntri, maxdepth, st, A);
  int rc;
  if ((rc = upload_stage(B)) || (rc = root_box_stage(B)) || (rc = levels_stage(B)) || (rc = preorder_stage(B)) ||
      (rc = emit_stage(B, nodes_out, tris_out)))
    return rc;
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KDPT_OK;
}

}  // namespace kdpt_host
