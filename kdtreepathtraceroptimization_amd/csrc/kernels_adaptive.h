// kernels_adaptive.h -- adaptive sampling (kdpt_trace_adaptive): the list of the pixels whose noise is above a
// threshold (k_adapt_flags, k_adapt_scan, k_adapt_list), bounce 0 of a batch that starts from that list
// (k_adapt_rays_b, k_adapt_geoms_b, the counterparts of k_gen_rays_b / k_gen_geoms_b), the add of a batch's partial
// images through the list (k_accumulate_adapt), a group's round added through it (k_adapt_slots) and the save pass with per-pixel sample counts (k_save_counted).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_frames.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// (defined in kernels_moments.h, the section after this one: kdpt_noise_map's per-pixel value)
__device__ __attribute__((always_inline)) inline float noise_of_pixel(const float* __restrict__ S,
                                                                      const float* __restrict__ Q, int p,
                                                                      long long samples, float floor);

// ---------------------------------------------------------------------------
// The active list A: the pixels p with isfinite(e_p) && e_p > threshold, ascending.  Three launches on one stream:
//   k_adapt_flags : one lane per pixel computes e_p (SELFTEST: reads it) and its flag; each wave64 keeps its ballot
//                   (masks, one word per wave), each workgroup its count (the waves' popcounts through LDS)
//   k_adapt_scan  : one workgroup turns the workgroup counts into exclusive offsets and the total |A| (a device word)
//   k_adapt_list  : lane l of a flagged pixel writes it at offset[workgroup] + the earlier waves' counts (LDS, in
//                   wave order) + the number of flagged lanes below l (mbcnt over the wave's ballot)
// A pixel's place is a function of the flags alone: no atomics anywhere, the same list on every call.
// ---------------------------------------------------------------------------
constexpr int ADAPT_BLOCK = 256;

// masks: [4 workgroups] one ballot per wave (a wave past the last pixel stores 0); block_counts: [workgroups]
template <bool SELFTEST>
__global__ __launch_bounds__(ADAPT_BLOCK) void k_adapt_flags(const float* __restrict__ image,
                                                             const float* __restrict__ sumsq,
                                                             const uint32_t* __restrict__ extra,
                                                             const float* __restrict__ values, int npix,
                                                             long long samples, float floor, float threshold,
                                                             unsigned long long* __restrict__ masks,
                                                             int* __restrict__ block_counts) {
  __shared__ int s_w[ADAPT_BLOCK / 64];
  const int p = blockIdx.x * ADAPT_BLOCK + threadIdx.x;
  bool active = false;
  if (p < npix) {
    const float e = SELFTEST ? values[p] : noise_of_pixel(image, sumsq, p, samples + (long long)extra[p], floor);
    active = isfinite(e) && e > threshold;
  }
  const unsigned long long m = __ballot(active);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    masks[(size_t)blockIdx.x * (ADAPT_BLOCK / 64) + wv] = m;
    s_w[wv] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < ADAPT_BLOCK / 64; w++) tot += s_w[w];
    block_counts[blockIdx.x] = tot;
  }
}

// (one workgroup: ADAPT_BLOCK counts at a time -- an inclusive scan within each wave by shuffles, the waves' totals
// through LDS in wave order, the running total carried from one round to the next)
__global__ __launch_bounds__(ADAPT_BLOCK) void k_adapt_scan(const int* __restrict__ block_counts, int nblocks,
                                                            int* __restrict__ block_off, int* __restrict__ count) {
  __shared__ int s_w[ADAPT_BLOCK / 64], s_carry;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += ADAPT_BLOCK) {
    const int i = base + threadIdx.x;
    const int v = i < nblocks ? block_counts[i] : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int before = s_carry;
    for (int w = 0; w < wv; w++) before += s_w[w];
    if (i < nblocks) block_off[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == ADAPT_BLOCK - 1) s_carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = s_carry;
}

// list: [npix]; entries 0 .. |A| - 1 are written (a slot is below the scan's total, which is at most npix)
__global__ __launch_bounds__(ADAPT_BLOCK) void k_adapt_list(const unsigned long long* __restrict__ masks,
                                                            const int* __restrict__ block_off,
                                                            int* __restrict__ list) {
  __shared__ int s_w[ADAPT_BLOCK / 64];
  const int p = blockIdx.x * ADAPT_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = masks[(size_t)blockIdx.x * (ADAPT_BLOCK / 64) + wv];
  if (lane == 0) s_w[wv] = __popcll(m);
  __syncthreads();
  if (!((m >> lane) & 1ull)) return;
  int slot = block_off[blockIdx.x];
  for (int w = 0; w < wv; w++) slot += s_w[w];
  list[slot + (int)lane_prefix(m)] = p;
}

// ---------------------------------------------------------------------------
// Bounce 0 from the list: path j of iteration blockIdx.y is the camera's ray through pixel list[j] (gen_rays_body
// with the slot and the pixel apart), counts[0] = n.  Everything after reads counts[depth] and the path buffers, as
// after a ray query's k_user_rays_b.  GEN_BLOCK-thread workgroups for the reason given above KDPT_GEN_BLOCK.
// ---------------------------------------------------------------------------
struct AdaptBatch {
  GenBatch g;
  const int* list;  // [n] pixel indices, ascending
  int n;
};

__device__ __attribute__((always_inline)) inline bool adapt_rays_body(const AdaptBatch& B, f3& ray_o, f3& ray_d) {
  const GenIter& g = B.g.it[blockIdx.y];
  return gen_rays_body(B.g.cam, g.iter, B.g.traceDepth, g.out, B.g.focalLength, B.g.dofAngle, B.g.antialias, g.counts,
                       B.g.ncounts, g.work, B.g.nwork, g.trace_t, g.lb, B.g.nlb, g.zero_image, B.n, B.list, ray_o,
                       ray_d);
}

// gen_geoms = 0, brute-force and box-view contexts: the paths alone.
__global__ __launch_bounds__(GEN_BLOCK) void k_adapt_rays_b(AdaptBatch B) {
  f3 o, d;
  (void)adapt_rays_body(B, o, d);
}

// The paths and their bounce-0 intersect-stage first part, counting the candidates into this use's ccount0 and
// zeroing the next use's, as k_gen_geoms_b does.
struct AdaptGeomsBatch {
  AdaptBatch a;
  DevScene S;
  GenGeomsIter it[MAXB];
  Counters* count_aabb;
};
__global__ __launch_bounds__(GEN_BLOCK) void k_adapt_geoms_b(AdaptGeomsBatch B) {
  const GenGeomsIter& q = B.it[blockIdx.y];
  f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
  const bool valid = adapt_rays_body(B.a, o, d);
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) *q.ccount0_next = 0;
  geoms_core<GEN_BLOCK>(B.S, valid && B.a.g.traceDepth > 0, j, o, d, q.cray, q.hits, q.cand, q.ccount0, q.qbase,
                        B.count_aabb);
}

// ---------------------------------------------------------------------------
// The add of a batch through the list, one lane per slot: for slot j and pixel p = list[j], image[p] += x and
// sumsq[p] += fl(x * x) for each partial value x = partial_b[j] in iteration order (k_accumulate_moments' two
// roundings), and extra[p] += nb.  The list has no pixel twice, so no two lanes meet.
// ---------------------------------------------------------------------------
struct AdaptParts {
  const float* p[MAXB];
  int nb;
};
__global__ void k_accumulate_adapt(float* __restrict__ image, float* __restrict__ sumsq,
                                   uint32_t* __restrict__ extra, const int* __restrict__ list, int n,
                                   AdaptParts parts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t dst = 3 * (size_t)list[j], src = 3 * (size_t)j;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v = image[dst + c], q = sumsq[dst + c];
    for (int b = 0; b < parts.nb; b++) {
      const float x = parts.p[b][src + c];
      v = __fadd_rn(v, x);
      q = __fadd_rn(q, __fmul_rn(x, x));
    }
    image[dst + c] = v;
    sumsq[dst + c] = q;
  }
  extra[list[j]] += (uint32_t)parts.nb;
}

// An adaptive round of a group (kdpt_group_trace_adaptive) on rank 0, one lane per slot.  Every part is a rank's slot
// buffer after the round: s at [0, 3 n), q at [3 n, 6 n) (the copy reduce's N staged parts, or RCCL's one reduced
// buffer).  For slot j, pixel p = list[j] and each channel: s = the parts' s[j] in rank order, q likewise, image[p] =
// fadd(image[p], s), sumsq[p] = fadd(sumsq[p], q), and extra[p] += count.  The list has no pixel twice.
__global__ void k_adapt_slots(float* __restrict__ image, float* __restrict__ sumsq, uint32_t* __restrict__ extra,
                              const int* __restrict__ list, int n, FrameParts parts, uint32_t count) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int p = list[j];
  const size_t dst = 3 * (size_t)p, src = 3 * (size_t)j, n3 = 3 * (size_t)n;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float s = parts.p[0][src + c], q = parts.p[0][n3 + src + c];
    for (int k = 1; k < parts.n; k++) {
      s = __fadd_rn(s, parts.p[k][src + c]);
      q = __fadd_rn(q, parts.p[k][n3 + src + c]);
    }
    image[dst + c] = __fadd_rn(image[dst + c], s);
    sumsq[dst + c] = __fadd_rn(sumsq[dst + c], q);
  }
  extra[p] += count;
}

// k_save_image with each source pixel divided by its own sample count n_p = samples + extra[p] (extra null: every
// pixel has `samples`); a pixel without samples gives 0.
__global__ void k_save_counted(const float* __restrict__ image, const uint32_t* __restrict__ extra, int W, int H,
                               long long samples, uint8_t* __restrict__ rgb, float* __restrict__ lin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, X = i - y * W;
  const size_t pix = (size_t)(W - 1 - X) + (size_t)y * W;
  const long long n = samples + (extra ? (long long)extra[pix] : 0);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float v = n > 0 ? image[3 * pix + k] / (float)n : 0.0f;
    if (lin) lin[3 * (size_t)i + k] = v;
    const float cl = glm_min(glm_max(v, 0.0f), 1.0f) * 255.f;
    if (rgb) rgb[3 * (size_t)i + k] = (uint8_t)cl;
  }
}

}  // namespace
