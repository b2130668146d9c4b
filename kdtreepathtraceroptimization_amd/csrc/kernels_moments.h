// kernels_moments.h -- per-pixel second moments: k_accumulate_moments (the sibling of k_accumulate_batch that
// also adds the squares), k_noise_map and the two-stage reduction of kdpt_noise_estimate (k_noise_partials,
// k_noise_final), and the first two again for per-pixel sample counts (k_noise_map_counted,
// k_noise_partials_counted: after kdpt_trace_adaptive).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_adaptive.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// A batch's partial images in iteration order (k_accumulate_batch's PartialImages, for this section).
struct MomentParts {
  const float* p[MAXB];
  int nb;
};

// image += x and sumsq += fl(x * x) for each partial value x, in iteration order: one read and one write of the
// image and of sumsq per batch.  The image's adds are k_accumulate_batch's, so its bits are; the product and the
// add of the second moment are rounded separately (no fused multiply-add, whatever the contraction flags say).
__global__ void k_accumulate_moments(float* __restrict__ image, float* __restrict__ sumsq, MomentParts parts,
                                     int n3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float v = image[i], q = sumsq[i];
  for (int b = 0; b < parts.nb; b++) {
    const float x = parts.p[b][i];
    v += x;
    q = __fadd_rn(q, __fmul_rn(x, x));
  }
  image[i] = v;
  sumsq[i] = q;
}

// The relative standard error of pixel p's mean from the float sums S (image) and Q (sumsq) of n >= 2 samples,
// in double arithmetic, in the operation order include/kdpt.h spells at kdpt_noise_map.
__device__ __attribute__((always_inline)) inline float noise_of_pixel(const float* __restrict__ S,
                                                                      const float* __restrict__ Q, int p,
                                                                      long long samples, float floor) {
  const double n = (double)samples;
  double m[3], v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double s = (double)S[3 * (size_t)p + c], q = (double)Q[3 * (size_t)p + c];
    m[c] = s / n;
    v[c] = (q - s * m[c]) / (n - 1);
    v[c] = v[c] < 0 ? 0 : v[c];
  }
  const double mbar = ((m[0] + m[1]) + m[2]) / 3;
  const double vbar = ((v[0] + v[1]) + v[2]) / 3;
  const double d = mbar > (double)floor ? mbar : (double)floor;
  return (float)(sqrt(vbar / n) / d);
}

__global__ void k_noise_map(const float* __restrict__ image, const float* __restrict__ sumsq, int npix,
                            long long samples, float floor, float* __restrict__ noise) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  noise[p] = noise_of_pixel(image, sumsq, p, samples, floor);
}

// kdpt_noise_estimate's reduction.  Stage one: every lane the values of its NOISE_PER_LANE pixels in pixel order,
// reduced within the wave64 with shuffles and across the workgroup's four waves through LDS in wave order, one
// partial per workgroup of NOISE_BLOCK * NOISE_PER_LANE pixels.  Stage two: one lane adds the partials in index
// order (so the fewer the better: the serial adds are that stage's whole time).  No atomics anywhere: the result
// is a function of the sums alone, the same bytes on every call.
struct NoisePartial {
  double sum;  // of the finite entries
  long long above, nonfinite;
  float max;   // of the finite entries (entries are >= 0)
  float pad_;
};
constexpr int NOISE_BLOCK = 256;
constexpr int NOISE_PER_LANE = 8;

__device__ __attribute__((always_inline)) inline NoisePartial noise_merge(NoisePartial a, const NoisePartial& b) {
  a.sum += b.sum;
  a.above += b.above;
  a.nonfinite += b.nonfinite;
  a.max = b.max > a.max ? b.max : a.max;
  return a;
}

__global__ __launch_bounds__(NOISE_BLOCK) void k_noise_partials(const float* __restrict__ image,
                                                                const float* __restrict__ sumsq, int npix,
                                                                long long samples, float floor, float threshold,
                                                                NoisePartial* __restrict__ partials) {
  __shared__ NoisePartial waves[NOISE_BLOCK / 64];
  NoisePartial r{0.0, 0, 0, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < NOISE_PER_LANE; k++) {  // (coalesced: the workgroup's lanes take neighbouring pixels)
    const long long p = ((long long)blockIdx.x * NOISE_PER_LANE + k) * NOISE_BLOCK + threadIdx.x;
    if (p >= npix) break;
    const float e = noise_of_pixel(image, sumsq, (int)p, samples, floor);
    if (isfinite(e)) {
      r.sum += (double)e;
      r.max = e > r.max ? e : r.max;
      r.above += e > threshold ? 1 : 0;
    } else {
      r.nonfinite += 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    NoisePartial o;
    o.sum = __shfl_down(r.sum, off, 64);
    o.above = __shfl_down(r.above, off, 64);
    o.nonfinite = __shfl_down(r.nonfinite, off, 64);
    o.max = __shfl_down(r.max, off, 64);
    r = noise_merge(r, o);
  }
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    NoisePartial t = waves[0];
    for (int w = 1; w < NOISE_BLOCK / 64; w++) t = noise_merge(t, waves[w]);
    t.pad_ = 0.0f;
    partials[blockIdx.x] = t;
  }
}

// The two per-pixel passes again with per-pixel sample counts n_p = samples + extra[p] (after kdpt_trace_adaptive,
// kernels_adaptive.h): noise_of_pixel as it is, and k_noise_partials' reduction restated, so that the kernels above
// stay the code they were.
__global__ void k_noise_map_counted(const float* __restrict__ image, const float* __restrict__ sumsq,
                                    const uint32_t* __restrict__ extra, int npix, long long samples, float floor,
                                    float* __restrict__ noise) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  noise[p] = noise_of_pixel(image, sumsq, p, samples + (long long)extra[p], floor);
}
__global__ __launch_bounds__(NOISE_BLOCK) void k_noise_partials_counted(
    const float* __restrict__ image, const float* __restrict__ sumsq, const uint32_t* __restrict__ extra, int npix,
    long long samples, float floor, float threshold, NoisePartial* __restrict__ partials) {
  __shared__ NoisePartial waves[NOISE_BLOCK / 64];
  NoisePartial r{0.0, 0, 0, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < NOISE_PER_LANE; k++) {  // (coalesced: the workgroup's lanes take neighbouring pixels)
    const long long p = ((long long)blockIdx.x * NOISE_PER_LANE + k) * NOISE_BLOCK + threadIdx.x;
    if (p >= npix) break;
    const float e = noise_of_pixel(image, sumsq, (int)p, samples + (long long)extra[p], floor);
    if (isfinite(e)) {
      r.sum += (double)e;
      r.max = e > r.max ? e : r.max;
      r.above += e > threshold ? 1 : 0;
    } else {
      r.nonfinite += 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    NoisePartial o;
    o.sum = __shfl_down(r.sum, off, 64);
    o.above = __shfl_down(r.above, off, 64);
    o.nonfinite = __shfl_down(r.nonfinite, off, 64);
    o.max = __shfl_down(r.max, off, 64);
    r = noise_merge(r, o);
  }
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    NoisePartial t = waves[0];
    for (int w = 1; w < NOISE_BLOCK / 64; w++) t = noise_merge(t, waves[w]);
    t.pad_ = 0.0f;
    partials[blockIdx.x] = t;
  }
}

// (one workgroup: the lanes fetch NOISE_BLOCK partials at a time into LDS, lane 0 adds them in index order)
__global__ __launch_bounds__(NOISE_BLOCK) void k_noise_final(const NoisePartial* __restrict__ partials, int nparts,
                                                             NoisePartial* __restrict__ out) {
  __shared__ NoisePartial stage[NOISE_BLOCK];
  NoisePartial t{0.0, 0, 0, 0.0f, 0.0f};
  for (int base = 0; base < nparts; base += NOISE_BLOCK) {
    const int m = nparts - base < NOISE_BLOCK ? nparts - base : NOISE_BLOCK;
    if ((int)threadIdx.x < m) stage[threadIdx.x] = partials[base + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 0; k < m; k++) t = noise_merge(t, stage[k]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = t;
}

}  // namespace
