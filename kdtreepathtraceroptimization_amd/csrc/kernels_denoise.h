// kernels_denoise.h -- the variance-guided edge-avoiding a-trous filter (kdpt_denoise, kdpt_denoise_buffers):
// k_denoise_rays (the camera's pinhole rays), the two pack kernels (caller arrays, or the context's sums and hit
// records, into three 16-byte records per pixel), k_denoise_pass (one filter pass) and k_denoise_unpack.
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_adaptive.h, and the kernels keep that order in the code object.  Device code and launch-argument
// structs only: no HIP host call lives here (tests/test_stream_discipline.py checks that; the guards read host_*.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// The filter's arithmetic (include/kdpt.h "Denoising"): float32 add, subtract, multiply, divide, sqrt, compare and
// abs, every operation rounded on its own (the _rn intrinsics: no fused multiply-add whatever the contraction flags
// say, as k_accumulate_moments spells its sums), denormals kept, no transcendental.  A numpy float32 restatement
// gives the same bits.
// Per pixel p, three records:
//   g0 = {normal.xyz, depth}      depth <= 0 marks an invalid pixel (validity is decided once, by the pack kernel)
//   g1 = {point.xyz, id bits}
//   cv = {color.rgb, variance}    the only record a pass rewrites (ping-pong)
// ---------------------------------------------------------------------------
constexpr int DN_TILE_W = 32, DN_TILE_H = 8;  // one 256-lane workgroup: lanes of a wave are neighbours in x
constexpr int DN_HALO = 2;                    // taps reach 2 lattice steps each way
constexpr int DN_LDS_W = DN_TILE_W + 2 * DN_HALO, DN_LDS_H = DN_TILE_H + 2 * DN_HALO;

struct DenoisePass {
  const float4* g0;
  const float4* g1;
  const float4* cv;  // pass k - 1's colour and variance
  float4* out;       // pass k's
  int W, H;
  int step;          // 1 << k
  int nrx, nry;      // TILED: the residues mod step that hold pixels, min(step, W) and min(step, H)
  int normal_power_log2;
  float sigma_l, sigma_z, eps_l;
};

__device__ __attribute__((always_inline)) inline bool dn_finite(float x) { return fabsf(x) < FLT_INFV; }

// lum(c) = ((r + g) + b) / 3
__device__ __attribute__((always_inline)) inline float dn_lum(const float4& c) {
  return __fdiv_rn(__fadd_rn(__fadd_rn(c.x, c.y), c.z), 3.0f);
}

// g(x) = 1 / (1 + x (1 + x / 2)): exp(-x) to second order at 0, rational, heavier in the tail
__device__ __attribute__((always_inline)) inline float dn_stop(float x) {
  return __fdiv_rn(1.0f, __fadd_rn(1.0f, __fmul_rn(x, __fadd_rn(1.0f, __fmul_rn(0.5f, x)))));
}

// What a pixel keeps over its 25 taps, and the sums they add to.
struct DenoisePixel {
  float4 n;     // g0 of p
  float4 pt;    // g1 of p
  float lum;    // of pass k - 1's colour of p
  float den_l;  // sigma_l sd + eps_l
  float den_z;  // sigma_z depth
  float sw, sr, sg, sb, sv;
};

// One tap q (inside the image) of weight hh = h[dy + 2] h[dx + 2]: skipped when q is invalid, of another id, or its
// weight is not > 0 (a NaN from an overflowed luminance or an underflowed denominator included).
__device__ __attribute__((always_inline)) inline void dn_tap(DenoisePixel& P, float hh, int power_log2,
                                                             const float4& q0, const float4& q1, const float4& q2) {
  if (!(q0.w > 0.0f)) return;
  if (fbits(q1.w) != fbits(P.pt.w)) return;
  float dn = __fadd_rn(__fadd_rn(__fmul_rn(P.n.x, q0.x), __fmul_rn(P.n.y, q0.y)), __fmul_rn(P.n.z, q0.z));
  dn = dn < 0.0f ? 0.0f : dn;
  dn = dn > 1.0f ? 1.0f : dn;
  for (int k = 0; k < power_log2; k++) dn = __fmul_rn(dn, dn);
  const float ex = __fsub_rn(q1.x, P.pt.x), ey = __fsub_rn(q1.y, P.pt.y), ez = __fsub_rn(q1.z, P.pt.z);
  const float dz = __fadd_rn(__fadd_rn(__fmul_rn(P.n.x, ex), __fmul_rn(P.n.y, ey)), __fmul_rn(P.n.z, ez));
  const float xz = __fdiv_rn(fabsf(dz), P.den_z);
  const float xl = __fdiv_rn(fabsf(__fsub_rn(P.lum, dn_lum(q2))), P.den_l);
  const float w = __fmul_rn(__fmul_rn(__fmul_rn(hh, dn), dn_stop(xz)), dn_stop(xl));
  if (!(w > 0.0f)) return;
  P.sw = __fadd_rn(P.sw, w);
  P.sr = __fadd_rn(P.sr, __fmul_rn(w, q2.x));
  P.sg = __fadd_rn(P.sg, __fmul_rn(w, q2.y));
  P.sb = __fadd_rn(P.sb, __fmul_rn(w, q2.z));
  P.sv = __fadd_rn(P.sv, __fmul_rn(__fmul_rn(w, w), q2.w));
}

// The 3 x 3 variance prefilter's sums, one tap: g3 = [1/4, 1/2, 1/4], the products exact.
__device__ __attribute__((always_inline)) inline void dn_prefilter_tap(float& sg, float& sv, int dx, int dy,
                                                                      float depth, float variance) {
  if (!(depth > 0.0f)) return;
  const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
  sg = __fadd_rn(sg, g);
  sv = __fadd_rn(sv, __fmul_rn(g, variance));
}

__device__ __attribute__((always_inline)) inline float dn_tap_weight(int dx, int dy) {
  const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
  const float hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
  return hy * hx;  // exact in binary
}

__device__ __attribute__((always_inline)) inline DenoisePixel dn_setup(const DenoisePass& A, const float4& p0,
                                                                       const float4& p1, const float4& p2, float sg,
                                                                       float sv) {
  DenoisePixel P;
  P.n = p0;
  P.pt = p1;
  P.lum = dn_lum(p2);
  // (sqrtf: the correctly rounded one, as normalize() uses; HIP's __fsqrt_rn is the native approximation)
  const float sd = sqrtf(__fdiv_rn(sv, sg));
  P.den_l = __fadd_rn(__fmul_rn(A.sigma_l, sd), A.eps_l);
  P.den_z = __fmul_rn(A.sigma_z, p0.w);
  P.sw = P.sr = P.sg = P.sb = P.sv = 0.0f;
  return P;
}

__device__ __attribute__((always_inline)) inline float4 dn_result(const DenoisePixel& P, const float4& p2) {
  if (!(P.sw > 0.0f)) return p2;
  return make_float4(__fdiv_rn(P.sr, P.sw), __fdiv_rn(P.sg, P.sw), __fdiv_rn(P.sb, P.sw),
                     __fdiv_rn(P.sv, __fmul_rn(P.sw, P.sw)));
}

// One pass.  TILED: the pixels congruent to (rx, ry) mod step form a lattice of their own on which the taps are
// neighbours, so a workgroup takes a 32 x 8 tile of one lattice and stages tile + halo (2 lattice steps: 2 step
// pixels on each side) of all three records in LDS -- at step 1 the plain image tile.  An entry outside the image
// is staged as invalid, so skipping covers both.  The 3 x 3 prefilter is always at step 1: from LDS at step 1, from
// memory otherwise.  !TILED: every tap straight from memory (through L2 / MALL), lanes neighbours in x.
// The two routes run the same arithmetic in the same order on the same values: they give the same bits.
template <bool TILED>
__global__ __launch_bounds__(DN_TILE_W * DN_TILE_H) void k_denoise_pass(DenoisePass A) {
  const int W = A.W, H = A.H, s = A.step;
  const int lx = threadIdx.x % DN_TILE_W, ly = threadIdx.x / DN_TILE_W;
  if (TILED) {
    __shared__ float4 s0[DN_LDS_H][DN_LDS_W], s1[DN_LDS_H][DN_LDS_W], s2[DN_LDS_H][DN_LDS_W];
    const int rx = blockIdx.x % A.nrx, ry = blockIdx.y % A.nry;
    const int X0 = (blockIdx.x / A.nrx) * DN_TILE_W, Y0 = (blockIdx.y / A.nry) * DN_TILE_H;  // lattice coordinates
    for (int e = threadIdx.x; e < DN_LDS_W * DN_LDS_H; e += DN_TILE_W * DN_TILE_H) {
      const int ex = e % DN_LDS_W, ey = e / DN_LDS_W;
      const long long x = (long long)(X0 + ex - DN_HALO) * s + rx, y = (long long)(Y0 + ey - DN_HALO) * s + ry;
      float4 a = make_float4(0.0f, 0.0f, 0.0f, -1.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = b;
      if (x >= 0 && x < W && y >= 0 && y < H) {
        const size_t q = (size_t)y * W + (size_t)x;
        a = A.g0[q];
        b = A.g1[q];
        c = A.cv[q];
      }
      s0[ey][ex] = a;
      s1[ey][ex] = b;
      s2[ey][ex] = c;
    }
    __syncthreads();
    const long long x = (long long)(X0 + lx) * s + rx, y = (long long)(Y0 + ly) * s + ry;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const int cx = lx + DN_HALO, cy = ly + DN_HALO;
    const float4 p0 = s0[cy][cx], p2 = s2[cy][cx];
    if (!(p0.w > 0.0f)) {  // an invalid pixel passes through, bit for bit
      A.out[p] = p2;
      return;
    }
    float sg = 0.0f, sv = 0.0f;
    if (s == 1) {
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) dn_prefilter_tap(sg, sv, dx, dy, s0[cy + dy][cx + dx].w, s2[cy + dy][cx + dx].w);
    } else {
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const long long qx = x + dx, qy = y + dy;
          if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
          const size_t q = (size_t)qy * W + (size_t)qx;
          dn_prefilter_tap(sg, sv, dx, dy, A.g0[q].w, A.cv[q].w);
        }
    }
    DenoisePixel P = dn_setup(A, p0, s1[cy][cx], p2, sg, sv);
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
      for (int dx = -2; dx <= 2; dx++)
        dn_tap(P, dn_tap_weight(dx, dy), A.normal_power_log2, s0[cy + dy][cx + dx], s1[cy + dy][cx + dx],
               s2[cy + dy][cx + dx]);
    A.out[p] = dn_result(P, p2);
  } else {
    const int x = blockIdx.x * DN_TILE_W + lx, y = blockIdx.y * DN_TILE_H + ly;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const float4 p0 = A.g0[p], p2 = A.cv[p];
    if (!(p0.w > 0.0f)) {
      A.out[p] = p2;
      return;
    }
    float sg = 0.0f, sv = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const size_t q = (size_t)qy * W + (size_t)qx;
        dn_prefilter_tap(sg, sv, dx, dy, A.g0[q].w, A.cv[q].w);
      }
    DenoisePixel P = dn_setup(A, p0, A.g1[p], p2, sg, sv);
    for (int dy = -2; dy <= 2; dy++) {
      const long long qy = (long long)y + (long long)dy * s;
      if (qy < 0 || qy >= H) continue;
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const long long qx = (long long)x + (long long)dx * s;
        if (qx < 0 || qx >= W) continue;
        const size_t q = (size_t)qy * W + (size_t)qx;
        const float4 q0 = A.g0[q];
        if (!(q0.w > 0.0f)) continue;
        dn_tap(P, dn_tap_weight(dx, dy), A.normal_power_log2, q0, A.g1[q], A.cv[q]);
      }
    }
    A.out[p] = dn_result(P, p2);
  }
}

// ---------------------------------------------------------------------------
// Packing.  Pixel p is valid iff its 11 floats (colour, variance, normal, point, depth) are finite, depth > 0 and
// variance >= 0; an invalid pixel's g0.w is -1, and its colour and variance travel in cv as they came.
// ---------------------------------------------------------------------------
__device__ __attribute__((always_inline)) inline void dn_pack_one(size_t p, float r, float g, float b, float variance,
                                                                  float nx, float ny, float nz, float px, float py,
                                                                  float pz, float depth, int id,
                                                                  float4* __restrict__ g0, float4* __restrict__ g1,
                                                                  float4* __restrict__ cv) {
  const bool valid = dn_finite(r) && dn_finite(g) && dn_finite(b) && dn_finite(variance) && dn_finite(nx) &&
                     dn_finite(ny) && dn_finite(nz) && dn_finite(px) && dn_finite(py) && dn_finite(pz) &&
                     dn_finite(depth) && depth > 0.0f && variance >= 0.0f;
  g0[p] = make_float4(nx, ny, nz, valid ? depth : -1.0f);
  g1[p] = make_float4(px, py, pz, ibits(id));
  cv[p] = make_float4(r, g, b, variance);
}

// kdpt_denoise_buffers: the caller's arrays (device copies).
struct DenoiseArrays {
  const float* color;     // [3 npix]
  const float* variance;  // [npix]
  const float* normal;    // [3 npix]
  const float* point;     // [3 npix]
  const float* depth;     // [npix]
  const int* id;          // [npix]
};
__global__ __launch_bounds__(256) void k_denoise_pack(DenoiseArrays in, int npix, float4* __restrict__ g0,
                                                      float4* __restrict__ g1, float4* __restrict__ cv) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)npix) return;
  dn_pack_one(p, in.color[3 * p], in.color[3 * p + 1], in.color[3 * p + 2], in.variance[p], in.normal[3 * p],
              in.normal[3 * p + 1], in.normal[3 * p + 2], in.point[3 * p], in.point[3 * p + 1], in.point[3 * p + 2],
              in.depth[p], in.id[p], g0, g1, cv);
}

// kdpt_denoise: the context's sums and the hit records of its pinhole rays.  n_p = samples + extra[p] (extra null:
// samples); colour = fdiv(S_c, (float)n_p); the variance of the mean is vbar / n_p with v_c and vbar as
// kdpt_noise_map spells them (noise_of_pixel's operations, restated so that its kernels stay the code they were),
// in double, then rounded to float.  depth = t, or -1 where nothing was hit (kind <= 0).
__global__ __launch_bounds__(256) void k_denoise_pack_render(const float* __restrict__ image,
                                                             const float* __restrict__ sumsq,
                                                             const uint32_t* __restrict__ extra, long long samples,
                                                             const kdpt_ray_hit* __restrict__ hits, int npix,
                                                             float4* __restrict__ g0, float4* __restrict__ g1,
                                                             float4* __restrict__ cv) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)npix) return;
  const long long np = samples + (extra ? (long long)extra[p] : 0);
  const float nf = (float)np;
  const double n = (double)np;
  float col[3];
  double v[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float sf = image[3 * p + c];
    col[c] = __fdiv_rn(sf, nf);
    const double s = (double)sf, q = (double)sumsq[3 * p + c];
    const double m = s / n;
    v[c] = (q - s * m) / (n - 1);
    v[c] = v[c] < 0 ? 0 : v[c];
  }
  const double vbar = ((v[0] + v[1]) + v[2]) / 3;
  const kdpt_ray_hit h = hits[p];
  dn_pack_one(p, col[0], col[1], col[2], (float)(vbar / n), h.normal[0], h.normal[1], h.normal[2], h.point[0],
              h.point[1], h.point[2], h.kind <= 0 ? -1.0f : h.t, h.material, g0, g1, cv);
}

__global__ __launch_bounds__(256) void k_denoise_unpack(const float4* __restrict__ cv, int npix,
                                                        float* __restrict__ color, float* __restrict__ variance) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)npix) return;
  const float4 c = cv[p];
  color[3 * p] = c.x;
  color[3 * p + 1] = c.y;
  color[3 * p + 2] = c.z;
  if (variance) variance[p] = c.w;
}

// The camera's pinhole ray through every pixel: generateRayFromCamera's first part (gen_rays_body, before the
// jitter and the lens), from the eye -- normalize(view - right pixelLength.x (x - W/2) - up pixelLength.y (y - H/2))
// with its operations in its order; packed triples, as kdpt_cast_rays takes them.
__global__ __launch_bounds__(256) void k_denoise_rays(kdpt_camera cam, float* __restrict__ o, float* __restrict__ d) {
  const int W = cam.resolution[0], H = cam.resolution[1];
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= W * H) return;
  const int x = index % W, y = index / W;
  const f3 view = mk3(cam.view[0], cam.view[1], cam.view[2]);
  const f3 right = mk3(cam.right[0], cam.right[1], cam.right[2]);
  const f3 upv = mk3(cam.up[0], cam.up[1], cam.up[2]);
  const f3 a = scl(scl(right, cam.pixelLength[0]), ((float)x - (float)W * 0.5f));
  const f3 b = scl(scl(upv, cam.pixelLength[1]), ((float)y - (float)H * 0.5f));
  const f3 dir = normalize(sub(sub(view, a), b));
  const size_t i = 3 * (size_t)index;
  o[i] = cam.position[0];
  o[i + 1] = cam.position[1];
  o[i + 2] = cam.position[2];
  d[i] = dir.x;
  d[i + 1] = dir.y;
  d[i + 2] = dir.z;
}

}  // namespace
