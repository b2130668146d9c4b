// kernels_temporal.h -- temporal accumulation for the denoiser (kdpt_denoise_temporal, kdpt_temporal_buffers):
// k_temporal (one pixel per lane: reproject the pixel's own hit point through the history's camera, accept the
// bilinear taps that lie on the same surface in world space, blend) and k_temporal_pack_history (a caller's history
// arrays into the records, as they come).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_denoise.h, whose records (g0, g1, cv), fbits and dn_* helpers it uses, and the kernels keep that
// order in the code object.  Device code and launch-argument structs only: no HIP host call lives here.
#pragma once

namespace {

// ---------------------------------------------------------------------------
// The stage's arithmetic (include/kdpt.h "Temporal accumulation"): float32 add, subtract, multiply, divide, compare,
// abs, floorf and float -> int conversion, every operation rounded on its own (the _rn intrinsics), denormals kept.
// A numpy float32 restatement gives the same bits.
// A frame is kernels_denoise.h's three records per pixel plus a history length:
//   g0 = {normal.xyz, depth}   g1 = {point.xyz, id bits}   cv = {color.rgb, variance}   len = L
// The current frame's g0.w is the pack kernels' validity (depth, or -1); a history pixel is usable iff its
// g0.w > 0 and its len > 0.
// ---------------------------------------------------------------------------
struct TemporalArgs {
  const float4* g0;    // the current frame
  const float4* g1;
  const float4* cv;
  const float4* h0;    // the history (all four null: none)
  const float4* h1;
  const float4* hcv;
  const float* hlen;
  float4* out_cv;      // C', V'
  float* out_len;      // L'
  unsigned int* counts;  // [0] valid pixels, [1] of which found history (null: not counted)
  kdpt_camera cam;     // the history's camera
  int W, H;
  float alpha, sigma_z, normal_min, max_history;  // (float)max_history
};

// One tap q (inside the image) of bilinear weight w.
struct TemporalSums {
  float sw, sr, sg, sb, sv, sl;
};
__device__ __attribute__((always_inline)) inline void tp_tap(TemporalSums& S, const TemporalArgs& A, const float4& p0,
                                                             const float4& p1, float den_z, float w, size_t q) {
  const float4 q0 = A.h0[q];
  const float lq = A.hlen[q];
  if (!(q0.w > 0.0f) || !(lq > 0.0f)) return;
  const float4 q1 = A.h1[q];
  if (fbits(q1.w) != fbits(p1.w)) return;
  const float dn = __fadd_rn(__fadd_rn(__fmul_rn(p0.x, q0.x), __fmul_rn(p0.y, q0.y)), __fmul_rn(p0.z, q0.z));
  if (!(dn >= A.normal_min)) return;
  const float ex = __fsub_rn(q1.x, p1.x), ey = __fsub_rn(q1.y, p1.y), ez = __fsub_rn(q1.z, p1.z);
  const float dz = __fadd_rn(__fadd_rn(__fmul_rn(p0.x, ex), __fmul_rn(p0.y, ey)), __fmul_rn(p0.z, ez));
  if (!(__fdiv_rn(fabsf(dz), den_z) <= 1.0f)) return;
  if (!(w > 0.0f)) return;
  const float4 q2 = A.hcv[q];
  S.sw = __fadd_rn(S.sw, w);
  S.sr = __fadd_rn(S.sr, __fmul_rn(w, q2.x));
  S.sg = __fadd_rn(S.sg, __fmul_rn(w, q2.y));
  S.sb = __fadd_rn(S.sb, __fmul_rn(w, q2.z));
  S.sv = __fadd_rn(S.sv, __fmul_rn(w, q2.w));
  S.sl = __fadd_rn(S.sl, __fmul_rn(w, lq));
}

// The image coordinate of point e (relative to the history's eye) along axis t: half - ((e . t) / z) / pixel.
__device__ __attribute__((always_inline)) inline float tp_dot(float ex, float ey, float ez, const float* t) {
  return __fadd_rn(__fadd_rn(__fmul_rn(ex, t[0]), __fmul_rn(ey, t[1])), __fmul_rn(ez, t[2]));
}

// One pixel per lane, lanes neighbours in x: the current records are three coalesced 16-byte loads, the history
// 4 taps x (h0, h1, hcv, hlen) gathered through L2 / MALL -- for a small camera move neighbouring lanes' taps are
// neighbouring pixels.  No LDS, no floating-point atomics; the two counters take one integer add per wave.
__global__ __launch_bounds__(256) void k_temporal(TemporalArgs A) {
  const int W = A.W, H = A.H;
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = p < (size_t)W * (size_t)H;
  bool valid = false, found = false;
  if (live) {
    const float4 p0 = A.g0[p], c = A.cv[p];
    float4 o = c;
    float len = 0.0f;
    valid = p0.w > 0.0f;
    if (valid) {
      len = 1.0f;
      TemporalSums S{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (A.h0) {
        const float4 p1 = A.g1[p];
        const float ex = __fsub_rn(p1.x, A.cam.position[0]), ey = __fsub_rn(p1.y, A.cam.position[1]),
                    ez = __fsub_rn(p1.z, A.cam.position[2]);
        const float z = tp_dot(ex, ey, ez, A.cam.view);
        if (z > 0.0f) {
          const float a = tp_dot(ex, ey, ez, A.cam.right), b = tp_dot(ex, ey, ez, A.cam.up);
          const float fx = __fsub_rn(__fmul_rn((float)W, 0.5f), __fdiv_rn(__fdiv_rn(a, z), A.cam.pixelLength[0]));
          const float fy = __fsub_rn(__fmul_rn((float)H, 0.5f), __fdiv_rn(__fdiv_rn(b, z), A.cam.pixelLength[1]));
          if (fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {
            const float flx = floorf(fx), fly = floorf(fy);
            const int ix = (int)flx, iy = (int)fly;  // -1 .. W - 1, -1 .. H - 1
            const float tx = __fsub_rn(fx, flx), ty = __fsub_rn(fy, fly);
            const float wx[2] = {__fsub_rn(1.0f, tx), tx}, wy[2] = {__fsub_rn(1.0f, ty), ty};
            const float den_z = __fmul_rn(A.sigma_z, p0.w);
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
              for (int i = 0; i < 2; i++) {
                const int qx = ix + i, qy = iy + j;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                tp_tap(S, A, p0, p1, den_z, __fmul_rn(wx[i], wy[j]), (size_t)qy * (size_t)W + (size_t)qx);
              }
          }
        }
      }
      if (S.sw > 0.0f) {
        found = true;
        const float lh = __fdiv_rn(S.sl, S.sw), vh = __fdiv_rn(S.sv, S.sw);
        const float l1 = __fadd_rn(lh, 1.0f);
        len = l1 < A.max_history ? l1 : A.max_history;
        const float il = __fdiv_rn(1.0f, len);
        const float al = il > A.alpha ? il : A.alpha;
        const float be = __fsub_rn(1.0f, al);
        o.x = __fadd_rn(__fmul_rn(be, __fdiv_rn(S.sr, S.sw)), __fmul_rn(al, c.x));
        o.y = __fadd_rn(__fmul_rn(be, __fdiv_rn(S.sg, S.sw)), __fmul_rn(al, c.y));
        o.z = __fadd_rn(__fmul_rn(be, __fdiv_rn(S.sb, S.sw)), __fmul_rn(al, c.z));
        o.w = __fadd_rn(__fmul_rn(__fmul_rn(be, be), vh), __fmul_rn(__fmul_rn(al, al), c.w));
      }
    }
    A.out_cv[p] = o;
    A.out_len[p] = len;
  }
  if (A.counts) {  // (uniform: every lane of the wave is here)
    const unsigned long long mv = __ballot(valid), mf = __ballot(found);
    if (__lane_id() == 0) {
      if (mv) atomicAdd(A.counts, (unsigned int)__popcll(mv));
      if (mf) atomicAdd(A.counts + 1, (unsigned int)__popcll(mf));
    }
  }
}

// kdpt_temporal_buffers' history: the caller's arrays into the records as they are (no validity is decided here:
// a history pixel's usability is its depth and length, k_temporal's rule).
__global__ __launch_bounds__(256) void k_temporal_pack_history(DenoiseArrays in, int npix, float4* __restrict__ g0,
                                                               float4* __restrict__ g1, float4* __restrict__ cv) {
  const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)npix) return;
  g0[p] = make_float4(in.normal[3 * p], in.normal[3 * p + 1], in.normal[3 * p + 2], in.depth[p]);
  g1[p] = make_float4(in.point[3 * p], in.point[3 * p + 1], in.point[3 * p + 2], ibits(in.id[p]));
  cv[p] = make_float4(in.color[3 * p], in.color[3 * p + 1], in.color[3 * p + 2], in.variance[p]);
}

// The lengths beside k_denoise_unpack's colour and variance are a plain float array already: no unpack of their own.

}  // namespace
