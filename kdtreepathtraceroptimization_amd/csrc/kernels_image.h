// kernels_image.h -- k_final_gather, k_pbo, k_save_image, k_unpack and k_accumulate_batch (the add of a batch's
// partial images).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_shade.h.  Device code and launch-argument structs only: no HIP host call lives here (the
// static guards read the host sections; tests/test_stream_discipline.py checks that none is here).
#pragma once

namespace {

// finalGather (src/pathtrace.cu:2373-2383), including index = paths[index].pixelIndex
__global__ void k_final_gather(PathBuf paths, const int* counts, int depth, float* image) {
  const int n = counts[depth];
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= n) return;
  const int j = fbits(paths.p1[index].w) & 0x7fffffff;
  const float4 c = paths.p2[j];
  const int pix = fbits(paths.p1[j].w) & 0x7fffffff;
  image[3 * (size_t)pix + 0] += c.x;
  image[3 * (size_t)pix + 1] += c.y;
  image[3 * (size_t)pix + 2] += c.z;
}

// sendImageToPBO (src/pathtrace.cu:69-89)
__global__ void k_pbo(const float* image, int npix, int iter, uchar4* pbo) {
  const int index = blockIdx.x * blockDim.x + threadIdx.x;
  if (index >= npix) return;
  int c[3];
  for (int k = 0; k < 3; k++) {
    int v = (int)((double)(image[3 * (size_t)index + k] / iter) * 255.0);
    c[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
  }
  pbo[index] = make_uchar4((unsigned char)c[0], (unsigned char)c[1], (unsigned char)c[2], 0);
}

// saveImage (src/main.cpp:1087-1108): x-flip and divide by the sample count, then image::savePNG's
// bytes (src/image.cpp:22-35): glm::clamp(pix, 0, 1) * 255.f truncated to unsigned char.  `lin`
// (optional) receives the flipped, divided float image that image::saveHDR writes.
__global__ void k_save_image(const float* __restrict__ image, int W, int H, float samples, uint8_t* __restrict__ rgb,
                             float* __restrict__ lin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, X = i - y * W;
  const size_t src = 3 * ((size_t)(W - 1 - X) + (size_t)y * W);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float v = image[src + k] / samples;
    if (lin) lin[3 * (size_t)i + k] = v;
    const float cl = glm_min(glm_max(v, 0.0f), 1.0f) * 255.f;
    rgb[3 * (size_t)i + k] = (uint8_t)cl;
  }
}

// debug: unpack the live path array into the reference PathSegment layout
__global__ void k_unpack(PathBuf src, const int* counts, int depth, kdpt_path_segment* out) {
  const int n = counts[depth];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 q0 = src.p0[i], q1 = src.p1[i], q2 = src.p2[i];
  kdpt_path_segment s;
  s.origin[0] = q0.x; s.origin[1] = q0.y; s.origin[2] = q0.z;
  s.direction[0] = q1.x; s.direction[1] = q1.y; s.direction[2] = q1.z;
  const int pw = fbits(q1.w);
  s.isinside = (uint8_t)((pw >> 31) & 1);
  s.pad_[0] = s.pad_[1] = s.pad_[2] = 0;
  s.sdepth = q0.w;
  s.color[0] = q2.x; s.color[1] = q2.y; s.color[2] = q2.z;
  s.pixelIndex = pw & 0x7fffffff;
  s.remainingBounces = fbits(q2.w);
  s.materialIdHit = src.pm[i];
  out[i] = s;
}

// A batch's partial images added in iteration order (one add per pixel and iteration, as partialGather
// does), with one read and one write of the accumulation image per batch instead of one per iteration.
struct PartialImages {
  const float* p[MAXB];
  int nb;
};
__global__ void k_accumulate_batch(float* __restrict__ image, PartialImages parts, int n3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float v = image[i];
  for (int b = 0; b < parts.nb; b++) v += parts.p[b][i];
  image[i] = v;
}

}  // namespace
