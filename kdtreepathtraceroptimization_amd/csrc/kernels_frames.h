// kernels_frames.h -- the frame path's kernels: k_sum_frames (the copy reduce's sum), k_frame_moments (rank 0's
// finish of a frame that carries second moments) and k_spin (the "reduce_spin_us" diagnostic).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_masks.h.  Device code and launch-argument structs only: no HIP host call lives here (the
// static guards read the host sections; tests/test_stream_discipline.py checks that none is here).
#pragma once


namespace {

// frame image = a + b + ... (rank order), the copy-reduce's sum
struct FrameParts {
  const float* p[8];
  int n;
};
__global__ void k_sum_frames(float* __restrict__ out, FrameParts parts, int n3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float v = parts.p[0][i];
  for (int k = 1; k < parts.n; k++) v += parts.p[k][i];
  out[i] = v;
}

// A frame that carries second moments (kdpt_group with KDPT_GROUP_MOMENTS), finished on rank 0 in one pass.  Every
// part holds S then Q, n3 floats each: the copy reduce's N staged parts, or RCCL's one reduced buffer.  For each
// float: S_f = the parts' S in rank order (k_sum_frames' adds), Q_f likewise, image = fadd(image, S_f) (the
// moments-off group's k_accumulate_batch add, so its bits) and sumsq = fadd(sumsq, Q_f); S_f goes to `frame` for
// the copy to the caller's `out` (null: the one part is the reduced buffer, which already holds it).  Adds only,
// each rounded once: a frame buffer never sees a fused multiply-add.
__global__ void k_frame_moments(float* __restrict__ image, float* __restrict__ sumsq, float* frame, FrameParts parts,
                                int n3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float s = parts.p[0][i], q = parts.p[0][(size_t)n3 + i];
  for (int k = 1; k < parts.n; k++) {
    s = __fadd_rn(s, parts.p[k][i]);
    q = __fadd_rn(q, parts.p[k][(size_t)n3 + i]);
  }
  if (frame) frame[i] = s;
  image[i] = __fadd_rn(image[i], s);
  sumsq[i] = __fadd_rn(sumsq[i], q);
}

// Diagnostic ("reduce_spin_us" knob): one wave that spins for `ticks` of the device's constant-rate clock on the
// reduce stream ahead of a frame's reduce -- what an ncclReduce waiting for a slower peer looks like to this
// GPU's queues (tools/reduce_spin_probe.py).
__global__ void k_spin(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}

}  // namespace
