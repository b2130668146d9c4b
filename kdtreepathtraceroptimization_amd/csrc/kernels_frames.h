// kernels_frames.h -- the frame path's two kernels: k_sum_frames (the copy reduce's sum) and k_spin (the
// "reduce_spin_us" diagnostic).
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

// Diagnostic ("reduce_spin_us" knob): one wave that spins for `ticks` of the device's constant-rate clock on the
// reduce stream ahead of a frame's reduce -- what an ncclReduce waiting for a slower peer looks like to this
// GPU's queues (tools/reduce_spin_probe.py).
__global__ void k_spin(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}

}  // namespace
