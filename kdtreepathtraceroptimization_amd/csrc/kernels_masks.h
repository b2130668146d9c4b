// kernels_masks.h -- k_build_masks, the masked cull's direction masks built on the device (host_create.h
// build_masks).
//
// A section of kdpt_runtime.hip's translation unit, not a stand-alone header: kdpt_runtime.hip includes it
// after kernels_selftest.h.  Device code and launch-argument structs only: no HIP host call lives here (the
// static guards read the host sections; tests/test_stream_discipline.py checks that none is here).
#pragma once


namespace {

// The masked cull's cells on the device (kdpt_cull.h dir_mask_cell, the code the host builder runs): one
// workgroup per (cluster, 256 buckets), the cluster's 64 entries staged in LDS (every lane reads the same entry:
// a broadcast), one mask per lane, written bucket-major.
__global__ void __launch_bounds__(256) k_build_masks(const double* __restrict__ ent, const float* __restrict__ krig,
                                                     const double* __restrict__ bd, int ncl, int nb, float Kf,
                                                     unsigned long long* __restrict__ masks) {
  __shared__ double se[5][64];
  __shared__ float sk[64];
  const int c = blockIdx.x;
  const size_t ne = 64 * (size_t)ncl;
  if (threadIdx.x < 64) {
    for (int f = 0; f < 5; f++) se[f][threadIdx.x] = ent[f * ne + 64 * (size_t)c + threadIdx.x];
    sk[threadIdx.x] = krig[64 * (size_t)c + threadIdx.x];
  }
  __syncthreads();
  const int b = blockIdx.y * 256 + threadIdx.x;
  if (b >= nb) return;
  masks[(size_t)b * ncl + c] = dir_mask_cell(se[0], se[1], se[2], se[3], se[4], sk, bd + 4 * (size_t)b, Kf);
}

}  // namespace
