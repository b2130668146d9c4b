// kdpt_wave.h -- whole-wave primitives for gfx950's 64-lane waves (HIP only): lane reads, DPP reductions and
// scans, the wave-level LDS fence, and pair_owner, the owner lane of a flattened (lane, item) pair.
#pragma once

#include "kdpt_math.h"

namespace kdpt {

// number of set bits of mask below this lane
__device__ inline unsigned int lane_prefix(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__device__ inline float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Whole-wave reductions on DPP lane moves (VALU only; HIP's __shfl_* are ds_bpermute, an LDS round trip per
// step).  quad_perm xor 1 and xor 2, then the half-row and row mirrors give every lane its 16-lane row's
// result; row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3) carry the lower rows into row 3, so lane 63
// ends with the whole wave's, read into a scalar register.  Every lane of the wave must be active.
template <int CTRL, int ROWS>
__device__ inline uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xF, false);
}
template <int CTRL, int ROWS>
__device__ inline unsigned long long dpp_u64(unsigned long long v) {
  return ((unsigned long long)dpp_u32<CTRL, ROWS>((uint32_t)(v >> 32)) << 32) | dpp_u32<CTRL, ROWS>((uint32_t)v);
}
__device__ inline unsigned long long readlane_u64(unsigned long long v, int lane) {
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}
__device__ inline unsigned long long lane63_u64(unsigned long long v) {
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
}
#define KDPT_WAVE_REDUCE(STEP) STEP(0xB1, 0xF) STEP(0x4E, 0xF) STEP(0x141, 0xF) STEP(0x140, 0xF) \
                               STEP(0x142, 0xA) STEP(0x143, 0xC)

// Inclusive prefix sum / max over the wave on DPP row shifts and row broadcasts (VALU only): shr 1, 2, 4, 8
// within each 16-lane row, then row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3) carry the rows below.
// Lanes whose source is outside the row, or rows the row mask leaves out, add the identity 0 (values >= 0
// for the max).  Every lane of the wave must be active.
template <bool MAX>
__device__ inline int wave_incl_scan(int v) {
#define KDPT_SCAN(C, R)                                                   \
  {                                                                       \
    const int o = __builtin_amdgcn_update_dpp(0, v, C, R, 0xF, false);    \
    v = MAX ? max(v, o) : v + o;                                          \
  }
  KDPT_SCAN(0x111, 0xF) KDPT_SCAN(0x112, 0xF) KDPT_SCAN(0x114, 0xF) KDPT_SCAN(0x118, 0xF)
  KDPT_SCAN(0x142, 0xA) KDPT_SCAN(0x143, 0xC)
#undef KDPT_SCAN
  return v;
}

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#define KDPT_STEP(C, R) { const unsigned long long o = dpp_u64<C, R>(v); v = o < v ? o : v; }
  KDPT_WAVE_REDUCE(KDPT_STEP)
#undef KDPT_STEP
  return lane63_u64(v);
}

__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
#define KDPT_STEP(C, R) { const unsigned long long o = dpp_u64<C, R>(v); v = o > v ? o : v; }
  KDPT_WAVE_REDUCE(KDPT_STEP)
#undef KDPT_STEP
  return lane63_u64(v);
}
__device__ inline int wave_max_i32(int v) {
#define KDPT_STEP(C, R) v = max(v, (int)dpp_u32<C, R>((uint32_t)v));
  KDPT_WAVE_REDUCE(KDPT_STEP)
#undef KDPT_STEP
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline float bpermute_f(float v, int src_lane) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}

// Position of the j-th (0-based) set bit of m (j < popcount(m)): a 6-step bisection on popcounts.
__device__ inline int select_bit(unsigned long long m, int j) {
  uint32_t x = (uint32_t)m;
  int base = 0, c = __popc(x);
  if (j >= c) {
    j -= c;
    x = (uint32_t)(m >> 32);
    base = 32;
  }
#pragma unroll
  for (int w = 16; w >= 1; w >>= 1) {
    c = __popc(x & ((1u << w) - 1u));
    if (j >= c) {
      j -= c;
      x >>= w;
      base += w;
    }
  }
  return base;
}

// Owner lane of pair B + lane in a flattened (lane, item) enumeration where lane L owns pairs
// [excl_L, excl_L + cnt_L) (lanes in order, so starts increase with L).  The segment starts inside the
// window [B, B + 64) are scattered into slot[] (lane + 1), an inclusive max-scan fills the gaps, and a
// window position no start precedes belongs to the previous window's last owner (carry, updated).  Replaces
// a 6-step binary search (6 dependent LDS reads) by one LDS round trip plus DPP.  Wave-uniform call; slot[]
// is all zero on entry and on exit.
__device__ inline int pair_owner(int* slot, int excl, int cnt, int B, int& carry) {
  const int lane = threadIdx.x & 63;
  const int rel = excl - B;
  const bool mine = cnt > 0 && rel >= 0 && rel < 64;
  if (mine) slot[rel] = lane + 1;
  wave_lds_sync();
  const int v = wave_incl_scan<true>(slot[lane]);
  if (mine) slot[rel] = 0;  // after the read above (same wave: LDS operations stay in order)
  const int own = v > 0 ? v - 1 : carry;
  carry = __builtin_amdgcn_readlane(own, 63);
  return own;
}

}  // namespace kdpt
