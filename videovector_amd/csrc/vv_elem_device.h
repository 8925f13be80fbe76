// vv_elem_device.h -- device helpers shared by kernels_score.hip and kernels_update.hip (and included by nothing else): the wave and
// workgroup sums.  A helper that one file alone uses stays in that file.
#pragma once
#include <hip/hip_runtime.h>

namespace vv {

// Sum over the 64 lanes with DPP row shifts / row broadcasts (no LDS crossbar traffic, six fused add+DPP
// instructions against twelve bpermute + add for the xor butterfly); the total is valid in LANE 63 only.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, true);
  return v + __builtin_bit_cast(float, moved);
}
__device__ __forceinline__ float wave_sum63(float v) {
  v = dpp_add<0x111, 0xF>(v);    // row_shr:1
  v = dpp_add<0x112, 0xF>(v);    // row_shr:2
  v = dpp_add<0x114, 0xF>(v);    // row_shr:4
  v = dpp_add<0x118, 0xF>(v);    // row_shr:8   -> lane 15 of every row holds the row's sum
  v = dpp_add<0x142, 0xA>(v);    // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xC>(v);    // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's sum
  return v;
}

// block-wide sum for 256 threads; red must hold >= 4 floats; result broadcast to all threads
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum63(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

}  // namespace vv
