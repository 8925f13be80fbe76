// kernels_gemm.hip -- the GEMM launch dispatch of the videovec training step (gfx950 only) and the round-1
// weight-gradient kernel.  The product kernels are the phase-staggered ones of kernels_gemm_ph.hip.
//
//   k_wgrad_gemm : dW = dY^T X (split-K partial slabs), X gathered through the triplet index.
//                  Replaces InnerProductLayer::Backward's weight gradient
//                  (inner_product_layer.cu:36-42).
//                  Kept for option wgrad_tr = 0: its fragment loader reads LDS eight 16-bit values at a
//                  time (slow, layout-obvious), the reference the transposed LDS reads of
//                  k_wgrad_gemm_ph are checked against bit for bit.
//
// 256x256 output tile per 512-thread workgroup, K advanced 64 at a time, operand tiles brought
// HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, 16 B per lane; the gather is simply the
// per-lane source address), double buffered; 8 waves x (8x4) MFMA 16x16x32 accumulators.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "vv_internal.h"

namespace vv {

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
  // LDS destination = wave-uniform base + lane * 16 (hardware rule); source is per lane.
  __builtin_amdgcn_global_load_lds(GLB_PTR(gsrc), LDS_PTR(lds_wave_base), 16, 0, 0);
}

__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  // Blocks b and b+8 share an XCD (round-robin dispatch): give each XCD a contiguous run of
  // logical tiles so tiles that share operand rows also share an L2.  Speed only.
  const int x = bid & 7, q = nblk >> 3, rem = nblk & 7;
  return x * q + (x < rem ? x : rem) + (bid >> 3);
}

// ------------------------------------------------------------------------------- wgrad --------
// LDS operand image: [64 k-rows][256 halves] = 512-B rows of 32 16-B chunks, both operands
// k-major exactly as they sit in HBM (dY rows / gathered feature rows).  MFMA fragments need 8
// consecutive k for one m (or n).  chunk' = chunk ^ (h(row) << 1), h = (row&3) | ((row>>3)&1)<<2:
// the image k_wgrad_gemm_ph's transposed reads use (tools/lds_banks.py).
__device__ __forceinline__ int wg_h(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

template <typename T>
__global__ __launch_bounds__(GEMM_THREADS) void k_wgrad_gemm(WgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int tilesM = a.Dp / BM, tilesN = a.Fp / BN;
  // logical order: tm fastest (the two M tiles of one (split, tn) read the same feature bytes)
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int tm = L % tilesM, tn = (L / tilesM) % tilesN, sp = L / (tilesM * tilesN);
  const int m0 = tm * BM, n0 = tn * BN;
  int total_steps = a.Rp / BK, kps = a.ksteps_per_split;
  if (a.n_dev) {                      // dedup mode: live K extent in device memory
    total_steps = (*a.n_dev + BK - 1) / BK;
    kps = (total_steps + a.S - 1) / a.S;
  }
  const int k_begin = sp * kps;
  int k_end = k_begin + kps;
  if (k_end > total_steps) k_end = total_steps;
  const int nk = k_end > k_begin ? k_end - k_begin : 0;

  int srow[4], slc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = (i * 8 + wave) * 64 + lane;
    srow[i] = c >> 5;
    slc[i] = (c & 31) ^ (wg_h(srow[i]) << 1);
  }

  f32x4 acc[8][4];
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  int32_t rid[4];   // table rows of the NEXT k-step to stage
  auto load_ids = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rid[i] = a.rows[(int64_t)(k_begin + kt) * BK + srow[i]];
  };
  auto stage = [&](int p, int kt) {
    unsigned char* As = smem + p * 2 * LDS_TILE_BYTES;
    unsigned char* Bs = As + LDS_TILE_BYTES;
    const int64_t kg = (int64_t)(k_begin + kt) * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16(a.dYh + (kg + srow[i]) * a.Dp + m0 + slc[i] * 8, As + (i * 8 + wave) * 1024);
      glds16(a.table + (int64_t)rid[i] * a.Fp + n0 + slc[i] * 8, Bs + (i * 8 + wave) * 1024);
    }
  };

  if (nk > 0) {
    load_ids(0);
    stage(0, 0);
    if (nk > 1) load_ids(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  const int g = lane >> 4, li = lane & 15;
  for (int t = 0; t < nk; ++t) {
    const int p = t & 1;
    if (t + 1 < nk) {
      stage(p ^ 1, t + 1);
      if (t + 2 < nk) load_ids(t + 2);
    }
    const unsigned char* As = smem + p * 2 * LDS_TILE_BYTES;
    const unsigned char* Bs = As + LDS_TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      i16x8 af[8], bf[4];
      // reference fragment loader: eight 16-bit LDS reads per fragment (slow, layout-obvious)
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        const int col = wm * 128 + mi * 16 + li;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int row = kk * 32 + 8 * g + j;
          af[mi][j] = *(const short*)(As + row * 512 + (((col >> 3) ^ (wg_h(row) << 1)) << 4) +
                                      (col & 7) * 2);
        }
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int col = wn * 64 + ni * 16 + li;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int row = kk * 32 + 8 * g + j;
          bf[ni][j] = *(const short*)(Bs + row * 512 + (((col >> 3) ^ (wg_h(row) << 1)) << 4) +
                                      (col & 7) * 2);
        }
      }
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = T::mfma(bf[ni], af[mi], acc[mi][ni]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // swapped operands (D' = X_tile^T dY_tile): lane column = m (output row d), registers = 4
  // consecutive n (feature columns) -> 16-B stores into the split's fp32 slab.
  float* slab = a.slabs + (int64_t)sp * slab_pitch(a.Dp, a.Fp);
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
    const int m = m0 + wm * 128 + mi * 16 + li;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wn * 64 + ni * 16 + g * 4;
      *(float4*)(slab + (int64_t)m * a.Fp + n) =
          make_float4(acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]);
    }
  }
}

// ------------------------------------------------------------------------------- launchers ----
// VV_ABLATE (lab builds only, KernelOpts) applies to the phase-staggered kernels.
bool ablate_on() { return ko().ablate != 0; }

void launch_fwd_gemm_ph(int prec, const FwdArgs& a, hipStream_t s);
void launch_fwd_gemm(int prec, const FwdArgs& a, hipStream_t s) {
  FwdArgs b = a; b.abl = ko().ablate; launch_fwd_gemm_ph(prec, b, s);
}

template <typename T>
static void launch_wgrad_t(const WgradArgs& a, hipStream_t s) {
  static bool once = ((void)hipFuncSetAttribute((const void*)k_wgrad_gemm<T>,
                      hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_BYTES), true);
  (void)once;
  const dim3 grid((a.Dp / BM) * (a.Fp / BN) * a.S), block(GEMM_THREADS);
  VV_LAUNCH((k_wgrad_gemm<T>), grid, block, GEMM_LDS_BYTES, s, a);
}

void launch_wgrad_gemm_ph(int prec, const WgradArgs& a, hipStream_t s);
// the update in the epilogue (WgradArgs::fuse_upd) exists in the phase-staggered kernel only: pass.hip asks (BackwardPlanIn::can_fuse_update) before it fills WgradUpd
bool wgrad_can_fuse_update() { return ko().wgrad_tr != 0 && !ko().ablate && !ko().lab_wg_abl; }
void launch_wgrad_gemm(int prec, const WgradArgs& a, hipStream_t s) {
  ko().last_wgrad_splits = a.S;           // ("last_wgrad_splits": both kernels' grids are built from this S)
  if (ko().wgrad_tr != 0) {
    // (lab: VV_LAB_WG_ABL ablates this kernel alone, at whatever size the step runs -- VV_ABLATE switches the de-duplication off)
    WgradArgs b = a; b.abl = ko().ablate ? ko().ablate : ko().lab_wg_abl; launch_wgrad_gemm_ph(prec, b, s); return;
  }
  if (prec == 0) launch_wgrad_t<F16>(a, s); else launch_wgrad_t<BF16>(a, s);
}

}  // namespace vv
