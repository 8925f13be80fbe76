// kernels_linear.hip -- a softmax linear classifier on gallery embeddings: the row-wise softmax / cross-entropy, the split-K
// fp32 weight-gradient product and the momentum update.  gfx950 (MI355X, CDNA4) only.  Replaces, for a classifier trained on
// embeddings, the reference's INNER_PRODUCT layer under SOFTMAX_LOSS: SoftmaxLayer::Forward_cpu (softmax_layer.cpp:25-59),
// SoftmaxWithLossLayer::Forward_cpu / Backward_cpu (softmax_loss_layer.cpp:34-83), InnerProductLayer::Backward_gpu
// (inner_product_layer.cu:29-59: dW = dz^T X, db = dz^T 1) and SGDSolver::ComputeUpdateValue (solver.cpp:485-531, L2).
// The logits' product is k_sim_f32 (kernels_retrieval.hip) as it stands: this file reads the float it stored, times -0.5f.
// k_hinge, at the end, is the same layer under HINGE_LOSS (hinge_loss_layer.cpp:13-77): a linear SVM per class.
//
// Nothing here adds floats atomically: every sum has one owner and a fixed order, so the same inputs give the same bits.
#include <cfloat>

#include "vv_internal.h"

namespace vv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The logit of column c from the stored similarity s: mul s + b[c].  mul is -0.5f or 1, so the product is exact and the sum is the one
// rounding.  k_softmax_xent and k_hinge both form it here, as the product and then the sum (what k_softmax_xent has always compiled
// to; contraction is off so that no setting at the point of use can fuse the two).
__device__ __forceinline__ float lin_logit(float mul, float s, const float* bias, int c) {
#pragma clang fp contract(off)
  const float p = mul * s;
  return bias ? p + bias[c] : p;
}

// ---------------------------------------------------------------------------------------------- softmax / cross-entropy
// A FIXED grid of LIN_SM_BLOCKS x 256 threads.  A group of `wd` lanes (64, or 32 when cols <= 32: two rows per wave) owns one row at
// a time, rows dealt group by group over the grid.  Three sweeps over the row's stored similarities, each lane its columns
// lane, lane + wd, ... ascending:
//   1  z = mul s + b[c] (mul is -0.5f or 1: the product is exact; one rounding for the bias), the first maximum over the non-NaN logits (strict >,
//      so the lowest column wins a tie; column 0 when there is none) and whether any logit is not finite
//   2  sum of expf(z - max): each lane's terms ascending, then the lanes folded by halves (l += l + wd/2, wd/4, ... 1)
//   3  p = expf(z - max) / sum; dz = (p - [c == label]) * scale; the label's lane forms -logf(max(p, FLT_MIN)) (:46-48)
// expf / logf are OCML's default functions, not the __expf / __logf approximations.  The group's row terms go into a double per
// group, the wave's groups are added in order, the workgroup's waves in order, and the workgroup that arrives last adds the
// LIN_SM_BLOCKS partials in index order into the step's record (k_grad_sumsq's pattern).
__global__ __launch_bounds__(256) void k_softmax_xent(LinSoftmaxArgs a) {
  const int wd = a.wd, lane = threadIdx.x & 63, sub = lane & (wd - 1), gpw = 64 / wd;
  const int64_t group = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * gpw + lane / wd, ngroups = (int64_t)LIN_SM_BLOCKS * 4 * gpw;
  double loss = 0.0;
  unsigned correct = 0, nonfinite = 0;
  for (int64_t r = group; r < a.rows; r += ngroups) {
    const float* s = a.sim + r * a.pitch;
    const int label = a.labels[r];
    float m = -INFINITY;
    int arg = INT32_MAX;
    bool bad = false;
    for (int c = sub; c < a.cols; c += wd) {
      const float z = lin_logit(a.mul, s[c], a.bias, c);
      bad |= !isfinite(z);
      if (z > m) { m = z; arg = c; }
    }
    for (int o = wd >> 1; o > 0; o >>= 1) {
      const float m2 = __shfl_down(m, o, wd);
      const int a2 = __shfl_down(arg, o, wd);
      bad |= __shfl_down((int)bad, o, wd) != 0;
      if (m2 > m || (m2 == m && a2 < arg)) { m = m2; arg = a2; }
    }
    m = __shfl(m, 0, wd); arg = __shfl(arg, 0, wd); bad = __shfl((int)bad, 0, wd) != 0;
    if (arg == INT32_MAX) arg = 0;
    float sum = 0.f;
    for (int c = sub; c < a.cols; c += wd) {
      const float z = lin_logit(a.mul, s[c], a.bias, c);
      sum += expf(z - m);
    }
    for (int o = wd >> 1; o > 0; o >>= 1) sum += __shfl_down(sum, o, wd);
    sum = __shfl(sum, 0, wd);
    float term = 0.f;
    for (int c = sub; c < a.pitch; c += wd) {
      float p = 0.f, d = 0.f;
      if (c < a.cols) {
        const float z = lin_logit(a.mul, s[c], a.bias, c);
        p = expf(z - m) / sum;
        d = (c == label ? p - 1.f : p) * a.scale;                         // :68-81
        if (c == label) term = -logf(fmaxf(p, FLT_MIN));                  // :46-48
      }
      if (a.dz) a.dz[r * a.pitch + c] = d;                                // (the pad columns: zero)
      if (a.prob && c < a.cols) a.prob[r * a.pitch + c] = p;
    }
    term = __shfl(term, label % wd, wd);
    if (sub == 0) {
      if (a.row_loss) { a.row_loss[r] = term; a.row_flags[r] = (arg == label ? 1 : 0) | (bad ? 2 : 0); }
      loss += (double)term; correct += arg == label; nonfinite += bad;
    }
  }
  // the wave's groups in order (only their first lanes carry anything), then the waves, then the workgroups
  if (wd == 32) { loss += __shfl_down(loss, 32, 64); correct += __shfl_down(correct, 32, 64); nonfinite += __shfl_down(nonfinite, 32, 64); }
  __shared__ double wl[LIN_SM_BLOCKS];
  __shared__ unsigned wc[LIN_SM_BLOCKS], wn[LIN_SM_BLOCKS];
  __shared__ int last;
  if (lane == 0) { wl[threadIdx.x >> 6] = loss; wc[threadIdx.x >> 6] = correct; wn[threadIdx.x >> 6] = nonfinite; }
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(a.part_loss + blockIdx.x, ((wl[0] + wl[1]) + wl[2]) + wl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.part_cnt + 2 * blockIdx.x, wc[0] + wc[1] + wc[2] + wc[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.part_cnt + 2 * blockIdx.x + 1, wn[0] + wn[1] + wn[2] + wn[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (release: the partials are visible at agent scope before the count; acquire: the last arrival sees every other partial)
    last = __hip_atomic_fetch_add(a.arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)LIN_SM_BLOCKS - 1;
  }
  __syncthreads();
  if (!last) return;
  for (int i = threadIdx.x; i < LIN_SM_BLOCKS; i += 256) {
    wl[i] = __hip_atomic_load(a.part_loss + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wc[i] = __hip_atomic_load(a.part_cnt + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wn[i] = __hip_atomic_load(a.part_cnt + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sl = 0.0;
  int64_t sc = 0, sn = 0;
  for (int i = 0; i < LIN_SM_BLOCKS; ++i) { sl += wl[i]; sc += wc[i]; sn += wn[i]; }
  LinRec& rec = *a.rec;                                                    // (a later row block of the same step adds to the earlier ones')
  if (a.first_block) { rec.loss_sum = sl; rec.correct = sc; rec.nonfinite = sn; }
  else { rec.loss_sum += sl; rec.correct += sc; rec.nonfinite += sn; }
  __hip_atomic_store(a.arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch
}

void launch_softmax_xent(const LinSoftmaxArgs& a, hipStream_t s) { VV_LAUNCH(k_softmax_xent, dim3(LIN_SM_BLOCKS), dim3(256), 0, s, a); }

// out [rows][cols] = -0.5f sim [rows][pitch] + bias: the logits as vv_linear_scores hands them out
__global__ __launch_bounds__(256) void k_lin_scores_out(const float* sim, int64_t pitch, int64_t rows, int cols, const float* bias, float* out) {
  const int64_t n = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    const float z = -0.5f * sim[r * pitch + c];
    out[i] = bias ? z + bias[c] : z;
  }
}
void launch_lin_scores_out(const float* sim, int64_t pitch, int64_t rows, int cols, const float* bias, float* out, hipStream_t s) {
  const int64_t n = rows * cols;
  hipLaunchKernelGGL(k_lin_scores_out, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, sim, pitch, rows, cols, bias, out);
}

// ---------------------------------------------------------------------------------------------- weight gradient
// out [m][n] = A^T B for A [k][m] and B [k][n], both k-major as they lie in memory (dz and the gallery rows), exact fp32 through
// v_mfma_f32_32x32x2_f32.  That instruction takes ONE float per lane and operand -- lane l: A[i = l & 31][kk = l >> 5],
// B[kk = l >> 5][j = l & 31] -- so with k-major operands a lane's element of either one is (row k0 + (l >> 5), column base + (l & 31))
// of the matrix as stored: 32 consecutive floats per half wave, for both.  Neither operand is transposed anywhere; the LDS image
// of a K-tile is the [32][128] block as it lies in memory (rows of 512 bytes, written and read conflict-free).
// 128 x 128 output tile per 256-thread workgroup, wave w the 64 x 64 sub-tile (w >> 1, w & 1) as 2 x 2 accumulators, K advanced 32
// at a time, the registers loaded one K-tile ahead of the MFMAs (k_sim_f32's structure).  Split s of K covers rows
// [s split_rows, (s + 1) split_rows) and owns slab s; workgroups of one split are neighbours in the grid, so B comes from HBM
// once per split.  accumulate: the slab's element is read and the sum written back (a later row block of one batch).
// dbs: the workgroups of the first column tile also add the columns of A over their split's rows, ascending -> dbs [S][m].
#define LW_LOAD4(dst, M, ld, row, col, ncols, vec) LW_LOAD4_FROM(dst, M, ld, row, row, col, ncols, vec)
// (row: the K row that is tested against k_end; src: the row of M it is read from -- `row` itself, or the list's index for it)
#define LW_LOAD4_FROM(dst, M, ld, row, src, col, ncols, vec)                                           \
  do {                                                                                                 \
    dst = make_float4(0.f, 0.f, 0.f, 0.f);                                                             \
    if ((row) < k_end) {                                                                               \
      const float* p_ = (M) + (src) * (ld) + (col);                                                    \
      if ((vec) && (col) + 3 < (ncols)) dst = *(const float4*)p_;                                      \
      else {                                                                                           \
        if ((col) < (ncols)) dst.x = p_[0];                                                            \
        if ((col) + 1 < (ncols)) dst.y = p_[1];                                                        \
        if ((col) + 2 < (ncols)) dst.z = p_[2];                                                        \
        if ((col) + 3 < (ncols)) dst.w = p_[3];                                                        \
      }                                                                                                \
    }                                                                                                  \
  } while (0)

// ROWS: row kk of B is B + rowidx[kk] * ldb (a row list, linear.hip); A stays contiguous, it was produced in list order.  A thread's four
// indices of a K-tile (ix0 .. ix3: named registers, as the row registers are) are loaded ONE TILE BEFORE the row loads that use them --
// TWO tiles ahead of the MFMAs -- so the K loop never waits on index -> row.  A row at or past k_end reads no index and stays zero.
// The fmaf chain, the splits, the slabs and dbs are untouched: the same bits as the contiguous product over the same row values.
template <bool ROWS>
__global__ __launch_bounds__(256) void k_lin_wgrad_t(LinWgradArgs a) {
  __shared__ __attribute__((aligned(16))) float sA[LIN_BK * LIN_BM];
  __shared__ __attribute__((aligned(16))) float sB[LIN_BK * LIN_BN];
  const int mtiles = (a.m + LIN_BM - 1) / LIN_BM, ntiles = (a.n + LIN_BN - 1) / LIN_BN, tiles = mtiles * ntiles;
  const int tile = (int)(blockIdx.x % tiles), split = (int)(blockIdx.x / tiles);
  const int m0 = (tile % mtiles) * LIN_BM, n0 = (tile / mtiles) * LIN_BN;
  const int64_t k_begin = (int64_t)split * a.split_rows, k_end = std::min<int64_t>(a.k, k_begin + a.split_rows);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  // thread t stages float4 (t & 31) of rows (t >> 5) + 8 i, i = 0..3, of both tiles
  const int srow = tid >> 5, c4 = (tid & 31) * 4, lo = srow * LIN_BM + c4;
  const int ca = m0 + c4, cb = n0 + c4;
  // a whole tile inside both matrices on 16-byte rows: the K loop's loads carry no column tests
  const bool fast = a.vec_a && a.vec_b && m0 + LIN_BM <= a.m && n0 + LIN_BN <= a.n;
  float4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
  int64_t ix0 = 0, ix1 = 0, ix2 = 0, ix3 = 0;            // ROWS: the list's entries for rows kr, kr + 8, kr + 16, kr + 24 of the tile staged NEXT
  // a whole tile inside the split: four plain loads; else each entry under its own row test, so nothing at or past k_end is read
#define LW_INDEX(k0)                                                                                                        \
  do {                                                                                                                      \
    if constexpr (ROWS) {                                                                                                   \
      const int64_t kr = (k0) + srow;                                                                                       \
      if ((k0) + LIN_BK <= k_end) { ix0 = a.rowidx[kr]; ix1 = a.rowidx[kr + 8]; ix2 = a.rowidx[kr + 16]; ix3 = a.rowidx[kr + 24]; } \
      else {                                                                                                                \
        ix0 = kr < k_end ? a.rowidx[kr] : 0; ix1 = kr + 8 < k_end ? a.rowidx[kr + 8] : 0;                                   \
        ix2 = kr + 16 < k_end ? a.rowidx[kr + 16] : 0; ix3 = kr + 24 < k_end ? a.rowidx[kr + 24] : 0;                       \
      }                                                                                                                     \
    }                                                                                                                       \
  } while (0)
#define LW_STAGE(k0)                                                                                                        \
  do {                                                                                                                      \
    const int64_t kr = (k0) + srow;                                                                                         \
    if (fast && (k0) + LIN_BK <= k_end) {                                                                                   \
      if constexpr (ROWS) {                                                                                                 \
        const float* pa = a.A + kr * a.lda + ca;                                                                            \
        ra0 = *(const float4*)pa; ra1 = *(const float4*)(pa + 8 * a.lda); ra2 = *(const float4*)(pa + 16 * a.lda); ra3 = *(const float4*)(pa + 24 * a.lda); \
        rb0 = *(const float4*)(a.B + ix0 * a.ldb + cb); rb1 = *(const float4*)(a.B + ix1 * a.ldb + cb);                     \
        rb2 = *(const float4*)(a.B + ix2 * a.ldb + cb); rb3 = *(const float4*)(a.B + ix3 * a.ldb + cb);                     \
      } else {                                                                                                              \
        const float* pa = a.A + kr * a.lda + ca; const float* pb = a.B + kr * a.ldb + cb;                                   \
        ra0 = *(const float4*)pa; ra1 = *(const float4*)(pa + 8 * a.lda); ra2 = *(const float4*)(pa + 16 * a.lda); ra3 = *(const float4*)(pa + 24 * a.lda); \
        rb0 = *(const float4*)pb; rb1 = *(const float4*)(pb + 8 * a.ldb); rb2 = *(const float4*)(pb + 16 * a.ldb); rb3 = *(const float4*)(pb + 24 * a.ldb); \
      }                                                                                                                     \
    } else {                                                                                                                \
      LW_LOAD4(ra0, a.A, a.lda, kr, ca, a.m, a.vec_a); LW_LOAD4(ra1, a.A, a.lda, kr + 8, ca, a.m, a.vec_a);                 \
      LW_LOAD4(ra2, a.A, a.lda, kr + 16, ca, a.m, a.vec_a); LW_LOAD4(ra3, a.A, a.lda, kr + 24, ca, a.m, a.vec_a);           \
      if constexpr (ROWS) {                                                                                                 \
        LW_LOAD4_FROM(rb0, a.B, a.ldb, kr, ix0, cb, a.n, a.vec_b); LW_LOAD4_FROM(rb1, a.B, a.ldb, kr + 8, ix1, cb, a.n, a.vec_b); \
        LW_LOAD4_FROM(rb2, a.B, a.ldb, kr + 16, ix2, cb, a.n, a.vec_b); LW_LOAD4_FROM(rb3, a.B, a.ldb, kr + 24, ix3, cb, a.n, a.vec_b); \
      } else {                                                                                                              \
        LW_LOAD4(rb0, a.B, a.ldb, kr, cb, a.n, a.vec_b); LW_LOAD4(rb1, a.B, a.ldb, kr + 8, cb, a.n, a.vec_b);               \
        LW_LOAD4(rb2, a.B, a.ldb, kr + 16, cb, a.n, a.vec_b); LW_LOAD4(rb3, a.B, a.ldb, kr + 24, cb, a.n, a.vec_b);         \
      }                                                                                                                     \
    }                                                                                                                       \
  } while (0)
  LW_INDEX(k_begin);
  LW_STAGE(k_begin);
  if (k_begin + LIN_BK < k_end) LW_INDEX(k_begin + LIN_BK);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // 32-row groups of the tile that lie wholly past m / n do no MFMAs (wave-uniform)
  const bool am1 = m0 + wm * 64 + 32 < a.m, bn1 = n0 + wn * 64 + 32 < a.n;
  const bool am0 = m0 + wm * 64 < a.m, bn0 = n0 + wn * 64 < a.n;
  const bool colsum = a.dbs && n0 == 0 && tid < LIN_BM;
  float dbacc = 0.f;

  for (int64_t k0 = k_begin; k0 < k_end; k0 += LIN_BK) {
    __syncthreads();                                   // the previous tile's fragment reads are done
    *(float4*)&sA[lo] = ra0; *(float4*)&sA[lo + 8 * LIN_BM] = ra1; *(float4*)&sA[lo + 16 * LIN_BM] = ra2; *(float4*)&sA[lo + 24 * LIN_BM] = ra3;
    *(float4*)&sB[lo] = rb0; *(float4*)&sB[lo + 8 * LIN_BN] = rb1; *(float4*)&sB[lo + 16 * LIN_BN] = rb2; *(float4*)&sB[lo + 24 * LIN_BN] = rb3;
    __syncthreads();
    if (k0 + LIN_BK < k_end) {
      LW_STAGE(k0 + LIN_BK);
      if (k0 + 2 * LIN_BK < k_end) LW_INDEX(k0 + 2 * LIN_BK);
    }
    if (colsum) {
#pragma unroll
      for (int kk = 0; kk < LIN_BK; ++kk) dbacc += sA[kk * LIN_BM + tid];      // (rows past k_end are zero)
    }
    if (am0 && bn0) {
#pragma unroll
      for (int kk = 0; kk < LIN_BK / 2; ++kk) {
        const float* pa = &sA[(2 * kk + h) * LIN_BM + wm * 64 + r];
        const float* pb = &sB[(2 * kk + h) * LIN_BN + wn * 64 + r];
        const float a0 = pa[0], a1 = pa[32], b0 = pb[0], b1 = pb[32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        if (bn1) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        if (am1) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        if (am1 && bn1) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
  }
#undef LW_STAGE
#undef LW_INDEX
  // C/D map of the 32x32 MFMA: column (n) = lane & 31, row (m) = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
  float* slab = a.slabs + (int64_t)split * a.slab_stride;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (row < a.m && col < a.n) {
          float* o = slab + (int64_t)row * a.n + col;
          *o = a.accumulate ? *o + acc[i][j][e] : acc[i][j][e];
        }
      }
    }
  if (colsum && m0 + tid < a.m) {
    float* o = a.dbs + (int64_t)split * a.m + m0 + tid;
    *o = a.accumulate ? *o + dbacc : dbacc;
  }
}
#undef LW_LOAD4
#undef LW_LOAD4_FROM

constexpr auto k_lin_wgrad = k_lin_wgrad_t<false>;          // the contiguous form: the launch vv_linear_fit and vv_op_gemm_tn have always run
constexpr auto k_lin_wgrad_rows = k_lin_wgrad_t<true>;

void launch_lin_wgrad(const LinWgradArgs& a, hipStream_t s) {
  const int tiles = ((a.m + LIN_BM - 1) / LIN_BM) * ((a.n + LIN_BN - 1) / LIN_BN);
  if (a.rowidx) VV_LAUNCH(k_lin_wgrad_rows, dim3((unsigned)(tiles * a.S)), dim3(256), 0, s, a);
  else VV_LAUNCH(k_lin_wgrad, dim3((unsigned)(tiles * a.S)), dim3(256), 0, s, a);
}

// The split plan: a function of (k, m, n, lin_split_rows) and the constants of vv_internal.h, never of the device.
LinPlan lin_plan(int64_t k, int m, int n, int64_t forced_split_rows) {
  LinPlan p;
  const int64_t tiles = (int64_t)((m + LIN_BM - 1) / LIN_BM) * ((n + LIN_BN - 1) / LIN_BN);
  if (forced_split_rows > 0) p.split_rows = forced_split_rows;
  else {
    const int64_t want = std::max<int64_t>(1, LIN_TARGET_BLOCKS / tiles);                 // splits that fill the grid target
    p.split_rows = std::max<int64_t>(LIN_MIN_SPLIT_ROWS, round_up((k + want - 1) / want, LIN_BK));
  }
  p.block_rows = p.split_rows * LIN_MAX_SPLITS;
  const int64_t first = std::min(k, p.block_rows);
  p.S = (int)((first + p.split_rows - 1) / p.split_rows);
  p.blocks = (int)((k + p.block_rows - 1) / p.block_rows);
  return p;
}

// ---------------------------------------------------------------------------------------------- reduction and update
// A FIXED grid of LIN_UPD_BLOCKS x 256 threads over the n4 16-byte items (or, vec == 0, the single elements) of the matrix.
// g = slab 0 + slab 1 + ... in slab order; rule == 0: g is stored (vv_linear_grad, vv_op_gemm_tn); rule == 1, solver.cpp:485-531
// with L2 decay, every product and sum rounded as written:  h = lr (g + wd w) + momentum h;  w = w - h.
// The bias (nb elements, no decay) is the last workgroup's tail, from the splits' column sums in the same order.
#pragma clang fp contract(off)
__device__ __forceinline__ void lin_step(float g, float& w, float& h, float lr, float momentum, float wd) {
  const float t1 = wd * w;
  const float t2 = g + t1;
  const float t3 = lr * t2;
  const float t4 = momentum * h;
  h = t3 + t4;
  w = w - h;
}

__global__ __launch_bounds__(256) void k_lin_update(LinUpdArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)LIN_UPD_BLOCKS * 256;
  if (a.vec) {
    const int64_t n4 = a.nW / 4;
    for (int64_t i = tid; i < n4; i += nth) {
      float4 g = ((const float4*)a.slabs)[i];
      for (int s = 1; s < a.S; ++s) {
        const float4 v = ((const float4*)(a.slabs + (int64_t)s * a.slab_stride))[i];
        g.x += v.x; g.y += v.y; g.z += v.z; g.w += v.w;
      }
      if (a.rule) {
        float4 w = ((float4*)a.W)[i], h = ((float4*)a.hW)[i];
        lin_step(g.x, w.x, h.x, a.lr, a.momentum, a.wd); lin_step(g.y, w.y, h.y, a.lr, a.momentum, a.wd);
        lin_step(g.z, w.z, h.z, a.lr, a.momentum, a.wd); lin_step(g.w, w.w, h.w, a.lr, a.momentum, a.wd);
        ((float4*)a.W)[i] = w; ((float4*)a.hW)[i] = h;
      } else ((float4*)a.W)[i] = g;
    }
  }
  for (int64_t i = (a.vec ? a.nW / 4 * 4 : 0) + tid; i < a.nW; i += nth) {
    float g = a.slabs[i];
    for (int s = 1; s < a.S; ++s) g += a.slabs[(int64_t)s * a.slab_stride + i];
    if (a.rule) { float w = a.W[i], h = a.hW[i]; lin_step(g, w, h, a.lr, a.momentum, a.wd); a.W[i] = w; a.hW[i] = h; }
    else a.W[i] = g;
  }
  if (blockIdx.x != LIN_UPD_BLOCKS - 1) return;
  for (int c = threadIdx.x; c < a.nb; c += 256) {
    float g = a.dbs[c];
    for (int s = 1; s < a.S; ++s) g += a.dbs[(int64_t)s * a.db_stride + c];
    if (a.rule) { float w = a.b[c], h = a.hb[c]; lin_step(g, w, h, a.lr, a.momentum, 0.f); a.b[c] = w; a.hb[c] = h; }
    else a.b[c] = g;
  }
}

void launch_lin_update(const LinUpdArgs& a, hipStream_t s) { VV_LAUNCH(k_lin_update, dim3(LIN_UPD_BLOCKS), dim3(256), 0, s, a); }

// ---------------------------------------------------------------------------------------------- one-vs-rest hinge loss
// HingeLossLayer::Forward_cpu / Backward_cpu (hinge_loss_layer.cpp:13-77): every column of the logits is a binary problem with target
// +1 on the label's column and -1 elsewhere.  Per element, every operation rounded as written (fp contract is off from above):
//   z = lin_logit;  t = c == label ? -z : z (:25);  m = 0 < 1 + t ? 1 + t : 0 (:29-30: a NaN gives 0, +Inf stays)
//   L1: term m (:36), dz = +-[m > 0] scale (:61-69);  L2: term m m (:39), dz = +-m scale (:71);  - on the label's column
// The same FIXED grid of LIN_SM_BLOCKS x 256 threads.  A group of wd = lin_hinge_lanes(cols) lanes (1 .. 64) owns one row at a time;
// a wave's 64 / wd groups take consecutive rows, and all of them run the row loop together.  ONE sweep: lane `sub` of the group
// reads the 4-column chunks sub, sub + wd, ... of the row once (vec: one 16-byte load each; else element by element, the same
// columns), forms z, m, dz and its running first maximum, stores dz (zero at columns cols .. pitch - 1) and adds its terms, columns
// ascending, into ITS double.  The first chunk and the label of the group's next row are loaded before the current row is worked on.
// One fold of (value, column) by halves within the group gives the row's first maximum (strict >, the lower column on a tie, NaN
// passed over, column 0 when there is none); the non-finite flag is one ballot.
// The loss: the lanes' doubles are folded pairwise with neighbours at distance 1, 2, 4 .. 32 (so a group's lanes first, then the wave's
// groups), then the workgroup's waves in order, then the last workgroup to arrive adds the LIN_SM_BLOCKS partials in index order:
// k_softmax_xent's last stage on k_softmax_xent's buffers.  No floating-point atomics.
__device__ __forceinline__ float4 hinge_load(const LinHingeArgs& a, const float* row, int c4) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.vec) {
    if (c4 < a.cols) v = *(const float4*)(row + c4);                      // (pitch % 4 == 0: the chunk lies inside the row)
  } else {
    if (c4 < a.cols) v.x = row[c4];
    if (c4 + 1 < a.cols) v.y = row[c4 + 1];
    if (c4 + 2 < a.cols) v.z = row[c4 + 2];
    if (c4 + 3 < a.cols) v.w = row[c4 + 3];
  }
  return v;
}

struct HingeLane { double sum; float mx; int arg; bool bad; };

__device__ __forceinline__ float hinge_elem(const LinHingeArgs& a, float s, int c, int label, HingeLane& st) {
  const float z = lin_logit(a.mul, s, a.bias, c);
  st.bad |= !isfinite(z);
  if (z > st.mx) { st.mx = z; st.arg = c; }
  const float t = c == label ? -z : z;
  const float u = 1.f + t;
  const float m = 0.f < u ? u : 0.f;
  if (a.norm == 1) {
    st.sum += (double)m;
    return m > 0.f ? (c == label ? -a.scale : a.scale) : 0.f;
  }
  st.sum += (double)m * (double)m;
  return (c == label ? -m : m) * a.scale;
}

__global__ __launch_bounds__(256) void k_hinge(LinHingeArgs a) {
  const int wd = a.wd, lane = threadIdx.x & 63, sub = lane & (wd - 1), gpw = 64 / wd, c0 = sub * 4, cstep = wd * 4;
  const int64_t wave_row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * gpw, pass = (int64_t)LIN_SM_BLOCKS * 4 * gpw;
  const unsigned long long gmask = wd == 64 ? ~0ull : (1ull << wd) - 1;
  HingeLane st;
  st.sum = 0.0;
  unsigned correct = 0, nonfinite = 0;
  float4 cur = make_float4(0.f, 0.f, 0.f, 0.f);
  int label = 0;
  if (wave_row + lane / wd < a.rows) { cur = hinge_load(a, a.sim + (wave_row + lane / wd) * a.pitch, c0); label = a.labels[wave_row + lane / wd]; }
  for (int64_t rb = wave_row; rb < a.rows; rb += pass) {                    // (the same trip count for the whole wave)
    const int64_t r = rb + lane / wd, rn = r + pass;
    const bool active = r < a.rows;
    float4 nxt = make_float4(0.f, 0.f, 0.f, 0.f);
    int label_nxt = 0;
    if (rn < a.rows) { nxt = hinge_load(a, a.sim + rn * a.pitch, c0); label_nxt = a.labels[rn]; }
    st.mx = -INFINITY; st.arg = INT32_MAX; st.bad = false;
    if (active) {
      const float* s = a.sim + r * a.pitch;
      float* d = a.dz ? a.dz + r * a.pitch : nullptr;
      for (int c4 = c0; c4 < a.pitch; c4 += cstep) {
        const float4 v = c4 == c0 ? cur : hinge_load(a, s, c4);
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < a.cols) o.x = hinge_elem(a, v.x, c4, label, st);
        if (c4 + 1 < a.cols) o.y = hinge_elem(a, v.y, c4 + 1, label, st);
        if (c4 + 2 < a.cols) o.z = hinge_elem(a, v.z, c4 + 2, label, st);
        if (c4 + 3 < a.cols) o.w = hinge_elem(a, v.w, c4 + 3, label, st);
        if (d) {
          if (a.vec) *(float4*)(d + c4) = o;
          else {
            d[c4] = o.x;
            if (c4 + 1 < a.pitch) d[c4 + 1] = o.y;
            if (c4 + 2 < a.pitch) d[c4 + 2] = o.z;
            if (c4 + 3 < a.pitch) d[c4 + 3] = o.w;
          }
        }
      }
    }
    float mx = st.mx;
    int arg = st.arg;
    for (int o = wd >> 1; o > 0; o >>= 1) {
      const float m2 = __shfl_down(mx, o, wd);
      const int a2 = __shfl_down(arg, o, wd);
      if (m2 > mx || (m2 == mx && a2 < arg)) { mx = m2; arg = a2; }
    }
    const unsigned long long bad = __ballot(st.bad);
    if (active && sub == 0) {
      correct += (arg == INT32_MAX ? 0 : arg) == label;
      nonfinite += ((bad >> (lane - sub)) & gmask) != 0;
    }
    cur = nxt; label = label_nxt;
  }
  double loss = st.sum;
  for (int o = 1; o < 64; o <<= 1) { loss += __shfl_down(loss, o, 64); correct += __shfl_down(correct, o, 64); nonfinite += __shfl_down(nonfinite, o, 64); }
  __shared__ double wl[LIN_SM_BLOCKS];
  __shared__ unsigned wc[LIN_SM_BLOCKS], wn[LIN_SM_BLOCKS];
  __shared__ int last;
  if (lane == 0) { wl[threadIdx.x >> 6] = loss; wc[threadIdx.x >> 6] = correct; wn[threadIdx.x >> 6] = nonfinite; }
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(a.part_loss + blockIdx.x, ((wl[0] + wl[1]) + wl[2]) + wl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.part_cnt + 2 * blockIdx.x, wc[0] + wc[1] + wc[2] + wc[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.part_cnt + 2 * blockIdx.x + 1, wn[0] + wn[1] + wn[2] + wn[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = __hip_atomic_fetch_add(a.arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)LIN_SM_BLOCKS - 1;
  }
  __syncthreads();
  if (!last) return;
  for (int i = threadIdx.x; i < LIN_SM_BLOCKS; i += 256) {
    wl[i] = __hip_atomic_load(a.part_loss + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wc[i] = __hip_atomic_load(a.part_cnt + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    wn[i] = __hip_atomic_load(a.part_cnt + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sl = 0.0;
  int64_t sc = 0, sn = 0;
  for (int i = 0; i < LIN_SM_BLOCKS; ++i) { sl += wl[i]; sc += wc[i]; sn += wn[i]; }
  LinRec& rec = *a.rec;
  if (a.first_block) { rec.loss_sum = sl; rec.correct = sc; rec.nonfinite = sn; }
  else { rec.loss_sum += sl; rec.correct += sc; rec.nonfinite += sn; }
  __hip_atomic_store(a.arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch
}

void launch_hinge(const LinHingeArgs& a, hipStream_t s) { VV_LAUNCH(k_hinge, dim3(LIN_SM_BLOCKS), dim3(256), 0, s, a); }

}  // namespace vv
