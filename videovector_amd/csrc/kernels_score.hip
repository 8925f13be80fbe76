// kernels_score.hip -- the score / loss kernels of the videovec training step and the segment-wise backward (gfx950 only).
//
//   k_score_loss : everything between ip2 and the loss, forward AND backward, one workgroup per
//                  batch item: context mean, the two L2 normalisations, the (1+Nn) dot-product
//                  scores, max-margin loss + violations, and the gradient w.r.t. ip1_nonorm.
//                  Replaces SLICE dim 0, ELTWISE SUM, NORMALIZATION x2, CONCAT, ELTWISE PROD x(1+Nn),
//                  SUM x(1+Nn), CONCAT dim 1, MAX_MARGIN_LOSS (CPU-only in the reference), SPLIT,
//                  and all their backward passes + ReLU/Dropout backward
//                  (reference: eltwise_layer.cu:34-119, normalization_layer.cu:10-97,
//                  sum_layer.cu:10-55, max_margin_loss_layer.cpp:53-214, split_layer.cu:18-33,
//                  relu_layer.cu:36-59, dropout_layer.cu:44-73).
//   k_score_loss_reg : its register-resident form for small (1+Nn) x D.
//   k_score_fwd / k_score_stream + k_seg_bwd / k_seg_bwd_cnt : the same graph for de-duplicated batches, the backward segment by
//                  segment of the shared rows (each described where it is defined).
//   k_final_loss / k_eval_loss : the loss reductions of the training pass and of the forward-only pass.
#include "../../include/videovec.h"
#include "vv_internal.h"
#include "vv_elem_device.h"

namespace vv {

constexpr int SL_THREADS = 256;

// Item of a workgroup in the item-major kernels (one workgroup per batch item).  Workgroups b, b + 8, ... share an XCD (and its L2): instead
// of dealing the items round-robin, XCD x takes the contiguous items [x B/8, (x+1) B/8) -- neighbouring items' own rows (target, context)
// are neighbouring rows of the de-duplicated H, so an XCD's L2 sees runs instead of every eighth row: k_score_fwd 26.5 -> 25.2 us at the benchmark's batch
// (bit-identical results: only which workgroup takes which item changes).  (rr: the lab's switch back to round-robin.)
__device__ __forceinline__ int item_of_block(int rr) {
  const int n = (int)gridDim.x, bid = (int)blockIdx.x;
  if (rr || (n & 7)) return bid;
  return (bid & 7) * (n >> 3) + (bid >> 3);
}

// ------------------------------------------------------------------------------- score/loss ---
// Rows of item b: r = b*CN + ch, ch 0 = target, 1..C-1 = context, C.. = negatives.
// Math:
//   A = sum_j c_j H[j],  Ah = A/(|A|+eps)
//   per q in {0, C..}: n_q = |H[q]|, t_q = Ah.H[q], score_q = t_q/(n_q+eps)
//   d_k = s+ - s-_k, h = max(0, margin - d), loss += w_b h^2 (L2) or w_b |h| (L1), viol += d < 0
//   g_k = grad_scale * w_b * (2h | [h>0]);  c_0 = -sum_k g_k, c_{C+k} = g_k
//   dAh = sum_q c_q H[q]/(n_q+eps);   dH[q] = c_q (n_q^2 Ah - H[q] t_q)/(n_q^3 + eps)
//   dA  = (sA dAh - A (A.dAh))/(sA^1.5 + eps), dH[j] = c_j dA
//   dY  = dH * drop_scale * [H > 0]
// block-wide sums over NW waves; red must hold >= 3 * NW floats; results broadcast to all threads
template <int NW>
__device__ __forceinline__ float block_sum_w(float v, float* red) {
  v = wave_sum63(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) s += red[w];
  return s;
}
// NT threads per item: 256 (four waves) where a batch brings a thousand items; 1024 for wide rows in small batches (the reference's
// shipped configuration: 128 items of 15 rows x 4096 columns -- with four waves per item half of the chip's SIMDs had no wave at all
// and every row was one wave's serial chain of loads: 55 us for 47 MB)
// FWD (ScoreArgs::fwd_only, vv_forward): the forward-only instantiation -- phases 1 to 3, then every workgroup leaves: scores, loss and violation
// partials; nothing of the backward is computed or stored (dYh, dbp, the guard's slots).  The exit is a RUN-TIME test of a.fwd_only that only this
// instantiation carries, not a truncated body: with phases 4 and 5 cut off at compile time the vectoriser formed phase 2's sums differently
// (fma chains where the training kernel has packed multiplies and adds) and the target score moved by one ulp -- the pass must give the
// training pass's bits.  FWD = false is the kernel as it always was, instruction for instruction.
template <typename T, bool VEC, int NT = SL_THREADS, bool FWD = false>
__global__ __launch_bounds__(NT) void k_score_loss(ScoreArgs a) {
  constexpr int NWV = NT / 64;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = a.D, C = a.C, Nn = a.Nn, CN = C + Nn;
  float* A = sm;               // [D] context mean
  float* Ah = A + D;           // [D] normalised context mean
  const int PD = D > 4 * NT ? D : 4 * NT;   // (phase 4: G row groups of D columns, G D <= 4 NT when D / 4 < NT -- score_loss_lds() sizes the same)
  float* acc0 = Ah + D;        // [G][D] row-group partial dAh (G*D <= PD)
  float* acc1 = acc0 + PD;     // [G][D] row-group partial db
  float* n2 = acc1 + PD;       // [CN] squared norms
  float* tq = n2 + CN;         // [CN] dots with Ah
  float* cq = tq + CN;         // [CN] upstream coefficients
  float* red = cq + CN;        // [16]
  int* hoff = (int*)(red + 16); // [CN] row of H holding channel ch (dedup: the shared per-slot row)
  int* ooff = hoff + CN;       // [CN] row of dYh receiving channel ch's gradient
  float* k1 = (float*)(ooff + CN);   // [CN] per-row constants of the backward pass (see phase 4)
  float* k2 = k1 + CN;
  float* k3 = k2 + CN;
  const int b = item_of_block(a.items_rr), tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float eps = 1e-10f;
  __shared__ float ggs[16];
  float sgm;
  if (!gg_begin(a.guard, ggs, sgm)) return;
  const float sg = a.sg * sgm;
  for (int ch = tid; ch < CN; ch += NT) {
    const int r = b * CN + ch;
    hoff[ch] = a.map ? a.map[r] : r;
    ooff[ch] = a.map ? a.seg_start[a.map[r]] + a.ord[r] : r;
  }
  __syncthreads();
#define HROW(ch) (a.H + (int64_t)hoff[ch] * D)

  // ---- phase 1: context mean (column-parallel) and its norm
  float ssq = 0.f;
  for (int d = tid; d < D; d += NT) {
    float s = 0.f;
    for (int j = 1; j < C; ++j) s += a.coeff[j - 1] * HROW(j)[d];
    A[d] = s;
    ssq += s * s;
  }
  const float sA = block_sum_w<NWV>(ssq, red);
  const float nA = sqrtf(sA) + eps;
  for (int d = tid; d < D; d += NT) {
    Ah[d] = A[d] / nA;
  }
  __syncthreads();

  // ---- phase 2: norms and dots of target / negative rows (one row per wave at a time)
  for (int qi = wave; qi < 1 + Nn; qi += NWV) {
    const int ch = qi == 0 ? 0 : C + qi - 1;
    const float* h = HROW(ch);
    float s = 0.f, t = 0.f;
    if (VEC) {
      for (int d = lane * 4; d < D; d += 256) {
        const float4 x = *(const float4*)(h + d);
        const float4 y = *(const float4*)(Ah + d);
        s += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
        t += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
      }
    } else {
      for (int d = lane; d < D; d += 64) { const float x = h[d]; s += x * x; t += x * Ah[d]; }
    }
    s = wave_sum63(s); t = wave_sum63(t);
    if (lane == 63) { n2[ch] = s; tq[ch] = t; }
  }
  __syncthreads();

  // ---- phase 3: scores, hinge, loss, coefficients
  const float sp = tq[0] / (sqrtf(n2[0]) + eps);
  const float wb = a.item_w ? a.item_w[b] : 1.f;
  float lsum = 0.f, vsum = 0.f, gsum = 0.f;
  for (int k = tid; k < Nn; k += NT) {
    const int ch = C + k;
    const float sn = tq[ch] / (sqrtf(n2[ch]) + eps);
    const float d = sp - sn;
    const float h = fmaxf(0.f, a.margin - d);
    float g;     // wb: max_margin_loss_layer.cpp:82-97 (sqrt(w)*h squared, or w*h) and :152-186
    if (a.norm == 2) { lsum += wb * h * h; g = 2.f * wb * h * a.grad_scale; }
    else { lsum += wb * fabsf(h); g = h > 0.f ? wb * a.grad_scale : 0.f; }
    vsum += d < 0.f ? 1.f : 0.f;
    gsum += g;
    cq[ch] = g;
    if (a.s_bogus) a.s_bogus[(int64_t)b * Nn + k] = sn;
  }
  lsum = block_sum_w<NWV>(lsum, red);
  vsum = block_sum_w<NWV>(vsum, red);
  gsum = block_sum_w<NWV>(gsum, red);
  if (tid == 0) {
    cq[0] = -gsum;
    a.loss_part[b] = lsum;
    a.viol_part[b] = vsum;
    if (a.s_true) a.s_true[b] = sp;
    // workgroup 0 is in the kernel's first round: "this step's forward GEMM has finished" (placed here, where few values
    // are live: at the kernel's head it cost the RPW 7 form six registers and, at 133, an occupancy step)
    if (a.gate_host && b == 0) __hip_atomic_store(a.gate_host, a.gate_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if constexpr (FWD) { if (a.fwd_only) return; }      // the forward-only pass ends here (a run-time exit: see FWD above)
  __syncthreads();
  // per-row constants, once per row instead of once per (row, column group): g*sg = k1*Ah - k2*x, dAh += k3*x
  for (int qi = tid; qi < 1 + Nn; qi += NT) {
    const int ch = qi == 0 ? 0 : C + qi - 1;
    const float c = cq[ch], s = n2[ch], rs = sqrtf(s);
    const float cd = c * __builtin_amdgcn_rcpf(s * rs + eps) * a.drop_scale * sg;
    k1[ch] = cd * s; k2[ch] = cd * tq[ch]; k3[ch] = c * __builtin_amdgcn_rcpf(rs + eps);
  }
  __syncthreads();

  // ---- phase 4: backward of the normalised target / negative rows, column-parallel: a thread
  // owns one group of W consecutive columns (16-B loads) and walks the rows of its row group,
  // keeping its dAh / db partial sums in registers (deterministic order, no atomics).
  float gmx = 0.f;                            // max |g| in scaled units before rounding (f16 gradient-scale guard)
  constexpr int W = VEC ? 4 : 1;
  const int Dv = D / W;                       // column groups
  const int Dvp = Dv < NT ? Dv : NT;
  const int G = NT / Dvp;             // row groups running side by side
  if (tid < G * Dvp) {
    const int rg = tid / Dvp;
    for (int cg = tid % Dvp; cg < Dv; cg += Dvp) {
      const int d = cg * W;
      float ya[W], pa[W], pb[W];
#pragma unroll
      for (int e = 0; e < W; ++e) { ya[e] = Ah[d + e]; pa[e] = 0.f; pb[e] = 0.f; }
      for (int qi = rg; qi < 1 + Nn; qi += G) {
        const int ch = qi == 0 ? 0 : C + qi - 1;
        const float r1 = k1[ch], r2 = k2[ch], r3 = k3[ch];
        const float* h = HROW(ch) + d;
        float xv[W];
        if (VEC) { const float4 x = *(const float4*)h; xv[0] = x.x; xv[1 % W] = x.y; xv[2 % W] = x.z; xv[3 % W] = x.w; }
        else xv[0] = h[0];
        uint16_t* dy = a.dYh + (int64_t)ooff[ch] * a.Dp + d;
        uint16_t o[W];
#pragma unroll
        for (int e = 0; e < W; ++e) {
          pa[e] += r3 * xv[e];
          float g = r1 * ya[e] - r2 * xv[e];            // already times sg (a power of two: exact)
          g = xv[e] > 0.f ? g : 0.f;
          pb[e] += g;
          gmx = fmaxf(gmx, fabsf(g));
          o[e] = T::from_float(g);
        }
        if (VEC) *(uint2*)dy = make_uint2(o[0] | ((uint32_t)o[1 % W] << 16), o[2 % W] | ((uint32_t)o[3 % W] << 16));
        else dy[0] = o[0];
      }
#pragma unroll
      for (int e = 0; e < W; ++e) { acc0[rg * D + d + e] = pa[e]; acc1[rg * D + d + e] = pb[e] * (1.f / sg); }
    }
  }
  __syncthreads();

  // ---- phase 5: backward of the context normalisation and mean (column-parallel)
  float dot = 0.f;
  for (int d = tid; d < D; d += NT) {
    float u = 0.f;
    for (int gI = 0; gI < G; ++gI) u += acc0[gI * D + d];
    acc0[d] = u;                 // each column is owned by one thread from here on
    dot += A[d] * u;
  }
  dot = block_sum_w<NWV>(dot, red);
  const float inv_denA = 1.f / (sA * sqrtf(sA) + eps);
  for (int d = tid; d < D; d += NT) {
    const float dA = (sA * acc0[d] - A[d] * dot) * inv_denA;
    float dbv = 0.f;
    for (int gI = 0; gI < G; ++gI) dbv += acc1[gI * D + d];
    for (int j = 1; j < C; ++j) {
      const float x = HROW(j)[d];
      float g = a.coeff[j - 1] * dA * a.drop_scale;
      g = x > 0.f ? g : 0.f;
      dbv += g;
      gmx = fmaxf(gmx, fabsf(g * sg));
      a.dYh[(int64_t)ooff[j] * a.Dp + d] = T::from_float(g * sg);
    }
    a.dbp[(int64_t)b * D + d] = dbv;
  }
  if (a.guard.gg) gg_end(a.guard, gg_block_max(gmx, ggs));
}

// Register-resident variant for small (1+Nn) x D: each wave keeps its target / negative rows in
// VGPRs between the forward reductions and the backward pass, so every row of ip2 is read from HBM
// exactly once (the streaming kernel above re-reads them, and at ~8 workgroups per CU the 110 KB per
// item do not survive in L2).  RPW = rows per wave, DV = float4 chunks per lane (D = 256*DV).
template <int NW>
__device__ __forceinline__ void block_sum3_w(float& x, float& y, float& z, float* red) {
  x = wave_sum63(x); y = wave_sum63(y); z = wave_sum63(z);
  __syncthreads();
  if ((threadIdx.x & 63) == 63) { const int w = threadIdx.x >> 6; red[w] = x; red[NW + w] = y; red[2 * NW + w] = z; }
  __syncthreads();
  x = y = z = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) { x += red[w]; y += red[NW + w]; z += red[2 * NW + w]; }
}

// NW waves per item, RPW target/negative rows per wave (row qi lives in wave qi % NW), DV float4 chunks per lane
// (D = 256 * DV); the context rows and the per-column tail are owned column-wise, CV = D / (64 NW) columns per thread.
// Eight waves with two rows each keep the register footprint small enough for every workgroup of a 1024-item batch to
// be resident at once (the four-wave form held 13 row slots per wave: ~200 VGPRs, two rounds of workgroups, and the
// block-wide sums of each phase were exposed latency).
// FWD: the forward-only instantiation, as k_score_loss's.
template <typename T, int NW, int RPW, int DV, bool FWD = false>
__global__ __launch_bounds__(64 * NW) void k_score_loss_reg(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int THREADS = 64 * NW;
  constexpr int CV = 256 * DV / THREADS;
  static_assert(CV >= 1 && CV * THREADS == 256 * DV, "D must be a multiple of the thread count");
  constexpr int CXM = 6;       // context rows kept in registers (C - 1 <= CXM on this path)
  const int D = a.D, C = a.C, Nn = a.Nn, CN = C + Nn;
  float* A = sm;               // [D]
  float* Ah = A + D;           // [D]
  float* acc0 = Ah + D;        // [NW][D] per-wave partial dAh
  float* acc1 = acc0 + NW * D; // [NW][D] per-wave partial db
  float* n2 = acc1 + NW * D;   // [CN]
  float* tq = n2 + CN;         // [CN]
  float* cq = tq + CN;         // [CN]
  float* red = cq + CN;        // [3 NW]
  int* ooff = (int*)(red + 3 * NW);   // [CN] row of dYh receiving channel ch's gradient
  const int b = item_of_block(a.items_rr), tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float eps = 1e-10f;
  __shared__ float ggs[16];
  float sgm;
  if (!gg_begin(a.guard, ggs, sgm)) return;
  const float sg = a.sg * sgm;

  // Every global read of ip2 is issued up front: the target / negative rows of this wave
  // (qi = wave, wave+NW, ...) and the context rows (thread tid owns columns tid + THREADS v).
  float4 x[RPW][DV];
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int qi = wave + NW * k;
    const int ch = qi == 0 ? 0 : C + qi - 1;
    const int r = b * CN + (qi <= Nn ? ch : 0);
    const int hr = a.map ? a.map[r] : r;
#pragma unroll
    for (int v = 0; v < DV; ++v)
      x[k][v] = qi <= Nn ? *(const float4*)(a.H + (int64_t)hr * D + lane * 4 + v * 256) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float cx[CXM][CV];
#pragma unroll
  for (int j = 0; j < CXM; ++j) {
    const int r = b * CN + (j + 1 < C ? j + 1 : 0);
    const int hr = a.map ? a.map[r] : r;
#pragma unroll
    for (int v = 0; v < CV; ++v) cx[j][v] = j + 1 < C ? a.H[(int64_t)hr * D + tid + v * THREADS] : 0.f;
  }
  float cf[CXM];
#pragma unroll
  for (int j = 0; j < CXM; ++j) cf[j] = j + 1 < C ? a.coeff[j] : 0.f;
  for (int ch = tid; ch < CN; ch += THREADS) {
    const int r = b * CN + ch;
    ooff[ch] = a.map ? a.seg_start[a.map[r]] + a.ord[r] : r;
  }

  // ---- phase 1: context mean and its norm
  float ssq = 0.f;
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CXM; ++j) s += cf[j] * cx[j][v];
    A[tid + v * THREADS] = s;
    ssq += s * s;
  }
  const float sA = block_sum_w<NW>(ssq, red);
  const float nA = sqrtf(sA) + eps;
#pragma unroll
  for (int v = 0; v < CV; ++v) Ah[tid + v * THREADS] = A[tid + v * THREADS] / nA;
  __syncthreads();

  // ---- phase 2: norms and dots from registers
  float4 y[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) y[v] = *(const float4*)(Ah + lane * 4 + v * 256);
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int qi = wave + NW * k;
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const float4 xx = x[k][v];
      s += xx.x * xx.x + xx.y * xx.y + xx.z * xx.z + xx.w * xx.w;
      t += xx.x * y[v].x + xx.y * y[v].y + xx.z * y[v].z + xx.w * y[v].w;
    }
    s = wave_sum63(s); t = wave_sum63(t);
    if (lane == 63 && qi <= Nn) { const int ch = qi == 0 ? 0 : C + qi - 1; n2[ch] = s; tq[ch] = t; }
  }
  __syncthreads();

  // ---- phase 3: scores, hinge, loss, coefficients
  const float sp = tq[0] / (sqrtf(n2[0]) + eps);
  const float wb = a.item_w ? a.item_w[b] : 1.f;
  float lsum = 0.f, vsum = 0.f, gsum = 0.f;
  for (int k = tid; k < Nn; k += THREADS) {
    const int ch = C + k;
    const float sn = tq[ch] / (sqrtf(n2[ch]) + eps);
    const float d = sp - sn;
    const float h = fmaxf(0.f, a.margin - d);
    float g;     // wb: max_margin_loss_layer.cpp:82-97 (sqrt(w)*h squared, or w*h) and :152-186
    if (a.norm == 2) { lsum += wb * h * h; g = 2.f * wb * h * a.grad_scale; }
    else { lsum += wb * fabsf(h); g = h > 0.f ? wb * a.grad_scale : 0.f; }
    vsum += d < 0.f ? 1.f : 0.f;
    gsum += g;
    cq[ch] = g;
    if (a.s_bogus) a.s_bogus[(int64_t)b * Nn + k] = sn;
  }
  block_sum3_w<NW>(lsum, vsum, gsum, red);
  if (tid == 0) {
    cq[0] = -gsum;
    a.loss_part[b] = lsum;
    a.viol_part[b] = vsum;
    if (a.s_true) a.s_true[b] = sp;
    // workgroup 0 is in the kernel's first round: "this step's forward GEMM has finished" (placed here, where few values
    // are live: at the kernel's head it cost the RPW 7 form six registers and, at 133, an occupancy step)
    if (a.gate_host && b == 0) __hip_atomic_store(a.gate_host, a.gate_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if constexpr (FWD) { if (a.fwd_only) return; }      // the forward-only pass ends here (a run-time exit: see FWD above)
  __syncthreads();

  // ---- phase 4: backward of this wave's rows from registers; one coalesced 512-B store per chunk.  Per row three
  // scalars k1 = c n^2/den, k2 = c t/den (both times drop_scale * sg) and k3 = c/(n+eps); per element
  // g*sg = k1*Ah - k2*x (masked), dAh += k3*x, db*sg += g*sg.  sg is a power of two, so carrying it through the sums
  // and dividing at the end changes no bit.
  float gmx = 0.f;
  float4 pa[DV], pb[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) { pa[v] = make_float4(0.f, 0.f, 0.f, 0.f); pb[v] = pa[v]; }
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int qi = wave + NW * k;
    if (qi > Nn) continue;                         // wave-uniform
    const int ch = qi == 0 ? 0 : C + qi - 1;
    const float c = cq[ch], s = n2[ch], t = tq[ch];
    const float rs = sqrtf(s);
    const float k3 = c * __builtin_amdgcn_rcpf(rs + eps);
    const float cd = c * __builtin_amdgcn_rcpf(s * rs + eps) * a.drop_scale * sg;
    const float k1 = cd * s, k2 = cd * t;
    uint16_t* dy = a.dYh + (int64_t)ooff[ch] * a.Dp;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const float xv[4] = {x[k][v].x, x[k][v].y, x[k][v].z, x[k][v].w};
      const float yv[4] = {y[v].x, y[v].y, y[v].z, y[v].w};
      float g[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        g[e] = k1 * yv[e] - k2 * xv[e];
        g[e] = xv[e] > 0.f ? g[e] : 0.f;
        gmx = fmaxf(gmx, fabsf(g[e]));
      }
      pa[v].x += k3 * xv[0]; pa[v].y += k3 * xv[1]; pa[v].z += k3 * xv[2]; pa[v].w += k3 * xv[3];
      pb[v].x += g[0]; pb[v].y += g[1]; pb[v].z += g[2]; pb[v].w += g[3];
      const uint32_t lo = T::from_float(g[0]) | ((uint32_t)T::from_float(g[1]) << 16);
      const uint32_t hi = T::from_float(g[2]) | ((uint32_t)T::from_float(g[3]) << 16);
      *(uint2*)(dy + lane * 4 + v * 256) = make_uint2(lo, hi);
    }
  }
  const float inv_sg = 1.f / sg;
#pragma unroll
  for (int v = 0; v < DV; ++v) {
    *(float4*)(acc0 + wave * D + lane * 4 + v * 256) = pa[v];
    *(float4*)(acc1 + wave * D + lane * 4 + v * 256) = make_float4(pb[v].x * inv_sg, pb[v].y * inv_sg, pb[v].z * inv_sg, pb[v].w * inv_sg);
  }
  __syncthreads();

  // ---- phase 5: backward of the context normalisation and mean (context rows still in registers)
  float dot = 0.f;
  float u[CV];
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    float us = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) us += acc0[w * D + d];
    u[v] = us;
    dot += A[d] * us;
  }
  dot = block_sum_w<NW>(dot, red);
  const float inv_denA = 1.f / (sA * sqrtf(sA) + eps);
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    const float dA = (sA * u[v] - A[d] * dot) * inv_denA;
    float dbv = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) dbv += acc1[w * D + d];
#pragma unroll
    for (int j = 0; j < CXM; ++j) {
      if (j + 1 < C) {
        float g = cf[j] * dA * a.drop_scale;
        g = cx[j][v] > 0.f ? g : 0.f;
        dbv += g;
        gmx = fmaxf(gmx, fabsf(g * sg));
        a.dYh[(int64_t)ooff[j + 1] * a.Dp + d] = T::from_float(g * sg);
      }
    }
    a.dbp[(int64_t)b * D + d] = dbv;
  }
  if (a.guard.gg) gg_end(a.guard, gg_block_max(gmx, ggs));
}
#undef HROW


template <typename T>
static bool launch_score_loss_reg(const ScoreArgs& a, hipStream_t s) {
  // fast path: D == 512, at most 6 context rows, at most 56 target/negative rows
  if (a.D != 512 || a.C - 1 > 6) return false;
  const int rows = 1 + a.Nn;
  const size_t lds = sizeof(float) * ((size_t)(2 + 2 * 8) * a.D + 4 * (a.C + a.Nn) + 3 * 8);
#define VV_SLR(RPW)                                                                                       \
  do {                                                                                                    \
    (void)hipFuncSetAttribute((const void*)k_score_loss_reg<T, 8, RPW, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    VV_LAUNCH((k_score_loss_reg<T, 8, RPW, 2>), dim3(a.B), dim3(512), lds, s, a);                         \
  } while (0)
#define VV_SLRF(RPW)                                                                                      \
  do {                                                                                                    \
    (void)hipFuncSetAttribute((const void*)k_score_loss_reg<F16, 8, RPW, 2, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    VV_LAUNCH((k_score_loss_reg<F16, 8, RPW, 2, true>), dim3(a.B), dim3(512), lds, s, a);                 \
  } while (0)
  if (rows > 56) return false;
  if (a.fwd_only) {                               // (the forward-only pass rounds nothing to 16 bits: one operand type serves both)
    if (rows <= 16) VV_SLRF(2); else if (rows <= 32) VV_SLRF(4); else VV_SLRF(7);
    return true;
  }
  if (rows <= 16) VV_SLR(2);
  else if (rows <= 32) VV_SLR(4);
  else VV_SLR(7);
#undef VV_SLR
#undef VV_SLRF
  return true;
}

// ---- rows of H as fp32 or as f16 (round 6, FwdArgs::h16 / ScoreArgs::h16).  The kernels below hold a row as float4 pieces per lane; which
// columns a piece covers depends on the storage: fp32 rows are read 16 bytes = 4 columns per lane and piece (piece v: columns lane 4 + 256 v),
// f16 rows 16 bytes = 8 columns per lane (pieces 2 w, 2 w + 1: columns 512 w + lane 8 .. + 3 and + 4 .. + 7) -- 8-byte row loads run at ~0.6 of the
// 16-byte rate per byte (profiles/r04_h16_intermediate.txt).  h_col: first column of piece v; h_row: the DV pieces of one row.
template <bool H16> __device__ __forceinline__ int h_col(int lane, int v) { return H16 ? (v >> 1) * 512 + lane * 8 + (v & 1) * 4 : lane * 4 + v * 256; }
template <bool H16> __device__ __forceinline__ float h_at(const float* H, int64_t i) { return H16 ? (float)((const _Float16*)H)[i] : H[i]; }
template <bool H16, int DV> __device__ __forceinline__ void h_row(const float* H, int64_t row, int D, int lane, float4* x) {
  if constexpr (H16) {
    static_assert(DV % 2 == 0, "f16 rows are read 8 columns at a time");
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const _Float16* hp = (const _Float16*)H + row * D + lane * 8;
#pragma unroll
    for (int w = 0; w < DV / 2; ++w) {
      const h8 q = *(const h8*)(hp + 512 * w);
      x[2 * w] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
      x[2 * w + 1] = make_float4((float)q[4], (float)q[5], (float)q[6], (float)q[7]);
    }
  } else {
#pragma unroll
    for (int v = 0; v < DV; ++v) x[v] = *(const float4*)(H + row * D + lane * 4 + v * 256);
  }
}

// ---- segment-wise backward, pass 1: k_score_loss_reg without the per-instance gradient rows.  Forward as there; the
// backward stops at the factored form (vv_internal.h: SegRec): one record per instance, Ah_b and dA_b per item.
// (Sixteen waves per item, four rows per wave -- one item per CU at a time instead of two items of eight waves: 36 against 25 us, round 4.)
// DROP (ScoreArgs::drop): the rows of H are the shared PRE-dropout projections; every instance applies its own mask (and 1 / (1 - ratio))
// as its row arrives, and everything behind that -- norms, scores, records -- is the reference's graph on the masked rows.
// (Round 6, with f16 rows -- 86 VGPRs instead of 112-127 -- two more residencies were measured and not kept: capped at 80 VGPRs = three
// workgroups per CU instead of two, 7 registers spilled: 22.9 -> 23.7 us; FOUR waves per item with 14 rows per wave, three or four 256-thread
// workgroups per CU = all 1024 items resident at once: 23.0 -> 26.2-27.1 us.  tools/sessions/r06_log.md s5, s8.)
// FWD (ScoreArgs::fwd_only, vv_forward): the forward-only instantiation -- the same row loads, masks, sums and scores, ending behind the loss
// and violation partials; neither the per-item vectors (V) nor the instances' records, positions or gradient bound are computed or stored.
template <int NW, int RPW, int DV, bool DROP = false, bool H16 = false, bool FWD = false>
__global__ __launch_bounds__(64 * NW) void k_score_fwd(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int THREADS = 64 * NW;
  constexpr int CV = 256 * DV / THREADS;
  static_assert(CV >= 1 && CV * THREADS == 256 * DV, "D must be a multiple of the thread count");
  constexpr int CXM = 6;
  const int D = a.D, C = a.C, Nn = a.Nn, CN = C + Nn;
  float* A = sm;               // [D]
  float* Ah = A + D;           // [D]
  float* acc0 = Ah + D;        // [NW][D] per-wave partial dAh
  float* n2 = acc0 + NW * D;   // [CN]
  float* tq = n2 + CN;         // [CN]
  float* cq = tq + CN;         // [CN]
  float* red = cq + CN;        // [3 NW]
  int* ooff = (int*)(red + 3 * NW);   // [CN] grouped position of channel ch's instance
  const int b = item_of_block(a.items_rr), tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float eps = 1e-10f;
#ifdef VV_LAB
  // (lab: phase stamps of wave 0, written by thread 0 at the kernel's end -- ScoreArgs::lab_ts)
  uint32_t ts_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long rt0_ = 0;
#define SF_TS(i) if (a.lab_ts && wave == 0) ts_[i] = (uint32_t)__builtin_readcyclecounter();
  if (a.lab_ts && wave == 0) rt0_ = __builtin_amdgcn_s_memrealtime();
#else
#define SF_TS(i)
#endif
  SF_TS(0)

  // (round 5: the context rows are requested FIRST -- vmcnt completes in order, and the context mean, its block sum and the normalised vector
  // are what the kernel computes first: behind the 14 target / negative rows they waited for all of them, profiles/r05_score_fwd_stamps.txt)
  float cx[CXM][CV];
#pragma unroll
  for (int j = 0; j < CXM; ++j) {
    const int r = b * CN + (j + 1 < C ? j + 1 : 0);
    const int hr = a.map[r];
#pragma unroll
    for (int v = 0; v < CV; ++v) cx[j][v] = j + 1 < C ? h_at<H16>(a.H, (int64_t)hr * D + tid + v * THREADS) : 0.f;
    if (DROP && j + 1 < C) {
      const int64_t rr = (int64_t)(j + 1) * a.B + b;
      const uint32_t rc = drop_row_ctr(rr, D, a.drop.s32);
#pragma unroll
      for (int v = 0; v < CV; ++v) {
        const int col = tid + v * THREADS;
        const uint32_t kp = drop_keep4(a.drop, rr, rc, col & ~3);
        cx[j][v] = ((kp >> (col & 3)) & 1u) ? cx[j][v] * a.drop.scale : 0.f;
      }
    }
  }
  // (round 6, ScoreArgs::prefetch, f16 rows: this workgroup is in the kernel's FIRST round -- blocks 0 .. n/2 - 1 are resident together, two per
  // CU --; block bid + n/2 of the second round runs on the same XCD.  While this item's compute phases run the memory system is idle (every
  // workgroup of a round loads, then computes, in step): one line of the second-round item's rows per thread is requested then, into the XCD's
  // L2, where the second round finds it.  The row index is requested here, with this item's own indices, so that nothing waits for it later.)
  int pf_row = -1;
  if (H16 && a.prefetch && !a.items_rr && !((int)gridDim.x & 7) && THREADS == 512) {
    const int bid2 = (int)blockIdx.x + ((int)gridDim.x >> 1), r2 = tid >> 3;
    if (bid2 < (int)gridDim.x && r2 < CN) pf_row = a.map[((bid2 & 7) * ((int)gridDim.x >> 3) + (bid2 >> 3)) * CN + r2];
  }
  float4 x[RPW][DV];
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int qi = wave + NW * k;
    const int ch = qi == 0 ? 0 : C + qi - 1;
    const int r = b * CN + (qi <= Nn ? ch : 0);
    const int hr = a.map[r];
#ifdef VV_LAB
    if (a.lab_hack) {                                // (lab: what the row loads' time depends on -- results wrong)
      const int64_t rs = a.lab_hack == 1 ? D / 2 : D;
#pragma unroll
      for (int v = 0; v < DV; ++v)
        x[k][v] = (qi <= Nn && !(a.lab_hack == 2 && v > 0)) ? *(const float4*)(a.H + (int64_t)hr * rs + lane * 4 + v * 256) : make_float4(1.f, 0.f, 0.f, 0.f);
    } else
#endif
    {
      h_row<H16, DV>(a.H, hr, D, lane, x[k]);          // (always a valid row: channel 0 stands in past the item's last negative)
#pragma unroll
      for (int v = 0; v < DV; ++v) x[k][v] = qi <= Nn ? x[k][v] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (DROP && qi <= Nn) {
      const int64_t rr = (int64_t)ch * a.B + b;                    // the instance's row in the reference's order
      const uint32_t rc = drop_row_ctr(rr, D, a.drop.s32);
#pragma unroll
      for (int v = 0; v < DV; ++v) {
        const uint32_t kp = drop_keep4(a.drop, rr, rc, h_col<H16>(lane, v));
        x[k][v].x = (kp & 1u) ? x[k][v].x * a.drop.scale : 0.f; x[k][v].y = (kp & 2u) ? x[k][v].y * a.drop.scale : 0.f;
        x[k][v].z = (kp & 4u) ? x[k][v].z * a.drop.scale : 0.f; x[k][v].w = (kp & 8u) ? x[k][v].w * a.drop.scale : 0.f;
      }
    }
  }
  float cf[CXM];
#pragma unroll
  for (int j = 0; j < CXM; ++j) cf[j] = j + 1 < C ? a.coeff[j] : 0.f;
  if constexpr (!FWD)
  for (int ch = tid; ch < CN; ch += THREADS) {
    const int r = b * CN + ch;
    ooff[ch] = a.seg_start[a.map[r]] + a.ord[r];
  }

  // ---- context mean and its norm
  float ssq = 0.f;
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CXM; ++j) s += cf[j] * cx[j][v];
    A[tid + v * THREADS] = s;
    ssq += s * s;
  }
  const float sA = block_sum_w<NW>(ssq, red);
  SF_TS(1)                                         // the context rows have arrived, first block-wide sum
  const float nA = sqrtf(sA) + eps;
  float* Vb = a.V + (int64_t)2 * b * D;
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const float ah = A[tid + v * THREADS] / nA;
    Ah[tid + v * THREADS] = ah;
    if constexpr (!FWD) Vb[tid + v * THREADS] = ah;
  }
  __syncthreads();

  // ---- norms and dots from registers
  float4 y[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) y[v] = *(const float4*)(Ah + h_col<H16>(lane, v));
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int qi = wave + NW * k;
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const float4 xx = x[k][v];
      s += xx.x * xx.x + xx.y * xx.y + xx.z * xx.z + xx.w * xx.w;
      t += xx.x * y[v].x + xx.y * y[v].y + xx.z * y[v].z + xx.w * y[v].w;
    }
    s = wave_sum63(s); t = wave_sum63(t);
    if (lane == 63 && qi <= Nn) { const int ch = qi == 0 ? 0 : C + qi - 1; n2[ch] = s; tq[ch] = t; }
  }
  __syncthreads();
  SF_TS(2)                                         // every wave's target / negative rows have arrived and are reduced
  if (H16 && a.prefetch) {
    // the second round's rows: one 128-byte line per thread, requested as an LDS-DMA into 256 dead bytes behind the kernel's LDS arrays (a
    // load into a register would land, whenever it lands, in a register the compiler has long handed to something else); never waited for
    const char* pf = (const char*)a.H + (int64_t)(pf_row >= 0 ? pf_row : 0) * D * 2 + (tid & 7) * 128;
    const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)((__attribute__((address_space(3))) void*)(ooff + CN + 4)));
    if (pf_row >= 0) asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, off" :: "s"(m0v & ~3u), "v"(pf) : "m0", "memory");
  }

  // ---- scores, hinge, loss, coefficients
  const float sp = tq[0] / (sqrtf(n2[0]) + eps);
  const float wb = a.item_w ? a.item_w[b] : 1.f;
  float lsum = 0.f, vsum = 0.f, gsum = 0.f;
  for (int k = tid; k < Nn; k += THREADS) {
    const int ch = C + k;
    const float sn = tq[ch] / (sqrtf(n2[ch]) + eps);
    const float d = sp - sn;
    const float h = fmaxf(0.f, a.margin - d);
    float g;
    if (a.norm == 2) { lsum += wb * h * h; g = 2.f * wb * h * a.grad_scale; }
    else { lsum += wb * fabsf(h); g = h > 0.f ? wb * a.grad_scale : 0.f; }
    vsum += d < 0.f ? 1.f : 0.f;
    gsum += g;
    if constexpr (!FWD) cq[ch] = g;
    if (a.s_bogus) a.s_bogus[(int64_t)b * Nn + k] = sn;
  }
  block_sum3_w<NW>(lsum, vsum, gsum, red);
  if (tid == 0) {
    if constexpr (!FWD) cq[0] = -gsum;
    a.loss_part[b] = lsum;
    a.viol_part[b] = vsum;
    if (a.s_true) a.s_true[b] = sp;
    // workgroup 0 is in the kernel's first round: "this step's forward GEMM has finished" (placed here, where few values
    // are live: at the kernel's head it cost the RPW 7 form six registers and, at 133, an occupancy step)
    if (a.gate_host && b == 0) __hip_atomic_store(a.gate_host, a.gate_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if constexpr (FWD) return;                       // the forward-only pass ends here
  __syncthreads();
  SF_TS(3)

  // ---- dAh = sum_q k3_q x_q from registers; the record of every target / negative instance
  float bnd = 0.f;
  float4 pa[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) pa[v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < RPW; ++k) {
    const int qi = wave + NW * k;
    if (qi > Nn) continue;                         // wave-uniform
    const int ch = qi == 0 ? 0 : C + qi - 1;
    const float c = cq[ch], s = n2[ch], t = tq[ch];
    const float rs = sqrtf(s);
    const float k3 = c * __builtin_amdgcn_rcpf(rs + eps);
    const float cd = c * __builtin_amdgcn_rcpf(s * rs + eps) * a.drop_scale * a.sg;
    bnd = fmaxf(bnd, fabsf(cd * s) + fabsf(cd * t) * rs);           // |alpha| + |beta| |x|: GuardArgs::bound
    if (lane == 0) { SegRec rc; rc.alpha = cd * s; rc.beta = cd * t; rc.vec = 2 * b; rc.pad = b * CN + ch; a.rec[ooff[ch]] = rc; }
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      pa[v].x += k3 * x[k][v].x; pa[v].y += k3 * x[k][v].y; pa[v].z += k3 * x[k][v].z; pa[v].w += k3 * x[k][v].w;
    }
  }
#pragma unroll
  for (int v = 0; v < DV; ++v) *(float4*)(acc0 + wave * D + h_col<H16>(lane, v)) = pa[v];
  if (tid < C - 1) {
    SegRec rc; rc.alpha = a.coeff[tid] * a.drop_scale * a.sg; rc.beta = 0.f; rc.vec = 2 * b + 1; rc.pad = b * CN + tid + 1;
    a.rec[ooff[tid + 1]] = rc;
  }
  if (lane == 0) red[wave] = bnd;                   // (red is free here: block_sum3_w's readers are past the barrier above)
  __syncthreads();
  SF_TS(4)

  // ---- backward of the context normalisation: dA_b
  float bnd_item = 0.f;
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < NW; ++w) bnd_item = fmaxf(bnd_item, red[w]);
  }
  float dot = 0.f;
  float u[CV];
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    float us = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) us += acc0[w * D + d];
    u[v] = us;
    dot += A[d] * us;
  }
  dot = block_sum_w<NW>(dot, red);
  const float inv_denA = 1.f / (sA * sqrtf(sA) + eps);
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    Vb[D + d] = (sA * u[v] - A[d] * dot) * inv_denA;
  }
  if (tid == 0 && a.bound_out) {
    // context instances: |coeff_j ds sg| max_d |dA_d| <= |alpha_j| 4 sA gsum / (sA^1.5 + eps)   (|u_d| <= sum_q |c_q| = 2 gsum)
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < CXM; ++j) am = fmaxf(am, fabsf(cf[j]));      // (the coefficients are in registers since the kernel's start)
    bnd_item = fmaxf(bnd_item, am * a.drop_scale * a.sg * 4.f * sA * gsum * inv_denA);
    atomicMax(a.bound_out + (b & (GG_BOUND_SLOTS - 1)) * GG_BOUND_STRIDE, ((unsigned long long)(unsigned)a.bound_seq << 32) | __float_as_uint(bnd_item));
  }
#ifdef VV_LAB
  SF_TS(5)
  if (a.lab_ts && tid == 0) {
    const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime();
    uint32_t* o = a.lab_ts + (size_t)blockIdx.x * 16;
#pragma unroll
    for (int i = 0; i < 6; ++i) o[i] = ts_[i];
    o[6] = (uint32_t)rt0_; o[7] = (uint32_t)rt1; o[8] = (uint32_t)b;
    o[9] = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 4);           // HW_ID (wave, simd, cu, sh, se ...)
    o[10] = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20);          // XCC_ID
  }
#endif
#undef SF_TS
}

// ---- the same pass for items that do not fit in registers (D = 1024, hundreds of negatives: the per-GPU shape of BASELINE
// configs[4]): ONE sweep over the item's rows.  A wave takes negatives wave, wave + NW, ...; a row is in registers (DV float4
// per lane) while its norm and its dot with Ah are reduced inside the wave, and because every wave has computed the TARGET's
// score for itself first, the row's hinge coefficient g_k is known right there: its record is written and k3 x_k is added to
// the wave's partial dAh before the row is dropped.  Only the target's own coefficient (-sum of all g_k) has to wait for the
// block-wide sum; wave 0 adds that row at the end.  (A segment-wise form of the streaming k_score_loss read every row twice: 0.92 ms of the
// 2.26 ms cfg-5 step; this kernel 0.47 ms.)  Sums in a fixed order: a wave's rows in sequence, then the waves in sequence.
// (DV = 4 sits at the edge of 128 VGPRs: two workgroups per CU need 4 waves per SIMD -- the gradient bound's two registers
// pushed it to 131 and one workgroup per CU, 0.47 -> 0.70 ms at cfg 5; the second launch bound holds it at 128)
// V16 (round 6, ScoreArgs::v16): the two per-item vectors k_seg_bwd gathers once per instance -- Ah_b and dA_b -- leave as f16 (840 k gathers
// of a 4 KB row at the per-GPU shape of configs[4]: half the bytes).  Ah_b as it is (|values| <= 1); dA_b times a power of two that puts its
// largest magnitude in [2^13, 2^14), whose inverse rides in the context instances' alpha (exact) -- so their records are written behind dA_b.
// DROP (ScoreArgs::drop, option "drop_dedup" = 2): as k_score_fwd's -- the rows of H are the shared PRE-dropout projections, every instance
// applies its own mask and 1 / (1 - ratio) as its row arrives (context rows in the column-parallel mean, the target row of every wave, every
// negative of the sweep); everything behind the masked rows is the kernel without DROP, and the records carry their one factor scale in
// a.drop_scale as before.  A separate instantiation: without DROP nothing of it is compiled.
// FWD: the forward-only instantiation, as k_score_fwd's -- the sweep keeps its loads, masks, reductions and sums, and stores scores and partials only.
template <int NW, int DV, bool H16 = false, bool V16 = false, bool DROP = false, bool FWD = false>
__global__ __launch_bounds__(64 * NW, DV == 4 ? 4 : 1) void k_score_stream(ScoreArgs a) {
  static_assert(!DROP || !V16, "dropout steps run with v16 off");
  static_assert(!FWD || !V16, "the forward-only pass stores no per-item vectors");
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int THREADS = 64 * NW;
  constexpr int CV = 256 * DV / THREADS;
  static_assert(CV >= 1 && CV * THREADS == 256 * DV, "D must be a multiple of the thread count");
  const int D = 256 * DV, C = a.C, Nn = a.Nn, CN = C + Nn;
  float* A = sm;               // [D]
  float* Ah = A + D;           // [D]
  float* acc0 = Ah + D;        // [NW][D] per-wave partial dAh
  float* red = acc0 + NW * D;  // [4 NW]: three groups for the loss sums, one for the waves' gradient bounds
  const int b = item_of_block(a.items_rr), tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float eps = 1e-10f;
  const int32_t* map = a.map + (int64_t)b * CN;
  const int32_t* ord = a.ord + (int64_t)b * CN;

  // ---- context mean and its norm (column-parallel: a thread owns CV columns)
  float ssq = 0.f;
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    float sx = 0.f;
    if constexpr (DROP) {
      for (int j = 1; j < C; ++j) {
        const int64_t rr = (int64_t)j * a.B + b;                       // the instance's row in the reference's order
        const uint32_t kp = drop_keep4(a.drop, rr, drop_row_ctr(rr, D, a.drop.s32), d & ~3);
        const float h = h_at<H16>(a.H, (int64_t)map[j] * D + d);
        sx += a.coeff[j - 1] * (((kp >> (d & 3)) & 1u) ? h * a.drop.scale : 0.f);
      }
    } else {
      for (int j = 1; j < C; ++j) sx += a.coeff[j - 1] * h_at<H16>(a.H, (int64_t)map[j] * D + d);
    }
    A[d] = sx;
    ssq += sx * sx;
  }
  const float sA = block_sum_w<NW>(ssq, red);
  const float nA = sqrtf(sA) + eps;
  float* Vb = a.V + (int64_t)2 * b * D;
  _Float16* Vh = (_Float16*)a.V + (int64_t)2 * b * D;
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    const float ah = A[d] / nA;
    Ah[d] = ah;
    if constexpr (!FWD) { if (V16) Vh[d] = (_Float16)ah; else Vb[d] = ah; }
  }
  __syncthreads();
  float4 y[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) y[v] = *(const float4*)(Ah + h_col<H16>(lane, v));

  auto load_row = [&](int ch, float4* x) { h_row<H16, DV>(a.H, map[ch], D, lane, x); };
  // DROP: channel ch's own mask and scale over its row (applied where the row is first used: its loads stay in flight until then)
  auto mask_row = [&](int ch, float4* x) {
    if constexpr (DROP) {
      const int64_t rr = (int64_t)ch * a.B + b;
      const uint32_t rc = drop_row_ctr(rr, D, a.drop.s32);
#pragma unroll
      for (int v = 0; v < DV; ++v) {
        const uint32_t kp = drop_keep4(a.drop, rr, rc, h_col<H16>(lane, v));
        x[v].x = (kp & 1u) ? x[v].x * a.drop.scale : 0.f; x[v].y = (kp & 2u) ? x[v].y * a.drop.scale : 0.f;
        x[v].z = (kp & 4u) ? x[v].z * a.drop.scale : 0.f; x[v].w = (kp & 8u) ? x[v].w * a.drop.scale : 0.f;
      }
    }
  };
  // norm^2 and dot with Ah of a row held in registers; both totals in every lane
  auto norm_dot = [&](const float4* x, float& s, float& t) {
    float ps = 0.f, pt = 0.f;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      ps += x[v].x * x[v].x + x[v].y * x[v].y + x[v].z * x[v].z + x[v].w * x[v].w;
      pt += x[v].x * y[v].x + x[v].y * y[v].y + x[v].z * y[v].z + x[v].w * y[v].w;
    }
    ps = wave_sum63(ps); pt = wave_sum63(pt);
    s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ps), 63));
    t = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pt), 63));
  };

  // ---- the target's score, by every wave for itself
  float4 x0[DV];
  load_row(0, x0);
  mask_row(0, x0);
  float s0, t0;
  norm_dot(x0, s0, t0);
  const float sp = t0 / (sqrtf(s0) + eps);
  const float wb = a.item_w ? a.item_w[b] : 1.f;

  // ---- the wave's negatives: one sweep, the next row's loads issued before this row's reductions
  float4 pa[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) pa[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  float lsum = 0.f, vsum = 0.f, gsum = 0.f, bnd = 0.f;
  float4 xc[DV], xn[DV];
  int k = wave;
  if (k < Nn) load_row(C + k, xc);
  for (; k < Nn; k += NW) {
    const int ch = C + k;
    const bool more = k + NW < Nn;               // wave-uniform
    if (more) load_row(ch + NW, xn);
    mask_row(ch, xc);
    float sq, tq;
    norm_dot(xc, sq, tq);
    const float rs = sqrtf(sq);
    const float sn = tq / (rs + eps);
    const float d = sp - sn;
    const float h = fmaxf(0.f, a.margin - d);
    float g;     // max_margin_loss_layer.cpp:82-97, 152-186 (as k_score_fwd)
    if (a.norm == 2) { lsum += wb * h * h; g = 2.f * wb * h * a.grad_scale; }
    else { lsum += wb * fabsf(h); g = h > 0.f ? wb * a.grad_scale : 0.f; }
    vsum += d < 0.f ? 1.f : 0.f;
    gsum += g;
    if constexpr (FWD) {
      if (lane == 0 && a.s_bogus) a.s_bogus[(int64_t)b * Nn + k] = sn;
    } else {
    const float k3 = g * __builtin_amdgcn_rcpf(rs + eps);
    const float cd = g * __builtin_amdgcn_rcpf(sq * rs + eps) * a.drop_scale * a.sg;
    bnd = fmaxf(bnd, fabsf(cd * sq) + fabsf(cd * tq) * rs);          // |alpha| + |beta| |x|: GuardArgs::bound
    if (lane == 0) {
      SegRec rc; rc.alpha = cd * sq; rc.beta = cd * tq; rc.vec = 2 * b; rc.pad = b * CN + ch;
      a.rec[a.seg_start[map[ch]] + ord[ch]] = rc;
      if (a.s_bogus) a.s_bogus[(int64_t)b * Nn + k] = sn;
    }
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      pa[v].x += k3 * xc[v].x; pa[v].y += k3 * xc[v].y; pa[v].z += k3 * xc[v].z; pa[v].w += k3 * xc[v].w;
    }
    }
    if (more) {
#pragma unroll
      for (int v = 0; v < DV; ++v) xc[v] = xn[v];
    }
  }
  // ---- block-wide loss / violations / sum of the coefficients (every lane of a wave holds the wave's values)
  __syncthreads();
  if (lane == 0) { red[wave] = lsum; red[NW + wave] = vsum; red[2 * NW + wave] = gsum; }
  __syncthreads();
  lsum = vsum = gsum = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) { lsum += red[w]; vsum += red[NW + w]; gsum += red[2 * NW + w]; }
  if (tid == 0) {
    a.loss_part[b] = lsum;
    a.viol_part[b] = vsum;
    if (a.s_true) a.s_true[b] = sp;
    if (a.gate_host && b == 0) __hip_atomic_store(a.gate_host, a.gate_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if constexpr (FWD) return;                        // the forward-only pass ends here
  // ---- the target row: coefficient -sum_k g_k (wave 0 adds it to its partial)
  if (wave == 0) {
    const float c = -gsum, rs = sqrtf(s0);
    const float k3 = c * __builtin_amdgcn_rcpf(rs + eps);
    const float cd = c * __builtin_amdgcn_rcpf(s0 * rs + eps) * a.drop_scale * a.sg;
    bnd = fmaxf(bnd, fabsf(cd * s0) + fabsf(cd * t0) * rs);
    if (lane == 0) { SegRec rc; rc.alpha = cd * s0; rc.beta = cd * t0; rc.vec = 2 * b; rc.pad = b * CN; a.rec[a.seg_start[map[0]] + ord[0]] = rc; }
    if constexpr (DROP && DV == 4) {               // (the mask's temporaries do not fit beside a row held through the sweep at 128 registers: wave 0
      load_row(0, x0);                             //  fetches and masks the target row again -- the same values, from L2 -- instead of a spill)
      mask_row(0, x0);
    }
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      pa[v].x += k3 * x0[v].x; pa[v].y += k3 * x0[v].y; pa[v].z += k3 * x0[v].z; pa[v].w += k3 * x0[v].w;
    }
  }
#pragma unroll
  for (int v = 0; v < DV; ++v) *(float4*)(acc0 + wave * D + h_col<H16>(lane, v)) = pa[v];
  if (!V16)
    for (int j = 1 + tid; j < C; j += THREADS) {
      SegRec rc; rc.alpha = a.coeff[j - 1] * a.drop_scale * a.sg; rc.beta = 0.f; rc.vec = 2 * b + 1; rc.pad = b * CN + j;
      a.rec[a.seg_start[map[j]] + ord[j]] = rc;
    }
  if (lane == 0) red[3 * NW + wave] = bnd;          // (a fourth group of NW words behind the three of the loss sums)
  __syncthreads();

  // ---- backward of the context normalisation: dA_b
  float bnd_item = 0.f;
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < NW; ++w) bnd_item = fmaxf(bnd_item, red[3 * NW + w]);
  }
  float dot = 0.f;
  float u[CV];
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int d = tid + v * THREADS;
    float us = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) us += acc0[w * D + d];
    u[v] = us;
    dot += A[d] * us;
  }
  dot = block_sum_w<NW>(dot, red);
  const float inv_denA = 1.f / (sA * sqrtf(sA) + eps);
  if (V16) {
    float da[CV], m = 0.f;
#pragma unroll
    for (int v = 0; v < CV; ++v) { da[v] = (sA * u[v] - A[tid + v * THREADS] * dot) * inv_denA; m = fmaxf(m, fabsf(da[v])); }
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) m = fmaxf(m, __shfl_xor(m, o2, 64));
    __syncthreads();                                // (block_sum_w's readers of red[0 .. NW) are done)
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w]);
    float sc = 1.f;
    // m sc in [2^13, 2^14); the exponent stops at 126 so that sc and 1 / sc stay normal floats (m below about 2^-113: 14 - e passed 127, sc was inf and
    // 1 / sc zero -- reachable with bf16 operands, whose gradient scale is 1, and a tiny loss_weight): below that dA_b keeps fewer bits
    if (m > 0.f && m < 3.0e38f) { int e; (void)frexpf(m, &e); sc = ldexpf(1.f, min(14 - e, 126)); }
#pragma unroll
    for (int v = 0; v < CV; ++v) Vh[D + tid + v * THREADS] = (_Float16)(da[v] * sc);
    const float isc = 1.f / sc;                     // (a power of two: alpha_j / sc times the stored row is alpha_j dA_b)
    for (int j = 1 + tid; j < C; j += THREADS) {
      SegRec rc; rc.alpha = a.coeff[j - 1] * a.drop_scale * a.sg * isc; rc.beta = 0.f; rc.vec = 2 * b + 1; rc.pad = b * CN + j;
      a.rec[a.seg_start[map[j]] + ord[j]] = rc;
    }
  } else {
#pragma unroll
    for (int v = 0; v < CV; ++v) {
      const int d = tid + v * THREADS;
      Vb[D + d] = (sA * u[v] - A[d] * dot) * inv_denA;
    }
  }
  if (tid == 0 && a.bound_out) {                    // as k_score_fwd
    float coeff_max = 0.f;       // max |coeff_j|: the context instances' gradient bound
    for (int j = 0; j + 1 < C; ++j) coeff_max = fmaxf(coeff_max, fabsf(a.coeff[j]));
    bnd_item = fmaxf(bnd_item, coeff_max * a.drop_scale * a.sg * 4.f * sA * gsum * inv_denA);
    atomicMax(a.bound_out + (b & (GG_BOUND_SLOTS - 1)) * GG_BOUND_STRIDE, ((unsigned long long)(unsigned)a.bound_seq << 32) | __float_as_uint(bnd_item));
  }
}

// (the shapes the segment-wise pair is built for, without and with dropout: score_fwd_supported / score_fwd_dropout_supported, vv_pass_plan.h)
void launch_score_fwd(const ScoreArgs& a_in, hipStream_t s) {
  ScoreArgs a = a_in;
  a.items_rr = ko().score_rr;
  a.prefetch = ko().score_pf;
  const int rows = 1 + a.Nn;
  const dim3 grid(a.B), block(512);
  if (!(a.D == 512 && a.C - 1 <= 6 && rows <= 56)) {
    const size_t lds = sizeof(float) * ((size_t)(2 + 8) * a.D + 4 * 8);
    ko().last_score_form = a.D == 512 ? 2 : 3;
    // V16 exists at DV = 4 over f16 rows alone, and neither with DROP (fp32 vectors: dropout steps run with v16 off) nor with FWD (no
    // per-item vectors leave the kernel: v16 has nothing to choose)
    if (a.D != 512 && a.h16 && a.v16 && !a.drop.mode && !a.fwd_only) {
      VV_LAUNCH_LDS((k_score_stream<8, 4, true, true>), grid, block, lds, s, a);
      return;
    }
    with_flags([&](auto d512, auto h16, auto drop, auto fwd) {
      VV_LAUNCH_LDS((k_score_stream<8, d512 ? 2 : 4, h16, false, drop, fwd>), grid, block, lds, s, a);
    }, a.D == 512, a.h16, a.drop.mode, a.fwd_only);
    return;
  }
  ko().last_score_form = 1;
  const size_t lds = sizeof(float) * ((size_t)(2 + 8) * a.D + 4 * (a.C + a.Nn) + 3 * 8) + 288;      // (+ 288: the prefetch's dead LDS-DMA target, ScoreArgs::prefetch)
  // (no second-round prefetch: its LDS-DMA is never waited for, and this form ends a few instructions behind where it would be issued)
  if (a.fwd_only) a.prefetch = 0;
  with_flags([&](auto drop, auto h16, auto fwd) {
    if (rows <= 16) VV_LAUNCH_LDS((k_score_fwd<8, 2, 2, drop, h16, fwd>), grid, block, lds, s, a);
    else if (rows <= 32) VV_LAUNCH_LDS((k_score_fwd<8, 4, 2, drop, h16, fwd>), grid, block, lds, s, a);
    else VV_LAUNCH_LDS((k_score_fwd<8, 7, 2, drop, h16, fwd>), grid, block, lds, s, a);
  }, a.drop.mode, a.h16, a.fwd_only);
}

// eight consecutive columns of a row of H (fp32: two 16-byte loads; f16, SegBwdArgs::h16: one)
template <bool H16> __device__ __forceinline__ void seg_row8(const float* H, int64_t i, float4& lo, float4& hi) {
  if constexpr (H16) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8 q = *(const h8*)((const _Float16*)H + i);
    lo = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
    hi = make_float4((float)q[4], (float)q[5], (float)q[6], (float)q[7]);
  } else {
    lo = *(const float4*)(H + i); hi = *(const float4*)(H + i + 4);
  }
}
// ---- segment-wise backward, pass 2: one wave per distinct row, a lane owns 8 consecutive columns (D = 512).
// Persistent grid: wave w of block g takes rows 4 g + w, + 4 SEGB_BLOCKS, ...; the column sums of the rows it produced
// (the bias gradient) leave as one partial row per block.
// The records of a row sit in ARRIVAL order (k_dd_map's atomic counter), which differs from run to run; the sums must
// not.  A segment of up to 64 records is put in instance order first (each lane holds one record, counts the smaller
// instance indices, and files its record at that rank in a wave-private LDS strip); longer segments -- a row repeated
// more than 64 times in one batch -- are summed in an order-independent way instead: every product is rounded to a
// multiple of 2^-36 in f64 ((p + M) - M, M = 1.5 * 2^16; exact for |p| < 2^15 in the gradient's scaled units), and
// sums of such multiples are exact in f64 up to 2^17, whatever the order.
// DROP (SegBwdArgs::drop): every instance carries its own dropout mask m_i over the shared row:
//   dx_u = [x_u > 0] (sum_i m_i alpha_i V_i - x_u scale sum_i m_i beta_i)        (alpha, beta already carry one factor scale)
// -- the mask regenerated per instance from its reference row (b = vec / 2, ch = pad - b CN) and per chunk (columns 512 c + c0 .. + 7), the
// beta sum per column of every chunk.  The DROP forms read fp32 vectors only: dropout steps run with v16 off (vv_pass_plan.h, option "drop_dedup").
// CNT (option "h16_guard", the k_seg_bwd_cnt kernels below; f16 rows only): the wave also counts what f16's range cost the rows it holds --
// elements stored as 65504, the largest finite f16 (the forward GEMM's epilogue saturates there; a true value in [65488, 65504) rounds to
// it and is counted too: conservative), and rows whose largest element is > 0 and < 2^-14 (every element subnormal; an all-zero row is
// not faint).  Taken from the row values where the wave consumes them (so both placements of the row load and both segment paths are
// covered), behind two wave-uniform ballots: a row that neither saturates nor is faint costs a running maximum and three compares.  One
// pair of 32-bit partials per workgroup goes to SegBwdArgs::h16_cnt -- every workgroup of the grid writes its pair every step, so nothing
// has to be reset -- and the loss workgroup folds them into the step's report entry (reduce_loss).  No value of the step depends on them.
template <typename T, int CH, bool DROP, bool H16, bool V16, bool CNT>
__device__ __forceinline__ void seg_bwd_body(const SegBwdArgs& a) {
  static_assert(!DROP || !V16, "dropout steps run with v16 off");
  static_assert(!CNT || H16, "only f16 rows are counted");
  constexpr int BC = DROP ? CH - 1 : 0, BJ = DROP ? 7 : 0;      // index masks of the per-column beta sums (one dummy element without DROP)
  __shared__ float cs[4][512 * CH];
  __shared__ SegRec strip[4][64];
  float sgm;                                          // a repeat (guard round 1) scales the sums by a further 2^-k
  if (!gg_begin(a.guard, &cs[0][0], sgm)) return;
  const bool first = a.guard.round == 0;              // the bias partials come out of the unrounded values: once
  int pro_shift = 0;
  if (a.guard.gg && a.guard.proactive) {              // GuardArgs::proactive: the scale is settled BEFORE anything is rounded
    const float bm = gg_bound_fold(a.guard.bound, a.guard.seq);
    const float G = bm * (float)(*a.guard.cnt_max) * 1.01f;          // no element of any row's sum can pass this
    // ... and the scale is settled here outright, in both directions: the bound is put in [2^13, 2^14) (the true maximum
    // then sits the bound's looseness below -- tens to hundreds; measured 44 .. 133 on ordinary batches, 790 (D = 512) and 1350
    // (D = 1024) where one row has 480 instances whose gradients partly cancel, tests/test_gpu_grad_guard_exact.py: the largest value
    // still above 2^3, the values normal f16 numbers over 17 binades below it), whatever the host's sg
    int e = 14;
    if (G > 0.f && G < 3.0e38f) (void)frexpf(G, &e);                 // G < 2^e  (zero gradient / inf / nan: no shift; gg_end's flag reports)
    pro_shift = e - 14 > 60 ? 60 : (e - 14 < -60 ? -60 : e - 14);
    sgm = ldexpf(1.f, -pro_shift);                                   // (first needed where the first row is rounded: the two loads above fly meanwhile)
  }
  const int U = a.info[0];
  const int Uk = min((U + BK - 1) / BK * BK, a.Rp);   // the wgrad K loop reads whole BK-row steps
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c0 = lane * 8, D = a.D;                   // D = 512 CH; chunk c covers columns 512 c + c0 .. + 7
  float col[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) col[c][j] = 0.f;
  float gmx = 0.f;
  uint32_t n_sat = 0, n_faint = 0;                    // CNT: this lane's saturated elements, this wave's faint rows
  // A wave's rows are a chain of dependent reads each: segment bounds, records, the vectors the records name, and the row
  // itself.  The row's own values (needed last) and the NEXT row's segment bounds are requested right behind the records,
  // so that only records -> vectors is exposed: 18.7 -> 17.9 us.  (More waves do not help: 89 registers and five blocks per
  // CU instead of four measured the same 17.8-18.3 us; so did requesting the NEXT row's records one row early, bounds two rows
  // early -- 17.8 us: the kernel moves 42 MB of fp32 rows in and 21 MB out, ~3.5 TB/s, and is not latency-chained any more.)
  const int u_first = blockIdx.x * 4 + wave, u_step = 4 * (int)gridDim.x;     // (block numbers by XCD ranges, as item_of_block: measured, no change)
  int seg_b = 0, seg_e = 0;
  if (u_first < U) { seg_b = a.seg_start[u_first]; seg_e = a.seg_start[u_first + 1]; }
  for (int u = u_first; u < Uk; u += u_step) {
    if (u >= U) {
#pragma unroll
      for (int c = 0; c < CH; ++c) *(uint4*)(a.dYu + (int64_t)u * a.Dp + 512 * c + c0) = make_uint4(0u, 0u, 0u, 0u);
      continue;
    }
    const int b = seg_b, e = seg_e, n = e - b;
    SegRec mine; mine.alpha = 0.f; mine.beta = 0.f; mine.vec = 0; mine.pad = 0x7fffffff;
    if (n > 1 && n <= 64 && lane < n) mine = a.rec[b + lane];
    float4 xr0[CH], xr1[CH];
    if (CH == 1) {                                    // (D = 1024 with its long segments: the early row costs more in registers than it hides -- 0.437 -> 0.473 ms at cfg 5)
#pragma unroll
      for (int c = 0; c < CH; ++c) seg_row8<H16>(a.H, (int64_t)u * D + 512 * c + c0, xr0[c], xr1[c]);      // (as non-temporal loads: no gain, profiles/r03_step_ablations.txt 5d)
    }
    if (u + u_step < U) { seg_b = a.seg_start[u + u_step]; seg_e = a.seg_start[u + u_step + 1]; }
    float acc[CH][8];
    float bs = 0.f;
    float bsv[DROP ? CH : 1][DROP ? 8 : 1];           // DROP: sum_i m_i beta_i per column
    if (DROP) {
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) bsv[c & BC][j & BJ] = 0.f;
    }
    // the instance's keep bits for this lane's eight columns of chunk c
    auto keep8 = [&](const SegRec& r, int c) -> uint32_t {
      const int bb = r.vec >> 1, ch = r.pad - bb * a.drop.CN;
      const int64_t rr = (int64_t)ch * a.drop.B + bb;
      const uint32_t rc = drop_row_ctr(rr, D, a.drop.s32);
      return drop_keep4(a.drop, rr, rc, 512 * c + c0) | (drop_keep4(a.drop, rr, rc, 512 * c + c0 + 4) << 4);
    };
    if (n <= 64) {
      const SegRec* rs = a.rec + b;
      if (n > 1) {                                    // instance order
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += __builtin_amdgcn_readlane(mine.pad, j) < mine.pad;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous row's reads of the strip are done
        if (lane < n) strip[wave][rank] = mine;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        rs = strip[wave];
      }
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c][j] = 0.f;
      constexpr int UN = CH == 1 ? 4 : 2;             // instances in flight
      int i = 0;
      for (; i + UN - 1 < n; i += UN) {
        SegRec r[UN]; float4 v0[UN][CH], v1[UN][CH];
#pragma unroll
        for (int k = 0; k < UN; ++k) r[k] = rs[i + k];
#pragma unroll
        for (int k = 0; k < UN; ++k)
#pragma unroll
          for (int c = 0; c < CH; ++c) seg_row8<V16>(a.V, (int64_t)r[k].vec * D + 512 * c + c0, v0[k][c], v1[k][c]);
#pragma unroll
        for (int k = 0; k < UN; ++k) {
          const float al = r[k].alpha;
          if (DROP) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
              const uint32_t kp = keep8(r[k], c);
              const float vv[8] = {v0[k][c].x, v0[k][c].y, v0[k][c].z, v0[k][c].w, v1[k][c].x, v1[k][c].y, v1[k][c].z, v1[k][c].w};
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const bool kj = (kp >> j) & 1u;
                acc[c][j] += kj ? al * vv[j] : 0.f;
                bsv[c & BC][j & BJ] += kj ? r[k].beta : 0.f;
              }
            }
            continue;
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            acc[c][0] += al * v0[k][c].x; acc[c][1] += al * v0[k][c].y; acc[c][2] += al * v0[k][c].z; acc[c][3] += al * v0[k][c].w;
            acc[c][4] += al * v1[k][c].x; acc[c][5] += al * v1[k][c].y; acc[c][6] += al * v1[k][c].z; acc[c][7] += al * v1[k][c].w;
          }
          bs += r[k].beta;
        }
      }
      for (; i < n; ++i) {
        const SegRec r = rs[i];
        if (DROP) {
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            float4 v0, v1;
            seg_row8<V16>(a.V, (int64_t)r.vec * D + 512 * c + c0, v0, v1);
            const uint32_t kp = keep8(r, c);
            const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const bool kj = (kp >> j) & 1u;
              acc[c][j] += kj ? r.alpha * vv[j] : 0.f;
              bsv[c & BC][j & BJ] += kj ? r.beta : 0.f;
            }
          }
          continue;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          float4 v0, v1;
          seg_row8<V16>(a.V, (int64_t)r.vec * D + 512 * c + c0, v0, v1);
          acc[c][0] += r.alpha * v0.x; acc[c][1] += r.alpha * v0.y; acc[c][2] += r.alpha * v0.z; acc[c][3] += r.alpha * v0.w;
          acc[c][4] += r.alpha * v1.x; acc[c][5] += r.alpha * v1.y; acc[c][6] += r.alpha * v1.z; acc[c][7] += r.alpha * v1.w;
        }
        bs += r.beta;
      }
    } else {                                          // order-independent sums
      const double M = 98304.0;
      double dacc[CH][8], dbs = 0.0;
      double dbsv[DROP ? CH : 1][DROP ? 8 : 1];
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) dacc[c][j] = 0.0;
      if (DROP) {
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int j = 0; j < 8; ++j) dbsv[c & BC][j & BJ] = 0.0;
      }
      for (int i = b; i < e; ++i) {
        const SegRec r = a.rec[i];
        const double al = (double)r.alpha;
        const double rb = ((double)r.beta + M) - M;
        dbs += rb;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const uint32_t kp = DROP ? keep8(r, c) : 0xffu;
          float4 v0, v1;
          seg_row8<V16>(a.V, (int64_t)r.vec * D + 512 * c + c0, v0, v1);
          const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) dacc[c][j] += (!DROP || ((kp >> j) & 1u)) ? (al * (double)vv[j] + M) - M : 0.0;
          if (DROP) {
#pragma unroll
            for (int j = 0; j < 8; ++j) dbsv[c & BC][j & BJ] += ((kp >> j) & 1u) ? rb : 0.0;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[c][j] = (float)dacc[c][j];
      bs = (float)dbs;
      if (DROP) {
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
          for (int j = 0; j < 8; ++j) bsv[c & BC][j & BJ] = (float)dbsv[c & BC][j & BJ];
      }
    }
    float rmx = 0.f;                                  // CNT: the largest of this lane's elements of the row
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (CH != 1) seg_row8<H16>(a.H, (int64_t)u * D + 512 * c + c0, xr0[c], xr1[c]);
      const float4 x0 = xr0[c], x1 = xr1[c];
      const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
      if constexpr (CNT) {
        const float cmx = fmaxf(fmaxf(fmaxf(xv[0], xv[1]), fmaxf(xv[2], xv[3])), fmaxf(fmaxf(xv[4], xv[5]), fmaxf(xv[6], xv[7])));
        if (__ballot(cmx >= 65504.f)) {               // (wave-uniform, rare)
#pragma unroll
          for (int j = 0; j < 8; ++j) n_sat += xv[j] >= 65504.f;
        }
        rmx = fmaxf(rmx, cmx);
      }
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        g[j] = xv[j] > 0.f ? (acc[c][j] - (DROP ? bsv[c & BC][j & BJ] * a.drop.scale : bs) * xv[j]) * sgm : 0.f;
        col[c][j] += g[j];
        gmx = fmaxf(gmx, fabsf(g[j]));
      }
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = T::from_float(g[2 * j]) | ((uint32_t)T::from_float(g[2 * j + 1]) << 16);
      *(uint4*)(a.dYu + (int64_t)u * a.Dp + 512 * c + c0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if constexpr (CNT) {
      if (!__ballot(rmx >= 6.103515625e-05f) && __ballot(rmx > 0.f)) ++n_faint;      // 2^-14: the smallest normal f16
    }
  }
  if constexpr (CNT) {
    __shared__ uint32_t hc[4][2];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_sat += __shfl_xor(n_sat, o, 64);
    if (lane == 0) { hc[wave][0] = n_sat; hc[wave][1] = n_faint; }
    __syncthreads();
    if (first && threadIdx.x == 0)
      *(uint2*)(a.h16_cnt + 2 * blockIdx.x) = make_uint2(hc[0][0] + hc[1][0] + hc[2][0] + hc[3][0], hc[0][1] + hc[1][1] + hc[2][1] + hc[3][1]);
  }
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) cs[wave][512 * c + c0 + j] = col[c][j];
  __syncthreads();
  if (first)
    for (int d = threadIdx.x; d < 512 * CH; d += 256)
        a.dbp[(int64_t)blockIdx.x * D + d] = (cs[0][d] + cs[1][d] + cs[2][d] + cs[3][d]) * (a.inv_sg / sgm);   // (sgm: a power of two, exact)
  if (a.guard.gg) {
    if (a.guard.proactive && blockIdx.x == 0 && threadIdx.x == 0) { a.guard.gg->shift[3] = pro_shift; a.guard.gg->mul = sgm; }   // for k_reduce
    __syncthreads();
    gg_end(a.guard, gg_block_max(gmx, &cs[0][0]));
  }
}

template <typename T, int CH, bool DROP = false, bool H16 = false, bool V16 = false>
__global__ __launch_bounds__(256) void k_seg_bwd(SegBwdArgs a) { seg_bwd_body<T, CH, DROP, H16, V16, false>(a); }
// ... the same over f16 rows, counting their range loss (SegBwdArgs::h16_cnt set: option "h16_guard" >= 1, guard round 0)
template <typename T, int CH, bool DROP = false, bool V16 = false>
__global__ __launch_bounds__(256) void k_seg_bwd_cnt(SegBwdArgs a) { seg_bwd_body<T, CH, DROP, true, V16, true>(a); }

void launch_seg_bwd(int prec, const SegBwdArgs& a, hipStream_t s) {
  const int ch = a.D / 512;
  // (a conditional repeat of the gradient-scale guard normally returns at once: a quarter of the grid starts faster)
  const dim3 grid(a.guard.round == 0 ? SEGB_BLOCKS : SEGB_BLOCKS / 4), block(256);
  const bool cnt = a.h16_cnt && a.h16 && a.guard.round == 0;      // the counting twins: one per H16 = true instantiation
  // V16 (the one-sweep score kernel's f16 vectors: SegBwdArgs::v16) exists at CH = 2 over f16 rows alone, and not with DROP (fp32
  // vectors: dropout steps run with v16 off)
  const bool v16 = ch == 2 && a.h16 && a.v16 && !a.drop.mode;
  with_prec(prec, [&](auto t) {
    using T = typename decltype(t)::type;
    if (v16) {
      if (cnt) VV_LAUNCH((k_seg_bwd_cnt<T, 2, false, true>), grid, block, 0, s, a);
      else VV_LAUNCH((k_seg_bwd<T, 2, false, true, true>), grid, block, 0, s, a);
      return;
    }
    with_flags([&](auto ch1, auto drop, auto h16) {
      constexpr int CH = ch1 ? 1 : 2;
      if constexpr (h16) { if (cnt) { VV_LAUNCH((k_seg_bwd_cnt<T, CH, drop>), grid, block, 0, s, a); return; } }
      VV_LAUNCH((k_seg_bwd<T, CH, drop, h16>), grid, block, 0, s, a);
    }, ch == 1, a.drop.mode, a.h16);
  });
}


void launch_score_loss(int prec, const ScoreArgs& a_in, hipStream_t s) {
  ScoreArgs a = a_in;
  ko().last_score_form = 4;
  a.items_rr = 1;          // per-instance rows (dense execution): an item's rows are contiguous already; XCD ranges measured + 1 us (42.8 against 41.8)
  if (ko().score_reg && (prec == 0 ? launch_score_loss_reg<F16>(a, s) : launch_score_loss_reg<BF16>(a, s))) return;
  const bool vec = a.D % 4 == 0;
  const bool wide = vec && a.D >= 2048 && a.B <= 512;       // few items of wide rows: sixteen waves per item
  // the two [G][D] partial-sum areas hold G D <= 4 NT floats (with the 1024-thread form and D = 2048 they ran over at a fixed 1024)
  const int nt = wide ? 1024 : SL_THREADS;
  const size_t lds = sizeof(float) * ((size_t)2 * a.D + 2 * (size_t)(a.D > 4 * nt ? a.D : 4 * nt) + 8 * (a.C + a.Nn) + 16);
  const dim3 grid(a.B), block(nt);
  auto launch = [&](auto t, auto fwd) {
    using T = typename decltype(t)::type;
    if (wide) VV_LAUNCH_LDS((k_score_loss<T, true, 1024, fwd>), grid, block, lds, s, a);
    else if (vec) VV_LAUNCH_LDS((k_score_loss<T, true, SL_THREADS, fwd>), grid, block, lds, s, a);
    else VV_LAUNCH_LDS((k_score_loss<T, false, SL_THREADS, fwd>), grid, block, lds, s, a);
  };
  // (FWD exists for F16 alone: the forward-only pass rounds nothing to 16 bits, one operand type serves both)
  if (a.fwd_only) launch(TypeTag<F16>{}, std::true_type{});
  else with_prec(prec, [&](auto t) { launch(t, std::false_type{}); });
}

// loss = scale * sum(loss_part), violations = sum(viol_part); fixed-order (deterministic)
__global__ void k_final_loss(const float* lp, const float* vp, int B, float scale, float* out2) {
  __shared__ float red[8];
  float l = 0.f, v = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) { l += lp[i]; v += vp[i]; }
  l = block_sum(l, red);
  v = block_sum(v, red + 4);
  if (threadIdx.x == 0) { out2[0] = l * scale; out2[1] = v; }
}
void launch_final_loss(const float* lp, const float* vp, int B, float scale, float* out2,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_final_loss, dim3(1), dim3(256), 0, s, lp, vp, B, scale, out2);
}

// The forward-only pass's loss reduction (vv_forward): one workgroup, the fold of the training path's loss workgroup (reduce_loss, kernels_update.hip:
// thread t adds partials t, t + 256, ... in order, then block_sum) -- the same bits from the same partials -- and the evaluation record:
// thread 0 alone updates it, so the sums are added in pass order with no atomics and nothing synchronises per pass.
__global__ __launch_bounds__(256) void k_eval_loss(const float* lp, const float* vp, int B, float scale, int64_t terms, EvalRec* rec) {
  __shared__ float red[8];
  float l = 0.f, v = 0.f;
  for (int i = threadIdx.x; i < B; i += 256) { l += lp[i]; v += vp[i]; }
  l = block_sum(l, red);
  v = block_sum(v, red + 4);
  if (threadIdx.x == 0) {
    const float loss = l * scale;
    rec->last_loss = loss; rec->last_viol = v;
    rec->loss_sum += (double)loss; rec->viol_sum += (double)v;      // (an fp32 value is exact in double)
    rec->passes += 1; rec->terms += terms;
  }
}
void launch_eval_loss(const float* lp, const float* vp, int B, float scale, int64_t terms, EvalRec* rec, hipStream_t s) {
  VV_LAUNCH(k_eval_loss, dim3(1), dim3(256), 0, s, lp, vp, B, scale, terms, rec);
}

}  // namespace vv
