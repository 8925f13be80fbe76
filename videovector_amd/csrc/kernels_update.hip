// kernels_update.hip -- the parameter update path of the videovec training step (gfx950 only).
//
//   k_reduce     : split-K slabs -> dW, per-item partials -> db (flat gradient buffer).
//   k_sgd        : SGDSolver::ComputeUpdateValue + Blob::Update in one pass
//                  (solver.cpp:502-531, blob.cpp:112-136), also refreshes the half copy of W.
//   k_reduce_sgd : k_reduce followed by k_sgd, element by element, in one launch.
//   k_grad_sumsq / k_grad_scale (gradient clipping), k_grad_bank (gradient accumulation), k_ema (moving average of the parameters),
//   k_scale_update / k_absmax / k_w_convert (the W -> half scale and copy), k_publish / k_delay.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "../../include/videovec.h"
#include "vv_internal.h"
#include "vv_elem_device.h"

namespace vv {

// 16-byte accesses with the non-temporal hint (streams that nobody reads again soon)
__device__ __forceinline__ float4 nt_load4(const float* p) {
  const f32x4 v = __builtin_nontemporal_load((const f32x4*)p);
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void nt_store4(float* p, const float4& v) {
  __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, (f32x4*)p);
}
// Four consecutive split-K partial products at element offset `off` of the slab buffer: fp32, or (S16, WgradArgs::slab16) f16 times the inverse
// factor of their (split, tile).  slab_tile: the tile of element (d, f) in the factor array's order (k_wgrad_gemm_ph: tm * tilesN + tn).
template <bool S16> __device__ __forceinline__ float4 slab_ld4(const float* slabs, int64_t off, float inv) {
  if constexpr (S16) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    const u32x2 q = __builtin_nontemporal_load((const u32x2*)((const uint16_t*)slabs + off));
    const h4 h = __builtin_bit_cast(h4, q);
    return make_float4((float)h[0] * inv, (float)h[1] * inv, (float)h[2] * inv, (float)h[3] * inv);
  } else {
    return nt_load4(slabs + off);
  }
}
__device__ __forceinline__ int slab_tile(int d, int f, int Fp) { return (d >> 8) * (Fp >> 8) + (f >> 8); }

// ------------------------------------------------------------------------------- reduce -------
// Blocks [0, nblk_dw) sum the split-K slabs into dW (grid-stride, 16-B accesses); the remaining
// blocks each own 64 bias columns and sum the per-item partials in a fixed order.
constexpr int RED_DW_BLOCKS = 2048;

// 16 bias columns per block, 16 row groups, 8 independent loads in flight per thread; the
// partial sums are combined in a fixed order (bit-reproducible, no atomics).  store(d, sum) for each of the
// block's columns d < D; part: the caller's 16 x 16 floats of LDS
template <typename Store>
__device__ __forceinline__ void db_colsum(const ReduceArgs& a, int blk, float (*part)[16], Store store) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int d = blk * 16 + tx;
  float s = 0.f;
  if (d < a.D) {
    const float* p = a.dbp + d;
    const int nb = a.db_rows > 0 ? a.db_rows : a.B;
    int b = ty;
    for (; b + 112 < nb; b += 128) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(b + 16 * u) * a.D];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < nb; b += 16) s += p[(int64_t)b * a.D];
  }
  part[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && d < a.D) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) t += part[u][tx];
    store(d, t);
  }
}
__device__ __forceinline__ void reduce_db(const ReduceArgs& a, int blk) {
  __shared__ float part[16][16];
  db_colsum(a, blk, part, [&](int d, float t) {      // (shard-major: every shard's db entries behind its rows)
    if (a.shard_rows > 0) a.grads[(int64_t)(d / a.shard_rows) * ((int64_t)a.shard_rows * a.F + a.shard_rows) + (int64_t)a.shard_rows * a.F + d % a.shard_rows] = t;
    else a.grads[(int64_t)a.D * a.F + d] = t;
  });
}

// loss = scale * sum(loss_part), violations = sum(viol_part); fixed-order (deterministic)
__device__ __forceinline__ void reduce_loss(const ReduceArgs& a) {
  __shared__ float red[8];
  float l = 0.f, v = 0.f;
  for (int i = threadIdx.x; i < a.B; i += 256) { l += a.loss_part[i]; v += a.viol_part[i]; }
  l = block_sum(l, red);
  v = block_sum(v, red + 4);
  if (threadIdx.x == 0) { a.loss_out[0] = l * a.loss_scale; a.loss_out[1] = v; }
  if (a.gmax_host) {
    // f16 rows of ip2 (option "h16_guard"): k_seg_bwd_cnt's per-workgroup partials, folded in a fixed order (integers: exact anyway)
    unsigned long long hsat = 0, hfaint = 0;
    if (a.h16_cnt) {
      __shared__ unsigned long long hred[4][2];
      for (int i = threadIdx.x; i < a.h16_cnt_n; i += 256) { const uint2 p = *(const uint2*)(a.h16_cnt + 2 * i); hsat += p.x; hfaint += p.y; }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { hsat += __shfl_xor(hsat, o, 64); hfaint += __shfl_xor(hfaint, o, 64); }
      if ((threadIdx.x & 63) == 0) { hred[threadIdx.x >> 6][0] = hsat; hred[threadIdx.x >> 6][1] = hfaint; }
      __syncthreads();
      hsat = hred[0][0] + hred[1][0] + hred[2][0] + hred[3][0]; hfaint = hred[0][1] + hred[1][1] + hred[2][1] + hred[3][1];
    }
    // f16 gradient-scale guard: the step's largest |dY| (unscaled: the normal pass's per-block maxima over the host's sg)
    // and the shift the repeats applied go to a host-visible ring; the host reads entry seq - 4 when it issues step seq
    __shared__ float gsm[16];
    float m = 0.f;
    for (int i = threadIdx.x; i < a.gmax_n0; i += 256) m = fmaxf(m, a.gmax_slots[i]);
    for (int i = threadIdx.x; i < a.gmax_n1; i += 256) m = fmaxf(m, a.gmax_slots[(size_t)a.gmax_stride + i]);
    m = gg_block_max(m, gsm);
    const float gbm = a.gbound ? gg_bound_fold(a.gbound, a.seq) : 0.f;
    if (threadIdx.x == 0) {
      // word 1: bits 0-15 the shift taken off on the device, bit 16 a conditional repeat ran, bit 30 a value passed the limit
      // in the step's FINAL round (cannot happen with the repeats / the proactive bound: the host treats it as an internal
      // error); high half: the proactive bound cnt_max x bound over the host's sg (0 on the other paths)
      unsigned fl = 0; float G = 0.f;
      if (a.gg) {
        fl = (unsigned)(a.gg->shift[3] & 0xFFFF) | (a.gg->repeat_seq == a.seq ? (1u << 16) : 0u) |
             (a.gg->flag[a.guard_last_round] == a.seq ? (1u << 30) : 0u);
        if (a.gbound) G = gbm * (float)(*a.gcnt) / a.sg;
      }
      unsigned long long* e = a.gmax_host + GMAX_ENTRY_WORDS * (a.seq & 15);
      __hip_atomic_store(e + 2, hsat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // words 2, 3: the f16 rows' saturated elements and faint rows (0 where nothing counted)
      __hip_atomic_store(e + 3, hfaint, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(e + 1, ((unsigned long long)__float_as_uint(G) << 32) | fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(e, ((unsigned long long)__float_as_uint(m / a.sg) << 32) | (unsigned)a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// next W->half scale from the running max: f16 keeps max|W|*sw in [2^11, 2^12); bf16 needs none.  One 256-thread workgroup.
__device__ __forceinline__ void scale_update_body(Scales* sc, const float* wmax_blocks, int nblocks, int prec) {
  __shared__ float red[8];
  float mm = 0.f;
  if (wmax_blocks)
    for (int i = threadIdx.x; i < nblocks; i += 256) mm = fmaxf(mm, wmax_blocks[i]);
  waves_max_to_lds(mm, red, threadIdx.x >> 6);
  if (threadIdx.x != 0) return;
  sc->sw_next = half_scale(fmaxf(lds_max<4>(red), __uint_as_float(sc->wmax_bits)), prec);
  sc->wmax_bits = 0u;
}

// where element (d, f) of dW goes in the gradient buffer: flat, chunk-major (ReduceArgs::n_chunks) or shard-major (ReduceArgs::shard_rows:
// every shard carries its db entries behind its rows)
__device__ __forceinline__ int64_t dw_offset(const ReduceArgs& a, int d, int f) {
  int64_t o = (int64_t)d * a.F + f;
  if (a.n_chunks > 0) {
    int cc = 0;
    while (cc + 1 < a.n_chunks && f >= a.chunk_c0[cc + 1]) ++cc;
    const int c0 = a.chunk_c0[cc], c1 = a.chunk_c0[cc + 1];
    o = (int64_t)a.D * c0 + (int64_t)d * (c1 - c0) + (f - c0);
  }
  if (a.shard_rows > 0) o += (int64_t)(d / a.shard_rows) * a.shard_rows;
  return o;
}

template <bool VEC, bool S16 = false>
__global__ __launch_bounds__(256) void k_reduce(ReduceArgs a) {
  // The few workgroups with serial work (bias columns: a loop over the per-block partials; loss; scale) are numbered last
  // but DISPATCHED first: the 2048 dW workgroups fill every CU's block slots, and a workgroup that only starts when the
  // first of them retires adds its own loop to the kernel's length (measured: 16.7 us with them last).
  const int n_special = (a.scale_sc ? 1 : 0) + ((a.parts & 2) ? (a.D + 15) / 16 + 1 : 0);
  int bid = (int)blockIdx.x < n_special ? (int)gridDim.x - n_special + (int)blockIdx.x : (int)blockIdx.x - n_special;
  // a pending W -> half scale update of the PREVIOUS step's SGD kernel rides as the last workgroup (its own one-workgroup
  // launch cost ~5 us of stream time a step: the kernel plus two dependent-launch gaps); this step's k_sgd reads the result
  const int G = (int)gridDim.x - (a.scale_sc ? 1 : 0);
  if (bid == G) { scale_update_body(a.scale_sc, a.scale_wmax, a.scale_n, a.scale_prec); return; }
  if (a.parts & 2) {
    if (bid == G - 1) { reduce_loss(a); return; }
    const int ndb = (a.D + 15) / 16;
    if (bid >= G - 1 - ndb) { reduce_db(a, bid - (G - 1 - ndb)); return; }
  }
  if (!(a.parts & 1)) return;
  const float inv = grad_unscale(a.ip_scale, a.sg, a.gg, a.sg_dev, a.scales);
  const int64_t slab_sz = slab_pitch(a.Dp, a.Fp);
  const int d0 = a.d_begin, dn = a.d_count > 0 ? a.d_count : a.D;
  if (VEC) {
    const int fb = a.f_count > 0 ? a.f_begin : 0, fn = a.f_count > 0 ? a.f_count : a.F;
    const int f4 = fn / 4;
    const int nblk = (int)gridDim.x - (a.scale_sc ? 1 : 0) - ((a.parts & 2) ? (a.D + 15) / 16 + 1 : 0);      // this launch's dW blocks
    for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < (int64_t)dn * f4;
         i += (int64_t)nblk * 256) {
      const int d = d0 + (int)(i / f4), f = fb + (int)(i % f4) * 4;
      const float* p = a.slabs + (int64_t)d * a.Fp + f;
      if constexpr (S16) {             // f16 partial products: every split's four values times the inverse factor of its tile, summed in slab order
        const int64_t po = (int64_t)d * a.Fp + f;
        const int tiles = (a.Dp >> 8) * (a.Fp >> 8), tl = slab_tile(d, f, a.Fp);
        float4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = u < a.S ? slab_ld4<true>(a.slabs, u * slab_sz + po, a.slab_sc[u * tiles + tl]) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 s = t[0];
#pragma unroll
        for (int u = 1; u < 8; ++u)
          if (u < a.S) { s.x += t[u].x; s.y += t[u].y; s.z += t[u].z; s.w += t[u].w; }
        *(float4*)(a.grads + dw_offset(a, d, f)) = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
        continue;
      }
      float4 s = nt_load4(p);
      int k = 1;
      if (a.S == 8) {                  // the usual split: all eight loads in flight at once, summed in slab order
        float4 t[7];
#pragma unroll
        for (int u = 0; u < 7; ++u) t[u] = nt_load4(p + (u + 1) * slab_sz);
#pragma unroll
        for (int u = 0; u < 7; ++u) { s.x += t[u].x; s.y += t[u].y; s.z += t[u].z; s.w += t[u].w; }
        k = 8;
      }
      for (; k + 3 < a.S; k += 4) {
        const float4 t0 = *(const float4*)(p + (k + 0) * slab_sz), t1 = *(const float4*)(p + (k + 1) * slab_sz);
        const float4 t2 = *(const float4*)(p + (k + 2) * slab_sz), t3 = *(const float4*)(p + (k + 3) * slab_sz);
        s.x += t0.x; s.y += t0.y; s.z += t0.z; s.w += t0.w;
        s.x += t1.x; s.y += t1.y; s.z += t1.z; s.w += t1.w;
        s.x += t2.x; s.y += t2.y; s.z += t2.z; s.w += t2.w;
        s.x += t3.x; s.y += t3.y; s.z += t3.z; s.w += t3.w;
      }
      for (; k < a.S; ++k) {
        const float4 t = *(const float4*)(p + k * slab_sz);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
      }
      *(float4*)(a.grads + dw_offset(a, d, f)) = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    }
  } else {
    const int64_t nW = (int64_t)dn * a.F;
    for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < nW; i += (int64_t)RED_DW_BLOCKS * 256) {
      const int d = d0 + (int)(i / a.F), f = (int)(i % a.F);
      float s = 0.f;
      for (int k = 0; k < a.S; ++k) s += a.slabs[k * slab_sz + (int64_t)d * a.Fp + f];
      a.grads[(int64_t)d * a.F + f] = s * inv;
    }
  }
}
void launch_reduce(const ReduceArgs& a, hipStream_t s) {
  // dW blocks (fewer for a launch that reduces a column range only), db blocks, the loss block, the scale block
  const int dwb = !(a.parts & 1) ? 0 : (a.f_count > 0 && a.F % 4 == 0 ? std::max(64, (int)((int64_t)RED_DW_BLOCKS * a.f_count / a.F)) : RED_DW_BLOCKS);
  const dim3 grid(dwb + ((a.parts & 2) ? (a.D + 15) / 16 + 1 : 0) + (a.scale_sc ? 1 : 0));
  if (a.F % 4 == 0 && a.slab16) VV_LAUNCH((k_reduce<true, true>), grid, dim3(256), 0, s, a);     // (slab16 needs F % 8 == 0 and S <= 8: vv_backward_plan.h)
  else if (a.F % 4 == 0) VV_LAUNCH(k_reduce<true>, grid, dim3(256), 0, s, a);
  else VV_LAUNCH(k_reduce<false>, grid, dim3(256), 0, s, a);
}

// ------------------------------------------------------------------------------- SGD ----------
// solver.cpp:502-531: g += local_decay * w (L2) | sign(w) (L1); h = local_rate * g + momentum * h;
// blob.cpp:118-120: w -= h.  Also writes the scaled half copy used by the next forward and tracks
// max |w| for the f16 range guard.
// A = SgdArgs2: the two-history form (Adam, SolverRule::step2) -- instantiations of their own with the sibling's access widths, so that
// the one-history kernels carry neither the second pointer nor its loads; v is read and written once: non-temporal like W and the history.
// RMS: the instantiation that also knows RMSProp (SolverRule::step<RMS>); the others are the parent's code for the three older rules.
template <typename T, bool VEC, typename A = SgdArgs, bool RMS = false>
__global__ __launch_bounds__(256) void k_sgd(A a) {
  constexpr bool H2 = std::is_same<A, SgdArgs2>::value;
  if (a.skip_if && __hip_atomic_load(a.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;   // (a failed exchange in front: SgdArgs::skip_if)
  const float sw = a.scales->sw_next;
  const int64_t nW = (int64_t)a.D * a.F;
  const SolverRule& rule = a.rule;
  const float lr_w = rule.rate * rule.lr_mult_w, dc_w = rule.weight_decay * rule.decay_mult_w;
  float wmax = 0.f;
  auto upd = [&](float w, float g, float& h) {
    w = rule.template step<RMS>(w, g, h, lr_w, dc_w);
    wmax = fmaxf(wmax, fabsf(w));
    return w;
  };
  auto upd2 = [&](float w, float g, float& h, float& v) {
    w = rule.step2(w, g, h, v, lr_w, dc_w);
    wmax = fmaxf(wmax, fabsf(w));
    return w;
  };
  if (VEC) {       // F % 4 == 0: 16-B accesses, one row segment per thread
    const int fc = a.chunked ? a.f_count : a.F;              // this launch's columns: one F-chunk, or all
    const int f4 = fc / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)a.D * f4;
         i += (int64_t)gridDim.x * 256) {
      const int d = (int)(i / f4), fl = (int)(i % f4) * 4, f = a.f_begin + fl;
      const int64_t o = (int64_t)d * a.F + f;
      const int64_t og = a.chunked ? (int64_t)a.D * a.f_begin + (int64_t)d * fc + fl : o;     // chunk-major gradient buffer
      float4 w = nt_load4(a.W + o), h = nt_load4(a.hW + o);
      const float4 g = nt_load4(a.grads + og);
      if constexpr (H2) {
        float4 v = nt_load4(a.vW + o);
        w.x = upd2(w.x, g.x, h.x, v.x); w.y = upd2(w.y, g.y, h.y, v.y); w.z = upd2(w.z, g.z, h.z, v.z); w.w = upd2(w.w, g.w, h.w, v.w);
        nt_store4(a.vW + o, v);
      } else {
      w.x = upd(w.x, g.x, h.x); w.y = upd(w.y, g.y, h.y); w.z = upd(w.z, g.z, h.z); w.w = upd(w.w, g.w, h.w);
      }
      nt_store4(a.W + o, w);
      nt_store4(a.hW + o, h);
      const uint2 q = pack_half4<T>(w.x, w.y, w.z, w.w, sw);
      if (a.pub_flag) __hip_atomic_store((unsigned long long*)(a.Wh + (int64_t)d * a.Fp + f), ((unsigned long long)q.y << 32) | q.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *(uint2*)(a.Wh + (int64_t)d * a.Fp + f) = q;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nW; i += (int64_t)gridDim.x * 256) {
      float h = a.hW[i];
      float w;
      if constexpr (H2) { float v = a.vW[i]; w = upd2(a.W[i], a.grads[i], h, v); a.vW[i] = v; }
      else w = upd(a.W[i], a.grads[i], h);
      a.hW[i] = h;
      a.W[i] = w;
      const int d = (int)(i / a.F), f = (int)(i % a.F);
      a.Wh[(int64_t)d * a.Fp + f] = T::from_float(w * sw);
    }
  }
  const float lr_b = rule.rate * rule.lr_mult_b, dc_b = rule.weight_decay * rule.decay_mult_b;
  for (int d = blockIdx.x * 256 + threadIdx.x; a.do_bias && d < a.D; d += gridDim.x * 256) {
    float h = a.hb[d];
    float bn;
    if constexpr (H2) { float v = a.vb[d]; bn = rule.step2(a.b[d], a.grads[nW + d], h, v, lr_b, dc_b); a.vb[d] = v; }
    else bn = rule.template step<RMS>(a.b[d], a.grads[nW + d], h, lr_b, dc_b);
    if (a.pub_flag) __hip_atomic_store(a.b + d, bn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else a.b[d] = bn;
    a.hb[d] = h;
  }
  // per-block max |w| -> one slot per block (no atomics: thousands of adds on one address
  // serialise at ~12 ns each); k_scale_update folds the slots.  (Folding them in this kernel's last workgroup instead --
  // an arrival counter -- was measured: the 1024 counter adds made the kernel 10 us longer, the saved launch is ~3 us.)
  __shared__ float wm[4];
  waves_max_to_lds(wmax, wm, threadIdx.x >> 6);
  if (threadIdx.x == 0) {
    // (published launches: at agent scope like everything else a kernel of the COMPUTE stream reads behind the gates -- the scale
    // workgroup of the next k_reduce folds these slots and is ordered behind this kernel by the gate flag only, not by its end)
    const float wmb = lds_max<4>(wm);
    if (a.pub_flag) __hip_atomic_store(a.wmax_blocks + a.blk_off + blockIdx.x, wmb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else a.wmax_blocks[a.blk_off + blockIdx.x] = wmb;
    if (blockIdx.x == 0 && a.set_scale) {
      if (a.pub_flag) __hip_atomic_store(&a.scales->sw_cur, sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else a.scales->sw_cur = sw;
    }
  }
  if (a.pub_flag) {                    // SgdArgs::pub_flag: every wave's stores have landed before the workgroup counts itself in
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(a.pub_count, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == (int)gridDim.x - 1) {
        __hip_atomic_store(a.pub_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.pub_flag, a.pub_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
__global__ void k_publish(int32_t* flag, int32_t seq) { __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// test hook (VV_COMM_TEST_DELAY_US): holds a stream for `us` microseconds, so that the gated forward GEMM really waits
__global__ void k_delay(int us) {
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
  while (__builtin_amdgcn_s_memrealtime() - t0 < (uint64_t)us * 100) __builtin_amdgcn_s_sleep(16);
}
void launch_delay(int us, hipStream_t s) { hipLaunchKernelGGL(k_delay, dim3(1), dim3(1), 0, s, us); }
void launch_publish(int32_t* flag, int32_t seq, hipStream_t s) { hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, s, flag, seq); }
// SolverRule::solver_type -> the kernels' args type / RMS pair, for launch_sgd and launch_reduce_sgd: f(args, RMS) with the two-history
// args A2 for Adam (solver.hip provides the second history), RMS = true for the instantiations that know RMSProp, the plain form otherwise.
template <typename A2, typename A, typename F> static void with_solver(const A& a, const SolverRule& rule, const char* who, float* vW, float* vb, F&& f) {
  if (rule.solver_type == VV_SOLVER_ADAM) {
    if (!vW || !vb) { fprintf(stderr, "%s: an Adam rule without its second history\n", who); abort(); }      // (a caller's bug: never a null store on the device)
    A2 a2; (A&)a2 = a; a2.vW = vW; a2.vb = vb;
    f(a2, std::false_type{});
  }
  else if (rule.solver_type == VV_SOLVER_RMSPROP) f(a, std::true_type{});
  else f(a, std::false_type{});
}
void launch_sgd(int prec, const SgdArgs& a, hipStream_t s, float* vW, float* vb) {
  const bool vec = a.F % 4 == 0;
  ko().last_update_form = vec ? 1 : 2;    // ("last_update_form": the chunked and the sharded update pass here too, F % 4 == 0 both)
  const dim3 grid(a.chunked ? a.n_blk : SGD_BLOCKS), block(256);
  with_solver<SgdArgs2>(a, a.rule, "launch_sgd", vW, vb, [&](const auto& args, auto rms) {
    using A = std::decay_t<decltype(args)>;
    with_prec(prec, [&](auto t) {
      using T = typename decltype(t)::type;
      if (vec) VV_LAUNCH((k_sgd<T, true, A, rms>), grid, block, 0, s, args);
      else VV_LAUNCH((k_sgd<T, false, A, rms>), grid, block, 0, s, args);
    });
  });
}

// ------------------------------------------------------------------------------- gradient clipping ----
// BVLC Caffe's SGDSolver::ClipGradients (sgd_solver.cpp; the reference tree has no such function): the L2 norm of ALL parameter gradients
// -- the flat buffer [dW | db] -- and, where it exceeds the threshold, g *= threshold / norm, before the regulariser and the rule.
// The buffer splits the same way in both kernels: the floats in front of the first 16-byte boundary (none in the library's own buffer;
// a bound one may start at any float), 16-byte items, the floats behind the last whole item.
struct ClipSplit { int64_t head, n4, tail0, rest; };
__device__ __forceinline__ ClipSplit clip_split(const float* g, int64_t n) {
  ClipSplit p;
  p.head = std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) / 4));
  p.n4 = (n - p.head) / 4;
  p.tail0 = p.head + p.n4 * 4;
  p.rest = p.head + (n - p.tail0);      // the scalar elements: at most 3 + 3, thread j of the grid takes the j-th
  return p;
}
// k_grad_sumsq: a FIXED grid of CLIP_BLOCKS x 256 threads; thread t squares items t, t + grid, ... in that order into four double sums
// (one per lane of the item; a float's square is exact in double), folds them as (x + y) + (z + w), adds its scalar element; the wave
// folds by halves (lane l += lane l + 32, 16, ... 1), the workgroup adds its four waves in order, and the workgroup that arrives last
// adds the CLIP_BLOCKS partials in index order.  No atomics on the sum: the same buffer gives the same bits on every run and on every
// rank.  That last workgroup forms norm and scale in double, rounds each once, and writes the record.
__global__ __launch_bounds__(256) void k_grad_sumsq(ClipArgs a) {
  if (a.skip_if && __hip_atomic_load(a.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const ClipSplit p = clip_split(a.g, a.n);
  const float4* g4 = (const float4*)(a.g + p.head);
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)CLIP_BLOCKS * 256;
  double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
  for (int64_t i = tid; i < p.n4; i += nth) {
    const float4 v = g4[i];
    sx += (double)v.x * (double)v.x; sy += (double)v.y * (double)v.y; sz += (double)v.z * (double)v.z; sw += (double)v.w * (double)v.w;
  }
  double s = (sx + sy) + (sz + sw);
  if (tid < p.rest) {
    const double v = (double)a.g[tid < p.head ? tid : p.tail0 + (tid - p.head)];
    s += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  __shared__ double ws[CLIP_BLOCKS > 4 ? CLIP_BLOCKS : 4];
  __shared__ int last;
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double b = ((ws[0] + ws[1]) + ws[2]) + ws[3];
    __hip_atomic_store(a.part + blockIdx.x, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // (release: the partial is visible at agent scope before the count; acquire: the last arrival sees every other partial)
    last = __hip_atomic_fetch_add(a.arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (uint32_t)CLIP_BLOCKS - 1;
  }
  __syncthreads();
  if (!last) return;
  for (int i = threadIdx.x; i < CLIP_BLOCKS; i += 256) ws[i] = __hip_atomic_load(a.part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sumsq = 0.0;
#pragma unroll 8
  for (int i = 0; i < CLIP_BLOCKS; ++i) sumsq += ws[i];
  const double norm = sqrt(sumsq);
  const float norm_f = (float)norm;
  const bool clipped = norm_f > a.clip;             // strictly, in fp32 as BVLC compares (norm == clip and norm == 0 scale nothing)
  ClipRec& r = *a.rec;
  r.sumsq = sumsq; r.norm = norm_f;
  r.scale = clipped ? (float)((double)a.clip / norm) : 1.f;     // (clipped: norm > clip >= 0, no division by zero)
  r.clipped = clipped ? 1 : 0;
  r.updates += 1; r.clipped_updates += clipped ? 1 : 0;
  __hip_atomic_store(a.arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // for the next launch
}
// k_grad_scale: g[i] = g[i] * scale -- one fp32 multiply per element -- where the record says the step is clipped
__global__ __launch_bounds__(256) void k_grad_scale(ClipArgs a) {
  if (a.skip_if && __hip_atomic_load(a.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  if (!a.rec->clipped) return;
  const float sc = a.rec->scale;
  const ClipSplit p = clip_split(a.g, a.n);
  float4* g4 = (float4*)(a.g + p.head);
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  for (int64_t i = tid; i < p.n4; i += nth) {
    float4 v = g4[i];
    v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
    g4[i] = v;
  }
  if (tid < p.rest) a.g[tid < p.head ? tid : p.tail0 + (tid - p.head)] *= sc;
}
void launch_grad_sumsq(const ClipArgs& a, hipStream_t s) { VV_LAUNCH(k_grad_sumsq, dim3(CLIP_BLOCKS), dim3(256), 0, s, a); }
void launch_grad_scale(const ClipArgs& a, hipStream_t s) { VV_LAUNCH(k_grad_scale, dim3(SGD_BLOCKS), dim3(256), 0, s, a); }

// ------------------------------------------------------------------------------- gradient accumulation ----
// BVLC Caffe's SolverParameter.iter_size (the reference tree has none): Solver::Step runs iter_size forward/backward passes whose layers
// add into the parameter diffs, and SGDSolver::Normalize multiplies the sum by Dtype(1) / iter_size in front of the regulariser and the
// rule.  k_grad_bank is the three element-wise passes of that over flat [dW | db] buffers (BankOp): Store dst = src, Add dst = dst + src
// (one fp32 add), Scale dst = src * inv (one fp32 multiply; src == dst allowed).  A FIXED grid of BANK_BLOCKS x 256 threads; thread t owns
// the 16-byte items t, t + grid, ... (non-temporal: each stream is read or written once per pass) and at most one of the scalar floats in
// front of the first 16-byte boundary / behind the last whole item, split as clip_split does by dst's address.  The host gives src the
// same offset from a boundary (the bank is placed that way); should the two ever differ -- a buffer bound in mid-cycle -- the launch
// takes every element as a scalar.  Every element has one owner and there are no atomics: the result is bit-reproducible.
// Thread 0 of the grid keeps the cycle's loss record (BankArgs::fold).
template <BankOp OP> __device__ __forceinline__ float bank_op(float s, float d, float inv) {
  if constexpr (OP == BankOp::Store) return s;
  else if constexpr (OP == BankOp::Add) return d + s;
  else return s * inv;
}
template <BankOp OP> __global__ __launch_bounds__(256) void k_grad_bank(BankArgs a) {
  if (a.skip_if && __hip_atomic_load(a.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)BANK_BLOCKS * 256;
  if (tid == 0 && a.fold == 1) {
    AccumRec& r = *a.rec;
    r.loss_sum = bank_op<OP>(a.loss2[0], r.loss_sum, 1.f); r.viol_sum = bank_op<OP>(a.loss2[1], r.viol_sum, 1.f);
  }
  if (tid == 0 && a.fold == 2) {
    AccumRec& r = *a.rec;
    r.last_mean_loss = r.loss_sum * a.inv; r.last_mean_viol = r.viol_sum * a.inv; r.last_count = a.m; r.updates += 1;
  }
  if ((((uintptr_t)a.src ^ (uintptr_t)a.dst) & 15) != 0) {          // no common 16-byte grid: scalars throughout
    for (int64_t i = tid; i < a.n; i += nth) a.dst[i] = bank_op<OP>(a.src[i], OP == BankOp::Add ? a.dst[i] : 0.f, a.inv);
    return;
  }
  const ClipSplit p = clip_split(a.dst, a.n);
  for (int64_t i = tid; i < p.n4; i += nth) {
    const int64_t o = p.head + i * 4;
    const float4 s = nt_load4(a.src + o);
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (OP == BankOp::Add) d = nt_load4(a.dst + o);
    nt_store4(a.dst + o, make_float4(bank_op<OP>(s.x, d.x, a.inv), bank_op<OP>(s.y, d.y, a.inv), bank_op<OP>(s.z, d.z, a.inv), bank_op<OP>(s.w, d.w, a.inv)));
  }
  if (tid < p.rest) {
    const int64_t o = tid < p.head ? tid : p.tail0 + (tid - p.head);
    a.dst[o] = bank_op<OP>(a.src[o], OP == BankOp::Add ? a.dst[o] : 0.f, a.inv);
  }
}
void launch_grad_bank(BankOp op, const BankArgs& a, hipStream_t s) {
  const dim3 grid(BANK_BLOCKS), block(256);
  if (op == BankOp::Store) VV_LAUNCH(k_grad_bank<BankOp::Store>, grid, block, 0, s, a);
  else if (op == BankOp::Add) VV_LAUNCH(k_grad_bank<BankOp::Add>, grid, block, 0, s, a);
  else VV_LAUNCH(k_grad_bank<BankOp::Scale>, grid, block, 0, s, a);
}

// ------------------------------------------------------------------------------- moving average of the parameters ----
// vv_ema_set (this project's own; neither the reference tree nor BVLC Caffe keeps one): e = decay * e + om * w behind every update.
// k_ema streams the matrix and then the bias in k_grad_bank's shape: a FIXED grid of EMA_BLOCKS x 256 threads; VEC -- thread t owns the
// 16-byte items t, t + grid, ... of each stream (non-temporal: 4 bytes read of W, 4 read and 4 written of e per element, none of it read
// again before the next update) and the bias's D % 4 last floats go one to a thread; scalar (F % 4 != 0) -- one float per thread and
// pass.  One owner per element, no atomics.  The two products and the sum are separate fp32 operations (contraction is off in
// ema_rule), so the result is the numpy-float32 restatement's bit for bit.
__device__ __forceinline__ float ema_rule(float e, float w, float decay, float om) {
#pragma clang fp contract(off)
  const float p = decay * e;
  const float q = om * w;
  return p + q;
}
template <bool VEC> __device__ __forceinline__ void ema_stream(const float* w, float* e, int64_t n, float decay, float om, int64_t tid, int64_t nth) {
  if constexpr (VEC) {
    const int64_t n4 = n / 4;
    for (int64_t i = tid; i < n4; i += nth) {
      const float4 x = nt_load4(w + i * 4), y = nt_load4(e + i * 4);
      nt_store4(e + i * 4, make_float4(ema_rule(y.x, x.x, decay, om), ema_rule(y.y, x.y, decay, om), ema_rule(y.z, x.z, decay, om), ema_rule(y.w, x.w, decay, om)));
    }
    const int64_t o = n4 * 4 + tid;             // the floats behind the last whole item: at most three
    if (o < n) e[o] = ema_rule(e[o], w[o], decay, om);
  } else {
    for (int64_t i = tid; i < n; i += nth) e[i] = ema_rule(e[i], w[i], decay, om);
  }
}
template <bool VEC> __global__ __launch_bounds__(256) void k_ema(EmaArgs a) {
  if (a.skip_if && __hip_atomic_load(a.skip_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)EMA_BLOCKS * 256;
  ema_stream<VEC>(a.W, a.eW, a.nW, a.decay, a.om, tid, nth);
  ema_stream<VEC>(a.b, a.eb, (int64_t)a.nb, a.decay, a.om, tid, nth);
}
void launch_ema(const EmaArgs& a, bool vec, hipStream_t s) {
  const dim3 grid(EMA_BLOCKS), block(256);
  if (vec) VV_LAUNCH(k_ema<true>, grid, block, 0, s, a);
  else VV_LAUNCH(k_ema<false>, grid, block, 0, s, a);
}

__global__ void k_scale_update(Scales* sc, const float* wmax_blocks, int nblocks, int prec) { scale_update_body(sc, wmax_blocks, nblocks, prec); }
void launch_scale_update(int prec, Scales* sc, const float* wmax_blocks, int n_blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_scale_update, dim3(1), dim3(256), 0, s, sc, wmax_blocks, n_blocks, prec);
}

// ------------------------------------------------------------------------------- reduction + update in one launch ----
// k_reduce_sgd = k_reduce followed by k_sgd, element by element: a thread sums its 16 bytes of the eight slabs, scales them
// (the gradient, stored for whoever asks: non-temporal), and applies the solver's rule to the same 16 bytes of W right
// there -- the gradient is not written and read back between two launches, and one dependent launch boundary goes.  Same
// sums in the same order, the same rule(): bit for bit the parameters of the two-launch form (tests/test_gpu_fused_update.py).
// The W -> half scale that k_scale_update would have computed between the two launches is derived by every parameter
// workgroup for itself from the previous update's per-block maxima (4-8 KB out of L2, while its slab loads fly).
// (Round 4, residency: 76 registers = six workgroups per CU resident, the eight of a CU in two uneven rounds.  A one-element form at 57
// registers with all eight resident is SLOWER (23.7 against 21.8 us), so is every cap below six (LDS-limited 5 / 4 / 3 per CU: 23.8-25 /
// 24.7 / 29.5 us); half or a quarter of the workgroups with two / four elements per thread: the same 21.3-22.6 us.)
// FA = FusedUpdArgs2: the two-history form (Adam), as k_sgd's -- 16-byte accesses of v beside those of the history, two per eight elements
// on f16 slabs, non-temporal.
template <typename T, bool S16 = false, typename FA = FusedUpdArgs, bool RMS = false>
__global__ __launch_bounds__(256) void k_reduce_sgd(FA fa) {
  constexpr bool H2 = std::is_same<FA, FusedUpdArgs2>::value;
  const ReduceArgs& a = fa.r;
  const SgdArgs& g = fa.g;
  const int ndb = (a.D + 15) / 16;
  const int n_special = ndb + 1;
  const int bid = (int)blockIdx.x < n_special ? (int)gridDim.x - n_special + (int)blockIdx.x : (int)blockIdx.x - n_special;
  const int G = (int)gridDim.x;
  const SolverRule& rule = g.rule;
  if (bid == G - 1) { reduce_loss(a); return; }
  if (bid >= G - 1 - ndb) {
    // bias columns: the partials' sum is the gradient (stored), and the bias is updated from it on the spot
    __shared__ float part[16][16];
    db_colsum(a, bid - (G - 1 - ndb), part, [&](int d, float t) {
      a.grads[(int64_t)a.D * a.F + d] = t;
      float h = g.hb[d];
      if constexpr (H2) { float v = fa.vb[d]; g.b[d] = rule.step2(g.b[d], t, h, v, rule.rate * rule.lr_mult_b, rule.weight_decay * rule.decay_mult_b); fa.vb[d] = v; }
      else g.b[d] = rule.template step<RMS>(g.b[d], t, h, rule.rate * rule.lr_mult_b, rule.weight_decay * rule.decay_mult_b);
      g.hb[d] = h;
    });
    return;
  }
  // ---- parameter workgroups: 16-byte elements, one per thread at the benchmark's size (2048 workgroups), more for larger matrices
  const int nblk = G - n_special;
  const int f4 = a.F / 4;
  const int64_t n4 = (int64_t)a.D * f4;
  const int64_t slab_sz = slab_pitch(a.Dp, a.Fp);
  int64_t i = (int64_t)bid * 256 + threadIdx.x;
  // the first element's loads fly while the scale is worked out
  float4 t[8], w = make_float4(0.f, 0.f, 0.f, 0.f), h = w, v = w, v1 = w;     // (v, v1: the second history, H2 only)
  auto load = [&](int64_t ii) {
    const int d = (int)(ii / f4), f = (int)(ii % f4) * 4;
    const int64_t po = (int64_t)d * a.Fp + f;
    if constexpr (S16) {
      const int tiles = (a.Dp >> 8) * (a.Fp >> 8), tl = slab_tile(d, f, a.Fp);
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = u < a.S ? slab_ld4<true>(a.slabs, u * slab_sz + po, a.slab_sc[u * tiles + tl]) : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = u < a.S ? nt_load4(a.slabs + po + u * slab_sz) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int64_t o = (int64_t)d * a.F + f;
    w = nt_load4(g.W + o); h = nt_load4(g.hW + o);
    if constexpr (H2) v = nt_load4(fa.vW + o);
  };
  // S16 (f16 partial products): EIGHT elements per thread -- 16-byte loads of the eight slabs (8-byte accesses run at ~0.6 of the 16-byte rate
  // per byte), two 16-byte accesses each for W and the history, one 16-byte store of the half copy; the same per-element arithmetic in the same
  // order as the four-element form and as k_reduce + k_sgd (bit-identical parameters, tests/test_gpu_fused_update.py)
  typedef _Float16 h8v __attribute__((ext_vector_type(8)));
  typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
  const int f8 = a.F / 8;
  const int64_t n8 = (int64_t)a.D * f8;
  h8v t8[8]; float sc8[8]; float4 w1 = w, h1 = w;
  auto load8 = [&](int64_t ii) {
    const int d = (int)(ii / f8), f = (int)(ii % f8) * 8;
    const int64_t po = (int64_t)d * a.Fp + f;
    const int tiles = (a.Dp >> 8) * (a.Fp >> 8), tl = slab_tile(d, f, a.Fp);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (u < a.S) {
        t8[u] = __builtin_bit_cast(h8v, __builtin_nontemporal_load((const u32x4v*)((const uint16_t*)a.slabs + u * slab_sz + po)));
        sc8[u] = a.slab_sc[u * tiles + tl];
      } else { t8[u] = h8v{0, 0, 0, 0, 0, 0, 0, 0}; sc8[u] = 0.f; }
    }
    const int64_t o = (int64_t)d * a.F + f;
    w = nt_load4(g.W + o); w1 = nt_load4(g.W + o + 4); h = nt_load4(g.hW + o); h1 = nt_load4(g.hW + o + 4);
    if constexpr (H2) { v = nt_load4(fa.vW + o); v1 = nt_load4(fa.vW + o + 4); }
  };
  if constexpr (S16) { if (i < n8) load8(i); }
  else { if (i < n4) load(i); }
  // the scale of the new half copy
  float sw = g.scales->sw_next;
  __shared__ float red[4];
  if (fa.recompute_scale) sw = fold_scale<4>(fa.wmax_prev, fa.wmax_prev_n, g.scales, fa.prec, red, threadIdx.x >> 6);
  const float inv = grad_unscale(a.ip_scale, a.sg, a.gg, a.sg_dev, a.scales);
  const float lr_w = rule.rate * rule.lr_mult_w, dc_w = rule.weight_decay * rule.decay_mult_w;
  float wmax = 0.f;
  if constexpr (S16) {
    for (; i < n8; ) {
      const int d = (int)(i / f8), f = (int)(i % f8) * 8;
      const int64_t o = (int64_t)d * a.F + f;
      float gr[8], wn[8], hn[8];
      const float w8[8] = {w.x, w.y, w.z, w.w, w1.x, w1.y, w1.z, w1.w}, hh8[8] = {h.x, h.y, h.z, h.w, h1.x, h1.y, h1.z, h1.w};
      float vn[8] = {v.x, v.y, v.z, v.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float sj = (float)t8[0][j] * sc8[0];
#pragma unroll
        for (int u = 1; u < 8; ++u)
          if (u < a.S) sj += (float)t8[u][j] * sc8[u];
        gr[j] = __fmul_rn(sj, inv);
        hn[j] = hh8[j];
        if constexpr (H2) wn[j] = rule.step2(w8[j], gr[j], hn[j], vn[j], lr_w, dc_w);
        else wn[j] = rule.template step<RMS>(w8[j], gr[j], hn[j], lr_w, dc_w);
        wmax = fmaxf(wmax, fabsf(wn[j]));
      }
      if (fa.store_grads) { nt_store4(a.grads + o, make_float4(gr[0], gr[1], gr[2], gr[3])); nt_store4(a.grads + o + 4, make_float4(gr[4], gr[5], gr[6], gr[7])); }
      i += (int64_t)nblk * 256;
      if (i < n8) load8(i);                      // the next element's loads before this one's stores
      nt_store4(g.W + o, make_float4(wn[0], wn[1], wn[2], wn[3])); nt_store4(g.W + o + 4, make_float4(wn[4], wn[5], wn[6], wn[7]));
      nt_store4(g.hW + o, make_float4(hn[0], hn[1], hn[2], hn[3])); nt_store4(g.hW + o + 4, make_float4(hn[4], hn[5], hn[6], hn[7]));
      if constexpr (H2) { nt_store4(fa.vW + o, make_float4(vn[0], vn[1], vn[2], vn[3])); nt_store4(fa.vW + o + 4, make_float4(vn[4], vn[5], vn[6], vn[7])); }
      const uint2 q0 = pack_half4<T>(wn[0], wn[1], wn[2], wn[3], sw), q1 = pack_half4<T>(wn[4], wn[5], wn[6], wn[7], sw);
      *(uint4*)(g.Wh + (int64_t)d * g.Fp + f) = make_uint4(q0.x, q0.y, q1.x, q1.y);
    }
  } else
  for (; i < n4; ) {
    const int d = (int)(i / f4), f = (int)(i % f4) * 4;
    const int64_t o = (int64_t)d * a.F + f;
    float4 s = t[0];
    for (int u = 1; u < 8; ++u)
      if (u < a.S) { s.x += t[u].x; s.y += t[u].y; s.z += t[u].z; s.w += t[u].w; }
    // (rounded products, as the two-launch form stores them: no contraction into the rule's first multiply-add)
    const float4 gr = make_float4(__fmul_rn(s.x, inv), __fmul_rn(s.y, inv), __fmul_rn(s.z, inv), __fmul_rn(s.w, inv));
    if (fa.store_grads) nt_store4(a.grads + o, gr);
    float4 wn = w, hn = h, vn = v;
    if constexpr (H2) {
      wn.x = rule.step2(wn.x, gr.x, hn.x, vn.x, lr_w, dc_w); wn.y = rule.step2(wn.y, gr.y, hn.y, vn.y, lr_w, dc_w);
      wn.z = rule.step2(wn.z, gr.z, hn.z, vn.z, lr_w, dc_w); wn.w = rule.step2(wn.w, gr.w, hn.w, vn.w, lr_w, dc_w);
    } else {
    wn.x = rule.template step<RMS>(wn.x, gr.x, hn.x, lr_w, dc_w); wn.y = rule.template step<RMS>(wn.y, gr.y, hn.y, lr_w, dc_w);
    wn.z = rule.template step<RMS>(wn.z, gr.z, hn.z, lr_w, dc_w); wn.w = rule.template step<RMS>(wn.w, gr.w, hn.w, lr_w, dc_w);
    }
    wmax = fmaxf(wmax, fmaxf(fmaxf(fabsf(wn.x), fabsf(wn.y)), fmaxf(fabsf(wn.z), fabsf(wn.w))));
    i += (int64_t)nblk * 256;
    if (i < n4) load(i);                       // the next element's loads before this one's stores
    nt_store4(g.W + o, wn);
    nt_store4(g.hW + o, hn);
    if constexpr (H2) nt_store4(fa.vW + o, vn);
    *(uint2*)(g.Wh + (int64_t)d * g.Fp + f) = pack_half4<T>(wn.x, wn.y, wn.z, wn.w, sw);
  }
  __shared__ float wm[4];
  update_end<4>(wmax, wm, threadIdx.x >> 6, g.wmax_blocks + bid, bid == 0, g.scales, sw, fa.recompute_scale);
}
int launch_reduce_sgd(const FusedUpdArgs& a, hipStream_t s, float* vW, float* vb) {
  const int ndb = (a.r.D + 15) / 16;
  const int ept = a.r.slab16 ? 8 : 4;                                       // elements per thread (k_reduce_sgd's S16 form: eight)
  const int nblk = a.no_params ? 0 : (int)std::min<int64_t>(((int64_t)a.r.D * (a.r.F / ept) + 255) / 256, WMAX_SLOTS);
  const dim3 grid(nblk + ndb + 1);
  ko().last_update_form = a.no_params ? 5 : a.r.slab16 ? 4 : 3;     // ("last_update_form"; no_params: the matrix was updated in the weight-gradient GEMM)
  // (Adam never comes with no_params: the epilogue declines it, vv_backward_plan.h)
  with_solver<FusedUpdArgs2>(a, a.g.rule, "launch_reduce_sgd", vW, vb, [&](const auto& args, auto rms) {
    using FA = std::decay_t<decltype(args)>;
    with_prec(a.prec, [&](auto t) {
      using T = typename decltype(t)::type;
      if (a.r.slab16) VV_LAUNCH((k_reduce_sgd<T, true, FA, rms>), grid, dim3(256), 0, s, args);
      else VV_LAUNCH((k_reduce_sgd<T, false, FA, rms>), grid, dim3(256), 0, s, args);
    });
  });
  return nblk;
}

__global__ __launch_bounds__(256) void k_absmax(const float* x, int64_t n, unsigned* out_bits) {
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    m = fmaxf(m, fabsf(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out_bits, __float_as_uint(m));
}
void launch_absmax(const float* x, int64_t n, unsigned* out_bits, hipStream_t s) {
  hipLaunchKernelGGL(k_absmax, dim3(512), dim3(256), 0, s, x, n, out_bits);
}

template <typename T>
__global__ __launch_bounds__(256) void k_w_convert(const float* W, uint16_t* Wh, int D, int F,
                                                   int Fp, Scales* sc) {
  const float sw = sc->sw_next;
  const int64_t nW = (int64_t)D * F;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nW; i += (int64_t)gridDim.x * 256) {
    const int d = (int)(i / F), f = (int)(i % F);
    Wh[(int64_t)d * Fp + f] = T::from_float(W[i] * sw);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) sc->sw_cur = sw;
}
void launch_w_convert(int prec, const float* W, uint16_t* Wh, int D, int F, int Dp, int Fp,
                      Scales* sc, hipStream_t s) {
  (void)Dp;
  if (prec == 0) hipLaunchKernelGGL(k_w_convert<F16>, dim3(1024), dim3(256), 0, s, W, Wh, D, F, Fp, sc);
  else hipLaunchKernelGGL(k_w_convert<BF16>, dim3(1024), dim3(256), 0, s, W, Wh, D, F, Fp, sc);
}

}  // namespace vv
