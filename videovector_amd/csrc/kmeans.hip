// kmeans.hip -- entry points of k-means on a gallery (include/videovec.h: vv_gallery_kmeans, vv_kmeans_init_rows, vv_kmeans_cfg_default).
// The kernels are in kernels_kmeans.hip, the similarity is launch_sim_f32 as the gallery calls run it, the sizes of every buffer are
// vv_kmeans_plan.h's.  Everything is queued on the context's stream with no host wait and no allocation between the first launch and the
// downloads at the end; of the context the call reads the km_block_rows option and writes the last_km_* ones.  None of this reads or
// writes the training step's state.  HAS NO REFERENCE COUNTERPART.
#include <algorithm>
#include <vector>

#include "vv_ctx.h"
#include "vv_rows.h"

using namespace vv;

extern "C" {

void vv_kmeans_cfg_default(vv_kmeans_cfg* cfg) {
  if (!cfg) return;
  cfg->num_clusters = 0; cfg->iters = 20; cfg->metric = VV_KMEANS_EUCLIDEAN; cfg->reserved_ = 0;
}

int vv_kmeans_init_rows(uint64_t seed, int32_t n, int32_t num_clusters, int32_t* rows_out) {
  if (!rows_out) return fail(VV_ERR_ARG, "vv_kmeans_init_rows: rows_out is NULL");
  if (n < 1) return fail(VV_ERR_ARG, "vv_kmeans_init_rows: n = %d", n);
  if (num_clusters < 1 || num_clusters > n) return fail(VV_ERR_ARG, "vv_kmeans_init_rows: num_clusters = %d is outside 1 .. n = %d", num_clusters, n);
  std::vector<int32_t> perm((size_t)n);
  rows_shuffled(seed, n, 1, perm.data());
  std::copy(perm.begin(), perm.begin() + num_clusters, rows_out);
  return VV_OK;
}

int vv_gallery_kmeans(vv_ctx* c, vv_gallery* items, const vv_kmeans_cfg* cfg, const float* init_centroids, const int32_t* init_rows,
                      float* centroids_out, int32_t* assign_out, int32_t* counts_out, double* objective_trace, int64_t* moved_trace,
                      vv_kmeans_report* out) {
  if (!c || !items || !cfg || !centroids_out || !out) return fail(VV_ERR_ARG, "vv_gallery_kmeans: NULL argument");
  return vv_kmeans_rows(c, gallery_rows(items), cfg, init_centroids, init_rows, centroids_out, assign_out, counts_out, objective_trace,
                        moved_trace, out, nullptr);
}

}  // extern "C"

// The call's body on device rows: vv_gallery_kmeans on its gallery's, pq.hip on a column slice of one (vv_ctx.h).
int vv_kmeans_rows(vv_ctx* c, const GalleryRows& gr, const vv_kmeans_cfg* cfg, const float* init_centroids, const int32_t* init_rows,
                   float* centroids_out, int32_t* assign_out, int32_t* counts_out, double* objective_trace, int64_t* moved_trace,
                   vv_kmeans_report* out, int32_t* assign_dev_out) {
  if (!c || !gr.feat || !cfg || !centroids_out || !out) return fail(VV_ERR_ARG, "vv_gallery_kmeans: NULL argument");
  if ((init_centroids != nullptr) == (init_rows != nullptr))
    return fail(VV_ERR_ARG, "vv_gallery_kmeans: exactly one of init_centroids and init_rows must be given");
  if (gr.ctx != c) return fail(VV_ERR_ARG, "vv_gallery_kmeans: the gallery belongs to another context");
  const int64_t n = gr.n_ref;
  const int C = cfg->num_clusters, iters = cfg->iters, Dp = gr.Dp, dim = gr.dim;
  if (C < 1 || C > KM_MAX_CLUSTERS) return fail(VV_ERR_ARG, "vv_gallery_kmeans: num_clusters = %d is outside 1 .. %d", C, KM_MAX_CLUSTERS);
  if (C > n) return fail(VV_ERR_ARG, "vv_gallery_kmeans: num_clusters = %d exceeds the gallery's %lld items", C, (long long)n);
  if (iters < 0) return fail(VV_ERR_ARG, "vv_gallery_kmeans: iters = %d is negative", iters);
  if (cfg->metric != VV_KMEANS_EUCLIDEAN && cfg->metric != VV_KMEANS_SPHERICAL) return fail(VV_ERR_ARG, "vv_gallery_kmeans: unknown metric %d", cfg->metric);
  if (Dp > 8192) return fail(VV_ERR_ARG, "vv_gallery_kmeans: rows of %d floats (8192 at most)", Dp);
  if (init_rows)
    for (int k = 0; k < C; ++k)
      if (init_rows[k] < 0 || init_rows[k] >= n)
        return fail(VV_ERR_ARG, "vv_gallery_kmeans: init_rows[%d] = %d is outside 0 .. %lld", k, init_rows[k], (long long)n - 1);
  const KmeansPlan p = kmeans_plan(n, dim, C, c->km_block_rows);
  if (!p.ok) return fail(VV_ERR_ARG, "vv_gallery_kmeans: %lld items in %d clusters do not fit the scratch limit", (long long)n, C);
  if (p.total_bytes + kmeans_record_bytes(iters) > GALLERY_SCRATCH_MAX)
    return fail(VV_ERR_ARG, "vv_gallery_kmeans: the record of %d iterations does not fit the scratch limit beside the call's %zu bytes", iters, p.total_bytes);
  VV_ENTER(c);
  const int euclid = cfg->metric == VV_KMEANS_EUCLIDEAN;
  const int passes = iters + 1;
  hipStream_t s = c->stream;

  DevTmp<float> score, cent, nn, part; DevTmp<int32_t> assign, list, hist, counts, start, cbase, nchunks, irows; DevTmp<double> slot;
  DevTmp<int4> chunks; DevTmp<KmRec> rec;
  HIPCHK(score.alloc((size_t)p.block_rows * C)); HIPCHK(cent.alloc((size_t)C * Dp)); HIPCHK(nn.alloc((size_t)C));
  HIPCHK(part.alloc((size_t)p.max_chunks * Dp)); HIPCHK(assign.alloc((size_t)n)); HIPCHK(list.alloc((size_t)n));
  HIPCHK(hist.alloc((size_t)p.tiles * C)); HIPCHK(counts.alloc((size_t)C)); HIPCHK(start.alloc((size_t)C + 1)); HIPCHK(cbase.alloc((size_t)C + 1));
  HIPCHK(nchunks.alloc(1)); HIPCHK(slot.alloc((size_t)p.slots)); HIPCHK(chunks.alloc((size_t)p.max_chunks)); HIPCHK(rec.alloc((size_t)passes));
  if (init_rows) HIPCHK(irows.alloc((size_t)C));
  // the timed iteration (the last one; with iters == 0 the only pass): events at the boundaries of its first KM_TIMED_BLOCKS blocks'
  // launches (a pass of more blocks reports those blocks' two legs scaled to all of them), at the pass's end, behind the grouping and
  // behind the update
  const int t_timed = std::max(0, iters - 1);
  const int64_t tb = std::min<int64_t>(p.blocks, KM_TIMED_BLOCKS);
  CallEvents ev;
  HIPCHK(ev.create((size_t)(2 * tb + 4)));
  const size_t e_pass = (size_t)(2 * tb + 1), e_group = e_pass + 1, e_update = e_group + 1;
  bool grouped = false;

  HIPCHK(hipMemsetAsync(rec, 0, (size_t)passes * sizeof(KmRec), s));
  HIPCHK(hipMemsetAsync(assign, 0xff, (size_t)n * 4, s));                // every item unassigned: -1
  HIPCHK(hipMemsetAsync(nn, 0, (size_t)C * 4, s));
  if (init_rows) {
    HIPCHK(hipMemcpyAsync(irows, init_rows, (size_t)C * 4, hipMemcpyHostToDevice, s));
    launch_km_gather(gr.feat, Dp, irows, C, cent, s);
  } else {
    if (Dp != dim) HIPCHK(hipMemsetAsync(cent, 0, (size_t)C * Dp * 4, s));
    HIPCHK(hipMemcpy2DAsync(cent, (size_t)Dp * 4, init_centroids, (size_t)dim * 4, (size_t)dim * 4, (size_t)C, hipMemcpyHostToDevice, s));
  }
  if (euclid) launch_km_finish(part, Dp, dim, counts, cbase, p.max_chunks, C, 1, 1, cent, nn, rec, s);
  int form = 0;
  for (int t = 0; t < passes; ++t) {
    const bool timed = t == t_timed;
    KmRec* r = rec.p + t;
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)C * 4, s));
    for (int64_t b = 0; b < p.blocks; ++b) {
      const int64_t r0 = b * p.block_rows;
      const int rows = (int)std::min<int64_t>(p.block_rows, n - r0);
      if (timed && b <= tb) HIPCHK(hipEventRecord(ev.e[2 * b], s));        // (b == tb: the end of the last timed block)
      launch_sim_f32(gr.feat + (size_t)r0 * Dp, cent, score, rows, C, Dp, C, s);
      if (timed && b < tb) HIPCHK(hipEventRecord(ev.e[2 * b + 1], s));
      form = launch_km_assign(score, C, r0, rows, euclid, nn, assign, counts, slot, r, s);
    }
    if (timed && tb == p.blocks) HIPCHK(hipEventRecord(ev.e[2 * tb], s));
    launch_km_fold(slot, p.slots, r, s);
    if (timed) HIPCHK(hipEventRecord(ev.e[e_pass], s));
    if (t == iters) break;
    launch_km_group(assign, n, C, p.tiles, counts, hist, start, cbase, chunks, p.max_chunks, nchunks, list, r, s);
    if (timed) HIPCHK(hipEventRecord(ev.e[e_group], s));
    launch_km_partial(gr.feat, n, Dp, list, chunks, nchunks, p.max_chunks, p.slices, part, s);
    launch_km_finish(part, Dp, dim, counts, cbase, p.max_chunks, C, euclid, 0, cent, nn, r, s);
    if (timed) { HIPCHK(hipEventRecord(ev.e[e_update], s)); grouped = true; }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipGetLastError());
  std::vector<KmRec> hrec((size_t)passes);
  std::vector<int32_t> hcounts;
  HIPCHK(hipMemcpyAsync(hrec.data(), rec, (size_t)passes * sizeof(KmRec), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpy2DAsync(centroids_out, (size_t)dim * 4, cent, (size_t)Dp * 4, (size_t)dim * 4, (size_t)C, hipMemcpyDeviceToHost, s));
  if (assign_out) HIPCHK(hipMemcpyAsync(assign_out, assign, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, counts, (size_t)C * 4, hipMemcpyDeviceToHost, s));
  if (assign_dev_out) HIPCHK(hipMemcpyAsync(assign_dev_out, assign, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                                       // the call's one wait

  for (int t = 0; t < passes; ++t) {
    if (objective_trace) objective_trace[t] = hrec[t].objective;
    if (moved_trace) moved_trace[t] = hrec[t].moved;
  }
  const KmRec& last = hrec[iters];
  out->n = n; out->num_clusters = C; out->iters = iters;
  out->empty_last = iters > 0 ? hrec[iters - 1].empty : 0; out->degenerate_last = iters > 0 ? hrec[iters - 1].degenerate : 0;
  out->moved_last = last.moved; out->objective_last = last.objective; out->nonfinite_rows = last.nonfinite;
  double ms_sim = 0, ms_assign = 0, ms_group = 0, ms_update = 0;
  for (int64_t b = 0; b < tb; ++b) {
    float a = 0, d = 0;
    HIPCHK(hipEventElapsedTime(&a, ev.e[2 * b], ev.e[2 * b + 1])); HIPCHK(hipEventElapsedTime(&d, ev.e[2 * b + 1], ev.e[2 * b + 2]));
    ms_sim += a; ms_assign += d;
  }
  ms_sim *= (double)p.blocks / (double)tb; ms_assign *= (double)p.blocks / (double)tb;
  if (grouped) {
    float a = 0, d = 0;
    HIPCHK(hipEventElapsedTime(&a, ev.e[e_pass], ev.e[e_group])); HIPCHK(hipEventElapsedTime(&d, ev.e[e_group], ev.e[e_update]));
    ms_group = a; ms_update = d;
  }
  c->last_km_blocks = (int)p.blocks; c->last_km_chunks = iters > 0 ? hrec[iters - 1].chunks : 0; c->last_km_assign_form = form;
  c->last_km_ms[0] = ms_sim; c->last_km_ms[1] = ms_assign; c->last_km_ms[2] = ms_group; c->last_km_ms[3] = ms_update;
  return VV_OK;
}
