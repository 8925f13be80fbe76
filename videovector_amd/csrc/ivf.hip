// ivf.hip -- entry points of the inverted-file index on a gallery (include/videovec.h: vv_ivf_create, vv_ivf_destroy, vv_ivf_search,
// vv_ivf_get, vv_ivf_lists).  The kernels are in kernels_ivf.hip, the probe's similarity is launch_sim_f32 as the gallery calls run it, the
// lists are built by the k-means grouping kernels as they stand, the sizes of every search buffer are vv_ivf_plan.h's.  A search queues
// everything on the context's stream with no host wait between its blocks and synchronises once, at its end; of the context it reads the
// ivf_block_rows / ivf_grid_wgs options.  None of this reads or writes the training step's state.  HAS NO REFERENCE COUNTERPART.
#include <algorithm>
#include <string>
#include <vector>

#include "vv_ctx.h"

using namespace vv;

struct vv_ivf {
  vv_ctx* ctx = nullptr;
  int64_t n_ref = 0;
  int dim = 0, Dp = 0, C = 0, metric = 0;
  float *rows = nullptr, *cent = nullptr, *nn = nullptr;       // [n_ref][Dp] cluster-contiguous, [C][Dp], [C] (EUCLIDEAN)
  int32_t *start = nullptr, *list = nullptr;                   // [C + 1], [n_ref]: position -> item index
  std::vector<int32_t> h_start;                                // host copy of start: the plan's pitch comes from it
  int largest = 0, empty = 0;
  char* scratch = nullptr; size_t scratch_cap = 0;             // one allocation, grown on demand, carved up by every search
  int64_t last_blocks = 0, last_tiles = 0, last_candidates = 0; int last_grid = 0;
  double last_ms[5] = {0, 0, 0, 0, 0};                         // probe, group, sim, select, the whole call
};

namespace {
struct IvfEvents {                                             // events that live for one call
  std::vector<hipEvent_t> e;
  ~IvfEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
void ivf_release(vv_ivf* ix) {
  dfree(ix->rows); dfree(ix->cent); dfree(ix->nn); dfree(ix->start); dfree(ix->list); dfree(ix->scratch);
  delete ix;
}
int ivf_build(vv_ctx* c, vv_ivf* ix, const GalleryRows& gr, const float* centroids, const int32_t* assign) {
  const int64_t n = ix->n_ref;
  const int C = ix->C, Dp = ix->Dp, dim = ix->dim;
  hipStream_t s = c->stream;
  const int64_t tiles = (n + KM_TILE - 1) / KM_TILE, max_chunks = n / KM_CHUNK + std::min<int64_t>(C, n);
  std::vector<int32_t> hcounts((size_t)C, 0);
  for (int64_t i = 0; i < n; ++i) ++hcounts[assign[i]];
  HIPCHK(hipMalloc((void**)&ix->rows, (size_t)n * Dp * 4)); HIPCHK(hipMalloc((void**)&ix->cent, (size_t)C * Dp * 4));
  HIPCHK(hipMalloc((void**)&ix->nn, (size_t)C * 4)); HIPCHK(hipMalloc((void**)&ix->start, ((size_t)C + 1) * 4));
  HIPCHK(hipMalloc((void**)&ix->list, (size_t)n * 4));
  DevTmp<int32_t> dassign, counts, hist, cbase, nchunks; DevTmp<int4> chunks; DevTmp<KmRec> rec;
  HIPCHK(dassign.alloc((size_t)n)); HIPCHK(counts.alloc((size_t)C)); HIPCHK(hist.alloc((size_t)tiles * C)); HIPCHK(cbase.alloc((size_t)C + 1));
  HIPCHK(nchunks.alloc(1)); HIPCHK(chunks.alloc((size_t)max_chunks)); HIPCHK(rec.alloc(1));
  HIPCHK(hipMemcpyAsync(dassign, assign, (size_t)n * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(counts, hcounts.data(), (size_t)C * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(rec, 0, sizeof(KmRec), s));
  // the lists: every cluster's items in ascending item index, the stable counting sort k-means runs
  launch_km_group(dassign, n, C, tiles, counts, hist, ix->start, cbase, chunks, max_chunks, nchunks, ix->list, rec, s);
  // the centroids, and under EUCLIDEAN nn_c as k-means forms it for centroids it is given
  if (Dp != dim) HIPCHK(hipMemsetAsync(ix->cent, 0, (size_t)C * Dp * 4, s));
  HIPCHK(hipMemcpy2DAsync(ix->cent, (size_t)Dp * 4, centroids, (size_t)dim * 4, (size_t)dim * 4, (size_t)C, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(ix->nn, 0, (size_t)C * 4, s));
  if (ix->metric == VV_KMEANS_EUCLIDEAN) launch_km_finish(nullptr, Dp, dim, nullptr, nullptr, 0, C, 1, 1, ix->cent, ix->nn, rec, s);
  // the cluster-contiguous copy of the rows: slab row p = item list[p]
  launch_km_gather(gr.feat, Dp, ix->list, (int)n, ix->rows, s);
  HIPCHK(hipGetLastError());
  ix->h_start.assign((size_t)C + 1, 0);
  HIPCHK(hipMemcpyAsync(ix->h_start.data(), ix->start, ((size_t)C + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int k = 0; k < C; ++k) {
    if (ix->h_start[k + 1] - ix->h_start[k] != hcounts[k]) return fail(VV_ERR_STATE, "vv_ivf_create: the device's list of cluster %d disagrees with the assignment", k);
    ix->largest = std::max(ix->largest, hcounts[k]); ix->empty += hcounts[k] == 0;
  }
  return VV_OK;
}
}  // namespace

extern "C" {

int vv_ivf_create(vv_ctx* c, vv_gallery* items, const float* centroids, int32_t C, int32_t metric, const int32_t* assign, vv_ivf** out) {
  if (!c) return fail(VV_ERR_ARG, "vv_ivf_create: ctx is NULL");
  if (!items) return fail(VV_ERR_ARG, "vv_ivf_create: items is NULL");
  if (!centroids) return fail(VV_ERR_ARG, "vv_ivf_create: centroids is NULL");
  if (!out) return fail(VV_ERR_ARG, "vv_ivf_create: out is NULL");
  const GalleryRows gr = gallery_rows(items);
  if (gr.ctx != c) return fail(VV_ERR_ARG, "vv_ivf_create: the items gallery belongs to another context");
  const int64_t n = gr.n_ref;
  if (C < 1 || C > KM_MAX_CLUSTERS) return fail(VV_ERR_ARG, "vv_ivf_create: C = %d is outside 1 .. %d", C, KM_MAX_CLUSTERS);
  if (C > n) return fail(VV_ERR_ARG, "vv_ivf_create: C = %d exceeds the gallery's %lld items", C, (long long)n);
  if (metric != VV_KMEANS_EUCLIDEAN && metric != VV_KMEANS_SPHERICAL) return fail(VV_ERR_ARG, "vv_ivf_create: unknown metric %d", metric);
  if (assign)
    for (int64_t i = 0; i < n; ++i)
      if (assign[i] < 0 || assign[i] >= C)
        return fail(VV_ERR_ARG, "vv_ivf_create: assign[%lld] = %d is outside 0 .. %d", (long long)i, assign[i], C - 1);
  std::vector<int32_t> own;
  if (!assign) {
    // what vv_gallery_kmeans with iters = 0 returns for these centroids and this metric: that call, not a restatement of it
    vv_kmeans_cfg cfg;
    vv_kmeans_cfg_default(&cfg);
    cfg.num_clusters = C; cfg.iters = 0; cfg.metric = metric;
    own.assign((size_t)n, 0);
    std::vector<float> cent_back((size_t)C * gr.dim);
    vv_kmeans_report rep;
    const int rc = vv_gallery_kmeans(c, items, &cfg, centroids, nullptr, cent_back.data(), own.data(), nullptr, nullptr, nullptr, &rep);
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)
      if (own[i] < 0 || own[i] >= C) return fail(VV_ERR_STATE, "vv_ivf_create: the assignment pass left item %lld in cluster %d", (long long)i, own[i]);
    assign = own.data();
  }
  VV_ENTER(c);
  vv_ivf* ix = new vv_ivf;
  ix->ctx = c; ix->n_ref = n; ix->dim = gr.dim; ix->Dp = gr.Dp; ix->C = C; ix->metric = metric;
  const int rc = ivf_build(c, ix, gr, centroids, assign);
  if (rc) { (void)hipStreamSynchronize(c->stream); ivf_release(ix); return rc; }
  *out = ix;
  return VV_OK;
}

int vv_ivf_destroy(vv_ctx* c, vv_ivf* ix) {
  if (!c) return fail(VV_ERR_ARG, "vv_ivf_destroy: ctx is NULL");
  if (!ix) return VV_OK;
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivf_destroy: the index belongs to another context");
  VV_ENTER(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  ivf_release(ix);
  return VV_OK;
}

int vv_ivf_get(const vv_ivf* ix, const char* name, double* value) {
  if (!ix || !name || !value) return fail(VV_ERR_ARG, "vv_ivf_get: NULL argument");
  const std::string n(name);
  if (n == "n_ref") *value = (double)ix->n_ref;
  else if (n == "dim") *value = ix->dim;
  else if (n == "num_clusters") *value = ix->C;
  else if (n == "metric") *value = ix->metric;
  else if (n == "largest_list") *value = ix->largest;
  else if (n == "empty_lists") *value = ix->empty;
  else if (n == "last_blocks") *value = (double)ix->last_blocks;
  else if (n == "last_tiles") *value = (double)ix->last_tiles;
  else if (n == "last_candidates") *value = (double)ix->last_candidates;
  else if (n == "last_grid_wgs") *value = ix->last_grid;
  else if (n == "last_probe_ms") *value = ix->last_ms[0];
  else if (n == "last_group_ms") *value = ix->last_ms[1];
  else if (n == "last_sim_ms") *value = ix->last_ms[2];
  else if (n == "last_select_ms") *value = ix->last_ms[3];
  else if (n == "last_device_ms") *value = ix->last_ms[4];
  else return fail(VV_ERR_ARG, "vv_ivf_get: unknown name '%s'", name);
  return VV_OK;
}

int vv_ivf_lists(vv_ctx* c, vv_ivf* ix, int32_t* start, int32_t* list) {
  if (!c || !ix || !start || !list) return fail(VV_ERR_ARG, "vv_ivf_lists: NULL argument");
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivf_lists: the index belongs to another context");
  VV_ENTER(c);
  HIPCHK(hipMemcpyAsync(start, ix->start, ((size_t)ix->C + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(list, ix->list, (size_t)ix->n_ref * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}

int vv_ivf_search(vv_ctx* c, vv_ivf* ix, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx, float* dist,
                  int32_t* n_candidates) {
  if (!c) return fail(VV_ERR_ARG, "vv_ivf_search: ctx is NULL");
  if (!ix) return fail(VV_ERR_ARG, "vv_ivf_search: index is NULL");
  if (!q) return fail(VV_ERR_ARG, "vv_ivf_search: q is NULL");
  if (!idx) return fail(VV_ERR_ARG, "vv_ivf_search: idx is NULL");
  if (!dist) return fail(VV_ERR_ARG, "vv_ivf_search: dist is NULL");
  if (ix->ctx != c) return fail(VV_ERR_ARG, "vv_ivf_search: the index belongs to another context");
  if (n_q < 1) return fail(VV_ERR_ARG, "vv_ivf_search: n_q = %d", n_q);
  const int C = ix->C, Dp = ix->Dp, dim = ix->dim;
  if (nprobe < 1 || nprobe > C || (nprobe > IVF_MAX_PROBE && nprobe != C))
    return fail(VV_ERR_ARG, "vv_ivf_search: nprobe = %d is neither in 1 .. %d nor the index's %d clusters", nprobe, std::min(C, IVF_MAX_PROBE), C);
  if (k < 1 || k > RT_MAX_K) return fail(VV_ERR_ARG, "vv_ivf_search: k = %d is outside 1 .. %d", k, RT_MAX_K);
  const IvfPlan p = ivf_plan(ix->n_ref, dim, C, nprobe, n_q, ivf_pitch_items(ix->h_start.data(), C, nprobe), c->ivf_block_rows, c->ivf_grid_wgs);
  if (!p.ok) return fail(VV_ERR_ARG, "vv_ivf_search: one query's %d probed lists of %lld items do not fit the scratch limit", nprobe, (long long)ix->n_ref);
  VV_ENTER(c);
  hipStream_t s = c->stream;
  if (p.total_bytes > ix->scratch_cap) {
    HIPCHK(hipStreamSynchronize(s));
    dfree(ix->scratch); ix->scratch = nullptr; ix->scratch_cap = 0;
    HIPCHK(hipMalloc((void**)&ix->scratch, p.total_bytes));
    ix->scratch_cap = p.total_bytes;
  }
  // the one allocation carved up: every buffer on IVF_ALIGN bytes (the plan counts IVF_BUFFERS of them)
  size_t used = 0; int taken = 0;
  auto take = [&](size_t bytes) { char* at = ix->scratch + used; used += (bytes + IVF_ALIGN - 1) / IVF_ALIGN * IVF_ALIGN; ++taken; return (void*)at; };
  const size_t R = (size_t)p.block_rows, P = (size_t)p.pairs;
  float* score = (float*)take(R * C * 4); float* qdev = (float*)take(R * Dp * 4); float* cand = (float*)take(R * p.pitch * 4);
  int32_t* m = (int32_t*)take(R * 4); int32_t* oidx = (int32_t*)take(R * RT_MAX_K * 4); float* odist = (float*)take(R * RT_MAX_K * 4);
  int32_t* probe = (int32_t*)take(P * 4); int32_t* off = (int32_t*)take(P * 4); int32_t* qlist = (int32_t*)take(P * 4);
  int32_t* hist = (int32_t*)take((size_t)p.pair_tiles * C * 4); int4* chunks = (int4*)take((size_t)p.max_chunks * 16);
  int32_t* counts = (int32_t*)take((size_t)C * 4); int32_t* qstart = (int32_t*)take(((size_t)C + 1) * 4); int32_t* cbase = (int32_t*)take(((size_t)C + 1) * 4);
  int4* tiles = (int4*)take((size_t)p.tile_cap * 16); KmRec* kmrec = (KmRec*)take(sizeof(KmRec)); IvfRec* rec = (IvfRec*)take(sizeof(IvfRec));
  int32_t* ntiles = (int32_t*)take(4); int32_t* nchunks = (int32_t*)take(4);
  if (used > ix->scratch_cap || taken > IVF_BUFFERS) return fail(VV_ERR_STATE, "vv_ivf_search: %zu bytes in %d buffers pass the plan's %zu", used, taken, p.total_bytes);

  const int64_t tb = std::min<int64_t>(p.blocks, IVF_TIMED_BLOCKS);
  IvfEvents ev;
  ev.e.assign((size_t)(5 * tb + 2), nullptr);
  for (hipEvent_t& x : ev.e) HIPCHK(hipEventCreate(&x));
  const size_t e_begin = (size_t)(5 * tb), e_end = e_begin + 1;
  const int all = nprobe == C, euclid = ix->metric == VV_KMEANS_EUCLIDEAN;

  HIPCHK(hipEventRecord(ev.e[e_begin], s));
  HIPCHK(hipMemsetAsync(rec, 0, sizeof(IvfRec), s));
  HIPCHK(hipMemsetAsync(kmrec, 0, sizeof(KmRec), s));
  if (Dp != dim) HIPCHK(hipMemsetAsync(qdev, 0, R * Dp * 4, s));      // the K padding of the query rows stays zero over the blocks
  for (int64_t b = 0; b < p.blocks; ++b) {
    const int64_t q0 = b * p.block_rows;
    const int rows = (int)std::min<int64_t>(p.block_rows, n_q - q0);
    const int64_t pairs = (int64_t)rows * nprobe;
    const bool timed = b < tb;
    hipEvent_t* e = timed ? &ev.e[(size_t)(5 * b)] : nullptr;
    if (timed) HIPCHK(hipEventRecord(e[0], s));
    // 1. probe
    HIPCHK(hipMemcpy2DAsync(qdev, (size_t)Dp * 4, q + (size_t)q0 * dim, (size_t)dim * 4, (size_t)dim * 4, (size_t)rows, hipMemcpyHostToDevice, s));
    launch_sim_f32(qdev, ix->cent, score, rows, C, Dp, C, s);
    HIPCHK(hipMemsetAsync(counts, 0, (size_t)C * 4, s));
    launch_ivf_probe(score, rows, C, nprobe, all, euclid, ix->nn, ix->start, probe, off, m, counts, rec, s);
    if (timed) HIPCHK(hipEventRecord(e[1], s));
    // 2. group the pairs by cluster, stably in ascending pair index; 3. the tile table
    launch_km_group(probe, pairs, C, (pairs + KM_TILE - 1) / KM_TILE, counts, hist, qstart, cbase, chunks, p.max_chunks, nchunks, qlist, kmrec, s);
    launch_ivf_tiles(ix->start, qstart, C, tiles, (int)p.tile_cap, ntiles, rec, s);
    if (timed) HIPCHK(hipEventRecord(e[2], s));
    // 4. grouped similarity
    IvfBlock blk;
    blk.Q = qdev; blk.slab = ix->rows; blk.start = ix->start; blk.list = ix->list; blk.probe = probe; blk.off = off; blk.qstart = qstart;
    blk.qlist = qlist; blk.tiles = tiles; blk.ntiles = ntiles; blk.cand = cand; blk.pitch = p.pitch; blk.rows = rows; blk.Dp = Dp; blk.C = C;
    blk.nprobe = nprobe; blk.tile_cap = (int)p.tile_cap;
    launch_sim_f32_grouped(blk, p.grid_wgs, s);
    if (timed) HIPCHK(hipEventRecord(e[3], s));
    // 5. select
    launch_ivf_select(blk, k, oidx, odist, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx + (size_t)q0 * k, oidx, (size_t)rows * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(dist + (size_t)q0 * k, odist, (size_t)rows * k * 4, hipMemcpyDeviceToHost, s));
    if (n_candidates) HIPCHK(hipMemcpyAsync(n_candidates + q0, m, (size_t)rows * 4, hipMemcpyDeviceToHost, s));
    if (timed) HIPCHK(hipEventRecord(e[4], s));
  }
  IvfRec hrec;
  HIPCHK(hipMemcpyAsync(&hrec, rec, sizeof(IvfRec), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev.e[e_end], s));
  HIPCHK(hipStreamSynchronize(s));                                       // the call's one wait

  double leg[4] = {0, 0, 0, 0};
  for (int64_t b = 0; b < tb; ++b)
    for (int l = 0; l < 4; ++l) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ev.e[(size_t)(5 * b + l)], ev.e[(size_t)(5 * b + l + 1)]));
      leg[l] += ms;
    }
  float total = 0;
  HIPCHK(hipEventElapsedTime(&total, ev.e[e_begin], ev.e[e_end]));
  for (int l = 0; l < 4; ++l) ix->last_ms[l] = leg[l] * (double)p.blocks / (double)tb;
  ix->last_ms[4] = total;
  ix->last_blocks = p.blocks; ix->last_tiles = hrec.tiles; ix->last_candidates = hrec.candidates; ix->last_grid = p.grid_wgs;
  return VV_OK;
}

}  // extern "C"
