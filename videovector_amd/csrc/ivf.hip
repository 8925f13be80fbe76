// ivf.hip -- entry points of the inverted-file index on a gallery (include/videovec.h: vv_ivf_create, vv_ivf_destroy, vv_ivf_search,
// vv_ivf_get, vv_ivf_lists).  The lists, their checks and accessors and the search loop are the coarse index's (vv_ivf_coarse.h,
// ivf_coarse.hip); this file adds what this index stores beside the lists -- the items' fp32 rows, cluster-contiguous -- and what a block
// of a search does between probe and select: the pairs grouped by cluster and the tile table, then the grouped similarity
// (kernels_ivf.hip).  The sizes of every search buffer are vv_ivf_plan.h's; of the context a search reads the ivf_block_rows /
// ivf_grid_wgs options.  HAS NO REFERENCE COUNTERPART.
#include <string>
#include <vector>

#include "vv_ivf_coarse.h"

using namespace vv;

struct vv_ivf : IvfCoarse {
  float* rows = nullptr;                                       // [n_ref][Dp] cluster-contiguous
  int64_t last_tiles = 0; int last_grid = 0;                   // last_ms[1], [2]: group, sim
};

namespace {
void ivf_release(vv_ivf* ix) {
  dfree(ix->rows); coarse_release(ix);
  delete ix;
}
int ivf_build(vv_ctx* c, vv_ivf* ix, const GalleryRows& gr, const float* centroids, const int32_t* assign) {
  const int rc = coarse_build("vv_ivf_create", ix, centroids, assign);
  if (rc) return rc;
  // the cluster-contiguous copy of the rows: slab row p = item list[p]
  HIPCHK(hipMalloc((void**)&ix->rows, (size_t)ix->n_ref * ix->Dp * 4));
  launch_km_gather(gr.feat, ix->Dp, ix->list, (int)ix->n_ref, ix->rows, c->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return VV_OK;
}
}  // namespace

extern "C" {

int vv_ivf_create(vv_ctx* c, vv_gallery* items, const float* centroids, int32_t C, int32_t metric, const int32_t* assign, vv_ivf** out) {
  GalleryRows gr;
  int rc = coarse_check("vv_ivf_create", c, items, centroids, {{"out", out}}, C, metric, &gr);
  if (rc) return rc;
  std::vector<int32_t> own;
  rc = coarse_assign("vv_ivf_create", c, items, gr, centroids, C, metric, &assign, &own);
  if (rc) return rc;
  VV_ENTER(c);
  vv_ivf* ix = new vv_ivf;
  ix->ctx = c; ix->n_ref = gr.n_ref; ix->dim = gr.dim; ix->Dp = gr.Dp; ix->C = C; ix->metric = metric;
  rc = ivf_build(c, ix, gr, centroids, assign);
  if (rc) { (void)hipStreamSynchronize(c->stream); ivf_release(ix); return rc; }
  *out = ix;
  return VV_OK;
}

int vv_ivf_destroy(vv_ctx* c, vv_ivf* ix) {
  const int rc = coarse_drain("vv_ivf_destroy", c, ix);
  if (!rc && ix) ivf_release(ix);
  return rc;
}

int vv_ivf_get(const vv_ivf* ix, const char* name, double* value) {
  if (!ix || !name || !value) return fail(VV_ERR_ARG, "vv_ivf_get: NULL argument");
  const std::string n(name);
  if (coarse_get(*ix, n, value)) return VV_OK;
  if (n == "last_tiles") *value = (double)ix->last_tiles;
  else if (n == "last_grid_wgs") *value = ix->last_grid;
  else if (n == "last_group_ms") *value = ix->last_ms[1];
  else if (n == "last_sim_ms") *value = ix->last_ms[2];
  else return fail(VV_ERR_ARG, "vv_ivf_get: unknown name '%s'", name);
  return VV_OK;
}

int vv_ivf_lists(vv_ctx* c, vv_ivf* ix, int32_t* start, int32_t* list) { return coarse_lists("vv_ivf_lists", c, ix, start, list); }

int vv_ivf_search(vv_ctx* c, vv_ivf* ix, const float* q, int32_t n_q, int32_t nprobe, int32_t k, int32_t* idx, float* dist,
                  int32_t* n_candidates) {
  IvfPlan p;
  int32_t *hist = nullptr, *qstart = nullptr, *cbase = nullptr, *qlist = nullptr, *ntiles = nullptr, *nchunks = nullptr;
  int4 *chunks = nullptr, *tiles = nullptr; KmRec* kmrec = nullptr;
  CoarseMiddle mid;
  mid.buffers = IVF_BUFFERS;
  mid.plan = [&](int64_t pitch_items) {
    p = ivf_plan(ix->n_ref, ix->dim, ix->C, nprobe, n_q, pitch_items, c->ivf_block_rows, c->ivf_grid_wgs);
    return CoarsePlan{p.ok, p.pitch, p.block_rows, p.blocks, p.total_bytes};
  };
  mid.carve = [&](const std::function<void*(size_t)>& take) {
    const size_t C = (size_t)ix->C;
    hist = (int32_t*)take((size_t)p.pair_tiles * C * 4); chunks = (int4*)take((size_t)p.max_chunks * 16);
    qstart = (int32_t*)take((C + 1) * 4); cbase = (int32_t*)take((C + 1) * 4); qlist = (int32_t*)take((size_t)p.pairs * 4);
    tiles = (int4*)take((size_t)p.tile_cap * 16); kmrec = (KmRec*)take(sizeof(KmRec));
    ntiles = (int32_t*)take(4); nchunks = (int32_t*)take(4);
  };
  mid.begin = [&]() -> int { HIPCHK(hipMemsetAsync(kmrec, 0, sizeof(KmRec), c->stream)); return VV_OK; };
  mid.block = [&](const CoarseBlock& b, const std::function<hipError_t()>& mark, IvfBlock* blk) -> int {
    hipStream_t s = c->stream;
    const int C = ix->C;
    const int64_t pairs = (int64_t)b.rows * nprobe;
    // the pairs grouped by cluster, stably in ascending pair index, and the tile table
    launch_km_group(b.probe, pairs, C, (pairs + KM_TILE - 1) / KM_TILE, b.counts, hist, qstart, cbase, chunks, p.max_chunks, nchunks, qlist, kmrec, s);
    launch_ivf_tiles(ix->start, qstart, C, tiles, (int)p.tile_cap, ntiles, b.rec, s);
    HIPCHK(mark());
    // the grouped similarity
    blk->slab = ix->rows; blk->qstart = qstart; blk->qlist = qlist; blk->tiles = tiles; blk->ntiles = ntiles; blk->tile_cap = (int)p.tile_cap;
    launch_sim_f32_grouped(*blk, p.grid_wgs, s);
    return VV_OK;
  };
  IvfRec rec;
  const int rc = coarse_search("vv_ivf_search", c, ix, q, n_q, nprobe, k, idx, dist, n_candidates, mid, &rec);
  if (rc) return rc;
  ix->last_tiles = rec.tiles; ix->last_grid = p.grid_wgs;
  return VV_OK;
}

}  // extern "C"
