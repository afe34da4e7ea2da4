// The frozen-weight image cache — the only file that reads or writes the cache's fields of ng_ctx (wimg, wver, wcache, wowner,
// wjobs_*, replay_token; ng_common.h states the contract of image_slot / image_pack) — and one kernel for every weight image
// of the step (round 4; pack_bodies.cuh has the bodies and the why).
//   pack_launch : ONE image now — first use of a cached image, or the cache is off (the job travels as a kernel argument)
//   repack_all  : every job registered in the context's image cache whose source weights lie inside the block Adam has
//                 just updated, in ONE launch behind the Adam kernel; the images then carry the new weight version and no
//                 consumer of the next step packs anything.  The job table lives in device memory and is uploaded only
//                 when the registry changes (a table in the kernel arguments indexed at run time is copied to scratch
//                 per thread: capi.hip, reduce_batch_kernel).
#include <algorithm>
#include <cstring>
#include <vector>

#include "pack_bodies.cuh"

namespace ng {

__global__ __launch_bounds__(PKB) void pack_one_kernel(PackJob j, unsigned ver) {
  pack_job_block(j, (int)blockIdx.x, (int)threadIdx.x, ver);
}

// block0[k] = first block of job k (ascending), block0[njobs] = grid
// `ver_dev` (armed launches: the word ng_replay_stage writes once per step, 0 = nothing staged): a recorded launch's `ver`
// argument is frozen at capture, and with one version at every replay a flag raised once could never be lowered again
__global__ __launch_bounds__(PKB) void repack_all_kernel(const PackJob* __restrict__ jobs, const unsigned* __restrict__ block0, int njobs,
                                                         unsigned ver, const unsigned* __restrict__ ver_dev) {
  if (ver_dev) { const unsigned staged = *ver_dev; ver = staged ? staged : ver; }
  int k = 0;
  for (int t = 1; t < njobs; ++t) k = blockIdx.x >= block0[t] ? t : k;      // uniform: scalar loads
  const PackJob j = jobs[k];
  pack_job_block(j, (int)(blockIdx.x - block0[k]), (int)threadIdx.x, ver);
}

unsigned pack_flag_version(const ng_ctx* ctx) { return (unsigned)ctx->wver | 0x80000000u; }

int pack_launch(ng_ctx* ctx, hipStream_t st, const PackJob& job) {
  if (job.kind == PK_NONE || job.blocks <= 0) return fail(ctx, NG_ERR_INVALID, "pack_launch: empty job");
  hipLaunchKernelGGL(pack_one_kernel, dim3(job.blocks), dim3(PKB), 0, st, job, pack_flag_version(ctx));
  NG_HIP(ctx, hipGetLastError());
  return NG_OK;
}

// the context's entry for (src, kind) with a buffer of `bytes`, *valid when it holds the image of the current weights;
// nullptr: not cacheable
static ng_ctx::WImage* cached_image(ng_ctx* ctx, const void* src, int kind, size_t bytes, bool* valid) {
  *valid = false;
  if (!ctx->wcache) return nullptr;
  // A source inside the context's own scratch is a temporary (a weight matrix repacked for THIS call: the same address
  // holds another layer's weights on the next call) — never a cache key.  Round-2 advisor finding: with the cache keyed
  // by such an address a frozen window around a multi-layer backward multiplied with the previous layer's image.
  auto inside = [&](const void* base, size_t n) {
    return base && (const char*)src >= (const char*)base && (const char*)src < (const char*)base + n;
  };
  if (inside(ctx->ws, ctx->ws_bytes) || inside(ctx->aux, ctx->aux_bytes)) return nullptr;
  ng_ctx::WImage& w = ctx->wimg[std::make_pair(src, kind)];
  if (w.bytes < bytes) {
    DeviceGuard dg(ctx->device);
    if (w.buf) { (void)hipDeviceSynchronize(); ctx->n_syncs++; (void)hipFree(w.buf); w.buf = nullptr; w.bytes = 0; }
    if (hipMalloc(&w.buf, bytes) != hipSuccess) { w.buf = nullptr; return nullptr; }
    ctx->n_allocs++;
    (void)hipMemset(w.buf, 0, bytes);      // (flag words inside an image start out equal to no version)
    w.bytes = bytes;
    w.ver = 0;
    w.has_job = false;                     // a registered job points into the old buffer
    ctx->wjobs_dirty = true;
  }
  *valid = w.ver == ctx->wver;
  w.ver = ctx->wver;
  return &w;
}

ImageSlot image_slot(ng_ctx* ctx, const void* src, ImageKind kind, size_t bytes, ImageScratch where, void* own) {
  bool fresh = false;
  if (ng_ctx::WImage* w = cached_image(ctx, src, kind, bytes, &fresh)) return ImageSlot{w->buf, true, fresh, w};
  if (!own && where != IMG_NONE) own = where == IMG_WS ? workspace(ctx, bytes) : aux_workspace(ctx, bytes);
  return ImageSlot{own, false, false, nullptr};
}

int image_pack(ng_ctx* ctx, hipStream_t st, const ImageSlot& slot, const PackJob& job) {
  if (slot.fresh) return NG_OK;
  if (int rc = pack_launch(ctx, st, job)) return rc;
  if (!slot.cached) return NG_OK;
  slot.entry->job = job;
  slot.entry->job.guard = RangeGuard{nullptr, 0};      // a per-call guard means nothing to a later refresh
  slot.entry->has_job = true;
  ctx->wjobs_dirty = true;
  return NG_OK;
}

void weights_bump(ng_ctx* ctx) { ctx->wver++; }

uint64_t image_cache_bytes(const ng_ctx* ctx) {
  uint64_t n = ctx->wjobs_cap + ctx->wjobs_private_bytes;
  for (auto& kv : ctx->wimg) n += kv.second.bytes;
  return n;
}

void image_cache_free(ng_ctx* ctx) {
  for (auto& kv : ctx->wimg)
    if (kv.second.buf) (void)hipFree(kv.second.buf);
  if (ctx->wjobs_dev) (void)hipFree(ctx->wjobs_dev);
  for (auto& kv : ctx->wjobs_private) (void)hipFree(kv.second);
}

int repack_all(ng_ctx* ctx, hipStream_t st, const void* lo, const void* hi) {
  if (!ctx->wcache || ctx->wimg.empty()) return NG_OK;
  auto inside = [&](const void* p) { return p == nullptr || ((const char*)p >= (const char*)lo && (const char*)p < (const char*)hi); };
  // the jobs to run: registered, and fed ONLY by weights of the updated block (an image with a source outside it may be
  // waiting for another ng_adam_step call: it stays invalid and is rebuilt at its next use, as before)
  std::vector<ng_ctx::WImage*> sel;
  for (auto& kv : ctx->wimg) {
    ng_ctx::WImage& w = kv.second;
    if (!w.has_job || !w.buf) continue;
    bool ok = true, any = false;
    for (const float* s : w.job.src) { ok = ok && inside(s); any = any || s != nullptr; }
    if (ok && any) sel.push_back(&w);
  }
  if (sel.empty()) return NG_OK;
  DeviceGuard dg(ctx->device);
  const int n = (int)sel.size();
  const size_t jobs_bytes = ((size_t)n * sizeof(PackJob) + 255) / 256 * 256;
  const size_t need = jobs_bytes + (size_t)(n + 1) * sizeof(unsigned);
  uint64_t hash = 1469598103934665603ull;      // which images, in which order, with which block counts
  for (ng_ctx::WImage* w : sel) {
    hash = (hash ^ (uint64_t)(uintptr_t)w->buf) * 1099511628211ull;
    hash = (hash ^ (uint64_t)w->job.blocks) * 1099511628211ull;
  }
  auto fill_host = [&](std::vector<char>& host, unsigned* blocks_out) {
    host.assign(need, 0);
    unsigned* b0 = reinterpret_cast<unsigned*>(host.data() + jobs_bytes);
    unsigned blocks = 0;
    for (int k = 0; k < n; ++k) {
      memcpy(host.data() + (size_t)k * sizeof(PackJob), &sel[k]->job, sizeof(PackJob));
      b0[k] = blocks;
      blocks += (unsigned)sel[k]->job.blocks;
    }
    b0[n] = blocks;
    *blocks_out = blocks;
  };
  const void* table = nullptr;
  int table_blocks = 0;
  const unsigned* ver_dev = nullptr;
  if (ctx->replay_armed) {
    if (const uint64_t* rs = replay_state(ctx)) ver_dev = reinterpret_cast<const unsigned*>(rs) + NG_REPLAY_VER_WORD;
    // a launch that may be captured (ng_replay_arm): its own immutable table.  The shared one below is rewritten whenever
    // another engine of the device updates its weights — a replayed step then rebuilt the OTHER engine's images (round 5:
    // two trainers on one device diverged at the second replayed step).  Uploaded by the warm-up steps, before any capture.
    hash = (hash ^ (uint64_t)n) * 1099511628211ull;
    for (ng_ctx::WImage* w : sel) {      // the whole job (sources, destinations, parameters) defines the table
      const unsigned char* jb = reinterpret_cast<const unsigned char*>(&w->job);
      for (size_t i = 0; i < sizeof(PackJob); ++i) hash = (hash ^ jb[i]) * 1099511628211ull;
    }
    unsigned blocks = 0;
    std::vector<char> host;
    fill_host(host, &blocks);
    auto it = ctx->wjobs_private.find(hash);
    if (it == ctx->wjobs_private.end()) {
      void* p = nullptr;
      if (hipMalloc(&p, need) != hipSuccess) return fail(ctx, NG_ERR_NOMEM, "repack_all: private job table");
      ctx->n_allocs++;
      ctx->wjobs_private_bytes += need;
      ctx->n_syncs++;
      NG_HIP(ctx, hipMemcpy(p, host.data(), need, hipMemcpyHostToDevice));      // synchronous: `host` is a local
      it = ctx->wjobs_private.emplace(hash, p).first;
    }
    table = it->second;
    table_blocks = (int)blocks;
    ctx->wjobs_private_sel[hash] = sel;
    ctx->replay_token = hash;
  } else {
  if (ctx->wjobs_dirty || ctx->wjobs_n != n || ctx->wjobs_hash != hash || ctx->wjobs_cap < need) {
    if (ctx->wjobs_cap < need) {
      if (ctx->wjobs_dev) { (void)hipStreamSynchronize(st); ctx->n_syncs++; (void)hipFree(ctx->wjobs_dev); ctx->wjobs_dev = nullptr; ctx->wjobs_cap = 0; }
      if (hipMalloc(&ctx->wjobs_dev, need * 2) != hipSuccess) return fail(ctx, NG_ERR_NOMEM, "repack_all: job table");
      ctx->n_allocs++;
      ctx->wjobs_cap = need * 2;
    }
    unsigned blocks = 0;
    fill_host(ctx->wjobs_host, &blocks);
    NG_HIP(ctx, hipMemcpyAsync(ctx->wjobs_dev, ctx->wjobs_host.data(), need, hipMemcpyHostToDevice, st));
    ctx->wjobs_n = n;
    ctx->wjobs_blocks = (int)blocks;
    ctx->wjobs_dirty = false;
    ctx->wjobs_hash = hash;
  }
  table = ctx->wjobs_dev;
  table_blocks = ctx->wjobs_blocks;
  }
  {
    ProfScope ps(ctx, st, "repack_all");
    const size_t jb = ((size_t)n * sizeof(PackJob) + 255) / 256 * 256;
    hipLaunchKernelGGL(repack_all_kernel, dim3(table_blocks), dim3(PKB), 0, st, (const PackJob*)table,
                       (const unsigned*)((const char*)table + jb), n, pack_flag_version(ctx), ver_dev);
    NG_HIP(ctx, hipGetLastError());
  }
  for (ng_ctx::WImage* w : sel) w->ver = ctx->wver;
  return NG_OK;
}

}  // namespace ng

extern "C" int ng_weights_frozen(ng_ctx* ctx, int owner) {
  if (!ctx) return NG_ERR_INVALID;
  if (owner != 0 && owner != ctx->wowner) {   // another model takes the cache over: nothing in it is its own
    ctx->wver++;
    ctx->wowner = owner;
    for (auto& kv : ctx->wimg) kv.second.has_job = false;     // (its weights may be gone: nothing of it is refreshed)
    ctx->wjobs_dirty = true;
  }
  ctx->wcache = owner != 0;
  return NG_OK;
}

extern "C" int ng_weights_changed(ng_ctx* ctx) {
  if (!ctx) return NG_ERR_INVALID;
  ctx->wver++;
  return NG_OK;
}

extern "C" int ng_replay_token(ng_ctx* ctx, uint64_t* token) {
  if (!ctx || !token) return NG_ERR_INVALID;
  *token = ctx->replay_token;
  return NG_OK;
}

// host bookkeeping of ONE replayed ng_adam_step: the weights moved, the captured repack launch rebuilt the images of `token`
extern "C" int ng_replay_commit(ng_ctx* ctx, uint64_t token) {
  if (!ctx) return NG_ERR_INVALID;
  ctx->wver++;
  auto it = ctx->wjobs_private_sel.find(token);
  if (token != 0 && it != ctx->wjobs_private_sel.end())
    for (ng_ctx::WImage* w : it->second)
      if (w->buf && w->has_job) w->ver = ctx->wver;
  return NG_OK;
}
