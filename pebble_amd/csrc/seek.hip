// seek.hip — batched SeekGE / SeekLT over a decoded batch, on the device
// (device side).
//
// Per-block mode is blockiter.Data.SeekGE / SeekLT (sstable/blockiter/
// block_iter.go:19-108; rowblk_iter.go:606-781, :782-1054) in a named block;
// table mode is singleLevelIterator.SeekGE / SeekLT (sstable/
// reader_iter_single_lvl.go:757-898): the index finds the first block whose
// last key is >= the query, the data block is searched, and an exhausted block
// is left for its neighbour.  The decoded arrays never leave HBM.
//
//   seek_fence_count_kernel / seek_fence_kernel  (pbl_seek_prepare) the fence
//       table: the blocks that decoded (PBL_OK) and hold a KV, compacted in
//       batch order, one 32-B record each (the first 16 bytes of the block's
//       last user key's Split-prefix as two big-endian words, that length, the
//       block id, the block's KV base)
//   seek_kernel<comparer>  lane per query: binary search over the fence
//       (decided from registers when the two prefixes differ inside the bytes
//       both records hold, else by the full compare), binary search inside
//       the block, the HideObsoletePoints skip, the flags, three plain stores
//
//   seek_kernel<comparer, true>  (pbl_seek_prefix_batch) SeekPrefixGE with
//       useFilterBlock (reader_iter_single_lvl.go:1037-1107): the same kernel
//       behind one more predicate, the table's bloom filter asked for the
//       query's Split-prefix (filter_core.hip.h); an excluded query's lane does
//       no search
//
// seek_one<R> (seek_core.hip.h, shared with scan.hip) is the whole search; the
// kernel instantiates it with GlobalReader and pbl_seek_batch_host with
// cmp::HostReader.  The comparers are key_cmp.hip.h's; GlobalReader specialises
// only the bytewise compare.
#include <algorithm>
#include <vector>

#include "filter_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace seek {

struct FenceArgs {
  pbl_decode_out d;
  uint32_t n_blocks, comparer;
  uint8_t* ws;
};
struct SeekArgs {
  pbl_decode_out d;
  pbl_seek_queries q;
  pbl_seek_out out;
  uint32_t n_blocks;
  const uint8_t* ws;
  const uint8_t* filter;  // pbl_seek_prefix_batch only
  uint64_t filter_len;
};

// What SeekPrefixGE asks the filter before it searches: 0 to go on, else the
// flags of the answer -- PBL_SEEK_FILTERED when the filter excludes the query's
// Split-prefix (no search), PBL_SEEK_BAD_BLOCK for a corrupt filter, which
// excludes nothing.
template <class R, uint32_t kCmp>
PBL_HD inline uint8_t filter_gate(typename R::template ptr<const uint8_t> filter, uint64_t filter_len,
                                  typename R::template ptr<const uint8_t> q_bytes,
                                  typename R::template ptr<const uint64_t> q_off, uint64_t i) {
  const filter::Header H = filter::bloom_parse<R>(filter, filter_len);
  if (H.status != PBL_OK) return PBL_SEEK_BAD_BLOCK;
  const uint64_t q0 = q_off[i];
  const uint32_t h = filter::prefix_hash<R>(kCmp, q_bytes + q0, q_off[i + 1] - q0);
  return filter::bloom_may<R>(filter, H, h) ? 0 : PBL_SEEK_FILTERED;
}

__device__ inline View<GlobalReader> fence_view(const FenceArgs& A) {
  pbl_seek_queries q{};
  return View<GlobalReader>(A.d, A.n_blocks, q, nullptr, 0);
}

// Listed blocks per chunk of kChunk blocks.
__global__ __launch_bounds__(kSeekTPB) void seek_fence_count_kernel(FenceArgs A) {
  __shared__ uint32_t part[kSeekTPB / kWave];
  const View<GlobalReader> V = fence_view(A);
  const uint64_t b0 = uint64_t(blockIdx.x) * kChunk + threadIdx.x * 4;
  uint32_t c = 0;
  for (uint32_t e = 0; e < 4; e++)
    if (b0 + e < A.n_blocks && listed(V, uint32_t(b0 + e))) c++;
  c = wave_sum(c);
  if (lane_id() == 0) part[wave_id()] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kSeekTPB / kWave; w++) t += part[w];
    to_glb(reinterpret_cast<uint32_t*>(A.ws + cnt_offset(A.n_blocks)))[blockIdx.x] = t;
  }
}

// The in-order compaction (as mixed_split_scatter_kernel): a chunk's base is
// the sum of the chunks before it; inside the chunk a workgroup scan.
__global__ __launch_bounds__(kSeekTPB) void seek_fence_kernel(FenceArgs A) {
  __shared__ uint32_t red[kSeekTPB / kWave], sc[2 * (kSeekTPB / kWave)];
  const View<GlobalReader> V = fence_view(A);
  const gptr<const uint32_t> cnt = to_glb(reinterpret_cast<const uint32_t*>(A.ws + cnt_offset(A.n_blocks)));
  uint32_t before = 0;
  for (uint32_t ch = threadIdx.x; ch < blockIdx.x; ch += kSeekTPB) before += cnt[ch];
  before = wave_sum(before);
  if (lane_id() == 0) red[wave_id()] = before;
  __syncthreads();
  before = 0;
  for (int w = 0; w < kSeekTPB / kWave; w++) before += red[w];

  const uint64_t b0 = uint64_t(blockIdx.x) * kChunk + threadIdx.x * 4;
  bool in[4];
  uint32_t c = 0;
  for (uint32_t e = 0; e < 4; e++) {
    in[e] = b0 + e < A.n_blocks && listed(V, uint32_t(b0 + e));
    c += in[e];
  }
  uint32_t ex, unused, tot, tot2;
  block_excl_scan2(c, 0u, &ex, &unused, sc, &tot, &tot2);
  const gptr<Fence> out = to_glb(reinterpret_cast<Fence*>(A.ws + kHdr));
  uint32_t at = before + ex;
  for (uint32_t e = 0; e < 4; e++)
    if (in[e]) {
      const Fence F = fence_of<GlobalReader>(A.comparer, V, uint32_t(b0 + e));
      out[at].w0 = F.w0;
      out[at].w1 = F.w1;
      out[at].plen = F.plen;
      out[at].block = F.block;
      out[at].kv_base = F.kv_base;
      at++;
    }
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) {
    const gptr<uint32_t> h = to_glb(reinterpret_cast<uint32_t*>(A.ws));
    h[0] = kMagic;
    h[1] = A.comparer;
    h[2] = A.n_blocks;
    h[3] = before + tot;
  }
}

template <uint32_t kCmp, bool kFilter>
__global__ __launch_bounds__(kSeekTPB) void seek_kernel(SeekArgs A) {
  const uint64_t i = uint64_t(blockIdx.x) * kSeekTPB + threadIdx.x;
  if (i >= A.q.n) return;
  uint8_t gate = 0;
  if (kFilter) {
    gate = filter_gate<GlobalReader, kCmp>(to_glb(A.filter), A.filter_len, to_glb(A.q.key_bytes),
                                           to_glb(A.q.key_off), i);
    if (gate & PBL_SEEK_FILTERED) {
      to_glb(A.out.kv)[i] = PBL_SEEK_NONE;
      if (A.out.block) to_glb(A.out.block)[i] = 0u;
      if (A.out.flags) to_glb(A.out.flags)[i] = gate;
      return;
    }
  }
  uint32_t nf = 0;
  bool stale = false;
  if (!A.q.block) {
    // the header pbl_seek_prepare wrote: another comparer's or another batch's
    // fence answers nothing
    const gptr<const uint32_t> h = to_glb(reinterpret_cast<const uint32_t*>(A.ws));
    stale = h[0] != kMagic || h[1] != kCmp || h[2] != A.n_blocks;
    nf = h[3] <= A.n_blocks ? h[3] : 0;
  }
  Landing L{PBL_SEEK_NONE, 0u, uint8_t(PBL_SEEK_BAD_BLOCK)};
  if (!stale) {
    const View<GlobalReader> V(A.d, A.n_blocks, A.q, A.ws ? reinterpret_cast<const Fence*>(A.ws + kHdr) : nullptr, nf);
    L = seek_one<GlobalReader, kCmp>(V, i);
  }
  to_glb(A.out.kv)[i] = L.kv;
  if (A.out.block) to_glb(A.out.block)[i] = L.block;
  if (A.out.flags) to_glb(A.out.flags)[i] = L.flags | gate;
}


// Argument checks shared by the device and the host entry points.
inline bool args_ok(const pbl_decode_out* d, const pbl_seek_queries* q, const pbl_seek_out* out) {
  if (!d || !q || !out) return false;
  if (q->comparer > PBL_CMP_CRDB || q->op > PBL_SEEK_LT) return false;
  if (!out->kv || !q->key_off || (q->n && !q->key_bytes)) return false;
  if (!d->blk_status || !d->blk_kv_base || !d->blk_key_base || !d->key_off || !d->key_bytes) return false;
  if (q->hide_obsolete_points && !d->kv_flags) return false;
  return true;
}
// pbl_seek_prefix_batch: table mode, SeekGE, a filter block.
inline bool prefix_args_ok(const pbl_decode_out* d, const pbl_seek_queries* q, const uint8_t* filter,
                           const pbl_seek_out* out) {
  return args_ok(d, q, out) && filter && !q->block && q->op == PBL_SEEK_GE;
}

template <bool kFilter>
int launch_seek(const pbl_decode_out* decoded, uint32_t n_blocks, const pbl_seek_queries* q, const uint8_t* filter,
                uint64_t filter_len, pbl_seek_out* out, const void* workspace, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  SeekArgs a;
  a.d = *decoded;
  a.q = *q;
  a.out = *out;
  a.n_blocks = n_blocks;
  a.ws = static_cast<const uint8_t*>(workspace);
  a.filter = filter;
  a.filter_len = filter_len;
  const uint32_t grid = uint32_t((uint64_t(q->n) + kSeekTPB - 1) / kSeekTPB);
  with_cmp(q->comparer, [&](auto c) {
    hipLaunchKernelGGL((seek_kernel<decltype(c)::value, kFilter>), dim3(grid), dim3(kSeekTPB), 0, st, a);
    return 0;
  });
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

// The host form of both entry points (filter == NULL: pbl_seek_batch_host).
inline int seek_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_seek_queries* q, const uint8_t* filter,
                     uint64_t filter_len, pbl_seek_out* out) {
  using R = cmp::HostReader;
  std::vector<Fence> fence;
  if (!q->block) {  // what pbl_seek_prepare builds, by the same two functions
    const View<R> V0(*host, n_blocks, *q, nullptr, 0);
    for (uint32_t b = 0; b < n_blocks; b++)
      if (listed(V0, b)) fence.push_back(fence_of<R>(q->comparer, V0, b));
  }
  const View<R> V(*host, n_blocks, *q, fence.data(), uint32_t(fence.size()));
  with_cmp(q->comparer, [&](auto c) {
    constexpr uint32_t kc = decltype(c)::value;
    for (uint64_t i = 0; i < q->n; i++) {
      const uint8_t gate = filter ? filter_gate<R, kc>(filter, filter_len, q->key_bytes, q->key_off, i) : uint8_t(0);
      Landing L{PBL_SEEK_NONE, 0u, gate};
      if (!(gate & PBL_SEEK_FILTERED)) {
        L = seek_one<R, kc>(V, i);
        L.flags |= gate;
      }
      out->kv[i] = L.kv;
      if (out->block) out->block[i] = L.block;
      if (out->flags) out->flags[i] = L.flags;
    }
    return 0;
  });
  return PBL_OK;
}

}  // namespace seek
}  // namespace pbl

extern "C" {

uint64_t pbl_seek_workspace_bytes(uint32_t n_blocks) { return pbl::seek::ws_size(n_blocks); }

int pbl_seek_prepare(const pbl_decode_out* decoded, uint32_t n_blocks, uint32_t comparer, void* workspace,
                     uint64_t workspace_bytes, void* stream) {
  namespace S = pbl::seek;
  if (!decoded || comparer > PBL_CMP_CRDB || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
      workspace_bytes < S::ws_size(n_blocks))
    return PBL_INVALID_ARG;
  if (!decoded->blk_status || !decoded->blk_kv_base || !decoded->blk_key_base || !decoded->key_off ||
      !decoded->key_bytes)
    return PBL_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  S::FenceArgs a;
  a.d = *decoded;
  a.n_blocks = n_blocks;
  a.comparer = comparer;
  a.ws = static_cast<uint8_t*>(workspace);
  const uint32_t grid = S::n_chunks(n_blocks);
  hipLaunchKernelGGL(S::seek_fence_count_kernel, dim3(grid), dim3(S::kSeekTPB), 0, st, a);
  hipLaunchKernelGGL(S::seek_fence_kernel, dim3(grid), dim3(S::kSeekTPB), 0, st, a);
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_seek_batch(const pbl_decode_out* decoded, uint32_t n_blocks, const pbl_seek_queries* q, pbl_seek_out* out,
                   const void* workspace, uint64_t workspace_bytes, void* stream) {
  namespace S = pbl::seek;
  if (!S::args_ok(decoded, q, out)) return PBL_INVALID_ARG;
  if (workspace && ((reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < S::ws_size(n_blocks)))
    return PBL_INVALID_ARG;
  if (!q->block && !workspace) return PBL_INVALID_ARG;
  if (q->n == 0) return PBL_OK;
  return S::launch_seek<false>(decoded, n_blocks, q, nullptr, 0, out, workspace, stream);
}

int pbl_seek_prefix_batch(const pbl_decode_out* decoded, uint32_t n_blocks, const pbl_seek_queries* q,
                          const uint8_t* filter, uint64_t filter_len, pbl_seek_out* out, const void* workspace,
                          uint64_t workspace_bytes, void* stream) {
  namespace S = pbl::seek;
  if (!S::prefix_args_ok(decoded, q, filter, out)) return PBL_INVALID_ARG;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < S::ws_size(n_blocks))
    return PBL_INVALID_ARG;
  if (q->n == 0) return PBL_OK;
  return S::launch_seek<true>(decoded, n_blocks, q, filter, filter_len, out, workspace, stream);
}

int pbl_seek_prefix_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_seek_queries* q,
                               const uint8_t* filter, uint64_t filter_len, pbl_seek_out* out) {
  namespace S = pbl::seek;
  if (!S::prefix_args_ok(host, q, filter, out)) return PBL_INVALID_ARG;
  if (q->n == 0) return PBL_OK;
  return S::seek_host(host, n_blocks, q, filter, filter_len, out);
}

int pbl_seek_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_seek_queries* q, pbl_seek_out* out) {
  namespace S = pbl::seek;
  if (!S::args_ok(host, q, out)) return PBL_INVALID_ARG;
  if (q->n == 0) return PBL_OK;
  return S::seek_host(host, n_blocks, q, nullptr, 0, out);
}

size_t pbl_seek_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_seek_queries), PBL_OFF(pbl_seek_queries, key_bytes), PBL_OFF(pbl_seek_queries, key_off),
      PBL_OFF(pbl_seek_queries, block), PBL_OFF(pbl_seek_queries, n), PBL_OFF(pbl_seek_queries, comparer),
      PBL_OFF(pbl_seek_queries, op), PBL_OFF(pbl_seek_queries, hide_obsolete_points),
      sizeof(pbl_seek_out), PBL_OFF(pbl_seek_out, kv), PBL_OFF(pbl_seek_out, block), PBL_OFF(pbl_seek_out, flags)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
