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
// seek_one<R> below is the whole search; the kernel instantiates it with
// GlobalReader and pbl_seek_batch_host with cmp::HostReader.  The comparers are
// key_cmp.hip.h's; GlobalReader specialises only the bytewise compare.
#include <algorithm>
#include <vector>

#include "common.hip.h"
#include "key_cmp.hip.h"

namespace pbl {
namespace seek {

constexpr uint32_t kMagic = 0x6b656553u;  // "Seek"
constexpr uint64_t kHdr = 64;             // u32 magic, comparer, n_blocks, n_fence; pad
constexpr uint32_t kChunk = 1024;         // blocks per compaction chunk (256 threads x 4)
constexpr int kSeekTPB = 256;
// A/B measurement, no effect on results: 0 decides every step
// of the search over blocks by the full compare against the block's last key.
#ifndef PBL_SEEK_FENCE_REGS
#define PBL_SEEK_FENCE_REGS 1
#endif

struct Fence {  // 32 B
  uint64_t w0, w1;   // first min(16, split) bytes of the last user key, big-endian, zero padded
  uint32_t plen;     // min(16, split)
  uint32_t block;
  uint64_t kv_base;  // blk_kv_base[block]
};
static_assert(sizeof(Fence) == 32, "fence record");

__host__ __device__ inline uint32_t n_chunks(uint32_t nb) { return nb ? (nb + kChunk - 1) / kChunk : 1; }
__host__ __device__ inline uint64_t cnt_offset(uint32_t nb) { return kHdr + 32ull * nb; }
__host__ __device__ inline uint64_t ws_size(uint32_t nb) {
  return (cnt_offset(nb) + 4ull * n_chunks(nb) + 15) & ~uint64_t(15);
}

// Keys through address_space(1) pointers.  bytes.Compare 16 B at a time: two
// unaligned u64 loads per side, byte-swapped so that an integer compare is the
// bytewise one, bytes past the shorter key masked off.  A chunk may start up to
// 15 bytes before a key's end: both key buffers are readable 16 B past theirs.
struct GlobalReader {
  template <class T>
  using ptr = gptr<T>;
  typedef uint64_t u64u __attribute__((aligned(1)));
  static __device__ __forceinline__ void be16(gptr<const uint8_t> p, uint64_t* w0, uint64_t* w1) {
    const gptr<const u64u> q = (gptr<const u64u>)p;
    *w0 = __builtin_bswap64(q[0]);
    *w1 = __builtin_bswap64(q[1]);
  }
  static __device__ __forceinline__ void keep(uint64_t n, uint64_t* w0, uint64_t* w1) {  // n < 16 bytes kept
    if (n < 8) {
      *w0 = n ? *w0 & (~0ull << (64 - 8 * n)) : 0;
      *w1 = 0;
    } else {
      *w1 = n > 8 ? *w1 & (~0ull << (128 - 8 * n)) : 0;
    }
  }
  static __device__ inline int bytes_cmp(gptr<const uint8_t> a, uint64_t al, gptr<const uint8_t> b, uint64_t bl) {
    const uint64_t m = al < bl ? al : bl;
    for (uint64_t o = 0; o < m; o += 16) {
      uint64_t x0, x1, y0, y1;
      be16(a + o, &x0, &x1);
      be16(b + o, &y0, &y1);
      if (m - o < 16) {
        keep(m - o, &x0, &x1);
        keep(m - o, &y0, &y1);
      }
      if (x0 != y0) return x0 < y0 ? -1 : 1;
      if (x1 != y1) return x1 < y1 ? -1 : 1;
    }
    return al < bl ? -1 : al > bl ? 1 : 0;
  }
  static __device__ inline void load_be16(gptr<const uint8_t> a, uint64_t n, uint64_t* w0, uint64_t* w1) {
    be16(a, w0, w1);
    if (n < 16) keep(n, w0, w1);
  }
};

// The arrays of a decoded batch and of the queries, through R's pointers.
template <class R>
struct View {
  template <class T>
  using P = typename R::template ptr<const T>;
  P<uint32_t> blk_status, key_off;
  P<uint64_t> blk_kv_base, blk_key_base;
  P<uint8_t> key_bytes, kv_flags;  // kv_flags: NULL unless hide
  uint32_t n_blocks;
  P<uint8_t> q_bytes;
  P<uint64_t> q_off;
  P<uint32_t> q_block;  // NULL: table mode
  uint32_t op;
  P<Fence> fence;  // table mode
  uint32_t n_fence;
  explicit PBL_HD View(const pbl_decode_out& D, uint32_t nb, const pbl_seek_queries& q, const Fence* f, uint32_t nf)
      : blk_status((P<uint32_t>)D.blk_status), key_off((P<uint32_t>)D.key_off),
        blk_kv_base((P<uint64_t>)D.blk_kv_base), blk_key_base((P<uint64_t>)D.blk_key_base),
        key_bytes((P<uint8_t>)D.key_bytes),
        kv_flags(q.hide_obsolete_points ? (P<uint8_t>)D.kv_flags : (P<uint8_t>) nullptr), n_blocks(nb),
        q_bytes((P<uint8_t>)q.key_bytes), q_off((P<uint64_t>)q.key_off), q_block((P<uint32_t>)q.block), op(q.op),
        fence((P<Fence>)f), n_fence(nf) {}
};

// One block's keys: key j = kb[ko[j] .. ko[j+1]).
template <class R>
struct Block {
  typename R::template ptr<const uint32_t> ko;
  typename R::template ptr<const uint8_t> kb;
  uint64_t kv0;
  uint32_t n;
  PBL_HD Block(const View<R>& V, uint32_t b) {
    kv0 = V.blk_kv_base[b];
    const uint64_t d = V.blk_kv_base[b + 1] - kv0;
    n = d < 0xffffffffull ? uint32_t(d) : 0u;  // (bases of an unordered or foreign batch: no KVs)
    ko = V.key_off + (kv0 + b);
    kb = V.key_bytes + V.blk_key_base[b];
  }
  PBL_HD typename R::template ptr<const uint8_t> key(uint32_t j, uint64_t* len) const {
    const uint32_t o = ko[j];
    *len = uint64_t(ko[j + 1]) - o;
    return kb + o;
  }
};

// rowblk_iter.go:606-781's search: the first KV of the block whose user key is
// >= the query under the comparer (n when there is none).
template <class R>
PBL_HD inline uint32_t lower(uint32_t cmp, const Block<R>& B, cmp::kptr<R> k, uint64_t kl) {
  uint32_t lo = 0, hi = B.n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    uint64_t ml;
    const cmp::kptr<R> mk = B.key(m, &ml);
    if (cmp::key_cmp<R>(cmp, mk, ml, k, kl) < 0) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// The fence record of block b (a PBL_OK block holding at least one KV).
template <class R>
PBL_HD inline Fence fence_of(uint32_t cmp, const View<R>& V, uint32_t b) {
  const Block<R> B(V, b);
  uint64_t kl;
  const cmp::kptr<R> k = B.key(B.n - 1, &kl);
  const uint64_t sp = cmp::key_split<R>(cmp, k, kl);
  Fence f;
  f.plen = uint32_t(sp < 16 ? sp : 16);
  R::load_be16(k, f.plen, &f.w0, &f.w1);
  f.block = b;
  f.kv_base = B.kv0;
  return f;
}
template <class R>
PBL_HD inline bool listed(const View<R>& V, uint32_t b) {
  return V.blk_status[b] == PBL_OK && V.blk_kv_base[b + 1] > V.blk_kv_base[b];
}

PBL_HD inline uint64_t first_bytes(uint64_t w, uint32_t n) {  // the first n (<= 8) bytes of a big-endian word
  return n >= 8 ? w : n ? w & (~0ull << (64 - 8 * n)) : 0;
}

struct Landing {
  uint64_t kv;
  uint32_t block;
  uint8_t flags;
};

// The whole seek of query i.  kCmp is the comparer (a template argument so that
// each kernel instantiation holds one comparer's code).
template <class R, uint32_t kCmp>
PBL_HD inline Landing seek_one(const View<R>& V, uint64_t i) {
  const uint64_t q0 = V.q_off[i];
  const uint64_t kl = V.q_off[i + 1] - q0;
  const cmp::kptr<R> k = V.q_bytes + q0;
  const bool lt = V.op == PBL_SEEK_LT;
  const bool table = !V.q_block;
  Landing L{PBL_SEEK_NONE, 0u, 0u};

  // ---- the block, and the lower bound inside it ---------------------------------
  uint32_t f = 0;  // table mode: position in the fence
  uint32_t b;
  uint32_t j;      // first KV of block b whose key is >= the query (may be B.n)
  if (table) {
    // index.SeekGE (reader_iter_single_lvl.go:788-822): the first listed block
    // whose last key is >= the query
    const uint64_t sp = cmp::key_split<R>(kCmp, k, kl);
    const uint32_t qn = uint32_t(sp < 16 ? sp : 16);
    uint64_t qw0, qw1;
    R::load_be16(k, qn, &qw0, &qw1);
    uint32_t lo = 0, hi = V.n_fence;
    while (lo < hi) {
      const uint32_t m = lo + (hi - lo) / 2;
      const Fence F{V.fence[m].w0, V.fence[m].w1, V.fence[m].plen, V.fence[m].block, 0};
      // all three comparers order by the Split-prefix bytes first: where the two
      // prefixes differ inside the bytes both records hold, that decides
      const uint32_t c = F.plen < qn ? F.plen : qn;
      const uint64_t a0 = first_bytes(F.w0, c), b0 = first_bytes(qw0, c);
      const uint64_t a1 = c > 8 ? first_bytes(F.w1, c - 8) : 0, b1 = c > 8 ? first_bytes(qw1, c - 8) : 0;
      int r;
      if (PBL_SEEK_FENCE_REGS && a0 != b0) r = a0 < b0 ? -1 : 1;
      else if (PBL_SEEK_FENCE_REGS && a1 != b1) r = a1 < b1 ? -1 : 1;
      else if (F.block >= V.n_blocks) r = 0;  // (a workspace that prepare did not write for this batch)
      else {
        const Block<R> B(V, F.block);
        if (B.n == 0) r = 0;
        else {
          uint64_t ml;
          const cmp::kptr<R> mk = B.key(B.n - 1, &ml);
          r = cmp::key_cmp<R>(kCmp, mk, ml, k, kl);
        }
      }
      if (r < 0) lo = m + 1;
      else hi = m;
    }
    f = lo;
    if (f < V.n_fence) {
      b = V.fence[f].block;
      if (b >= V.n_blocks) return L;
      j = lower<R>(kCmp, Block<R>(V, b), k, kl);
    } else {  // past the last key: SeekLT starts from the last KV, SeekGE finds nothing
      if (!lt || V.n_fence == 0) return L;
      f = V.n_fence - 1;
      b = V.fence[f].block;
      if (b >= V.n_blocks) return L;
      j = Block<R>(V, b).n;
    }
  } else {
    b = V.q_block[i];
    if (b >= V.n_blocks || V.blk_status[b] != PBL_OK) {
      L.flags = PBL_SEEK_BAD_BLOCK;
      return L;
    }
    j = lower<R>(kCmp, Block<R>(V, b), k, kl);
  }

  // ---- the first visible KV at or after (b, j), or the last one before it ---------
  // (rowblk_iter.go:1168-1179; in table mode the walk goes on into the
  // neighbouring listed blocks: skipForward / skipBackward,
  // reader_iter_single_lvl.go:1180-1260)
  Block<R> B(V, b);
  bool found = false;
  if (!lt) {
    for (;;) {
      while (j < B.n && V.kv_flags && (V.kv_flags[B.kv0 + j] & PBL_KV_OBSOLETE)) j++;
      if (j < B.n) { found = true; break; }
      if (!table || ++f >= V.n_fence) break;
      b = V.fence[f].block;
      if (b >= V.n_blocks) break;
      B = Block<R>(V, b);
      j = 0;
    }
  } else {
    for (;;) {
      while (j > 0 && V.kv_flags && (V.kv_flags[B.kv0 + j - 1] & PBL_KV_OBSOLETE)) j--;
      if (j > 0) { j--; found = true; break; }
      if (!table || f == 0) break;
      b = V.fence[--f].block;
      if (b >= V.n_blocks) break;
      B = Block<R>(V, b);
      j = B.n;
    }
  }
  if (!found) return L;
  L.kv = B.kv0 + j;
  L.block = b;
  uint64_t ll;
  const cmp::kptr<R> lk = B.key(j, &ll);
  if (!lt && cmp::key_cmp<R>(kCmp, lk, ll, k, kl) == 0) L.flags |= PBL_SEEK_EXACT;
  const uint64_t ks = cmp::key_split<R>(kCmp, k, kl), ls = cmp::key_split<R>(kCmp, lk, ll);
  if (ks == ls && R::bytes_cmp(k, ks, lk, ls) == 0) L.flags |= PBL_SEEK_SAME_PREFIX;
  return L;
}

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
};

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

template <uint32_t kCmp>
__global__ __launch_bounds__(kSeekTPB) void seek_kernel(SeekArgs A) {
  const uint64_t i = uint64_t(blockIdx.x) * kSeekTPB + threadIdx.x;
  if (i >= A.q.n) return;
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
  if (A.out.flags) to_glb(A.out.flags)[i] = L.flags;
}

template <class F>
auto with_cmp(uint32_t c, F&& f) {
  return c == PBL_CMP_TESTKEYS ? f(std::integral_constant<uint32_t, PBL_CMP_TESTKEYS>{})
         : c == PBL_CMP_CRDB   ? f(std::integral_constant<uint32_t, PBL_CMP_CRDB>{})
                               : f(std::integral_constant<uint32_t, PBL_CMP_DEFAULT>{});
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
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  S::SeekArgs a;
  a.d = *decoded;
  a.q = *q;
  a.out = *out;
  a.n_blocks = n_blocks;
  a.ws = static_cast<const uint8_t*>(workspace);
  const uint32_t grid = uint32_t((uint64_t(q->n) + S::kSeekTPB - 1) / S::kSeekTPB);
  S::with_cmp(q->comparer, [&](auto c) {
    hipLaunchKernelGGL(S::seek_kernel<decltype(c)::value>, dim3(grid), dim3(S::kSeekTPB), 0, st, a);
    return 0;
  });
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_seek_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_seek_queries* q, pbl_seek_out* out) {
  namespace S = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!S::args_ok(host, q, out)) return PBL_INVALID_ARG;
  if (q->n == 0) return PBL_OK;
  std::vector<S::Fence> fence;
  if (!q->block) {  // what pbl_seek_prepare builds, by the same two functions
    const S::View<R> V0(*host, n_blocks, *q, nullptr, 0);
    for (uint32_t b = 0; b < n_blocks; b++)
      if (S::listed(V0, b)) fence.push_back(S::fence_of<R>(q->comparer, V0, b));
  }
  const S::View<R> V(*host, n_blocks, *q, fence.data(), uint32_t(fence.size()));
  S::with_cmp(q->comparer, [&](auto c) {
    for (uint64_t i = 0; i < q->n; i++) {
      const S::Landing L = S::seek_one<R, decltype(c)::value>(V, i);
      out->kv[i] = L.kv;
      if (out->block) out->block[i] = L.block;
      if (out->flags) out->flags[i] = L.flags;
    }
    return 0;
  });
  return PBL_OK;
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
