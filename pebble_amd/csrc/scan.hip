// scan.hip — batched bounded scans over a decoded batch, on the device
// (DESIGN.md §3.10): for query i with bounds [lower_i, upper_i) the KVs that
// singleLevelIterator returns for SetBounds(lower, upper); First(); Next()...
// (sstable/reader_iter_single_lvl.go:443-473, :1367-1390, :1573-1647; skipForward
// :1765-1840), compacted and copied inside HBM into a result that has the layout
// of a decoded batch with one "block" per query (include/pebble_amd.h).
//
//   scan_tile_kernel / scan_tile_scan_kernel  (pbl_scan_prepare, after the seek
//       fence) the visible prefix: per aligned tile of 256 source KVs the
//       exclusive prefix of {visible KVs, their key bytes, their value bytes}
//       and the tile's first block
//   scan_bounds_kernel<comparer>  lane per query: two lower-bound searches
//       (bounds_one, over seek_core.hip.h's fence_lower / lower) give [kv_lo,
//       kv_hi) in global KV index space; the visible prefix at both ends (a
//       tile prefix plus a partial tile) gives the query's sizes
//   scan_sum_kernel / scan_bases_kernel  the exclusive scan over queries
//       (result_core.hip.h's chunk_sums / bases, with the tiles per query as a
//       fourth component): the result's bases, statuses, totals, the capacity
//       check
//   scan_emit_kernel  work item = (query, source tile), one wave each, a
//       persistent grid striding over items whose number only the device knows;
//       an item finds its query by binary search in the scanned tiles-per-query
//       array.  Per-KV arrays lane per KV (output rank by ballot / popcount),
//       keys lane per KV in 16-B chunks, values by result_core.hip.h's
//       copy_values.
//
// The tile scan, every query's last offset and the per-KV arrays are
// result_core.hip.h's too.
//
// bounds_one<R> is the whole bounds search; the kernel instantiates it with
// GlobalReader and pbl_scan_batch_host with cmp::HostReader.
#include <algorithm>
#include <vector>

#include "result_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace scan {

constexpr uint32_t kMagic = 0x6e616353u;  // "Scan"
constexpr uint64_t kHdr = 64;
constexpr uint32_t kTileShift = 8, kTile = 1u << kTileShift;  // source KVs per tile
constexpr int kScanTPB = 256;
constexpr uint32_t kChunk = 256;      // queries per chunk of the scan over queries
static_assert(kScanTPB == result::kTPB && kChunk == uint32_t(result::kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kEmitGrid = 2048;  // workgroups of the persistent emit grid, at most
constexpr uint64_t kMaxBytes = 0xffffffffull;  // a query's key / value bytes (u32 offsets)
// header words (u32): magic, comparer, n_blocks, hide, overflow (per call); u64
// at byte 24: the n_kv the workspace was prepared for
enum { kHMagic = 0, kHCmp = 1, kHBlocks = 2, kHHide = 3, kHOverflow = 4 };
// per-query u64 arrays, n + 1 entries each
enum { kQLo = 0, kQHi, kQPlo0, kQPlo1, kQPlo2, kQKv, kQKey, kQVal, kQTiles, kQTBase, kQArrays };

struct Layout {
  uint64_t nt;                                    // tiles (n_kv / 256 + 1: the last holds the totals)
  uint64_t fence, pfx, tblk, q64, qblo, qst, csum, size;
  uint32_t n_chunks;
};
__host__ __device__ inline Layout layout(uint32_t nq, uint32_t nb, uint64_t n_kv) {
  Layout L;
  L.nt = (n_kv >> kTileShift) + 1;
  L.n_chunks = nq ? (nq + kChunk - 1) / kChunk : 1;
  uint64_t o = kHdr;
  L.fence = o; o += seek::ws_size(nb);
  L.pfx = o;   o += 3 * 8 * L.nt;
  L.tblk = o;  o += (4 * L.nt + 15) & ~uint64_t(15);
  L.q64 = o;   o += uint64_t(kQArrays) * 8 * (uint64_t(nq) + 1);
  L.csum = o;  o += 4ull * 8 * L.n_chunks;
  L.qblo = o;  o += 4ull * nq;
  L.qst = o;   o += 4ull * nq;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

// The queries through R's pointers.
template <class R>
struct QView {
  template <class T>
  using P = typename R::template ptr<const T>;
  P<uint8_t> lo_bytes, hi_bytes, flags;
  P<uint64_t> lo_off, hi_off;
  P<uint32_t> block;
  explicit PBL_HD QView(const pbl_scan_queries& q)
      : lo_bytes((P<uint8_t>)q.lower_bytes), hi_bytes((P<uint8_t>)q.upper_bytes), flags((P<uint8_t>)q.flags),
        lo_off((P<uint64_t>)q.lower_off), hi_off((P<uint64_t>)q.upper_off), block((P<uint32_t>)q.block) {}
};

struct Bounds {
  uint64_t lo, hi;  // source KV index range, before hiding
  uint32_t status;
};

// The first KV of the whole batch, in global KV index space, whose user key is
// >= k (index.SeekGE, then data.SeekGE: reader_iter_single_lvl.go:788-850);
// `total` when there is none.
template <class R, uint32_t kCmp>
PBL_HD inline uint64_t table_lower(const seek::View<R>& V, cmp::kptr<R> k, uint64_t kl, uint64_t total) {
  const uint32_t f = seek::fence_lower<R, kCmp>(V, k, kl);
  if (f >= V.n_fence) return total;
  const uint32_t b = V.fence[f].block;
  if (b >= V.n_blocks) return total;
  const seek::Block<R> B(V, b);
  return B.kv0 + seek::lower<R>(kCmp, B, k, kl);
}

// The whole bounds search of query i: SetBounds(lower, upper) and First()
// (reader_iter_single_lvl.go:443-473, :1367-1390).
template <class R, uint32_t kCmp>
PBL_HD inline Bounds bounds_one(const seek::View<R>& V, const QView<R>& Q, uint64_t i, uint64_t total) {
  const uint64_t l0 = Q.lo_off[i], ll = Q.lo_off[i + 1] - l0;
  const uint64_t u0 = Q.hi_off[i], ul = Q.hi_off[i + 1] - u0;
  const cmp::kptr<R> lk = Q.lo_bytes + l0, uk = Q.hi_bytes + u0;
  const bool no_upper = Q.flags && (Q.flags[i] & PBL_SCAN_NO_UPPER);
  Bounds r{0, 0, PBL_OK};
  if (!Q.block) {
    r.lo = ll ? table_lower<R, kCmp>(V, lk, ll, total) : 0;
    r.hi = no_upper ? total : table_lower<R, kCmp>(V, uk, ul, total);
  } else {
    const uint32_t b = Q.block[i];
    if (b >= V.n_blocks) {
      r.status = PBL_INVALID_ARG;
      return r;
    }
    if (V.blk_status[b] != PBL_OK) {
      r.status = V.blk_status[b];
      return r;
    }
    const seek::Block<R> B(V, b);
    r.lo = B.kv0 + (ll ? seek::lower<R>(kCmp, B, lk, ll) : 0u);
    r.hi = B.kv0 + (no_upper ? B.n : seek::lower<R>(kCmp, B, uk, ul));
  }
  if (r.lo > total) r.lo = total;  // (bases of an unordered or foreign batch)
  if (r.hi > total) r.hi = total;
  if (r.hi < r.lo) r.hi = r.lo;    // upper <= lower
  return r;
}

// ---- device side ---------------------------------------------------------------
struct ScanArgs {
  pbl_decode_out d;
  pbl_scan_queries q;
  pbl_scan_out out;
  uint32_t n_blocks, comparer, hide, size_only;
  uint64_t n_kv;
  uint8_t* ws;
};

// The workspace's arrays.
struct Ws {
  gptr<uint32_t> hdr;
  gptr<uint64_t> pfx[3];
  gptr<uint32_t> tblk;
  gptr<uint64_t> q64, csum;
  gptr<uint32_t> qblo, qst;
  uint64_t nt, qs;  // tiles; stride of the per-query u64 arrays
  uint32_t n_chunks;
  __device__ Ws(uint8_t* ws, uint32_t nq, uint32_t nb, uint64_t n_kv) {
    const Layout L = layout(nq, nb, n_kv);
    hdr = to_glb(reinterpret_cast<uint32_t*>(ws));
    for (int c = 0; c < 3; c++) pfx[c] = to_glb(reinterpret_cast<uint64_t*>(ws + L.pfx)) + uint64_t(c) * L.nt;
    tblk = to_glb(reinterpret_cast<uint32_t*>(ws + L.tblk));
    q64 = to_glb(reinterpret_cast<uint64_t*>(ws + L.q64));
    csum = to_glb(reinterpret_cast<uint64_t*>(ws + L.csum));
    qblo = to_glb(reinterpret_cast<uint32_t*>(ws + L.qblo));
    qst = to_glb(reinterpret_cast<uint32_t*>(ws + L.qst));
    nt = L.nt;
    qs = uint64_t(nq) + 1;
    n_chunks = L.n_chunks;
  }
  __device__ gptr<uint64_t> q(int a) const { return q64 + uint64_t(a) * qs; }
  // the four scanned components: kQKv, kQKey, kQVal, kQTiles
  __device__ result::Sizes sizes() const { return result::Sizes{q(kQKv), csum, qst, qs, n_chunks}; }
  __device__ uint64_t prepared_kv() const { return *(gptr<const uint64_t>)(hdr + 6); }
};

// The source KVs the kernels may touch: what the batch holds, never more than
// the workspace was sized for.
__device__ inline uint64_t source_total(const pbl_decode_out& D, uint32_t nb, uint64_t n_kv) {
  const uint64_t t = nb ? to_glb(D.blk_kv_base)[nb] : 0;
  return t < n_kv ? t : n_kv;
}

using result::block_of;
using result::block_sum64;

// One source KV as the scan sees it.
struct Kv {
  bool vis;
  uint32_t klen, vlen;
  uint64_t ksrc, vsrc;  // positions in key_bytes / val_bytes
};
__device__ __forceinline__ Kv kv_view(const pbl_decode_out& D, bool hide, uint64_t kv, uint32_t b) {
  Kv r{false, 0u, 0u, 0ull, 0ull};
  if (to_glb(D.blk_status)[b] != PBL_OK) return r;
  if (hide && (to_glb(D.kv_flags)[kv] & PBL_KV_OBSOLETE)) return r;
  const uint32_t k0 = to_glb(D.key_off)[kv + b], k1 = to_glb(D.key_off)[kv + b + 1];
  const uint32_t v0 = to_glb(D.val_off)[kv + b], v1 = to_glb(D.val_off)[kv + b + 1];
  r.vis = true;
  r.klen = k1 - k0;
  r.vlen = v1 - v0;
  r.ksrc = to_glb(D.blk_key_base)[b] + k0;
  r.vsrc = to_glb(D.blk_val_base)[b] + v0;
  return r;
}

// Per tile: its visible KVs, key bytes and value bytes (scanned in place by
// scan_tile_scan_kernel) and the block of its first KV (n_blocks: no KV).
__global__ __launch_bounds__(kScanTPB) void scan_tile_kernel(ScanArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, 0, A.n_blocks, A.n_kv);
  const uint64_t total = source_total(A.d, A.n_blocks, A.n_kv);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t kv = (t << kTileShift) + threadIdx.x;
    uint32_t b = A.n_blocks;
    Kv v{false, 0u, 0u, 0ull, 0ull};
    if (kv < total) {
      b = block_of(to_glb(A.d.blk_kv_base), A.n_blocks, kv);
      v = kv_view(A.d, A.hide != 0, kv, b);
    }
    const uint64_t n = block_sum64(v.vis ? 1u : 0u, lds), k = block_sum64(v.klen, lds), x = block_sum64(v.vlen, lds);
    if (threadIdx.x == 0) {
      W.pfx[0][t] = n;
      W.pfx[1][t] = k;
      W.pfx[2][t] = x;
      W.tblk[t] = b;
    }
  }
}

// One workgroup: the exclusive scan over tiles, in place, and the header.
__global__ __launch_bounds__(kScanTPB) void scan_tile_scan_kernel(ScanArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, 0, A.n_blocks, A.n_kv);
  result::tile_scan_inplace(W.pfx, W.nt, lds);
  if (threadIdx.x == 0) {
    // a batch that holds more KVs than the workspace was sized for is not
    // described by it: no header, and every query reports it
    const uint64_t held = A.n_blocks ? to_glb(A.d.blk_kv_base)[A.n_blocks] : 0;
    W.hdr[kHMagic] = held <= A.n_kv ? kMagic : 0u;
    W.hdr[kHCmp] = A.comparer;
    W.hdr[kHBlocks] = A.n_blocks;
    W.hdr[kHHide] = A.hide;
    W.hdr[kHOverflow] = 0;
    *(gptr<uint64_t>)(W.hdr + 6) = A.n_kv;
  }
}

// p += the visible KVs of [x0, x1) and their bytes; *blk: the block x0 lies in
// on entry, the block x1 lies in on return.
__device__ inline void walk(const ScanArgs& A, uint64_t x0, uint64_t x1, uint32_t* blk, uint64_t p[3]) {
  const gptr<const uint64_t> base = to_glb(A.d.blk_kv_base);
  const uint32_t nb = A.n_blocks;
  uint32_t b = *blk;
  uint64_t next = b + 1 < nb ? base[b + 1] : ~0ull;  // the first KV index past block b
  for (uint64_t x = x0; x <= x1; x++) {
    while (x >= next) {
      b++;
      next = b + 1 < nb ? base[b + 1] : ~0ull;
    }
    if (x == x1) break;
    const Kv v = kv_view(A.d, A.hide != 0, x, b);
    p[0] += v.vis ? 1u : 0u;
    p[1] += v.klen;
    p[2] += v.vlen;
  }
  *blk = b;
}

// The visible prefix at a tile's start, and the block of its first KV.
__device__ inline void tile_start(const Ws& W, uint32_t nb, uint64_t t, uint64_t p[3], uint32_t* blk) {
  p[0] = W.pfx[0][t];
  p[1] = W.pfx[1][t];
  p[2] = W.pfx[2][t];
  const uint32_t b = W.tblk[t];
  *blk = b < nb ? b : nb - 1;
}

// p and *blk hold the visible prefix at x0 and x0's block, x0 <= kv in kv's tile
// (its start, or a bound before kv); on return those of kv (<= total).
__device__ inline void prefix_to(const ScanArgs& A, const Ws& W, uint64_t x0, uint64_t kv, uint64_t p[3],
                                 uint32_t* blk) {
  const uint64_t t = kv >> kTileShift;
  const uint32_t nb = A.n_blocks, b = *blk;
  if (t + 1 < W.nt && W.pfx[0][t + 1] - W.pfx[0][t] == kTile) {
    // every KV of the tile is visible, so its keys and values are contiguous
    // (their blocks are PBL_OK): the sizes of [x0, kv) are two offset reads
    const gptr<const uint64_t> base = to_glb(A.d.blk_kv_base);
    uint32_t l = b, h = W.tblk[t + 1] < nb ? W.tblk[t + 1] : nb - 1;
    while (l < h) {
      const uint32_t m = l + (h - l + 1) / 2;
      if (base[m] <= kv) l = m;
      else h = m - 1;
    }
    p[0] += kv - x0;
    p[1] += (to_glb(A.d.blk_key_base)[l] + to_glb(A.d.key_off)[kv + l]) -
            (to_glb(A.d.blk_key_base)[b] + to_glb(A.d.key_off)[x0 + b]);
    p[2] += (to_glb(A.d.blk_val_base)[l] + to_glb(A.d.val_off)[kv + l]) -
            (to_glb(A.d.blk_val_base)[b] + to_glb(A.d.val_off)[x0 + b]);
    *blk = l;
    return;
  }
  walk(A, x0, kv, blk, p);
}

template <uint32_t kCmp>
__global__ __launch_bounds__(kScanTPB) void scan_bounds_kernel(ScanArgs A) {
  const uint64_t i = uint64_t(blockIdx.x) * kScanTPB + threadIdx.x;
  if (i >= A.q.n) return;
  const Ws W(A.ws, A.q.n, A.n_blocks, A.n_kv);
  // the header pbl_scan_prepare wrote: another batch's, hide flag's or (table
  // mode) comparer's workspace answers nothing
  const bool stale = W.hdr[kHMagic] != kMagic || W.hdr[kHBlocks] != A.n_blocks || W.hdr[kHHide] != A.hide ||
                     W.prepared_kv() != A.n_kv || (!A.q.block && W.hdr[kHCmp] != kCmp) || A.n_blocks == 0;
  Bounds B{0, 0, A.n_blocks == 0 && W.hdr[kHMagic] == kMagic ? uint32_t(PBL_OK) : uint32_t(PBL_INVALID_ARG)};
  uint64_t plo[3] = {0, 0, 0}, phi[3] = {0, 0, 0};
  uint32_t blo = 0;
  if (!stale) {
    const uint8_t* fw = A.ws + layout(A.q.n, A.n_blocks, A.n_kv).fence;
    const gptr<const uint32_t> fh = to_glb(reinterpret_cast<const uint32_t*>(fw));
    const uint32_t nf = fh[3] <= A.n_blocks ? fh[3] : 0;
    pbl_seek_queries sq{};
    sq.hide_obsolete_points = 0;  // the bounds are positions before hiding
    const seek::View<seek::GlobalReader> V(A.d, A.n_blocks, sq, reinterpret_cast<const seek::Fence*>(fw + seek::kHdr),
                                           nf);
    const QView<seek::GlobalReader> Q(A.q);
    B = bounds_one<seek::GlobalReader, kCmp>(V, Q, i, source_total(A.d, A.n_blocks, A.n_kv));
    if (B.status == PBL_OK && B.hi > B.lo) {
      uint32_t bhi;
      tile_start(W, A.n_blocks, B.lo >> kTileShift, plo, &blo);
      prefix_to(A, W, (B.lo >> kTileShift) << kTileShift, B.lo, plo, &blo);
      // the upper end: on from kv_lo when both lie in one tile, else from its tile's start
      uint64_t x0 = B.lo;
      phi[0] = plo[0];
      phi[1] = plo[1];
      phi[2] = plo[2];
      bhi = blo;
      if ((B.hi >> kTileShift) != (B.lo >> kTileShift)) {
        x0 = (B.hi >> kTileShift) << kTileShift;
        tile_start(W, A.n_blocks, B.hi >> kTileShift, phi, &bhi);
      }
      prefix_to(A, W, x0, B.hi, phi, &bhi);
      if (phi[1] - plo[1] > kMaxBytes || phi[2] - plo[2] > kMaxBytes) B.status = PBL_UNSUPPORTED;
    }
  }
  const bool some = B.status == PBL_OK && B.hi > B.lo;
  W.q(kQLo)[i] = B.lo;
  W.q(kQHi)[i] = B.hi;
  W.q(kQPlo0)[i] = plo[0];
  W.q(kQPlo1)[i] = plo[1];
  W.q(kQPlo2)[i] = plo[2];
  W.q(kQKv)[i] = some ? phi[0] - plo[0] : 0;
  W.q(kQKey)[i] = some ? phi[1] - plo[1] : 0;
  W.q(kQVal)[i] = some ? phi[2] - plo[2] : 0;
  W.q(kQTiles)[i] = some ? ((B.hi - 1) >> kTileShift) - (B.lo >> kTileShift) + 1 : 0;
  W.qblo[i] = blo;
  W.qst[i] = B.status;
}

// Per chunk of kChunk queries: the sums of {KVs, key bytes, value bytes, tiles}.
__global__ __launch_bounds__(kScanTPB) void scan_sum_kernel(ScanArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.q.n, A.n_blocks, A.n_kv);
  result::chunk_sums<4>(W.sizes(), A.q.n, lds);
}

// The result's bases, statuses and totals; the tiles-per-query scan; the
// capacity check (the last chunk).  Totals were zeroed by the entry point.
__global__ __launch_bounds__(kScanTPB) void scan_bases_kernel(ScanArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.q.n, A.n_blocks, A.n_kv);
  const uint32_t n = A.q.n;
  const uint64_t i = uint64_t(blockIdx.x) * kChunk + threadIdx.x;
  uint64_t ex[4], end[4];
  bool over;
  const bool last = result::bases<4>(W.sizes(), A.out.result, n, A.size_only != 0, lds, ex, end, &over);
  if (i < n) {
    W.q(kQTBase)[i] = ex[3];
    if (A.out.range) {
      to_glb(A.out.range)[2 * i] = W.q(kQLo)[i];
      to_glb(A.out.range)[2 * i + 1] = W.q(kQHi)[i];
    }
  }
  if (last) {
    W.q(kQTBase)[n] = end[3];
    W.hdr[kHOverflow] = over ? 1u : 0u;
  }
}

#ifndef PBL_SCAN_EMIT_WAVES
#define PBL_SCAN_EMIT_WAVES 5  // as tf_scatter_kernel (transforms.hip): the same copy loops
#endif
__global__ void __launch_bounds__(kScanTPB) __attribute__((amdgpu_waves_per_eu(PBL_SCAN_EMIT_WAVES)))
scan_emit_kernel(ScanArgs A) {
  const Ws W(A.ws, A.q.n, A.n_blocks, A.n_kv);
  if (W.hdr[kHOverflow] != 0) return;  // sizes only
  const pbl_decode_out& I = A.d;
  const pbl_decode_out& O = A.out.result;
  const uint32_t n = A.q.n, nb = A.n_blocks;
  const uint32_t lane = lane_id();
  const bool hide = A.hide != 0;
  const gptr<const uint64_t> okvb = to_glb(O.blk_kv_base), okeyb = to_glb(O.blk_key_base), ovalb = to_glb(O.blk_val_base);
  result::last_offsets(O, n, ~0ull);  // (an empty query's only offset)
  const gptr<const uint64_t> tbase = W.q(kQTBase), base = to_glb(I.blk_kv_base);
  const uint64_t n_items = tbase[n];
  const uint32_t wpb = kScanTPB / kWave;
  for (uint64_t item = uint64_t(blockIdx.x) * wpb + wave_id(); item < n_items; item += uint64_t(gridDim.x) * wpb) {
    // the query of the item: the last q with tbase[q] <= item
    uint32_t q;
    {
      uint32_t lo = 0, hi = n;
      while (lo < hi) {
        const uint32_t m = lo + (hi - lo) / 2;
        if (tbase[m] <= item) lo = m + 1;
        else hi = m;
      }
      q = lo - 1;
    }
    const uint64_t lo_kv = W.q(kQLo)[q], hi_kv = W.q(kQHi)[q];
    const uint64_t t = (lo_kv >> kTileShift) + (item - tbase[q]);  // source tile
    const bool first = (t << kTileShift) <= lo_kv;
    const uint64_t s = first ? lo_kv : t << kTileShift;
    const uint64_t e = hi_kv < ((t + 1) << kTileShift) ? hi_kv : (t + 1) << kTileShift;
    // the query-relative output position of s: a difference of visible prefixes
    const uint64_t p0 = W.q(kQPlo0)[q], p1 = W.q(kQPlo1)[q], p2 = W.q(kQPlo2)[q];
    uint32_t jo = first ? 0u : uint32_t(W.pfx[0][t] - p0);
    uint32_t kcur = first ? 0u : uint32_t(W.pfx[1][t] - p1);
    uint32_t vcur = first ? 0u : uint32_t(W.pfx[2][t] - p2);
    // the blocks the tile's KVs lie in
    const uint32_t b_s = first ? W.qblo[q] : W.tblk[t];
    uint32_t b_e = t + 1 < W.nt ? W.tblk[t + 1] : nb - 1;
    if (b_e >= nb) b_e = nb - 1;
    const uint64_t okv = okvb[q], okb = okeyb[q], ovb = ovalb[q];
    for (uint64_t j0 = s; j0 < e; j0 += kWave) {
      const uint64_t kv = j0 + lane;
      Kv v{false, 0u, 0u, 0ull, 0ull};
      if (kv < e) {
        uint32_t l = b_s, h = b_e;  // the last block of [b_s, b_e] whose base is <= kv
        while (l < h) {
          const uint32_t m = l + (h - l + 1) / 2;
          if (base[m] <= kv) l = m;
          else h = m - 1;
        }
        v = kv_view(I, hide, kv, l);
      }
      const bool vis = v.vis;
      const uint64_t vm = __ballot(vis);
      const uint32_t rank = __builtin_popcountll(vm & ((1ull << lane) - 1));
      const uint32_t kx = wave_incl_scan(v.klen), vx = wave_incl_scan(v.vlen);
      const uint32_t ko = kcur + kx - v.klen, vo = vcur + vx - v.vlen;
      if (vis) {
        const uint64_t k = okv + jo + rank;
        result::copy_kv_arrays(O, k, I, kv, 0xff, false);
        if (A.out.src_kv) to_glb(A.out.src_kv)[k] = kv;
        to_glb(O.key_off)[k + q] = ko;
        to_glb(O.val_off)[k + q] = vo;
        copy_chunks(to_glb(O.key_bytes) + okb + ko, to_glb(I.key_bytes) + v.ksrc, v.klen);
      }
      result::copy_values(vis, v.vlen, to_glb((const uint8_t*)I.val_bytes) + v.vsrc, to_glb(O.val_bytes) + (ovb + vo));
      jo += __builtin_popcountll(vm);
      kcur += uint32_t(__shfl(int(kx), kWave - 1, kWave));
      vcur += uint32_t(__shfl(int(vx), kWave - 1, kWave));
    }
  }
}

// ---- host side -----------------------------------------------------------------
// Argument checks shared by the device and the host entry points.
inline bool args_ok(const pbl_decode_out* d, const pbl_scan_queries* q, const pbl_scan_out* out, bool size_only) {
  if (!result::source_ok(d) || !q || !out) return false;
  if (q->comparer > PBL_CMP_CRDB) return false;
  if (!q->lower_off || !q->upper_off || (q->n && (!q->lower_bytes || !q->upper_bytes))) return false;
  if (q->hide_obsolete_points && !d->kv_flags) return false;
  return result::result_ok(out->result, size_only);
}
inline bool ws_ok(const void* ws, uint64_t bytes, uint32_t nq, uint32_t nb, uint64_t n_kv) {
  return result::ws_aligned(ws) && bytes >= layout(nq, nb, n_kv).size;
}

inline int launch(const pbl_decode_out* d, uint32_t nb, uint64_t n_kv, const pbl_scan_queries* q, pbl_scan_out* out, void* ws,
           uint64_t ws_bytes, bool size_only, bool sized, hipStream_t st) {
  if (!args_ok(d, q, out, size_only) || !ws_ok(ws, ws_bytes, q->n, nb, n_kv)) return PBL_INVALID_ARG;
  ScanArgs a{};
  a.d = *d;
  a.q = *q;
  a.out = *out;
  a.n_blocks = nb;
  a.comparer = q->comparer;
  a.hide = q->hide_obsolete_points ? 1u : 0u;
  a.size_only = size_only ? 1u : 0u;
  a.n_kv = n_kv;
  a.ws = static_cast<uint8_t*>(ws);
  if (hipMemsetAsync(out->result.totals, 0, sizeof(pbl_totals), st) != hipSuccess) return PBL_DEVICE_ERROR;
  const Layout L = layout(q->n, nb, n_kv);
  if (q->n && !sized) {
    const uint32_t grid = uint32_t((uint64_t(q->n) + kScanTPB - 1) / kScanTPB);
    seek::with_cmp(q->comparer, [&](auto c) {
      hipLaunchKernelGGL(scan_bounds_kernel<decltype(c)::value>, dim3(grid), dim3(kScanTPB), 0, st, a);
      return 0;
    });
  }
  if (q->n) hipLaunchKernelGGL(scan_sum_kernel, dim3(L.n_chunks), dim3(kScanTPB), 0, st, a);
  hipLaunchKernelGGL(scan_bases_kernel, dim3(L.n_chunks), dim3(kScanTPB), 0, st, a);
  if (!size_only && q->n && out->result.key_off) {
    // items <= queries x tiles, four per workgroup; the grid also covers the queries once
    const uint64_t items = uint64_t(q->n) * L.nt;
    const uint64_t need = std::max<uint64_t>((items + 3) / 4, (uint64_t(q->n) + kScanTPB - 1) / kScanTPB);
    const uint32_t grid = uint32_t(std::min<uint64_t>(need, kEmitGrid));
    hipLaunchKernelGGL(scan_emit_kernel, dim3(grid), dim3(kScanTPB), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

}  // namespace scan
}  // namespace pbl

extern "C" {

uint64_t pbl_scan_workspace_bytes(uint32_t n_queries, uint32_t n_blocks, uint64_t n_kv) {
  return pbl::scan::layout(n_queries, n_blocks, n_kv).size;
}

int pbl_scan_prepare(const pbl_decode_out* decoded, uint32_t n_blocks, uint64_t n_kv, uint32_t comparer,
                     uint32_t hide_obsolete_points, void* workspace, uint64_t workspace_bytes, void* stream) {
  namespace S = pbl::scan;
  if (!pbl::result::source_ok(decoded) || comparer > PBL_CMP_CRDB || (hide_obsolete_points && !decoded->kv_flags) ||
      !S::ws_ok(workspace, workspace_bytes, 0, n_blocks, n_kv))
    return PBL_INVALID_ARG;
  const S::Layout L = S::layout(0, n_blocks, n_kv);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const int rc = pbl_seek_prepare(decoded, n_blocks, comparer, ws + L.fence, pbl::seek::ws_size(n_blocks), stream);
  if (rc != PBL_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  S::ScanArgs a{};
  a.d = *decoded;
  a.n_blocks = n_blocks;
  a.comparer = comparer;
  a.hide = hide_obsolete_points ? 1u : 0u;
  a.n_kv = n_kv;
  a.ws = ws;
  const uint32_t grid = uint32_t(std::min<uint64_t>(L.nt, 1u << 20));
  hipLaunchKernelGGL(S::scan_tile_kernel, dim3(grid), dim3(S::kScanTPB), 0, st, a);
  hipLaunchKernelGGL(S::scan_tile_scan_kernel, dim3(1), dim3(S::kScanTPB), 0, st, a);
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_scan_size(const pbl_decode_out* decoded, uint32_t n_blocks, uint64_t n_kv, const pbl_scan_queries* q,
                  pbl_scan_out* out, void* workspace, uint64_t workspace_bytes, void* stream) {
  return pbl::scan::launch(decoded, n_blocks, n_kv, q, out, workspace, workspace_bytes, true, false,
                           reinterpret_cast<hipStream_t>(stream));
}

int pbl_scan_batch(const pbl_decode_out* decoded, uint32_t n_blocks, uint64_t n_kv, const pbl_scan_queries* q,
                   pbl_scan_out* out, void* workspace, uint64_t workspace_bytes, uint32_t flags, void* stream) {
  if (flags & ~uint32_t(PBL_SCAN_SIZED)) return PBL_INVALID_ARG;
  return pbl::scan::launch(decoded, n_blocks, n_kv, q, out, workspace, workspace_bytes, false,
                           (flags & PBL_SCAN_SIZED) != 0, reinterpret_cast<hipStream_t>(stream));
}

int pbl_scan_batch_host(const pbl_decode_out* host, uint32_t n_blocks, const pbl_scan_queries* q, pbl_scan_out* out) {
  namespace S = pbl::scan;
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!S::args_ok(host, q, out, false)) return PBL_INVALID_ARG;
  const pbl_decode_out& D = *host;
  const pbl_decode_out& O = out->result;
  const uint32_t n = q->n;
  const uint64_t total = n_blocks ? D.blk_kv_base[n_blocks] : 0;
  const bool hide = q->hide_obsolete_points != 0;
  pbl_seek_queries sq{};
  std::vector<K::Fence> fence;
  if (!q->block) {  // what pbl_scan_prepare builds, by pbl_seek_prepare's two functions
    const K::View<R> V0(D, n_blocks, sq, nullptr, 0);
    for (uint32_t b = 0; b < n_blocks; b++)
      if (K::listed(V0, b)) fence.push_back(K::fence_of<R>(q->comparer, V0, b));
  }
  const K::View<R> V(D, n_blocks, sq, fence.data(), uint32_t(fence.size()));
  const S::QView<R> Q(*q);
  std::vector<S::Bounds> bounds(n);
  K::with_cmp(q->comparer, [&](auto c) {
    for (uint64_t i = 0; i < n; i++) {
      if (n_blocks == 0) bounds[i] = S::Bounds{0, 0, PBL_OK};
      else bounds[i] = S::bounds_one<R, decltype(c)::value>(V, Q, i, total);
    }
    return 0;
  });
  // a plain walk over [lo, hi): sizes first, then (when they fit) the gather
  auto walk = [&](const S::Bounds& B, auto&& f) {
    uint32_t b = 0;
    for (uint64_t kv = B.lo; kv < B.hi; kv++) {
      while (b + 1 < n_blocks && kv >= D.blk_kv_base[b + 1]) b++;
      if (D.blk_status[b] != PBL_OK || (hide && (D.kv_flags[kv] & PBL_KV_OBSOLETE))) continue;
      f(kv, b);
    }
  };
  pbl_totals T{};
  uint64_t kvb = 0, keyb = 0, valb = 0;
  for (uint32_t i = 0; i < n; i++) {
    S::Bounds& B = bounds[i];
    uint64_t nk = 0, kb = 0, vb = 0;
    if (B.status == PBL_OK) {
      walk(B, [&](uint64_t kv, uint32_t b) {
        nk++;
        kb += D.key_off[kv + b + 1] - D.key_off[kv + b];
        vb += D.val_off[kv + b + 1] - D.val_off[kv + b];
      });
      if (kb > S::kMaxBytes || vb > S::kMaxBytes) {
        B.status = PBL_UNSUPPORTED;
        nk = kb = vb = 0;
      }
    }
    O.blk_kv_base[i] = kvb;
    O.blk_key_base[i] = keyb;
    O.blk_val_base[i] = valb;
    if (O.blk_rst_base) O.blk_rst_base[i] = 0;
    O.blk_status[i] = B.status;
    if (B.status != PBL_OK) {
      T.status_mask |= 1u << B.status;
      T.n_bad_blocks++;
    }
    if (out->range) {
      out->range[2 * i] = B.lo;
      out->range[2 * i + 1] = B.hi;
    }
    kvb += nk;
    keyb += kb;
    valb += vb;
  }
  O.blk_kv_base[n] = kvb;
  O.blk_key_base[n] = keyb;
  O.blk_val_base[n] = valb;
  if (O.blk_rst_base) O.blk_rst_base[n] = 0;
  T.n_kv = kvb;
  T.key_bytes = keyb;
  T.val_bytes = valb;
  const bool over = kvb > O.kv_cap || keyb > O.key_cap || valb > O.val_cap;
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *O.totals = T;
  if (over || !O.key_off) return PBL_OK;
  for (uint32_t i = 0; i < n; i++) {
    uint64_t k = O.blk_kv_base[i];
    uint32_t ko = 0, vo = 0;
    if (bounds[i].status == PBL_OK)
      walk(bounds[i], [&](uint64_t kv, uint32_t b) {
        const uint32_t k0 = D.key_off[kv + b], kl = D.key_off[kv + b + 1] - k0;
        const uint32_t v0 = D.val_off[kv + b], vl = D.val_off[kv + b + 1] - v0;
        O.trailer[k] = D.trailer[kv];
        if (O.kv_flags) O.kv_flags[k] = D.kv_flags ? D.kv_flags[kv] : uint8_t(0);
        if (O.entry_off && D.entry_off) O.entry_off[k] = D.entry_off[kv];
        if (O.tiering_span_id && D.tiering_span_id) {
          O.tiering_span_id[k] = D.tiering_span_id[kv];
          O.tiering_attr[k] = D.tiering_attr[kv];
        }
        if (out->src_kv) out->src_kv[k] = kv;
        O.key_off[k + i] = ko;
        O.val_off[k + i] = vo;
        if (kl) memcpy(O.key_bytes + O.blk_key_base[i] + ko, D.key_bytes + D.blk_key_base[b] + k0, kl);
        if (vl) memcpy(O.val_bytes + O.blk_val_base[i] + vo, D.val_bytes + D.blk_val_base[b] + v0, vl);
        ko += kl;
        vo += vl;
        k++;
      });
    O.key_off[k + i] = ko;
    O.val_off[k + i] = vo;
  }
  return PBL_OK;
}

size_t pbl_scan_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_scan_queries), PBL_OFF(pbl_scan_queries, lower_bytes), PBL_OFF(pbl_scan_queries, lower_off),
      PBL_OFF(pbl_scan_queries, upper_bytes), PBL_OFF(pbl_scan_queries, upper_off), PBL_OFF(pbl_scan_queries, flags),
      PBL_OFF(pbl_scan_queries, block), PBL_OFF(pbl_scan_queries, n), PBL_OFF(pbl_scan_queries, comparer),
      PBL_OFF(pbl_scan_queries, hide_obsolete_points), PBL_OFF(pbl_scan_queries, reserved),
      sizeof(pbl_scan_out), PBL_OFF(pbl_scan_out, result), PBL_OFF(pbl_scan_out, range),
      PBL_OFF(pbl_scan_out, src_kv)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
