// seek_core.hip.h — the search of the batched seeks and scans, stated once
// (DESIGN.md §3.9, §3.10): the fence record, the view of a decoded batch, the
// lower bound inside a block, the search over the fence and the whole seek of
// one key.  Every function is templated on a byte reader R (key_cmp.hip.h):
// seek.hip and scan.hip instantiate them with GlobalReader in their kernels and
// with cmp::HostReader in pbl_seek_batch_host / pbl_scan_batch_host.
#pragma once
#include <type_traits>

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
  // 16 bytes as four little-endian words; the words past the first n bytes hold
  // whatever follows the key (filter_core.hip.h uses only the bytes inside it)
  static __device__ __forceinline__ void load_le16(gptr<const uint8_t> a, uint64_t, uint32_t w[4]) {
    const gptr<const u64u> q = (gptr<const u64u>)a;
    const uint64_t x = q[0], y = q[1];
    w[0] = uint32_t(x);
    w[1] = uint32_t(x >> 32);
    w[2] = uint32_t(y);
    w[3] = uint32_t(y >> 32);
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

// The same search over internal keys (cmp::ikey_cmp; `tr`: the trailers of the
// block's KVs): the first KV of the block that is >= the internal key (k, ktr),
// or with kAfter the first that is > it (n when there is none).  The block is
// sorted under ikey_cmp, non-strictly (merge.hip checks that before it
// searches).
template <class R, uint32_t kCmp, bool kAfter>
PBL_HD inline uint32_t ibound(const Block<R>& B, typename R::template ptr<const uint64_t> tr, cmp::kptr<R> k,
                              uint64_t kl, uint64_t ktr) {
  uint32_t lo = 0, hi = B.n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    uint64_t ml;
    const cmp::kptr<R> mk = B.key(m, &ml);
    const int c = cmp::ikey_cmp<R, kCmp>(mk, ml, tr[m], k, kl, ktr);
    if (kAfter ? c <= 0 : c < 0) lo = m + 1;
    else hi = m;
  }
  return lo;
}
template <class R, uint32_t kCmp>
PBL_HD inline uint32_t ilower(const Block<R>& B, typename R::template ptr<const uint64_t> tr, cmp::kptr<R> k,
                              uint64_t kl, uint64_t ktr) {
  return ibound<R, kCmp, false>(B, tr, k, kl, ktr);
}
template <class R, uint32_t kCmp>
PBL_HD inline uint32_t iupper(const Block<R>& B, typename R::template ptr<const uint64_t> tr, cmp::kptr<R> k,
                              uint64_t kl, uint64_t ktr) {
  return ibound<R, kCmp, true>(B, tr, k, kl, ktr);
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

// index.SeekGE (reader_iter_single_lvl.go:788-822) over the fence: the position
// of the first listed block whose last key is >= k (n_fence when there is none).
template <class R, uint32_t kCmp>
PBL_HD inline uint32_t fence_lower(const View<R>& V, cmp::kptr<R> k, uint64_t kl) {
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
  return lo;
}

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
    f = fence_lower<R, kCmp>(V, k, kl);
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

template <class F>
auto with_cmp(uint32_t c, F&& f) {
  return c == PBL_CMP_TESTKEYS ? f(std::integral_constant<uint32_t, PBL_CMP_TESTKEYS>{})
         : c == PBL_CMP_CRDB   ? f(std::integral_constant<uint32_t, PBL_CMP_CRDB>{})
                               : f(std::integral_constant<uint32_t, PBL_CMP_DEFAULT>{});
}

}  // namespace seek
}  // namespace pbl
