// compact.hip — the compaction view of a sorted decoded batch, on the device
// (DESIGN.md §3.18): result block q is what compact.Iter's First(); Next()...
// returns over block q's KVs as the point-key stream, with DefaultMerger
// (internal/compact/iterator.go:439-1363; include/pebble_amd.h states the rules).
//
// Everything the iterator does to a KV depends on the KVs before it in its
// segment (equal user key, equal snapshot stripe), and a segment may be of any
// length.  Each KV is a map on eight states -- seeking, SET head looking for a
// tombstone, merging, SINGLEDEL pending, SINGLEDEL pending under elision,
// DELSIZED holding a value, DELSIZED with an empty value, skipping -- 8 -> 8 in
// 32 bits; a segment's first KV first resets to seeking, composition is
// associative, and a scan of the maps over the flat KV index gives every KV its
// incoming state.  What looks non-local is local: the holder of a DELSIZED's
// value is always the KV just before (the size comparison reads one neighbour),
// a chain's handle check reads one neighbour, and `pinned` depends on a head and
// the KV before it.  Nothing below loops over a segment.
//
// Unlike the reader's view, a result's final kind, and for SINGLEDEL whether it
// exists at all, is decided by a later KV.  Two devices settle that:
//   - a result whose existence is known at its head (SET, SETWITHDEL, MERGE,
//     DEL, DELSIZED) is counted at the head and written by it; the KV that later
//     ends the episode (the first tombstone after a SET, a chain's end, the KV
//     that turns a DELSIZED into a DEL) patches the kind byte of the last result
//     before it, in the launch after the one that wrote the trailers;
//   - a SINGLEDEL's result is counted at the KV that decides it (the KV after
//     the run of SINGLEDELs, or the segment's last KV).  That KV needs its head:
//     the first of the run of consecutive SINGLEDELs it closes, a "last run
//     start" scan that does not depend on the states and rides with the maps.
// A DELSIZED's value is contributed by the segment's last KV (when that is a
// DELSIZED with a value met in a DELSIZED state) and placed as a chain's
// operands are: at X[r] + X[r+1] - P[i].
//
//   compact_classify_kernel<comparer>  tile of 256 source KVs per workgroup:
//       stripe (binary search of the snapshots), comparison with the successor,
//       kind, flags, the neighbour facts; the tile's map and last run start
//   compact_chunk_map_kernel / compact_state_kernel  every tile's incoming state
//       and run start, chunked two-launch form (visible.hip)
//   compact_role_kernel  per tile: states, roles, counters, head indices; the
//       tile's sums of {results, contributors, key bytes, value bytes}
//   compact_chunk_sum_kernel / compact_tile_scan_kernel / compact_prefix_kernel
//       the exclusive prefixes of every KV
//   compact_persize_kernel / compact_sum_kernel / compact_bases_kernel
//       per-block status and sizes; result_core.hip.h's scan over blocks; counters
//   compact_heads_kernel   every result's arrays, trailer, key, pinned
//   compact_values_kernel  values (result_core.hip.h's copy_values), n_src, the
//       kind patches
//
// Both emit kernels check what they read from the workspace against the source
// block and the result block's recorded sizes.
//
// pbl_compact_batch_host is the sequential loop, a different algorithm on purpose.
#include <algorithm>
#include <vector>

#include "result_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace compact {

constexpr uint64_t kHdr = 64;
constexpr uint32_t kTileShift = 8, kTile = 1u << kTileShift;  // source KVs per tile
constexpr int kTPB = 256;
constexpr uint32_t kChunk = 256;
static_assert(kTPB == result::kTPB && kChunk == uint32_t(result::kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kGrid = 2048;
constexpr uint64_t kMaxBytes = 0xffffffffull;
constexpr uint64_t kMaxKvs = 0xffffffffull;
enum { kHSkip = 0 };  // header word 0: nonzero = sizes only

// classes of a KV (bits 0-2 of its code) and their InternalKeyKind (internal/base/internal.go:29-130)
enum : uint32_t { kD = 0, kS = 1, kM = 2, kX = 3, kW = 4, kZ = 5, kNoClass = 7 };
PBL_HD inline uint32_t kind_of_class(uint32_t c) {
  return c == kD ? 0u : c == kS ? 1u : c == kM ? 2u : c == kX ? 7u : c == kW ? 18u : 23u;
}
PBL_HD inline uint32_t class_of_kind(uint32_t k) {
  return k == 0 ? kD : k == 1 ? kS : k == 2 ? kM : k == 7 ? kX : k == 18 ? kW : k == 23 ? kZ : uint32_t(kNoClass);
}
PBL_HD inline bool is_tomb(uint32_t c) { return c == kD || c == kX || c == kZ; }
// the facts of a KV, from the classify kernel
constexpr uint32_t kCls = 7, kSegStart = 0x8, kKeyStart = 0x10, kHandle = 0x20, kStripe0 = 0x40, kSegLast = 0x80,
                   kHasVal = 0x100,     // its value is not empty
                   kPredMatch = 0x200,  // the KV before is a DELSIZED whose uvarint equals this KV's key + value bytes
                   kPredBad = 0x400,    // the KV before is a DELSIZED whose value is not exactly one uvarint
                   kNextSame = 0x800,   // the KV after has the same user key and is SET / SETWITHDEL / MERGE
                   kPredHandle = 0x1000, kPredX = 0x2000;
// its role, from the role kernel
constexpr uint32_t kSlot = 0x10000,     // carries a result
                   kValue = 0x20000,    // its value goes into the last result at or before it
                   kPatchShift = 18,    // 3 bits: 0, or 1 + the class that result's kind becomes
                   kEmitShift = 21,     // 3 bits: the class its own result is emitted with
                   kZeroSeq = 0x1000000;  // its result gets sequence number 0
constexpr uint32_t kBadOrder = 1, kBadKind = 2, kBadCorrupt = 4;
constexpr uint32_t kHandleBits = PBL_KV_VALBLK_HANDLE | PBL_KV_BLOB_HANDLE;

enum : uint32_t { sSeek = 0, sSetL = 1, sMrg = 2, sSdp = 3, sSde = 4, sDsv = 5, sDse = 6, sSkip = 7 };
// a map holds the image of state s in bits 4s..4s+2
constexpr uint32_t kIdentity = 0x76543210u;
PBL_HD inline uint32_t map_apply(uint32_t m, uint32_t s) { return (m >> (4 * s)) & 7u; }
PBL_HD inline uint32_t map_then(uint32_t a, uint32_t b) {  // a, then b
  uint32_t r = 0;
#pragma unroll
  for (uint32_t s = 0; s < 8; s++) r |= map_apply(b, map_apply(a, s)) << (4 * s);
  return r;
}

// What a KV does when the state before it is s (include/pebble_amd.h, head rules).
struct Step {
  uint32_t next;
  uint32_t emit;   // 0, or 1 + the class of the result this KV carries
  uint32_t patch;  // 0, or 1 + the class the last result's kind becomes
  bool value, zero_seq, bad_handle, corrupt;
  uint32_t miss, ineff, nondet;
};
PBL_HD inline Step step(uint32_t s, uint32_t code, uint32_t flags) {
  Step r{};
  const uint32_t c = code & kCls;
  if (code & kSegStart) s = sSeek;
  const bool st0 = (code & kStripe0) != 0;
  const bool elid = (flags & PBL_COMPACT_ELIDE_TOMBSTONES) && st0;
  const bool bottom = (flags & PBL_COMPACT_BOTTOMMOST) && st0;
  const bool tomb = is_tomb(c);
  const uint32_t held = (code & kHasVal) ? uint32_t(sDsv) : uint32_t(sDse);  // a DELSIZED's state by its own value
  r.next = s;
  switch (s) {
    case sSeek:
      if (c == kD) {
        r.next = sSkip;
        if (!elid) r.emit = 1 + kD;
      } else if (c == kZ) {
        r.next = elid ? uint32_t(sSkip) : held;
        if (!elid) r.emit = 1 + kZ;
      } else if (c == kX) {
        r.next = elid ? sSde : sSdp;
      } else if (c == kS) {
        r.next = sSetL;
        r.emit = 1 + kS;
        r.value = true;
        r.zero_seq = bottom;
      } else if (c == kW) {
        r.next = sSkip;
        r.emit = 1 + kW;
        r.value = true;
        r.zero_seq = bottom;
      } else {
        r.next = sMrg;
        r.emit = 1 + (bottom ? kS : kM);
        r.value = true;
        r.zero_seq = bottom;
      }
      break;
    case sSetL:
      if (tomb) {
        r.patch = 1 + kW;
        r.next = sSkip;
      }
      break;
    case sMrg:
      if (tomb) {
        r.patch = 1 + kW;
        r.next = sSkip;
      } else {
        r.value = true;
        r.bad_handle = (code & (kHandle | kPredHandle)) != 0;
        if (c != kM) {
          r.patch = 1 + kS;
          r.next = sSkip;
        }
      }
      break;
    case sSdp:
    case sSde:
      if (c == kX) {
        r.ineff = 1;
      } else if (c == kD || c == kZ || c == kW) {
        r.ineff = c != kW;
        if (s == sSdp) r.emit = 1 + kD;
        r.next = sSkip;
      } else {
        r.next = sSeek;
        r.nondet = (code & kNextSame) ? 1u : 0u;
      }
      break;
    case sDsv:
      r.corrupt = (code & kPredBad) != 0;
      if (tomb) {
        r.miss = 1;
        if (c == kZ) r.next = held;
        else {
          r.patch = 1 + kD;
          r.next = sSkip;
        }
      } else if (code & kPredMatch) {
        r.next = sDse;
      } else {
        r.miss = 1;
        r.patch = 1 + kD;
        r.next = sSkip;
      }
      break;
    case sDse:
      if (c == kZ) r.next = held;
      else {
        r.patch = 1 + kD;
        r.next = sSkip;
      }
      break;
    default:
      break;
  }
  if (code & kSegLast) {  // the segment ends on this KV
    if (r.next == sSdp) r.emit = 1 + kX;
    if (r.next == sSde) r.ineff += 1;
    if (r.next == sDsv) r.value = true;
  }
  return r;
}
PBL_HD inline uint32_t map_of(uint32_t code, uint32_t flags) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t s = 0; s < 8; s++) m |= step(s, code, flags).next << (4 * s);
  return m;
}
// The "last run start" value of a KV: 0 for a SINGLEDEL that continues a run of
// SINGLEDELs inside its segment, its index + 1 otherwise.
PBL_HD inline uint64_t run_of(uint32_t code, uint64_t i) {
  return ((code & kCls) == kX && (code & kPredX) && !(code & kSegStart)) ? 0 : i + 1;
}
// binary.Uvarint over exactly n bytes: true and the value iff the bytes are one uvarint
template <class P>
PBL_HD inline bool uvarint_exact(P p, uint64_t n, uint64_t* out) {
  uint64_t x = 0;
  if (n == 0 || n > 10) return false;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t b = p[i];
    if (i == 9 && b > 1) return false;
    x |= uint64_t(b & 0x7f) << (7 * i);
    if (b < 0x80) {
      *out = x;
      return i + 1 == n;
    }
  }
  return false;
}
// Snapshots.Index: the snapshots <= seq
template <class P>
PBL_HD inline uint64_t stripe_of(P snaps, uint64_t n, uint64_t seq) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t m = lo + (hi - lo) / 2;
    if (snaps[m] > seq) hi = m;
    else lo = m + 1;
  }
  return lo;
}

struct Layout {
  uint64_t nt, ntc;
  uint64_t bad, cnt, qst, q64, csum, tsum, tcs, pre, trs, trin, tcr, hd, tmap, tin, tcm, blk, cst, code, size;
  uint32_t n_chunks;
};
__host__ __device__ inline Layout layout(uint32_t nb, uint64_t n_kv) {
  Layout L;
  L.nt = (n_kv >> kTileShift) + 1;
  L.ntc = (L.nt + kChunk - 1) / kChunk;
  L.n_chunks = nb ? (nb + kChunk - 1) / kChunk : 1;
  uint64_t o = kHdr;
  L.bad = o;  o += 4ull * nb;
  L.cnt = o;  o += 3ull * 4 * nb;
  L.qst = o;  o += 4ull * nb;
  o = (o + 15) & ~uint64_t(15);
  L.q64 = o;  o += 3ull * 8 * (uint64_t(nb) + 1);
  L.csum = o; o += 3ull * 8 * L.n_chunks;
  L.tsum = o; o += 4ull * 8 * L.nt;
  L.tcs = o;  o += 4ull * 8 * L.ntc;
  L.pre = o;  o += 4ull * 8 * (n_kv + 1);
  L.trs = o;  o += 8ull * L.nt;
  L.trin = o; o += 8ull * L.nt;
  L.tcr = o;  o += 8ull * L.ntc;
  L.hd = o;   o += 8ull * n_kv;
  L.tmap = o; o += 4ull * L.nt;
  L.tin = o;  o += 4ull * L.nt;
  L.tcm = o;  o += 4ull * L.ntc;
  L.blk = o;  o += 4ull * n_kv;
  L.cst = o;  o += 4ull * (n_kv + 1);
  L.code = o; o += 4ull * n_kv;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

// ---- device side ---------------------------------------------------------------
struct Args {
  pbl_decode_out in;
  pbl_compact_out out;
  uint32_t n_blocks, comparer, size_only, flags;
  uint64_t n_kv;
  const uint64_t* snaps;
  uint64_t n_snaps;
  uint8_t* ws;
};

struct Ws {
  gptr<uint32_t> hdr, bad, cnt, qst, tmap, tin, tcm, blk, cst, code;
  gptr<uint64_t> q64, csum, tsum, tcs, pre, trs, trin, tcr, hd;
  uint64_t nt, ntc, qs, ps;
  uint32_t n_chunks;
  __device__ Ws(uint8_t* ws, uint32_t nb, uint64_t n_kv) {
    const Layout L = layout(nb, n_kv);
    auto w32 = [&](uint64_t o) { return to_glb(reinterpret_cast<uint32_t*>(ws + o)); };
    auto w64 = [&](uint64_t o) { return to_glb(reinterpret_cast<uint64_t*>(ws + o)); };
    hdr = w32(0);
    bad = w32(L.bad);
    cnt = w32(L.cnt);
    qst = w32(L.qst);
    q64 = w64(L.q64);
    csum = w64(L.csum);
    tsum = w64(L.tsum);
    tcs = w64(L.tcs);
    pre = w64(L.pre);
    trs = w64(L.trs);
    trin = w64(L.trin);
    tcr = w64(L.tcr);
    hd = w64(L.hd);
    tmap = w32(L.tmap);
    tin = w32(L.tin);
    tcm = w32(L.tcm);
    blk = w32(L.blk);
    cst = w32(L.cst);
    code = w32(L.code);
    nt = L.nt;
    ntc = L.ntc;
    qs = uint64_t(nb) + 1;
    ps = n_kv + 1;
    n_chunks = L.n_chunks;
  }
  __device__ gptr<uint64_t> q(int c) const { return q64 + uint64_t(c) * qs; }
  __device__ result::Sizes sizes() const { return result::Sizes{q64, csum, qst, qs, n_chunks}; }
  __device__ gptr<uint64_t> ts(int c) const { return tsum + uint64_t(c) * nt; }
  // per-KV exclusive prefixes (n_kv + 1 entries each): 0 results, 1 contributors, 2 key bytes, 3 value bytes
  __device__ gptr<uint64_t> p(int c) const { return pre + uint64_t(c) * ps; }
};
enum { kPH = 0, kPC = 1, kPK = 2, kPV = 3 };

__device__ inline uint64_t held(const Args& A) { return A.n_blocks ? to_glb(A.in.blk_kv_base)[A.n_blocks] : 0; }
__device__ inline bool described(const Args& A) { return held(A) <= A.n_kv; }

using result::block_excl_scan64;
using result::block_of;
using result::block_sum64;

// Exclusive scan of maps under map_then over the workgroup (visible.hip's, for
// these maps); *total = all 256.  `lds`: 4 words.
__device__ inline uint32_t block_excl_scan_map(uint32_t m, uint32_t* lds, uint32_t* total) {
  const int l = lane_id();
  uint32_t inc = m;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t o = uint32_t(__shfl_up(int(inc), d, kWave));
    if (l >= d) inc = map_then(o, inc);
  }
  uint32_t ex = uint32_t(__shfl_up(int(inc), 1, kWave));
  if (l == 0) ex = kIdentity;
  __syncthreads();
  if (l == kWave - 1) lds[wave_id()] = inc;
  __syncthreads();
  uint32_t before = kIdentity, t = kIdentity;
  for (int w = 0; w < kTPB / kWave; w++) {
    const uint32_t s = lds[w];
    if (w < wave_id()) before = map_then(before, s);
    t = map_then(t, s);
  }
  *total = t;
  return map_then(before, ex);
}
// Exclusive "last nonzero" scan over the workgroup: the last nonzero value of
// the threads before this one, 0 for none; *total = the last nonzero of all.
__device__ inline uint64_t block_excl_scan_last(uint64_t v, uint64_t* lds, uint64_t* total) {
  const int l = lane_id();
  uint64_t inc = v;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint64_t o = __shfl_up((unsigned long long)inc, d, kWave);
    if (l >= d && !inc) inc = o;
  }
  uint64_t ex = __shfl_up((unsigned long long)inc, 1, kWave);
  if (l == 0) ex = 0;
  __syncthreads();
  if (l == kWave - 1) lds[wave_id()] = inc;
  __syncthreads();
  uint64_t before = 0, t = 0;
  for (int w = 0; w < kTPB / kWave; w++) {
    const uint64_t s = lds[w];
    if (w < wave_id() && s) before = s;
    if (s) t = s;
  }
  *total = t;
  return ex ? ex : before;
}

using GR = seek::GlobalReader;

__device__ inline seek::View<GR> in_view(const Args& A) {
  pbl_seek_queries sq{};
  return seek::View<GR>(A.in, A.n_blocks, sq, nullptr, 0);
}

// What a KV's neighbours need to know about it.
struct Info {
  uint32_t cls;
  bool handle, uv_ok, has_val;
  uint64_t stripe, expect, klen, vlen;
};
// KV j of block B (q), global index i = B.kv0 + j.
__device__ inline Info info_of(const Args& A, const seek::Block<GR>& B, uint32_t q, uint32_t j) {
  Info I{};
  const uint64_t i = B.kv0 + j;
  const uint64_t t = to_glb(A.in.trailer)[i];
  I.cls = class_of_kind(uint32_t(t & 0xff));
  I.handle = A.in.kv_flags && (to_glb(A.in.kv_flags)[i] & kHandleBits);
  I.stripe = stripe_of(to_glb(A.snaps), A.n_snaps, t >> 8);
  const uint32_t v0 = to_glb(A.in.val_off)[i + q], v1 = to_glb(A.in.val_off)[i + q + 1];
  const uint32_t k0 = to_glb(A.in.key_off)[i + q], k1 = to_glb(A.in.key_off)[i + q + 1];
  I.vlen = v1 - v0;
  I.klen = k1 - k0;
  I.has_val = I.vlen != 0;
  if (I.cls == kZ && I.has_val)
    I.uv_ok = uvarint_exact(to_glb((const uint8_t*)A.in.val_bytes) + (to_glb(A.in.blk_val_base)[q] + v0), I.vlen, &I.expect);
  return I;
}

template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void compact_classify_kernel(Args A) {
  __shared__ uint32_t lds[4];
  __shared__ uint64_t lds64[4];
  __shared__ uint32_t sh_next[kTile];   // bit 0: the KV after starts a key; bit 1: starts a segment
  __shared__ uint32_t sh_me[kTile];     // class | handle << 3 | (DELSIZED with a value: 1 << 4, uvarint ok: 1 << 5)
  __shared__ uint64_t sh_stripe[kTile], sh_expect[kTile];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint32_t nb = A.n_blocks;
  const uint64_t n = held(A);
  const seek::View<GR> V = in_view(A);
  const gptr<const uint64_t> tr = to_glb((const uint64_t*)A.in.trailer);
  const gptr<const uint8_t> fl = to_glb((const uint8_t*)A.in.kv_flags);
  auto pack = [](const Info& I) {
    return I.cls | (I.handle ? 8u : 0u) | ((I.cls == kZ && I.has_val) ? 16u : 0u) | (I.uv_ok ? 32u : 0u);
  };
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    bool live = false, first_of_block = true, last_of_block = true;
    uint32_t q = 0, j = 0, code = kNoClass, nx = 3, badw = 0;
    Info me{};
    if (i < n) {
      q = block_of(V.blk_kv_base, nb, i);
      W.blk[i] = q;
    }
    const seek::Block<GR> B(V, q);
    if (i < n && V.blk_status[q] == PBL_OK && i >= B.kv0 && i - B.kv0 < B.n) {
      live = true;
      j = uint32_t(i - B.kv0);
      me = info_of(A, B, q, j);
      first_of_block = j == 0;
      last_of_block = j + 1 == B.n;
    }
    __syncthreads();
    sh_me[threadIdx.x] = live ? pack(me) : uint32_t(kNoClass);
    sh_stripe[threadIdx.x] = me.stripe;
    sh_expect[threadIdx.x] = me.expect;
    __syncthreads();
    if (live) {
      const uint32_t f = fl ? fl[i] : 0u;
      if (me.cls == kNoClass || (f & PBL_KV_INVALID_KEY)) badw |= kBadKind;
      code = me.cls | (me.handle ? kHandle : 0u) | (me.has_val ? kHasVal : 0u) | (me.stripe == 0 ? kStripe0 : 0u);
      if (!last_of_block) {
        uint32_t nme;
        uint64_t nstripe;
        if (threadIdx.x + 1 < kTile) {
          nme = sh_me[threadIdx.x + 1];
          nstripe = sh_stripe[threadIdx.x + 1];
        } else {
          const Info N = info_of(A, B, q, j + 1);
          nme = pack(N);
          nstripe = N.stripe;
        }
        uint64_t al, bl;
        const cmp::kptr<GR> a = B.key(j, &al), b = B.key(j + 1, &bl);
        const int c = cmp::key_cmp<GR>(kCmp, a, al, b, bl);
        nx = (c != 0 ? 1u : 0u) | ((c != 0 || nstripe != me.stripe) ? 2u : 0u);
        if (c > 0 || (c == 0 && (tr[i] >> 8) <= (tr[i + 1] >> 8))) badw |= kBadOrder;
        const uint32_t nc = nme & 7u;
        if (c == 0 && (nc == kS || nc == kW || nc == kM)) code |= kNextSame;
      }
      if (!first_of_block) {
        uint32_t pme;
        uint64_t pexpect;
        if (threadIdx.x > 0) {
          pme = sh_me[threadIdx.x - 1];
          pexpect = sh_expect[threadIdx.x - 1];
        } else {  // the tile's first KV looks back once
          const Info P = info_of(A, B, q, j - 1);
          pme = pack(P);
          pexpect = P.expect;
          uint64_t al, bl;
          const cmp::kptr<GR> a = B.key(j - 1, &al), b = B.key(j, &bl);
          const int c = cmp::key_cmp<GR>(kCmp, a, al, b, bl);
          if (c != 0) code |= kKeyStart | kSegStart;
          else if (P.stripe != me.stripe) code |= kSegStart;
        }
        if (pme & 8u) code |= kPredHandle;
        if ((pme & 7u) == kX) code |= kPredX;
        if (pme & 16u) {
          if (!(pme & 32u)) code |= kPredBad;
          else if (pexpect == me.klen + me.vlen) code |= kPredMatch;
        }
      }
      if (badw) g_atomic_or((uint32_t*)(W.bad + q), badw);
    }
    __syncthreads();
    sh_next[threadIdx.x] = nx;
    __syncthreads();
    if (first_of_block) code |= kKeyStart | kSegStart;
    else if (threadIdx.x > 0) code |= ((sh_next[threadIdx.x - 1] & 1u) ? kKeyStart : 0u) | ((sh_next[threadIdx.x - 1] & 2u) ? kSegStart : 0u);
    if (nx & 2u) code |= kSegLast;
    if (i < n) W.code[i] = code;
    uint32_t total;
    block_excl_scan_map(i < n ? map_of(code, A.flags) : kIdentity, lds, &total);
    uint64_t rtot;
    block_excl_scan_last(i < n ? run_of(code, i) : 0, lds64, &rtot);
    if (threadIdx.x == 0) {
      W.tmap[t] = total;
      W.trs[t] = rtot;
    }
  }
}

// Per chunk of kChunk tiles: the composition of its tiles' maps, its last run start.
__global__ __launch_bounds__(kTPB) void compact_chunk_map_kernel(Args A) {
  __shared__ uint32_t lds[4];
  __shared__ uint64_t lds64[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  for (uint64_t c = blockIdx.x; c < W.ntc; c += gridDim.x) {
    const uint64_t t = c * kChunk + threadIdx.x;
    uint32_t total;
    block_excl_scan_map(t < W.nt ? W.tmap[t] : kIdentity, lds, &total);
    uint64_t rtot;
    block_excl_scan_last(t < W.nt ? W.trs[t] : 0, lds64, &rtot);
    if (threadIdx.x == 0) {
      W.tcm[c] = total;
      W.tcr[c] = rtot;
    }
  }
}

// Every tile's incoming state and run start: the chunks before this one in
// order, then the scan inside the chunk.
__global__ __launch_bounds__(kTPB) void compact_state_kernel(Args A) {
  __shared__ uint32_t lds[4];
  __shared__ uint64_t lds64[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  for (uint64_t c = blockIdx.x; c < W.ntc; c += gridDim.x) {
    uint32_t carry = sSeek;
    uint64_t rcarry = 0;
    for (uint64_t c0 = 0; c0 < c; c0 += kTPB) {
      const bool in = c0 + threadIdx.x < c;
      uint32_t total;
      block_excl_scan_map(in ? W.tcm[c0 + threadIdx.x] : kIdentity, lds, &total);
      carry = map_apply(total, carry);
      uint64_t rtot;
      block_excl_scan_last(in ? W.tcr[c0 + threadIdx.x] : 0, lds64, &rtot);
      if (rtot) rcarry = rtot;
    }
    const uint64_t t = c * kChunk + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_excl_scan_map(t < W.nt ? W.tmap[t] : kIdentity, lds, &total);
    uint64_t rtot;
    const uint64_t rex = block_excl_scan_last(t < W.nt ? W.trs[t] : 0, lds64, &rtot);
    if (t < W.nt) {
      W.tin[t] = map_apply(ex, carry);
      W.trin[t] = rex ? rex : rcarry;
    }
  }
}

// What a KV with this role adds to {results, contributors, key bytes, value bytes}.
__device__ inline void contribution(const Args& A, const Ws& W, uint64_t i, uint32_t code, uint64_t* v) {
  const bool slot = (code & kSlot) != 0, val = (code & kValue) != 0;
  v[kPH] = slot;
  v[kPC] = slot || (val && (code & kCls) != kZ);  // a result, or a chain's operand (not a DELSIZED's adopted value)
  v[kPK] = v[kPV] = 0;
  const uint32_t q = W.blk[i];
  if (val) v[kPV] = to_glb(A.in.val_off)[i + q + 1] - to_glb(A.in.val_off)[i + q];
  if (slot) {
    const uint64_t h = W.hd[i];  // (checked by the role kernel)
    v[kPK] = to_glb(A.in.key_off)[h + q + 1] - to_glb(A.in.key_off)[h + q];
  }
}

__global__ __launch_bounds__(kTPB) void compact_role_kernel(Args A) {
  __shared__ uint32_t lds32[4];
  __shared__ uint64_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint64_t n = held(A);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    uint32_t code = i < n ? W.code[i] : uint32_t(kNoClass | kSegStart);
    uint32_t total;
    const uint32_t ex = block_excl_scan_map(i < n ? map_of(code, A.flags) : kIdentity, lds32, &total);
    uint64_t rtot;
    uint64_t rex = block_excl_scan_last(i < n ? run_of(code, i) : 0, lds, &rtot);
    if (!rex) rex = W.trin[t];
    uint64_t v[4] = {0, 0, 0, 0};
    if (i < n && (code & kCls) != kNoClass) {
      const uint32_t q = W.blk[i];
      const uint32_t s = map_apply(ex, W.tin[t]);
      const Step S = step(s, code, A.flags);
      uint32_t badw = (S.bad_handle ? kBadKind : 0u) | (S.corrupt ? kBadCorrupt : 0u);
      code &= 0xffffu;
      if (S.value) code |= kValue;
      code |= S.patch << kPatchShift;
      if (S.emit) {
        code |= kSlot | ((S.emit - 1) << kEmitShift) | (S.zero_seq ? kZeroSeq : 0u);
        // the head: this KV, or for a SINGLEDEL decided here the start of the run it closes
        uint64_t h = i;
        const uint32_t state = (code & kSegStart) ? uint32_t(sSeek) : s;
        if (state == sSdp || (state == sSeek && (code & kCls) == kX)) {
          const uint64_t r = run_of(code, i) ? ((code & kCls) == kX ? i + 1 : rex) : rex;
          h = r ? r - 1 : ~0ull;
        }
        const uint64_t kv0 = to_glb(A.in.blk_kv_base)[q];
        if (h > i || h < kv0) {  // (no input leads here; a stale workspace might)
          badw |= kBadKind;
          h = i;
        }
        W.hd[i] = h;
      }
      if (S.miss) g_atomic_add((uint32_t*)(W.cnt + 3ull * q), S.miss);
      if (S.ineff) g_atomic_add((uint32_t*)(W.cnt + 3ull * q + 1), S.ineff);
      if (S.nondet) g_atomic_add((uint32_t*)(W.cnt + 3ull * q + 2), S.nondet);
      if (badw) g_atomic_or((uint32_t*)(W.bad + q), badw);
      W.code[i] = code;
      contribution(A, W, i, code, v);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint64_t sum = block_sum64(v[c], lds);
      if (threadIdx.x == 0) W.ts(c)[t] = sum;
    }
  }
}

__global__ __launch_bounds__(kTPB) void compact_chunk_sum_kernel(Args A) {
  __shared__ uint64_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  for (uint64_t ch = blockIdx.x; ch < W.ntc; ch += gridDim.x) {
    const uint64_t t = ch * kChunk + threadIdx.x;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint64_t s = block_sum64(t < W.nt ? W.ts(c)[t] : 0, lds);
      if (threadIdx.x == 0) W.tcs[uint64_t(c) * W.ntc + ch] = s;
    }
  }
}

__global__ __launch_bounds__(kTPB) void compact_tile_scan_kernel(Args A) {
  __shared__ uint64_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  for (uint64_t ch = blockIdx.x; ch < W.ntc; ch += gridDim.x) {
    const uint64_t t = ch * kChunk + threadIdx.x;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      uint64_t before = 0;
      for (uint64_t e = threadIdx.x; e < ch; e += kTPB) before += W.tcs[uint64_t(c) * W.ntc + e];
      before = block_sum64(before, lds);
      uint64_t tot;
      const uint64_t ex = block_excl_scan64(t < W.nt ? W.ts(c)[t] : 0, lds, &tot);
      if (t < W.nt) W.ts(c)[t] = before + ex;
    }
  }
}

__global__ __launch_bounds__(kTPB) void compact_prefix_kernel(Args A) {
  __shared__ uint64_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint64_t n = held(A);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    uint64_t v[4] = {0, 0, 0, 0};
    if (i < n) {
      const uint32_t code = W.code[i];
      if ((code & kCls) != kNoClass) contribution(A, W, i, code, v);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      uint64_t tot;
      const uint64_t ex = W.ts(c)[t] + block_excl_scan64(v[c], lds, &tot);
      if (i <= n) W.p(c)[i] = ex;  // (entry n: the totals)
    }
  }
}

// Lane per block: its status and sizes.
__global__ __launch_bounds__(kTPB) void compact_persize_kernel(Args A) {
  const uint64_t q = uint64_t(blockIdx.x) * kTPB + threadIdx.x;
  if (q >= A.n_blocks) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  uint32_t st = described(A) ? to_glb(A.in.blk_status)[q] : uint32_t(PBL_INVALID_ARG);
  uint64_t n = 0, k = 0, v = 0;
  if (st == PBL_OK) {
    const uint64_t a = to_glb(A.in.blk_kv_base)[q], b = to_glb(A.in.blk_kv_base)[q + 1];
    const uint32_t bad = W.bad[q];
    if (a > b || b > held(A) || (bad & kBadOrder)) st = PBL_INVALID_ARG;
    else if (bad & kBadKind) st = PBL_UNSUPPORTED;
    else if (bad & kBadCorrupt) st = PBL_CORRUPT_BOUNDS;
    else {
      n = W.p(kPH)[b] - W.p(kPH)[a];
      k = W.p(kPK)[b] - W.p(kPK)[a];
      v = W.p(kPV)[b] - W.p(kPV)[a];
      if (n > kMaxKvs || k > kMaxBytes || v > kMaxBytes) st = PBL_UNSUPPORTED;
    }
  }
  const bool some = st == PBL_OK;
  W.q(0)[q] = some ? n : 0;
  W.q(1)[q] = some ? k : 0;
  W.q(2)[q] = some ? v : 0;
  W.qst[q] = st;
}

__global__ __launch_bounds__(kTPB) void compact_sum_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  result::chunk_sums<3>(W.sizes(), A.n_blocks, lds);
}

// The result's bases, statuses and totals, the capacity check; the counters.
__global__ __launch_bounds__(kTPB) void compact_bases_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  uint64_t ex[3], end[3];
  bool over;
  if (result::bases<3>(W.sizes(), A.out.result, A.n_blocks, A.size_only != 0, lds, ex, end, &over))
    W.hdr[kHSkip] = (over || !described(A)) ? 1u : 0u;
  const uint64_t q = uint64_t(blockIdx.x) * kTPB + threadIdx.x;
  if (q < A.n_blocks) {
    const bool ok = W.qst[q] == PBL_OK;
    if (A.out.n_missized) to_glb(A.out.n_missized)[q] = ok ? W.cnt[3 * q] : 0u;
    if (A.out.n_ineffectual) to_glb(A.out.n_ineffectual)[q] = ok ? W.cnt[3 * q + 1] : 0u;
    if (A.out.n_nondeterministic) to_glb(A.out.n_nondeterministic)[q] = ok ? W.cnt[3 * q + 2] : 0u;
  }
}

// A source KV and the result it writes to: its own (a slot) or the last one at
// or before it (a value, a patch).
struct Place {
  bool ok;
  uint32_t q, code;
  uint64_t kv0, kv1;
  uint64_t p;             // the result KV, global
  uint64_t ksize, vsize;  // the result block's bytes
};
// i < held.  Everything read from the workspace is checked against the source
// block and the result block's sizes.
__device__ inline Place place_of(const Args& A, const Ws& W, uint64_t i) {
  const pbl_decode_out& O = A.out.result;
  Place P{};
  P.code = W.code[i];
  P.q = W.blk[i];
  if (!(P.code & (kSlot | kValue | (7u << kPatchShift))) || P.q >= A.n_blocks) return P;
  if (to_glb(O.blk_status)[P.q] != PBL_OK) return P;
  P.kv0 = to_glb(A.in.blk_kv_base)[P.q];
  P.kv1 = to_glb(A.in.blk_kv_base)[P.q + 1];
  if (i < P.kv0 || i >= P.kv1 || P.kv1 > A.n_kv) return P;
  uint64_t r = W.p(kPH)[i] - W.p(kPH)[P.kv0];
  if (!(P.code & kSlot)) r -= 1;  // (0 - 1 fails the check below)
  const uint64_t o0 = to_glb(O.blk_kv_base)[P.q], o1 = to_glb(O.blk_kv_base)[P.q + 1];
  if (o1 < o0 || o1 > O.kv_cap || r >= o1 - o0) return P;
  P.p = o0 + r;
  const uint64_t k0 = to_glb(O.blk_key_base)[P.q], k1 = to_glb(O.blk_key_base)[P.q + 1];
  const uint64_t v0 = to_glb(O.blk_val_base)[P.q], v1 = to_glb(O.blk_val_base)[P.q + 1];
  if (k1 < k0 || k1 > O.key_cap || v1 < v0 || v1 > O.val_cap) return P;
  P.ksize = k1 - k0;
  P.vsize = v1 - v0;
  P.ok = true;
  return P;
}

#ifndef PBL_COMPACT_EMIT_WAVES
#define PBL_COMPACT_EMIT_WAVES 5  // as every caller of result::copy_values
#endif
// Every result KV's arrays, trailer, offsets, key and pinned; every block's last offset.
__global__ void __launch_bounds__(kTPB) __attribute__((amdgpu_waves_per_eu(PBL_COMPACT_EMIT_WAVES)))
compact_heads_kernel(Args A) {
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;  // sizes only
  const pbl_decode_out& O = A.out.result;
  const pbl_decode_out& I = A.in;
  const gptr<const uint64_t> okeyb = to_glb((const uint64_t*)O.blk_key_base);
  result::last_offsets(O, A.n_blocks, O.kv_cap);
  const uint64_t n = held(A);
  const uint64_t n_items = (n + kWave - 1) / kWave;
  const uint32_t wpb = kTPB / kWave;
  for (uint64_t item = uint64_t(blockIdx.x) * wpb + wave_id(); item < n_items; item += uint64_t(gridDim.x) * wpb) {
    const uint64_t i = item * kWave + lane_id();
    if (i >= n) continue;
    const Place P = place_of(A, W, i);
    if (!P.ok || !(P.code & kSlot)) continue;
    const uint64_t h = W.hd[i];
    if (h < P.kv0 || h > i) continue;
    const uint64_t at = h + P.q;
    const uint32_t k0 = to_glb(I.key_off)[at], klen = to_glb(I.key_off)[at + 1] - k0;
    const uint64_t ko = W.p(kPK)[i] - W.p(kPK)[P.kv0], vo = W.p(kPV)[i] - W.p(kPV)[P.kv0];
    if (ko + klen > P.ksize || vo > P.vsize) continue;
    const uint64_t p = P.p;
    result::copy_kv_arrays(O, p, I, h, uint8_t(kHandleBits), true);
    const uint64_t seq = (P.code & kZeroSeq) ? 0ull : to_glb(I.trailer)[h] >> 8;
    to_glb(O.trailer)[p] = (seq << 8) | kind_of_class((P.code >> kEmitShift) & 7u);
    if (A.out.src_kv) to_glb(A.out.src_kv)[p] = h;
    if (A.out.pinned) {
      const uint32_t ch = W.code[h];
      const bool pin = ((ch & kSegStart) && !(ch & kKeyStart)) ||
                       ((A.flags & PBL_COMPACT_ELIDE_TOMBSTONES) && is_tomb(ch & kCls) && !(ch & kStripe0));
      to_glb(A.out.pinned)[p] = pin ? 1 : 0;
    }
    to_glb(O.key_off)[p + P.q] = uint32_t(ko);
    to_glb(O.val_off)[p + P.q] = uint32_t(vo);
    // the contributors before this result, for n_src
    const uint64_t hh = W.p(kPH)[i];
    if (hh <= A.n_kv) W.cst[hh] = uint32_t(W.p(kPC)[i] - W.p(kPC)[P.kv0]);
    copy_chunks(to_glb(O.key_bytes) + (okeyb[P.q] + ko), to_glb((const uint8_t*)I.key_bytes) + (to_glb(I.blk_key_base)[P.q] + k0),
                klen);
  }
}

// Every contributing KV's value, n_src, and the kind patches.
__global__ void __launch_bounds__(kTPB) __attribute__((amdgpu_waves_per_eu(PBL_COMPACT_EMIT_WAVES)))
compact_values_kernel(Args A) {
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;  // sizes only
  const pbl_decode_out& O = A.out.result;
  const pbl_decode_out& I = A.in;
  const uint32_t lane = lane_id();
  const uint64_t n = held(A);
  const uint64_t n_items = (n + kWave - 1) / kWave;
  const uint32_t wpb = kTPB / kWave;
  for (uint64_t item = uint64_t(blockIdx.x) * wpb + wave_id(); item < n_items; item += uint64_t(gridDim.x) * wpb) {
    const uint64_t i = item * kWave + lane;
    bool ok = false;
    uint32_t vlen = 0;
    gptr<const uint8_t> vsrc = nullptr;
    gptr<uint8_t> vdst = nullptr;
    if (i < n) {
      const Place P = place_of(A, W, i);
      if (P.ok) {
        const uint32_t patch = (P.code >> kPatchShift) & 7u;
        if (patch) to_glb(O.trailer)[P.p] = (to_glb(O.trailer)[P.p] & ~0xffull) | kind_of_class(patch - 1);
        if ((P.code & kSlot) && A.out.n_src) {
          const uint64_t h = W.p(kPH)[i];
          if (h < A.n_kv) {
            const bool last = h + 1 == W.p(kPH)[P.kv1];
            const uint32_t mine = W.cst[h];
            to_glb(A.out.n_src)[P.p] = last ? uint32_t(W.p(kPC)[P.kv1] - W.p(kPC)[P.kv0]) - mine : W.cst[h + 1] - mine;
          }
        }
        if (P.code & kValue) {
          const uint64_t at = i + P.q;
          const uint32_t v0 = to_glb(I.val_off)[at];
          vlen = to_glb(I.val_off)[at + 1] - v0;
          const uint64_t x0 = to_glb(O.val_off)[P.p + P.q], x1 = to_glb(O.val_off)[P.p + P.q + 1];
          // the result's values lie in [x0, x1), oldest first: this one ends where
          // the ones after it in the source begin
          const uint64_t pin = W.p(kPV)[i] - W.p(kPV)[P.kv0] + vlen;
          const uint64_t dst = x0 + x1 - pin;
          ok = x0 <= x1 && pin >= x0 && pin <= x1 && x1 <= P.vsize && dst >= x0 && dst + vlen <= x1;
          vsrc = to_glb((const uint8_t*)I.val_bytes) + (to_glb(I.blk_val_base)[P.q] + v0);
          vdst = to_glb(O.val_bytes) + (to_glb(O.blk_val_base)[P.q] + dst);
        }
      }
    }
    result::copy_values(ok, vlen, vsrc, vdst);
  }
}

// ---- host side -----------------------------------------------------------------
constexpr uint32_t kRuleFlags = PBL_COMPACT_ELIDE_TOMBSTONES | PBL_COMPACT_BOTTOMMOST;

inline bool args_ok(const pbl_compact_in* in, const pbl_compact_out* out, uint32_t flags, uint32_t allowed, bool size_only) {
  if (!in || !out || (flags & ~allowed)) return false;
  if (in->comparer > PBL_CMP_CRDB || !result::source_ok(&in->batch)) return false;
  if (in->n_snapshots && !in->snapshots) return false;
  return result::result_ok(out->result, size_only);
}

inline int launch(const pbl_compact_in* in, pbl_compact_out* out, void* ws, uint64_t ws_bytes, uint32_t flags, bool size_only,
                  hipStream_t st) {
  const uint32_t allowed = kRuleFlags | (size_only ? 0u : uint32_t(PBL_COMPACT_SIZED));
  if (!args_ok(in, out, flags, allowed, size_only)) return PBL_INVALID_ARG;
  if (!result::ws_aligned(ws) || ws_bytes < layout(in->n_blocks, in->n_kv).size) return PBL_INVALID_ARG;
  const bool sized = (flags & PBL_COMPACT_SIZED) != 0;
  const uint32_t nb = in->n_blocks;
  const uint64_t n_kv = in->n_kv;
  Args a{};
  a.in = in->batch;
  a.out = *out;
  a.n_blocks = nb;
  a.comparer = in->comparer;
  a.size_only = size_only ? 1u : 0u;
  a.flags = flags & kRuleFlags;
  a.n_kv = n_kv;
  a.snaps = in->snapshots;
  a.n_snaps = in->n_snapshots;
  a.ws = static_cast<uint8_t*>(ws);
  const Layout L = layout(nb, n_kv);
  if (hipMemsetAsync(out->result.totals, 0, sizeof(pbl_totals), st) != hipSuccess) return PBL_DEVICE_ERROR;
  const uint32_t t_grid = uint32_t(std::min<uint64_t>(L.nt, kGrid));
  const uint32_t c_grid = uint32_t(std::min<uint64_t>(L.ntc, kGrid));
  const uint32_t q_grid = (nb + kTPB - 1) / kTPB;
  if (!sized) {
    // the header, the per-block flags and the counters
    if (hipMemsetAsync(a.ws, 0, L.qst, st) != hipSuccess) return PBL_DEVICE_ERROR;
    if (nb) {
      seek::with_cmp(in->comparer, [&](auto c) {
        hipLaunchKernelGGL((compact_classify_kernel<decltype(c)::value>), dim3(t_grid), dim3(kTPB), 0, st, a);
        return 0;
      });
      hipLaunchKernelGGL(compact_chunk_map_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_state_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_role_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_chunk_sum_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_tile_scan_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_prefix_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_persize_kernel, dim3(q_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(compact_sum_kernel, dim3(L.n_chunks), dim3(kTPB), 0, st, a);
    }
  }
  hipLaunchKernelGGL(compact_bases_kernel, dim3(L.n_chunks), dim3(kTPB), 0, st, a);
  if (!size_only && nb && out->result.key_off) {
    const uint32_t grid = std::max(n_kv ? t_grid : 1u, std::min(q_grid, kGrid));
    hipLaunchKernelGGL(compact_heads_kernel, dim3(grid), dim3(kTPB), 0, st, a);
    if (n_kv) hipLaunchKernelGGL(compact_values_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

// The sequential loop: a cursor over the block, a head at a time, each head
// walking on through its segment as the reference's setNext / mergeNext /
// singleDeleteNext / skipDueToSingleDeleteElision / deleteSizedNext do.
int batch_host(const pbl_compact_in* in, pbl_compact_out* out, uint32_t flags) {
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!args_ok(in, out, flags, kRuleFlags, false)) return PBL_INVALID_ARG;
  for (uint64_t s = 1; s < in->n_snapshots; s++)
    if (in->snapshots[s - 1] > in->snapshots[s]) return PBL_INVALID_ARG;
  const pbl_decode_out& D = in->batch;
  const pbl_decode_out& O = out->result;
  const uint32_t nb = in->n_blocks, comparer = in->comparer;
  const bool elide = (flags & PBL_COMPACT_ELIDE_TOMBSTONES) != 0, bottommost = (flags & PBL_COMPACT_BOTTOMMOST) != 0;
  pbl_seek_queries sq{};
  const K::View<R> V(D, nb, sq, nullptr, 0);

  struct Sizes {
    uint64_t n, k, v;
  };
  struct Counts {
    uint32_t miss, ineff, nondet;
  };
  std::vector<uint32_t> chain;
  auto walk = [&](uint32_t q, bool emit, uint64_t p0, Sizes* sz, Counts* cn) -> uint32_t {
    const K::Block<R> B(V, q);
    const uint64_t* tr = D.trailer + B.kv0;
    const uint32_t* vo = D.val_off + B.kv0 + q;
    const uint8_t* vb = D.val_bytes + D.blk_val_base[q];
    const uint32_t n = B.n;
    auto kind = [&](uint32_t x) { return class_of_kind(uint32_t(tr[x] & 0xff)); };
    auto stripe = [&](uint32_t x) { return stripe_of(in->snapshots, in->n_snapshots, tr[x] >> 8); };
    auto same_key = [&](uint32_t a, uint32_t b) {
      uint64_t al, bl;
      const uint8_t *ka = B.key(a, &al), *kb = B.key(b, &bl);
      return pbl::cmp::key_cmp<R>(comparer, ka, al, kb, bl) == 0;
    };
    auto vlen = [&](uint32_t x) { return uint64_t(vo[x + 1] - vo[x]); };
    auto handle = [&](uint32_t x) { return D.kv_flags && (D.kv_flags[B.kv0 + x] & kHandleBits); };
    uint64_t p = p0;
    uint32_t ko = 0, vout = 0;
    Sizes s{0, 0, 0};
    Counts c{0, 0, 0};
    // result KV from head h with this trailer; its value: none (src < 0), KV
    // src's, or the chain's, oldest first
    auto result = [&](uint32_t h, uint64_t trailer, int64_t src, const std::vector<uint32_t>* ops, bool pinned) {
      uint64_t kl;
      const uint8_t* k = B.key(h, &kl);
      uint64_t vl = 0;
      if (ops) for (uint32_t x : *ops) vl += vlen(x);
      else if (src >= 0) vl = vlen(uint32_t(src));
      if (emit) {
        const uint64_t kv = B.kv0 + h;
        O.trailer[p] = trailer;
        if (O.kv_flags) O.kv_flags[p] = D.kv_flags ? uint8_t(D.kv_flags[kv] & kHandleBits) : uint8_t(0);
        if (O.entry_off) O.entry_off[p] = D.entry_off ? D.entry_off[kv] : 0u;
        if (O.tiering_span_id) {
          O.tiering_span_id[p] = D.tiering_span_id ? D.tiering_span_id[kv] : 0ull;
          O.tiering_attr[p] = D.tiering_attr ? D.tiering_attr[kv] : 0ull;
        }
        if (out->src_kv) out->src_kv[p] = kv;
        if (out->n_src) out->n_src[p] = ops ? uint32_t(ops->size()) : 1u;
        if (out->pinned) out->pinned[p] = pinned ? 1 : 0;
        O.key_off[p + q] = ko;
        O.val_off[p + q] = vout;
        if (kl) memcpy(O.key_bytes + O.blk_key_base[q] + ko, k, kl);
        uint8_t* dst = O.val_bytes + O.blk_val_base[q] + vout;
        if (ops) {
          for (size_t x = ops->size(); x-- > 0;) {
            const uint32_t o = (*ops)[x];
            if (vlen(o)) memcpy(dst, vb + vo[o], vlen(o));
            dst += vlen(o);
          }
        } else if (vl) {
          memcpy(dst, vb + vo[src], vl);
        }
      }
      ko += uint32_t(kl);
      vout += uint32_t(vl);
      s.n++;
      s.k += kl;
      s.v += vl;
      p++;
    };
    uint32_t st = PBL_OK;
    bool unsupported = false, corrupt = false;
    uint32_t j = 0;  // the cursor: the next head
    while (j < n) {
      const uint32_t h = j;
      const uint64_t my = stripe(h);
      // whether KV x + 1 is still in this head's segment
      auto more = [&](uint32_t x) { return x + 1 < n && same_key(x, x + 1) && stripe(x + 1) == my; };
      auto past = [&](uint32_t x) {  // skipInStripe from x: the first KV after the segment
        while (more(x)) x++;
        return x + 1;
      };
      const uint32_t kd = kind(h);
      const bool tomb = is_tomb(kd);
      const bool elid = elide && my == 0;
      bool pinned = h > 0 && same_key(h - 1, h) && stripe(h - 1) != my;
      if (tomb && elide && my != 0) pinned = true;
      const uint64_t seq = tr[h] >> 8;
      const uint64_t low_seq = (bottommost && my == 0) ? 0 : seq;
      auto trailer = [](uint64_t sq, uint32_t cls) { return (sq << 8) | kind_of_class(cls); };
      // the KV after a consumed SET / MERGE
      auto after_consumed = [&](uint32_t x) {
        if (x + 1 < n && same_key(x, x + 1)) {
          const uint32_t nk = kind(x + 1);
          if (nk == kS || nk == kW || nk == kM) c.nondet++;
        }
        return x + 1;
      };
      if (kd == kD) {
        if (!elid) result(h, trailer(seq, kD), -1, nullptr, pinned);
        j = past(h);
      } else if (kd == kW) {
        result(h, trailer(low_seq, kW), h, nullptr, pinned);
        j = past(h);
      } else if (kd == kS) {
        uint32_t x = h, out_kind = kS;
        while (more(x)) {
          x++;
          if (is_tomb(kind(x))) {
            out_kind = kW;
            break;
          }
        }
        result(h, trailer(low_seq, out_kind), h, nullptr, pinned);
        j = past(x);
      } else if (kd == kM) {
        chain.clear();
        chain.push_back(h);
        uint32_t x = h, out_kind = (bottommost && my == 0) ? uint32_t(kS) : uint32_t(kM);
        while (more(x)) {
          x++;
          const uint32_t k = kind(x);
          if (is_tomb(k)) {
            out_kind = kW;
            break;
          }
          chain.push_back(x);
          if (k != kM) {
            out_kind = kS;
            break;
          }
        }
        if (chain.size() > 1)
          for (uint32_t o : chain)
            if (handle(o)) unsupported = true;
        result(h, trailer(low_seq, out_kind), -1, &chain, pinned);
        j = past(x);
      } else if (kd == kX) {
        uint32_t x = h;
        for (;;) {
          if (!more(x)) {  // the segment ends on a pending SINGLEDEL
            if (elid) c.ineff++;
            else result(h, trailer(seq, kX), -1, nullptr, pinned);
            j = x + 1;
            break;
          }
          x++;
          const uint32_t k = kind(x);
          if (k == kX) {
            c.ineff++;
            continue;
          }
          if (k == kS || k == kM) {
            j = after_consumed(x);
            break;
          }
          if (k != kW) c.ineff++;
          if (!elid) result(h, trailer(seq, kD), -1, nullptr, pinned);
          j = past(x);
          break;
        }
      } else if (kd == kZ) {
        if (elid) {
          j = past(h);
          continue;
        }
        int64_t holder = vlen(h) ? int64_t(h) : -1;  // the KV whose value is held, or none
        uint32_t x = h, out_kind = kZ;
        while (more(x)) {
          x++;
          const uint32_t k = kind(x);
          uint64_t expected = 0;
          if (holder >= 0 && !uvarint_exact(vb + vo[holder], vlen(uint32_t(holder)), &expected)) {
            corrupt = true;  // (the block's status; the walk goes on for the precedence of the statuses)
            expected = ~0ull;
          }
          if (is_tomb(k)) {
            if (holder >= 0) c.miss++;
            holder = (k == kZ && vlen(x)) ? int64_t(x) : -1;
            if (k != kZ) {
              out_kind = kD;
              break;
            }
          } else if (holder < 0) {
            out_kind = kD;
            break;
          } else {
            uint64_t kl;
            B.key(x, &kl);
            holder = -1;
            if (kl + vlen(x) != expected) {
              c.miss++;
              out_kind = kD;
              break;
            }
          }
        }
        result(h, trailer(seq, out_kind), holder, nullptr, pinned);
        j = past(x);
      } else {
        unsupported = true;
        j++;
      }
    }
    if (unsupported) st = PBL_UNSUPPORTED;
    else if (corrupt) st = PBL_CORRUPT_BOUNDS;
    if (st == PBL_OK && (s.n > kMaxKvs || s.k > kMaxBytes || s.v > kMaxBytes)) st = PBL_UNSUPPORTED;
    if (emit) {
      O.key_off[p + q] = ko;
      O.val_off[p + q] = vout;
    }
    *sz = s;
    *cn = c;
    return st;
  };

  std::vector<uint32_t> status(nb);
  pbl_totals T{};
  uint64_t kvb = 0, keyb = 0, valb = 0;
  K::with_cmp(comparer, [&](auto c) {
    constexpr uint32_t kCmp = decltype(c)::value;
    for (uint32_t q = 0; q < nb; q++) {
      uint32_t st = D.blk_status[q];
      Sizes s{0, 0, 0};
      Counts cn{0, 0, 0};
      if (st == PBL_OK) {
        const K::Block<R> B(V, q);
        const uint64_t* tr = D.trailer + B.kv0;
        bool order = true, kinds = true;
        for (uint32_t j = 0; j < B.n; j++) {
          if (class_of_kind(uint32_t(tr[j] & 0xff)) == kNoClass || (D.kv_flags && (D.kv_flags[B.kv0 + j] & PBL_KV_INVALID_KEY)))
            kinds = false;
          if (j + 1 < B.n) {
            uint64_t al, bl;
            const uint8_t *a = B.key(j, &al), *b = B.key(j + 1, &bl);
            const int k = pbl::cmp::key_cmp<R>(kCmp, a, al, b, bl);
            if (k > 0 || (k == 0 && (tr[j] >> 8) <= (tr[j + 1] >> 8))) order = false;
          }
        }
        if (!order) st = PBL_INVALID_ARG;
        else if (!kinds) st = PBL_UNSUPPORTED;
        else st = walk(q, false, 0, &s, &cn);
      }
      if (st != PBL_OK) {
        s = Sizes{0, 0, 0};
        cn = Counts{0, 0, 0};
        T.status_mask |= 1u << st;
        T.n_bad_blocks++;
      }
      status[q] = st;
      if (out->n_missized) out->n_missized[q] = cn.miss;
      if (out->n_ineffectual) out->n_ineffectual[q] = cn.ineff;
      if (out->n_nondeterministic) out->n_nondeterministic[q] = cn.nondet;
      O.blk_kv_base[q] = kvb;
      O.blk_key_base[q] = keyb;
      O.blk_val_base[q] = valb;
      if (O.blk_rst_base) O.blk_rst_base[q] = 0;
      O.blk_status[q] = st;
      kvb += s.n;
      keyb += s.k;
      valb += s.v;
    }
    return 0;
  });
  O.blk_kv_base[nb] = kvb;
  O.blk_key_base[nb] = keyb;
  O.blk_val_base[nb] = valb;
  if (O.blk_rst_base) O.blk_rst_base[nb] = 0;
  T.n_kv = kvb;
  T.key_bytes = keyb;
  T.val_bytes = valb;
  const bool over = kvb > O.kv_cap || keyb > O.key_cap || valb > O.val_cap;
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *O.totals = T;
  if (over || !O.key_off) return PBL_OK;

  for (uint32_t q = 0; q < nb; q++) {
    Sizes s;
    Counts cn;
    if (status[q] == PBL_OK) {
      walk(q, true, O.blk_kv_base[q], &s, &cn);
    } else {
      O.key_off[O.blk_kv_base[q] + q] = 0;
      O.val_off[O.blk_kv_base[q] + q] = 0;
    }
  }
  return PBL_OK;
}

}  // namespace compact
}  // namespace pbl

extern "C" {

uint64_t pbl_compact_workspace_bytes(uint32_t n_blocks, uint64_t n_kv) {
  return pbl::compact::layout(n_blocks, n_kv).size;
}

int pbl_compact_size(const pbl_compact_in* in, pbl_compact_out* out, void* workspace, uint64_t workspace_bytes,
                     uint32_t flags, void* stream) {
  return pbl::compact::launch(in, out, workspace, workspace_bytes, flags, true, reinterpret_cast<hipStream_t>(stream));
}

int pbl_compact_batch(const pbl_compact_in* in, pbl_compact_out* out, void* workspace, uint64_t workspace_bytes,
                      uint32_t flags, void* stream) {
  return pbl::compact::launch(in, out, workspace, workspace_bytes, flags, false, reinterpret_cast<hipStream_t>(stream));
}

int pbl_compact_batch_host(const pbl_compact_in* in, pbl_compact_out* out, uint32_t flags) {
  return pbl::compact::batch_host(in, out, flags);
}

size_t pbl_compact_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_compact_in), PBL_OFF(pbl_compact_in, batch), PBL_OFF(pbl_compact_in, n_blocks),
      PBL_OFF(pbl_compact_in, comparer), PBL_OFF(pbl_compact_in, n_kv), PBL_OFF(pbl_compact_in, snapshots),
      PBL_OFF(pbl_compact_in, n_snapshots),
      sizeof(pbl_compact_out), PBL_OFF(pbl_compact_out, result), PBL_OFF(pbl_compact_out, src_kv),
      PBL_OFF(pbl_compact_out, n_src), PBL_OFF(pbl_compact_out, pinned), PBL_OFF(pbl_compact_out, n_missized),
      PBL_OFF(pbl_compact_out, n_ineffectual), PBL_OFF(pbl_compact_out, n_nondeterministic)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
