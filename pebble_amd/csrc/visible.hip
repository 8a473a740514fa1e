// visible.hip — the snapshot-visible view of a sorted decoded batch, on the
// device: result block q is what Iterator.First(); Next()...
// returns over block q's KVs as the point-key stream, with DefaultMerger
// (iterator.go:649-664, 1239-1305; include/pebble_amd.h states the rules).
//
// A KV's role -- result head, operand of a MERGE chain, or nothing -- depends on
// every KV before it in its group of equal user keys, and a group may be of any
// length.  Each KV is therefore a map on the states {seeking, merging, merging
// under a head whose value is a handle, done}: 4 -> 4, eight bits.  (The issue's
// sketch has three states; the fourth carries the one fact about the head that
// the "no handle inside a folded chain" rule needs, so that no lane looks back.)
// Invisible KVs are the identity, a group's first KV first resets to seeking,
// and composition is associative: a scan of the maps over the flat KV index
// gives every KV its incoming state.  Nothing below loops over a group.
//
//   visible_classify_kernel<comparer>  tile of 256 source KVs per workgroup: a
//       lane compares its KV with the successor (sortedness, and whether the
//       successor starts a group), checks kind and flags, writes the KV's class
//       and block; the tile's composed map.  Instantiated on "has cover": with
//       the per-KV cover of rangedel.hip (the _rd entry points)
//       a KV under a newer range tombstone is invisible too
//   visible_chunk_map_kernel / visible_state_kernel  every tile's incoming
//       state: the scan of the tile maps in the chunked two-launch form (chunks
//       of 256 tiles; a chunk composes the maps of the chunks before it in order)
//   visible_role_kernel  per tile: the scan of the maps inside the tile gives
//       the roles; the tile's sums of {heads, contributors, key bytes, value bytes}
//   visible_chunk_sum_kernel / visible_tile_scan_kernel  the exclusive scan of
//       those sums over tiles, in the same two-launch form
//   visible_prefix_kernel  per tile: the four exclusive prefixes of every KV
//   visible_persize_kernel  lane per block: status, and sizes as differences of
//       the prefixes at the block's two ends
//   visible_sum_kernel / visible_bases_kernel  the exclusive scan over result
//       blocks (result_core.hip.h's chunk_sums / bases): bases, statuses,
//       totals, capacity
//   visible_heads_kernel  wave per 64 source KVs: a KV that is a result writes
//       its per-KV arrays (result_core.hip.h's copy_kv_arrays, flags masked to
//       the handle bits), offsets and key; every block's last offset
//   visible_values_kernel  wave per 64 source KVs: every contributing KV copies
//       its value to X[r] + X[r+1] - P[i] (X: the result's value offsets, P: the
//       inclusive value prefix), so a chain's oldest operand comes first and no
//       lane looks for its chain's end; n_src from the heads' contributor counts.
//       The copy itself is result_core.hip.h's copy_values.
//
// The cross-tile steps use the two-launch chunk form of the scans over blocks
// rather than result_core.hip.h's one workgroup over all tiles (measured first in
// that form: 76 + 182 us of a 500 us size call at 17 K tiles).  The maps do not
// commute, so where the sums add the earlier chunks' totals in any order, the
// state kernel scans them in order, 256 chunks (16.7 M KVs) per step.
//
// Both emit kernels check what they read from the workspace against the source
// block and the result block's recorded sizes: no input, and no stale
// workspace, leads outside the arrays.
//
// pbl_visible_batch_host is the sequential state machine over the same
// comparers, a different algorithm on purpose (batch_host<has cover>).
#include <algorithm>
#include <vector>

#include "result_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace visible {

constexpr uint64_t kHdr = 64;
constexpr uint32_t kTileShift = 8, kTile = 1u << kTileShift;  // source KVs per tile
constexpr int kTPB = 256;
constexpr uint32_t kChunk = 256;  // result blocks per chunk of the scan over blocks
static_assert(kTPB == result::kTPB && kChunk == uint32_t(result::kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kGrid = 2048;  // workgroups of a grid-striding kernel, at most
constexpr uint64_t kMaxBytes = 0xffffffffull;
constexpr uint64_t kMaxKvs = 0xffffffffull;
enum { kHSkip = 0 };  // header word 0: nonzero = sizes only

// InternalKeyKind (internal/base/internal.go:29-130)
constexpr uint32_t kKindDel = 0, kKindSet = 1, kKindMerge = 2, kKindSingleDel = 7, kKindSetWithDel = 18,
                   kKindDelSized = 23;
// classes of a KV, bits 0-1 of its code byte
enum : uint32_t { kNone = 0, kDel = 1, kSet = 2, kMerge = 3 };
constexpr uint32_t kCodeHead = 4, kCodeHandle = 8;  // starts a group; its value is a handle
// after visible_role_kernel the code byte's bits 0-1 are the role
enum : uint32_t { kRoleNone = 0, kRoleHead = 1, kRoleOperand = 2 };
// bits of the per-block flag word
constexpr uint32_t kBadOrder = 1, kBadKind = 2;
constexpr uint32_t kHandleBits = PBL_KV_VALBLK_HANDLE | PBL_KV_BLOB_HANDLE;

// states: 0 seeking, 1 merging, 2 merging under a handle head, 3 done; a map
// holds the image of state s in bits 2s, 2s+1
constexpr uint32_t kIdentity = 0xE4u;
PBL_HD inline uint32_t map_apply(uint32_t m, uint32_t s) { return (m >> (2 * s)) & 3u; }
PBL_HD inline uint32_t map_then(uint32_t a, uint32_t b) {  // a, then b
  uint32_t r = 0;
  for (uint32_t s = 0; s < 4; s++) r |= map_apply(b, map_apply(a, s)) << (2 * s);
  return r;
}
PBL_HD inline uint32_t map_of(uint32_t code) {
  const uint32_t cls = code & 3u;
  uint32_t m = cls == kNone ? kIdentity : cls == kMerge ? (kIdentity | ((code & kCodeHandle) ? 2u : 1u)) : 0xFFu;
  if (code & kCodeHead) m = map_apply(m, 0) * 0x55u;
  return m;
}
PBL_HD inline bool is_visible(uint64_t trailer, uint64_t snapshot) {
  return snapshot >= PBL_SEQNUM_MAX || (trailer >> 8) < snapshot;
}
// class of a KV by its kind; *ok = one of the six kinds
PBL_HD inline uint32_t kind_class(uint64_t trailer, bool* ok) {
  const uint32_t k = uint32_t(trailer & 0xff);
  *ok = true;
  if (k == kKindSet || k == kKindSetWithDel) return kSet;
  if (k == kKindMerge) return kMerge;
  if (k == kKindDel || k == kKindSingleDel || k == kKindDelSized) return kDel;
  *ok = false;
  return kNone;
}

struct Layout {
  uint64_t nt;  // tiles (n_kv / 256 + 1)
  uint64_t ntc;  // chunks of 256 tiles
  uint64_t bad, qst, q64, csum, tmap, tin, tsum, tcs, tcm, code, blk, cst, pre, size;
  uint32_t n_chunks;
};
__host__ __device__ inline Layout layout(uint32_t nb, uint64_t n_kv) {
  Layout L;
  L.nt = (n_kv >> kTileShift) + 1;
  L.ntc = (L.nt + kChunk - 1) / kChunk;
  L.n_chunks = nb ? (nb + kChunk - 1) / kChunk : 1;
  uint64_t o = kHdr;
  L.bad = o;  o += 4ull * nb;
  L.qst = o;  o += 4ull * nb;
  o = (o + 15) & ~uint64_t(15);
  L.q64 = o;  o += 3ull * 8 * (uint64_t(nb) + 1);
  L.csum = o; o += 3ull * 8 * L.n_chunks;
  L.tsum = o; o += 4ull * 8 * L.nt;
  L.tcs = o;  o += 4ull * 8 * L.ntc;
  L.pre = o;  o += 4ull * 8 * (n_kv + 1);
  L.tmap = o; o += 4ull * L.nt;
  L.tin = o;  o += 4ull * L.nt;
  L.tcm = o;  o += 4ull * L.ntc;
  L.blk = o;  o += 4ull * n_kv;
  L.cst = o;  o += 4ull * (n_kv + 1);
  L.code = o; o += n_kv;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

// ---- device side ---------------------------------------------------------------
struct Args {
  pbl_decode_out in;
  pbl_visible_out out;
  uint32_t n_blocks, comparer, size_only, keep;
  uint64_t n_kv;  // the batch's KVs, as the workspace was sized
  uint64_t snapshot;
  uint8_t* ws;
  const uint64_t* cover;  // [n_kv] per KV: the newest visible range tombstone over its key (rangedel.hip), or NULL
};

struct Ws {
  gptr<uint32_t> hdr, bad, qst, tmap, tin, tcm, blk, cst;
  gptr<uint64_t> q64, csum, tsum, tcs, pre;
  gptr<uint8_t> code;
  uint64_t nt, ntc, qs, ps;
  uint32_t n_chunks;
  __device__ Ws(uint8_t* ws, uint32_t nb, uint64_t n_kv) {
    const Layout L = layout(nb, n_kv);
    hdr = to_glb(reinterpret_cast<uint32_t*>(ws));
    bad = to_glb(reinterpret_cast<uint32_t*>(ws + L.bad));
    qst = to_glb(reinterpret_cast<uint32_t*>(ws + L.qst));
    q64 = to_glb(reinterpret_cast<uint64_t*>(ws + L.q64));
    csum = to_glb(reinterpret_cast<uint64_t*>(ws + L.csum));
    tsum = to_glb(reinterpret_cast<uint64_t*>(ws + L.tsum));
    pre = to_glb(reinterpret_cast<uint64_t*>(ws + L.pre));
    tmap = to_glb(reinterpret_cast<uint32_t*>(ws + L.tmap));
    tin = to_glb(reinterpret_cast<uint32_t*>(ws + L.tin));
    tcm = to_glb(reinterpret_cast<uint32_t*>(ws + L.tcm));
    tcs = to_glb(reinterpret_cast<uint64_t*>(ws + L.tcs));
    blk = to_glb(reinterpret_cast<uint32_t*>(ws + L.blk));
    cst = to_glb(reinterpret_cast<uint32_t*>(ws + L.cst));
    code = to_glb(ws + L.code);
    nt = L.nt;
    ntc = L.ntc;
    qs = uint64_t(nb) + 1;
    ps = n_kv + 1;
    n_chunks = L.n_chunks;
  }
  __device__ gptr<uint64_t> q(int c) const { return q64 + uint64_t(c) * qs; }   // per-block KVs, key bytes, value bytes
  __device__ result::Sizes sizes() const { return result::Sizes{q64, csum, qst, qs, n_chunks}; }
  __device__ gptr<uint64_t> ts(int c) const { return tsum + uint64_t(c) * nt; }  // per-tile sums
  // per-KV exclusive prefixes (n_kv + 1 entries each): 0 heads, 1 contributors, 2 key bytes, 3 value bytes
  __device__ gptr<uint64_t> p(int c) const { return pre + uint64_t(c) * ps; }
};
enum { kPH = 0, kPC = 1, kPK = 2, kPV = 3 };

// The KVs the batch holds; more than the workspace was sized for: not described.
__device__ inline uint64_t held(const Args& A) { return A.n_blocks ? to_glb(A.in.blk_kv_base)[A.n_blocks] : 0; }
__device__ inline bool described(const Args& A) { return held(A) <= A.n_kv; }

using result::block_excl_scan64;
using result::block_of;
using result::block_sum64;

// block_excl_scan64 for maps under map_then: the composition of the maps of the threads
// before this one (the identity for thread 0); *total = all 256.  `lds`: 4 words.
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

using GR = seek::GlobalReader;

__device__ inline seek::View<GR> in_view(const Args& A) {
  pbl_seek_queries sq{};
  return seek::View<GR>(A.in, A.n_blocks, sq, nullptr, 0);
}

// kCover: the batch comes with a cover (the _rd entry points); a KV under a newer
// range tombstone is invisible like one at or above the snapshot.
template <uint32_t kCmp, bool kCover>
__global__ __launch_bounds__(kTPB) void visible_classify_kernel(Args A) {
  __shared__ uint32_t lds[4];
  __shared__ uint32_t next_head[kTile];  // whether the KV after this thread's starts a group
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint32_t nb = A.n_blocks;
  const uint64_t n = held(A);
  const seek::View<GR> V = in_view(A);
  const gptr<const uint64_t> tr = to_glb((const uint64_t*)A.in.trailer);
  const gptr<const uint8_t> fl = to_glb((const uint8_t*)A.in.kv_flags);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    uint32_t code = kNone | kCodeHead, nh = 1;
    bool first_of_block = true;
    if (i < n) {
      const uint32_t q = block_of(V.blk_kv_base, nb, i);
      W.blk[i] = q;
      const seek::Block<GR> B(V, q);
      if (V.blk_status[q] == PBL_OK && i >= B.kv0 && i - B.kv0 < B.n) {
        const uint32_t j = uint32_t(i - B.kv0);
        const uint64_t ti = tr[i];
        const uint32_t f = fl ? fl[i] : 0u;
        bool kind_ok;
        uint32_t cls = kind_class(ti, &kind_ok);
        uint32_t badw = (kind_ok && !(f & PBL_KV_INVALID_KEY)) ? 0u : kBadKind;
        if (!is_visible(ti, A.snapshot)) cls = kNone;
        if constexpr (kCover) {
          if (to_glb(A.cover)[i] > (ti >> 8)) cls = kNone;
        }
        code = cls | ((f & kHandleBits) ? kCodeHandle : 0u);
        first_of_block = j == 0;
        if (j + 1 < B.n) {
          uint64_t al, bl;
          const cmp::kptr<GR> a = B.key(j, &al), b = B.key(j + 1, &bl);
          const int c = cmp::key_cmp<GR>(kCmp, a, al, b, bl);
          nh = c != 0;
          if (c > 0 || (c == 0 && ti < tr[i + 1])) badw |= kBadOrder;
        }
        if (threadIdx.x == 0 && j > 0) {  // the tile's first KV looks back once
          uint64_t al, bl;
          const cmp::kptr<GR> a = B.key(j - 1, &al), b = B.key(j, &bl);
          if (cmp::key_cmp<GR>(kCmp, a, al, b, bl) != 0) code |= kCodeHead;
        }
        if (badw) g_atomic_or((uint32_t*)(W.bad + q), badw);
      }
    }
    __syncthreads();
    next_head[threadIdx.x] = nh;
    __syncthreads();
    if (first_of_block || (threadIdx.x > 0 && next_head[threadIdx.x - 1])) code |= kCodeHead;
    if (i < n) W.code[i] = uint8_t(code);
    uint32_t total;
    block_excl_scan_map(i < n ? map_of(code) : kIdentity, lds, &total);
    if (threadIdx.x == 0) W.tmap[t] = total;
  }
}

// Per chunk of kChunk tiles: the composition of its tiles' maps.
__global__ __launch_bounds__(kTPB) void visible_chunk_map_kernel(Args A) {
  __shared__ uint32_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  for (uint64_t c = blockIdx.x; c < W.ntc; c += gridDim.x) {
    const uint64_t t = c * kChunk + threadIdx.x;
    uint32_t total;
    block_excl_scan_map(t < W.nt ? W.tmap[t] : kIdentity, lds, &total);
    if (threadIdx.x == 0) W.tcm[c] = total;
  }
}

// Every tile's incoming state: the chunks before this one composed in order
// (from "seeking"), then the scan inside the chunk.
__global__ __launch_bounds__(kTPB) void visible_state_kernel(Args A) {
  __shared__ uint32_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  for (uint64_t c = blockIdx.x; c < W.ntc; c += gridDim.x) {
    uint32_t carry = 0;
    for (uint64_t c0 = 0; c0 < c; c0 += kTPB) {
      uint32_t total;
      block_excl_scan_map(c0 + threadIdx.x < c ? W.tcm[c0 + threadIdx.x] : kIdentity, lds, &total);
      carry = map_apply(total, carry);
    }
    const uint64_t t = c * kChunk + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_excl_scan_map(t < W.nt ? W.tmap[t] : kIdentity, lds, &total);
    if (t < W.nt) W.tin[t] = map_apply(ex, carry);
  }
}

// What a KV with this role adds to {heads, contributors, key bytes, value bytes}.
__device__ inline void contribution(const Args& A, const Ws& W, uint64_t i, uint32_t role, uint64_t* v) {
  v[kPH] = role == kRoleHead;
  v[kPC] = role != kRoleNone;
  v[kPK] = v[kPV] = 0;
  if (role == kRoleNone) return;
  const uint64_t at = i + W.blk[i];
  v[kPV] = to_glb(A.in.val_off)[at + 1] - to_glb(A.in.val_off)[at];
  if (A.keep || role == kRoleHead) v[kPK] = to_glb(A.in.key_off)[at + 1] - to_glb(A.in.key_off)[at];
}

__global__ __launch_bounds__(kTPB) void visible_role_kernel(Args A) {
  __shared__ uint32_t lds32[4];
  __shared__ uint64_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint64_t n = held(A);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    const uint32_t code = i < n ? W.code[i] : uint32_t(kNone | kCodeHead);
    uint32_t total;
    const uint32_t ex = block_excl_scan_map(i < n ? map_of(code) : kIdentity, lds32, &total);
    const uint32_t s = (code & kCodeHead) ? 0u : map_apply(ex, W.tin[t]);
    const uint32_t cls = code & 3u;
    const uint32_t role = (cls == kSet || cls == kMerge) ? (s == 0 ? kRoleHead : s == 3 ? kRoleNone : kRoleOperand) : kRoleNone;
    uint64_t v[4] = {0, 0, 0, 0};
    if (i < n) {
      // folded, a chain of more than one operand must hold no handle
      if (!A.keep && role == kRoleOperand && (s == 2 || (code & kCodeHandle))) g_atomic_or((uint32_t*)(W.bad + W.blk[i]), kBadKind);
      W.code[i] = uint8_t((code & ~3u) | role);
      contribution(A, W, i, role, v);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint64_t sum = block_sum64(v[c], lds);
      if (threadIdx.x == 0) W.ts(c)[t] = sum;
    }
  }
}

// Per chunk of kChunk tiles: the sums of the tiles' four sums.
__global__ __launch_bounds__(kTPB) void visible_chunk_sum_kernel(Args A) {
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

// The exclusive scan over tiles, in place (a chunk writes its own tiles only).
__global__ __launch_bounds__(kTPB) void visible_tile_scan_kernel(Args A) {
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

__global__ __launch_bounds__(kTPB) void visible_prefix_kernel(Args A) {
  __shared__ uint64_t lds[4];
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint64_t n = held(A);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    uint64_t v[4] = {0, 0, 0, 0};
    if (i < n) contribution(A, W, i, W.code[i] & 3u, v);
#pragma unroll
    for (int c = 0; c < 4; c++) {
      uint64_t tot;
      const uint64_t ex = W.ts(c)[t] + block_excl_scan64(v[c], lds, &tot);
      if (i <= n) W.p(c)[i] = ex;  // (entry n: the totals)
    }
  }
}

// Lane per block: its status (the input's; out of order; a kind, a flag or a
// handle this stage does not take; sizes past the u32 offsets) and sizes.
__global__ __launch_bounds__(kTPB) void visible_persize_kernel(Args A) {
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
    else {
      const int pr = A.keep ? kPC : kPH;
      n = W.p(pr)[b] - W.p(pr)[a];
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

// Per chunk of kChunk result blocks: the sums of {KVs, key bytes, value bytes}.
__global__ __launch_bounds__(kTPB) void visible_sum_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  result::chunk_sums<3>(W.sizes(), A.n_blocks, lds);
}

// The result's bases, statuses and totals; the capacity check (the last chunk).
// Totals were zeroed by the entry point.
__global__ __launch_bounds__(kTPB) void visible_bases_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  uint64_t ex[3], end[3];
  bool over;
  if (result::bases<3>(W.sizes(), A.out.result, A.n_blocks, A.size_only != 0, lds, ex, end, &over))
    W.hdr[kHSkip] = (over || !described(A)) ? 1u : 0u;
}

// A source KV and the place of what it contributes to.
struct Place {
  bool ok;
  uint32_t q, role;
  uint64_t kv0, kv1;  // the source block
  uint64_t p;         // the result KV, global
  uint64_t ksize, vsize;  // the result block's bytes
};
// i < held.  Everything read from the workspace is checked against the source
// block and the result block's sizes.
__device__ inline Place place_of(const Args& A, const Ws& W, uint64_t i) {
  const pbl_decode_out& O = A.out.result;
  Place P{};
  P.role = W.code[i] & 3u;
  P.q = W.blk[i];
  if (P.role == kRoleNone || P.role > kRoleOperand || P.q >= A.n_blocks) return P;
  if (to_glb(O.blk_status)[P.q] != PBL_OK) return P;
  P.kv0 = to_glb(A.in.blk_kv_base)[P.q];
  P.kv1 = to_glb(A.in.blk_kv_base)[P.q + 1];
  if (i < P.kv0 || i >= P.kv1 || P.kv1 > A.n_kv) return P;
  const int pr = A.keep ? kPC : kPH;
  uint64_t r = W.p(pr)[i] - W.p(pr)[P.kv0];
  if (!A.keep && P.role == kRoleOperand) r -= 1;  // its chain's head
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

#ifndef PBL_VISIBLE_EMIT_WAVES
#define PBL_VISIBLE_EMIT_WAVES 5  // as every caller of result::copy_values
#endif
// Every result KV's arrays, offsets and key; every block's last offset.
__global__ void __launch_bounds__(kTPB) __attribute__((amdgpu_waves_per_eu(PBL_VISIBLE_EMIT_WAVES)))
visible_heads_kernel(Args A) {
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
    if (!P.ok) continue;
    const bool head = P.role == kRoleHead;
    if (!head && !A.keep) continue;
    const uint64_t at = i + P.q;
    const uint32_t k0 = to_glb(I.key_off)[at], klen = to_glb(I.key_off)[at + 1] - k0;
    const uint64_t ko = W.p(kPK)[i] - W.p(kPK)[P.kv0], vo = W.p(kPV)[i] - W.p(kPV)[P.kv0];
    if (ko + klen > P.ksize || vo > P.vsize) continue;
    const uint64_t p = P.p;
    result::copy_kv_arrays(O, p, I, i, uint8_t(kHandleBits), true);
    if (A.out.src_kv) to_glb(A.out.src_kv)[p] = i;
    to_glb(O.key_off)[p + P.q] = uint32_t(ko);
    to_glb(O.val_off)[p + P.q] = uint32_t(vo);
    // the contributors before this head, for n_src
    const uint64_t h = W.p(kPH)[i];
    if (head && h <= A.n_kv) W.cst[h] = uint32_t(W.p(kPC)[i] - W.p(kPC)[P.kv0]);
    copy_chunks(to_glb(O.key_bytes) + (okeyb[P.q] + ko), to_glb((const uint8_t*)I.key_bytes) + (to_glb(I.blk_key_base)[P.q] + k0),
                klen);
  }
}

// Every contributing KV's value, and n_src.
__global__ void __launch_bounds__(kTPB) __attribute__((amdgpu_waves_per_eu(PBL_VISIBLE_EMIT_WAVES)))
visible_values_kernel(Args A) {
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
        const uint64_t at = i + P.q;
        const uint32_t v0 = to_glb(I.val_off)[at];
        vlen = to_glb(I.val_off)[at + 1] - v0;
        const uint64_t x0 = to_glb(O.val_off)[P.p + P.q], x1 = to_glb(O.val_off)[P.p + P.q + 1];
        uint64_t dst = x0;
        if (!A.keep) {
          // the chain's values lie in [x0, x1), oldest first: this one ends where
          // the ones after it in the source begin
          const uint64_t pin = W.p(kPV)[i] - W.p(kPV)[P.kv0] + vlen;
          dst = x0 + x1 - pin;
          ok = x0 <= x1 && pin >= x0 && pin <= x1;
        } else {
          ok = x0 <= x1;
        }
        ok = ok && x1 <= P.vsize && dst >= x0 && dst + vlen <= x1;
        vsrc = to_glb((const uint8_t*)I.val_bytes) + (to_glb(I.blk_val_base)[P.q] + v0);
        vdst = to_glb(O.val_bytes) + (to_glb(O.blk_val_base)[P.q] + dst);
        if (ok && A.out.n_src) {
          const uint64_t h = W.p(kPH)[i];
          if (P.role == kRoleHead && h < A.n_kv) {
            const bool last = h + 1 == W.p(kPH)[P.kv1];
            const uint32_t mine = W.cst[h];
            to_glb(A.out.n_src)[P.p] = last ? uint32_t(W.p(kPC)[P.kv1] - W.p(kPC)[P.kv0]) - mine : W.cst[h + 1] - mine;
          } else if (A.keep) {
            to_glb(A.out.n_src)[P.p] = 0u;
          }
        }
      }
    }
    result::copy_values(ok, vlen, vsrc, vdst);
  }
}

// ---- host side -----------------------------------------------------------------
// Argument checks shared by the device and the host entry points.
inline bool args_ok(const pbl_visible_in* in, const pbl_visible_out* out, uint32_t flags, uint32_t allowed, bool size_only) {
  if (!in || !out || (flags & ~allowed)) return false;
  if (in->comparer > PBL_CMP_CRDB || !result::source_ok(&in->batch)) return false;
  return result::result_ok(out->result, size_only);
}
inline bool ws_ok(const void* ws, uint64_t bytes, uint32_t nb, uint64_t n_kv) {
  return result::ws_aligned(ws) && bytes >= layout(nb, n_kv).size;
}

inline int launch(const pbl_visible_in* in, pbl_visible_out* out, void* ws, uint64_t ws_bytes, uint32_t flags,
                  bool size_only, const uint64_t* cover, hipStream_t st) {
  const uint32_t allowed = PBL_VISIBLE_KEEP_OPERANDS | (size_only ? 0u : uint32_t(PBL_VISIBLE_SIZED));
  if (!args_ok(in, out, flags, allowed, size_only) || !ws_ok(ws, ws_bytes, in->n_blocks, in->n_kv)) return PBL_INVALID_ARG;
  const bool sized = (flags & PBL_VISIBLE_SIZED) != 0;
  const uint32_t nb = in->n_blocks;
  const uint64_t n_kv = in->n_kv;
  Args a{};
  a.in = in->batch;
  a.out = *out;
  a.n_blocks = nb;
  a.comparer = in->comparer;
  a.size_only = size_only ? 1u : 0u;
  a.keep = (flags & PBL_VISIBLE_KEEP_OPERANDS) ? 1u : 0u;
  a.n_kv = n_kv;
  a.snapshot = in->snapshot;
  a.ws = static_cast<uint8_t*>(ws);
  a.cover = cover;
  const Layout L = layout(nb, n_kv);
  if (hipMemsetAsync(out->result.totals, 0, sizeof(pbl_totals), st) != hipSuccess) return PBL_DEVICE_ERROR;
  const uint32_t t_grid = uint32_t(std::min<uint64_t>(L.nt, kGrid));
  const uint32_t c_grid = uint32_t(std::min<uint64_t>(L.ntc, kGrid));
  const uint32_t q_grid = (nb + kTPB - 1) / kTPB;
  if (!sized) {
    // the header and the per-block flags
    if (hipMemsetAsync(a.ws, 0, L.qst, st) != hipSuccess) return PBL_DEVICE_ERROR;
    if (nb) {
      seek::with_cmp(in->comparer, [&](auto c) {
        if (cover) hipLaunchKernelGGL((visible_classify_kernel<decltype(c)::value, true>), dim3(t_grid), dim3(kTPB), 0, st, a);
        else hipLaunchKernelGGL((visible_classify_kernel<decltype(c)::value, false>), dim3(t_grid), dim3(kTPB), 0, st, a);
        return 0;
      });
      hipLaunchKernelGGL(visible_chunk_map_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_state_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_role_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_chunk_sum_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_tile_scan_kernel, dim3(c_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_prefix_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_persize_kernel, dim3(q_grid), dim3(kTPB), 0, st, a);
      hipLaunchKernelGGL(visible_sum_kernel, dim3(L.n_chunks), dim3(kTPB), 0, st, a);
    }
  }
  hipLaunchKernelGGL(visible_bases_kernel, dim3(L.n_chunks), dim3(kTPB), 0, st, a);
  if (!size_only && nb && out->result.key_off) {
    const uint32_t grid = std::max(n_kv ? t_grid : 1u, std::min(q_grid, kGrid));
    hipLaunchKernelGGL(visible_heads_kernel, dim3(grid), dim3(kTPB), 0, st, a);
    if (n_kv) hipLaunchKernelGGL(visible_values_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

// The sequential state machine; kCover: with the per-KV cover of rangedel.hip.
template <bool kCover>
int batch_host(const pbl_visible_in* in, pbl_visible_out* out, uint32_t flags, const uint64_t* cover);

}  // namespace visible
}  // namespace pbl

extern "C" {

uint64_t pbl_visible_workspace_bytes(uint32_t n_blocks, uint64_t n_kv) {
  return pbl::visible::layout(n_blocks, n_kv).size;
}

int pbl_visible_size(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                     uint32_t flags, void* stream) {
  return pbl::visible::launch(in, out, workspace, workspace_bytes, flags, true, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int pbl_visible_batch(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                      uint32_t flags, void* stream) {
  return pbl::visible::launch(in, out, workspace, workspace_bytes, flags, false, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int pbl_visible_size_rd(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                        uint32_t flags, const uint64_t* cover_seq, void* stream) {
  return pbl::visible::launch(in, out, workspace, workspace_bytes, flags, true, cover_seq, reinterpret_cast<hipStream_t>(stream));
}

int pbl_visible_batch_rd(const pbl_visible_in* in, pbl_visible_out* out, void* workspace, uint64_t workspace_bytes,
                         uint32_t flags, const uint64_t* cover_seq, void* stream) {
  return pbl::visible::launch(in, out, workspace, workspace_bytes, flags, false, cover_seq, reinterpret_cast<hipStream_t>(stream));
}

int pbl_visible_batch_host(const pbl_visible_in* in, pbl_visible_out* out, uint32_t flags) {
  return pbl::visible::batch_host<false>(in, out, flags, nullptr);
}

int pbl_visible_batch_host_rd(const pbl_visible_in* in, pbl_visible_out* out, uint32_t flags, const uint64_t* cover_seq) {
  return cover_seq ? pbl::visible::batch_host<true>(in, out, flags, cover_seq)
                   : pbl::visible::batch_host<false>(in, out, flags, nullptr);
}

}  // extern "C"

template <bool kCover>
int pbl::visible::batch_host(const pbl_visible_in* in, pbl_visible_out* out, uint32_t flags, const uint64_t* cover) {
  namespace M = pbl::visible;
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!M::args_ok(in, out, flags, PBL_VISIBLE_KEEP_OPERANDS, false)) return PBL_INVALID_ARG;
  const pbl_decode_out& D = in->batch;
  const pbl_decode_out& O = out->result;
  const uint32_t nb = in->n_blocks, comparer = in->comparer;
  const bool keep = (flags & PBL_VISIBLE_KEEP_OPERANDS) != 0;
  pbl_seek_queries sq{};
  const K::View<R> V(D, nb, sq, nullptr, 0);

  struct Sizes {
    uint64_t n, k, v;
  };
  // The state machine over block q.  `emit`: write the results at result KV p0
  // (the sizes are known to fit); otherwise only count.  Returns the status.
  std::vector<uint64_t> chain;
  auto walk = [&](uint32_t q, bool emit, uint64_t p0, Sizes* sz) -> uint32_t {
    const K::Block<R> B(V, q);
    const uint64_t* tr = D.trailer + B.kv0;
    // rule 1: below the snapshot and under no newer range tombstone
    auto seen = [&](uint32_t x) {
      if (!M::is_visible(tr[x], in->snapshot)) return false;
      if constexpr (kCover) return !(cover[B.kv0 + x] > (tr[x] >> 8));
      return true;
    };
    const uint32_t* vo = D.val_off + B.kv0 + q;
    const uint8_t* vb = D.val_bytes + D.blk_val_base[q];
    uint64_t p = p0;
    uint32_t ko = 0, vout = 0;
    Sizes s{0, 0, 0};
    auto result = [&](uint32_t j, const std::vector<uint64_t>* ops, uint32_t n_src) {
      // result KV from source KV j; its value: KV j's, or the chain's, oldest first
      uint64_t kl;
      const uint8_t* k = B.key(j, &kl);
      uint64_t vl = 0;
      if (ops) for (uint64_t x : *ops) vl += vo[x + 1] - vo[x];
      else vl = vo[j + 1] - vo[j];
      if (emit) {
        const uint64_t kv = B.kv0 + j;
        O.trailer[p] = tr[j];
        if (O.kv_flags) O.kv_flags[p] = D.kv_flags ? uint8_t(D.kv_flags[kv] & M::kHandleBits) : uint8_t(0);
        if (O.entry_off) O.entry_off[p] = D.entry_off ? D.entry_off[kv] : 0u;
        if (O.tiering_span_id) {
          O.tiering_span_id[p] = D.tiering_span_id ? D.tiering_span_id[kv] : 0ull;
          O.tiering_attr[p] = D.tiering_attr ? D.tiering_attr[kv] : 0ull;
        }
        if (out->src_kv) out->src_kv[p] = kv;
        if (out->n_src) out->n_src[p] = n_src;
        O.key_off[p + q] = ko;
        O.val_off[p + q] = vout;
        if (kl) memcpy(O.key_bytes + O.blk_key_base[q] + ko, k, kl);
        uint8_t* dst = O.val_bytes + O.blk_val_base[q] + vout;
        if (ops) {
          for (size_t x = ops->size(); x-- > 0;) {
            const uint64_t o = (*ops)[x];
            if (vo[o + 1] - vo[o]) memcpy(dst, vb + vo[o], vo[o + 1] - vo[o]);
            dst += vo[o + 1] - vo[o];
          }
        } else if (vl) {
          memcpy(dst, vb + vo[j], vl);
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
    uint32_t j = 0;
    while (j < B.n && st == PBL_OK) {
      // the group [j, e)
      uint32_t e = j + 1;
      for (; e < B.n; e++) {
        uint64_t al, bl;
        const uint8_t *a = B.key(e - 1, &al), *b = B.key(e, &bl);
        if (pbl::cmp::key_cmp<R>(comparer, a, al, b, bl) != 0) break;
      }
      uint32_t h = j;
      while (h < e && !seen(h)) h++;
      bool ok;
      const uint32_t cls = h < e ? M::kind_class(tr[h], &ok) : uint32_t(M::kNone);
      if (cls == M::kSet) {
        result(h, nullptr, 1);
      } else if (cls == M::kMerge) {
        chain.clear();
        chain.push_back(h);
        for (uint32_t x = h + 1; x < e; x++) {
          if (!seen(x)) continue;
          const uint32_t c = M::kind_class(tr[x], &ok);
          if (c == M::kDel) break;
          chain.push_back(x);
          if (c == M::kSet) break;
        }
        if (keep) {
          for (size_t x = 0; x < chain.size(); x++) result(uint32_t(chain[x]), nullptr, x == 0 ? uint32_t(chain.size()) : 0u);
        } else {
          if (chain.size() > 1 && D.kv_flags)
            for (uint64_t x : chain)
              if (D.kv_flags[B.kv0 + x] & M::kHandleBits) st = PBL_UNSUPPORTED;
          if (st == PBL_OK) {
            result(h, &chain, uint32_t(chain.size()));
          }
        }
      }
      j = e;
    }
    if (st == PBL_OK && (s.n > M::kMaxKvs || s.k > M::kMaxBytes || s.v > M::kMaxBytes)) st = PBL_UNSUPPORTED;
    if (emit) {
      O.key_off[p + q] = ko;
      O.val_off[p + q] = vout;
    }
    *sz = s;
    return st;
  };

  // statuses and sizes
  std::vector<uint32_t> status(nb);
  pbl_totals T{};
  uint64_t kvb = 0, keyb = 0, valb = 0;
  K::with_cmp(comparer, [&](auto c) {
    constexpr uint32_t kCmp = decltype(c)::value;
    for (uint32_t q = 0; q < nb; q++) {
      uint32_t st = D.blk_status[q];
      Sizes s{0, 0, 0};
      if (st == PBL_OK) {
        const K::Block<R> B(V, q);
        const uint64_t* tr = D.trailer + B.kv0;
        bool order = true, kinds = true;
        for (uint32_t j = 0; j < B.n; j++) {
          bool ok;
          M::kind_class(tr[j], &ok);
          if (!ok || (D.kv_flags && (D.kv_flags[B.kv0 + j] & PBL_KV_INVALID_KEY))) kinds = false;
          if (j + 1 < B.n) {
            uint64_t al, bl;
            const uint8_t *a = B.key(j, &al), *b = B.key(j + 1, &bl);
            if (pbl::cmp::ikey_cmp<R, kCmp>(a, al, tr[j], b, bl, tr[j + 1]) > 0) order = false;
          }
        }
        if (!order) st = PBL_INVALID_ARG;
        else if (!kinds) st = PBL_UNSUPPORTED;
        else st = walk(q, false, 0, &s);
      }
      if (st != PBL_OK) {
        s = Sizes{0, 0, 0};
        T.status_mask |= 1u << st;
        T.n_bad_blocks++;
      }
      status[q] = st;
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
    if (status[q] == PBL_OK) {
      walk(q, true, O.blk_kv_base[q], &s);
    } else {
      O.key_off[O.blk_kv_base[q] + q] = 0;
      O.val_off[O.blk_kv_base[q] + q] = 0;
    }
  }
  return PBL_OK;
}

extern "C" {

size_t pbl_visible_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_visible_in), PBL_OFF(pbl_visible_in, batch), PBL_OFF(pbl_visible_in, n_blocks),
      PBL_OFF(pbl_visible_in, comparer), PBL_OFF(pbl_visible_in, n_kv), PBL_OFF(pbl_visible_in, snapshot),
      sizeof(pbl_visible_out), PBL_OFF(pbl_visible_out, result), PBL_OFF(pbl_visible_out, src_kv),
      PBL_OFF(pbl_visible_out, n_src)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
