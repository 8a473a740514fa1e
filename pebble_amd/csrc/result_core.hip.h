// result_core.hip.h — the back half that the batched scan, merge and visible
// view share: given per-block sizes and a place for every KV,
// assemble a result that has the layout of a decoded batch (include/pebble_amd.h).
//
//   chunk_sums / bases     the exclusive scan over result blocks in chunks of 256
//       (chunk sums, then each chunk adds the chunks before it): the result's
//       bases, statuses, totals and the capacity check
//   tile_scan_inplace      one workgroup's exclusive scan over per-tile sums
//   last_offsets           every block's last key / value offset
//   copy_kv_arrays         one KV's trailer, flags, entry offset and KVMeta
//   copy_values            a wave's values: at most 512 B by 8 lanes per KV,
//       longer ones by the whole wave
//   source_ok / result_ok / ws_aligned   the host-side checks of the arguments
//
// There are no kernels here: every kernel stays in its operator's file, which
// also keeps its workspace layout, its header word and its own rules.
#pragma once
#include "common.hip.h"
#include "key_cmp.hip.h"

namespace pbl {
namespace result {

// Threads of every kernel that calls in here (four waves), and so the result
// blocks per chunk of the scan over blocks and the tiles per step of a tile scan.
constexpr int kTPB = 256;

// The block that owns KV index kv: the last b with base[b] <= kv (blocks that
// own no KV index are stepped over).
__device__ inline uint32_t block_of(gptr<const uint64_t> base, uint32_t nb, uint64_t kv) {
  uint32_t lo = 0, hi = nb;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (base[m] <= kv) lo = m + 1;
    else hi = m;
  }
  return lo ? lo - 1 : 0;
}

// Sum of v over the workgroup (every thread gets it).  `lds`: 4 words.
__device__ inline uint64_t block_sum64(uint64_t v, uint64_t* lds) {
  v = wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) lds[wave_id()] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}
// Exclusive scan of v over the workgroup; *total = the sum.  `lds`: 4 words.
__device__ inline uint64_t block_excl_scan64(uint64_t v, uint64_t* lds, uint64_t* total) {
  const uint64_t inc = wave_incl_scan(v);
  __syncthreads();
  if (lane_id() == kWave - 1) lds[wave_id()] = inc;
  __syncthreads();
  uint64_t before = 0, t = 0;
  for (int w = 0; w < kTPB / kWave; w++) {
    const uint64_t s = lds[w];
    if (w < wave_id()) before += s;
    t += s;
  }
  *total = t;
  return before + inc - v;
}

// The per-block size arrays of a workspace: component c of block i is
// q64[c * qs + i] (0 KVs, 1 key bytes, 2 value bytes, then the operator's own),
// csum[c * n_chunks + chunk] its chunk sums, qst the statuses.
struct Sizes {
  gptr<uint64_t> q64, csum;
  gptr<uint32_t> qst;
  uint64_t qs;
  uint32_t n_chunks;
  __device__ gptr<uint64_t> q(int c) const { return q64 + uint64_t(c) * qs; }
};

// Workgroup = chunk blockIdx.x of the n blocks: the sums of its C components.
template <int C>
__device__ __forceinline__ void chunk_sums(const Sizes& S, uint32_t n, uint64_t* lds) {
  const uint64_t i = uint64_t(blockIdx.x) * kTPB + threadIdx.x;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const uint64_t s = block_sum64(i < n ? S.q(c)[i] : 0, lds);
    if (threadIdx.x == 0) S.csum[uint64_t(c) * S.n_chunks + blockIdx.x] = s;
  }
}

// Workgroup = chunk blockIdx.x of the n blocks, grid = the chunks: the result's
// bases, blk_rst_base zeros and statuses, with status_mask / n_bad_blocks (the
// entry point zeroed the totals).  ex[]: block i's exclusive prefixes (i =
// chunk * 256 + thread, to be used when i < n).  Returns true in one thread,
// the last chunk's thread 0, which has written the end bases and the totals
// and made the capacity check: end[] are the sums over all blocks, *over
// whether the result does not fit (then PBL_OVERFLOW is in the status mask).
template <int C>
__device__ __forceinline__ bool bases(const Sizes& S, const pbl_decode_out& O, uint32_t n, bool size_only, uint64_t* lds,
                                      uint64_t ex[C], uint64_t end[C], bool* over) {
  static_assert(C >= 3, "KVs, key bytes, value bytes");
  const uint64_t i = uint64_t(blockIdx.x) * kTPB + threadIdx.x;
#pragma unroll
  for (int c = 0; c < C; c++) {
    uint64_t before = 0;
    for (uint32_t ch = threadIdx.x; ch < blockIdx.x; ch += kTPB) before += S.csum[uint64_t(c) * S.n_chunks + ch];
    before = block_sum64(before, lds);
    uint64_t tot;
    ex[c] = before + block_excl_scan64(i < n ? S.q(c)[i] : 0, lds, &tot);
    end[c] = before + tot;
  }
  if (i < n) {
    to_glb(O.blk_kv_base)[i] = ex[0];
    to_glb(O.blk_key_base)[i] = ex[1];
    to_glb(O.blk_val_base)[i] = ex[2];
    if (O.blk_rst_base) to_glb(O.blk_rst_base)[i] = 0;
    const uint32_t st = S.qst[i];
    to_glb(O.blk_status)[i] = st;
    if (st != PBL_OK) {
      g_atomic_or(&O.totals->status_mask, 1u << st);
      g_atomic_add(&O.totals->n_bad_blocks, 1u);
    }
  }
  if (blockIdx.x != gridDim.x - 1 || threadIdx.x != 0) return false;
  to_glb(O.blk_kv_base)[n] = end[0];
  to_glb(O.blk_key_base)[n] = end[1];
  to_glb(O.blk_val_base)[n] = end[2];
  if (O.blk_rst_base) to_glb(O.blk_rst_base)[n] = 0;
  const gptr<pbl_totals> T = to_glb(O.totals);
  T->n_kv = end[0];
  T->key_bytes = end[1];
  T->val_bytes = end[2];
  T->n_restarts = 0;
  *over = !size_only && (end[0] > O.kv_cap || end[1] > O.key_cap || end[2] > O.val_cap);
  if (*over) g_atomic_or(&O.totals->status_mask, 1u << PBL_OVERFLOW);
  return true;
}

// One workgroup: the exclusive scan of C arrays of nt per-tile sums, in place.
template <int C>
__device__ __forceinline__ void tile_scan_inplace(const gptr<uint64_t> (&a)[C], uint64_t nt, uint64_t* lds) {
  uint64_t carry[C] = {};
  for (uint64_t t0 = 0; t0 < nt; t0 += kTPB) {
    const uint64_t t = t0 + threadIdx.x;
#pragma unroll
    for (int c = 0; c < C; c++) {
      const uint64_t v = t < nt ? a[c][t] : 0;
      uint64_t tot;
      const uint64_t ex = block_excl_scan64(v, lds, &tot);
      if (t < nt) a[c][t] = carry[c] + ex;
      carry[c] += tot;
    }
  }
}

// Every block's last offset (an empty block's only one), grid-striding over the
// nb blocks.  A block whose KVs end past kv_cap is left out.
__device__ __forceinline__ void last_offsets(const pbl_decode_out& O, uint32_t nb, uint64_t kv_cap) {
  const gptr<const uint64_t> okvb = to_glb((const uint64_t*)O.blk_kv_base), okeyb = to_glb((const uint64_t*)O.blk_key_base),
                             ovalb = to_glb((const uint64_t*)O.blk_val_base);
  for (uint64_t q = uint64_t(blockIdx.x) * kTPB + threadIdx.x; q < nb; q += uint64_t(gridDim.x) * kTPB) {
    const uint64_t at = okvb[q + 1] + q;
    if (okvb[q + 1] > kv_cap) continue;
    to_glb(O.key_off)[at] = uint32_t(okeyb[q + 1] - okeyb[q]);
    to_glb(O.val_off)[at] = uint32_t(ovalb[q + 1] - ovalb[q]);
  }
}

// Result KV p's per-KV arrays from KV kv of the source I.  kv_flags pass through
// flags_mask, and are zero for a source without them.  entry_off and the
// tiering arrays (KVMeta travels with its KV) of a source without them:
// zero_missing writes zeros, otherwise the result's are left unwritten.
__device__ __forceinline__ void copy_kv_arrays(const pbl_decode_out& O, uint64_t p, const pbl_decode_out& I, uint64_t kv,
                                               uint8_t flags_mask, bool zero_missing) {
  to_glb(O.trailer)[p] = to_glb(I.trailer)[kv];
  if (O.kv_flags) to_glb(O.kv_flags)[p] = I.kv_flags ? uint8_t(to_glb(I.kv_flags)[kv] & flags_mask) : uint8_t(0);
  if (O.entry_off && (zero_missing || I.entry_off)) to_glb(O.entry_off)[p] = I.entry_off ? to_glb(I.entry_off)[kv] : 0u;
  if (O.tiering_span_id && (zero_missing || I.tiering_span_id)) {
    to_glb(O.tiering_span_id)[p] = I.tiering_span_id ? to_glb(I.tiering_span_id)[kv] : 0ull;
    to_glb(O.tiering_attr)[p] = I.tiering_attr ? to_glb(I.tiering_attr)[kv] : 0ull;
  }
}

// The whole wave copies its lanes' values: lane l's is vlen bytes from vsrc to
// vdst when ok.  Values of at most 512 B: 8 lanes per KV (lane c of a group
// copies the value's 16-B chunks c, c + 8, ...); longer ones by the whole wave.
// Every lane of the wave calls it.
__device__ __forceinline__ void copy_values(bool ok, uint32_t vlen, gptr<const uint8_t> vsrc, gptr<uint8_t> vdst) {
  const uint32_t lane = lane_id();
#pragma unroll 1
  for (uint32_t u = 0; u < kWave / 8; u++) {
    const int sl = int(8 * u + (lane >> 3));
    const bool sv = __shfl(int(ok && vlen <= 512), sl, kWave) != 0;
    const gptr<const uint8_t> sp = (gptr<const uint8_t>)__shfl((unsigned long long)vsrc, sl, kWave);
    const gptr<uint8_t> dp = (gptr<uint8_t>)__shfl((unsigned long long)vdst, sl, kWave);
    const uint32_t sn = uint32_t(__shfl(int(vlen), sl, kWave));
    if (!sv) continue;
    for (uint32_t i = 16 * (lane & 7u); i < sn; i += 128) copy_chunks(dp + i, sp + i, sn - i < 16 ? sn - i : 16u);
  }
  for (uint64_t m = __ballot(ok && vlen > 512); m; m &= m - 1) {
    const int src_lane = __builtin_ctzll(m);
    const gptr<const uint8_t> sp = (gptr<const uint8_t>)__shfl((unsigned long long)vsrc, src_lane, kWave);
    const gptr<uint8_t> dp = (gptr<uint8_t>)__shfl((unsigned long long)vdst, src_lane, kWave);
    const uint32_t sn = uint32_t(__shfl(int(vlen), src_lane, kWave));
    for (uint32_t i = 16 * lane; i < sn; i += 16 * kWave) copy_chunks(dp + i, sp + i, sn - i < 16 ? sn - i : 16u);
  }
}

// ---- host side -----------------------------------------------------------------
// A decoded batch that can be a source: every array the operators read.
inline bool source_ok(const pbl_decode_out* d) {
  return d && d->blk_status && d->blk_kv_base && d->blk_key_base && d->blk_val_base && d->key_off && d->val_off &&
         d->key_bytes && d->val_bytes && d->trailer && !d->tiering_span_id == !d->tiering_attr;
}
// A result that can be written: the sizes' arrays always, the rest unless only
// sizes are asked for.
inline bool result_ok(const pbl_decode_out& o, bool size_only) {
  if (!o.blk_kv_base || !o.blk_key_base || !o.blk_val_base || !o.blk_status || !o.totals) return false;
  if (size_only) return true;
  if (!o.tiering_span_id != !o.tiering_attr) return false;
  const bool any = o.kv_cap || o.key_cap || o.val_cap;  // (all zero: sizes are all that can come out)
  if (any && (!o.trailer || !o.key_off || !o.val_off || !o.key_bytes || !o.val_bytes)) return false;
  return true;
}
inline bool ws_aligned(const void* ws) { return ws && !(reinterpret_cast<uintptr_t>(ws) & 15); }

}  // namespace result
}  // namespace pbl
