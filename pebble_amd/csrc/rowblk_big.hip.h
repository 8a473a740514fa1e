// rowblk_big.hip.h — the passes for row blocks past the 32 KiB LDS stage:
// big_block_sizes_kernel / big_block_sizes2_kernel before the decode launch,
// big_block_values_kernel after it for what the row kernel left.  Each is the
// general walk (rowblk_general.hip.h) over global memory.
#pragma once

#include "rowblk_core.hip.h"
#include "rowblk_general.hip.h"

namespace pbl {
namespace row {
namespace rowc {

#ifndef PBL_BIG_WIN
#define PBL_BIG_WIN 8  // blocks per sizes tier-1 workgroup (the values pass's form: 126 us at 8, 170 at 16)
#endif
#ifndef PBL_BIG_U
#define PBL_BIG_U 8  // value granules per lane in flight (16: within noise on config 5)
#endif
#ifndef PBL_BIG_KEYBUF
#define PBL_BIG_KEYBUF 8192
#endif
constexpr uint32_t kBigKeySmall = PBL_BIG_KEYBUF;  // the sizes tier-1 key buffer
constexpr int kWsBigRedo = 5;  // header u32 [5]: sizes tier-2 blocks (their ids in the redo area, ws_redo_offset)
constexpr int kWsBigPend = 6;  // header u32 [6]: blocks the row kernel did not write (ids at ws_pend_offset)
constexpr int kWsBigLong = 7;  // header u32 [7]: a key past the 32 KiB buffer (rowblk_long.hip.h)

// Size pass for the blocks past the LDS stage (blen > kMaxFastLen), launched
// ahead of the row kernel on the same stream.  Their count walk reads global
// memory entry by entry; inside the pipeline it would hold back the look-back
// of every later ticket.  Here all of them walk at once and publish their
// aggregates, so the row kernel's block_big only resolves.  Same init checks
// and the same general walk as a staged block's, so the aggregate is the one
// the row kernel would compute.  Two tiers: tier 1 one one-wave
// workgroup per PBL_BIG_WIN-block window with a kBigKeySmall key buffer; a
// block whose walk needs more (PBL_UNSUPPORTED) is listed in the redo area and
// walked by tier 2 with the whole 32 KiB buffer.  (Tier 1 was one workgroup per
// 64 blocks, 4 per CU, with the 32 KiB buffer: config 5's 2195 big blocks took
// 59 us, two to three serial walks per wave; 33 us in windows, 16 us without
// one atomic per big block on a shared counter.)
__device__ __forceinline__ void big_block_publish(const Args& A, uint32_t b, const SlowState& ss) {
  const uint32_t nb = A.in.n_blocks;
  uint64_t* lb_state = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) + kWsHeader);
  const bool okk = ss.status == PBL_OK;
  const uint64_t agg[kNumComp] = {okk ? ss.nkv : 0, okk ? ss.kb : 0, okk ? ss.vb : 0, okk ? ss.nr : 0};
  lb_publish(lb_state, nb, b, agg);
  if (lane_id() == 0) {  // for block_big (write_block_meta replaces them)
    to_glb(A.out.blk_status)[b] = ss.status;
    to_glb(A.out.blk_kv_base)[b] = agg[0];
    to_glb(A.out.blk_key_base)[b] = agg[1];
    to_glb(A.out.blk_val_base)[b] = agg[2];
  }
}

// The count walk of a big block; a block failing Iter.Init's checks (zero
// restarts, a restart table past the block, a bad first entry) gets that
// status and a zero aggregate, which big_block_publish publishes like any other.
template <bool kSpill = false>
__device__ __forceinline__ void big_block_count(const Args& A, uint32_t b, lptr<uint8_t> keybuf, uint32_t keycap,
                                                SlowState* ss, gptr<uint8_t> spill = nullptr, uint64_t spillcap = 0) {
  const uint32_t blen = A.in.block_len[b];
  const uint8_t* gblk = A.in.blocks + A.in.block_off[b];
  uint32_t roff, nres;
  const uint32_t st = init_checks(GlbBlk{to_glb(gblk), blen}, blen, A.in.flags, &roff, &nres);
  if (st != PBL_OK) {
    ss->nkv = ss->kb = ss->vb = ss->nr = 0;
    ss->status = st;
    return;
  }
  const uint64_t dummy[kNumComp] = {0, 0, 0, 0};
  slow_walk_t<GlbBlk, 1, kSpill>(GlbBlk{to_glb(gblk), blen}, blen, A.in.flags, A.in.synthetic_seq_num, keybuf, keycap,
                                  kPassCount, A.out, b, dummy, ss, spill, spillcap);
}

__global__ void __launch_bounds__(kWave) big_block_sizes_kernel(Args A) {
  __shared__ uint4 keybuf4[kBigKeySmall / 16];
  const uint32_t nb = A.in.n_blocks;
  uint32_t* hdr = reinterpret_cast<uint32_t*>(A.out.workspace);
  uint32_t* redo = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) + ws_redo_offset(nb));
  for (uint64_t base = uint64_t(blockIdx.x) * PBL_BIG_WIN; base < nb; base += uint64_t(gridDim.x) * PBL_BIG_WIN) {
    const uint64_t bl = base + lane_id();
    // (row blocks only: a mixed batch's colblk blocks are the colblk pipeline's)
    uint64_t big = __ballot(lane_id() < PBL_BIG_WIN && bl < nb && to_glb(A.in.block_len)[bl] > kMaxFastLen &&
                            (!A.in.block_format || to_glb(A.in.block_format)[bl] == PBL_FMT_ROW));
    while (big) {
      const uint32_t b = uint32_t(base) + uint32_t(__builtin_ctzll(big));
      big &= big - 1;
      SlowState ss;
      big_block_count(A, b, to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)), kBigKeySmall, &ss);
      if (ss.status == PBL_UNSUPPORTED) {  // a key past the small buffer (or a total past 4 GiB): tier 2
        if (lane_id() == 0) to_glb(redo)[g_atomic_add(hdr + kWsBigRedo, 1u)] = b;
        continue;
      }
      big_block_publish(A, b, ss);
    }
  }
}

// Tier 2's body.  kList (long_key_sizes2_kernel in rowblk_long.hip.h, launched
// in its place for a workspace with key spill slots): a block whose walk
// stopped at a key past the 32 KiB buffer is listed for tier 3 instead of
// published (ids at ws_ent_offset, which the pool path leaves unused; their
// count at header word kWsBigLong).  A block whose totals pass 4 GiB stays
// PBL_UNSUPPORTED.  The two are told apart by the sums at the point where the
// walk stopped: a block whose sums had already passed 4 GiB when it met the
// long key is published as PBL_UNSUPPORTED without tier 3, which is its final
// status unless a later entry is corrupt (the oracle would then report
// PBL_CORRUPT_BOUNDS); that needs more than 4 GiB of decoded keys or values
// ahead of a long key in one block, which no table holds.
template <bool kList>
__device__ __forceinline__ void big_block_sizes2_body(const Args& A, uint4* keybuf4) {
  const uint32_t nb = A.in.n_blocks;
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(A.out.workspace);
  const uint32_t n = __hip_atomic_load(to_glb(hdr) + kWsBigRedo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t* redo = reinterpret_cast<const uint32_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) +
                                                           ws_redo_offset(nb));
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t b = to_glb(redo)[i];
    SlowState ss;
    big_block_count(A, b, to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)), uint32_t(kLdsBlkBytes), &ss);
    if constexpr (kList) {
      if (ss.status == PBL_UNSUPPORTED && !((ss.kb | ss.vb) >> 32)) {
        uint32_t* lng = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) + ws_ent_offset(nb));
        if (lane_id() == 0) to_glb(lng)[g_atomic_add(const_cast<uint32_t*>(hdr) + kWsBigLong, 1u)] = b;
        continue;
      }
    }
    big_block_publish(A, b, ss);
  }
}

__global__ void __launch_bounds__(kWave) big_block_sizes2_kernel(Args A) {
  __shared__ uint4 keybuf4[kLdsBlkBytes / 16];
  big_block_sizes2_body<false>(A, keybuf4);
}

// Outputs of the blocks past the LDS stage.  The row kernel walks each one
// itself once its look-back has resolved the block's bases (block_big in
// rowblk_pool.hip.h: the wave's slot as the key buffer, the value copy hidden
// behind the other waves' work); the blocks it could not (a key past the slot)
// it lists, and this pass, launched after it on the same stream, walks them
// with the whole 32 KiB key buffer.  8 value granules per lane in flight.
__global__ void __launch_bounds__(kWave) big_block_values_kernel(Args A) {
  __shared__ uint4 keybuf4[kLdsBlkBytes / 16];
  const uint32_t nb = A.in.n_blocks;
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(A.out.workspace);
  const uint32_t n = __hip_atomic_load(to_glb(hdr) + kWsBigPend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t* pend = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(A.out.workspace) +
                                                           ws_pend_offset(nb));
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t b = to_glb(pend)[i];
    const uint32_t blen = A.in.block_len[b];
    const uint64_t bases[kNumComp] = {A.out.blk_kv_base[b], A.out.blk_key_base[b], A.out.blk_val_base[b],
                                      A.out.blk_rst_base ? A.out.blk_rst_base[b] : 0};
    SlowState ss;
    slow_walk_t<GlbBlk, PBL_BIG_U>(GlbBlk{to_glb(A.in.blocks + A.in.block_off[b]), blen}, blen, A.in.flags,
                                    A.in.synthetic_seq_num, to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)),
                                    uint32_t(kLdsBlkBytes), kPassAll, A.out, b, bases, &ss);
  }
}

}  // namespace rowc
}  // namespace row
}  // namespace pbl
