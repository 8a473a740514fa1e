// rowblk_long.hip.h — row blocks with a key past the general walk's 32 KiB LDS
// key buffer: the kernels that size and write them with slow_walk_t's spill
// form (rowblk_general.hip.h), the key continuing in a slot of the workspace.
// Launched only for a workspace that holds slots (pbl_workspace_bytes_for);
// every other launch runs the kernels it always did.
#pragma once

#include "rowblk_core.hip.h"
#include "rowblk_general.hip.h"
#include "rowblk_big.hip.h"

namespace pbl {
namespace row {
namespace rowc {

// ---- keys past the 32 KiB buffer ----------------------------------------------
// Go's readEntry grows fullKey without bound (rowblk_iter.go:400-403).  Here the
// key continues in a spill slot in global memory (slow_walk_t's spill form):
// kLongKeyWgs one-wave workgroups, workgroup i owning slot i of the slots the
// caller's workspace holds past ws_alloc_bytes (pbl_workspace_bytes_for), each
// looping over a list of block ids.  Launched only for a workspace with slots.
// A key that outgrows its slot is PBL_UNSUPPORTED, as every long key is
// without slots.
struct LongSlot {
  gptr<uint8_t> p;
  uint64_t cap;
};
__device__ __forceinline__ LongSlot long_slot(const Args& A) {
  const uint32_t nb = A.in.n_blocks;
  const uint64_t cap = ws_spill_slot_bytes(A.out.workspace_bytes, nb);
  return LongSlot{to_glb(reinterpret_cast<uint8_t*>(A.out.workspace) + ws_alloc_bytes(nb) + uint64_t(blockIdx.x) * cap),
                  cap};
}

// Sizes tier 2 for a workspace with slots, between row_prepare_kernel and the
// row kernel (without slots the row kernel's block_big does tier 2 itself):
// every block that tier 1 marked kBigRedo (rowblk_big.hip.h) is walked with the
// whole 32 KiB buffer.  A block whose walk stopped at a key past that buffer
// is listed for tier 3 instead of published (ids at ws_ent_offset, which the
// pool path leaves unused; their count at header word kWsBigLong).  A block
// whose totals pass 4 GiB stays PBL_UNSUPPORTED.  The two are told apart by the
// sums at the point where the walk stopped: a block whose sums had already
// passed 4 GiB when it met the long key is published as PBL_UNSUPPORTED without
// tier 3, which is its final status unless a later entry is corrupt (the
// oracle would then report PBL_CORRUPT_BOUNDS); that needs more than 4 GiB of
// decoded keys or values ahead of a long key in one block, which no table
// holds.  The marks are found by a scan of the batch, kWave ids per step: tier
// 1 keeps no list, because nothing in it may add to a header counter.
__global__ void __launch_bounds__(kWave) long_key_sizes2_kernel(Args A) {
  __shared__ uint4 keybuf4[kLdsBlkBytes / 16];
  const uint32_t nb = A.in.n_blocks;
  uint32_t* hdr = reinterpret_cast<uint32_t*>(A.out.workspace);
  uint32_t* lng = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) + ws_ent_offset(nb));
  for (uint64_t base = uint64_t(blockIdx.x) * kWave; base < nb; base += uint64_t(gridDim.x) * kWave) {
    const uint64_t bl = base + lane_id();
    uint64_t redo = __ballot(bl < nb && to_glb(A.in.block_len)[bl] > kMaxFastLen &&
                             (!A.in.block_format || to_glb(A.in.block_format)[bl] == PBL_FMT_ROW) &&
                             to_glb(A.out.blk_status)[bl] == kBigRedo);
    while (redo) {
      const uint32_t b = uint32_t(base) + uint32_t(__builtin_ctzll(redo));
      redo &= redo - 1;
      SlowState ss;
      big_block_count(A, b, to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)), uint32_t(kLdsBlkBytes), &ss);
      if (ss.status == PBL_UNSUPPORTED && !((ss.kb | ss.vb) >> 32)) {
        if (lane_id() == 0) to_glb(lng)[g_atomic_add(hdr + kWsBigLong, 1u)] = b;
        continue;
      }
      big_block_publish(A, b, ss);
    }
  }
}

// Sizes tier 3: the blocks tier 2 listed, sized with the spill form and
// published before the row kernel starts (its block_big only resolves, as for
// every other big block).
__global__ void __launch_bounds__(kWave) long_key_sizes_kernel(Args A) {
  __shared__ uint4 keybuf4[kLdsBlkBytes / 16];
  const uint32_t nb = A.in.n_blocks;
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(A.out.workspace);
  const uint32_t n = __hip_atomic_load(to_glb(hdr) + kWsBigLong, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t* lng = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(A.out.workspace) +
                                                          ws_ent_offset(nb));
  const LongSlot sp = long_slot(A);
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t b = to_glb(lng)[i];
    SlowState ss;
    big_block_count<true>(A, b, to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)), uint32_t(kLdsBlkBytes), &ss, sp.p,
                          sp.cap);
    big_block_publish(A, b, ss);
  }
}

// The outputs of long-key blocks, after every other row kernel of the launch:
// the ids at workspace byte offset `list_off`, their count at header word
// `count_word` (the pool path: tier 3's list; the two-pass form: the blocks
// its emit listed).  A listed block's bases are final; one that is not PBL_OK
// (an overflow, a key past its slot) has no outputs.  The walk rewrites what
// an earlier walk of the block wrote up to its long key.  On the pool path
// there are two of those, both block_big's: with the wave's slot, then with a
// 32 KiB stage; both stop at the long key, inside the block's own output range.
// The second is wasted work, left as it is: skipping it would put a lookup of
// tier 3's list into block_big, that is into the pool kernel every batch runs,
// to save one partial walk per long-key block on a cold path.
__global__ void __launch_bounds__(kWave) long_key_values_kernel(Args A, uint64_t list_off, int count_word) {
  __shared__ uint4 keybuf4[kLdsBlkBytes / 16];
  const pbl_decode_out& O = A.out;
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(O.workspace);
  const uint32_t n = __hip_atomic_load(to_glb(hdr) + count_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t* list = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(O.workspace) + list_off);
  const LongSlot sp = long_slot(A);
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t b = to_glb(list)[i];
    if (to_glb(O.blk_status)[b] != PBL_OK) continue;
    const uint32_t blen = to_glb(A.in.block_len)[b];
    const uint64_t bases[kNumComp] = {to_glb(O.blk_kv_base)[b], to_glb(O.blk_key_base)[b], to_glb(O.blk_val_base)[b],
                                      O.blk_rst_base ? to_glb(O.blk_rst_base)[b] : 0};
    SlowState ss;
    slow_walk_t<GlbBlk, PBL_BIG_U, true>(GlbBlk{to_glb(A.in.blocks + to_glb(A.in.block_off)[b]), blen}, blen,
                                          A.in.flags, A.in.synthetic_seq_num,
                                          to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)), uint32_t(kLdsBlkBytes),
                                          kPassAll, O, b, bases, &ss, sp.p, sp.cap);
    if (ss.status != PBL_OK && lane_id() == 0) {
      // the same walk as the sizes pass over the same bytes cannot disagree
      // with it; if it ever did, the block reports the walk's status
      to_glb(O.blk_status)[b] = ss.status;
      g_atomic_or(&O.totals->status_mask, 1u << ss.status);
      g_atomic_add(&O.totals->n_bad_blocks, 1u);
    }
  }
}

}  // namespace rowc
}  // namespace row
}  // namespace pbl
