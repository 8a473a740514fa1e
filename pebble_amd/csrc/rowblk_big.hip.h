// rowblk_big.hip.h — row blocks past the 32 KiB LDS stage, and the launch that
// prepares a pool-path batch: row_prepare_kernel clears the look-back state and
// sizes those blocks ahead of the row kernel; the count walk and the publish
// it shares with the row kernel's own second tier (block_big in
// rowblk_pool.hip.h) and with the long-key kernels (rowblk_long.hip.h).  Each
// walk is the general walk (rowblk_general.hip.h) over global memory.
#pragma once

#include "rowblk_core.hip.h"
#include "rowblk_general.hip.h"

namespace pbl {
namespace row {
namespace rowc {

#ifndef PBL_BIG_WIN
#define PBL_BIG_WIN 8  // blocks per row_prepare_kernel workgroup (the values pass's form: 126 us at 8, 170 at 16)
#endif
#ifndef PBL_BIG_U
#define PBL_BIG_U 8  // value granules per lane in flight (16: within noise on config 5)
#endif
#ifndef PBL_BIG_KEYBUF
#define PBL_BIG_KEYBUF 8192
#endif
constexpr uint32_t kBigKeySmall = PBL_BIG_KEYBUF;  // the sizes tier-1 key buffer
constexpr int kWsBigRedo = 5;  // header u32 [5]: the two-pass row form's dense blocks (ids at ws_redo_offset)
constexpr int kWsBigPend = 6;  // header u32 [6]: the two-pass row form's long-key blocks (ids at ws_pend_offset)
constexpr int kWsBigLong = 7;  // header u32 [7]: a key past the 32 KiB buffer (rowblk_long.hip.h)
// blk_status[b] of a block past the stage whose tier-1 walk needs more than
// the small key buffer (or whose totals pass 4 GiB): not published yet.  The
// wave of the row kernel that draws the block walks it again with a stage as
// the key buffer (tier 2, block_big); with key spill slots
// long_key_sizes2_kernel does, before the row kernel.  Never a final status:
// whoever walks the block again replaces it.
constexpr uint32_t kBigRedo = 0x80000000u | PBL_UNSUPPORTED;

// Sizes of the blocks past the LDS stage (blen > kMaxFastLen), ahead of the row
// kernel on the same stream.  Their count walk reads global memory entry by
// entry; inside the pipeline it would hold back the look-back of every later
// ticket.  In row_prepare_kernel all of them walk at once and publish their
// aggregates, so the row kernel's block_big only resolves.  Same init checks
// and the same general walk as a staged block's, so the aggregate is the one
// the row kernel would compute.  Two tiers: tier 1 in row_prepare_kernel, one
// one-wave workgroup per PBL_BIG_WIN-block window with a kBigKeySmall key
// buffer; a block whose walk needs more (PBL_UNSUPPORTED) is marked kBigRedo
// and walked with a whole 32 KiB stage by the wave of the row kernel that draws
// its ticket (tier 2).  (Tier 1 was one workgroup per 64 blocks, 4 per CU, with
// the 32 KiB buffer: config 5's 2195 big blocks took 59 us, two to three serial
// walks per wave; 33 us in windows, 16 us without one atomic per big block on
// a shared counter.)
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

// The one launch ahead of the row kernel on the pool path (row batches and
// mixed batches): it clears what the two memsets cleared and does the sizes
// tier 1.  Workgroup w owns the block ids of its windows: it zeroes their
// entries of rec[], pfx[][] and wide[][] and the chunk records whose first block
// it owns, workgroup 0 also the workspace header and *totals; then it walks its
// windows' big blocks (row blocks only: a mixed batch's colblk blocks are the
// colblk pipeline's) and publishes them.  A workgroup publishes only into
// records it zeroed itself, after its zeroing stores have completed, so nothing
// depends on the order in which workgroups run.  Nothing here adds to a header
// counter or to *totals: workgroup 0 may be zeroing them at that moment.
__global__ void __launch_bounds__(kWave) row_prepare_kernel(Args A) {
  __shared__ uint4 keybuf4[kBigKeySmall / 16];
  static_assert(sizeof(pbl_totals) % 8 == 0 && kWsHeader / 8 <= kWave && sizeof(pbl_totals) / 8 <= kWave, "one store per lane");
  const uint32_t nb = A.in.n_blocks;
  const uint32_t l = lane_id();
  uint64_t* ws = reinterpret_cast<uint64_t*>(A.out.workspace);
  const LbPtrs P(ws + kWsHeader / 8, nb);
  if (blockIdx.x == 0) {
    if (l < kWsHeader / 8) st_agent(ws + l, 0);
    if (l < sizeof(pbl_totals) / 8) st_agent(reinterpret_cast<uint64_t*>(A.out.totals) + l, 0);
  }
  for (uint64_t base = uint64_t(blockIdx.x) * PBL_BIG_WIN; base < nb; base += uint64_t(gridDim.x) * PBL_BIG_WIN) {
    const uint32_t n = nb - base < PBL_BIG_WIN ? uint32_t(nb - base) : uint32_t(PBL_BIG_WIN);
    for (uint32_t i = l; i < 2 * n; i += kWave) st_agent(P.rec + 2 * base + i, 0);
    // (wide[][] follows pfx[][]: 2 * kNumComp arrays of n_blocks words)
    for (uint32_t i = l; i < 2 * kNumComp * PBL_BIG_WIN; i += kWave) {
      const uint32_t a = i / PBL_BIG_WIN, j = i % PBL_BIG_WIN;
      if (j < n) st_agent(P.pfx + uint64_t(a) * nb + base + j, 0);
    }
    for (uint64_t c = (base + kL2Chunk - 1) / kL2Chunk + l; c * kL2Chunk < base + n; c += kWave) {
      st_agent(P.l2 + 2 * c, 0);
      st_agent(P.l2 + 2 * c + 1, 0);
    }
    const uint64_t bl = base + l;
    uint64_t big = __ballot(l < PBL_BIG_WIN && bl < nb && to_glb(A.in.block_len)[bl] > kMaxFastLen &&
                            (!A.in.block_format || to_glb(A.in.block_format)[bl] == PBL_FMT_ROW));
    // the zeroes have landed before a record of the window is published
    if (big) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    while (big) {
      const uint32_t b = uint32_t(base) + uint32_t(__builtin_ctzll(big));
      big &= big - 1;
      SlowState ss;
      big_block_count(A, b, to_lds_ptr(reinterpret_cast<uint8_t*>(keybuf4)), kBigKeySmall, &ss);
      if (ss.status == PBL_UNSUPPORTED) {  // a key past the small buffer (or a total past 4 GiB): tier 2
        if (l == 0) to_glb(A.out.blk_status)[b] = kBigRedo;
        continue;
      }
      big_block_publish(A, b, ss);
    }
  }
}

}  // namespace rowc
}  // namespace row
}  // namespace pbl
