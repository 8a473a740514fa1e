// rowblk_pool.hip.h — the row-format decode with one wave per block, eight
// waves per CU and a shared pool of LDS staging buffers.
//
// Only the parse needs a block's bytes in LDS; the keys and the value bytes
// (80 % of the output) are gathered global->global from the block that was
// just read (L2 / MALL-hot) through compact per-KV metadata in the wave's own
// slot.  So a 32 KiB stage is held only for the DMA, the walk and the
// metadata pass, and the other waves stage their blocks while this one emits.
//
//   acquire   a wave takes a free stage from the workgroup's pool (LDS mask),
//             THEN a ticket (the only order that keeps the look-back
//             deadlock-free: every ticket holder either holds a stage or has
//             published its aggregate)
//   stage     the block HBM -> LDS by LDS-DMA, one round trip
//   walk      lane per restart run (rowblk_writer.go:147-155 cuts the prefix
//             chain there): headers parked in registers, a DPP scan places the
//             runs, the block's aggregate is published.  One run per lane
//             (up to 64 runs): 16 straight-line entries, no exec-masked
//             branch on the common path, the failure causes looked at once
//             after the loop (PBL_POOL_FRONT, round 12)
//   meta      per-entry metadata words (key source, shared and key length,
//             prefix parent, header length, flags) and per-KV value offsets
//             written from the registers into the slot, 16 flat bodies; the
//             stage is released (before this pass when it reads the registers
//             only: PBL_POOL_EARLYREL)
//   resolve   the exclusive prefix by decoupled look-back, issued together
//             with the first step's and the restart words' loads
//   prefetch  (PBL_POOL_PREFETCH, off by default: measured slower, DESIGN.md
//             3.1) under the emit's last steps: a free stage if there is
//             one, the next ticket and that block's DMA, so the next acquire
//             / stage find their work done
//   steps     64 KVs per step, keys and values together (a line of the block
//             is fetched once for both), each step's loads issued before the
//             previous step's stores:
//               keys    lane per KV: offsets (a wave scan of the key lengths),
//                       trailer, flags, entry offset, the user key merged from
//                       its prefix chain
//               values  8 lanes per KV, 16-B chunks; a step whose values are
//                       all empty or 16..128 B long is the fast step
//                       (PBL_POOL_VFAST): descriptors read once, lane per
//                       KV, permuted to the groups, no per-KV branch
//             (PBL_POOL_SBASE, off by default: measured no gain, DESIGN.md
//             3.1) the step's uniform bases in SGPRs, lane offsets unsigned
//             32-bit
//
// LDS per CU: 3 stages x 32.8 KB + 8 slots x ~8 KB (one per wave).
//
// Blocks outside the fast-path limits (more entries than a slot holds, keys
// past kMaxKl, 3-byte header varints, ...) take the wave-serial general walk
// (rowblk_general.hip.h) on the staged bytes; blocks past kMaxFastLen are sized
// by row_prepare_kernel before this launch (rowblk_big.hip.h; the few it leaves,
// by the wave that draws them, with its stage as the key buffer) and written by
// the wave that draws their ticket (block_big).  Results are identical on
// every path.
//
// Semantics: cockroachdb/pebble sstable/rowblk/rowblk_iter.go — Init :241-276,
// readFirstKey :418-485, readEntry :333-416, decodeInternalKey :487-504, value
// prefix :1192-1199 (sstable/block/kv.go:14-41), decodeRestart :1092-1096,
// HideObsoletePoints :1168-1179.
#pragma once

#include "rowblk_core.hip.h"
#include "rowblk_general.hip.h"
#include "rowblk_big.hip.h"

namespace pbl {
namespace row {
namespace pool {

#ifndef PBL_POOL_WAVES
#define PBL_POOL_WAVES 8
#endif
#ifndef PBL_POOL_STAGES
#define PBL_POOL_STAGES 3
#endif
#ifndef PBL_POOL_SLEEP
#define PBL_POOL_SLEEP 8  // s_sleep units (64 cycles) between polls of the stage mask
#endif
#ifndef PBL_POOL_PRIO
#define PBL_POOL_PRIO 2  // the stage holder's issue priority (the emits run at 0)
#endif
// PBL_POOL_EARLYREL: the stage goes back to the pool right after the walk when
// the metadata pass does not read it (no value prefixes, every run within the
// parked registers).  0: after the metadata pass, always; 1: early, the
// metadata pass at the emit's priority; 2: early, PBL_POOL_PRIO kept until the
// metadata pass is done.
#ifndef PBL_POOL_EARLYREL
#define PBL_POOL_EARLYREL 2
#endif
// PBL_POOL_PREFETCH: the wave's next block is staged under its emit, the DMA
// issued before the loads of the emit step this many steps before the last
// one (a block with fewer steps: before its first stores).  0: off.
#ifndef PBL_POOL_PREFETCH
#define PBL_POOL_PREFETCH 0  // compiled out: the measurements are in DESIGN.md 3.1
#endif
// PBL_POOL_PREFETCH_LATE 1: one step later than that (PBL_POOL_PREFETCH 1:
// before the last step's stores, after every load of the emit).
#ifndef PBL_POOL_PREFETCH_LATE
#define PBL_POOL_PREFETCH_LATE 1
#endif
// PBL_POOL_LB_WIN / PBL_POOL_LB_WIN_LATER: windows of 64 predecessor records
// the emit loads with its first step, and per later round trip of the same
// resolve (this kernel's own counts: the other kernels keep PBL_LB_WIN for
// both).  Round 9's stamps: 94 % of config 2's resolves take two round trips
// and meet the prefix 130 records back, i.e. within the second trip's first
// records, so a later trip of 128 records loads 120 it never needs, and every
// record is an 8-byte agent-scope load of lines that some 2000 waves read and
// write.  Plain bench.py, GiB/s, parent / first-later (DESIGN.md 3.1, round 9,
// profiles/r09/ab_variants.txt):
//   config 2      1379-1380 / 2-1: 1469-1471, 3-1: 1517-1521, 4-1: 1477-1479
//   zipf on pool   933-943  / 2-1: 955, 3-1: 921-923, 4-1: 902-907
// 2-1 is the one form under which no measured workload falls below its
// parent's range; with first = later config 2 gives 3: 1438-1444, 4: 1485-1488,
// 5: 1318-1340, 6: 1235-1239, 8: 1172-1174.
#ifndef PBL_POOL_LB_WIN
#define PBL_POOL_LB_WIN PBL_LB_WIN
#endif
#ifndef PBL_POOL_LB_WIN_LATER
#define PBL_POOL_LB_WIN_LATER 1
#endif
// PBL_LB_V16 / PBL_POOL_LB_ST16 / PBL_POOL_LB_LATER_LANES (round 10, DESIGN.md
// 3.1): this kernel's look-back records as single 16-byte accesses (the blocks
// handed to block_big / block_slow included; every other kernel keeps the
// 8-byte form).
//   PBL_LB_V16 1              a window is one 16-byte sc1 buffer load per lane
//                             (8 line touches) instead of two 8-byte loads (16)
//   PBL_POOL_LB_ST16 1        a packed prefix is one 16-byte sc1 store, not two
//                             8-byte ones
//   PBL_POOL_LB_LATER_LANES   64, 32 or 16: the records a resolve's first later
//                             trip loads (the median resolve needs 1-9 of them);
//                             a trip after a partial one that found no prefix is
//                             a full window again.  Needs PBL_POOL_LB_WIN_LATER 1.
// Per resolve (2 trips): 6 loads and 48 line touches before, 3 loads and 18-19
// line touches now.  Plain bench.py, config 2, GiB/s, one box, one session,
// parent 1509-1520 (profiles/r10/ab_variants.txt): each piece alone
// V16 1581, ST16 1593, 16 lanes 1628; V16 + ST16 1636; with 32 lanes 1684;
// all three at 16 lanes (shipped) 1700-1702; the same with a 3-window first
// trip 1716, which gains on config 2, hide 4 and mixed and loses 2 % on
// Zipf-sized blocks against 2-1 (above the parent everywhere): 2-1 stays.
#ifndef PBL_LB_V16
#define PBL_LB_V16 1
#endif
#ifndef PBL_POOL_LB_ST16
#define PBL_POOL_LB_ST16 1
#endif
#ifndef PBL_POOL_LB_LATER_LANES
#define PBL_POOL_LB_LATER_LANES 16
#endif
constexpr int kPoolLbF = (PBL_LB_V16 ? kLbV16 : 0) | (PBL_POOL_LB_ST16 ? kLbSt16 : 0);
constexpr int kPoolLbLaterLanes = kLbL2 ? kWave : PBL_POOL_LB_LATER_LANES;
constexpr int kPoolLbWin = PBL_POOL_LB_WIN;
// (the two-level form's windows must reach the chunk edge: it keeps the first count)
constexpr int kPoolLbWinLater = kLbL2 ? kPoolLbWin : PBL_POOL_LB_WIN_LATER;
constexpr int kEarlyRel = PBL_POOL_EARLYREL;
constexpr uint32_t kPrefetch = PBL_POOL_PREFETCH;
constexpr int kNW = PBL_POOL_WAVES;      // waves per workgroup (one workgroup per CU)
constexpr int kNS = PBL_POOL_STAGES;     // staging buffers per workgroup
constexpr int kTPBP = kNW * kWave;
constexpr uint32_t kMaxKl = 4095;        // internal-key bytes per entry on the fast path

// A stage: the block, byte i at kPad + (boff & 15) + i.
struct Stage {
  uint4 x[kLdsBlkBytes / 16];
};

// Per-entry metadata word (m0): key source offset (15 bits: blocks <= 32 KiB),
// shared length (12), internal key length (12), prefix parent (9), entry
// header length (4), PBL_KV_* flags (8; OBSOLETE is added at emit time).
__device__ __forceinline__ uint32_t m_ksrc(uint64_t m) { return uint32_t(m) & 0x7fffu; }
__device__ __forceinline__ uint32_t m_sh(uint64_t m) { return uint32_t(m >> 15) & 0xfffu; }
__device__ __forceinline__ uint32_t m_klen(uint64_t m) { return uint32_t(m >> 27) & 0xfffu; }
__device__ __forceinline__ uint32_t m_par(uint64_t m) { return uint32_t(m >> 39) & 0x1ffu; }
__device__ __forceinline__ uint32_t m_hl(uint64_t m) { return uint32_t(m >> 48) & 0xfu; }
__device__ __forceinline__ uint32_t m_fl(uint64_t m) { return uint32_t(m >> 52) & 0xffu; }
__device__ __forceinline__ uint64_t m_pack(uint32_t ksrc, uint32_t sh, uint32_t kl, uint32_t par, uint32_t hl,
                                           uint32_t fl) {
  return uint64_t(ksrc) | uint64_t(sh) << 15 | uint64_t(kl) << 27 | uint64_t(par) << 39 | uint64_t(hl) << 48 |
         uint64_t(fl) << 52;
}

// A slot (one block's metadata, what the emits need after the stage is gone):
// m0 by entry (the prefix-parent chain runs over every entry), vp and ent by
// visible KV (HideObsoletePoints drops obsolete entries from the outputs, never
// from the chain; without hiding the two indices agree).  Entries per slot:
// what the LDS left after the stages holds, at most 511 (the parent field).
constexpr int kPerSlot = (163840 - kNS * int(sizeof(Stage)) - 256) / kNW;
template <bool kHide>
constexpr int slot_kv() {
  const int n = ((kPerSlot - 32) / (kHide ? 14 : 12)) & ~7;
  return n > 511 ? 511 : n;
}
template <bool kHide>
struct Slot {
  static constexpr int kKv = slot_kv<kHide>();
  uint64_t m0[kKv];
  uint32_t vp[kKv + 5];  // value output offset | value source offset << 16;
                         // entries nkv..nkv+4 hold the value total
  uint16_t ent[kHide ? kKv : 1];  // the entry of visible KV v
};

template <bool kHide>
struct PoolLds {
  Stage st[kNS];
  Slot<kHide> sl[kNW];
  uint32_t free_mask;  // bit s: stage s is free
};
static_assert(sizeof(PoolLds<true>) <= 163840 && sizeof(PoolLds<false>) <= 163840, "one pool workgroup per CU");

typedef u32x4 u32x4_ug __attribute__((aligned(1)));
typedef uint32_t u32_ug __attribute__((aligned(1)));
typedef uint64_t u64_ug __attribute__((aligned(1)));
typedef uint16_t u16_ug __attribute__((aligned(1)));

// Inclusive wave scan by DPP row shifts and row broadcasts (no ds_bpermute).
__device__ __forceinline__ uint32_t dpp_incl_scan(uint32_t v) {
  v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
  v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return v;
}
__device__ __forceinline__ uint32_t last_lane(uint32_t v) { return __builtin_amdgcn_readlane(v, kWave - 1); }

// Output stores.  PBL_POOL_NT: non-temporal (streaming) stores, so the
// outputs do not displace the staged blocks' lines that the emit re-reads
// from L2 (A/B).
#ifndef PBL_POOL_NT
#define PBL_POOL_NT 1  // measured: config 2 1200 vs 1183, config 4 1073 vs 1062 GiB/s
#endif
template <class T>
__device__ __forceinline__ void st_out(gptr<T> p, T v) {
#if PBL_POOL_NT
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}

// PBL_POOL_SBASE: the emit's global accesses address a wave-uniform base held
// in SGPRs plus an unsigned 32-bit lane offset (global_load / global_store
// "v_off, s[base:base+1]": no 64-bit address pair built per access).  The
// block's exclusive bases and source pointer go through readfirstlane once.
#ifndef PBL_POOL_SBASE
#define PBL_POOL_SBASE 0  // compiled out: no gain alone or on top of the other two
#endif
// PBL_POOL_VFAST: an emit step whose 64 values are all empty or 16..128 B
// long copies them as straight-line code, the descriptors read from the slot
// once, lane per KV, and handed to the 8-lane groups by cross-lane permutes.
#ifndef PBL_POOL_VFAST
#define PBL_POOL_VFAST 1
#endif
constexpr bool kSBase = PBL_POOL_SBASE != 0;
constexpr bool kVFast = PBL_POOL_VFAST != 0;

// A wave-uniform value / pointer moved to SGPRs (kOn false: as it is).
template <bool kOn>
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  if (!kOn) return v;
  return uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))))) |
         uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))))) << 32;
}
template <bool kOn, class T>
__device__ __forceinline__ gptr<T> ubase(gptr<T> p) {
  return (gptr<T>)uni64<kOn>((uint64_t)p);
}

// Bytes [0, n) of w (n <= 16) to b + off, any alignment: one 16-B store when
// whole, else the fewest 8/4/2/1-B stores (nothing past n: the next key
// belongs to another lane).
__device__ __forceinline__ void store_n(gptr<uint8_t> b, uint32_t off, const uint4& w, uint32_t n) {
  if (n == 16) {
    st_out((gptr<u32x4_ug>)(b + off), u32x4_ug{w.x, w.y, w.z, w.w});
    return;
  }
  uint64_t lo = uint64_t(w.x) | uint64_t(w.y) << 32, hi = uint64_t(w.z) | uint64_t(w.w) << 32;
  uint32_t o = off;
  if (n & 8) {
    st_out((gptr<u64_ug>)(b + o), u64_ug(lo));
    lo = hi;
    o += 8;
  }
  if (n & 4) {
    st_out((gptr<u32_ug>)(b + o), u32_ug(lo));
    lo >>= 32;
    o += 4;
  }
  if (n & 2) {
    st_out((gptr<u16_ug>)(b + o), u16_ug(lo));
    lo >>= 16;
    o += 2;
  }
  if (n & 1) st_out(b + o, uint8_t(lo));
}

__device__ __forceinline__ void store_n(gptr<uint8_t> p, const uint4& w, uint32_t n) {
  if (n == 16) {
    st_out((gptr<u32x4_ug>)p, u32x4_ug{w.x, w.y, w.z, w.w});
    return;
  }
  uint64_t lo = uint64_t(w.x) | uint64_t(w.y) << 32, hi = uint64_t(w.z) | uint64_t(w.w) << 32;
  uint32_t o = 0;
  if (n & 8) {
    st_out((gptr<u64_ug>)p, u64_ug(lo));
    lo = hi;
    o = 8;
  }
  if (n & 4) {
    st_out((gptr<u32_ug>)(p + o), u32_ug(lo));
    lo >>= 32;
    o += 4;
  }
  if (n & 2) {
    st_out((gptr<u16_ug>)(p + o), u16_ug(lo));
    lo >>= 16;
    o += 2;
  }
  if (n & 1) st_out(p + o, uint8_t(lo));
}

// 16 bytes of the block in global memory at block offset i (any alignment,
// i may be up to 15 below 0 or end past the block: those bytes are
// don't-cares).  One unaligned load inside the block's 16-B granules; at the
// two edges the general path's aligned pair (never a byte outside them).
__device__ __forceinline__ uint4 gld16(gptr<const uint8_t> g, int32_t i, uint32_t blen, uint32_t end16) {
  if (i >= 0 && uint32_t(i) + 16u <= end16) {
    const u32x4 v = *(gptr<const u32x4_ug>)(g + uint32_t(i));
    return make_uint4(v.x, v.y, v.z, v.w);
  }
  return GlbBlk{g, blen}.ld16(i);
}

// ---- the walk: lane per restart run ------------------------------------------
// Entries are indexed in block order (the prefix-parent chain runs over every
// entry); outputs by visible index (HideObsoletePoints drops obsolete entries
// from the outputs, never from the chain).  Without hiding the two agree.
struct PAcc {
  uint32_t ne, cnt, kb, vb;  // entries, visible KVs, their user-key / value bytes
};
#ifndef PBL_POOL_RUNBUF
#define PBL_POOL_RUNBUF 16  // entries of a run parked in registers by its walk
#endif
constexpr int kRunBuf = PBL_POOL_RUNBUF;
// One run's head, parked in registers by the walk for the metadata pass.
struct PRun {
  uint32_t ea[kRunBuf];  // entry offset | hidden << 15 | shared << 16 | SET-with-value-prefix << 31
  uint32_t eb[kRunBuf];  // unshared | header length << 14 | value length << 17
  uint32_t n, rw, pos, e0, prev_kl, prev_kind;  // parked entries; where a longer run continues
};

// Whether an entry is hidden (HideObsoletePoints: the trailer's kind byte has
// the obsolete bit, rowblk_iter.go:1168-1179) and whether its value carries a
// value prefix (kind SET, :1192-1199).  The kind byte sits at key byte kl - 8:
// in the entry's unshared bytes, or inside the shared prefix, where it is the
// previous key's kind byte if that key has the same length.  Returns false
// when the byte is elsewhere (the general walk takes the block).
template <bool kHide>
__device__ __forceinline__ bool entry_class(const View& V, uint32_t pos, uint32_t h, uint32_t sh, uint32_t kl,
                                            uint32_t k, uint32_t prev_kl, uint32_t& prev_kind, uint32_t flags,
                                            bool vprefix, bool& hidden, bool& setv) {
  hidden = false;
  setv = false;
  if ((kHide || vprefix) && kl >= 8 && !(flags & PBL_ROW_RAW_KEYS)) {
    uint32_t kind;
    if (kl - 8 >= sh) kind = V.byte(pos + h + (kl - 8 - sh));
    else if (k > 0 && prev_kl == kl) kind = prev_kind;
    else return false;
    hidden = kHide && (kind & 64u);
    setv = vprefix && !hidden && (kind & 0xBFu) == 1;
    prev_kind = kind;
  }
  return true;
}

__device__ __forceinline__ uint32_t ukey_len(uint32_t kl, uint32_t flags) {
  return (flags & PBL_ROW_RAW_KEYS) ? kl : (kl >= 8 ? kl - 8 : 0);
}

// Count entries [pos, e0) of a run whose first k entries were already counted
// (prev_kl / prev_kind: the last one's).  `ok` clears where the run is not
// walkable per run, `bad` sets on shared > len(previous key) (rowblk_iter.go:
// 403), `vbad` on a visible SET value without its prefix byte.
template <bool kHide>
__device__ __forceinline__ void count_span(const View& V, uint32_t pos, uint32_t e0, uint32_t k, uint32_t prev_kl,
                                           uint32_t prev_kind, uint32_t flags, bool vprefix, PAcc& acc, bool& ok,
                                           bool& bad, bool& vbad) {
  while (pos < e0) {
    uint32_t sh, un, vl, h;
    const bool hok = hdr2(V.ld8(pos), &sh, &un, &vl, &h);
    const uint32_t np = pos + h + un + vl;  // < 2^23: no overflow
    if (!hok || (k == 0 && sh != 0) || np > e0) { ok = false; return; }
    bad = bad || (k > 0 && sh > prev_kl);
    const uint32_t kl = sh + un;
    bool hidden, setv;
    if (kl > kMaxKl || !entry_class<kHide>(V, pos, h, sh, kl, k, prev_kl, prev_kind, flags, vprefix, hidden, setv)) {
      ok = false;
      return;
    }
    uint32_t vlen = vl;
    if (setv) {
      if (vl == 0) vbad = true;
      else if ((V.byte(pos + h + un) & 0xC0) == 0 || (flags & PBL_ROW_NO_VALUER)) vlen--;
    }
    acc.ne++;
    if (!hidden) {
      acc.cnt++;
      acc.kb += ukey_len(kl, flags);
      acc.vb += vlen;
    }
    k++;
    prev_kl = kl;
    pos = np;
  }
}

__device__ __forceinline__ bool run_bounds(const View& V, uint32_t r, uint32_t nres, uint32_t roff, uint32_t* rw,
                                           uint32_t* e0) {
  const uint32_t st = roff + 4 * r;
  *rw = V.le32(st);
  const uint32_t s0 = *rw & kRestartMask;
  *e0 = (r + 1 < nres) ? (V.le32(st + 4) & kRestartMask) : roff;
  return (r != 0 || s0 == 0) && s0 < *e0 && *e0 <= roff;
}

// Walk run r once, its first kRunBuf entries parked in registers (static
// indices: no scratch); `over` sets if the run is longer.
template <bool kHide>
__device__ __forceinline__ void run_walk(const View& V, uint32_t r, uint32_t nres, uint32_t roff, uint32_t flags,
                                         bool vprefix, PRun& B, PAcc& acc, bool& ok, bool& bad, bool& vbad,
                                         bool& over) {
  B.n = 0;
  uint32_t e0;
  if (!run_bounds(V, r, nres, roff, &B.rw, &e0)) { ok = false; return; }
  uint32_t pos = B.rw & kRestartMask, n = 0, prev_kl = 0, prev_kind = 0;
  bool go = true;
#pragma unroll
  for (int k = 0; k < kRunBuf; k++) {
    if (go && pos < e0) {
      uint32_t sh, un, vl, h;
      const bool hok = hdr2(V.ld8(pos), &sh, &un, &vl, &h);
      const uint32_t np = pos + h + un + vl;
      bool hidden = false, setv = false;
      if (!hok || (k == 0 && sh != 0) || np > e0) {
        ok = false;
        go = false;
      } else {
        bad = bad || (k > 0 && sh > prev_kl);
        const uint32_t kl = sh + un;
        if (kl > kMaxKl ||
            !entry_class<kHide>(V, pos, h, sh, kl, uint32_t(k), prev_kl, prev_kind, flags, vprefix, hidden, setv)) {
          ok = false;
          go = false;
        } else {
          uint32_t vlen = vl;
          if (setv) {
            if (vl == 0) vbad = true;
            else if ((V.byte(pos + h + un) & 0xC0) == 0 || (flags & PBL_ROW_NO_VALUER)) vlen--;
          }
          B.ea[k] = pos | uint32_t(hidden) << 15 | sh << 16 | uint32_t(setv) << 31;
          B.eb[k] = un | (h << 14) | (vl << 17);
          acc.ne++;
          if (!hidden) {
            acc.cnt++;
            acc.kb += ukey_len(kl, flags);
            acc.vb += vlen;
          }
          n++;
          prev_kl = kl;
          pos = np;
        }
      }
    }
  }
  if (go && pos < e0) over = true;
  B.n = n;
  B.pos = pos;
  B.e0 = e0;
  B.prev_kl = prev_kl;
  B.prev_kind = prev_kind;
}

// Chain and output state of the metadata pass, carried from one entry of a run
// to the next: entry / visible index, value output offset, the previous
// entry's shared length, its prefix parent and that parent's shared length.
struct MState {
  uint32_t e, v, vb, prev_sh, pp, ppsh;
};

// Metadata of one entry (validated by the walk).  The prefix parent is the
// nearest earlier entry of the run with a smaller shared length (all-nearest-
// smaller-values over the parents, amortised O(1)).
template <bool kHide>
__device__ __forceinline__ void entry_meta(Slot<kHide>& W, const View& V, uint32_t pos, bool hidden, uint32_t sh,
                                           uint32_t un, uint32_t h, uint32_t vl, bool setv, bool first, uint32_t rw,
                                           uint32_t flags, MState& M) {
  const uint32_t kl = sh + un;
  uint32_t par = M.e, parsh = 0;
  if (sh != 0) {
    uint32_t c = M.e - 1, csh = M.prev_sh;
    if (csh >= sh) { c = M.pp; csh = M.ppsh; }
    while (csh >= sh) {
      c = m_par(W.m0[c]);
      csh = m_sh(W.m0[c]);
    }
    par = c;
    parsh = csh;
  }
  uint32_t vs = pos + h + un, vlen = vl, fl = 0;
  if (first) fl = PBL_KV_RESTART | ((rw >> 31) ? PBL_KV_RESTART_SAMEPFX : 0u);
  if (!(flags & PBL_ROW_RAW_KEYS) && kl < 8) fl |= PBL_KV_INVALID_KEY;
  if (setv) {
    const uint32_t pre = V.byte(vs);
    if ((pre & 0xC0) == 0 || (flags & PBL_ROW_NO_VALUER)) { vs++; vlen--; }
    else if ((pre & 0xC0) == 0x80) fl |= PBL_KV_VALBLK_HANDLE;
    else fl |= PBL_KV_BLOB_HANDLE;
  }
  W.m0[M.e] = m_pack(pos + h, sh, kl, par, h, fl);
  if (!(kHide && hidden)) {
    if (kHide) W.ent[M.v] = uint16_t(M.e);
    W.vp[M.v] = M.vb | (vs << 16);
    M.vb += vlen;
    M.v++;
  }
  M.prev_sh = sh;
  M.pp = par;
  M.ppsh = parsh;
  M.e++;
}

// Metadata of the parked entries of a run.
template <bool kHide>
__device__ __forceinline__ void park_meta(Slot<kHide>& W, const View& V, const PRun& B, uint32_t flags, MState& M) {
#pragma unroll
  for (int k = 0; k < kRunBuf; k++) {
    if (uint32_t(k) < B.n)
      entry_meta<kHide>(W, V, B.ea[k] & 0x7fffu, (B.ea[k] >> 15) & 1u, (B.ea[k] >> 16) & 0x7fffu,
                        B.eb[k] & 0x3fffu, (B.eb[k] >> 14) & 7u, B.eb[k] >> 17, B.ea[k] >> 31, k == 0, B.rw, flags, M);
  }
}

// Metadata of entries [pos, e0) of a run, re-read from the stage (k = entries
// of the run before pos; prev_kl / prev_kind: the last one's).
template <bool kHide>
__device__ __forceinline__ void span_meta(Slot<kHide>& W, const View& V, uint32_t pos, uint32_t e0, uint32_t rw,
                                          uint32_t k, uint32_t prev_kl, uint32_t prev_kind, uint32_t flags,
                                          bool vprefix, MState& M) {
  while (pos < e0) {
    uint32_t sh, un, vl, h;
    hdr2(V.ld8(pos), &sh, &un, &vl, &h);
    const uint32_t kl = sh + un;
    bool hidden, setv;
    entry_class<kHide>(V, pos, h, sh, kl, k, prev_kl, prev_kind, flags, vprefix, hidden, setv);
    entry_meta<kHide>(W, V, pos, hidden, sh, un, h, vl, setv, k == 0, rw, flags, M);
    k++;
    prev_kl = kl;
    pos = pos + h + un + vl;
  }
}

// A lane's runs [r0, r1) walked and counted into acc.  `single` (one run per
// lane at most): the run's head is parked in RB; a run longer than kRunBuf
// keeps its parked head and counts only its tail.
template <bool kHide>
__device__ __forceinline__ void walk_runs(const View& V, uint32_t r0, uint32_t r1, uint32_t nres, uint32_t roff,
                                          uint32_t flags, bool vprefix, bool single, PRun& RB, PAcc& acc, bool& ok,
                                          bool& bad, bool& vbad, bool& over) {
  if (single) {
    if (r0 < nres) run_walk<kHide>(V, r0, nres, roff, flags, vprefix, RB, acc, ok, bad, vbad, over);
    if (over && ok)
      count_span<kHide>(V, RB.pos, RB.e0, RB.n, RB.prev_kl, RB.prev_kind, flags, vprefix, acc, ok, bad, vbad);
    return;
  }
  for (uint32_t r = r0; r < r1 && ok; r++) {
    uint32_t rw, e0;
    if (!run_bounds(V, r, nres, roff, &rw, &e0)) ok = false;
    else count_span<kHide>(V, rw & kRestartMask, e0, 0, 0, 0, flags, vprefix, acc, ok, bad, vbad);
  }
}

// The metadata of the runs walk_runs accepted, M placed at the lane's first entry.
template <bool kHide>
__device__ __forceinline__ void meta_runs(Slot<kHide>& W, const View& V, uint32_t r0, uint32_t r1, uint32_t nres,
                                          uint32_t roff, uint32_t flags, bool vprefix, bool single, bool over,
                                          const PRun& RB, MState& M) {
  if (single) {
    if (r0 >= nres) return;
    park_meta<kHide>(W, V, RB, flags, M);
    if (over) span_meta<kHide>(W, V, RB.pos, RB.e0, RB.rw, RB.n, RB.prev_kl, RB.prev_kind, flags, vprefix, M);
    return;
  }
  for (uint32_t r = r0; r < r1; r++) {
    uint32_t rw, e0;
    run_bounds(V, r, nres, roff, &rw, &e0);
    M.prev_sh = M.pp = M.ppsh = 0;
    span_meta<kHide>(W, V, rw & kRestartMask, e0, rw, 0, 0, 0, flags, vprefix, M);
  }
}

// ---- the pool kernel's own front (PBL_POOL_FRONT) ----
// The same walk and metadata pass for the one-run-per-lane case, written so
// that the lanes execute fewer instructions and waits: every value, every
// fallback and the slot layout are the forms' above (which the row-wave and
// mixed kernels keep).
//   walk   one entry's body is straight-line: a lane past its run's end, or
//          one that has failed, goes on with pos clamped to the restart table
//          (inside the stage) and its results unused; the failure causes are
//          OR-ed into flags looked at once after the loop.  Whether entries
//          need their kind byte at all (kCls) is decided per block, and the
//          header's three-one-byte-varints form by a ballot of the live lanes.
//   meta   the parked entries are 16 flat bodies, the state carried by plain
//          arithmetic (a lane's parked entries are its first B.n, so nothing
//          after them reads it), the stores alone under `k < B.n`; the value-
//          prefix byte only in the kVp form; m0 built as two 32-bit halves.
// 0: the shared forms, as before round 12.
#ifndef PBL_POOL_FRONT
#define PBL_POOL_FRONT 1
#endif
constexpr bool kFront = PBL_POOL_FRONT != 0;

// hdr3 out of line (the walk's 16 unrolled entries would each carry a copy of
// a form that few blocks reach): shared, unshared, value length, header length
// | ok << 3.  One- and two-byte varints included: what hdr2 returns.
__device__ __noinline__ uint4 hdr3_out(uint64_t w) {
  uint32_t sh, un, vl, h;
  const bool ok = hdr3(w, &sh, &un, &vl, &h);
  return make_uint4(sh, un, vl, (h & 7u) | uint32_t(ok) << 3);
}

// hdr2 for a whole wave: the one-byte form when every live lane has it (no
// divergent region), the branch-free 1..3-byte form for all lanes otherwise.
__device__ __forceinline__ bool hdr2_wave(uint64_t w, bool live, uint32_t* sh, uint32_t* un, uint32_t* vl,
                                          uint32_t* h) {
  if (__builtin_amdgcn_ballot_w64(live && (uint32_t(w) & 0x808080u) != 0) == 0) {
    *sh = uint32_t(w) & 0xffu;
    *un = uint32_t(w >> 8) & 0xffu;
    *vl = uint32_t(w >> 16) & 0xffu;
    *h = 3;
    return true;
  }
  const uint4 r = hdr3_out(w);
  *sh = r.x;
  *un = r.y;
  *vl = r.z;
  *h = r.w & 7u;
  return (r.w >> 3) != 0;
}

// run_walk for every lane of the wave at once (r >= nres: a lane without a
// run).  kCls: entries are classified by their kind byte (entry_class's rules).
template <bool kHide, bool kCls>
__device__ __forceinline__ void run_walk_flat(const View& V, uint32_t r, uint32_t nres, uint32_t roff, uint32_t flags,
                                              bool vprefix, PRun& B, PAcc& acc, bool& ok, bool& bad, bool& vbad,
                                              bool& over) {
  // run_bounds: both restart words in one read (the last run's second word is
  // the block's restart count: inside the block)
  const uint32_t rc = min(r, nres - 1);
  const uint64_t two = V.ld8(roff + 4 * rc);
  B.rw = uint32_t(two);
  const uint32_t s0 = B.rw & kRestartMask;
  const uint32_t e0 = rc + 1 < nres ? (uint32_t(two >> 32) & kRestartMask) : roff;
  const bool bok = (rc != 0 || s0 == 0) && s0 < e0 && e0 <= roff;
  const uint32_t tsub = (flags & PBL_ROW_RAW_KEYS) ? 0u : 8u;  // trailer bytes of a key
  bool live = r < nres && bok, fail = r < nres && !bok;
  // pos stays inside [0, roff] whatever the lane has read (a lane that is not
  // live reads some 8 bytes of the block), so the next entry's read waits for
  // this entry's lengths only, not for its checks
  uint32_t pos = min(s0, roff), n = 0, cnt = 0, kb = 0, vb = 0, prev_kl = 0, prev_kind = 0;
#pragma unroll
  for (int k = 0; k < kRunBuf; k++) {
    const uint32_t p = pos;
    uint32_t sh, un, vl, h;
    const bool hok = hdr2_wave(V.ld8(p), live, &sh, &un, &vl, &h);
    const uint32_t np = p + h + un + vl;  // < 2^23: no overflow
    const uint32_t kl = sh + un;
    const bool g1 = hok && (k != 0 || sh == 0) && np <= e0;
    if (k > 0) bad = bad || (live && g1 && sh > prev_kl);
    bool g2 = g1 && kl <= kMaxKl, hidden = false, setv = false;
    uint32_t vlen = vl;
    if constexpr (kCls) {
      // the kind byte: key byte kl - 8, among the unshared bytes (un >= 8) or
      // the previous key's when that has the same length
      const bool has = kl >= 8, own = kl >= sh + 8;
      const uint32_t kbyte = V.byte(live && g2 && own ? p + h + (un - 8) : 0u);  // < np <= e0
      const uint32_t kind = own ? kbyte : prev_kind;
      g2 = g2 && (!has || own || (k > 0 && prev_kl == kl));
      hidden = kHide && has && (kind & 64u);
      setv = vprefix && has && !hidden && (kind & 0xBFu) == 1;
      prev_kind = has ? kind : prev_kind;
      if (vprefix) {  // uniform
        const bool rd = live && g2 && setv;
        vbad = vbad || (rd && vl == 0);
        const uint32_t pre = V.byte(rd && vl != 0 ? p + h + un : 0u);  // < np <= e0
        if (rd && vl != 0 && ((pre & 0xC0) == 0 || (flags & PBL_ROW_NO_VALUER))) vlen--;
      }
    }
    const bool take = live && g2, vis = take && !hidden;
    fail = fail || (live && !g2);
    B.ea[k] = p | uint32_t(hidden) << 15 | sh << 16 | uint32_t(setv) << 31;
    B.eb[k] = un | (h << 14) | (vl << 17);
    n += take;
    cnt += vis;
    kb += vis ? kl - min(kl, tsub) : 0u;
    vb += vis ? vlen : 0u;
    prev_kl = kl;
    pos = min(np, roff);  // (live: np < e0 <= roff)
    live = take && np < e0;
  }
  if (live) over = true;
  if (fail) ok = false;
  acc.ne += n;
  acc.cnt += cnt;
  acc.kb += kb;
  acc.vb += vb;
  B.n = n;
  B.pos = pos;
  B.e0 = e0;
  B.prev_kl = prev_kl;
  B.prev_kind = prev_kind;
}

// park_meta as flat bodies.  kVp: SET values carry a value prefix (the one
// form that reads the stage).
template <bool kHide, bool kVp>
__device__ __forceinline__ void park_meta_flat(Slot<kHide>& W, const View& V, const PRun& B, uint32_t flags,
                                               MState& M) {
  const uint32_t tmin = (flags & PBL_ROW_RAW_KEYS) ? 0u : 8u;
  const uint32_t fl0 = PBL_KV_RESTART | ((B.rw >> 31) ? PBL_KV_RESTART_SAMEPFX : 0u);
#pragma unroll
  for (int k = 0; k < kRunBuf; k++) {
    const uint32_t ea = B.ea[k], eb = B.eb[k];
    const uint32_t pos = ea & 0x7fffu, sh = (ea >> 16) & 0x7fffu, un = eb & 0x3fffu, h = (eb >> 14) & 7u, vl = eb >> 17;
    const bool on = uint32_t(k) < B.n, hidden = kHide && ((ea >> 15) & 1u);
    const uint32_t kl = sh + un;
    uint32_t par = M.e, parsh = 0;
    if (k > 0) {  // (a run's first entry shares nothing)
      const bool up = M.prev_sh >= sh;
      uint32_t c = up ? M.pp : M.e - 1, csh = up ? M.ppsh : M.prev_sh;
      if (on && sh != 0) {
        while (csh >= sh) {
          c = m_par(W.m0[c]);
          csh = m_sh(W.m0[c]);
        }
      }
      par = sh != 0 ? c : M.e;
      parsh = sh != 0 ? csh : 0u;
    }
    uint32_t vs = pos + h + un, vlen = vl, fl = k == 0 ? fl0 : 0u;
    if (kl < tmin) fl |= PBL_KV_INVALID_KEY;
    if constexpr (kVp) {
      const bool setv = on && (ea >> 31);
      const uint32_t pre = V.byte(setv ? vs : 0u);
      const bool strip = (pre & 0xC0) == 0 || (flags & PBL_ROW_NO_VALUER);
      if (setv) {
        vs += strip;
        vlen -= strip;
        fl |= strip ? 0u : (pre & 0xC0) == 0x80 ? PBL_KV_VALBLK_HANDLE : PBL_KV_BLOB_HANDLE;
      }
    }
    // m_pack in halves: bit 32 falls inside the key length
    const uint32_t lo = (pos + h) | sh << 15 | kl << 27, hi = kl >> 5 | par << 7 | h << 16 | fl << 20;
    if (on) {
      W.m0[M.e] = uint64_t(hi) << 32 | lo;
      if (!hidden) {
        if (kHide) W.ent[M.v] = uint16_t(M.e);
        W.vp[M.v] = M.vb | (vs << 16);
      }
    }
    const bool vis = on && !hidden;
    M.vb += vis ? vlen : 0u;
    M.v += vis;
    M.prev_sh = sh;
    M.pp = par;
    M.ppsh = parsh;
    M.e += on;
  }
}

// walk_runs / meta_runs of the pool kernel: the flat forms where a lane has
// one run at most, the shared forms otherwise.
template <bool kHide>
__device__ __forceinline__ void front_walk(const View& V, uint32_t r0, uint32_t r1, uint32_t nres, uint32_t roff,
                                           uint32_t flags, bool vprefix, bool single, PRun& RB, PAcc& acc, bool& ok,
                                           bool& bad, bool& vbad, bool& over) {
  if (!kFront) {
    walk_runs<kHide>(V, r0, r1, nres, roff, flags, vprefix, single, RB, acc, ok, bad, vbad, over);
    return;
  }
  if (!single) {  // (the constant: the shared single-run form is not instantiated here)
    walk_runs<kHide>(V, r0, r1, nres, roff, flags, vprefix, false, RB, acc, ok, bad, vbad, over);
    return;
  }
  if ((kHide || vprefix) && !(flags & PBL_ROW_RAW_KEYS))
    run_walk_flat<kHide, true>(V, r0, nres, roff, flags, vprefix, RB, acc, ok, bad, vbad, over);
  else
    run_walk_flat<kHide, false>(V, r0, nres, roff, flags, vprefix, RB, acc, ok, bad, vbad, over);
  if (over && ok)
    count_span<kHide>(V, RB.pos, RB.e0, RB.n, RB.prev_kl, RB.prev_kind, flags, vprefix, acc, ok, bad, vbad);
}

template <bool kHide>
__device__ __forceinline__ void front_meta(Slot<kHide>& W, const View& V, uint32_t r0, uint32_t r1, uint32_t nres,
                                           uint32_t roff, uint32_t flags, bool vprefix, bool single, bool over,
                                           const PRun& RB, MState& M) {
  if (!kFront) {
    meta_runs<kHide>(W, V, r0, r1, nres, roff, flags, vprefix, single, over, RB, M);
    return;
  }
  if (!single) {
    meta_runs<kHide>(W, V, r0, r1, nres, roff, flags, vprefix, false, over, RB, M);
    return;
  }
  if (vprefix) park_meta_flat<kHide, true>(W, V, RB, flags, M);
  else park_meta_flat<kHide, false>(W, V, RB, flags, M);
  if (over) span_meta<kHide>(W, V, RB.pos, RB.e0, RB.rw, RB.n, RB.prev_kl, RB.prev_kind, flags, vprefix, M);
}

// The block's bytes in global memory for the emits (the stage is gone by
// then).  ld16 windows may start up to 15 bytes before the block.
struct GSrc {
  gptr<const uint8_t> g;
  uint32_t blen, end16;
  __device__ __forceinline__ uint32_t byte(uint32_t i) const { return g[i]; }
  __device__ __forceinline__ uint64_t ld8(uint32_t i) const { return *(gptr<const u64_ug>)(g + i); }
  __device__ __forceinline__ uint32_t le32(uint32_t i) const { return *(gptr<const u32_ug>)(g + i); }
  __device__ __forceinline__ uint4 ld16(int32_t i) const { return gld16(g, i, blen, end16); }
};

// byte p of the internal key of entry j (source = max{i <= j : shared_i <= p})
template <class Src>
__device__ __forceinline__ uint32_t key_byte(const uint64_t* M0, const Src& V, int j, uint32_t p) {
  uint64_t m = M0[j];
  while (p < m_sh(m)) m = M0[--j];
  return V.byte(m_ksrc(m) + p - m_sh(m));
}

template <class Src>
__device__ __forceinline__ uint64_t trailer_of(const uint64_t* M0, const Src& V, int j, uint64_t m, uint32_t* fl,
                                               uint32_t flags) {
  const uint32_t kl = m_klen(m), sh = m_sh(m);
  uint64_t raw = 0, t, ukl;
  if (!(flags & PBL_ROW_RAW_KEYS) && kl >= 8) {
    if (kl - 8 >= sh) raw = V.ld8(m_ksrc(m) + (kl - 8 - sh));
    else
      for (int i = 0; i < 8; i++) raw |= uint64_t(key_byte(M0, V, j, kl - 8 + i)) << (8 * i);
  }
  split_trailer(raw, kl, flags, &t, &ukl, fl);
  return t;
}

// Key bytes [c, c + n) of KV m (n <= 16) merged from the segments of its prefix
// chain: each a 16-B read that starts where the chunk's first byte would sit in
// that entry (at most 15 bytes before the block).
template <class Src>
__device__ __forceinline__ uint4 key_chunk(const uint64_t* M0, const Src& V, uint64_t m, uint32_t c, uint32_t n) {
  const uint32_t ce = c + n;
  uint32_t cur = ce;
  uint4 w = make_uint4(0, 0, 0, 0);
  for (;;) {
    const uint32_t shi = m_sh(m);
    const uint32_t lo_i = shi < cur ? shi : cur;
    const uint32_t a = lo_i > c ? lo_i : c;
    if (a < cur) {
      const uint4 v = V.ld16(int32_t(m_ksrc(m)) - int32_t(shi) + int32_t(c));
      if (a == c && cur - a == 16) return v;
      merge16(w, v, a - c, cur - c);
    }
    if (lo_i <= c) break;
    cur = lo_i;
    m = M0[m_par(m)];
  }
  return w;
}

// ---- keys: lane per KV, kKU KVs per lane per batch ---------------------------
// The loads are L2 / MALL round trips, so a batch goes through its metadata
// words (slot), then every global load (the trailer's 8 bytes; the user key's
// segments: its own unshared bytes and, for a key that shares a prefix, its
// prefix parent's bytes), then the merges and stores.  The fast form covers
// keys of at most 16 bytes whose prefix chain ends at the parent (a restart-
// interval row block: the parent is the run's first key) with the trailer in
// the entry's own bytes; the rest take the general form (trailer_of,
// key_chunk).  Only the loaded data and the words they were addressed by are
// held between the loads and the stores.
#ifndef PBL_POOL_KU
#define PBL_POOL_KU 1
#endif
constexpr int kKU = PBL_POOL_KU;
// PBL_POOL_KMETA 0: the metadata words are not held between a batch's loads
// and its stores (re-read from the slot: two LDS reads, fewer VGPRs per
// step in flight).
#ifndef PBL_POOL_KMETA
#define PBL_POOL_KMETA 1
#endif
struct KBatch {
#if PBL_POOL_KMETA
  uint64_t m[kKU], mp[kKU];
#endif
  uint64_t tr[kKU];
  uint4 ka[kKU], kp[kKU];
};
// The metadata word of visible KV j and its prefix parent's (0 past nkv).
template <bool kHide>
__device__ __forceinline__ void kv_meta(const Slot<kHide>& W, uint32_t j, uint32_t nkv, uint64_t* m, uint64_t* mp) {
  const uint32_t e = kHide ? (j < nkv ? uint32_t(W.ent[j]) : 0u) : j;
  *m = j < nkv ? W.m0[e] : 0ull;
  *mp = (j < nkv && m_sh(*m) != 0) ? W.m0[m_par(*m)] : 0ull;
}

__device__ __forceinline__ uint32_t ukl_of(uint64_t m, bool raw) {
  const uint32_t kl = m_klen(m);
  return raw ? kl : (kl >= 8 ? kl - 8 : 0u);
}
__device__ __forceinline__ bool key_fast(uint64_t m, uint64_t mp, bool raw) {
  const uint32_t kl = m_klen(m), sh = m_sh(m);
  return ukl_of(m, raw) <= 16 && (sh == 0 || m_sh(mp) == 0) && (raw || kl < 8 || kl - 8 >= sh);
}

// PBL_POOL_KWIN: a key is on the fast form only if its 16-B windows lie inside
// the block's 16-B granules, so key_load issues plain loads and nothing else:
// the edge form of GSrc::ld16 (an aligned pair merged after a vmcnt wait) inside
// it made the compiler drain every memory operation in flight, the previous
// step's stores included, between a step's key loads and its value loads.  A
// key at the block's edge takes the general form (same bytes, loaded at its
// stores).  Sources without edges (the stage in LDS): as before.
#ifndef PBL_POOL_KWIN
#define PBL_POOL_KWIN 1
#endif
constexpr bool kKWin = PBL_POOL_KWIN != 0;
template <class Src>
__device__ __forceinline__ bool win_in(const Src&, int32_t) { return true; }
__device__ __forceinline__ bool win_in(const GSrc& V, int32_t i) {
  return !kKWin || (i >= 0 && uint32_t(i) + 16u <= V.end16);
}
template <class Src>
__device__ __forceinline__ uint4 ld16_in(const Src& V, int32_t i) { return V.ld16(i); }
__device__ __forceinline__ uint4 ld16_in(const GSrc& V, int32_t i) {
  if (!kKWin) return V.ld16(i);
  const u32x4 v = *(gptr<const u32x4_ug>)(V.g + uint32_t(i));
  return make_uint4(v.x, v.y, v.z, v.w);
}
template <class Src>
__device__ __forceinline__ bool key_fast_at(const Src& V, uint64_t m, uint64_t mp, bool raw) {
  const uint32_t sh = m_sh(m);
  return key_fast(m, mp, raw) &&
         (ukl_of(m, raw) == 0 ||
          (win_in(V, int32_t(m_ksrc(m)) - int32_t(sh)) && (sh == 0 || win_in(V, int32_t(m_ksrc(mp))))));
}

template <bool kHide, class Src>
__device__ __forceinline__ void key_load(const Slot<kHide>& W, const Src& V, bool raw, uint32_t j0, uint32_t nkv,
                                         KBatch& K) {
  const int l = lane_id();
  uint64_t Km[kKU], Kmp[kKU];
#pragma unroll
  for (int u = 0; u < kKU; u++) kv_meta<kHide>(W, j0 + kWave * u + l, nkv, &Km[u], &Kmp[u]);
#if PBL_POOL_KMETA
#pragma unroll
  for (int u = 0; u < kKU; u++) {
    K.m[u] = Km[u];
    K.mp[u] = Kmp[u];
  }
#endif
#pragma unroll
  for (int u = 0; u < kKU; u++) {
    const uint32_t j = j0 + kWave * u + l;
    const uint64_t m = Km[u];
    const uint32_t kl = m_klen(m), sh = m_sh(m), ukl = ukl_of(m, raw);
    const bool fast = j < nkv && key_fast_at(V, m, Kmp[u], raw);
    K.tr[u] = 0;
    if (fast && !raw && kl >= 8) K.tr[u] = V.ld8(m_ksrc(m) + (kl - 8 - sh));
    if (fast && ukl) K.ka[u] = ld16_in(V, int32_t(m_ksrc(m)) - int32_t(sh));
    if (fast && ukl && sh) K.kp[u] = ld16_in(V, int32_t(m_ksrc(Kmp[u])));
  }
}

// A user key off the fast form (longer than 16 bytes, or a deeper prefix
// chain): the chunks that reach into the shared prefix are merged along the
// chain; the rest lie in the entry's own bytes and go four 16-B loads at a
// time (the loads of a step in flight together).
#ifndef PBL_POOL_KOWN
#define PBL_POOL_KOWN 4
#endif
// Keys whose own bytes run past kWaveKey leave those to the whole wave
// (wave_key_own): only the chunks that reach into the shared prefix are
// stored here.
#ifndef PBL_POOL_WAVEKEY
#define PBL_POOL_WAVEKEY 128
#endif
constexpr uint32_t kWaveKey = PBL_POOL_WAVEKEY;
__device__ __forceinline__ bool wave_key(uint32_t ukl, uint32_t sh) { return ukl > kWaveKey && ukl >= sh + 16; }
template <bool kOff, class Src>
__device__ __forceinline__ void store_key_general(const uint64_t* M0, const Src& V, uint64_t m, uint32_t ukl,
                                                  gptr<uint8_t> kbytes, uint32_t ko) {
  const gptr<uint8_t> dst = kbytes + ko;
  const uint32_t sh = m_sh(m);
  const int32_t own = int32_t(m_ksrc(m)) - int32_t(sh);  // block offset of key byte 0 in the entry's bytes
  uint32_t c = 0;
  for (; c < ukl && c < sh; c += 16) {
    const uint32_t n = ukl - c < 16 ? ukl - c : 16u;
    if (kOff) store_n(kbytes, ko + c, key_chunk(M0, V, m, c, n), n);
    else store_n(dst + c, key_chunk(M0, V, m, c, n), n);
  }
  if (wave_key(ukl, sh)) return;
  for (; c < ukl; c += 16 * PBL_POOL_KOWN) {
    uint4 w[PBL_POOL_KOWN];
#pragma unroll
    for (int k = 0; k < PBL_POOL_KOWN; k++) {
      const uint32_t cc = c + 16 * k;
      w[k] = cc < ukl ? V.ld16(own + int32_t(cc)) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < PBL_POOL_KOWN; k++) {
      const uint32_t cc = c + 16 * k;
      if (cc < ukl) {
        if (kOff) store_n(kbytes, ko + cc, w[k], ukl - cc < 16 ? ukl - cc : 16u);
        else store_n(dst + cc, w[k], ukl - cc < 16 ? ukl - cc : 16u);
      }
    }
  }
}

// The batch's stores.  Key output offsets: an exclusive wave scan of the user-
// key lengths per u, `kcar` carrying the running total (KV nkv gets the total).
// kPart (the two-pass row emit splits the stores over two waves): 0 all, 1 all
// but the long keys' own bytes, 2 only those (K unused).
// kOff (the pool kernel's emit): every store addresses the batch's base of
// its array plus the lane's unsigned 32-bit offset (the caller's b, j0, kvb and
// kbb are wave-uniform), the bases in SGPRs with PBL_POOL_SBASE.  kVo: the
// KVs' value offsets come in `vo` (the caller's one read of vp), kKU == 1.
template <bool kHide, class Src, int kPart = 0, bool kOff = false, bool kVo = false>
__device__ __forceinline__ void key_store(const Slot<kHide>& W, const Src& V, const Args& A, uint32_t b, uint32_t j0,
                                          uint32_t nkv, uint64_t kvb, uint64_t kbb, const KBatch& K, uint32_t& kcar,
                                          uint32_t vo = 0) {
  static_assert(!kVo || kKU == 1, "one value offset per lane");
  const int l = lane_id();
  const uint32_t flags = A.in.flags;
  const pbl_decode_out& O = A.out;
  constexpr bool kSB = kOff && kSBase;
  const gptr<uint8_t> kbytes = ubase<kSB>(to_glb(O.key_bytes) + kbb);
  // the batch's first element of every per-KV array
  const gptr<uint32_t> p_koff = ubase<kSB>(to_glb(O.key_off) + (kvb + b + j0));
  const gptr<uint32_t> p_voff = ubase<kSB>(to_glb(O.val_off) + (kvb + b + j0));
  const gptr<uint64_t> p_tr = ubase<kSB>(to_glb(O.trailer) + (kvb + j0));
  const gptr<uint8_t> p_fl = ubase<kSB>(to_glb(O.kv_flags) + (kvb + j0));
  const gptr<uint32_t> p_eo = ubase<kSB>(to_glb(O.entry_off) + (kvb + j0));
  const bool raw = (flags & PBL_ROW_RAW_KEYS) != 0;
  uint32_t kc0[kKU];
  uint64_t Km[kKU], Kmp[kKU];
#pragma unroll
  for (int u = 0; u < kKU; u++) {
#if PBL_POOL_KMETA
    if (kPart != 2) {
      Km[u] = K.m[u];
      Kmp[u] = K.mp[u];
      continue;
    }
#endif
    kv_meta<kHide>(W, j0 + kWave * u + l, nkv, &Km[u], &Kmp[u]);
  }
#pragma unroll
  for (int u = 0; u < kKU; u++) {
    const uint32_t lj = uint32_t(kWave * u + l), j = j0 + lj;
    const uint64_t m = Km[u];
    const uint32_t ukl = j < nkv ? ukl_of(m, raw) : 0u;
    const uint32_t incl = dpp_incl_scan(ukl);
    kc0[u] = kcar;
    const uint32_t ko = kcar + incl - ukl;
    kcar += last_lane(incl);
    if (kPart == 2 || j > nkv) continue;
    if (kOff) {
      st_out(p_koff + lj, ko);
      st_out(p_voff + lj, kVo ? vo : uint32_t(W.vp[j] & 0xffffu));
    } else {
      st_out(to_glb(O.key_off) + (kvb + b + j), ko);
      st_out(to_glb(O.val_off) + (kvb + b + j), uint32_t(W.vp[j] & 0xffffu));
    }
    if (j == nkv) continue;
    const uint32_t kl = m_klen(m), sh = m_sh(m);
    uint64_t t;
    uint32_t f = m_fl(m);
    if (!key_fast_at(V, m, Kmp[u], raw)) {
      const uint32_t e = kHide ? uint32_t(W.ent[j]) : j;
      t = trailer_of(W.m0, V, int(e), m, &f, flags);
      store_key_general<kOff>(W.m0, V, m, ukl, kbytes, ko);
    } else {
      uint64_t tukl;
      split_trailer(K.tr[u], kl, flags, &t, &tukl, &f);
      if (ukl) {
        const uint32_t lo = sh < ukl ? sh : ukl;
        uint4 w = K.ka[u];
        if (lo) {
          w = make_uint4(0, 0, 0, 0);
          merge16(w, K.ka[u], lo, ukl);
          merge16(w, K.kp[u], 0, lo);
        }
        if (kOff) store_n(kbytes, ko, w, ukl);
        else store_n(kbytes + ko, w, ukl);
      }
    }
    if (kOff) {
      st_out(p_tr + lj, uint64_t(with_seq(t, A.in.synthetic_seq_num, flags)));
      if (O.kv_flags) st_out(p_fl + lj, uint8_t(f));
      if (O.entry_off) st_out(p_eo + lj, uint32_t(m_ksrc(m) - m_hl(m)));
    } else {
      st_out(to_glb(O.trailer) + (kvb + j), uint64_t(with_seq(t, A.in.synthetic_seq_num, flags)));
      if (O.kv_flags) st_out(to_glb(O.kv_flags) + (kvb + j), uint8_t(f));
      if (O.entry_off) st_out(to_glb(O.entry_off) + (kvb + j), uint32_t(m_ksrc(m) - m_hl(m)));
    }
  }
  if (kPart == 1) return;
  // the own bytes [shared, ukl) of long keys: one contiguous range of the
  // entry each, copied by the whole wave (16-B chunks, the last one ending at
  // the key's end, four per lane in flight)
#pragma unroll
  for (int u = 0; u < kKU; u++) {
    const uint32_t j = j0 + kWave * u + l;
    const uint64_t m = Km[u];
    const uint32_t ukl = j < nkv ? ukl_of(m, raw) : 0u, sh = m_sh(m);
    const bool wk = j < nkv && !key_fast(m, Kmp[u], raw) && wave_key(ukl, sh);
    const uint32_t incl = dpp_incl_scan(ukl);  // (the batch's key offsets again)
    const uint32_t ko = kc0[u] + incl - ukl;
    for (uint64_t lm = __ballot(wk); lm; lm &= lm - 1) {
      const int sl = __builtin_ctzll(lm);
      const int32_t src = __shfl(int32_t(m_ksrc(m)), sl, kWave);
      const uint32_t len = __shfl(ukl - sh, sl, kWave), dst = __shfl(ko + sh, sl, kWave);
      for (uint32_t o0 = 16u * l; o0 < len; o0 += 64u * kWave) {
        uint4 y[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t o = o0 + 16u * kWave * k, q = o < len - 16 ? o : len - 16;
          y[k] = V.ld16(src + int32_t(o < len ? q : 0u));
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t o = o0 + 16u * kWave * k, q = o < len - 16 ? o : len - 16;
          if (o < len) st_out((gptr<u32x4_ug>)(kbytes + dst + q), u32x4_ug{y[k].x, y[k].y, y[k].z, y[k].w});
        }
      }
    }
  }
}

// Value bytes of a block, 8 lanes per KV: lane c of a group copies its
// value's 16-B chunks c, c + 8, ... from the block in global memory to the
// output with plain (unaligned) 16-B loads and stores.  A value's last chunk
// is the one that ENDS at the value's end, overlapping the chunk before it, so
// every store writes bytes of its own value only and no store is partial.
// kVG KVs per group per step, all their first chunks loaded before any store:
// the loads are L2 / MALL round trips, and a step costs about one of them.
// Values shorter than 16 B go byte by byte; values longer than kWaveVal are
// copied by the whole wave, four 16-B chunks per lane in flight.
#ifndef PBL_POOL_VG
#define PBL_POOL_VG 8
#endif
constexpr int kVG = PBL_POOL_VG;
#ifndef PBL_POOL_WAVEVAL
#define PBL_POOL_WAVEVAL 1024
#endif
constexpr uint32_t kWaveVal = PBL_POOL_WAVEVAL;
#ifndef PBL_POOL_MEDU
#define PBL_POOL_MEDU 4
#endif
constexpr int kMedU = PBL_POOL_MEDU;  // chunks per lane in flight for values of 129 B .. kWaveVal
// One step of the value copy: kVG KVs per 8-lane group, j = j0 + 8 u + lane / 8.
// Only the loaded chunks are held between a step's loads and its stores (the
// offsets are re-read from the slot).
struct VBatch {
  u32x4 x[kVG];
};
struct VSeg {
  uint32_t vo, vl, vs, q;
  bool has;
};
__device__ __forceinline__ VSeg val_seg(const uint32_t* vp, uint32_t nkv, uint32_t j) {
  const uint32_t c = uint32_t(lane_id()) & 7u;
  const uint32_t a = j < nkv ? vp[j] : 0u, z = j < nkv ? vp[j + 1] : 0u;
  VSeg S;
  S.vo = a & 0xffffu;
  S.vl = (z & 0xffffu) - S.vo;
  S.vs = a >> 16;
  S.has = S.vl >= 16 && S.vl <= kWaveVal && 16 * c < S.vl;
  S.q = S.has ? (16 * c < S.vl - 16 ? 16 * c : S.vl - 16) : 0u;
  return S;
}

// The step's first chunks from the block (every lane loads, from the block's
// first 16-B aligned granule when it has no chunk: no conditionally defined
// registers, and no read past the block's last granule however short it is).
__device__ __forceinline__ void val_load(const uint32_t* vp, gptr<const uint8_t> g, uint32_t nkv, uint32_t j0, VBatch& B) {
  const uint32_t jl = j0 + (uint32_t(lane_id()) >> 3);
  const uint32_t ph = uint32_t(reinterpret_cast<uintptr_t>(g) & 15u);
#pragma unroll
  for (int u = 0; u < kVG; u++) {
    const VSeg S = val_seg(vp, nkv, jl + 8 * u);
    B.x[u] = *(gptr<const u32x4_ug>)(g + (S.has ? int32_t(S.vs + S.q) : -int32_t(ph)));
  }
}

__device__ __forceinline__ void val_store(const uint32_t* vp, uint32_t nkv, uint32_t j0, const VBatch& B,
                                          gptr<const uint8_t> g, gptr<uint8_t> vbytes) {
  const uint32_t c = uint32_t(lane_id()) & 7u, jl = j0 + (uint32_t(lane_id()) >> 3);
#pragma unroll
  for (int u = 0; u < kVG; u++) {
    const VSeg S = val_seg(vp, nkv, jl + 8 * u);
    if (S.has) st_out((gptr<u32x4_ug>)(vbytes + S.vo + S.q), u32x4_ug(B.x[u]));
    if (S.vl > 128 && S.vl <= kWaveVal) {
      // the value's further chunks, kMedU per lane in flight
      for (uint32_t o0 = 16 * c + 128; o0 < S.vl; o0 += 128 * kMedU) {
        u32x4 y[kMedU];
#pragma unroll
        for (int k = 0; k < kMedU; k++) {
          const uint32_t o = o0 + 128 * k, q = o < S.vl - 16 ? o : S.vl - 16;
          if (o < S.vl) y[k] = *(gptr<const u32x4_ug>)(g + S.vs + q);
        }
#pragma unroll
        for (int k = 0; k < kMedU; k++) {
          const uint32_t o = o0 + 128 * k, q = o < S.vl - 16 ? o : S.vl - 16;
          if (o < S.vl) st_out((gptr<u32x4_ug>)(vbytes + S.vo + q), u32x4_ug(y[k]));
        }
      }
    } else if (S.vl < 16) {
      for (uint32_t o = c; o < S.vl; o += 8) vbytes[S.vo + o] = g[S.vs + o];
    }
  }
}

// ---- the fast value step (PBL_POOL_VFAST) --------------------------------------
// The descriptors of a step's 64 KVs, read from the slot once, lane per KV
// (the index clamped to nkv: vp[nkv .. nkv + 4] hold the total, so a lane past
// the last KV sees an empty value at the end): the value's length above its
// source offset (lw, for the loads) and above its output offset (sw, for the
// stores and for val_off).  All three fields fit 16 bits (blocks <= 32 KiB).
// `fast`: every value of the step is empty or 16 .. 128 B long, one chunk per
// lane of its group and no byte loop.
struct VDesc {
  uint32_t lw, sw;
  bool fast;
};
__device__ __forceinline__ VDesc val_desc(const uint32_t* vp, uint32_t nkv, uint32_t j0) {
  const uint32_t j = min(j0 + uint32_t(lane_id()), nkv);
  const uint32_t a = vp[j], z = vp[j + 1];
  const uint32_t vo = a & 0xffffu, vl = (z & 0xffffu) - vo;
  VDesc D;
  D.lw = (a >> 16) | vl << 16;
  D.sw = vo | vl << 16;
  D.fast = __ballot(vl != 0 && vl - 16u > 112u) == 0;
  return D;
}
// KV 8 u + lane / 8 of the step is group lane / 8's u-th: its word from the
// lane that read it (every lane reads: the caller's branch is wave-uniform).
__device__ __forceinline__ uint32_t grp_word(uint32_t w, int u) {
  return uint32_t(__builtin_amdgcn_ds_bpermute(int(4u * (8u * uint32_t(u) + (uint32_t(lane_id()) >> 3))), int(w)));
}
// A lane's chunk of a fast step's value of length vl at offset `at`: the
// offset of its 16 bytes (the last chunk ends at the value's end), or kNoChunk.
constexpr uint32_t kNoChunk = ~0u;
__device__ __forceinline__ uint32_t fast_chunk(uint32_t w) {
  const uint32_t c16 = 16u * (uint32_t(lane_id()) & 7u), at = w & 0xffffu, vl = w >> 16;
  return c16 < vl ? at + min(c16, vl - 16u) : kNoChunk;
}
// The loads of a fast step.  g16: the block's pointer aligned down to 16 B,
// ph: the block's first byte in it; a lane with no chunk loads granule 0.
__device__ __forceinline__ void val_load_fast(gptr<const uint8_t> g16, uint32_t ph, uint32_t lw, VBatch& B) {
  uint32_t w[kVG];
#pragma unroll
  for (int u = 0; u < kVG; u++) w[u] = grp_word(lw, u);
#pragma unroll
  for (int u = 0; u < kVG; u++) {
    const uint32_t o = fast_chunk(w[u]);
    B.x[u] = *(gptr<const u32x4_ug>)(g16 + (o != kNoChunk ? ph + o : 0u));
  }
}
__device__ __forceinline__ void val_store_fast(uint32_t sw, const VBatch& B, gptr<uint8_t> vbytes) {
  uint32_t w[kVG];
#pragma unroll
  for (int u = 0; u < kVG; u++) w[u] = grp_word(sw, u);
#pragma unroll
  for (int u = 0; u < kVG; u++) {
    const uint32_t o = fast_chunk(w[u]);
    if (o != kNoChunk) st_out((gptr<u32x4_ug>)(vbytes + o), u32x4_ug(B.x[u]));
  }
}

// Steps are software-pipelined: step i + 1's loads are issued before step i's
// stores (vmcnt retires loads and stores in issue order, so a load issued
// after a store would wait for that store's acknowledgement too).  B: step 0,
// loaded by the caller.
__device__ __forceinline__ void copy_long_values(const uint32_t* vp, gptr<const uint8_t> g, uint32_t nkv,
                                                 gptr<uint8_t> vbytes);

// PBL_POOL_VDEPTH 2: two steps in flight (B: step 0, B1: step 1, both loaded
// by the caller), each step's loads issued two steps ahead of its stores.
#ifndef PBL_POOL_VDEPTH
#define PBL_POOL_VDEPTH 1
#endif
constexpr int kVDepth = PBL_POOL_VDEPTH;
// PBL_POOL_UNI: the keys and the values of 64 KVs per step (one key batch, one
// value step of 8 KVs per 8-lane group)
#ifndef PBL_POOL_UNI
#define PBL_POOL_UNI 1
#endif
constexpr bool kUni = PBL_POOL_UNI != 0;
static_assert(!kUni || (kKU == 1 && 8 * kVG == kWave), "unified steps: one 64-KV key batch = one value step");
static_assert(kVDepth == 1 || kVDepth == 2, "value steps in flight: 1 or 2");
__device__ __forceinline__ void copy_values_grp(const uint32_t* vp, gptr<const uint8_t> g, uint32_t nkv,
                                                gptr<uint8_t> vbytes, VBatch& B, VBatch& B1) {
  const int l = lane_id();
  constexpr uint32_t S = 8 * kVG;  // KVs per step
  if (kVDepth == 1) {
    for (uint32_t j0 = 0; j0 < nkv; j0 += S) {
      if (j0 + S < nkv) {
        VBatch N;
        val_load(vp, g, nkv, j0 + S, N);
        val_store(vp, nkv, j0, B, g, vbytes);
        B = N;
      } else {
        val_store(vp, nkv, j0, B, g, vbytes);
      }
    }
  } else {
    for (uint32_t j0 = 0; j0 < nkv; j0 += 2 * S) {
      VBatch N;
      if (j0 + 2 * S < nkv) val_load(vp, g, nkv, j0 + 2 * S, N);
      val_store(vp, nkv, j0, B, g, vbytes);
      if (j0 + S >= nkv) break;
      VBatch N1;
      if (j0 + 3 * S < nkv) val_load(vp, g, nkv, j0 + 3 * S, N1);
      val_store(vp, nkv, j0 + S, B1, g, vbytes);
      B = N;
      B1 = N1;
    }
  }
  copy_long_values(vp, g, nkv, vbytes);
}

// Values longer than kWaveVal: the whole wave, kLongU 16-B chunks per lane in
// flight.
#ifndef PBL_POOL_LONGU
#define PBL_POOL_LONGU 8  // config 5 RI 16: 889 / 905 / 874 GiB/s at 4 / 8 / 16
#endif
constexpr int kLongU = PBL_POOL_LONGU;
__device__ __forceinline__ void copy_long_values(const uint32_t* vp, gptr<const uint8_t> g, uint32_t nkv,
                                                 gptr<uint8_t> vbytes) {
  const int l = lane_id();
  for (uint32_t j0 = 0; j0 < nkv; j0 += kWave) {
    const uint32_t j = j0 + uint32_t(l);
    const uint32_t a = j < nkv ? vp[j] : 0u, z = j < nkv ? vp[j + 1] : 0u;
    const uint32_t len = (z & 0xffffu) - (a & 0xffffu);
    for (uint64_t lm = __ballot(j < nkv && len > kWaveVal); lm; lm &= lm - 1) {
      const int sl = __builtin_ctzll(lm);
      const uint32_t ls = __shfl(a >> 16, sl, kWave), ll = __shfl(len, sl, kWave), lo = __shfl(a & 0xffffu, sl, kWave);
      for (uint32_t o0 = 16u * l; o0 < ll; o0 += 16u * kLongU * kWave) {
        u32x4 y[kLongU];
#pragma unroll
        for (int k = 0; k < kLongU; k++) {
          const uint32_t o = o0 + 16u * kWave * k, q = o < ll - 16 ? o : ll - 16;
          y[k] = *(gptr<const u32x4_ug>)(g + ls + (o < ll ? q : 0u));
        }
#pragma unroll
        for (int k = 0; k < kLongU; k++) {
          const uint32_t o = o0 + 16u * kWave * k, q = o < ll - 16 ? o : ll - 16;
          if (o < ll) st_out((gptr<u32x4_ug>)(vbytes + lo + q), u32x4_ug(y[k]));
        }
      }
    }
  }
}

// Take a free stage (lane 0 spins on the workgroup's mask); returns its index.
// (The mask by pointer: block_big, out of line and not a template, takes and
// returns stages too.)
template <class M>
__device__ __forceinline__ uint32_t acquire_stage(M* free_mask) {
  uint32_t s = 0;
  if (lane_id() == 0) {
    for (;;) {
      const uint32_t m = __hip_atomic_load(free_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (m) {
        const uint32_t c = uint32_t(__builtin_ctz(m));
        const uint32_t old =
            __hip_atomic_fetch_and(free_mask, ~(1u << c), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old & (1u << c)) {
          s = c;
          break;
        }
      } else {
        __builtin_amdgcn_s_sleep(PBL_POOL_SLEEP);
      }
    }
  }
  // the stage holder's work (staging, walk, metadata) gates every wave
  // waiting for a stage: it wins issue arbitration against the emitting waves
  if (PBL_POOL_PRIO) __builtin_amdgcn_s_setprio(PBL_POOL_PRIO);
  return __builtin_amdgcn_readfirstlane(__shfl(s, 0, kWave));
}
template <bool kHide>
__device__ __forceinline__ uint32_t acquire(PoolLds<kHide>& L) {
  return acquire_stage(&L.free_mask);
}

// Take a free stage if there is one: one read of the mask and one fetch_and,
// no spin and no sleep (the prefetch of a wave whose emit is unfinished must
// never wait for a stage).  Returns the stage, or -1.  The priority stays the
// emit's.
template <bool kHide>
__device__ __forceinline__ int32_t try_acquire(PoolLds<kHide>& L) {
  int32_t s = -1;
  if (lane_id() == 0) {
    const uint32_t m = __hip_atomic_load(&L.free_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (m) {
      const uint32_t c = uint32_t(__builtin_ctz(m));
      const uint32_t old =
          __hip_atomic_fetch_and(&L.free_mask, ~(1u << c), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (old & (1u << c)) s = int32_t(c);
    }
  }
  return __builtin_amdgcn_readfirstlane(__shfl(s, 0, kWave));
}

// Return stage s to the pool once every LDS read of it has completed.
// `drop_prio`: the wave's issue priority falls back to the emit's.
template <class M>
__device__ __forceinline__ void release_stage(M* free_mask, uint32_t s, bool drop_prio = true) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  wave_sync();
  if (lane_id() == 0) __hip_atomic_fetch_or(free_mask, 1u << s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (PBL_POOL_PRIO && drop_prio) __builtin_amdgcn_s_setprio(0);
}
template <bool kHide>
__device__ __forceinline__ void release(PoolLds<kHide>& L, uint32_t s, bool drop_prio = true) {
  release_stage(&L.free_mask, s, drop_prio);
}

// The block [boff, boff + blen) into stage S by LDS-DMA (granule g of the 16-B
// aligned range at x[1 + g]); the caller waits vmcnt(0) before reading it.
__device__ __forceinline__ void stage_dma(Stage& S, const uint8_t* blocks, uint64_t boff, uint32_t blen) {
  const int l = lane_id();
  const uint64_t a0 = boff & ~uint64_t(15), a1 = (boff + blen + 15) & ~uint64_t(15);
  const uint32_t n16 = uint32_t((a1 - a0) >> 4);
  const gptr<const uint8_t> base = to_glb(blocks + a0);
  for (uint32_t g0 = 0; g0 < n16; g0 += kWave) {
    if (g0 + l < n16)
      __builtin_amdgcn_global_load_lds((gptr<const void>)(base + 16ull * (g0 + l)),
                                       (lptr<void>)to_lds_ptr(reinterpret_cast<void*>(&S.x[1 + g0])), 16, 0, 0);
  }
}

// General path for one block (wave-serial Iter.Next) on the staged block, the
// slot as its key buffer; a key that outgrows it re-runs from global memory
// with the whole stage as the key buffer.  Publishes and resolves its own
// look-back and writes every output.  Out of line: rare and large.
__device__ __noinline__ void block_slow(Stage& S, uint8_t* keybuf, uint32_t keycap, const Args A, uint32_t b,
                                        uint64_t boff, uint32_t blen) {
  const int l = lane_id();
  const uint32_t nb = A.in.n_blocks, flags = A.in.flags;
  const pbl_decode_out& O = A.out;
  uint64_t* lb_state = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(O.workspace) + kWsHeader);
  SlowState ss;
  uint64_t dummy[kNumComp] = {0, 0, 0, 0}, excl[kNumComp];
  const uint8_t* src = reinterpret_cast<const uint8_t*>(S.x) + kPad + (boff & 15);
  bool from_lds = true;
  slow_walk(src, true, blen, flags, A.in.synthetic_seq_num, keybuf, keycap, kPassCount, O, b, dummy, &ss);
  if (ss.status == PBL_UNSUPPORTED) {
    from_lds = false;
    src = A.in.blocks + boff;
    keybuf = reinterpret_cast<uint8_t*>(S.x);
    keycap = uint32_t(kLdsBlkBytes);
    slow_walk(src, false, blen, flags, A.in.synthetic_seq_num, keybuf, keycap, kPassCount, O, b, dummy, &ss);
  }
  const bool okk = ss.status == PBL_OK;
  const uint64_t agg[kNumComp] = {okk ? ss.nkv : 0, okk ? ss.kb : 0, okk ? ss.vb : 0, okk ? ss.nr : 0};
  lookback<kLbL2, kPoolLbF>(lb_state, nb, b, agg, excl, &O.totals->status_mask);
  uint32_t st2 = ss.status;
  if (okk && overflows(O, excl, agg)) st2 = PBL_OVERFLOW;
  if (st2 == PBL_OK) slow_walk(src, from_lds, blen, flags, A.in.synthetic_seq_num, keybuf, keycap, kPassAll, O, b, excl, &ss);
  else if (l == 0 && O.key_off && excl[0] + b < O.kv_cap + nb) {
    to_glb(O.key_off)[excl[0] + b] = 0;
    to_glb(O.val_off)[excl[0] + b] = 0;
  }
  if (l == 0) write_block_meta(O, b, nb, st2, excl, agg, true);
}

// A block past the stage (stage s held on entry, released here).
// row_prepare_kernel walked it, published its aggregate and left {status,
// counts} in its block-metadata slots; or it marked the block kBigRedo (a key
// past its small buffer), and then this wave, which still holds its stage,
// runs the count walk with that stage as the 32 KiB key buffer and publishes
// (sizes tier 2), and only then lets the stage go.  Once the block's bases
// resolve, the wave walks it from global memory and writes its outputs, its
// slot as the key buffer; at a key past the slot it takes a stage again and
// repeats the walk with that as the key buffer.  (Config 5: 2195 big blocks,
// one 48 KB value each; a separate values pass took 87 us.)  Out of line.
// `stages`, `free_mask`: the workgroup's pool.
__device__ __noinline__ void block_big(const Args A, uint32_t b, uint64_t boff, uint32_t blen, uint8_t* keybuf,
                                       uint32_t keycap, Stage* stages, uint32_t* free_mask, uint32_t s) {
  const int l = lane_id();
  const uint32_t nb = A.in.n_blocks;
  const pbl_decode_out& O = A.out;
  const lptr<uint32_t> fm = to_lds_ptr(free_mask);
  uint64_t* lb_state = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(O.workspace) + kWsHeader);
  uint32_t st0 = to_glb(O.blk_status)[b];
  uint64_t agg[kNumComp];
  if (st0 == rowc::kBigRedo) {
    SlowState ss;
    rowc::big_block_count(A, b, to_lds_ptr(reinterpret_cast<uint8_t*>(stages[s].x)), uint32_t(kLdsBlkBytes), &ss);
    rowc::big_block_publish(A, b, ss);
    release_stage(fm, s);
    st0 = ss.status;
    const bool ok2 = st0 == PBL_OK;
    agg[0] = ok2 ? ss.nkv : 0;
    agg[1] = ok2 ? ss.kb : 0;
    agg[2] = ok2 ? ss.vb : 0;
    agg[3] = ok2 ? ss.nr : 0;
  } else {
    release_stage(fm, s);
    const bool ok1 = st0 == PBL_OK;
    agg[0] = ok1 ? to_glb(O.blk_kv_base)[b] : 0;
    agg[1] = ok1 ? to_glb(O.blk_key_base)[b] : 0;
    agg[2] = ok1 ? to_glb(O.blk_val_base)[b] : 0;
    agg[3] = ok1 ? uint64_t(GlbBlk{to_glb(A.in.blocks + boff), blen}.le32(blen - 4)) : 0;
  }
  const bool okk = st0 == PBL_OK;
  uint64_t excl[kNumComp];
  lb_resolve<kLbWin, kLbL2, kPoolLbF>(lb_state, nb, b, agg, excl, &O.totals->status_mask);
  uint32_t st2 = st0;
  if (okk && overflows(O, excl, agg)) st2 = PBL_OVERFLOW;
  if (l == 0) {
    if (st2 != PBL_OK && O.key_off && excl[0] + b < O.kv_cap + nb) {
      to_glb(O.key_off)[excl[0] + b] = 0;
      to_glb(O.val_off)[excl[0] + b] = 0;
    }
    write_block_meta(O, b, nb, st2, excl, agg, true);
  }
  if (st2 == PBL_OK) {
    // the wave has published and resolved: it may wait for a stage, no stage
    // holder ever waits on it
    lptr<uint8_t> kb = to_lds_ptr(keybuf);
    bool staged = false;
    uint32_t s2 = 0;
    SlowState ss;
    for (;;) {
      slow_walk_t<GlbBlk, PBL_BIG_U>(GlbBlk{to_glb(A.in.blocks + boff), blen}, blen, A.in.flags,
                                      A.in.synthetic_seq_num, kb, keycap, kPassAll, O, b, excl, &ss);
      // a key past the slot: once more with a stage, which rewrites the block
      // (a key past the stage too: the block's outputs are the long-key
      // kernels', rowblk_long.hip.h)
      if (staged || ss.status != PBL_UNSUPPORTED) break;
      s2 = acquire_stage(fm);
      staged = true;
      kb = to_lds_ptr(reinterpret_cast<uint8_t*>(stages[s2].x));
      keycap = uint32_t(kLdsBlkBytes);
    }
    if (staged) release_stage(fm, s2);
    if (!staged && ss.status != PBL_OK && l == 0) {
      // the same walk as the sizes pass over the same bytes cannot disagree
      // with it; if it ever did, the block reports the walk's status
      to_glb(O.blk_status)[b] = ss.status;
      g_atomic_or(&O.totals->status_mask, 1u << ss.status);
      g_atomic_add(&O.totals->n_bad_blocks, 1u);
    }
  }
}

// A block between its walk and its emit: what the emit needs besides the slot.
struct Pend {
  uint64_t boff;
  uint32_t b, status, nkv, tkb, tvb, nres, roff, blen;
  bool live;  // the emit (look-back, outputs) is still to do
};

// Stage, walk and describe block b (stage s held on entry, released before
// return).  The block's aggregate is always published before return, so every
// later ticket can resolve past it while this wave goes on.  Blocks off the
// fast path are finished here (live = false).
// `staged`: the block's DMA into the stage was issued by the prefetch of the
// emit before (still to be waited for).
template <bool kHide>
__device__ __forceinline__ Pend block_front(PoolLds<kHide>& L, uint32_t s, uint32_t b, uint64_t boff, uint32_t blen,
                                            bool staged, Slot<kHide>& W, const Args& A) {
  Stage& S = L.st[s];
  const int l = lane_id();
  const uint32_t nb = A.in.n_blocks, flags = A.in.flags;
  const bool vprefix = (flags & PBL_ROW_VALUE_PREFIX) && !(flags & PBL_ROW_RAW_KEYS);
  uint64_t* lb_state = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) + kWsHeader);
  constexpr uint32_t kKv = uint32_t(Slot<kHide>::kKv);
  Pend P;
  P.b = b;
  P.boff = boff;
  P.blen = blen;
  P.live = false;
  P.nkv = P.tkb = P.tvb = P.nres = P.roff = 0;
  P.status = PBL_OK;

  if (blen > kMaxFastLen) {
    block_big(A, b, boff, blen, reinterpret_cast<uint8_t*>(&W), uint32_t(sizeof(W)), L.st, &L.free_mask, s);
    return P;
  }
  PSTAMP(A, b, 1, l == 0);
  if (!staged) stage_dma(S, A.in.blocks, boff, blen);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  wave_sync();
  PSTAMP(A, b, 2, l == 0);
  const View V = lds_view(S.x, uint32_t(kPad + (boff & 15)));
  uint32_t roff, nres;
  uint32_t status = init_checks(LdsBlk{V}, blen, flags, &roff, &nres);
  bool slow = status == PBL_OK && nres > kKv;
  uint32_t nkv = 0, tkb = 0, tvb = 0;
  bool published = false, released = false;
  if (status == PBL_OK && !slow && roff > 0) {
    // lane l owns runs [r0, r1): contiguous, so a lane scan orders them
    const uint32_t R = (nres + kWave - 1) / kWave;
    const uint32_t r0 = min(uint32_t(l) * R, nres), r1 = min(r0 + R, nres);
    PAcc acc{0, 0, 0, 0};
    bool ok = true, bad = false, vbad = false, over = false;
    PRun RB;
    RB.n = 0;
    RB.pos = RB.e0 = RB.prev_kl = RB.prev_kind = RB.rw = 0;
    const bool single = R == 1;
    front_walk<kHide>(V, r0, r1, nres, roff, flags, vprefix, single, RB, acc, ok, bad, vbad, over);
    const uint32_t ic = dpp_incl_scan(acc.cnt), ik = dpp_incl_scan(acc.kb), iv = dpp_incl_scan(acc.vb);
    const uint32_t ie = kHide ? dpp_incl_scan(acc.ne) : ic;
    nkv = last_lane(ic);
    tkb = last_lane(ik);
    tvb = last_lane(iv);
    const uint32_t nent = kHide ? last_lane(ie) : nkv;
    if (__ballot(bad)) status = PBL_CORRUPT_BOUNDS;
    else if (__ballot(!ok) || nent > kKv) slow = true;
    else if (__ballot(vbad)) status = PBL_CORRUPT_BOUNDS;  // Go: i.val[0] on an empty SET value
    if (status == PBL_OK && !slow) {
      // the sizes are final: publish, then write the metadata
      const uint64_t agg[kNumComp] = {nkv, tkb, tvb, nres};
      lb_publish(lb_state, nb, b, agg);
      published = true;
      PSTAMP(A, b, 3, l == 0);
      // Without value prefixes, with every run inside the parked registers,
      // the metadata pass reads the registers only (entry_meta touches V under
      // setv alone, and setv needs the value-prefix flag): the stage goes back
      // to the pool now.  (slow is false here, so this is the block's one release.)
      if (kEarlyRel && single && !vprefix && !__ballot(over)) {
        release(L, s, kEarlyRel != 2);
        released = true;
        PSTAMP(A, b, 9, l == 0);
      }
      MState M{ie - (kHide ? acc.ne : acc.cnt), ic - acc.cnt, iv - acc.vb, 0, 0, 0};
      front_meta<kHide>(W, V, r0, r1, nres, roff, flags, vprefix, single, over, RB, M);
      if (l < 5) W.vp[nkv + l] = tvb;
      PSTAMP(A, b, 4, l == 0);
    }
  }
  if (status == PBL_OK && slow) {
    block_slow(S, reinterpret_cast<uint8_t*>(W.m0), uint32_t(sizeof(W.m0)), A, b, boff, blen);
    release(L, s);
    PSTAMP(A, b, 9, l == 0);
    return P;
  }
  if (!released) {
    release(L, s);
    PSTAMP(A, b, 9, l == 0);
  } else if (PBL_POOL_PRIO && kEarlyRel == 2) {
    __builtin_amdgcn_s_setprio(0);
  }
  if (!published) {  // a failed or empty block: its (zero) aggregate
    const bool okb = status == PBL_OK;
    const uint64_t agg[kNumComp] = {okb ? nkv : 0, okb ? tkb : 0, okb ? tvb : 0, okb ? nres : 0};
    lb_publish(lb_state, nb, b, agg);
    if (l < 5) W.vp[l] = 0;  // (an empty block's lone N+1 offsets)
  }
  P.status = status;
  P.nkv = status == PBL_OK ? nkv : 0;
  P.tkb = status == PBL_OK ? tkb : 0;
  P.tvb = status == PBL_OK ? tvb : 0;
  P.nres = status == PBL_OK ? nres : 0;
  P.roff = roff;
  P.live = true;
  return P;
}

// What a wave's emit hands to its next loop iteration: a stage and a ticket
// taken ahead and whether the block's DMA is in flight.
// kNextDone: the ticket was past the end of the batch (the stage went straight
// back): the wave has no more blocks.
struct Next {
  uint32_t t, w;  // the ticket's block; stage | kNext* flags
};
constexpr uint32_t kNextHave = 4, kNextStaged = 8, kNextDone = 16;
static_assert(kNS <= 4, "Next::w keeps the stage in two bits");

// The prefetch: try to take a stage; with one in hand take the wave's next
// ticket, read its descriptor and start the block's DMA into the stage.  Never
// waits on anything but the wave's own memory operations.  Only the Stage is
// filled: the wave's slot stays the current block's until its emit returns.
template <bool kHide>
__device__ __forceinline__ void prefetch(PoolLds<kHide>& L, const Args& A, const uint32_t* ids, uint32_t nt, Next& X) {
  const int32_t s = try_acquire(L);
  if (s < 0) return;  // no stage free: the next loop iteration acquires one
  uint32_t t = 0;
  if (lane_id() == 0) t = g_atomic_add(reinterpret_cast<uint32_t*>(A.out.workspace), 1u);
  t = __builtin_amdgcn_readfirstlane(__shfl(t, 0, kWave));
  if (t >= nt) {
    release(L, uint32_t(s));
    X.w = kNextDone;
    return;
  }
  if (ids) t = __builtin_amdgcn_readfirstlane(to_glb(ids)[t]);
  const uint64_t boff = to_glb(A.in.block_off)[t];
  const uint32_t blen = to_glb(A.in.block_len)[t];
  // (a block past the stage is handed on as it is: block_big lets the stage go before its look-back)
  const bool staged = blen <= kMaxFastLen;
  X.t = t;
  X.w = uint32_t(s) | kNextHave | (staged ? kNextStaged : 0u);
  if (staged) stage_dma(L.st[s], A.in.blocks, boff, blen);
  PSTAMP(A, t, 10, lane_id() == 0);
}

// Resolve block P's look-back and write its outputs from slot W.  `X`: the
// wave's next block, staged under the last steps (kPrefetch).
template <bool kHide>
__device__ __forceinline__ void block_emit(const Pend& P, const Slot<kHide>& W, const Args& A, PoolLds<kHide>& L,
                                           const uint32_t* ids, uint32_t nt, Next& X) {
  const int l = lane_id();
  const uint32_t nb = A.in.n_blocks, flags = A.in.flags, b = P.b;
  const pbl_decode_out& O = A.out;
  uint64_t* lb_state = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(O.workspace) + kWsHeader);
  const uint8_t* gblk = A.in.blocks + P.boff;
  const gptr<const uint8_t> gb = ubase<kSBase>(to_glb(gblk));
  // (the fast value step's loads: the block's first 16-B granule and the block's phase in it)
  const uint32_t ph = uint32_t(uint64_t(gblk) & 15u);
  const gptr<const uint8_t> g16 = ubase<kSBase>(to_glb(gblk - ph));
  constexpr bool kFastSteps = kVFast && kUni && kVDepth == 1;
  const GSrc KS{gb, P.blen, uint32_t(((uint64_t(gblk) + P.blen + 15) & ~uint64_t(15)) - uint64_t(gblk))};
  const bool raw = (flags & PBL_ROW_RAW_KEYS) != 0;
  const uint32_t nkv = P.nkv, nres = P.nres;
  // the look-back windows, the first key batch, the first value step and the
  // first restart words: all in one round trip
  LbWindows<kPoolLbWin, kLbL2, kPoolLbF> G;
  if (b > 0) G.issue(LbPtrs(lb_state, nb), int64_t(b) - 1);
  KBatch K;
  VBatch VB, VB1;
  VDesc VD{0, 0, true};
  uint32_t rs0 = 0;
  const bool ok0 = P.status == PBL_OK;
  if (ok0) {
    key_load<kHide, GSrc>(W, KS, raw, 0, nkv, K);
    if (kFastSteps) VD = val_desc(W.vp, nkv, 0);
    if (kFastSteps && VD.fast) val_load_fast(g16, ph, VD.lw, VB);
    else val_load(W.vp, gb, nkv, 0, VB);
    if (kVDepth == 2) val_load(W.vp, gb, nkv, 8 * kVG, VB1);
    if (O.restarts && uint32_t(l) < nres) rs0 = KS.le32(P.roff + 4 * l);
  }
  const uint64_t agg[kNumComp] = {nkv, P.tkb, P.tvb, nres};
  uint64_t excl[kNumComp];
#ifdef PBL_STAMPS
  LbDiag LD;
  lb_finish<kPoolLbWin, kLbL2, kPoolLbWinLater, kPoolLbF, kPoolLbLaterLanes>(lb_state, nb, b, agg, excl, &O.totals->status_mask, G, &LD);
  if (l == 0) {  // slots 11-14: what the resolve cost (counts, not times)
    uint64_t* sp = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(O.workspace) + ws_bytes(nb)) + uint64_t(b) * 16;
    sp[11] = LD.trips;
    sp[12] = LD.recs;
    sp[13] = LD.poll;
    sp[14] = LD.recs2;
  }
#else
  lb_finish<kPoolLbWin, kLbL2, kPoolLbWinLater, kPoolLbF, kPoolLbLaterLanes>(lb_state, nb, b, agg, excl, &O.totals->status_mask, G);
#endif
  PSTAMP(A, b, 5, l == 0);
  uint32_t status = P.status;
  if (ok0 && overflows(O, excl, agg)) status = PBL_OVERFLOW;
  if (l == 0) {
    if (status != PBL_OK && O.key_off && excl[0] + b < O.kv_cap + nb) {
      to_glb(O.key_off)[excl[0] + b] = 0;
      to_glb(O.val_off)[excl[0] + b] = 0;
    }
    write_block_meta(O, b, nb, status, excl, agg, false);
  }
  if (status != PBL_OK) return;

  // ---- keys and per-KV arrays: lane per KV ------------------------------------
  const uint64_t kvb = uni64<kSBase>(excl[0]), kbb = uni64<kSBase>(excl[1]), vbb = uni64<kSBase>(excl[2]),
                 rbb = uni64<kSBase>(excl[3]);
  const gptr<uint32_t> p_rst = ubase<kSBase>(to_glb(O.restarts) + rbb);
  if (O.restarts && uint32_t(l) < nres) p_rst[uint32_t(l)] = rs0;
  uint32_t kcar = 0;
  const gptr<uint8_t> vbytes = ubase<kSBase>(to_glb(O.val_bytes) + vbb);
  if (kUni) {
    // keys and values of the same 64 KVs in one step: a line of the block is
    // fetched once for both
    // the prefetch point: past lb_finish, so nothing from here to the wave's
    // next publish waits on another wave; before the step's loads, so their
    // vmcnt wait covers the DMA
    bool pf = kPrefetch != 0;
    if (kFastSteps) {
      // a step's class (VD.fast) is decided at its loads and carried, with its
      // descriptors, to its stores one iteration later
      for (uint32_t j0 = 0; j0 <= nkv; j0 += kWave) {
        KBatch KN;
        VBatch VN;
        VDesc DN{0, 0, true};
        const bool more = j0 + kWave <= nkv;
        if (pf && (nkv - j0) / kWave + PBL_POOL_PREFETCH_LATE <= kPrefetch) {
          prefetch<kHide>(L, A, ids, nt, X);
          pf = false;
        }
        if (more) {
          DN = val_desc(W.vp, nkv, j0 + kWave);
          if (DN.fast) val_load_fast(g16, ph, DN.lw, VN);
          else val_load(W.vp, gb, nkv, j0 + kWave, VN);
          key_load<kHide, GSrc>(W, KS, raw, j0 + kWave, nkv, KN);
        }
        key_store<kHide, GSrc, 0, true, true>(W, KS, A, b, j0, nkv, kvb, kbb, K, kcar, VD.sw & 0xffffu);
        if (VD.fast) val_store_fast(VD.sw, VB, vbytes);
        else val_store(W.vp, nkv, j0, VB, gb, vbytes);
        K = KN;
        VB = VN;
        VD = DN;
      }
    } else if (kVDepth == 1) {
      for (uint32_t j0 = 0; j0 <= nkv; j0 += kWave) {
        KBatch KN;
        VBatch VN;
        const bool more = j0 + kWave <= nkv;
        if (pf && (nkv - j0) / kWave + PBL_POOL_PREFETCH_LATE <= kPrefetch) {
          prefetch<kHide>(L, A, ids, nt, X);
          pf = false;
        }
        if (more) {
          key_load<kHide, GSrc>(W, KS, raw, j0 + kWave, nkv, KN);
          val_load(W.vp, gb, nkv, j0 + kWave, VN);
        }
        key_store<kHide, GSrc, 0, true>(W, KS, A, b, j0, nkv, kvb, kbb, K, kcar);
        val_store(W.vp, nkv, j0, VB, gb, vbytes);
        K = KN;
        VB = VN;
      }
    } else {
      // the values two steps ahead, the keys one
      for (uint32_t j0 = 0; j0 <= nkv; j0 += kWave) {
        KBatch KN;
        VBatch VN;
        if (pf && (nkv - j0) / kWave + PBL_POOL_PREFETCH_LATE <= kPrefetch) {
          prefetch<kHide>(L, A, ids, nt, X);
          pf = false;
        }
        if (j0 + kWave <= nkv) key_load<kHide, GSrc>(W, KS, raw, j0 + kWave, nkv, KN);
        if (j0 + 2 * kWave < nkv) val_load(W.vp, gb, nkv, j0 + 2 * kWave, VN);
        key_store<kHide, GSrc>(W, KS, A, b, j0, nkv, kvb, kbb, K, kcar);
        val_store(W.vp, nkv, j0, VB, gb, vbytes);
        K = KN;
        VB = VB1;
        VB1 = VN;
      }
    }
    if (O.restarts)
      for (uint32_t r = kWave + l; r < nres; r += kWave) p_rst[r] = KS.le32(P.roff + 4 * r);
    copy_long_values(W.vp, gb, nkv, vbytes);
    PSTAMP(A, b, 6, l == 0);
    PSTAMP(A, b, 7, l == 0);
    return;
  }
  key_store<kHide, GSrc>(W, KS, A, b, 0, nkv, kvb, kbb, K, kcar);
  for (uint32_t j0 = kWave * kKU; j0 <= nkv; j0 += kWave * kKU) {
    KBatch N;
    key_load<kHide, GSrc>(W, KS, raw, j0, nkv, N);
    key_store<kHide, GSrc>(W, KS, A, b, j0, nkv, kvb, kbb, N, kcar);
  }
  if (O.restarts)
    for (uint32_t r = kWave + l; r < nres; r += kWave) to_glb(O.restarts)[rbb + r] = KS.le32(P.roff + 4 * r);
  PSTAMP(A, b, 6, l == 0);

  // ---- values, global -> global --------------------------------------------
  if (P.tvb) copy_values_grp(W.vp, gb, nkv, vbytes, VB, VB1);
  PSTAMP(A, b, 7, l == 0);
}

// The persistent kernel: one workgroup of kNW waves per CU, each wave a loop
// of (acquire a stage, take a ticket, stage / walk / describe the block into
// its slot, let the stage go, emit the block from the slot).  With
// PBL_POOL_PREFETCH the acquire, the ticket and the DMA of the wave's next
// block are done under the last steps of its emit (prefetch) and handed to
// the next iteration in `Next`.
// Deadlock-free for any residency:
//  - a wave takes a ticket only while holding a stage (acquire, then ticket;
//    the prefetch too), and publishes the block's aggregate before it lets
//    that stage go;
//  - between taking a ticket and publishing its aggregate a wave waits on
//    nothing but its own memory operations: in the loop that is the DMA and
//    the walk; after a prefetch it is the rest of the current emit, which has
//    no look-back left (the prefetch point is past lb_finish) and no wait on
//    another wave, and then the same DMA wait and walk;
//  - the prefetch's try_acquire never blocks, so a wave with an unfinished
//    emit never waits for a stage: every stage holder runs on to its publish
//    and its release without needing any other wave to move;
//  - the look-back waits only on smaller tickets, each held by a wave that
//    holds a stage (and so reaches its publish by the above) or has published;
//    every poll of it (lb_finish's single-lane poll, lb_poll) is bounded by the
//    spin cap and ends in PBL_TIMEOUT;
//  - a block past the stage that row_prepare_kernel left unsized (kBigRedo) is
//    sized by the wave that draws it, which still holds the ticket's stage: it
//    runs the count walk (its own memory operations only) with that stage as
//    the key buffer, publishes, and only then lets the stage go, so the first
//    two points hold for it as for a staged block;
//  - block_big's second write walk (a key past the slot) waits for a stage
//    after the wave has published AND resolved: it holds no stage and no
//    unpublished ticket while it waits, and no stage holder waits on it (a
//    holder waits on its own memory operations, or in block_slow's look-back on
//    smaller tickets, which this wave's publish already satisfies); every
//    holder therefore runs on to its release, and the waiting wave gets a
//    stage.  With every wave of a workgroup in that wait at once, no stage is
//    held and the first to look takes one;
//  - the two-level form (PBL_LB_L2) adds two stores and no wait: the wave that
//    resolves a chunk's last block stores the chunk's summed aggregate after
//    its first window (only from records it has already loaded) and the
//    chunk's prefix with its own; a resolve reads chunk records in the round
//    trip it makes anyway and never polls one: an absent, half-written or
//    never-written record (a wide aggregate, a last block that another kernel
//    resolves) costs exactly the one-level walk over that chunk's block
//    records, so the four points above stand unchanged.
// `ids` (mixed batches): the ascending ids of the batch's row blocks, their
// count at workspace header word kWsRowCount; the colblk blocks' aggregates are
// published before this launch (mixed_col_size_kernel), so the look-back walks
// through them and still waits only on smaller tickets.  Null: every block.
template <bool kHide>
__global__ void __launch_bounds__(kTPBP, 1) rowblk_pool_kernel(Args A, const uint32_t* ids) {
  __shared__ PoolLds<kHide> L;
  if (threadIdx.x == 0) L.free_mask = (1u << kNS) - 1u;
  __syncthreads();
  Slot<kHide>& W = L.sl[wave_id()];
  const uint32_t nb = A.in.n_blocks;
  uint32_t* tick = reinterpret_cast<uint32_t*>(A.out.workspace);
  const uint32_t nt = ids ? __hip_atomic_load(to_glb(tick) + kWsRowCount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                          : nb;
  Next X{0, 0};
  for (;;) {
#ifdef PBL_STAMPS
    const uint64_t t_acq = __builtin_amdgcn_s_memtime();  // (the end of the emit before)
#endif
    uint32_t s, t0;
    bool staged = false;
    if (kPrefetch && (X.w & kNextDone)) break;
    if (kPrefetch && (X.w & kNextHave)) {
      // the emit before took the stage and the ticket and started the DMA
      // (the descriptor is read again: two words, cache-hot, under the DMA)
      s = X.w & 3u;
      t0 = X.t;
      staged = (X.w & kNextStaged) != 0;
      X.w = 0;
      if (PBL_POOL_PRIO) __builtin_amdgcn_s_setprio(PBL_POOL_PRIO);
    } else {
      s = acquire(L);
      t0 = 0;
      if (lane_id() == 0) t0 = g_atomic_add(tick, 1u);
      t0 = __builtin_amdgcn_readfirstlane(__shfl(t0, 0, kWave));
      if (t0 >= nt) {
        release(L, s);
        break;
      }
      if (ids) t0 = __builtin_amdgcn_readfirstlane(to_glb(ids)[t0]);
      PSTAMP(A, t0, 0, lane_id() == 0);
    }
    const uint64_t boff = to_glb(A.in.block_off)[t0];
    const uint32_t blen = to_glb(A.in.block_len)[t0];
#ifdef PBL_STAMPS
    if (lane_id() == 0)
      reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(A.out.workspace) + ws_bytes(nb))[uint64_t(t0) * 16 + 8] = t_acq;
#endif
    const Pend Q = block_front<kHide>(L, s, t0, boff, blen, staged, W, A);
    if (Q.live) block_emit<kHide>(Q, W, A, L, ids, nt, X);
    wave_sync();  // (the slot is the next block's)
  }
}

}  // namespace pool
}  // namespace row
}  // namespace pbl
