// rowblk_general.hip.h — slow_walk: the general (non-fast-path) row-block
// decoder, a wave-serial restatement of Iter.First/Next (rowblk_iter.go).  Block
// bytes come through a reader of rowblk_core.hip.h (LdsBlk when staged, else
// GlbBlk); the current key lives in an LDS key buffer.  One wave executes it.
#pragma once

#include <type_traits>

#include "rowblk_core.hip.h"

namespace pbl {
namespace row {

struct SlowState {
  uint64_t nkv, kb, vb, nr;
  uint32_t status;
};

// Key buffer: LDS bytes with a 16-B front pad and a 32-B tail so that 16-B
// gathers around the key stay inside it.
constexpr uint32_t kKeyBufPad = 16, kKeyBufSlack = 48;

// Walk passes: kPassCount counts; kPassAll writes every output at the given bases.
enum { kPassCount = 0, kPassAll = 1 };

#ifndef PBL_SLOW_U
#define PBL_SLOW_U 1
#endif

// The spill form's key store past the LDS buffer: a per-workgroup slot in
// global memory (16-B aligned).  With C the LDS capacity, key byte p lives in
// LDS for p < C + kSpillSeam and at spill[p - C] for p >= C: the seam bytes are
// kept in both, so every 16-B window and every trailer comes whole from one of
// the two (windows that start at or below C from LDS, the rest from the slot).
constexpr uint32_t kSpillSeam = 16;
static_assert(kSpillSeam + 16 <= kKeyBufSlack - kKeyBufPad, "the seam and a window past it fit the LDS tail");

// Bytes [lo, hi) of the slot's 16-B granule at ga from w: plain stores (the
// slot is read back, never streamed past).
__device__ __forceinline__ void spill_put16(gptr<uint8_t> spill, uint64_t ga, uint64_t lo, uint64_t hi, const uint4& w) {
  if (ga >= lo && ga + 16 <= hi) {
    *(gptr<u32x4>)(spill + ga) = u32x4{w.x, w.y, w.z, w.w};
    return;
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint32_t word = i < 4 ? w.x : i < 8 ? w.y : i < 12 ? w.z : w.w;
    if (ga + i >= lo && ga + i < hi) spill[ga + i] = uint8_t(word >> (8 * (i & 3)));
  }
}
// Slot reads are served from L2 (agent-scope loads): the CU's L1 may hold the
// line as it was for an earlier key.  The caller has drained its stores.
__device__ __forceinline__ uint4 spill_granule(gptr<uint8_t> spill, uint64_t a) {
  const gptr<uint64_t> q = (gptr<uint64_t>)(spill + a);
  const uint64_t x = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint64_t y = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return make_uint4(uint32_t(x), uint32_t(x >> 32), uint32_t(y), uint32_t(y >> 32));
}
// 16 slot bytes at x (any alignment): the aligned pair, funnelled
__device__ __forceinline__ uint4 spill_get16(gptr<uint8_t> spill, uint64_t x) {
  const uint64_t a = x & ~uint64_t(15);
  const uint32_t sh = uint32_t(x - a);
  const uint4 v = spill_granule(spill, a);
  return sh ? funnel16(v, spill_granule(spill, a + 16), sh) : v;
}
__device__ __forceinline__ uint32_t spill_byte(gptr<uint8_t> spill, uint64_t x) {
  return __hip_atomic_load(spill + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// U: value granules per lane in flight.  kSpill: keys longer than the LDS
// buffer continue in the slot `spill` of `spillcap` bytes (the long-key
// kernels of rowblk_long.hip.h; the block in global memory); every other walk
// keeps the key in LDS alone.
template <class Src, int U, bool kSpill = false>
__device__ __forceinline__ void slow_walk_t(const Src S, uint64_t len, uint32_t flags, uint64_t seq, lptr<uint8_t> kbuf,
                                            uint32_t keycap, int pass, const pbl_decode_out& O, uint32_t b,
                                            const uint64_t bases[kNumComp], SlowState* st,
                                            gptr<uint8_t> spill = nullptr, uint64_t spillcap = 0) {
  const int l = lane_id();
  lptr<uint8_t> keybuf = kbuf + kKeyBufPad;
  const lptr<const uint32_t> KW = (lptr<const uint32_t>)kbuf;
  keycap = keycap > kKeyBufSlack ? keycap - kKeyBufSlack : 0;
  // the longest key the walk holds: the slot keeps kKeyBufSlack bytes for the
  // windows that end past a key
  const uint64_t keymax = uint64_t(keycap) + (kSpill && spillcap > kKeyBufSlack ? spillcap - kKeyBufSlack : 0);
  const gptr<uint64_t> o_trailer = to_glb(O.trailer);
  const gptr<uint8_t> o_flags = to_glb(O.kv_flags);
  const gptr<uint32_t> o_entry = to_glb(O.entry_off), o_koff = to_glb(O.key_off), o_voff = to_glb(O.val_off);
  const int32_t nr = int32_t(S.le32(len - 4));
  const int64_t restarts = int64_t(len) - 4 * (1 + int64_t(nr));
  uint64_t nkv = 0, kb = 0, vb = 0, full_len = 0;
  int64_t offset = 0;
  uint32_t ri = 0;
  // restart word ri, held in a register: re-read only when the walk passes it
  uint32_t rw_ri = (pass == kPassAll && nr > 0 && restarts >= 0) ? S.le32(uint64_t(restarts)) : 0u;
  uint32_t status = PBL_OK;
  // the next entry's header window is loaded before this entry's stores: a
  // load's data waits for every older vector-memory op, so a header read
  // behind the value stores would wait for all of them (config 5's big-block
  // values walk)
  uint4 hw_next = restarts > 0 ? S.ld16(0) : make_uint4(0, 0, 0, 0);
  while (offset >= 0 && offset < restarts) {
    // the header's bytes in one window, the three varints from registers
    const uint4 hw = hw_next;
    const uint32_t hn = uint32_t(min<int64_t>(15, int64_t(len) - offset));
    uint32_t shared, unshared, vlen;
    const uint32_t h = entry_header(hw, hn, &shared, &unshared, &vlen);
    if (!h) { status = PBL_CORRUPT_BOUNDS; break; }
    const uint64_t kp = uint64_t(offset) + h;
    if (len - kp < unshared) { status = PBL_CORRUPT_BOUNDS; break; }
    const uint64_t vp = kp + unshared;
    if (len - vp < vlen) { status = PBL_CORRUPT_BOUNDS; break; }
    if (shared > full_len) { status = PBL_CORRUPT_BOUNDS; break; }
    const uint64_t klen = uint64_t(shared) + unshared;
    if (klen > keymax) { status = PBL_UNSUPPORTED; break; }
    if (int64_t(vp + vlen) < restarts) hw_next = S.ld16(int64_t(vp + vlen));
    wave_sync();
    // unshared key bytes -> keybuf[shared, klen): one 16-B window per lane step
    // (the spill form: up to the end of the seam)
    const uint32_t un_lds =
        !kSpill ? unshared
                : uint32_t(min<uint64_t>(klen, uint64_t(keycap) + kSpillSeam) - min<uint64_t>(shared, uint64_t(keycap) + kSpillSeam));
    for (uint32_t i0 = 16u * l; i0 < un_lds; i0 += 16u * kWave) {
      const uint4 w = S.ld16(int64_t(kp + i0));
      const uint32_t n = min(16u, un_lds - i0);
#pragma unroll
      for (uint32_t k = 0; k < 16; k++)
        if (k < n) keybuf[shared + i0 + k] = uint8_t(win_byte(w, k));
    }
    if constexpr (kSpill) {
      if (klen > keycap) {
        // key bytes [max(shared, C), klen) -> the slot, by its 16-B granules;
        // slot offset x holds block byte d + x
        const uint64_t lo = max<uint64_t>(shared, keycap) - keycap, hi = klen - keycap;
        const int64_t d = int64_t(kp) + int64_t(keycap) - int64_t(shared);
        for (uint64_t ga = (lo & ~uint64_t(15)) + 16ull * l; ga < hi; ga += 16ull * kWave)
          spill_put16(spill, ga, lo, hi, S.ld16(d + int64_t(ga)));
        // the stores reach L2 before any read of the slot
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    wave_sync();
    full_len = klen;
    uint64_t trailer, ukl, raw = 0;
    uint32_t fl = 0;
    if (!(flags & PBL_ROW_RAW_KEYS) && klen >= 8) {
      if (kSpill && klen > uint64_t(keycap) + kSpillSeam) {  // wholly past C
#pragma unroll
        for (int i = 0; i < 8; i++) raw |= uint64_t(spill_byte(spill, klen - 8 - keycap + i)) << (8 * i);
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++) raw |= uint64_t(keybuf[klen - 8 + i]) << (8 * i);
      }
    }
    split_trailer(raw, klen, flags, &trailer, &ukl, &fl);
    // blockiter.Transforms.HideObsoletePoints: the entry is skipped before its
    // value is looked at (rowblk_iter.go:1168-1179); its key still feeds the
    // prefix compression of the entries after it
    if ((flags & PBL_ROW_HIDE_OBSOLETE) && (fl & PBL_KV_OBSOLETE)) {
      offset = int64_t(vp) + vlen;
      continue;
    }
    uint64_t v = vp, vl = vlen;
    if ((flags & PBL_ROW_VALUE_PREFIX) && !(flags & PBL_ROW_RAW_KEYS) && (trailer & 0xff) == 1) {
      if (vl == 0) { status = PBL_CORRUPT_BOUNDS; break; }
      uint32_t skip;
      value_prefix(S.byte(v), flags, &skip, &fl);
      v += skip;
      vl -= skip;
    }
    if (pass == kPassAll) {
      while (ri < uint32_t(nr) && int64_t(rw_ri & kRestartMask) < offset) {
        ri++;
        if (ri < uint32_t(nr)) rw_ri = S.le32(uint64_t(restarts) + 4 * ri);
      }
      if (ri < uint32_t(nr)) {
        const uint32_t rw = rw_ri;
        if (int64_t(rw & kRestartMask) == offset) {
          fl |= PBL_KV_RESTART;
          if (rw & 0x80000000u) fl |= PBL_KV_RESTART_SAMEPFX;
        }
      }
      const uint64_t kv = bases[0] + nkv, o = bases[0] + b + nkv;
      if (l == 0) {
        o_trailer[kv] = with_seq(trailer, seq, flags);
        if (O.kv_flags) o_flags[kv] = uint8_t(fl);
        if (O.entry_off) o_entry[kv] = uint32_t(offset);
        o_koff[o] = uint32_t(kb);
        o_voff[o] = uint32_t(vb);
      }
      // user key: 16-B destination granules gathered from the key buffer
      {
        const uint64_t lo = bases[1] + kb, hi = lo + ukl;
        for (uint64_t ga = (lo & ~uint64_t(15)) + 16ull * l; ga < hi; ga += 16ull * kWave) {
          if (kSpill && int64_t(ga - lo) > int64_t(keycap))  // a window past C: from the slot
            store16(O.key_bytes, ga, lo, hi, spill_get16(spill, (ga - lo) - keycap));
          else
            store16(O.key_bytes, ga, lo, hi, lds_gather16(KW, uint32_t(int64_t(kKeyBufPad) + int64_t(ga - lo))));
        }
      }
    }
    if (pass == kPassAll) {
      // value: 16-B destination granules from source windows, U per lane in flight
      const uint64_t lo = bases[2] + vb, hi = lo + vl;
      if constexpr (std::is_same<Src, GlbBlk>::value) {
        S.template copy<U>(v, O.val_bytes, lo, hi);
      } else {
        for (uint64_t g0 = (lo & ~uint64_t(15)) + 16ull * l; g0 < hi; g0 += 16ull * kWave * U) {
          uint4 w[U];
#pragma unroll
          for (int u = 0; u < U; u++) {
            const uint64_t ga = g0 + 16ull * kWave * u;
            w[u] = ga < hi ? S.ld16(int64_t(v) + int64_t(ga - lo)) : make_uint4(0, 0, 0, 0);
          }
#pragma unroll
          for (int u = 0; u < U; u++) {
            const uint64_t ga = g0 + 16ull * kWave * u;
            if (ga < hi) store16(O.val_bytes, ga, lo, hi, w[u]);
          }
        }
      }
    }
    nkv++;
    kb += ukl;
    vb += vl;
    offset = int64_t(vp) + vlen;
  }
  if (status == PBL_OK && (kb >> 32 || vb >> 32)) status = PBL_UNSUPPORTED;
  if (pass == kPassAll && status == PBL_OK) {
    const uint64_t o = bases[0] + b + nkv;
    if (l == 0) { o_koff[o] = uint32_t(kb); o_voff[o] = uint32_t(vb); }
    if (O.restarts) {
      const gptr<uint32_t> o_rst = to_glb(O.restarts);
      for (int32_t r = l; r < nr; r += kWave) o_rst[bases[3] + r] = S.le32(uint64_t(restarts) + 4ull * r);
    }
  }
  st->status = status;
  st->nkv = nkv;
  st->kb = kb;
  st->vb = vb;
  st->nr = uint64_t(nr);
}

// blk: the block's first byte, in LDS (staged, blk_lds) or global memory;
// keybuf: LDS (dword aligned) of keycap bytes.
__device__ __noinline__ void slow_walk(const uint8_t* blk, bool blk_lds, uint64_t len, uint32_t flags, uint64_t seq,
                                       uint8_t* keybuf, uint32_t keycap, int pass, const pbl_decode_out O,
                                       uint32_t b, const uint64_t* bases_p, SlowState* st) {
  const uint64_t bases[kNumComp] = {bases_p[0], bases_p[1], bases_p[2], bases_p[3]};
  const lptr<uint8_t> kbuf = to_lds_ptr(keybuf);
  if (blk_lds) {
    // View base: the 16-B granule below the block's own granule (ld16 windows
    // start up to 15 bytes early; the staging buffers carry a 16-B front pad)
    const uint32_t a = uint32_t(uint64_t(to_lds_ptr(blk)));
    const uint32_t base = 16u + (a & 15u);
    slow_walk_t<LdsBlk, PBL_SLOW_U>(LdsBlk{lds_view(reinterpret_cast<const void*>(blk - base), base)}, len, flags,
                                     seq, kbuf, keycap, pass, O, b, bases, st);
  } else {
    slow_walk_t<GlbBlk, PBL_SLOW_U>(GlbBlk{to_glb(blk), len}, len, flags, seq, kbuf, keycap, pass, O, b, bases, st);
  }
}

}  // namespace row
}  // namespace pbl
