// rowblk_core.hip.h — the row-block rules every row kernel shares, stated once:
// the staged-block View and its 16-byte gathers, the uint32 varint, the LDS
// and global block readers, the entry header (general and 1-3 byte forms),
// the Iter.Init checks, the trailer split, the value-prefix classification and
// the diagnostic phase stamps.
//
// Semantics follow cockroachdb/pebble sstable/rowblk/rowblk_iter.go:
//   Init :241-276, readFirstKey :418-485, readEntry :333-416 (three uint32
//   varints :345-398, decoder :2020-2038), decodeInternalKey :487-504 (LE64
//   trailer & TrailerObsoleteMask, < 8 B => InternalKeyKindInvalid), value
//   prefix :1192-1199 (sstable/block/kv.go:14-41).
#pragma once

#include "common.hip.h"

namespace pbl {
namespace row {

constexpr int kPad = 16;                  // LDS front pad: segment gathers may start up to 15 B early
constexpr int kLdsBlkBytes = kPad + 32768 + 32;  // block staging (any 16-B phase of a <=32 KiB block)
constexpr uint32_t kMaxFastLen = 32768;   // blocks up to this length take the LDS path
constexpr uint32_t kRestartMask = 0x7fffffffu;
constexpr uint64_t kTrailerObsoleteMask = ((((uint64_t)1 << 56) - 1) << 8) | 191u;
constexpr uint64_t kKindInvalid = kKindInvalidTrailer;

#ifdef PBL_STAMPS
// diagnostic build only: per-block phase timestamps (s_memtime) written past the
// look-back state in the workspace; never part of an output
#define PSTAMP(A_, b_, i_, lane0_)                                                             \
  do {                                                                                          \
    if (lane0_)                                                                                 \
      reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>((A_).out.workspace) +             \
                                  ws_bytes((A_).in.n_blocks))[uint64_t(b_) * 16 + (i_)] =       \
          __builtin_amdgcn_s_memtime();                                                         \
  } while (0)
// slot i_ = the wave's HW_ID (SIMD / CU / SE) and XCC_ID: where the roles run
#define PHWID(A_, b_, i_, lane0_)                                                              \
  do {                                                                                          \
    if (lane0_)                                                                                 \
      reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>((A_).out.workspace) +             \
                                  ws_bytes((A_).in.n_blocks))[uint64_t(b_) * 16 + (i_)] =       \
          uint64_t(__builtin_amdgcn_s_getreg(4 | (31 << 11))) |                                 \
          uint64_t(__builtin_amdgcn_s_getreg(20 | (15 << 11))) << 32;                           \
  } while (0)
#else
#define PSTAMP(A_, b_, i_, lane0_) do {} while (0)
#define PHWID(A_, b_, i_, lane0_) do {} while (0)
#endif

// Unaligned LDS access.  gfx950 runs in unaligned access mode (the HSA
// runtime's default), where one ds_read_b128 / b64 / b32 serves any byte
// address: a 16-byte gather is one instruction instead of five dword reads
// and four alignbytes.  Measured on config 2 (same box, A/B): unaligned 16-byte
// gathers +2.7 % (992 vs 965 GiB/s), unaligned 8-byte header reads in the
// parse walk -1.5 %; so gathers are unaligned and ld8/le32 stay dword reads
// (PBL_LDS_UA8 / PBL_LDS_UA16 switch each form for A/B builds).
typedef u32x4 u32x4_u __attribute__((aligned(1)));
typedef u32x2 u32x2_u __attribute__((aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));
#ifndef PBL_LDS_UA8
#define PBL_LDS_UA8 0
#endif
#ifndef PBL_LDS_UA16
#define PBL_LDS_UA16 1
#endif

// 16 bytes at LDS byte address a (any alignment)
__device__ inline uint4 lds_gather16(lptr<const uint32_t> W, uint32_t a) {
#if !PBL_LDS_UA16
  uint32_t q = a >> 2, r = a & 3;
  uint32_t x0 = W[q], x1 = W[q + 1], x2 = W[q + 2], x3 = W[q + 3], x4 = W[q + 4];
  return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, r), __builtin_amdgcn_alignbyte(x2, x1, r),
                    __builtin_amdgcn_alignbyte(x3, x2, r), __builtin_amdgcn_alignbyte(x4, x3, r));
#else
  const u32x4 v = *(lptr<const u32x4_u>)(reinterpret_cast<lptr<const uint8_t>>(W) + a);
  return make_uint4(v.x, v.y, v.z, v.w);
#endif
}

// Read-only view of the staged block: its base offset lives in a register.
struct View {
  lptr<const uint8_t> B;   // LDS bytes (array start)
  lptr<const uint32_t> W;  // LDS words (array start)
  uint32_t base;      // byte index of block byte 0 (kPad + shift)
  __device__ inline uint32_t byte(uint32_t i) const { return B[base + i]; }
  // 8 block bytes [i, i+8) as a little-endian u64
  __device__ inline uint64_t ld8(uint32_t i) const {
#if !PBL_LDS_UA8
    uint32_t a = base + i, q = a >> 2, r = a & 3;
    uint32_t x0 = W[q], x1 = W[q + 1], x2 = W[q + 2];
    uint32_t lo = __builtin_amdgcn_alignbyte(x1, x0, r);
    uint32_t hi = __builtin_amdgcn_alignbyte(x2, x1, r);
    return uint64_t(hi) << 32 | lo;
#else
    const u32x2 v = *(lptr<const u32x2_u>)(B + base + i);
    return uint64_t(v.y) << 32 | v.x;
#endif
  }
  __device__ inline uint32_t le32(uint32_t i) const {
#if !PBL_LDS_UA8
    uint32_t a = base + i, q = a >> 2, r = a & 3;
    return __builtin_amdgcn_alignbyte(W[q + 1], W[q], r);
#else
    return *(lptr<const u32_u>)(B + base + i);
#endif
  }
  // 16 block bytes starting at block offset i (i may be up to 15 below 0)
  __device__ inline uint4 ld16(int32_t i) const { return lds_gather16(W, uint32_t(int32_t(base) + i)); }
};

__device__ __forceinline__ View lds_view(const void* lds, uint32_t base) {
  return View{to_lds_ptr(reinterpret_cast<const uint8_t*>(lds)), to_lds_ptr(reinterpret_cast<const uint32_t*>(lds)),
              base};
}

// mask of the low n bytes of a word, n clamped to [0, 4]
__device__ inline uint32_t low_bytes(int n) {
  n = n < 0 ? 0 : n;
  return n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
}
// byte mask of bytes [a, b) within the 4-byte word k of a 16-byte granule
__device__ inline uint32_t word_mask(int k, uint32_t a, uint32_t b) {
  return low_bytes(int(b) - 4 * k) & ~low_bytes(int(a) - 4 * k);
}
__device__ inline void merge16(uint4& w, const uint4& v, uint32_t a, uint32_t b) {
  uint32_t m;
  m = word_mask(0, a, b); w.x = (w.x & ~m) | (v.x & m);
  m = word_mask(1, a, b); w.y = (w.y & ~m) | (v.y & m);
  m = word_mask(2, a, b); w.z = (w.z & ~m) | (v.z & m);
  m = word_mask(3, a, b); w.w = (w.w & ~m) | (v.w & m);
}

// uint32 varint (rowblk_iter.go:2020-2038) from a byte fetch at(0), at(1), ...
// of which n bytes exist: the 5th byte is shifted left by 28 whatever its high
// bits, no byte at or past n is fetched.  Returns the bytes used, 0 if the
// varint runs past n.
template <class At>
__device__ __forceinline__ uint32_t varint_at(At at, uint32_t n, uint32_t* v) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t i = 0; i < 5; i++) {
    if (i >= n) return 0;
    const uint32_t b = at(i);
    if (i == 4) { *v = r | (b << 28); return 5; }
    r |= (b & 0x7f) << (7 * i);
    if (b < 128) { *v = r; return i + 1; }
  }
  return 0;
}

// Block readers.  Both read bytes, LE32 words, varints and 16-byte windows at
// block offsets; an ld16 window may start up to 15 bytes before the block or
// end past it (those bytes are don't-cares; nothing outside the block's 16-B
// granules is touched).  Typed address spaces throughout: a generic (FLAT) LDS
// read would wait for every outstanding global store.
struct LdsBlk {  // block staged in LDS (byte 0 at B[base])
  View V;
  __device__ __forceinline__ uint32_t byte(uint32_t i) const { return V.byte(i); }
  __device__ __forceinline__ uint32_t le32(uint32_t i) const { return V.le32(i); }
  __device__ __forceinline__ uint4 ld16(int32_t i) const { return V.ld16(i); }
  __device__ __forceinline__ uint32_t varint(uint32_t p, uint32_t end, uint32_t* v) const {
    return varint_at([this, p](uint32_t i) { return V.byte(p + i); }, end > p ? end - p : 0u, v);
  }
};
struct GlbBlk {  // block in global memory
  gptr<const uint8_t> g;
  uint64_t len;
  __device__ __forceinline__ uint32_t byte(uint64_t i) const { return g[i]; }
  __device__ __forceinline__ uint32_t le32(uint64_t i) const {
    return uint32_t(g[i]) | uint32_t(g[i + 1]) << 8 | uint32_t(g[i + 2]) << 16 | uint32_t(g[i + 3]) << 24;
  }
  __device__ __forceinline__ uint32_t varint(uint32_t p, uint32_t end, uint32_t* v) const {
    const gptr<const uint8_t> q = g + p;
    return varint_at([q](uint32_t i) { return uint32_t(q[i]); }, end > p ? end - p : 0u, v);
  }
  __device__ __forceinline__ uint4 ld16(int64_t i) const {
    const uint64_t s0 = uint64_t(g), s1 = s0 + len, sx = s0 + uint64_t(i), sa = sx & ~uint64_t(15);
    const uint32_t sh = uint32_t(sx - sa);
    uint4 x = make_uint4(0, 0, 0, 0), y = make_uint4(0, 0, 0, 0);
    if (sa + 16 > s0 && sa < s1) {
      const u32x4 v = *(gptr<const u32x4>)(sa);
      x = make_uint4(v.x, v.y, v.z, v.w);
    }
    if (sh && sa + 32 > s0 && sa + 16 < s1) {
      const u32x4 v = *(gptr<const u32x4>)(sa + 16);
      y = make_uint4(v.x, v.y, v.z, v.w);
    }
    return sh ? funnel16(x, y, sh) : x;
  }
  // Block bytes from offset v -> out[lo, hi), 16-B destination granules, U per
  // lane in flight.  Every granule's two source loads are issued before any is
  // used, at addresses clamped to the block's own granules (those bytes feed
  // only masked destination bytes); the shift is one per value.  Through ld16
  // each granule's guarded loads and funnel waited in turn: config 5's
  // big-block values pass, one 48 KB value per block, took 125 us.
  template <int U>
  __device__ __forceinline__ void copy(uint64_t v, uint8_t* out, uint64_t lo, uint64_t hi) const {
    const uint64_t s0 = uint64_t(g), g_lo = s0 & ~uint64_t(15), g_hi = (s0 + len - 1) & ~uint64_t(15);
    const uint64_t d = s0 + v - lo;  // source address of destination offset ga: d + ga
    const uint32_t sh = __builtin_amdgcn_readfirstlane(uint32_t(d) & 15u);
    for (uint64_t g0 = (lo & ~uint64_t(15)) + 16ull * lane_id(); g0 < hi; g0 += 16ull * kWave * U) {
      u32x4 x[U], y[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t sa = (d + g0 + 16ull * kWave * u) & ~uint64_t(15);
        x[u] = *(gptr<const u32x4>)(min(max(sa, g_lo), g_hi));
        if (sh) y[u] = *(gptr<const u32x4>)(min(max(sa + 16, g_lo), g_hi));
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint64_t ga = g0 + 16ull * kWave * u;
        const uint4 a = make_uint4(x[u].x, x[u].y, x[u].z, x[u].w);
        if (ga < hi)
          store16(out, ga, lo, hi, sh ? funnel16(a, make_uint4(y[u].x, y[u].y, y[u].z, y[u].w), sh) : a);
      }
    }
  }
};

// byte k (< 16) of a 16-byte window, by shifts (a runtime-indexed register
// array would live in scratch)
__device__ __forceinline__ uint32_t win_byte(const uint4& w, uint32_t k) {
  const uint64_t q = k < 8 ? (uint64_t(w.x) | uint64_t(w.y) << 32) : (uint64_t(w.z) | uint64_t(w.w) << 32);
  return uint32_t(q >> (8 * (k & 7))) & 0xffu;
}

// Entry header (readEntry :345-398): the three uint32 varints from the 16-byte
// window at the entry, of which `avail` (<= 15) bytes lie inside the block.
// Returns the header's length, 0 if a varint runs past `avail`.
__device__ __forceinline__ uint32_t entry_header(const uint4& w, uint32_t avail, uint32_t* shared, uint32_t* unshared,
                                                 uint32_t* vlen) {
  const auto from = [&w](uint32_t i0) { return [&w, i0](uint32_t i) { return win_byte(w, i0 + i); }; };
  const uint32_t a = varint_at(from(0), avail, shared);
  const uint32_t b = a ? varint_at(from(a), avail - a, unshared) : 0;
  const uint32_t c = b ? varint_at(from(a + b), avail - a - b, vlen) : 0;
  return c ? a + b + c : 0;
}

// The same header decoded without branches from the 8 bytes at the entry, for
// the lane-per-run walks.  The common 1-2 byte varints are decoded inline
// (hdr2); a 3-byte varint (values of 16 KiB and more, config 5) takes hdr3 on
// the lanes that need it.  False for anything longer: the block takes the
// general walk.
__device__ __forceinline__ bool hdr3(uint64_t w, uint32_t* sh, uint32_t* un, uint32_t* vl, uint32_t* h) {
  uint32_t p = 0, v[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t x = uint32_t(w >> (8 * p));  // p <= 6 here
    const uint32_t b0 = x & 0xff, b1 = (x >> 8) & 0xff, b2 = (x >> 16) & 0xff;
    const bool c0 = (b0 & 0x80) != 0, c1 = c0 && (b1 & 0x80) != 0;
    v[k] = c1 ? ((b0 & 0x7f) | ((b1 & 0x7f) << 7) | (b2 << 14)) : c0 ? ((b0 & 0x7f) | (b1 << 7)) : b0;
    ok = ok && !(c1 && (b2 & 0x80));
    p += c1 ? 3 : c0 ? 2 : 1;
  }
  *sh = v[0];
  *un = v[1];
  *vl = v[2];
  *h = p;
  // RunBuf packs unshared in 14 bits and the header length in 3
  return ok && p <= 7 && v[1] < 16384u;
}

__device__ __forceinline__ bool hdr2(uint64_t w, uint32_t* sh, uint32_t* un, uint32_t* vl, uint32_t* h) {
  if (__builtin_expect((uint32_t(w) & 0x808080u) == 0, 1)) {  // three 1-byte varints (values < 128)
    *sh = uint32_t(w) & 0xffu;
    *un = uint32_t(w >> 8) & 0xffu;
    *vl = uint32_t(w >> 16) & 0xffu;
    *h = 3;
    return true;
  }
  uint32_t p = 0, v[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint32_t x = uint32_t(w >> (8 * p));
    const uint32_t b0 = x & 0xff, b1 = (x >> 8) & 0xff;
    const bool two = (b0 & 0x80) != 0;
    v[k] = two ? ((b0 & 0x7f) | (b1 << 7)) : b0;
    ok = ok && !(two && (b1 & 0x80));
    p += two ? 2 : 1;
  }
  *sh = v[0];
  *un = v[1];
  *vl = v[2];
  *h = p;
  if (__builtin_expect(!ok, 0)) ok = hdr3(w, sh, un, vl, h);
  return ok;
}

// Init checks (Init :248-256, readFirstKey :418-485) evaluated by every lane.
// Returns the status; *roff_o / *nres_o are set when it is PBL_OK.
template <class Rd>
__device__ __forceinline__ uint32_t init_checks(const Rd& rd, uint32_t blen, uint32_t flags, uint32_t* roff_o,
                                                uint32_t* nres_o) {
  *roff_o = 0;
  *nres_o = 0;
  if (blen < 4) return PBL_CORRUPT_BOUNDS;
  const uint32_t nw = rd.le32(blen - 4);
  if (nw == 0) return PBL_CORRUPT_NO_RESTARTS;
  if (nw >> 31) return PBL_CORRUPT_BOUNDS;
  const uint64_t need = 4ull * (1ull + nw);
  if (need > blen) return PBL_CORRUPT_BOUNDS;
  const uint32_t roff = blen - uint32_t(need);
  if (roff > 0 && !(flags & PBL_ROW_RAW_KEYS)) {
    if (rd.byte(0) != 0) return PBL_CORRUPT_FIRST_KEY;
    uint32_t un, vl;
    const uint32_t n1 = rd.varint(1, blen, &un);
    const uint32_t n2 = n1 ? rd.varint(1 + n1, blen, &vl) : 0;
    if (!n2) return PBL_CORRUPT_BOUNDS;
    if (un < 8) return PBL_CORRUPT_FIRST_KEY;
  }
  *roff_o = roff;
  *nres_o = nw;
  return PBL_OK;
}

// decodeInternalKey (:487-504) of a key of klen bytes whose last 8 bytes are
// raw8 (little-endian; only looked at when the key has them): the trailer
// without the obsolete bit, the user key's length, and PBL_KV_OBSOLETE /
// PBL_KV_INVALID_KEY added to *fl.  PBL_ROW_RAW_KEYS: the whole key is the
// user key (RawIter.readEntry :1784-1794).
__device__ __forceinline__ void split_trailer(uint64_t raw8, uint64_t klen, uint32_t flags, uint64_t* trailer,
                                              uint64_t* ukl, uint32_t* fl) {
  if (flags & PBL_ROW_RAW_KEYS) {
    *trailer = 0;
    *ukl = klen;
  } else if (klen >= 8) {
    if (raw8 & 64u) *fl |= PBL_KV_OBSOLETE;
    *trailer = raw8 & kTrailerObsoleteMask;
    *ukl = klen - 8;
  } else {
    *trailer = kKindInvalid;
    *ukl = 0;
    *fl |= PBL_KV_INVALID_KEY;
  }
}

// Value prefix of a SET's non-empty value whose first byte is `pre` (:1192-1199,
// block/kv.go:14-41): an in-place value (or any value with PBL_ROW_NO_VALUER)
// drops the byte (*skip = 1); a handle keeps it and sets its kind in *fl.
__device__ __forceinline__ void value_prefix(uint32_t pre, uint32_t flags, uint32_t* skip, uint32_t* fl) {
  *skip = 0;
  if ((pre & 0xC0) == 0 || (flags & PBL_ROW_NO_VALUER)) *skip = 1;
  else *fl |= (pre & 0xC0) == 0x80 ? PBL_KV_VALBLK_HANDLE : PBL_KV_BLOB_HANDLE;
}

}  // namespace row
}  // namespace pbl
