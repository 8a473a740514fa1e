// filter_core.hip.h — the rules of the table bloom filter, stated once
// (DESIGN.md §3.17): the key hash, the filter block's trailer, the probe of one
// 64-byte line, the setting of a hash's bits.  This is the RocksDB full-file
// format that sstable/tablefilters/bloom reads and writes
// ("rocksdb.BuiltinBloomFilter"): nLines * 64 bytes of bits, one byte of
// probes, LE32 nLines.  Every function is templated on a byte reader R
// (key_cmp.hip.h): filter.hip and seek.hip instantiate them with GlobalReader
// in their kernels and with cmp::HostReader in the host forms; no rule is
// restated anywhere else.
//
// The reader gives, besides key_cmp.hip.h's list,
//   R::load_le16(a, n, w)   16 bytes at `a` as four little-endian words, of
//                           which only the first min(n, 16) bytes are used
//                           (HostReader reads no byte past n; GlobalReader
//                           loads all 16: every key array of this library is
//                           readable 16 B past its end)
#pragma once
#include "key_cmp.hip.h"

namespace pbl {
namespace filter {

constexpr uint32_t kSeed = 0xbc9f1d34u, kMul = 0xc6a4a793u;
constexpr uint32_t kLine = 64;     // bytes per line (bits.go cacheLineSize)
constexpr uint64_t kTrailer = 5;   // probes byte + LE32 nLines
// A/B measurement, no effect on results: 1 (the default, the
// faster of the two on the device) loads the whole line as sixteen words and
// picks the probed bits out of registers; 0 loads the probed bytes.  The host
// forms always read the probed bytes.
#ifndef PBL_FILTER_WIDE_LINE
#define PBL_FILTER_WIDE_LINE 1
#endif

// bloom.go:41-78.  Four bytes little-endian per step; the 1 to 3 tail bytes are
// sign-extended (uint32(int8(b))), which is what RocksDB's char arithmetic did.
template <class R>
PBL_HD inline uint32_t bloom_hash(cmp::kptr<R> k, uint64_t len) {
  uint32_t h = kSeed ^ (uint32_t(len) * kMul);
  for (uint64_t o = 0; o < len; o += 16) {
    const uint64_t left = len - o;
    uint32_t w[4];
    R::load_le16(k + o, left, w);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      if (4 * j + 4 <= left) {
        h += w[j];
        h *= kMul;
        h ^= h >> 16;
      } else if (4 * j < left) {
        const uint32_t r = uint32_t(left) - 4 * j;
        if (r == 3) h += uint32_t(int32_t(int8_t(w[j] >> 16))) << 16;
        if (r >= 2) h += uint32_t(int32_t(int8_t(w[j] >> 8))) << 8;
        h += uint32_t(int32_t(int8_t(w[j])));
        h *= kMul;
        h ^= h >> 24;
      }
    }
  }
  return h;
}

struct Header {
  uint32_t n_lines;   // 0: the filter holds nothing, or is corrupt
  uint32_t n_probes;  // 0 .. 255
  int32_t status;     // PBL_OK / PBL_CORRUPT_FILTER
};

// bits.go:93-105.  A filter of five bytes or fewer holds nothing; nLines must
// be what the length says (the reference panics where it is not).  After the
// check n_lines * 64 <= len - 5: no probe reads outside the filter.
template <class R>
PBL_HD inline Header bloom_parse(cmp::kptr<R> f, uint64_t len) {
  Header H{0u, 0u, PBL_OK};
  if (len <= kTrailer) return H;
  const uint64_t n = len - kTrailer;
  H.n_probes = f[n];
  const uint32_t nl = uint32_t(f[n + 1]) | uint32_t(f[n + 2]) << 8 | uint32_t(f[n + 3]) << 16 | uint32_t(f[n + 4]) << 24;
  if (nl == 0 || n / nl != kLine) {
    H.status = PBL_CORRUPT_FILTER;
    return H;
  }
  H.n_lines = nl;
  return H;
}

PBL_HD inline uint32_t rotr17(uint32_t h) { return h >> 17 | h << 15; }

// bits.go:39-53 over a parsed filter with n_lines > 0: every probe's bit of
// line h % n_lines.  The reference leaves at the first clear bit; here every
// load is issued before any bit is tested (a CPU's early exit would make each
// load wait for the one before it): the whole line on the device, the probed
// bytes eight at a time on the host.
template <class R>
PBL_HD inline bool bloom_probe(cmp::kptr<R> bits, const Header& H, uint32_t h) {
  const uint32_t delta = rotr17(h);
  const cmp::kptr<R> line = bits + uint64_t(h % H.n_lines) * kLine;
  uint32_t all = 1;
#if PBL_FILTER_WIDE_LINE && defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t u32u __attribute__((aligned(1)));
  uint32_t wd[16];
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) wd[j] = ((typename R::template ptr<const u32u>)line)[j];
  for (uint32_t p = 0; p < H.n_probes; p++) {
    const uint32_t at = (h >> 5) & 15;
    uint32_t x = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) x = at == j ? wd[j] : x;
    all &= x >> (h & 31);
    h += delta;
  }
#else
  for (uint32_t p0 = 0; p0 < H.n_probes; p0 += 8) {
    uint32_t b[8];
#pragma unroll
    for (uint32_t e = 0; e < 8; e++) {
      // (a probe past n_probes still reads its byte, which lies inside the
      // line, and is then not counted: eight loads and no branch)
      b[e] = uint32_t(line[(h >> 3) & (kLine - 1)]) >> (h & 7);
      h += delta;
    }
#pragma unroll
    for (uint32_t e = 0; e < 8; e++) all &= p0 + e < H.n_probes ? b[e] : 1u;
  }
#endif
  return (all & 1) != 0;
}

// MayContain (bits.go:93-105) of hash h in a parsed filter: a filter that holds
// nothing contains nothing, a corrupt one may contain anything (a caller that
// ignores statuses must never lose a key).
template <class R>
PBL_HD inline bool bloom_may(cmp::kptr<R> bits, const Header& H, uint32_t h) {
  if (H.n_lines == 0) return H.status != PBL_OK;
  return bloom_probe<R>(bits, H, h);
}

// bloom_hash of key[:Split(key)]: what a table's filter holds of a key.
template <class R>
PBL_HD inline uint32_t prefix_hash(uint32_t cmp, cmp::kptr<R> k, uint64_t kl) {
  return bloom_hash<R>(k, cmp::key_split<R>(cmp, k, kl));
}

// ---- the writer side (host only; bloom.go:100-123, bits.go:56-89) --------------
inline uint32_t probes_for(uint32_t bits_per_key) {  // bloom.go:23-38
  static const uint8_t t[11] = {0, 1, 1, 2, 3, 3, 4, 4, 5, 5, 6};
  return t[bits_per_key < 10 ? bits_per_key : 10];
}
inline uint64_t lines_for(uint64_t n_hashes, uint32_t bits_per_key) {
  return ((n_hashes * bits_per_key + 8 * kLine - 1) / (8 * kLine)) | 1;
}
inline void bloom_set(uint8_t* bits, uint32_t n_lines, uint32_t n_probes, uint32_t h) {
  const uint32_t delta = rotr17(h);
  uint8_t* line = bits + uint64_t(h % n_lines) * kLine;
  for (uint32_t p = 0; p < n_probes; p++) {
    line[(h >> 3) & (kLine - 1)] |= uint8_t(1u << (h & 7));
    h += delta;
  }
}

}  // namespace filter
}  // namespace pbl
