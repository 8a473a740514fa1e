// key_cmp.hip.h — the one statement of the three comparers, for host and device.
//
// base.DefaultComparer (internal/base/comparer.go: bytes.Compare, Split = len),
// testkeys.Comparer (internal/testkeys/testkeys.go:136-171) and
// cockroachkvs.Comparer (cockroachkvs/cockroachkvs.go:298-339, :479-...).
// data_iter.cpp (the host blockiter.Data adapter) and seek.hip (the batched
// seeks, host and device) both instantiate these; neither restates a rule.
//
// Every function is templated on a byte reader R (the way row::varint_at is
// templated on its byte source):
//   R::ptr<T>                          the pointer type the keys are read through
//   R::bytes_cmp(a, al, b, bl)         bytes.Compare: -1 / 0 / +1
//   R::load_be16(a, n, &w0, &w1)       the first min(n, 16) bytes as two
//                                      big-endian words, zero padded
// The bytewise compare is the one part a reader may specialise (HostReader:
// memcmp, never reading past a key; seek.hip's GlobalReader: 16 B at a time
// through address_space(1) pointers).  The suffix rules below are written once.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/pebble_amd.h"

#ifdef __HIP__
#define PBL_HD __host__ __device__
#else
#define PBL_HD  // a host-only translation unit
#endif

namespace pbl {
namespace cmp {

struct HostReader {
  template <class T>
  using ptr = T*;
  static int bytes_cmp(const uint8_t* a, uint64_t al, const uint8_t* b, uint64_t bl) {
    const int c = memcmp(a, b, al < bl ? al : bl);
    if (c) return c < 0 ? -1 : 1;
    return al < bl ? -1 : al > bl ? 1 : 0;
  }
  static void load_be16(const uint8_t* a, uint64_t n, uint64_t* w0, uint64_t* w1) {
    uint64_t w[2] = {0, 0};
    for (uint64_t i = 0; i < n && i < 16; i++) w[i >> 3] |= uint64_t(a[i]) << (56 - 8 * (i & 7));
    *w0 = w[0];
    *w1 = w[1];
  }
  // the first min(n, 16) bytes as four little-endian words, zero padded
  static void load_le16(const uint8_t* a, uint64_t n, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (uint64_t i = 0; i < n && i < 16; i++) w[i >> 2] |= uint32_t(a[i]) << (8 * (i & 3));
  }
};

template <class R>
using kptr = typename R::template ptr<const uint8_t>;

// ---- testkeys.Comparer -------------------------------------------------------
template <class R>
PBL_HD inline uint64_t tk_split(kptr<R> a, uint64_t n) {
  for (uint64_t i = n; i > 0; i--)
    if (a[i - 1] == '@') return i - 1;
  return n;
}
// the suffix without a trailing "_synthetic" (testkeys.go ignorableSuffix)
template <class R>
PBL_HD inline uint64_t tk_trim(kptr<R> s, uint64_t n) {
  const uint64_t il = 10;
  if (n < il) return n;
  for (uint64_t k = 0; k < il; k++)
    if (s[n - il + k] != uint8_t("_synthetic"[k])) return n;
  return n - il;
}
// "@N" -> N (parseUintBytes base 10); malformed suffixes (Go panics) sort by bytes
template <class R>
PBL_HD inline bool tk_ts(kptr<R> s, uint64_t n, uint64_t* v) {
  n = tk_trim<R>(s, n);
  if (n < 2 || s[0] != '@') return false;
  uint64_t x = 0;
  for (uint64_t k = 1; k < n; k++) {
    if (s[k] < '0' || s[k] > '9') return false;
    x = x * 10 + (s[k] - '0');
  }
  *v = x;
  return true;
}
template <class R>
PBL_HD inline int tk_cmp(kptr<R> a, uint64_t al, kptr<R> b, uint64_t bl) {
  const uint64_t ai = tk_split<R>(a, al), bi = tk_split<R>(b, bl);
  const int c = R::bytes_cmp(a, ai, b, bi);
  if (c) return c;
  const uint64_t as = tk_trim<R>(a + ai, al - ai), bs = tk_trim<R>(b + bi, bl - bi);
  if (as == 0 || bs == 0) return as < bs ? -1 : as > bs ? 1 : 0;  // the empty suffix sorts first
  uint64_t x, y;
  if (!tk_ts<R>(a + ai, al - ai, &x) || !tk_ts<R>(b + bi, bl - bi, &y)) return R::bytes_cmp(a + ai, as, b + bi, bs);
  return y < x ? -1 : y > x ? 1 : 0;  // cmp.Compare(bi, ai): newer first
}

// ---- cockroachkvs.Comparer ---------------------------------------------------
template <class R>
PBL_HD inline uint64_t crdb_split(kptr<R> a, uint64_t n) {  // cockroachkvs.go:298-311
  if (n == 0) return 0;
  const uint64_t s = uint64_t(a[n - 1]);
  return s <= n ? n - s : 0;
}
// normalizeEngineSuffixForCompare (cockroachkvs.go): the suffix without its
// length byte, with a zero logical component and a synthetic bit dropped so that
// equal timestamps compare equal
template <class R>
PBL_HD inline uint64_t crdb_norm(kptr<R> s, uint64_t n) {
  if (n == 0) return 0;
  uint64_t v = n - 1;  // the version, without the length byte
  // engineKeyVersionWallLogicalAndSyntheticTimeLen = 13, WallAndLogical = 12,
  // WallTime = 8: drop the synthetic byte, then a zero logical
  if (v == 13) v = 12;
  if (v == 12) {
    kptr<R> lg = s + 8;
    if (lg[0] == 0 && lg[1] == 0 && lg[2] == 0 && lg[3] == 0) v = 8;
  }
  return v;
}
template <class R>
PBL_HD inline int crdb_cmp(kptr<R> a, uint64_t al, kptr<R> b, uint64_t bl) {  // cockroachkvs.go:313-339
  if (al == 0 || bl == 0) return al < bl ? -1 : al > bl ? 1 : 0;
  const uint64_t asl = a[al - 1], bsl = b[bl - 1];
  const uint64_t ass = asl <= al ? al - asl : 0, bss = bsl <= bl ? bl - bsl : 0;
  const int c = R::bytes_cmp(a, ass, b, bss);
  if (c) return c;
  if (asl == 0 || bsl == 0) return asl < bsl ? -1 : asl > bsl ? 1 : 0;
  const uint64_t an = crdb_norm<R>(a + ass, al - ass), bn = crdb_norm<R>(b + bss, bl - bss);
  return R::bytes_cmp(b + bss, bn, a + ass, an);  // descending versions
}

template <class R>
PBL_HD inline int key_cmp(uint32_t cmp, kptr<R> a, uint64_t al, kptr<R> b, uint64_t bl) {
  switch (cmp) {
    case PBL_CMP_TESTKEYS: return tk_cmp<R>(a, al, b, bl);
    case PBL_CMP_CRDB: return crdb_cmp<R>(a, al, b, bl);
    default: return R::bytes_cmp(a, al, b, bl);
  }
}
// Comparer.CompareRangeSuffixes: the order of range-key suffixes (DESIGN.md
// §3.16).  It is not key_cmp's suffix step: bytes.Compare for the default
// comparer (internal/base/comparer.go:317); testkeys' compareSuffixes
// (testkeys.go:173-186), which orders two equal timestamps by the "_synthetic"
// mark (the unmarked one first); cockroachkvs.CompareRangeSuffixes
// (cockroachkvs.go:346-355), the versions without their length byte, descending
// and NOT normalised.  Malformed testkeys suffixes sort by bytes, as in tk_cmp.
template <class R>
PBL_HD inline int suffix_cmp(uint32_t cmp, kptr<R> a, uint64_t al, kptr<R> b, uint64_t bl) {
  switch (cmp) {
    case PBL_CMP_TESTKEYS: {
      const uint64_t at = tk_trim<R>(a, al), bt = tk_trim<R>(b, bl);
      int c;
      uint64_t x, y;
      if (at == 0 || bt == 0) c = at < bt ? -1 : at > bt ? 1 : 0;
      else if (!tk_ts<R>(a, at, &x) || !tk_ts<R>(b, bt, &y)) c = R::bytes_cmp(a, at, b, bt);
      else c = y < x ? -1 : y > x ? 1 : 0;
      if (c == 0 && (at != al) != (bt != bl)) c = at != al ? 1 : -1;
      return c;
    }
    case PBL_CMP_CRDB:
      if (al == 0 || bl == 0) return al < bl ? -1 : al > bl ? 1 : 0;
      return R::bytes_cmp(b, bl - 1, a, al - 1);
    default: return R::bytes_cmp(a, al, b, bl);
  }
}
// base.InternalCompare (internal/base/internal.go:431-437), which is also
// mergingIterHeap.less (merging_iter_heap.go:55-67): the user keys under the
// comparer, then the trailers in reverse (the newer version sorts first).
template <class R, uint32_t kCmp>
PBL_HD inline int ikey_cmp(kptr<R> a, uint64_t al, uint64_t atr, kptr<R> b, uint64_t bl, uint64_t btr) {
  const int c = key_cmp<R>(kCmp, a, al, b, bl);
  if (c) return c;
  return atr > btr ? -1 : atr < btr ? 1 : 0;
}
template <class R>
PBL_HD inline uint64_t key_split(uint32_t cmp, kptr<R> a, uint64_t n) {
  switch (cmp) {
    case PBL_CMP_TESTKEYS: return tk_split<R>(a, n);
    case PBL_CMP_CRDB: return crdb_split<R>(a, n);
    default: return n;
  }
}

}  // namespace cmp
}  // namespace pbl
