// span_run.hip.h — a RUN of span fragments read as two sorted key lists, stated
// once for range deletions (rangedel.hip) and range keys
// (rangekey.hip, §3.16): visibility at a snapshot, the upper-bound search, the
// run's view and the order part of the fragmentation check.  Templated on a
// byte reader R like everything in seek_core.hip.h.
#pragma once
#include "seek_core.hip.h"

namespace pbl {
namespace span {

PBL_HD inline bool is_visible(uint64_t seq, uint64_t snapshot) { return snapshot >= PBL_SEQNUM_MAX || seq < snapshot; }

// The first KV of the block whose user key is > the query (n when there is
// none): seek::lower's search with the other inequality.
template <class R>
PBL_HD inline uint32_t upper(uint32_t cmp, const seek::Block<R>& B, cmp::kptr<R> k, uint64_t kl) {
  uint32_t lo = 0, hi = B.n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    uint64_t ml;
    const cmp::kptr<R> mk = B.key(m, &ml);
    if (cmp::key_cmp<R>(cmp, mk, ml, k, kl) <= 0) lo = m + 1;
    else hi = m;
  }
  return lo;
}

// One run's two sorted lists: S.key(j) = fragment j's start, E.key(j) = its end
// (the value arrays read as keys), tr[j] its trailer.
template <class R>
struct Run {
  seek::Block<R> S, E;
  typename R::template ptr<const uint64_t> tr;
  typename R::template ptr<const uint8_t> fl;  // kv_flags or NULL
};
// Block b of D as a run (rangedel.hip's runs have one block; a clipped range-key
// batch has one per range).
template <class R>
PBL_HD inline Run<R> run_of(const pbl_decode_out& D, uint32_t b = 0, uint32_t nb = 1) {
  pbl_seek_queries sq{};
  const seek::View<R> VS(D, nb, sq, nullptr, 0);
  pbl_decode_out e = D;
  e.key_off = D.val_off;
  e.key_bytes = D.val_bytes;
  e.blk_key_base = D.blk_val_base;
  const seek::View<R> VE(e, nb, sq, nullptr, 0);
  const seek::Block<R> S(VS, b), E(VE, b);
  using P64 = typename R::template ptr<const uint64_t>;
  using P8 = typename R::template ptr<const uint8_t>;
  return Run<R>{S, E, (P64)D.trailer + S.kv0, D.kv_flags ? (P8)D.kv_flags + S.kv0 : (P8) nullptr};
}

// Fragment j of a run against itself and its successor: whether the run is not
// fragmented there (start <= end; starts ascending; equal starts have equal ends
// and trailers descending; otherwise end_j <= start_{j+1}).
template <class R>
PBL_HD inline bool unordered_at(uint32_t cmpr, const Run<R>& U, uint32_t j) {
  bool bad = false;
  uint64_t sl, el;
  const cmp::kptr<R> s = U.S.key(j, &sl), e = U.E.key(j, &el);
  // (start == end is an empty fragment that covers nothing: the reference's own
  // fixture tables hold one, [a, a), and its readers pass over it)
  if (cmp::key_cmp<R>(cmpr, s, sl, e, el) > 0) bad = true;
  if (j + 1 < U.S.n) {
    uint64_t s2l, e2l;
    const cmp::kptr<R> s2 = U.S.key(j + 1, &s2l), e2 = U.E.key(j + 1, &e2l);
    const int c = cmp::key_cmp<R>(cmpr, s, sl, s2, s2l);
    if (c > 0) bad = true;
    else if (c == 0) {
      if (U.tr[j] < U.tr[j + 1] || cmp::key_cmp<R>(cmpr, e, el, e2, e2l) != 0) bad = true;
    } else if (cmp::key_cmp<R>(cmpr, e, el, s2, s2l) > 0) {
      bad = true;
    }
  }
  return bad;
}

}  // namespace span
}  // namespace pbl
