// rangekey.hip — range keys in the device read path (DESIGN.md §3.16;
// include/pebble_amd.h states the rules): the coalesced, defragmented set of up
// to 16 runs of range-key fragments at a snapshot, its truncation to ranges,
// and the masking of every KV of a decoded batch, which goes into the cover that
// the snapshot-visible view (visible.hip, the _rd entry points) already takes.
//
// A run is one table's range-key fragments as pbl_keyspan_decode with `extra`
// produces them: key = start, value = end, trailer kind in {19, 20, 21}, and per
// KV the keyspan.Key's suffix and value.  It is fragmented as rangedel.hip's
// runs are (span_run.hip.h states that once).
//
//   rangekey_mask_kernel<comparer>  THE HOT PATH, per source KV of a batch: a
//       wave handles 64 consecutive KVs, a lane per KV: one upper-bound search
//       over the set's starts, one compare with the end, one split, one
//       lower-bound search over the span's suffix-ordered keys and one suffix
//       compare.  It has rangedel_cover_kernel's shape: typed global pointers,
//       no LDS, no scratch.  It only ever stores PBL_RANGEDEL_ALL, so a cover
//       from pbl_rangedel_cover composes with it.
//
// The set and its truncation are built by the host forms here (DESIGN.md §9:
// the device builder is not built yet).  They follow the reference's
// sequential shape: sort the boundaries, per elementary interval gather the
// keys, sort them by trailer and run CoalesceInto literally, then walk left to
// right defragmenting (pbl_rangekey_set_host).  pbl_rangekey_mask_host takes
// the RUNS, not the set: per KV it gathers the keys of every fragment that
// covers it and coalesces them, so it checks the set builder (defragmenting
// included) and the lookup together.
#include <algorithm>
#include <vector>

#include "result_core.hip.h"
#include "seek_core.hip.h"
#include "span_run.hip.h"

namespace pbl {
namespace rangekey {

constexpr uint32_t kMaxRuns = PBL_RANGEDEL_MAX_RUNS;
constexpr int kTPB = 256;
constexpr uint64_t kMaxFrags = 0x7fffffffull;
constexpr uint64_t kMaxBytes = 0xffffffffull;
constexpr uint32_t kBadKind = 1, kBadOrder = 2;

using span::is_visible;
using span::Run;
using span::run_of;
using span::upper;

PBL_HD inline uint32_t status_of(uint32_t run_status, uint32_t bad) {
  return run_status != PBL_OK ? run_status : (bad & kBadKind) ? uint32_t(PBL_UNSUPPORTED)
                                           : (bad & kBadOrder) ? uint32_t(PBL_INVALID_ARG) : uint32_t(PBL_OK);
}
PBL_HD inline bool kind_ok(uint64_t trailer) {
  const uint32_t k = uint32_t(trailer & 0xff);
  return k == PBL_KIND_RANGEKEYDEL || k == PBL_KIND_RANGEKEYUNSET || k == PBL_KIND_RANGEKEYSET;
}

// Block b's suffixes and values: suffix j = sb[so[j] .. so[j+1]), likewise values.
template <class R>
struct Extra {
  typename R::template ptr<const uint32_t> so, vo, sp;
  typename R::template ptr<const uint8_t> sb, vb;
  PBL_HD cmp::kptr<R> suffix(uint32_t j, uint64_t* len) const {
    const uint32_t o = so[j];
    *len = uint64_t(so[j + 1]) - o;
    return sb + o;
  }
  PBL_HD cmp::kptr<R> value(uint32_t j, uint64_t* len) const {
    const uint32_t o = vo[j];
    *len = uint64_t(vo[j + 1]) - o;
    return vb + o;
  }
};
template <class R>
PBL_HD inline Extra<R> extra_of(const pbl_keyspan_extra& X, uint64_t kv0, uint32_t b) {
  using P32 = typename R::template ptr<const uint32_t>;
  using P64 = typename R::template ptr<const uint64_t>;
  using P8 = typename R::template ptr<const uint8_t>;
  const P64 bs = (P64)X.blk_suffix_base, bv = (P64)X.blk_value_base;
  return Extra<R>{(P32)X.suffix_off + (kv0 + b), (P32)X.value_off + (kv0 + b), (P32)X.span + kv0,
                  (P8)X.suffix_bytes + bs[b], (P8)X.value_bytes + bv[b]};
}

// ---- the mask -------------------------------------------------------------------
// Whether the span of the set that covers k masks it.  S: the set's block (key =
// start, value = end, one KV per set, a span's KVs in suffix order), X its
// extras (X.sp[kv] = the span's first KV).  t: the threshold suffix.
template <class R>
PBL_HD inline bool masked(uint32_t cmpr, const Run<R>& S, const Extra<R>& X, cmp::kptr<R> k, uint64_t kl,
                          cmp::kptr<R> t, uint64_t tl) {
  const uint64_t sp = cmp::key_split<R>(cmpr, k, kl);
  if (sp >= kl) return false;  // a point without a suffix is never masked
  const uint32_t ub = upper<R>(cmpr, S.S, k, kl);
  if (ub == 0) return false;
  const uint32_t last = ub - 1;  // the last KV of the last span with start <= k
  uint64_t el;
  const cmp::kptr<R> e = S.E.key(last, &el);
  if (cmp::key_cmp<R>(cmpr, k, kl, e, el) >= 0) return false;
  // the span's KVs [first, last], suffixes ascending and distinct: the first
  // with a non-empty suffix that is >= t (the empty suffix sorts first under
  // every comparer, so "empty or < t" holds for a prefix of the span's KVs)
  uint32_t lo = X.sp[last], hi = ub;
  if (lo > last) return false;  // (a foreign array)
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    uint64_t ml;
    const cmp::kptr<R> ms = X.suffix(m, &ml);
    if (ml == 0 || cmp::suffix_cmp<R>(cmpr, ms, ml, t, tl) < 0) lo = m + 1;
    else hi = m;
  }
  if (lo >= ub) return false;
  uint64_t rl;
  const cmp::kptr<R> r = X.suffix(lo, &rl);
  return cmp::suffix_cmp<R>(cmpr, r, rl, k + sp, kl - sp) < 0;
}

using GR = seek::GlobalReader;

struct MaskArgs {
  pbl_decode_out set, batch;
  pbl_keyspan_extra extra;
  uint32_t n_blocks, comparer;
  uint64_t n_kv;
  uint64_t* cover;
  const uint8_t* t;
  uint64_t tl;
};

// Wave per 64 consecutive KVs, lane per KV.
template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void rangekey_mask_kernel(MaskArgs A) {
  pbl_seek_queries sq{};
  const seek::View<GR> V(A.batch, A.n_blocks, sq, nullptr, 0);
  const gptr<const uint32_t> sst = to_glb((const uint32_t*)A.set.blk_status);
  const gptr<const uint64_t> skv = to_glb((const uint64_t*)A.set.blk_kv_base);
  // (a set that overflowed its capacity has sizes and no bytes)
  if (sst[0] != PBL_OK || skv[1] <= skv[0] || skv[1] > A.set.kv_cap) return;
  const Run<GR> S = run_of<GR>(A.set);
  const Extra<GR> X = extra_of<GR>(A.extra, S.S.kv0, 0);
  const gptr<uint64_t> out = to_glb(A.cover);
  const gptr<const uint8_t> t = to_glb(A.t);
  const uint32_t nb = A.n_blocks;
  const uint64_t held = nb ? V.blk_kv_base[nb] : 0;
  const uint64_t lim = A.n_kv < held ? A.n_kv : held;
  const uint64_t n_items = (lim + kWave - 1) / kWave;
  const uint32_t wpb = kTPB / kWave;
  for (uint64_t item = uint64_t(blockIdx.x) * wpb + wave_id(); item < n_items; item += uint64_t(gridDim.x) * wpb) {
    const uint64_t i = item * kWave + lane_id();
    if (i >= lim) continue;
    const uint32_t q = result::block_of(V.blk_kv_base, nb, i);
    if (V.blk_status[q] != PBL_OK) continue;
    const seek::Block<GR> B(V, q);
    if (i < B.kv0 || i - B.kv0 >= B.n) continue;
    uint64_t kl;
    const cmp::kptr<GR> k = B.key(uint32_t(i - B.kv0), &kl);
    if (masked<GR>(kCmp, S, X, k, kl, t, A.tl)) out[i] = PBL_RANGEDEL_ALL;
  }
}

// ---- host side -------------------------------------------------------------------
using HR = cmp::HostReader;

inline bool extra_ok(const pbl_keyspan_extra* x) {
  return x && x->span && x->suffix_off && x->value_off && x->suffix_bytes && x->value_bytes && x->blk_suffix_base &&
         x->blk_value_base;
}
inline bool runs_ok(const pbl_rangekey_runs* in) {
  if (!in || in->n_runs > kMaxRuns || in->comparer > PBL_CMP_CRDB) return false;
  if (in->n_runs && (!in->runs || !in->extras || !in->n_kv)) return false;
  uint64_t t = 0;
  for (uint32_t r = 0; r < in->n_runs; r++) {
    if (!result::source_ok(&in->runs[r]) || !extra_ok(&in->extras[r]) || in->n_kv[r] > kMaxFrags) return false;
    t += in->n_kv[r];
  }
  return t <= kMaxFrags;
}

struct HRun {
  Run<HR> U;
  Extra<HR> X;
  uint32_t r;
};

// The status the set of these (host) runs has, by the sequential checks.
inline uint32_t host_status(const pbl_rangekey_runs* in, std::vector<HRun>* runs) {
  uint32_t st = PBL_OK, bad = 0;
  for (uint32_t r = 0; r < in->n_runs; r++) {
    const uint32_t s = in->runs[r].blk_status[0];
    if (s != PBL_OK) {
      if (st == PBL_OK) st = s;
      continue;
    }
    const Run<HR> U = run_of<HR>(in->runs[r]);
    const uint64_t k0 = in->runs[r].blk_kv_base[0], k1 = in->runs[r].blk_kv_base[1];
    if (k1 < k0 || k1 - k0 != in->n_kv[r] || uint64_t(U.S.n) != in->n_kv[r]) {
      bad |= kBadOrder;
      continue;
    }
    for (uint32_t j = 0; j < U.S.n; j++) {
      if (!kind_ok(U.tr[j]) || (U.fl && (U.fl[j] & PBL_KV_INVALID_KEY))) bad |= kBadKind;
      if (span::unordered_at<HR>(in->comparer, U, j)) bad |= kBadOrder;
    }
    if (runs) runs->push_back(HRun{U, extra_of<HR>(in->extras[r], U.S.kv0, 0), r});
  }
  return status_of(st, bad);
}

struct HKey {  // a keyspan.Key, and where it came from
  uint64_t tr;
  uint32_t run, idx;
  const uint8_t *sfx, *val;
  uint64_t sl, vl;
};
inline HKey key_of(const HRun& H, uint32_t j) {
  HKey k{H.U.tr[j], H.r, j, nullptr, nullptr, 0, 0};
  k.sfx = H.X.suffix(j, &k.sl);
  k.val = H.X.value(j, &k.vl);
  return k;
}

// rangekey.CoalesceInto (coalesce.go:64-151) followed by the user form of
// UserIteratorConfig.Transform (user_iterator.go:163-186): `keys` sorted by
// trailer descending; the surviving sets in suffix order.
inline std::vector<HKey> coalesce(uint32_t cmpr, uint64_t snapshot, const std::vector<HKey>& keys) {
  std::vector<HKey> dst;
  for (const HKey& k : keys) {
    if (!is_visible(k.tr >> 8, snapshot)) continue;
    if ((k.tr & 0xff) == PBL_KIND_RANGEKEYDEL) break;
    dst.push_back(k);
  }
  std::stable_sort(dst.begin(), dst.end(), [cmpr](const HKey& a, const HKey& b) {
    return cmp::suffix_cmp<HR>(cmpr, a.sfx, a.sl, b.sfx, b.sl) < 0;
  });
  std::vector<HKey> out;
  const HKey* prev = nullptr;
  for (const HKey& k : dst) {
    if (prev && cmp::suffix_cmp<HR>(cmpr, prev->sfx, prev->sl, k.sfx, k.sl) == 0) continue;
    prev = &k;
    if ((k.tr & 0xff) == PBL_KIND_RANGEKEYSET) out.push_back(k);
  }
  return out;
}
inline void sort_by_trailer(std::vector<HKey>* keys) {  // keyspan.SortKeysByTrailer; ties by (run, index)
  std::stable_sort(keys->begin(), keys->end(), [](const HKey& a, const HKey& b) { return a.tr > b.tr; });
}
// UserIteratorConfig.ShouldDefragment (user_iterator.go:200-241)
inline bool should_defragment(uint32_t cmpr, const std::vector<HKey>& a, const std::vector<HKey>& b) {
  if (a.size() != b.size() || a.empty()) return false;
  for (size_t i = 0; i < a.size(); i++) {
    if (cmp::suffix_cmp<HR>(cmpr, a[i].sfx, a[i].sl, b[i].sfx, b[i].sl) != 0) return false;
    if (a[i].vl != b[i].vl || (a[i].vl && memcmp(a[i].val, b[i].val, a[i].vl) != 0)) return false;
  }
  return true;
}

struct HBound {
  const uint8_t* k;
  uint64_t kl;
};
struct HSpan {
  HBound s, e;
  std::vector<HKey> keys;
};

// Writes `spans`, block by block (blk_first[b] .. blk_first[b+1]), as a decoded
// batch with extras: one KV per (span, key); sizes only when a capacity is too
// small (PBL_OVERFLOW) or there are no arrays to write.
inline void write_spans(const std::vector<HSpan>& spans, const std::vector<size_t>& blk_first,
                        const std::vector<uint32_t>& blk_status, const pbl_decode_out& O, const pbl_keyspan_extra& X) {
  const uint32_t nb = uint32_t(blk_status.size());
  pbl_totals T{};
  uint64_t kv = 0, kb = 0, vb = 0, sb = 0, xb = 0;
  for (uint32_t b = 0; b < nb; b++) {
    O.blk_kv_base[b] = kv;
    O.blk_key_base[b] = kb;
    O.blk_val_base[b] = vb;
    X.blk_suffix_base[b] = sb;
    X.blk_value_base[b] = xb;
    if (O.blk_rst_base) O.blk_rst_base[b] = 0;
    O.blk_status[b] = blk_status[b];
    if (blk_status[b] != PBL_OK) {
      T.status_mask |= 1u << blk_status[b];
      T.n_bad_blocks++;
    }
    for (size_t s = blk_first[b]; s < blk_first[b + 1]; s++) {
      const uint64_t n = spans[s].keys.size();
      kv += n;
      kb += n * spans[s].s.kl;
      vb += n * spans[s].e.kl;
      for (const HKey& k : spans[s].keys) {
        sb += k.sl;
        xb += k.vl;
      }
    }
  }
  O.blk_kv_base[nb] = kv;
  O.blk_key_base[nb] = kb;
  O.blk_val_base[nb] = vb;
  X.blk_suffix_base[nb] = sb;
  X.blk_value_base[nb] = xb;
  if (O.blk_rst_base) O.blk_rst_base[nb] = 0;
  T.n_kv = kv;
  T.key_bytes = kb;
  T.val_bytes = vb;
  const bool over = kv > O.kv_cap || kb > O.key_cap || vb > O.val_cap || sb > X.suffix_cap || xb > X.value_cap;
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *O.totals = T;
  if (over || !O.key_off) return;
  uint64_t i = 0;
  for (uint32_t b = 0; b < nb; b++) {
    uint32_t ko = 0, vo = 0, so = 0, xo = 0, first = 0, ord = 0;
    uint8_t* const kbytes = O.key_bytes + O.blk_key_base[b];
    uint8_t* const vbytes = O.val_bytes + O.blk_val_base[b];
    uint8_t* const sbytes = X.suffix_bytes + X.blk_suffix_base[b];
    uint8_t* const xbytes = X.value_bytes + X.blk_value_base[b];
    for (size_t s = blk_first[b]; s < blk_first[b + 1]; s++, ord++) {
      for (const HKey& k : spans[s].keys) {
        const uint64_t o = i + b;
        O.trailer[i] = k.tr;
        if (O.kv_flags) O.kv_flags[i] = 0;
        if (O.entry_off) O.entry_off[i] = ord;
        if (O.tiering_span_id) O.tiering_span_id[i] = O.tiering_attr[i] = 0;
        X.span[i] = first;
        O.key_off[o] = ko;
        O.val_off[o] = vo;
        X.suffix_off[o] = so;
        X.value_off[o] = xo;
        if (spans[s].s.kl) memcpy(kbytes + ko, spans[s].s.k, spans[s].s.kl);
        if (spans[s].e.kl) memcpy(vbytes + vo, spans[s].e.k, spans[s].e.kl);
        if (k.sl) memcpy(sbytes + so, k.sfx, k.sl);
        if (k.vl) memcpy(xbytes + xo, k.val, k.vl);
        ko += uint32_t(spans[s].s.kl);
        vo += uint32_t(spans[s].e.kl);
        so += uint32_t(k.sl);
        xo += uint32_t(k.vl);
        i++;
      }
      first += uint32_t(spans[s].keys.size());
    }
    const uint64_t o = i + b;
    O.key_off[o] = ko;
    O.val_off[o] = vo;
    X.suffix_off[o] = so;
    X.value_off[o] = xo;
  }
}

inline bool out_ok(const pbl_decode_out* o, const pbl_keyspan_extra* x) {
  if (!o || !x || !result::result_ok(*o, false) || !x->blk_suffix_base || !x->blk_value_base) return false;
  if (o->key_off && !(x->span && x->suffix_off && x->value_off && x->suffix_bytes && x->value_bytes)) return false;
  return true;
}

// The spans of block b of a set (host arrays), whole.
inline std::vector<HSpan> spans_of(const pbl_decode_out& D, const pbl_keyspan_extra& X, uint32_t b, uint32_t nb) {
  const Run<HR> U = run_of<HR>(D, b, nb);
  const Extra<HR> E = extra_of<HR>(X, U.S.kv0, b);
  std::vector<HSpan> spans;
  for (uint32_t j = 0; j < U.S.n; j++) {
    if (j == 0 || E.sp[j] == j) {
      HSpan s;
      s.s.k = U.S.key(j, &s.s.kl);
      s.e.k = U.E.key(j, &s.e.kl);
      spans.push_back(s);
    }
    HKey k{U.tr[j], 0, j, nullptr, nullptr, 0, 0};
    k.sfx = E.suffix(j, &k.sl);
    k.val = E.value(j, &k.vl);
    spans.back().keys.push_back(k);
  }
  return spans;
}

}  // namespace rangekey
}  // namespace pbl

extern "C" {

int pbl_range_suffix_compare(uint32_t comparer, const uint8_t* a, uint64_t a_len, const uint8_t* b, uint64_t b_len) {
  return pbl::cmp::suffix_cmp<pbl::cmp::HostReader>(comparer, a, a_len, b, b_len);
}

int pbl_rangekey_set_host(const pbl_rangekey_runs* in, pbl_decode_out* set, pbl_keyspan_extra* set_extra) {
  namespace M = pbl::rangekey;
  using R = pbl::cmp::HostReader;
  if (!M::runs_ok(in) || !M::out_ok(set, set_extra)) return PBL_INVALID_ARG;
  std::vector<M::HRun> runs;
  uint32_t status = M::host_status(in, &runs);
  const uint32_t c = in->comparer;
  std::vector<M::HBound> bs;
  std::vector<M::HSpan> spans;
  if (status == PBL_OK) {
    // every boundary in (run, fragment index, start before end) order
    for (const M::HRun& H : runs)
      for (uint32_t j = 0; j < H.U.S.n; j++) {
        M::HBound s, e;
        s.k = H.U.S.key(j, &s.kl);
        e.k = H.U.E.key(j, &e.kl);
        bs.push_back(s);
        bs.push_back(e);
      }
    std::stable_sort(bs.begin(), bs.end(), [c](const M::HBound& a, const M::HBound& b) {
      return pbl::cmp::key_cmp<R>(c, a.k, a.kl, b.k, b.kl) < 0;
    });
    bs.erase(std::unique(bs.begin(), bs.end(),
                         [c](const M::HBound& a, const M::HBound& b) {
                           return pbl::cmp::key_cmp<R>(c, a.k, a.kl, b.k, b.kl) == 0;
                         }),
             bs.end());
    // keyspanimpl.MergingIter: per elementary interval the keys of every fragment
    // that contains it, by trailer descending; Transform; DefragmentingIter's
    // forward walk keeps the leftmost fragment's keys
    bool open = false;  // the last span ends at this interval's start
    std::vector<uint32_t> cur(runs.size(), 0);  // per run, the first fragment that ends after this interval's start
    for (size_t i = 0; i + 1 < bs.size(); i++) {
      std::vector<M::HKey> keys;
      for (size_t r = 0; r < runs.size(); r++) {
        // the merging iterator's walk: a fragmented run covers the interval with at
        // most one group of fragments that share their bounds
        const M::HRun& H = runs[r];
        uint64_t sl, el, s2l;
        while (cur[r] < H.U.S.n) {
          const uint8_t* e = H.U.E.key(cur[r], &el);
          if (pbl::cmp::key_cmp<R>(c, e, el, bs[i].k, bs[i].kl) > 0) break;
          cur[r]++;
        }
        if (cur[r] >= H.U.S.n) continue;
        const uint8_t* s = H.U.S.key(cur[r], &sl);
        if (pbl::cmp::key_cmp<R>(c, s, sl, bs[i].k, bs[i].kl) > 0) continue;
        for (uint32_t j = cur[r]; j < H.U.S.n; j++) {
          const uint8_t* s2 = H.U.S.key(j, &s2l);
          if (pbl::cmp::key_cmp<R>(c, s, sl, s2, s2l) != 0) break;
          keys.push_back(M::key_of(H, j));
        }
      }
      M::sort_by_trailer(&keys);
      std::vector<M::HKey> sets = M::coalesce(c, in->snapshot, keys);
      if (sets.empty()) {
        open = false;
        continue;
      }
      if (open && M::should_defragment(c, spans.back().keys, sets)) {
        spans.back().e = bs[i + 1];
      } else {
        spans.push_back(M::HSpan{bs[i], bs[i + 1], std::move(sets)});
      }
      open = true;
    }
    uint64_t kb = 0, vb = 0, sb = 0, xb = 0;
    for (const M::HSpan& s : spans) {
      kb += s.keys.size() * s.s.kl;
      vb += s.keys.size() * s.e.kl;
      for (const M::HKey& k : s.keys) sb += k.sl, xb += k.vl;
    }
    if (kb > M::kMaxBytes || vb > M::kMaxBytes || sb > M::kMaxBytes || xb > M::kMaxBytes) {
      status = PBL_UNSUPPORTED;
      spans.clear();
    }
  }
  M::write_spans(spans, {0, spans.size()}, {status}, *set, *set_extra);
  return PBL_OK;
}

int pbl_rangekey_clip_host(const pbl_decode_out* set, const pbl_keyspan_extra* set_extra, const pbl_scan_queries* ranges,
                           pbl_decode_out* out, pbl_keyspan_extra* out_extra) {
  namespace M = pbl::rangekey;
  using R = pbl::cmp::HostReader;
  if (!pbl::result::source_ok(set) || !M::extra_ok(set_extra) || !ranges || ranges->comparer > PBL_CMP_CRDB ||
      !M::out_ok(out, out_extra))
    return PBL_INVALID_ARG;
  const uint32_t n = ranges->n, c = ranges->comparer;
  if (n && (!ranges->lower_off || !ranges->upper_off || !ranges->lower_bytes || !ranges->upper_bytes)) return PBL_INVALID_ARG;
  const uint32_t st = set->blk_status[0];
  std::vector<M::HSpan> all, spans;
  if (st == PBL_OK && set->blk_kv_base[1] <= set->kv_cap) all = M::spans_of(*set, *set_extra, 0, 1);
  std::vector<size_t> first{0};
  std::vector<uint32_t> status;
  for (uint32_t q = 0; q < n; q++) {
    const M::HBound lo{ranges->lower_bytes + ranges->lower_off[q], ranges->lower_off[q + 1] - ranges->lower_off[q]};
    const M::HBound hi{ranges->upper_bytes + ranges->upper_off[q], ranges->upper_off[q + 1] - ranges->upper_off[q]};
    const bool no_upper = ranges->flags && (ranges->flags[q] & PBL_SCAN_NO_UPPER);
    for (const M::HSpan& s : all) {
      // BoundedIter keeps the spans that intersect [lower, upper); the
      // interleaving iterator truncates them to it
      if (pbl::cmp::key_cmp<R>(c, s.e.k, s.e.kl, lo.k, lo.kl) <= 0) continue;
      if (!no_upper && pbl::cmp::key_cmp<R>(c, s.s.k, s.s.kl, hi.k, hi.kl) >= 0) continue;
      M::HSpan t = s;
      if (pbl::cmp::key_cmp<R>(c, t.s.k, t.s.kl, lo.k, lo.kl) < 0) t.s = lo;
      if (!no_upper && pbl::cmp::key_cmp<R>(c, hi.k, hi.kl, t.e.k, t.e.kl) < 0) t.e = hi;
      // an empty or inverted range (upper <= lower) intersects nothing: no empty or inverted span
      if (pbl::cmp::key_cmp<R>(c, t.s.k, t.s.kl, t.e.k, t.e.kl) >= 0) continue;
      spans.push_back(std::move(t));
    }
    first.push_back(spans.size());
    status.push_back(st);
  }
  M::write_spans(spans, first, status, *out, *out_extra);
  return PBL_OK;
}

int pbl_rangekey_mask(const pbl_decode_out* set, const pbl_keyspan_extra* set_extra, const pbl_decode_out* batch,
                      uint32_t n_blocks, uint64_t n_kv, uint32_t comparer, const uint8_t* mask_suffix,
                      uint64_t mask_suffix_len, uint64_t* cover_seq, void* stream) {
  namespace M = pbl::rangekey;
  using namespace pbl;
  if (!set || !set_extra || !batch || !cover_seq || comparer > PBL_CMP_CRDB || (!mask_suffix && mask_suffix_len))
    return PBL_INVALID_ARG;
  if (!set->blk_status || !set->blk_kv_base || !set->blk_key_base || !set->blk_val_base || !set->key_off ||
      !set->val_off || !set->key_bytes || !set->val_bytes || !set->trailer || !M::extra_ok(set_extra))
    return PBL_INVALID_ARG;
  if (!batch->blk_status || !batch->blk_kv_base || !batch->blk_key_base || !batch->key_off || !batch->key_bytes)
    return PBL_INVALID_ARG;
  if (n_kv == 0) return PBL_OK;
  M::MaskArgs a{*set, *batch, *set_extra, n_blocks, comparer, n_kv, cover_seq, mask_suffix, mask_suffix_len};
  const uint64_t waves = (n_kv + kWave - 1) / kWave, wpb = M::kTPB / kWave;
  const uint32_t grid = uint32_t(std::min<uint64_t>((waves + wpb - 1) / wpb, 1u << 16));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  seek::with_cmp(comparer, [&](auto c) {
    hipLaunchKernelGGL(M::rangekey_mask_kernel<decltype(c)::value>, dim3(grid), dim3(M::kTPB), 0, st, a);
    return 0;
  });
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_rangekey_mask_set_host(const pbl_decode_out* set, const pbl_keyspan_extra* set_extra, const pbl_decode_out* batch,
                               uint32_t n_blocks, uint32_t comparer, const uint8_t* mask_suffix,
                               uint64_t mask_suffix_len, uint64_t* cover_seq) {
  namespace M = pbl::rangekey;
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!pbl::result::source_ok(set) || !M::extra_ok(set_extra) || !batch || !cover_seq || comparer > PBL_CMP_CRDB ||
      (!mask_suffix && mask_suffix_len))
    return PBL_INVALID_ARG;
  if (!batch->blk_status || !batch->blk_kv_base || !batch->blk_key_base || !batch->key_off || !batch->key_bytes)
    return PBL_INVALID_ARG;
  if (set->blk_status[0] != PBL_OK || set->blk_kv_base[1] <= set->blk_kv_base[0] || set->blk_kv_base[1] > set->kv_cap)
    return PBL_OK;
  const M::Run<R> S = M::run_of<R>(*set);
  const M::Extra<R> X = M::extra_of<R>(*set_extra, S.S.kv0, 0);
  pbl_seek_queries sq{};
  const K::View<R> V(*batch, n_blocks, sq, nullptr, 0);
  for (uint32_t q = 0; q < n_blocks; q++) {
    if (batch->blk_status[q] != PBL_OK) continue;
    const K::Block<R> B(V, q);
    for (uint32_t x = 0; x < B.n; x++) {
      uint64_t kl;
      const uint8_t* k = B.key(x, &kl);
      if (M::masked<R>(comparer, S, X, k, kl, mask_suffix, mask_suffix_len)) cover_seq[B.kv0 + x] = PBL_RANGEDEL_ALL;
    }
  }
  return PBL_OK;
}

int pbl_rangekey_mask_host(const pbl_rangekey_runs* in, const pbl_decode_out* batch, uint32_t n_blocks,
                           const uint8_t* mask_suffix, uint64_t mask_suffix_len, uint64_t* cover_seq,
                           uint32_t* status) {
  namespace M = pbl::rangekey;
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!M::runs_ok(in) || !batch || !cover_seq || (!mask_suffix && mask_suffix_len)) return PBL_INVALID_ARG;
  if (!batch->blk_status || !batch->blk_kv_base || !batch->blk_key_base || !batch->key_off || !batch->key_bytes)
    return PBL_INVALID_ARG;
  std::vector<M::HRun> runs;
  const uint32_t st = M::host_status(in, &runs);
  if (status) *status = st;
  if (st != PBL_OK) return PBL_OK;
  const uint32_t c = in->comparer;
  pbl_seek_queries sq{};
  const K::View<R> V(*batch, n_blocks, sq, nullptr, 0);
  for (uint32_t q = 0; q < n_blocks; q++) {
    if (batch->blk_status[q] != PBL_OK) continue;
    const K::Block<R> B(V, q);
    for (uint32_t x = 0; x < B.n; x++) {
      uint64_t kl;
      const uint8_t* k = B.key(x, &kl);
      const uint64_t sp = pbl::cmp::key_split<R>(c, k, kl);
      if (sp >= kl) continue;
      // every key of every fragment that covers k, coalesced
      std::vector<M::HKey> keys;
      for (const M::HRun& H : runs)
        for (uint32_t j = 0; j < H.U.S.n; j++) {
          uint64_t sl, el;
          const uint8_t *s = H.U.S.key(j, &sl), *e = H.U.E.key(j, &el);
          if (pbl::cmp::key_cmp<R>(c, s, sl, k, kl) <= 0 && pbl::cmp::key_cmp<R>(c, k, kl, e, el) < 0)
            keys.push_back(M::key_of(H, j));
        }
      M::sort_by_trailer(&keys);
      // rangeKeyMasking.SpanChanged: the smallest suffix that is not below the threshold
      const M::HKey* act = nullptr;
      const std::vector<M::HKey> sets = M::coalesce(c, in->snapshot, keys);
      for (const M::HKey& s : sets) {
        if (s.sl == 0 || pbl::cmp::suffix_cmp<R>(c, s.sfx, s.sl, mask_suffix, mask_suffix_len) < 0) continue;
        if (!act || pbl::cmp::suffix_cmp<R>(c, act->sfx, act->sl, s.sfx, s.sl) > 0) act = &s;
      }
      // SkipPoint
      if (act && pbl::cmp::suffix_cmp<R>(c, act->sfx, act->sl, k + sp, kl - sp) < 0)
        cover_seq[B.kv0 + x] = PBL_RANGEDEL_ALL;
    }
  }
  return PBL_OK;
}

size_t pbl_rangekey_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {sizeof(pbl_rangekey_runs),          PBL_OFF(pbl_rangekey_runs, runs),
                        PBL_OFF(pbl_rangekey_runs, extras), PBL_OFF(pbl_rangekey_runs, n_kv),
                        PBL_OFF(pbl_rangekey_runs, n_runs), PBL_OFF(pbl_rangekey_runs, comparer),
                        PBL_OFF(pbl_rangekey_runs, snapshot)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
