// rangedel.hip — range deletions in the device read path (DESIGN.md §3.14;
// include/pebble_amd.h states the rules): the flattened set of up to 16 runs of
// range-deletion fragments, and the cover of every KV of a decoded batch, which
// the snapshot-visible view (visible.hip, the _rd entry points) takes as one
// more invisible predicate per KV.
//
// A run is one table's fragments as a decoded batch with one block (key = start,
// trailer = seq << 8 | 15, value = end).  A run's starts are sorted and, because
// it is fragmented, so are its ends: 2K sorted lists of boundary keys.  T, the
// fragments of all runs, is small next to a batch's KV count, so the set builder
// is kept simple and every lane's work is bounded (searches only, no walks).
//
//   rangedel_validate_kernel<comparer>  lane per fragment against its successor
//       (as merge_validate_kernel): kind, start <= end, order, fragmentation; one
//       thread reads the runs' block statuses and KV counts
//   rangedel_rank_kernel<comparer>  lane per boundary (2T of them): its place is
//       the sum over the 2K lists of the boundaries that go before it (sk::lower
//       in the lists after its own, the upper bound in the lists before it; ties
//       by list and index): the merge's rank stage in small
//   rangedel_place_kernel<comparer>  workgroup per tile of 256 sorted places: a
//       head flag (the key differs from its predecessor's), the cover (per run:
//       the last fragment with start <= b, then b < end, then the first of its
//       equal-start fragments that is visible), the tile's heads and key bytes
//   rangedel_bases_kernel  one workgroup: the status, the scan over the tile sums
//       (result::tile_scan_inplace), the result's bases, totals and capacity
//       check (result::bases)
//   rangedel_emit_kernel  workgroup per tile: a head's place from the in-tile
//       scan; trailer, offsets and key bytes; the last offsets
//       (result::last_offsets)
//   rangedel_cover_kernel<comparer>  THE HOT PATH, per source KV of a batch: a
//       wave handles 64 consecutive KVs, a lane per KV: one upper-bound search
//       over the set's one block.  Neighbouring lanes hold neighbouring keys and
//       walk the same boundaries.  Typed global pointers, no LDS, no scratch.
//
// Levels (optional; include/pebble_amd.h "Levels"): with a level per run the
// place stage also keeps, per boundary, the shallowest level that holds a visible
// covering fragment (the set's entry_off), and the cover kernel, given per KV the
// run it came from and that run's level, answers PBL_RANGEDEL_ALL where that
// level is shallower than the KV's: the reference's level-by-level rule.
//
// The host forms use other algorithms on purpose: a stable sort plus unique
// over all boundaries and a brute-force maximum per boundary
// (pbl_rangedel_set_host); a brute-force maximum over every fragment of the
// RUNS per KV (pbl_rangedel_cover_host).
#include <algorithm>
#include <vector>

#include "result_core.hip.h"
#include "seek_core.hip.h"
#include "span_run.hip.h"

namespace pbl {
namespace rangedel {

constexpr uint64_t kHdr = 64;
constexpr uint32_t kMaxRuns = PBL_RANGEDEL_MAX_RUNS;
constexpr int kTPB = 256;
constexpr uint32_t kTileShift = 8;
static_assert(kTPB == result::kTPB && (1u << kTileShift) == uint32_t(kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kGrid = 2048;                 // workgroups of a grid-striding kernel, at most
constexpr uint64_t kMaxFrags = 0x7fffffffull;    // 2T boundaries are indexed by u32
constexpr uint64_t kMaxBytes = 0xffffffffull;
enum { kHSkip = 0, kHRunStatus = 1, kHBad = 2 };  // header words: sizes only; first run status; flag bits
constexpr uint32_t kBadKind = 1, kBadOrder = 2;
// A boundary's workspace word: the cover in the low 56 bits, above it 1 + the
// shallowest level that holds a visible covering fragment (0: none, or no levels).
constexpr int kLvShift = 56;
constexpr uint64_t kSeqMask = (1ull << kLvShift) - 1;

using span::is_visible;
using span::Run;
using span::run_of;
using span::upper;
PBL_HD inline uint32_t status_of(uint32_t run_status, uint32_t bad) {
  return run_status != PBL_OK ? run_status : (bad & kBadKind) ? uint32_t(PBL_UNSUPPORTED)
                                           : (bad & kBadOrder) ? uint32_t(PBL_INVALID_ARG) : uint32_t(PBL_OK);
}

struct Layout {
  uint64_t n_items, nt;  // boundaries (2T); tiles of 256 of them (at least one)
  uint64_t q64, csum, qst, tsum, cover, perm, hk, size;
};
__host__ __device__ inline Layout layout(uint64_t n_frag) {
  Layout L;
  L.n_items = 2 * n_frag;
  L.nt = L.n_items ? (L.n_items + kTPB - 1) >> kTileShift : 1;
  uint64_t o = kHdr;
  L.q64 = o;   o += 3ull * 8 * 2;
  L.csum = o;  o += 3ull * 8;
  L.qst = o;   o += 8;
  L.tsum = o;  o += 2ull * 8 * (L.nt + 1);  // heads, key bytes; entry nt: the totals
  L.cover = o; o += 8ull * L.n_items;
  L.perm = o;  o += 4ull * L.n_items;
  L.hk = o;    o += 4ull * L.n_items;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

// Fragment j of a run against itself and its successor: kBad* bits.
template <class R>
PBL_HD inline uint32_t check_fragment(uint32_t cmpr, const Run<R>& U, uint32_t j) {
  uint32_t bad = 0;
  if ((U.tr[j] & 0xff) != PBL_KIND_RANGEDEL || (U.fl && (U.fl[j] & PBL_KV_INVALID_KEY))) bad |= kBadKind;
  if (span::unordered_at<R>(cmpr, U, j)) bad |= kBadOrder;
  return bad;
}

// The largest visible sequence number among the run's fragments that cover b
// (start <= b < end), 0 when there is none.  Three searches, no walk.
template <class R>
PBL_HD inline uint64_t run_cover(uint32_t cmpr, const Run<R>& U, cmp::kptr<R> b, uint64_t bl, uint64_t snapshot) {
  const uint32_t ub = upper<R>(cmpr, U.S, b, bl);
  if (ub == 0) return 0;
  const uint32_t last = ub - 1;  // the last fragment with start <= b
  uint64_t el, sl;
  const cmp::kptr<R> e = U.E.key(last, &el);
  if (cmp::key_cmp<R>(cmpr, b, bl, e, el) >= 0) return 0;
  // its equal-start fragments [g0, last], trailers descending: the first visible one
  const cmp::kptr<R> s = U.S.key(last, &sl);
  uint32_t lo = seek::lower<R>(cmpr, U.S, s, sl), hi = ub;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (!is_visible(U.tr[m] >> 8, snapshot)) lo = m + 1;
    else hi = m;
  }
  return lo < ub ? U.tr[lo] >> 8 : 0;
}

// ---- device side ---------------------------------------------------------------
struct Args {
  pbl_decode_out run[kMaxRuns];
  pbl_decode_out out;
  uint64_t base[kMaxRuns + 1];  // fragments before run r; [n_runs] = T
  uint64_t snapshot;
  uint32_t n_runs, comparer;
  uint8_t* ws;
  uint8_t level[kMaxRuns];  // the runs' levels (smaller = shallower)
  uint32_t has_level;
};

struct Ws {
  gptr<uint32_t> hdr, qst, perm, hk;
  gptr<uint64_t> q64, csum, tsum[2], cover;
  uint64_t n_items, nt;
  __device__ Ws(uint8_t* ws, uint64_t n_frag) {
    const Layout L = layout(n_frag);
    hdr = to_glb(reinterpret_cast<uint32_t*>(ws));
    q64 = to_glb(reinterpret_cast<uint64_t*>(ws + L.q64));
    csum = to_glb(reinterpret_cast<uint64_t*>(ws + L.csum));
    qst = to_glb(reinterpret_cast<uint32_t*>(ws + L.qst));
    tsum[0] = to_glb(reinterpret_cast<uint64_t*>(ws + L.tsum));
    tsum[1] = tsum[0] + (L.nt + 1);
    cover = to_glb(reinterpret_cast<uint64_t*>(ws + L.cover));
    perm = to_glb(reinterpret_cast<uint32_t*>(ws + L.perm));
    hk = to_glb(reinterpret_cast<uint32_t*>(ws + L.hk));
    n_items = L.n_items;
    nt = L.nt;
  }
  __device__ result::Sizes sizes() const { return result::Sizes{q64, csum, qst, 2, 1}; }
  __device__ uint32_t status() const { return status_of(hdr[kHRunStatus], hdr[kHBad]); }
};

using GR = seek::GlobalReader;
using result::block_excl_scan64;
using result::block_sum64;

// Boundary e = 2 * (flat fragment) + side (0 start, 1 end): its run, fragment and side.
struct Item {
  uint32_t r, j, side;
};
__device__ inline Item item_of(const Args& A, uint64_t e) {
  const uint64_t f = e >> 1;
  uint32_t r = 0;
  for (uint32_t x = 1; x < A.n_runs; x++)
    if (A.base[x] <= f) r = x;
  return Item{r, uint32_t(f - A.base[r]), uint32_t(e & 1)};
}
__device__ inline cmp::kptr<GR> item_key(const Run<GR>& U, const Item& I, uint64_t* len) {
  return I.side ? U.E.key(I.j, len) : U.S.key(I.j, len);
}

template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void rangedel_validate_kernel(Args A) {
  const uint64_t T = A.base[A.n_runs];
  const Ws W(A.ws, T);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the first run status that is not PBL_OK; a run that holds another number of KVs than announced
    uint32_t st = PBL_OK, bad = 0;
    for (uint32_t r = 0; r < A.n_runs; r++) {
      const uint32_t s = to_glb(A.run[r].blk_status)[0];
      if (s != PBL_OK) {
        if (st == PBL_OK) st = s;
        continue;
      }
      const uint64_t k0 = to_glb(A.run[r].blk_kv_base)[0], k1 = to_glb(A.run[r].blk_kv_base)[1];
      if (k1 < k0 || k1 - k0 != A.base[r + 1] - A.base[r]) bad |= kBadOrder;
    }
    W.hdr[kHRunStatus] = st;
    if (bad) g_atomic_or((uint32_t*)(W.hdr + kHBad), bad);
  }
  for (uint64_t f = uint64_t(blockIdx.x) * kTPB + threadIdx.x; f < T; f += uint64_t(gridDim.x) * kTPB) {
    const Item I = item_of(A, 2 * f);
    if (to_glb(A.run[I.r].blk_status)[0] != PBL_OK) continue;
    const Run<GR> U = run_of<GR>(A.run[I.r]);
    if (uint64_t(U.S.n) != A.base[I.r + 1] - A.base[I.r] || I.j >= U.S.n) continue;  // (flagged above)
    const uint32_t bad = check_fragment<GR>(kCmp, U, I.j);
    if (bad) g_atomic_or((uint32_t*)(W.hdr + kHBad), bad);
  }
}

__device__ inline uint32_t clamp(uint32_t x, uint32_t lo, uint32_t hi) { return x < lo ? lo : x > hi ? hi : x; }

// perm[place] = boundary.  The workspace was filled with 0xff: a place nobody
// ranks (which a validated input does not leave) names no boundary.
template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void rangedel_rank_kernel(Args A) {
  const uint64_t T = A.base[A.n_runs];
  const Ws W(A.ws, T);
  if (W.status() != PBL_OK) return;
  for (uint64_t e = uint64_t(blockIdx.x) * kTPB + threadIdx.x; e < W.n_items; e += uint64_t(gridDim.x) * kTPB) {
    const Item I = item_of(A, e);
    const Run<GR> own = run_of<GR>(A.run[I.r]);
    uint64_t bl;
    const cmp::kptr<GR> b = item_key(own, I, &bl);
    uint64_t rank = 0;
    for (uint32_t r = 0; r < A.n_runs; r++) {
      const Run<GR> U = r == I.r ? own : run_of<GR>(A.run[r]);
      if (r < I.r) {  // equal keys of an earlier list go first
        rank += upper<GR>(kCmp, U.S, b, bl) + upper<GR>(kCmp, U.E, b, bl);
      } else if (r > I.r) {
        rank += seek::lower<GR>(kCmp, U.S, b, bl) + seek::lower<GR>(kCmp, U.E, b, bl);
      } else {
        // its own run: of the equal keys, the starts of fragments <= j (< j for a
        // start) and the ends of fragments < j go first
        const uint32_t ls = seek::lower<GR>(kCmp, U.S, b, bl), us = upper<GR>(kCmp, U.S, b, bl);
        const uint32_t le = seek::lower<GR>(kCmp, U.E, b, bl), ue = upper<GR>(kCmp, U.E, b, bl);
        const uint32_t lim_s = I.side ? I.j + 1 : I.j, lim_e = I.j;
        rank += clamp(lim_s, ls, us) + clamp(lim_e, le, ue);
      }
    }
    if (rank < W.n_items) W.perm[rank] = uint32_t(e);
  }
}

template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void rangedel_place_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const uint64_t T = A.base[A.n_runs];
  const Ws W(A.ws, T);
  if (W.status() != PBL_OK) return;
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t p = (t << kTileShift) + threadIdx.x;
    uint64_t head = 0, kbytes = 0;
    if (p < W.n_items) {
      const uint32_t e = W.perm[p];
      uint32_t hk = 0;
      uint64_t cover = 0;
      if (e < W.n_items) {
        const Item I = item_of(A, e);
        const Run<GR> own = run_of<GR>(A.run[I.r]);
        uint64_t bl;
        const cmp::kptr<GR> b = item_key(own, I, &bl);
        bool first = p == 0;
        if (!first) {
          const uint32_t e0 = W.perm[p - 1];
          first = e0 >= W.n_items;
          if (!first) {
            const Item I0 = item_of(A, e0);
            const Run<GR> U0 = run_of<GR>(A.run[I0.r]);
            uint64_t al;
            const cmp::kptr<GR> a = item_key(U0, I0, &al);
            first = cmp::key_cmp<GR>(kCmp, a, al, b, bl) != 0;
          }
        }
        if (first) {
          uint32_t lv = 0;  // 1 + the shallowest covering level
          for (uint32_t r = 0; r < A.n_runs; r++) {
            const uint64_t c = run_cover<GR>(kCmp, r == I.r ? own : run_of<GR>(A.run[r]), b, bl, A.snapshot);
            cover = c > cover ? c : cover;
            if (c && A.has_level && (lv == 0 || uint32_t(A.level[r]) + 1 < lv)) lv = uint32_t(A.level[r]) + 1;
          }
          cover = (cover & kSeqMask) | uint64_t(lv) << kLvShift;
          hk = uint32_t(bl) + 1;
          head = 1;
          kbytes = bl;
        }
      }
      W.hk[p] = hk;
      W.cover[p] = cover;
    }
    const uint64_t hs = block_sum64(head, lds), ks = block_sum64(kbytes, lds);
    if (threadIdx.x == 0) {
      W.tsum[0][t] = hs;
      W.tsum[1][t] = ks;
    }
  }
}

// One workgroup.  Totals were zeroed by the entry point.
__global__ __launch_bounds__(kTPB) void rangedel_bases_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const uint64_t T = A.base[A.n_runs];
  const Ws W(A.ws, T);
  uint32_t st = W.status();
  uint64_t n = 0, k = 0;
  if (st == PBL_OK) {
    if (threadIdx.x == 0) W.tsum[0][W.nt] = W.tsum[1][W.nt] = 0;
    __syncthreads();
    const gptr<uint64_t> a[2] = {W.tsum[0], W.tsum[1]};
    result::tile_scan_inplace<2>(a, W.nt + 1, lds);
    __syncthreads();
    n = W.tsum[0][W.nt];
    k = W.tsum[1][W.nt];
    if (k > kMaxBytes) st = PBL_UNSUPPORTED;
  }
  if (threadIdx.x == 0) {
    const bool some = st == PBL_OK;
    W.q64[0] = some ? n : 0;
    W.q64[2] = some ? k : 0;
    W.q64[4] = 0;
    W.qst[0] = st;
  }
  __syncthreads();
  uint64_t ex[3], end[3];
  bool over;
  if (result::bases<3>(W.sizes(), A.out, 1, false, lds, ex, end, &over))
    W.hdr[kHSkip] = (over || !A.out.key_off) ? 1u : 0u;
}

__global__ __launch_bounds__(kTPB) void rangedel_emit_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const uint64_t T = A.base[A.n_runs];
  const Ws W(A.ws, T);
  if (W.hdr[kHSkip] != 0) return;  // sizes only
  const pbl_decode_out& O = A.out;
  result::last_offsets(O, 1, O.kv_cap);
  const uint64_t n_out = to_glb(O.blk_kv_base)[1], k_out = to_glb(O.blk_key_base)[1];
  if (W.qst[0] != PBL_OK) return;  // (an empty set: its one offset is written)
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t p = (t << kTileShift) + threadIdx.x;
    const uint32_t hk = p < W.n_items ? W.hk[p] : 0u;
    const uint32_t e = p < W.n_items ? W.perm[p] : 0xffffffffu;
    const bool head = hk != 0 && e < W.n_items;
    const uint64_t klen = head ? hk - 1 : 0;
    uint64_t tot;
    const uint64_t i = W.tsum[0][t] + block_excl_scan64(head ? 1 : 0, lds, &tot);
    const uint64_t ko = W.tsum[1][t] + block_excl_scan64(klen, lds, &tot);
    if (!head || i >= n_out || i >= O.kv_cap || ko + klen > k_out || ko + klen > O.key_cap) continue;
    to_glb(O.trailer)[i] = ((W.cover[p] & kSeqMask) << 8) | PBL_KIND_RANGEDEL;
    if (O.kv_flags) to_glb(O.kv_flags)[i] = 0;
    if (O.entry_off) to_glb(O.entry_off)[i] = uint32_t(W.cover[p] >> kLvShift);
    if (O.tiering_span_id) {
      to_glb(O.tiering_span_id)[i] = 0;
      to_glb(O.tiering_attr)[i] = 0;
    }
    to_glb(O.key_off)[i] = uint32_t(ko);
    to_glb(O.val_off)[i] = 0;
    const Item I = item_of(A, e);
    const Run<GR> U = run_of<GR>(A.run[I.r]);
    uint64_t bl;
    const cmp::kptr<GR> b = item_key(U, I, &bl);
    if (bl == klen) copy_chunks(to_glb(O.key_bytes) + ko, b, uint32_t(klen));
  }
}

struct CoverArgs {
  pbl_decode_out set, batch;
  uint32_t n_blocks, comparer;
  uint64_t n_kv;
  uint64_t* cover;
  const uint8_t* src_run;       // per KV the run (table) it came from, or NULL: no levels
  uint8_t run_level[kMaxRuns];  // that run's level
};

// Wave per 64 consecutive KVs, lane per KV: one upper-bound search over the set.
template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void rangedel_cover_kernel(CoverArgs A) {
  pbl_seek_queries sq{};
  const seek::View<GR> VS(A.set, 1, sq, nullptr, 0), V(A.batch, A.n_blocks, sq, nullptr, 0);
  const seek::Block<GR> SB(VS, 0);
  // (a set that overflowed its capacity has sizes and no bytes)
  const bool set_ok = VS.blk_status[0] == PBL_OK && SB.n > 0 && SB.kv0 + SB.n <= A.set.kv_cap;
  const gptr<const uint64_t> str = to_glb((const uint64_t*)A.set.trailer) + SB.kv0;
  const gptr<uint64_t> out = to_glb(A.cover);
  // levels: the set's entry_off holds 1 + the shallowest covering level per boundary
  const bool leveled = A.src_run != nullptr && A.set.entry_off != nullptr;
  const gptr<const uint32_t> slv = to_glb((const uint32_t*)A.set.entry_off) + SB.kv0;
  const gptr<const uint8_t> srun = to_glb(A.src_run);
  const uint32_t nb = A.n_blocks;
  const uint64_t held = nb ? V.blk_kv_base[nb] : 0;
  const uint64_t n_items = (A.n_kv + kWave - 1) / kWave;
  const uint32_t wpb = kTPB / kWave;
  for (uint64_t item = uint64_t(blockIdx.x) * wpb + wave_id(); item < n_items; item += uint64_t(gridDim.x) * wpb) {
    const uint64_t i = item * kWave + lane_id();
    if (i >= A.n_kv) continue;
    uint64_t c = 0;
    if (set_ok && i < held) {
      const uint32_t q = result::block_of(V.blk_kv_base, nb, i);
      if (V.blk_status[q] == PBL_OK) {
        const seek::Block<GR> B(V, q);
        if (i >= B.kv0 && i - B.kv0 < B.n) {
          uint64_t kl;
          const cmp::kptr<GR> k = B.key(uint32_t(i - B.kv0), &kl);
          const uint32_t ub = upper<GR>(kCmp, SB, k, kl);
          if (ub) {
            c = str[ub - 1] >> 8;
            if (leveled) {
              const uint32_t lv = slv[ub - 1], r = srun[i];
              if (lv && r < kMaxRuns && lv - 1 < uint32_t(A.run_level[r])) c = PBL_RANGEDEL_ALL;
            }
          }
        }
      }
    }
    out[i] = c;
  }
}

// ---- host side -----------------------------------------------------------------
inline bool runs_ok(const pbl_rangedel_runs* in) {
  if (!in || in->n_runs > kMaxRuns || in->comparer > PBL_CMP_CRDB) return false;
  if (in->n_runs && (!in->runs || !in->n_kv)) return false;
  uint64_t t = 0;
  for (uint32_t r = 0; r < in->n_runs; r++) {
    if (!result::source_ok(&in->runs[r]) || in->n_kv[r] > kMaxFrags) return false;
    t += in->n_kv[r];
  }
  return t <= kMaxFrags;
}
inline uint64_t total(const pbl_rangedel_runs* in) {
  uint64_t t = 0;
  for (uint32_t r = 0; r < in->n_runs; r++) t += in->n_kv[r];
  return t;
}

// The status the set of these (host) runs has, by the sequential checks.
inline uint32_t host_status(const pbl_rangedel_runs* in, std::vector<Run<cmp::HostReader>>* runs) {
  using R = cmp::HostReader;
  uint32_t st = PBL_OK, bad = 0;
  for (uint32_t r = 0; r < in->n_runs; r++) {
    const uint32_t s = in->runs[r].blk_status[0];
    if (s != PBL_OK) {
      if (st == PBL_OK) st = s;
      continue;
    }
    const Run<R> U = run_of<R>(in->runs[r]);
    const uint64_t k0 = in->runs[r].blk_kv_base[0], k1 = in->runs[r].blk_kv_base[1];
    if (k1 < k0 || k1 - k0 != in->n_kv[r] || uint64_t(U.S.n) != in->n_kv[r]) {
      bad |= kBadOrder;
      continue;
    }
    for (uint32_t j = 0; j < U.S.n; j++) bad |= check_fragment<R>(in->comparer, U, j);
    if (runs) runs->push_back(U);
  }
  return status_of(st, bad);
}

}  // namespace rangedel
}  // namespace pbl

extern "C" {

uint64_t pbl_rangedel_workspace_bytes(uint64_t n_fragments) { return pbl::rangedel::layout(n_fragments).size; }

int pbl_rangedel_set(const pbl_rangedel_runs* in, pbl_decode_out* set, void* ws, uint64_t ws_bytes, void* stream) {
  namespace M = pbl::rangedel;
  using namespace pbl;
  if (!M::runs_ok(in) || !set || !result::result_ok(*set, false)) return PBL_INVALID_ARG;
  const uint64_t T = M::total(in);
  const M::Layout L = M::layout(T);
  if (!result::ws_aligned(ws) || ws_bytes < L.size) return PBL_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  M::Args a{};
  for (uint32_t r = 0; r < in->n_runs; r++) {
    a.run[r] = in->runs[r];
    a.base[r + 1] = a.base[r] + in->n_kv[r];
  }
  a.out = *set;
  a.snapshot = in->snapshot;
  a.n_runs = in->n_runs;
  a.comparer = in->comparer;
  a.ws = static_cast<uint8_t*>(ws);
  a.has_level = in->level ? 1u : 0u;
  for (uint32_t r = 0; r < in->n_runs && in->level; r++) a.level[r] = in->level[r];
  if (hipMemsetAsync(set->totals, 0, sizeof(pbl_totals), st) != hipSuccess) return PBL_DEVICE_ERROR;
  // the header, the sizes and the tile sums; places nobody ranks name no boundary
  if (hipMemsetAsync(a.ws, 0, L.cover, st) != hipSuccess) return PBL_DEVICE_ERROR;
  if (L.n_items && hipMemsetAsync(a.ws + L.perm, 0xff, 4ull * L.n_items, st) != hipSuccess) return PBL_DEVICE_ERROR;
  const uint32_t f_grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>((T + M::kTPB - 1) / M::kTPB, 1), M::kGrid));
  const uint32_t e_grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>((L.n_items + M::kTPB - 1) / M::kTPB, 1), M::kGrid));
  const uint32_t t_grid = uint32_t(std::min<uint64_t>(L.nt, M::kGrid));
  seek::with_cmp(in->comparer, [&](auto c) {
    constexpr uint32_t kCmp = decltype(c)::value;
    hipLaunchKernelGGL(M::rangedel_validate_kernel<kCmp>, dim3(f_grid), dim3(M::kTPB), 0, st, a);
    if (T) hipLaunchKernelGGL(M::rangedel_rank_kernel<kCmp>, dim3(e_grid), dim3(M::kTPB), 0, st, a);
    hipLaunchKernelGGL(M::rangedel_place_kernel<kCmp>, dim3(t_grid), dim3(M::kTPB), 0, st, a);
    return 0;
  });
  hipLaunchKernelGGL(M::rangedel_bases_kernel, dim3(1), dim3(M::kTPB), 0, st, a);
  if (set->key_off) hipLaunchKernelGGL(M::rangedel_emit_kernel, dim3(t_grid), dim3(M::kTPB), 0, st, a);
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_rangedel_set_host(const pbl_rangedel_runs* in, pbl_decode_out* set) {
  namespace M = pbl::rangedel;
  using R = pbl::cmp::HostReader;
  if (!M::runs_ok(in) || !set || !pbl::result::result_ok(*set, false)) return PBL_INVALID_ARG;
  const pbl_decode_out& O = *set;
  std::vector<M::Run<R>> runs;
  const uint32_t st = M::host_status(in, &runs);
  struct B {
    const uint8_t* k;
    uint64_t kl;
  };
  std::vector<B> bs;
  if (st == PBL_OK) {
    // every boundary in (run, fragment index, start before end) order
    for (const M::Run<R>& U : runs)
      for (uint32_t j = 0; j < U.S.n; j++) {
        uint64_t l;
        const uint8_t* k = U.S.key(j, &l);
        bs.push_back(B{k, l});
        k = U.E.key(j, &l);
        bs.push_back(B{k, l});
      }
    const uint32_t c = in->comparer;
    std::stable_sort(bs.begin(), bs.end(), [c](const B& a, const B& b) { return pbl::cmp::key_cmp<R>(c, a.k, a.kl, b.k, b.kl) < 0; });
    bs.erase(std::unique(bs.begin(), bs.end(),
                         [c](const B& a, const B& b) { return pbl::cmp::key_cmp<R>(c, a.k, a.kl, b.k, b.kl) == 0; }),
             bs.end());
  }
  uint64_t kbytes = 0;
  for (const B& b : bs) kbytes += b.kl;
  uint32_t status = st;
  if (status == PBL_OK && kbytes > M::kMaxBytes) {
    status = PBL_UNSUPPORTED;
    bs.clear();
    kbytes = 0;
  }
  pbl_totals T{};
  T.n_kv = bs.size();
  T.key_bytes = kbytes;
  if (status != PBL_OK) {
    T.status_mask |= 1u << status;
    T.n_bad_blocks = 1;
  }
  O.blk_kv_base[0] = O.blk_key_base[0] = O.blk_val_base[0] = 0;
  O.blk_kv_base[1] = bs.size();
  O.blk_key_base[1] = kbytes;
  O.blk_val_base[1] = 0;
  if (O.blk_rst_base) O.blk_rst_base[0] = O.blk_rst_base[1] = 0;
  O.blk_status[0] = status;
  const bool over = bs.size() > O.kv_cap || kbytes > O.key_cap;
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *O.totals = T;
  if (over || !O.key_off) return PBL_OK;
  uint32_t ko = 0;
  for (size_t i = 0; i < bs.size(); i++) {
    // the brute-force maximum over all fragments
    uint64_t cover = 0;
    uint32_t lv = 0;
    for (size_t r = 0; r < runs.size(); r++) {
      const M::Run<R>& U = runs[r];
      for (uint32_t j = 0; j < U.S.n; j++) {
        uint64_t sl, el;
        const uint8_t *s = U.S.key(j, &sl), *e = U.E.key(j, &el);
        const uint64_t t = U.tr[j] >> 8;
        if (t == 0 || !M::is_visible(t, in->snapshot) || pbl::cmp::key_cmp<R>(in->comparer, s, sl, bs[i].k, bs[i].kl) > 0 ||
            pbl::cmp::key_cmp<R>(in->comparer, bs[i].k, bs[i].kl, e, el) >= 0)
          continue;
        if (t > cover) cover = t;
        if (in->level && (lv == 0 || uint32_t(in->level[r]) + 1 < lv)) lv = uint32_t(in->level[r]) + 1;
      }
    }
    O.trailer[i] = (cover << 8) | PBL_KIND_RANGEDEL;
    if (O.kv_flags) O.kv_flags[i] = 0;
    if (O.entry_off) O.entry_off[i] = lv;
    if (O.tiering_span_id) O.tiering_span_id[i] = O.tiering_attr[i] = 0;
    O.key_off[i] = ko;
    O.val_off[i] = 0;
    if (bs[i].kl) memcpy(O.key_bytes + ko, bs[i].k, bs[i].kl);
    ko += uint32_t(bs[i].kl);
  }
  O.key_off[bs.size()] = ko;
  O.val_off[bs.size()] = 0;
  return PBL_OK;
}

int pbl_rangedel_cover(const pbl_decode_out* set, const pbl_decode_out* batch, uint32_t n_blocks, uint64_t n_kv,
                       uint32_t comparer, uint64_t* cover_seq, void* stream) {
  return pbl_rangedel_cover_lv(set, batch, n_blocks, n_kv, comparer, nullptr, nullptr, cover_seq, stream);
}

int pbl_rangedel_cover_lv(const pbl_decode_out* set, const pbl_decode_out* batch, uint32_t n_blocks, uint64_t n_kv,
                          uint32_t comparer, const uint8_t* src_run, const uint8_t* run_level, uint64_t* cover_seq,
                          void* stream) {
  namespace M = pbl::rangedel;
  using namespace pbl;
  if (!set || !batch || !cover_seq || comparer > PBL_CMP_CRDB || !src_run != !run_level) return PBL_INVALID_ARG;
  if (src_run && !set->entry_off) return PBL_INVALID_ARG;
  if (!set->blk_status || !set->blk_kv_base || !set->blk_key_base || !set->key_off || !set->key_bytes || !set->trailer)
    return PBL_INVALID_ARG;
  if (!batch->blk_status || !batch->blk_kv_base || !batch->blk_key_base || !batch->key_off || !batch->key_bytes)
    return PBL_INVALID_ARG;
  if (n_kv == 0) return PBL_OK;
  M::CoverArgs a{*set, *batch, n_blocks, comparer, n_kv, cover_seq, src_run, {}};
  for (uint32_t r = 0; r < M::kMaxRuns && run_level; r++) a.run_level[r] = run_level[r];
  const uint64_t waves = (n_kv + kWave - 1) / kWave, wpb = M::kTPB / kWave;
  const uint32_t grid = uint32_t(std::min<uint64_t>((waves + wpb - 1) / wpb, 1u << 16));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  seek::with_cmp(comparer, [&](auto c) {
    hipLaunchKernelGGL(M::rangedel_cover_kernel<decltype(c)::value>, dim3(grid), dim3(M::kTPB), 0, st, a);
    return 0;
  });
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_rangedel_cover_host(const pbl_rangedel_runs* in, const pbl_decode_out* batch, uint32_t n_blocks,
                            uint64_t* cover_seq, uint32_t* status) {
  return pbl_rangedel_cover_host_lv(in, batch, n_blocks, nullptr, nullptr, cover_seq, status);
}

int pbl_rangedel_cover_host_lv(const pbl_rangedel_runs* in, const pbl_decode_out* batch, uint32_t n_blocks,
                               const uint8_t* src_run, const uint8_t* run_level, uint64_t* cover_seq, uint32_t* status) {
  namespace M = pbl::rangedel;
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!M::runs_ok(in) || !batch || !cover_seq || !src_run != !run_level || (src_run && !in->level)) return PBL_INVALID_ARG;
  if (!batch->blk_status || !batch->blk_kv_base || !batch->blk_key_base || !batch->key_off || !batch->key_bytes)
    return PBL_INVALID_ARG;
  std::vector<M::Run<R>> runs;
  const uint32_t st = M::host_status(in, &runs);
  if (status) *status = st;
  const uint64_t n_kv = n_blocks ? batch->blk_kv_base[n_blocks] : 0;
  for (uint64_t i = 0; i < n_kv; i++) cover_seq[i] = 0;
  if (st != PBL_OK) return PBL_OK;
  pbl_seek_queries sq{};
  const K::View<R> V(*batch, n_blocks, sq, nullptr, 0);
  for (uint32_t q = 0; q < n_blocks; q++) {
    if (batch->blk_status[q] != PBL_OK) continue;
    const K::Block<R> B(V, q);
    for (uint32_t x = 0; x < B.n; x++) {
      uint64_t kl;
      const uint8_t* k = B.key(x, &kl);
      uint64_t cover = 0;
      const uint32_t pr = src_run ? src_run[B.kv0 + x] : 0u;
      for (size_t r = 0; r < runs.size(); r++) {
        const M::Run<R>& U = runs[r];
        for (uint32_t j = 0; j < U.S.n; j++) {
          uint64_t sl, el;
          const uint8_t *s = U.S.key(j, &sl), *e = U.E.key(j, &el);
          const uint64_t t = U.tr[j] >> 8;
          if (t == 0 || !M::is_visible(t, in->snapshot) || pbl::cmp::key_cmp<R>(in->comparer, s, sl, k, kl) > 0 ||
              pbl::cmp::key_cmp<R>(in->comparer, k, kl, e, el) >= 0)
            continue;
          // a tombstone of a shallower level deletes whatever the sequence numbers say
          if (src_run && pr < M::kMaxRuns && in->level[r] < run_level[pr]) cover = PBL_RANGEDEL_ALL;
          else if (t > cover) cover = t;
        }
      }
      cover_seq[B.kv0 + x] = cover;
    }
  }
  return PBL_OK;
}

size_t pbl_rangedel_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {sizeof(pbl_rangedel_runs),         PBL_OFF(pbl_rangedel_runs, runs),
                        PBL_OFF(pbl_rangedel_runs, n_kv),  PBL_OFF(pbl_rangedel_runs, n_runs),
                        PBL_OFF(pbl_rangedel_runs, comparer), PBL_OFF(pbl_rangedel_runs, snapshot),
                        PBL_OFF(pbl_rangedel_runs, level)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
