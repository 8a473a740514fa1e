// rowenc.hip — the row-block encoder: a sorted decoded batch back into row-format
// data blocks, on the device.  include/pebble_amd.h states the
// rules (RawRowWriter + rowblk.Writer + FlushGovernor) once; this file is
//   pbl_rowenc_size / pbl_rowenc_batch   the device form
//   pbl_rowenc_batch_host                the reference's sequential loop over host
//                                        arrays, built on pbl_rowblk_writer
//
// The reference walks a table KV by KV.  Nothing in it needs the walk:
//   describe   a lane per KV.  An entry's bytes depend on its stream predecessor
//              only: set_same, the obsolete inputs, the shared length and two
//              sizes, e_sh (the entry as a non-restart) and e_rs (with shared =
//              0).  The obsolete bit x_k = a_k | (p_k & x_{k-1}) is a scan of
//              2-bit maps.  Prefix sums: A over e_sh, C over !set_same, and D
//              over d = e_rs - e_sh + 4 WITH STRIDE ri (D sums every KV congruent
//              to k mod ri), scanned in column-major order of a matrix with ri
//              columns.  With them, for a block that starts at KV i,
//                S(i, j) = A[j] - A[i] + (D over i, i + ri, .. < j) + 4
//              and every entry offset and restart word are closed forms.
//   partition  next(i) per KV: a binary search on the monotone S(i, .) >= low,
//              then a walk to the first j that satisfies rule 7 (it ends where
//              S > high at the latest: bounded by a block, not by a stream).
//              Block starts are the orbit of each stream's first KV under next,
//              marked by pointer doubling: round r marks next^(2^r) of every
//              marked KV and squares the map; a round with nothing left to do
//              says so and the remaining launches return at once.  A scan over
//              the marks gives block ordinals, offsets and restart counts.
//   emit       a wave per output block, a lane per entry, 64 entries a step:
//              headers and key suffixes by their lane, values by the wave
//              (result::copy_values), global to global with byte-exact edges.
// Every scan is the tile form of result_core.hip.h: tile sums, one workgroup
// over the tile sums, then the tiles again.
#include <algorithm>

#include "result_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace rowenc {

constexpr int kTPB = 256;
constexpr uint32_t kTile = 256;  // KVs per tile
static_assert(kTPB == result::kTPB && kTile == uint32_t(kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kGrid = 2048;
constexpr uint64_t kHdr = 256;      // u32 words
constexpr uint32_t kHdrOver = 1;    // the result does not fit the capacities
constexpr uint32_t kHdrRound = 16;  // [16, 16 + 40): doubling round r has work left
constexpr uint32_t kMaxRounds = 40;
constexpr uint64_t kMaxEntry = 1ull << 31;
constexpr uint64_t kMaxKvs = 0xfffffffeull;

constexpr uint32_t kDel = 0, kSet = 1, kMerge = 2, kSingleDel = 7, kDelSized = 23;
constexpr uint32_t kAllFlags = PBL_ENC_VALUE_PREFIX | PBL_ENC_OBSOLETE | PBL_ENC_LOWEST_LEVEL;
// Per-KV flags (Ws::f).  kA | kP is the KV's obsolete map x -> a | (p & x).
constexpr uint32_t kA = 1, kP = 2, kSame = 4, kObs = 8, kAddP = 16, kFirst = 32;
constexpr uint32_t kId = kP;  // the identity map

PBL_HD inline bool tombstone(uint32_t kind) { return kind == kDel || kind == kSingleDel || kind == kDelSized; }
PBL_HD inline uint32_t uvarint_len(uint64_t x) {
  uint32_t n = 1;
  while (x >= 0x80) {
    x >>= 7;
    n++;
  }
  return n;
}
PBL_HD inline uint32_t low_of(const pbl_rowenc_opts& o) {
  return uint32_t((uint64_t(o.target_block_size) * o.block_size_threshold + 99) / 100);
}
PBL_HD inline uint64_t mn(uint64_t a, uint64_t b) { return a < b ? a : b; }
// m1, then m2
PBL_HD inline uint32_t then(uint32_t m1, uint32_t m2) { return ((m2 & kA) | ((m2 >> 1) & m1 & kA)) | (m1 & m2 & kP); }

struct Layout {
  uint64_t nt, ntp;
  uint64_t sbad, a, dx, ta, tc, td, tm, cn, sh, esh, d, c, nx, ord, tobs, tobx, f, reach, size;
};
__host__ __device__ inline Layout layout(uint32_t nb, uint64_t n_kv) {
  Layout L;
  L.nt = n_kv / kTile + 1;
  L.ntp = (2 * n_kv + 1) / kTile + 1;
  uint64_t o = kHdr;
  L.sbad = o;  o += 4ull * nb;
  o = (o + 15) & ~uint64_t(15);
  L.a = o;     o += 8ull * (n_kv + 1);
  L.dx = o;    o += 8ull * (2 * n_kv + 2);
  L.ta = o;    o += 8ull * L.nt;
  L.tc = o;    o += 8ull * L.nt;
  L.td = o;    o += 8ull * L.ntp;
  L.tm = o;    o += 3ull * 8 * L.nt;
  L.cn = o;    o += 4ull * (n_kv + 1);
  L.sh = o;    o += 4ull * n_kv;
  L.esh = o;   o += 4ull * n_kv;
  L.d = o;     o += 4ull * n_kv;
  L.c = o;     o += 4ull * n_kv;
  L.nx = o;    o += 3ull * 4 * (n_kv + 1);
  L.ord = o;   o += 4ull * (n_kv + 1);
  L.tobs = o;  o += 4ull * L.nt;
  L.tobx = o;  o += 4ull * (L.nt + 1);
  L.f = o;     o += n_kv;
  L.reach = o; o += n_kv + 1;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

// ---- device side ---------------------------------------------------------------
struct Args {
  pbl_decode_out in;
  pbl_rowenc_out out;
  pbl_rowenc_opts o;
  uint32_t nb, size_only, low, high;
  uint64_t n_kv;
  uint8_t* ws;
};

using GR = seek::GlobalReader;
using result::block_excl_scan64;
using result::block_of;
using result::block_sum64;

struct Ws {
  gptr<uint32_t> hdr, sbad, cn, sh, esh, d, c, nx0, nx1, nx2, ord, tobs, tobx;
  gptr<uint64_t> a, dx, ta, tc, td, tm;
  gptr<uint8_t> f, reach;
  gptr<const uint64_t> kvb;
  uint64_t N;         // KVs the batch holds
  uint64_t nt, ntp;   // tiles in use: of [0, N] and of [0, P]
  uint64_t ri, rows, P;  // the stride-ri scan: ri columns (at most N), rows, ri * rows positions
  uint64_t tms;
  bool fits;          // the batch holds no more KVs than the host said
  __device__ explicit Ws(const Args& A) {
    const Layout L = layout(A.nb, A.n_kv);
    uint8_t* ws = A.ws;
    auto w32 = [&](uint64_t o) { return to_glb(reinterpret_cast<uint32_t*>(ws + o)); };
    auto w64 = [&](uint64_t o) { return to_glb(reinterpret_cast<uint64_t*>(ws + o)); };
    hdr = w32(0);
    sbad = w32(L.sbad);
    a = w64(L.a);
    dx = w64(L.dx);
    ta = w64(L.ta);
    tc = w64(L.tc);
    td = w64(L.td);
    tm = w64(L.tm);
    cn = w32(L.cn);
    sh = w32(L.sh);
    esh = w32(L.esh);
    d = w32(L.d);
    c = w32(L.c);
    nx0 = w32(L.nx);
    nx1 = nx0 + (A.n_kv + 1);
    nx2 = nx1 + (A.n_kv + 1);
    ord = w32(L.ord);
    tobs = w32(L.tobs);
    tobx = w32(L.tobx);
    f = to_glb(ws + L.f);
    reach = to_glb(ws + L.reach);
    kvb = to_glb((const uint64_t*)A.in.blk_kv_base);
    const uint64_t held = A.nb ? kvb[A.nb] : 0;
    fits = held <= A.n_kv;
    N = fits ? held : 0;
    nt = N / kTile + 1;
    ri = N && A.o.restart_interval > N ? N : A.o.restart_interval;
    rows = (N + ri - 1) / ri;
    P = ri * rows;
    ntp = P / kTile + 1;
    tms = L.nt;
  }
  __device__ gptr<uint64_t> tmk(int comp) const { return tm + uint64_t(comp) * tms; }
  // the sum of d over KVs i, i + ri, ... < j (j > i)
  __device__ uint64_t dsum(uint64_t i, uint64_t j) const {
    const uint64_t base = (i % ri) * rows + i / ri;
    return dx[base + (j - 1 - i) / ri + 1] - dx[base];
  }
  // EstimatedSize of the block of KVs [i, j), j > i
  __device__ uint64_t S(uint64_t i, uint64_t j) const { return a[j] - a[i] + dsum(i, j) + 4; }
  // the KV at position p of the stride scan's order (>= N: none)
  __device__ uint64_t kv_at(uint64_t p) const { return p < P ? (p % rows) * ri + p / rows : ~0ull; }
};

struct KeyRef {
  gptr<const uint8_t> p;
  uint64_t n;
};
__device__ inline KeyRef key_of(const Args& A, uint32_t q, uint64_t i) {
  const gptr<const uint32_t> ko = to_glb((const uint32_t*)A.in.key_off) + (i + q);
  const uint32_t o = ko[0];
  return KeyRef{to_glb((const uint8_t*)A.in.key_bytes) + (to_glb((const uint64_t*)A.in.blk_key_base)[q] + o),
                uint64_t(ko[1]) - o};
}
__device__ inline bool stream_ok(const Args& A, const Ws& W, uint32_t q) {
  return to_glb((const uint32_t*)A.in.blk_status)[q] == PBL_OK && W.sbad[q] == 0;
}

// Inclusive scan of obsolete maps over the workgroup; *total = all 256.  `lds`: 4 words.
__device__ inline uint32_t block_incl_scan_map(uint32_t m, uint32_t* lds, uint32_t* total) {
  const int l = lane_id();
  uint32_t inc = m;
#pragma unroll
  for (int dd = 1; dd < kWave; dd <<= 1) {
    const uint32_t o = uint32_t(__shfl_up(int(inc), dd, kWave));
    if (l >= dd) inc = then(o, inc);
  }
  __syncthreads();
  if (l == kWave - 1) lds[wave_id()] = inc;
  __syncthreads();
  uint32_t before = kId, t = kId;
  for (int w = 0; w < kTPB / kWave; w++) {
    const uint32_t s = lds[w];
    if (w < wave_id()) before = then(before, s);
    t = then(t, s);
  }
  *total = t;
  return then(before, inc);
}

// The common prefix of a[0, n) and b[0, n), 8 bytes a step (both readable past n).
__device__ inline uint64_t common_prefix(gptr<const uint8_t> a, gptr<const uint8_t> b, uint64_t n) {
  for (uint64_t o = 0; o < n; o += 8) {
    const uint64_t x = *(gptr<const u64_u>)(a + o) ^ *(gptr<const u64_u>)(b + o);
    if (x) {
      const uint64_t s = o + (uint64_t(__builtin_ctzll(x)) >> 3);
      return s < n ? s : n;
    }
  }
  return n;
}

// Describe, first half: what needs the comparer.  f[] and the tiles' obsolete maps.
template <uint32_t kCmp>
__global__ __launch_bounds__(kTPB) void rowenc_classify_kernel(Args A) {
  __shared__ uint32_t lds[4];
  const Ws W(A);
  const bool vp = (A.o.flags & PBL_ENC_VALUE_PREFIX) != 0, ob = (A.o.flags & PBL_ENC_OBSOLETE) != 0,
             lowest = (A.o.flags & PBL_ENC_LOWEST_LEVEL) != 0;
  const gptr<const uint64_t> tr = to_glb((const uint64_t*)A.in.trailer);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = t * kTile + threadIdx.x;
    uint32_t f = kId;
    if (i < W.N) {
      f = 0;
      const uint32_t q = block_of(W.kvb, A.nb, i);
      const bool pred = i > W.kvb[q];
      const uint32_t kind = uint32_t(tr[i] & 0xff);
      if (!pred) f |= kFirst;
      if (vp && kind == kSet) f |= kAddP;
      if (pred && vp) {
        const KeyRef cur = key_of(A, q, i), prev = key_of(A, q, i - 1);
        const uint32_t pk = uint32_t(tr[i - 1] & 0xff);
        if (kind == kSet && pk == kSet) {
          const uint64_t sc = cmp::key_split<GR>(kCmp, cur.p, cur.n), sp = cmp::key_split<GR>(kCmp, prev.p, prev.n);
          if (cmp::key_cmp<GR>(kCmp, prev.p, sp, cur.p, sc) == 0) f |= kSame;
        }
        if (ob && cmp::key_cmp<GR>(kCmp, prev.p, prev.n, cur.p, cur.n) == 0) f |= kP | (pk != kMerge ? kA : 0u);
      }
      if (ob) {
        if (A.in.kv_flags && (to_glb((const uint8_t*)A.in.kv_flags)[i] & PBL_KV_OBSOLETE)) f |= kA;
        if (pred && lowest && tombstone(kind)) f |= kA;
      }
      W.f[i] = uint8_t(f);
    }
    uint32_t tot;
    block_incl_scan_map(f & (kA | kP), lds, &tot);
    if (threadIdx.x == 0) W.tobs[t] = tot;
  }
}

// One workgroup: tobx[t] = the maps of the tiles before t, composed.
__global__ __launch_bounds__(kTPB) void rowenc_obs_tiles_kernel(Args A) {
  __shared__ uint32_t lds[4];
  const Ws W(A);
  uint32_t carry = kId;
  if (threadIdx.x == 0) W.tobx[0] = kId;
  for (uint64_t t0 = 0; t0 < W.nt; t0 += kTPB) {
    const uint64_t t = t0 + threadIdx.x;
    uint32_t tot;
    const uint32_t inc = block_incl_scan_map(t < W.nt ? W.tobs[t] : kId, lds, &tot);
    if (t < W.nt) W.tobx[t + 1] = then(carry, inc);
    carry = then(carry, tot);
  }
}

// Describe, second half: the obsolete bit, the shared length, the sizes; the tile
// sums of A and C.
__global__ __launch_bounds__(kTPB) void rowenc_describe_kernel(Args A) {
  __shared__ uint32_t lds[4];
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  const bool vp = (A.o.flags & PBL_ENC_VALUE_PREFIX) != 0;
  const gptr<const uint64_t> trl = to_glb((const uint64_t*)A.in.trailer);
  const gptr<const uint32_t> vo = to_glb((const uint32_t*)A.in.val_off);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = t * kTile + threadIdx.x;
    uint32_t f = i < W.N ? W.f[i] : kId;
    uint32_t tot;
    const uint32_t inc = block_incl_scan_map(f & (kA | kP), lds, &tot);
    uint64_t esh = 0, ns = 0;
    if (i < W.N) {
      const bool obs = (then(W.tobx[t], inc) & kA) != 0;
      if (obs) f |= kObs;
      const uint32_t q = block_of(W.kvb, A.nb, i);
      const KeyRef cur = key_of(A, q, i);
      const uint64_t tr = trl[i] | (obs ? 64u : 0u);
      const uint64_t svl = uint64_t(vo[i + q + 1] - vo[i + q]) + ((f & kAddP) ? 1 : 0), ikl = cur.n + 8;
      uint64_t shared = 0;
      if (!(f & kFirst)) {
        const KeyRef prev = key_of(A, q, i - 1);
        const uint64_t ptr = trl[i - 1];  // (read only without VALUE_PREFIX, where nothing is obsolete)
        const uint64_t cap = vp ? cmp::key_split<GR>(A.o.comparer, prev.p, prev.n) : cur.n;
        const uint64_t limit = mn(cap, mn(prev.n + 8, ikl));
        const uint64_t m = mn(limit, mn(prev.n, cur.n));
        uint64_t s = common_prefix(prev.p, cur.p, m);
        if (s == m) {
          while (s < limit) {
            const uint32_t bp = s < prev.n ? uint32_t(prev.p[s]) : uint32_t(ptr >> (8 * (s - prev.n))) & 0xffu;
            const uint32_t bc = s < cur.n ? uint32_t(cur.p[s]) : uint32_t(tr >> (8 * (s - cur.n))) & 0xffu;
            if (bp != bc) break;
            s++;
          }
        }
        shared = s;
      }
      const uint64_t lv = uvarint_len(svl);
      esh = uvarint_len(shared) + uvarint_len(ikl - shared) + lv + (ikl - shared) + svl;
      uint64_t ers = 1 + uvarint_len(ikl) + lv + ikl + svl;
      uint64_t cost = ikl + svl + 4 + uvarint_len(ikl) + lv;
      if (ers >= kMaxEntry) {  // rule 8: the stream is refused; its sizes are never used
        W.sbad[q] = PBL_UNSUPPORTED;
        esh = ers = cost = 3;
      }
      W.sh[i] = uint32_t(shared);
      W.esh[i] = uint32_t(esh);
      W.d[i] = uint32_t(ers - esh + 4);
      W.c[i] = uint32_t(cost);
      W.f[i] = uint8_t(f);
      ns = (f & kSame) ? 0 : 1;
    }
    const uint64_t sa = block_sum64(esh, lds64), sc = block_sum64(ns, lds64);
    if (threadIdx.x == 0) {
      W.ta[t] = sa;
      W.tc[t] = sc;
    }
  }
}

// The tile sums of d in the stride scan's order.
__global__ __launch_bounds__(kTPB) void rowenc_dsum_kernel(Args A) {
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  for (uint64_t t = blockIdx.x; t < W.ntp; t += gridDim.x) {
    const uint64_t k = W.kv_at(t * kTile + threadIdx.x);
    const uint64_t s = block_sum64(k < W.N ? W.d[k] : 0, lds64);
    if (threadIdx.x == 0) W.td[t] = s;
  }
}

// One workgroup: the tile sums of A, C and D to exclusive prefixes.
__global__ __launch_bounds__(kTPB) void rowenc_tile_scan_kernel(Args A) {
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  const gptr<uint64_t> ac[2] = {W.ta, W.tc};
  result::tile_scan_inplace<2>(ac, W.nt, lds64);
  const gptr<uint64_t> dd[1] = {W.td};
  result::tile_scan_inplace<1>(dd, W.ntp, lds64);
}

// The per-KV prefixes: a[0..N], cn[0..N], dx[0..P].
__global__ __launch_bounds__(kTPB) void rowenc_prefix_kernel(Args A) {
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  const uint64_t tiles = W.nt > W.ntp ? W.nt : W.ntp;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint64_t i = t * kTile + threadIdx.x;
    uint64_t tot;
    if (t < W.nt) {
      const uint64_t ea = block_excl_scan64(i < W.N ? W.esh[i] : 0, lds64, &tot);
      const uint64_t ec = block_excl_scan64(i < W.N ? ((W.f[i] & kSame) ? 0 : 1) : 0, lds64, &tot);
      if (i <= W.N) {
        W.a[i] = W.ta[t] + ea;
        W.cn[i] = uint32_t(W.tc[t] + ec);
      }
    }
    if (t < W.ntp) {
      const uint64_t k = W.kv_at(i);
      const uint64_t ed = block_excl_scan64(k < W.N ? W.d[k] : 0, lds64, &tot);
      if (i <= W.P) W.dx[i] = W.td[t] + ed;
    }
  }
}

// Partition: next(i) for every KV (N = the stream ends with this block), and
// the marks of the streams' first KVs.
__global__ __launch_bounds__(kTPB) void rowenc_next_kernel(Args A) {
  const Ws W(A);
  const uint64_t N = W.N, ri = A.o.restart_interval;
  for (uint64_t i = uint64_t(blockIdx.x) * kTPB + threadIdx.x; i <= N; i += uint64_t(gridDim.x) * kTPB) {
    uint64_t nx = N;
    bool start = false;
    if (i < N) {
      const uint32_t q = block_of(W.kvb, A.nb, i);
      if (stream_ok(A, W, q)) {
        const uint64_t e = W.kvb[q + 1];
        start = i == W.kvb[q];
        // the first j in (i, e] with S(i, j) >= low; e when there is none
        uint64_t lo = i + 1, hi = e;
        while (lo < hi) {
          const uint64_t m = lo + (hi - lo) / 2;
          if (W.S(i, m) >= A.low) hi = m;
          else lo = m + 1;
        }
        uint64_t j = lo;
        if (j < e) {
          uint64_t s = W.S(i, j);  // >= low: the search found j below e
          for (; j < e; j++) {
            const bool rst = (j - i) % ri == 0;
            if (s + W.c[j] + (rst ? 4 : 0) > A.high) break;
            s += (W.a[j + 1] - W.a[j]) + (rst ? W.d[j] : 0);
          }
        }
        nx = j < e ? j : N;
      }
    }
    W.nx0[i] = uint32_t(nx);
    W.reach[i] = start ? 1 : 0;
  }
}

// Doubling round r: every marked KV marks next_r of itself; next_{r+1} = next_r . next_r.
__global__ __launch_bounds__(kTPB) void rowenc_round_kernel(Args A, uint32_t r) {
  const Ws W(A);
  if (r && W.hdr[kHdrRound + r] == 0) return;
  const uint32_t N = uint32_t(W.N);
  const gptr<uint32_t> R = r == 0 ? W.nx0 : (r & 1) ? W.nx1 : W.nx2, Wr = (r & 1) ? W.nx2 : W.nx1;
  bool more = false;
  for (uint64_t i = uint64_t(blockIdx.x) * kTPB + threadIdx.x; i <= N; i += uint64_t(gridDim.x) * kTPB) {
    const uint32_t n1 = R[i];
    uint32_t n2 = N;
    if (n1 < N) {
      if (W.reach[i]) W.reach[n1] = 1;
      n2 = R[n1];
      more |= n2 < N;
    }
    Wr[i] = n2;
  }
  if (__ballot(more) && lane_id() == 0 && r + 1 < kMaxRounds) W.hdr[kHdrRound + r + 1] = 1;
}

// What a marked KV's block is.
struct Mark {
  uint64_t end, len, nrst;
  uint32_t q;
};
__device__ inline Mark mark_of(const Args& A, const Ws& W, uint64_t i) {
  Mark M;
  M.q = block_of(W.kvb, A.nb, i);
  const uint32_t nx = W.nx0[i];
  M.end = nx < W.N ? nx : W.kvb[M.q + 1];
  M.len = W.S(i, M.end);
  M.nrst = (M.end - 1 - i) / A.o.restart_interval + 1;
  return M;
}

__global__ __launch_bounds__(kTPB) void rowenc_mark_sum_kernel(Args A) {
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = t * kTile + threadIdx.x;
    uint64_t v[3] = {0, 0, 0};
    if (i < W.N && W.reach[i]) {
      const Mark M = mark_of(A, W, i);
      v[0] = 1;
      v[1] = (M.len + 15) & ~uint64_t(15);
      v[2] = M.nrst;
    }
    for (int c = 0; c < 3; c++) {
      const uint64_t s = block_sum64(v[c], lds64);
      if (threadIdx.x == 0) W.tmk(c)[t] = s;
    }
  }
}

__global__ __launch_bounds__(kTPB) void rowenc_mark_scan_kernel(Args A) {
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  const gptr<uint64_t> m[3] = {W.tmk(0), W.tmk(1), W.tmk(2)};
  result::tile_scan_inplace<3>(m, W.nt, lds64);
}

// Block ordinals per KV, the per-block arrays, the totals and the capacity check.
__global__ __launch_bounds__(kTPB) void rowenc_blocks_kernel(Args A) {
  __shared__ uint64_t lds64[4];
  const Ws W(A);
  const pbl_rowenc_out& O = A.out;
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t i = t * kTile + threadIdx.x;
    uint64_t v[3] = {0, 0, 0}, ex[3], tot;
    Mark M{};
    const bool marked = i < W.N && W.reach[i];
    if (marked) {
      M = mark_of(A, W, i);
      v[0] = 1;
      v[1] = (M.len + 15) & ~uint64_t(15);
      v[2] = M.nrst;
    }
    for (int c = 0; c < 3; c++) ex[c] = W.tmk(c)[t] + block_excl_scan64(v[c], lds64, &tot);
    if (i <= W.N) W.ord[i] = uint32_t(ex[0]);
    if (!A.size_only) {
      if (marked && ex[0] < O.block_cap) {
        to_glb(O.block_off)[ex[0]] = ex[1];
        to_glb(O.block_len)[ex[0]] = uint32_t(M.len);
        to_glb(O.block_stream)[ex[0]] = M.q;
        to_glb(O.block_first_kv)[ex[0]] = i;
        to_glb(O.block_n_kv)[ex[0]] = uint32_t(M.end - i);
      }
      if (O.obsolete && i < W.N)
        to_glb(O.obsolete)[i] = stream_ok(A, W, block_of(W.kvb, A.nb, i)) && (W.f[i] & kObs) ? 1 : 0;
    }
    if (i == W.N) {
      const gptr<pbl_rowenc_totals> T = to_glb(O.totals);
      T->n_blocks = ex[0];
      T->block_bytes = ex[1];
      T->n_restarts = ex[2];
      const bool over = !A.size_only && (ex[0] > O.block_cap || ex[1] > O.blocks_cap);
      W.hdr[kHdrOver] = over ? 1 : 0;
      if (over) g_atomic_or(&O.totals->status_mask, 1u << PBL_OVERFLOW);
    }
  }
}

__global__ __launch_bounds__(kTPB) void rowenc_streams_kernel(Args A) {
  const Ws W(A);
  const pbl_rowenc_out& O = A.out;
  for (uint64_t q = uint64_t(blockIdx.x) * kTPB + threadIdx.x; q <= A.nb; q += uint64_t(gridDim.x) * kTPB) {
    const uint64_t at = W.fits ? W.kvb[q] : 0;
    to_glb(O.stream_block_base)[q] = W.ord[at < W.N ? at : W.N];
    if (q == A.nb) break;
    uint32_t st = to_glb((const uint32_t*)A.in.blk_status)[q];
    if (st == PBL_OK) st = W.fits ? W.sbad[q] : uint32_t(PBL_INVALID_ARG);
    to_glb(O.stream_status)[q] = st;
    if (st != PBL_OK) {
      g_atomic_or(&O.totals->status_mask, 1u << st);
      g_atomic_add(&O.totals->n_bad_streams, 1u);
    }
  }
}

__device__ inline gptr<uint8_t> put_uvarint(gptr<uint8_t> p, uint32_t x) {
  while (x >= 0x80) {
    *p++ = uint8_t(x) | 0x80;
    x >>= 7;
  }
  *p++ = uint8_t(x);
  return p;
}

// Emit: a wave per output block, a lane per entry, 64 entries a step.  Every
// byte of [block_off, block_off + align16(block_len)) is written exactly once.
__global__ __launch_bounds__(kTPB) void rowenc_emit_kernel(Args A) {
  const Ws W(A);
  if (W.hdr[kHdrOver]) return;
  const pbl_rowenc_out& O = A.out;
  const uint64_t n_blocks = to_glb(O.totals)->n_blocks, ri = A.o.restart_interval;
  const uint32_t lane = lane_id();
  const gptr<const uint64_t> trl = to_glb((const uint64_t*)A.in.trailer);
  const gptr<const uint32_t> vo = to_glb((const uint32_t*)A.in.val_off);
  const gptr<const uint8_t> vbytes = to_glb((const uint8_t*)A.in.val_bytes);
  const gptr<const uint64_t> valb = to_glb((const uint64_t*)A.in.blk_val_base);
  for (uint64_t b = uint64_t(blockIdx.x) * (kTPB / kWave) + wave_id(); b < n_blocks;
       b += uint64_t(gridDim.x) * (kTPB / kWave)) {
    const uint64_t i0 = to_glb(O.block_first_kv)[b], n = to_glb(O.block_n_kv)[b];
    const uint32_t q = to_glb(O.block_stream)[b], len = to_glb(O.block_len)[b];
    const gptr<uint8_t> dst = to_glb(O.blocks) + to_glb(O.block_off)[b];
    const uint64_t a0 = W.a[i0], vbase = valb[q];
    // the offset of block entry at KV k (k = i0 + n: the end of the entry area)
    auto entry_off = [&](uint64_t k) -> uint64_t {
      return k == i0 ? 0 : W.a[k] - a0 + W.dsum(i0, k) - 4 * ((k - 1 - i0) / ri + 1);
    };
    for (uint64_t base = 0; base < n; base += kWave) {
      const uint64_t rel = base + lane, k = i0 + rel;
      const bool ok = rel < n;
      uint32_t vlen = 0;
      gptr<const uint8_t> vsrc = vbytes;
      gptr<uint8_t> vdst = dst;
      if (ok) {
        const uint32_t f = W.f[k];
        const bool rst = rel % ri == 0;
        const uint32_t shared = rst ? 0u : W.sh[k];
        const KeyRef key = key_of(A, q, k);
        const uint64_t tr = trl[k] | ((f & kObs) ? 64u : 0u);
        const uint32_t v0 = vo[k + q];
        vlen = vo[k + q + 1] - v0;
        vsrc = vbytes + (vbase + v0);
        const uint32_t addp = (f & kAddP) ? 1 : 0, ikl = uint32_t(key.n) + 8;
        gptr<uint8_t> p = dst + entry_off(k);
        p = put_uvarint(p, shared);
        p = put_uvarint(p, ikl - shared);
        p = put_uvarint(p, vlen + addp);
        if (shared < key.n) {
          copy_chunks(p, key.p + shared, uint32_t(key.n) - shared);
          p += key.n - shared;
        }
        const uint32_t tb = shared > key.n ? shared - uint32_t(key.n) : 0;  // trailer bytes shared (rule 2's trap)
        if (tb == 0) {
          *(gptr<u64_u>)p = tr;
        } else {
          for (uint32_t x = tb; x < 8; x++) p[x - tb] = uint8_t(tr >> (8 * x));
        }
        p += 8 - tb;
        if (addp) *p++ = (f & kSame) ? 0x20 : 0x00;
        vdst = p;
      }
      result::copy_values(ok, vlen, vsrc, vdst);
    }
    // the restart words, their count, and zeros up to the 16-byte boundary
    const uint64_t nrst = (n - 1) / ri + 1;
    const gptr<uint8_t> tail = dst + entry_off(i0 + n);
    for (uint64_t r = lane; r <= nrst; r += kWave) {
      uint32_t w = uint32_t(nrst);
      if (r < nrst) {
        const uint64_t k = i0 + r * ri;
        w = uint32_t(entry_off(k));
        if (r >= 1 && W.cn[k + 1] == W.cn[k - ri + 1]) w |= 1u << 31;
      }
      *(gptr<u32_u>)(tail + 4 * r) = w;
    }
    const uint32_t pad = (16 - (len & 15)) & 15;
    if (lane < pad) dst[len + lane] = 0;
  }
}

// ---- host side -----------------------------------------------------------------
inline bool opts_ok(const pbl_rowenc_opts* o) {
  if (!o || o->restart_interval == 0 || o->target_block_size == 0 || o->target_block_size >= (1u << 31)) return false;
  if (o->comparer > PBL_CMP_CRDB || (o->flags & ~kAllFlags)) return false;
  if ((o->flags & PBL_ENC_OBSOLETE) && !(o->flags & PBL_ENC_VALUE_PREFIX)) return false;
  return (uint64_t(o->target_block_size) * o->block_size_threshold + 99) / 100 <= 0xffffffffull;  // low fits 32 bits
}
inline bool out_ok(const pbl_rowenc_out* o, bool size_only) {
  if (!o || !o->totals || !o->stream_block_base || !o->stream_status) return false;
  if (size_only) return true;
  if (o->block_cap && (!o->block_off || !o->block_len || !o->block_stream || !o->block_first_kv || !o->block_n_kv))
    return false;
  return !(o->blocks_cap && !o->blocks);
}

inline int launch(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out, void* ws, uint64_t ws_bytes,
                  uint32_t flags, bool size_only, hipStream_t st) {
  if (!in || !opts_ok(opts) || !out_ok(out, size_only) || !result::source_ok(&in->batch)) return PBL_INVALID_ARG;
  if (flags & ~(size_only ? 0u : uint32_t(PBL_ROWENC_SIZED))) return PBL_INVALID_ARG;
  if (in->n_kv > kMaxKvs) return PBL_UNSUPPORTED;
  const uint32_t nb = in->n_streams;
  const uint64_t n_kv = in->n_kv;
  const Layout L = layout(nb, n_kv);
  if (!result::ws_aligned(ws) || ws_bytes < L.size) return PBL_INVALID_ARG;
  Args a{};
  a.in = in->batch;
  a.out = *out;
  a.o = *opts;
  a.nb = nb;
  a.size_only = size_only ? 1u : 0u;
  a.low = low_of(*opts);
  a.high = opts->target_block_size;
  a.n_kv = n_kv;
  a.ws = static_cast<uint8_t*>(ws);
  if (hipMemsetAsync(out->totals, 0, sizeof(pbl_rowenc_totals), st) != hipSuccess) return PBL_DEVICE_ERROR;
  const uint32_t t_grid = uint32_t(std::min<uint64_t>(L.nt, kGrid));
  const uint32_t p_grid = uint32_t(std::min<uint64_t>(L.ntp, kGrid));
  if (!(flags & PBL_ROWENC_SIZED)) {
    if (hipMemsetAsync(a.ws, 0, L.a, st) != hipSuccess) return PBL_DEVICE_ERROR;  // the header and the stream flags
    seek::with_cmp(opts->comparer, [&](auto c) {
      hipLaunchKernelGGL((rowenc_classify_kernel<decltype(c)::value>), dim3(t_grid), dim3(kTPB), 0, st, a);
      return 0;
    });
    hipLaunchKernelGGL(rowenc_obs_tiles_kernel, dim3(1), dim3(kTPB), 0, st, a);
    hipLaunchKernelGGL(rowenc_describe_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
    hipLaunchKernelGGL(rowenc_dsum_kernel, dim3(p_grid), dim3(kTPB), 0, st, a);
    hipLaunchKernelGGL(rowenc_tile_scan_kernel, dim3(1), dim3(kTPB), 0, st, a);
    hipLaunchKernelGGL(rowenc_prefix_kernel, dim3(p_grid), dim3(kTPB), 0, st, a);
    hipLaunchKernelGGL(rowenc_next_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
    // 2^rounds > n_kv >= the blocks of any stream
    uint32_t rounds = 0;
    while (rounds < kMaxRounds && (n_kv >> rounds)) rounds++;
    for (uint32_t r = 0; r < rounds; r++)
      hipLaunchKernelGGL(rowenc_round_kernel, dim3(t_grid), dim3(kTPB), 0, st, a, r);
    hipLaunchKernelGGL(rowenc_mark_sum_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
    hipLaunchKernelGGL(rowenc_mark_scan_kernel, dim3(1), dim3(kTPB), 0, st, a);
  }
  hipLaunchKernelGGL(rowenc_blocks_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
  hipLaunchKernelGGL(rowenc_streams_kernel, dim3(std::min((nb + 1 + kTPB - 1) / kTPB, kGrid)), dim3(kTPB), 0, st, a);
  if (!size_only && out->block_cap) {
    const uint64_t wgs = (out->block_cap + kTPB / kWave - 1) / (kTPB / kWave);
    hipLaunchKernelGGL(rowenc_emit_kernel, dim3(uint32_t(std::min<uint64_t>(wgs, kGrid))), dim3(kTPB), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

// The sequential loop: RawRowWriter.addPoint per KV, one pbl_rowblk_writer per
// block, shouldFlush before every Add.
int batch_host(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out) {
  using R = cmp::HostReader;
  if (!in || !opts_ok(opts) || !out_ok(out, false) || !result::source_ok(&in->batch)) return PBL_INVALID_ARG;
  const pbl_decode_out& D = in->batch;
  const uint32_t nb = in->n_streams, cmpr = opts->comparer;
  const int ri = int(std::min<uint32_t>(opts->restart_interval, 0x7fffffffu));
  const bool vp = (opts->flags & PBL_ENC_VALUE_PREFIX) != 0, ob = (opts->flags & PBL_ENC_OBSOLETE) != 0,
             lowest = (opts->flags & PBL_ENC_LOWEST_LEVEL) != 0;
  const uint64_t low = low_of(*opts), high = opts->target_block_size;
  pbl_rowenc_totals T{};
  pbl_rowblk_writer* w = pbl_rowblk_writer_new(ri);
  bool over = false;
  if (out->obsolete && nb)
    for (uint64_t i = 0; i < D.blk_kv_base[nb]; i++) out->obsolete[i] = 0;
  for (uint32_t q = 0; q < nb; q++) {
    out->stream_block_base[q] = T.n_blocks;
    uint32_t st = D.blk_status[q];
    const uint64_t k0 = D.blk_kv_base[q], k1 = D.blk_kv_base[q + 1];
    const uint32_t *ko = D.key_off + k0 + q, *vo = D.val_off + k0 + q;
    const uint8_t *kb = D.key_bytes + D.blk_key_base[q], *vb = D.val_bytes + D.blk_val_base[q];
    auto ikl_of = [&](uint64_t j) { return uint64_t(ko[j + 1] - ko[j]) + 8; };
    auto svl_of = [&](uint64_t j) {
      return uint64_t(vo[j + 1] - vo[j]) + (vp && (D.trailer[k0 + j] & 0xff) == kSet ? 1 : 0);
    };
    if (st == PBL_OK)
      for (uint64_t j = 0; j < k1 - k0; j++)
        if (1 + uvarint_len(ikl_of(j)) + uvarint_len(svl_of(j)) + ikl_of(j) + svl_of(j) >= kMaxEntry) st = PBL_UNSUPPORTED;
    out->stream_status[q] = st;
    if (st != PBL_OK) {
      T.status_mask |= 1u << st;
      T.n_bad_streams++;
      continue;
    }
    uint64_t first = k0;
    auto flush = [&](uint64_t end) {  // the block of KVs [first, end)
      const uint64_t len = pbl_rowblk_writer_estimated_size(w), al = (len + 15) & ~uint64_t(15);
      const uint64_t b = T.n_blocks, off = T.block_bytes;
      T.n_restarts += (end - first - 1) / uint64_t(ri) + 1;
      if (b < out->block_cap && off + al <= out->blocks_cap) {
        out->block_off[b] = off;
        out->block_len[b] = uint32_t(len);
        out->block_stream[b] = q;
        out->block_first_kv[b] = first;
        out->block_n_kv[b] = uint32_t(end - first);
        pbl_rowblk_writer_finish(w, out->blocks + off, len);
        std::fill(out->blocks + off + len, out->blocks + off + al, uint8_t(0));
      } else {
        over = true;
        pbl_rowblk_writer_finish(w, nullptr, 0);
      }
      pbl_rowblk_writer_reset(w, ri);
      T.n_blocks++;
      T.block_bytes += al;
      first = end;
    };
    pbl_rowblk_writer_reset(w, ri);
    bool prev_obs = false;
    for (uint64_t j = 0; j < k1 - k0; j++) {
      const uint8_t* key = kb + ko[j];
      const uint64_t kl = ko[j + 1] - ko[j], vl = vo[j + 1] - vo[j];
      const uint64_t tr = D.trailer[k0 + j];
      const uint32_t kind = uint32_t(tr & 0xff);
      bool set_same = false, obs = false;
      int64_t max_shared = int64_t(kl);
      const bool addp = vp && kind == kSet;
      if (vp) {
        max_shared = 0;  // lastPointKeyInfo.prefixLen of a fresh writer
        if (j) {
          const uint8_t* pkey = kb + ko[j - 1];
          const uint64_t pl = ko[j] - ko[j - 1];
          const uint32_t pk = uint32_t(D.trailer[k0 + j - 1] & 0xff);
          const uint64_t sp = cmp::key_split<R>(cmpr, pkey, pl), sc = cmp::key_split<R>(cmpr, key, kl);
          max_shared = int64_t(sp);
          set_same = kind == kSet && pk == kSet && cmp::key_cmp<R>(cmpr, pkey, sp, key, sc) == 0;
          const bool same_user = cmp::key_cmp<R>(cmpr, pkey, pl, key, kl) == 0;
          obs = (same_user && (prev_obs || pk != kMerge)) || (lowest && tombstone(kind));
        }
        obs = ob && (obs || (D.kv_flags && (D.kv_flags[k0 + j] & PBL_KV_OBSOLETE)));
      }
      prev_obs = obs;
      const uint64_t ikl = kl + 8, svl = vl + (addp ? 1 : 0);
      const uint64_t cnt = pbl_rowblk_writer_entry_count(w), est = pbl_rowblk_writer_estimated_size(w);
      if (cnt && est >= low) {  // shouldFlush
        uint64_t ns = est + ikl + svl + (cnt % uint64_t(ri) == 0 ? 4 : 0) + 4 + uvarint_len(ikl) + uvarint_len(svl);
        if (ns > high) flush(k0 + j);
      }
      pbl_rowblk_writer_add(w, key, kl, tr, obs ? 1 : 0, vb + vo[j], vl, max_shared, addp ? 1 : 0,
                            set_same ? 0x20 : 0x00, set_same ? 1 : 0);
      if (out->obsolete) out->obsolete[k0 + j] = obs ? 1 : 0;
    }
    if (pbl_rowblk_writer_entry_count(w)) flush(k1);
  }
  pbl_rowblk_writer_free(w);
  out->stream_block_base[nb] = T.n_blocks;
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *out->totals = T;
  return PBL_OK;
}

}  // namespace rowenc
}  // namespace pbl

extern "C" {

uint64_t pbl_rowenc_workspace_bytes(uint32_t n_streams, uint64_t n_kv) {
  return pbl::rowenc::layout(n_streams, n_kv).size;
}

int pbl_rowenc_size(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out, void* workspace,
                    uint64_t workspace_bytes, void* stream) {
  return pbl::rowenc::launch(in, opts, out, workspace, workspace_bytes, 0, true, reinterpret_cast<hipStream_t>(stream));
}

int pbl_rowenc_batch(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out, void* workspace,
                     uint64_t workspace_bytes, uint32_t flags, void* stream) {
  return pbl::rowenc::launch(in, opts, out, workspace, workspace_bytes, flags, false,
                             reinterpret_cast<hipStream_t>(stream));
}

int pbl_rowenc_batch_host(const pbl_rowenc_in* in, const pbl_rowenc_opts* opts, pbl_rowenc_out* out) {
  return pbl::rowenc::batch_host(in, opts, out);
}

size_t pbl_rowenc_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_rowenc_opts), PBL_OFF(pbl_rowenc_opts, restart_interval), PBL_OFF(pbl_rowenc_opts, target_block_size),
      PBL_OFF(pbl_rowenc_opts, block_size_threshold), PBL_OFF(pbl_rowenc_opts, comparer), PBL_OFF(pbl_rowenc_opts, flags),
      PBL_OFF(pbl_rowenc_opts, reserved),
      sizeof(pbl_rowenc_in), PBL_OFF(pbl_rowenc_in, batch), PBL_OFF(pbl_rowenc_in, n_streams),
      PBL_OFF(pbl_rowenc_in, reserved), PBL_OFF(pbl_rowenc_in, n_kv),
      sizeof(pbl_rowenc_totals), PBL_OFF(pbl_rowenc_totals, n_blocks), PBL_OFF(pbl_rowenc_totals, block_bytes),
      PBL_OFF(pbl_rowenc_totals, n_restarts), PBL_OFF(pbl_rowenc_totals, status_mask),
      PBL_OFF(pbl_rowenc_totals, n_bad_streams),
      sizeof(pbl_rowenc_out), PBL_OFF(pbl_rowenc_out, blocks), PBL_OFF(pbl_rowenc_out, block_off),
      PBL_OFF(pbl_rowenc_out, block_len), PBL_OFF(pbl_rowenc_out, block_stream), PBL_OFF(pbl_rowenc_out, block_first_kv),
      PBL_OFF(pbl_rowenc_out, block_n_kv), PBL_OFF(pbl_rowenc_out, stream_block_base),
      PBL_OFF(pbl_rowenc_out, stream_status), PBL_OFF(pbl_rowenc_out, obsolete), PBL_OFF(pbl_rowenc_out, totals),
      PBL_OFF(pbl_rowenc_out, blocks_cap), PBL_OFF(pbl_rowenc_out, block_cap)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
