// keyspan.hip — gfx950 decode of columnar keyspan blocks (DESIGN.md §3.15;
// include/pebble_amd.h states the rules): the block a columnar table keeps its
// range deletions (and range keys) in, decoded into a RUN as §3.14 defines it.
//
// Restates (cockroachdb/pebble, paths relative to the repo root):
//   KeyspanDecoder.Init                  sstable/colblk/keyspan.go:234-248
//   keyspanIter.First / Next             keyspan.go:478-508
//   gatherKeysForward / isNonemptySpan   keyspan.go:524-543, :572-574
//   materializeSpan                      keyspan.go:578-604
//   header / DecodeColumn / Uint / RawBytes   as colblk_block.hip.h lists them
//
// A batch is a handful of blocks (one per table) and a block may hold tens of
// thousands of fragments, so the parallelism comes from inside a block.  Every
// key's span is found by a search and every byte's place has a closed form:
//
//   keyspan_describe_kernel  wave per block: header, column directory and the
//       five columns (Dir::column, dec_rawbytes, dec_uints) into a descriptor in
//       the workspace; idx[B-1] <= R; n_kv = idx[B-1] - idx[0]; the block's
//       spans and span tiles.  It also clears the totals and the workspace's
//       sums and flags, so that an entry point launches kernels only
//   keyspan_layout_kernel  one workgroup: the exclusive scans of spans and span
//       tiles over blocks (result::tile_scan_inplace); a block whose spans end
//       past the workspace's boundaries is PBL_INVALID_ARG
//   keyspan_spans_kernel  workgroup per tile of 256 spans of one block, lane per
//       span: boundary offsets and idx ascending, the gap rules, nk = idx[s+1] -
//       idx[s], key bytes nk * len(boundary[s]), value bytes nk *
//       len(boundary[s+1]); the in-tile prefixes (16 B per boundary) and the
//       tile's sums.  Then, striding over the grid: the suffix and value offsets
//       of the key rows that are output ascend
//   keyspan_sizes_kernel  one workgroup: the scan over the tile sums; per block
//       the status and the five sizes (KVs, key, value, suffix, value-column bytes)
//   keyspan_sum_kernel / keyspan_bases_kernel  result::chunk_sums / bases: the
//       result's bases, statuses, totals, the capacity check
//   keyspan_emit_kernel  lane per KV over tiles of 256 KVs: the block by a search
//       over the result's KV bases, the span by an upper-bound search over idx[]
//       (u_at), trailer, entry_off, offsets; the boundary bytes 8 lanes per KV in
//       16-B chunks; the last offsets; with the extra output the span, the suffix
//       and value offsets rebased, and the two columns' bytes as ranged copies
//
// Typed global pointers throughout, no LDS beyond the scans' four words, no
// scratch.  Every byte is written by a vector store.
//
// The host form uses another algorithm on purpose: the reference's sequential
// walk, one span after the other (gatherKeysForward / materializeSpan), over
// host arrays, with a host restatement of the column decoders.
#include <algorithm>
#include <vector>

#include "colblk_block.hip.h"
#include "result_core.hip.h"

namespace pbl {
namespace keyspan {

using col::Dir;
using col::Src;
using col::UCol;
using col::u_at;

constexpr int kTPB = 256;
constexpr uint32_t kTileShift = 8;
static_assert(kTPB == result::kTPB && (1u << kTileShift) == uint32_t(kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kGrid = 2048;
constexpr uint64_t kHdr = 64;
constexpr uint32_t kCustom = 4;  // keyspanHeaderSize
constexpr uint32_t kCols = 5;
constexpr uint64_t kMaxBytes = 0xffffffffull;
constexpr int kC = 5;  // per-block sizes: KVs, key bytes, value bytes, suffix bytes, value-column bytes
enum { kHSkip = 0 };
constexpr uint32_t kBadBounds = 1;

struct Desc {
  UCol boff, idx, trl, soff, voff;  // boundary offsets, idx[], trailers, suffix offsets, value offsets
  uint32_t status, B, R;
  uint32_t bdata, sdata, vdata;  // data starts of the three RawBytes columns
  uint32_t idx0, n_kv;           // the first key row that is output, and how many are
  uint32_t s_lo, v_lo;           // soff[idx0], voff[idx0]
  uint32_t s_len, v_len;         // suffix / value-column bytes of the rows that are output
};
constexpr int kDescWords = sizeof(Desc) / 8;
static_assert(sizeof(Desc) % 8 == 0, "descriptors are stored back to back as 8-byte words");
// A descriptor to and from the workspace as typed global words (the address is
// the same in every lane of a wave).
__device__ __forceinline__ Desc load_desc(gptr<const Desc> p) {
  const gptr<const uint64_t> w = (gptr<const uint64_t>)p;
  uint64_t x[kDescWords];
#pragma unroll
  for (int i = 0; i < kDescWords; i++) x[i] = w[i];
  Desc d;
  __builtin_memcpy(&d, x, sizeof(Desc));
  return d;
}
__device__ __forceinline__ void store_desc(gptr<Desc> p, const Desc& d) {
  const gptr<uint64_t> w = (gptr<uint64_t>)p;
  uint64_t x[kDescWords];
  __builtin_memcpy(x, &d, sizeof(Desc));
#pragma unroll
  for (int i = 0; i < kDescWords; i++) w[i] = x[i];
}

struct Layout {
  uint64_t cap_b, nt_cap;  // boundaries and span tiles the workspace holds
  uint32_t n_chunks;
  uint64_t desc, bad, sbase, tbase, q64, csum, qst, tsum, pre, size;
};
__host__ __device__ inline Layout layout(uint32_t nb, uint64_t total_boundaries) {
  Layout L;
  L.cap_b = total_boundaries;
  L.nt_cap = (total_boundaries >> kTileShift) + nb;
  L.n_chunks = nb ? (nb + kTPB - 1) / kTPB : 1;
  uint64_t o = kHdr;
  L.desc = o;  o += sizeof(Desc) * uint64_t(nb);
  L.sbase = o; o += 8ull * (uint64_t(nb) + 1);
  L.tbase = o; o += 8ull * (uint64_t(nb) + 1);
  L.q64 = o;   o += 8ull * kC * nb;
  L.csum = o;  o += 8ull * kC * L.n_chunks;
  L.tsum = o;  o += 2ull * 8 * (L.nt_cap + 1);
  L.pre = o;   o += 16ull * total_boundaries;
  L.bad = o;   o += 4ull * nb;
  L.qst = o;   o += 4ull * nb;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

struct Args {
  pbl_block_batch in;
  pbl_decode_out out;
  pbl_keyspan_extra ex;
  uint8_t* ws;
  uint64_t total_boundaries;
  uint32_t has_extra, size_only;
};

struct Ws {
  gptr<uint32_t> hdr, bad, qst;
  gptr<uint64_t> sbase, tbase, q64, csum, tsum[2], pre;
  gptr<Desc> desc;
  uint64_t cap_b, nt_cap, qs;
  uint32_t n_chunks;
  __device__ Ws(const Args& A) {
    const Layout L = layout(A.in.n_blocks, A.total_boundaries);
    uint8_t* ws = A.ws;
    hdr = to_glb(reinterpret_cast<uint32_t*>(ws));
    desc = to_glb(reinterpret_cast<Desc*>(ws + L.desc));
    bad = to_glb(reinterpret_cast<uint32_t*>(ws + L.bad));
    qst = to_glb(reinterpret_cast<uint32_t*>(ws + L.qst));
    sbase = to_glb(reinterpret_cast<uint64_t*>(ws + L.sbase));
    tbase = to_glb(reinterpret_cast<uint64_t*>(ws + L.tbase));
    q64 = to_glb(reinterpret_cast<uint64_t*>(ws + L.q64));
    csum = to_glb(reinterpret_cast<uint64_t*>(ws + L.csum));
    tsum[0] = to_glb(reinterpret_cast<uint64_t*>(ws + L.tsum));
    tsum[1] = tsum[0] + (L.nt_cap + 1);
    pre = to_glb(reinterpret_cast<uint64_t*>(ws + L.pre));
    cap_b = L.cap_b;
    nt_cap = L.nt_cap;
    qs = A.in.n_blocks;
    n_chunks = L.n_chunks;
  }
  __device__ result::Sizes sizes() const { return result::Sizes{q64, csum, qst, qs, n_chunks}; }
  __device__ gptr<uint64_t> q(int c) const { return q64 + uint64_t(c) * qs; }
};

__device__ inline Src block_src(const pbl_block_batch& B, uint32_t b, col::lds_cu8 dummy) {
  return Src{dummy, dummy, (col::glb_cu8)(B.blocks + to_glb(B.block_off)[b]), 0u, to_glb(B.block_len)[b],
             to_glb(B.block_len)[b]};
}

// Offset i of a RawBytes column (its offsets have base 0).
__device__ __forceinline__ uint32_t off_at(const Src& S, const UCol& o, uint32_t i) {
  return o.w ? uint32_t(S.le(o.at + i * o.w, o.w)) : 0u;
}

// KeyspanDecoder.Init: every DecodeColumn check, then the two ends of idx[].
__device__ inline uint32_t describe(const Src& S, Desc* D) {
  D->B = D->R = D->idx0 = D->n_kv = D->s_lo = D->v_lo = D->s_len = D->v_len = 0;
  if (S.len < kCustom + 7) return PBL_CORRUPT_COLBLK_HEADER;
  const uint32_t B = uint32_t(S.le_u(0, 4));
  Dir dir;
  dir.custom = kCustom;
  dir.ncols = uint32_t(S.le_u(kCustom + 1, 2));
  const uint32_t R = uint32_t(S.le_u(kCustom + 3, 4));
  if (dir.ncols != kCols) return PBL_CORRUPT_COLBLK_HEADER;
  uint64_t s, nx, e;
  if (!dir.column(S, 0, col::kDtBytes, &s, &nx) || !col::dec_rawbytes(S, s, B, &D->boff, &D->bdata, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!dir.column(S, 1, col::kDtUint, &s, &nx) || !col::dec_uints(S, s, B, &D->idx, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!dir.column(S, 2, col::kDtUint, &s, &nx) || !col::dec_uints(S, s, R, &D->trl, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!dir.column(S, 3, col::kDtBytes, &s, &nx) || !col::dec_rawbytes(S, s, R, &D->soff, &D->sdata, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!dir.column(S, 4, col::kDtBytes, &s, &nx) || !col::dec_rawbytes(S, s, R, &D->voff, &D->vdata, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  D->B = B;
  D->R = R;
  if (B < 2) return PBL_OK;
  // (a block of len bytes holds fewer than len spans that are not empty: more
  // boundaries than bytes means a constant idx[], whose last span is empty)
  if (B > S.len) return PBL_CORRUPT_BOUNDS;
  const uint64_t i0 = u_at<false>(S, D->idx, 0), iN = u_at<false>(S, D->idx, B - 1);
  if (iN > R || i0 > iN) return PBL_CORRUPT_BOUNDS;
  D->idx0 = uint32_t(i0);
  D->n_kv = uint32_t(iN - i0);
  const uint32_t s0 = off_at(S, D->soff, uint32_t(i0)), s1 = off_at(S, D->soff, uint32_t(iN));
  const uint32_t v0 = off_at(S, D->voff, uint32_t(i0)), v1 = off_at(S, D->voff, uint32_t(iN));
  // the last slice that is output ends inside its column (dec_rawbytes bounds
  // only the column's last offset, that of row R, and idx[B-1] may be below R)
  if (s0 > s1 || v0 > v1 || s1 > off_at(S, D->soff, R) || v1 > off_at(S, D->voff, R)) return PBL_CORRUPT_BOUNDS;
  D->s_lo = s0;
  D->v_lo = v0;
  D->s_len = s1 - s0;
  D->v_len = v1 - v0;
  return PBL_OK;
}

// Wave per block.  Every lane parses (the reads are the same in all of them);
// lane 0 writes the descriptor, the block's spans and its span tiles.
__global__ __launch_bounds__(kTPB) void keyspan_describe_kernel(Args A) {
  __shared__ uint8_t dummy[16];
  const Ws W(A);
  const uint32_t nb = A.in.n_blocks, wpb = kTPB / kWave;
  // what a memset would clear, without its launches: the tile sums (a tile
  // nobody sums adds nothing), the header word, the totals, the bad flags
  const uint64_t gtid = uint64_t(blockIdx.x) * kTPB + threadIdx.x, gsize = uint64_t(gridDim.x) * kTPB;
  for (uint64_t i = gtid; i < 2 * (W.nt_cap + 1); i += gsize) W.tsum[0][i] = 0;
  if (gtid == 0) {
    W.hdr[kHSkip] = 0;
    const gptr<pbl_totals> T = to_glb(A.out.totals);
    T->n_kv = T->key_bytes = T->val_bytes = T->n_restarts = 0;
    T->status_mask = T->n_bad_blocks = T->n_slow_blocks = T->pad = 0;
  }
  for (uint32_t b = blockIdx.x * wpb + wave_id(); b < nb; b += gridDim.x * wpb) {
    const Src S = block_src(A.in, b, (col::lds_cu8)col::to_lds(dummy));
    Desc D{};
    D.status = describe(S, &D);
    if (lane_id() != 0) continue;
    const uint64_t nsp = (D.status == PBL_OK && D.B >= 2) ? D.B - 1 : 0;
    store_desc(W.desc + b, D);
    W.bad[b] = 0;
    W.sbase[b] = nsp;
    W.tbase[b] = (nsp + kTPB - 1) >> kTileShift;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) W.sbase[nb] = W.tbase[nb] = 0;
}

// One workgroup: spans and span tiles before every block.
__global__ __launch_bounds__(kTPB) void keyspan_layout_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A);
  const uint32_t nb = A.in.n_blocks;
  const gptr<uint64_t> a[2] = {W.sbase, W.tbase};
  result::tile_scan_inplace<2>(a, uint64_t(nb) + 1, lds);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += kTPB)
    if (W.sbase[b + 1] > W.cap_b && W.desc[b].status == PBL_OK) W.desc[b].status = PBL_INVALID_ARG;
}

// The block that owns span tile t: the last b with tbase[b] <= t.
__device__ inline uint32_t block_of_tile(const Ws& W, uint32_t nb, uint64_t t) {
  return result::block_of((gptr<const uint64_t>)W.tbase, nb, t);
}

__global__ __launch_bounds__(kTPB) void keyspan_spans_kernel(Args A) {
  __shared__ uint64_t lds[4];
  __shared__ uint8_t dummy[16];
  const Ws W(A);
  const uint32_t nb = A.in.n_blocks;
  const uint64_t nt = W.tbase[nb];
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    const uint32_t b = block_of_tile(W, nb, t);
    if (W.desc[b].status != PBL_OK || t >= W.nt_cap) continue;  // (uniform over the workgroup)
    const Desc D = load_desc(W.desc + b);
    const Src S = block_src(A.in, b, (col::lds_cu8)col::to_lds(dummy));
    const UCol boff = D.boff, idx = D.idx;
    const uint32_t B = D.B;
    const uint64_t s = ((t - W.tbase[b]) << kTileShift) + threadIdx.x;
    uint64_t kb = 0, vb = 0;
    bool bad = false;
    if (s + 1 < B) {
      const uint32_t si = uint32_t(s);
      const uint32_t o0 = off_at(S, boff, si), o1 = off_at(S, boff, si + 1), o2 = off_at(S, boff, si + 2);
      const uint64_t i0 = u_at<false>(S, idx, si), i1 = u_at<false>(S, idx, si + 1);
      bad = o0 > o1 || o1 > o2 || i0 > i1;
      if (!bad && i0 == i1) {
        // a gap: not the last span, and the next one holds keys
        bad = si + 2 >= B || u_at<false>(S, idx, si + 2) <= i1;
      }
      if (!bad) {
        const uint64_t nk = i1 - i0;
        kb = nk * (o1 - o0);
        vb = nk * (o2 - o1);
      }
    }
    if (__syncthreads_or(bad)) {
      if (threadIdx.x == 0) g_atomic_or((uint32_t*)(W.bad + b), kBadBounds);
      continue;
    }
    uint64_t tk, tv;
    const uint64_t pk = result::block_excl_scan64(kb, lds, &tk), pv = result::block_excl_scan64(vb, lds, &tv);
    if (s + 1 < B) {
      const uint64_t g = W.sbase[b] + s;
      W.pre[2 * g] = pk;
      W.pre[2 * g + 1] = pv;
    }
    if (threadIdx.x == 0) {
      W.tsum[0][t] = tk;
      W.tsum[1][t] = tv;
    }
  }
  // the suffix and value slices of the key rows that are output: ascending
  // (their ends are inside the columns: dec_rawbytes)
  const uint64_t gtid = uint64_t(blockIdx.x) * kTPB + threadIdx.x, gsize = uint64_t(gridDim.x) * kTPB;
  for (uint32_t b = 0; b < nb; b++) {
    if (W.desc[b].status != PBL_OK || W.desc[b].n_kv == 0) continue;
    const Desc D = load_desc(W.desc + b);
    const Src S = block_src(A.in, b, (col::lds_cu8)col::to_lds(dummy));
    const UCol soff = D.soff, voff = D.voff;
    const uint32_t r0 = D.idx0, n = D.n_kv;
    bool bad = false;
    for (uint64_t r = gtid; r < n; r += gsize) {
      const uint32_t j = r0 + uint32_t(r);
      bad |= off_at(S, soff, j) > off_at(S, soff, j + 1) || off_at(S, voff, j) > off_at(S, voff, j + 1);
    }
    if (bad) g_atomic_or((uint32_t*)(W.bad + b), kBadBounds);
  }
}

// One workgroup: the scan over the tile sums, then every block's status and sizes.
__global__ __launch_bounds__(kTPB) void keyspan_sizes_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A);
  const uint32_t nb = A.in.n_blocks;
  const uint64_t nt_all = W.tbase[nb], nt = nt_all < W.nt_cap ? nt_all : W.nt_cap;
  const gptr<uint64_t> a[2] = {W.tsum[0], W.tsum[1]};
  result::tile_scan_inplace<2>(a, nt + 1, lds);  // (entry nt: zero before, the totals after)
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += kTPB) {
    const gptr<const Desc> D = W.desc + b;
    uint32_t st = D->status;
    if (st == PBL_OK && W.bad[b]) st = PBL_CORRUPT_BOUNDS;
    uint64_t k = 0, v = 0;
    if (st == PBL_OK && D->n_kv) {
      const uint64_t t0 = W.tbase[b], t1 = W.tbase[b + 1];
      k = W.tsum[0][t1] - W.tsum[0][t0];
      v = W.tsum[1][t1] - W.tsum[1][t0];
      if (k > kMaxBytes || v > kMaxBytes) st = PBL_UNSUPPORTED;
    }
    const bool ok = st == PBL_OK;
    W.q(0)[b] = ok ? D->n_kv : 0;
    W.q(1)[b] = ok ? k : 0;
    W.q(2)[b] = ok ? v : 0;
    W.q(3)[b] = ok ? D->s_len : 0;
    W.q(4)[b] = ok ? D->v_len : 0;
    W.qst[b] = st;
  }
}

__global__ __launch_bounds__(kTPB) void keyspan_sum_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A);
  result::chunk_sums<kC>(W.sizes(), A.in.n_blocks, lds);
}

// The result's bases, statuses and totals; the extra output's bases; the
// capacity check (the last chunk).  Totals were zeroed by the describe kernel.
__global__ __launch_bounds__(kTPB) void keyspan_bases_kernel(Args A) {
  __shared__ uint64_t lds[4];
  const Ws W(A);
  const uint32_t nb = A.in.n_blocks;
  uint64_t ex[kC], end[kC];
  bool over;
  const bool last = result::bases<kC>(W.sizes(), A.out, nb, A.size_only != 0, lds, ex, end, &over);
  const uint64_t i = uint64_t(blockIdx.x) * kTPB + threadIdx.x;
  if (A.has_extra && i < nb) {
    to_glb(A.ex.blk_suffix_base)[i] = ex[3];
    to_glb(A.ex.blk_value_base)[i] = ex[4];
  }
  if (!last) return;
  if (A.has_extra) {
    to_glb(A.ex.blk_suffix_base)[nb] = end[3];
    to_glb(A.ex.blk_value_base)[nb] = end[4];
    if (!A.size_only && (end[3] > A.ex.suffix_cap || end[4] > A.ex.value_cap)) {
      over = true;
      g_atomic_or(&A.out.totals->status_mask, 1u << PBL_OVERFLOW);
    }
  }
  W.hdr[kHSkip] = (over || A.size_only) ? 1u : 0u;
}

// dst[0, n) = src[0, n), n <= 16, without reading past the 16-byte granule that
// holds src[n - 1] (a block is readable up to the next 16-byte boundary only).
__device__ __forceinline__ void copy_tail(gptr<uint8_t> dst, gptr<const uint8_t> src, uint32_t n) {
  if (n == 0) return;
  if (n >= 16) {
    *(gptr<u32x4_u>)dst = *(gptr<const u32x4_u>)src;
    return;
  }
  const uint64_t a = reinterpret_cast<uint64_t>(src);
  const uint32_t sh = uint32_t(a & 15);
  const gptr<const u32x4> p = (gptr<const u32x4>)(a & ~uint64_t(15));
  const u32x4 x = p[0];
  const u32x4 y = sh + n > 16 ? p[1] : x;
  const uint4 w = funnel16(make_uint4(x.x, x.y, x.z, x.w), make_uint4(y.x, y.y, y.z, y.w), sh);
  uint64_t lo = uint64_t(w.x) | uint64_t(w.y) << 32, hi = uint64_t(w.z) | uint64_t(w.w) << 32;
  uint32_t o = 0;
  if (n & 8) {
    *(gptr<u64_u>)(dst + o) = lo;
    lo = hi;
    o += 8;
  }
  if (n & 4) {
    *(gptr<u32_u>)(dst + o) = uint32_t(lo);
    lo >>= 32;
    o += 4;
  }
  if (n & 2) {
    *(gptr<u16_u>)(dst + o) = uint16_t(lo);
    lo >>= 16;
    o += 2;
  }
  if (n & 1) dst[o] = uint8_t(lo);
}

// The whole wave copies its lanes' slices, as result::copy_values does: 8 lanes
// per slice of at most 512 B (lane c of a group copies the 16-B chunks c, c + 8,
// ...), longer ones by the whole wave.  Every lane of the wave calls it.
__device__ __forceinline__ void copy_slices(bool ok, uint32_t len, gptr<const uint8_t> src, gptr<uint8_t> dst) {
  const uint32_t lane = lane_id();
#pragma unroll 1
  for (uint32_t u = 0; u < kWave / 8; u++) {
    const int sl = int(8 * u + (lane >> 3));
    const bool sv = __shfl(int(ok && len <= 512), sl, kWave) != 0;
    const gptr<const uint8_t> sp = (gptr<const uint8_t>)__shfl((unsigned long long)src, sl, kWave);
    const gptr<uint8_t> dp = (gptr<uint8_t>)__shfl((unsigned long long)dst, sl, kWave);
    const uint32_t sn = uint32_t(__shfl(int(len), sl, kWave));
    if (!sv) continue;
    for (uint32_t i = 16 * (lane & 7u); i < sn; i += 128) copy_tail(dp + i, sp + i, sn - i < 16 ? sn - i : 16u);
  }
  for (uint64_t m = __ballot(ok && len > 512); m; m &= m - 1) {
    const int src_lane = __builtin_ctzll(m);
    const gptr<const uint8_t> sp = (gptr<const uint8_t>)__shfl((unsigned long long)src, src_lane, kWave);
    const gptr<uint8_t> dp = (gptr<uint8_t>)__shfl((unsigned long long)dst, src_lane, kWave);
    const uint32_t sn = uint32_t(__shfl(int(len), src_lane, kWave));
    for (uint32_t i = 16 * lane; i < sn; i += 16 * kWave) copy_tail(dp + i, sp + i, sn - i < 16 ? sn - i : 16u);
  }
}

// The last s with idx[s] <= j over idx[0, B): j lies in [idx[0], idx[B-1]), so
// the answer is a span that holds keys (of equal idx the last one).
__device__ __forceinline__ uint32_t span_of(const Src& S, const UCol& idx, uint32_t B, uint64_t j) {
  uint32_t lo = 0, hi = B;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (u_at<false>(S, idx, m) <= j) lo = m + 1;
    else hi = m;
  }
  return lo ? lo - 1 : 0;
}

__global__ __launch_bounds__(kTPB) void keyspan_emit_kernel(Args A) {
  __shared__ uint8_t dummy[16];
  const Ws W(A);
  if (W.hdr[kHSkip] != 0) return;  // sizes only
  const pbl_decode_out& O = A.out;
  const uint32_t nb = A.in.n_blocks;
  const gptr<const uint64_t> kvb = to_glb((const uint64_t*)O.blk_kv_base), keyb = to_glb((const uint64_t*)O.blk_key_base),
                             valb = to_glb((const uint64_t*)O.blk_val_base);
  result::last_offsets(O, nb, O.kv_cap);
  const bool extra = A.has_extra != 0;
  const uint64_t gtid = uint64_t(blockIdx.x) * kTPB + threadIdx.x, gsize = uint64_t(gridDim.x) * kTPB;
  if (extra) {
    const gptr<const uint64_t> sb = to_glb((const uint64_t*)A.ex.blk_suffix_base), vb = to_glb((const uint64_t*)A.ex.blk_value_base);
    for (uint64_t q = gtid; q < nb; q += gsize) {
      const uint64_t at = kvb[q + 1] + q;
      to_glb(A.ex.suffix_off)[at] = uint32_t(sb[q + 1] - sb[q]);
      to_glb(A.ex.value_off)[at] = uint32_t(vb[q + 1] - vb[q]);
    }
  }
  const uint64_t n_kv = kvb[nb];
  const uint64_t n_tiles = (n_kv + kTPB - 1) >> kTileShift;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t i = (t << kTileShift) + threadIdx.x;
    bool ok = i < n_kv;
    uint32_t klen = 0, vlen = 0;
    gptr<const uint8_t> ksrc = nullptr, vsrc = nullptr;
    gptr<uint8_t> kdst = nullptr, vdst = nullptr;
    if (ok) {
      const uint32_t b = result::block_of(kvb, nb, i);
      const Desc D = load_desc(W.desc + b);
      const Src S = block_src(A.in, b, (col::lds_cu8)col::to_lds(dummy));
      const UCol idx = D.idx, boff = D.boff;
      const uint64_t kv0 = kvb[b];
      const uint32_t j = D.idx0 + uint32_t(i - kv0);  // the key row
      const uint32_t s = span_of(S, idx, D.B, j);
      const uint64_t is = u_at<false>(S, idx, s);
      const uint32_t o0 = off_at(S, boff, s), o1 = off_at(S, boff, s + 1), o2 = off_at(S, boff, s + 2);
      klen = o1 - o0;
      vlen = o2 - o1;
      const uint64_t t0 = W.tbase[b], ts = t0 + (s >> kTileShift), g = W.sbase[b] + s;
      const uint64_t kbase = W.tsum[0][ts] - W.tsum[0][t0] + W.pre[2 * g];
      const uint64_t vbase = W.tsum[1][ts] - W.tsum[1][t0] + W.pre[2 * g + 1];
      const uint64_t ko = kbase + (j - is) * uint64_t(klen), vo = vbase + (j - is) * uint64_t(vlen);
      uint64_t tr = u_at<false>(S, D.trl, j);
      if (A.in.synthetic_seq_num) tr = A.in.synthetic_seq_num << 8 | (tr & 0xff);
      to_glb(O.trailer)[i] = tr;
      if (O.kv_flags) to_glb(O.kv_flags)[i] = 0;
      if (O.entry_off) to_glb(O.entry_off)[i] = j;
      if (O.tiering_span_id) {
        to_glb(O.tiering_span_id)[i] = 0;
        to_glb(O.tiering_attr)[i] = 0;
      }
      to_glb(O.key_off)[i + b] = uint32_t(ko);
      to_glb(O.val_off)[i + b] = uint32_t(vo);
      if (extra) {
        to_glb(A.ex.span)[i] = s;
        to_glb(A.ex.suffix_off)[i + b] = off_at(S, D.soff, j) - D.s_lo;
        to_glb(A.ex.value_off)[i + b] = off_at(S, D.voff, j) - D.v_lo;
      }
      ksrc = S.g + D.bdata + o0;
      vsrc = S.g + D.bdata + o1;
      kdst = to_glb(O.key_bytes) + keyb[b] + ko;
      vdst = to_glb(O.val_bytes) + valb[b] + vo;
    }
    copy_slices(ok, klen, ksrc, kdst);
    copy_slices(ok, vlen, vsrc, vdst);
  }
  if (!extra) return;
  // the suffix and value columns of the rows that are output: contiguous in the block
  const uint32_t wpb = kTPB / kWave;
  const uint64_t gw = uint64_t(blockIdx.x) * wpb + wave_id(), nw = uint64_t(gridDim.x) * wpb;
  for (uint32_t b = 0; b < nb; b++) {
    if (kvb[b + 1] == kvb[b]) continue;
    const gptr<const Desc> D = W.desc + b;  // (scalar fields only)
    const Src S = block_src(A.in, b, (col::lds_cu8)col::to_lds(dummy));
    for (int c = 0; c < 2; c++) {
      const uint32_t n = c ? D->v_len : D->s_len;
      const gptr<const uint8_t> src = S.g + (c ? D->vdata + D->v_lo : D->sdata + D->s_lo);
      const gptr<uint8_t> dst = c ? to_glb(A.ex.value_bytes) + to_glb(A.ex.blk_value_base)[b]
                                  : to_glb(A.ex.suffix_bytes) + to_glb(A.ex.blk_suffix_base)[b];
      for (uint64_t o = (gw * kWave + lane_id()) * 16; o < n; o += nw * kWave * 16)
        copy_tail(dst + o, src + o, n - o < 16 ? uint32_t(n - o) : 16u);
    }
  }
}

// ---- host side -----------------------------------------------------------------
inline bool batch_ok(const pbl_block_batch* in) {
  return in && (in->n_blocks == 0 || (in->blocks && in->block_off && in->block_len)) &&
         in->synthetic_seq_num <= PBL_SEQNUM_MAX;
}
inline bool extra_ok(const pbl_keyspan_extra* x, bool size_only) {
  if (!x) return true;
  if (!x->blk_suffix_base || !x->blk_value_base) return false;
  if (size_only) return true;
  return x->span && x->suffix_off && x->value_off && x->suffix_bytes && x->value_bytes;
}

inline int launch(const pbl_block_batch* in, pbl_decode_out* out, pbl_keyspan_extra* extra, void* ws, uint64_t ws_bytes,
                  uint64_t total_boundaries, bool size_only, void* stream) {
  if (!batch_ok(in) || !out || !result::result_ok(*out, size_only) || !extra_ok(extra, size_only)) return PBL_INVALID_ARG;
  const uint32_t nb = in->n_blocks;
  const Layout L = layout(nb, total_boundaries);
  if (!result::ws_aligned(ws) || ws_bytes < L.size) return PBL_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Args a{};
  a.in = *in;
  a.out = *out;
  if (extra) a.ex = *extra;
  a.has_extra = extra ? 1u : 0u;
  a.size_only = (size_only || !out->key_off) ? 1u : 0u;
  a.ws = static_cast<uint8_t*>(ws);
  a.total_boundaries = total_boundaries;
  // (no memset: the describe kernel clears the totals and what the workspace needs cleared)
  const uint32_t wpb = kTPB / kWave;
  const uint64_t clear_wgs = (2 * (L.nt_cap + 1) + 8 * kTPB - 1) / (8 * kTPB);
  const uint32_t b_grid =
      uint32_t(std::min<uint64_t>(std::max<uint64_t>(std::max<uint64_t>((uint64_t(nb) + wpb - 1) / wpb, clear_wgs), 1), kGrid));
  const uint32_t t_grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>(L.nt_cap, 1), kGrid));
  hipLaunchKernelGGL(keyspan_describe_kernel, dim3(b_grid), dim3(kTPB), 0, st, a);
  hipLaunchKernelGGL(keyspan_layout_kernel, dim3(1), dim3(kTPB), 0, st, a);
  if (nb) hipLaunchKernelGGL(keyspan_spans_kernel, dim3(t_grid), dim3(kTPB), 0, st, a);
  hipLaunchKernelGGL(keyspan_sizes_kernel, dim3(1), dim3(kTPB), 0, st, a);
  if (L.n_chunks > 1) hipLaunchKernelGGL(keyspan_sum_kernel, dim3(L.n_chunks), dim3(kTPB), 0, st, a);
  hipLaunchKernelGGL(keyspan_bases_kernel, dim3(L.n_chunks), dim3(kTPB), 0, st, a);
  if (!a.size_only && nb) {
    // a lane per KV: the KV count is on the device, bounded by the capacity
    const uint64_t tiles = std::max<uint64_t>((out->kv_cap + kTPB - 1) >> kTileShift, (uint64_t(nb) + kTPB - 1) / kTPB);
    const uint32_t e_grid = uint32_t(std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kGrid));
    hipLaunchKernelGGL(keyspan_emit_kernel, dim3(e_grid), dim3(kTPB), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

// ---- the host form: a host restatement of the column decoders, then the
// reference's walk span by span -----------------------------------------------
struct HCol {
  uint64_t base = 0;
  uint64_t at = 0;
  uint32_t w = 0;
};
struct HBlock {
  const uint8_t* p;
  uint64_t len;
  uint64_t le(uint64_t o, uint32_t w) const {
    uint64_t v = 0;
    for (uint32_t i = 0; i < w; i++) v |= uint64_t(p[o + i]) << (8 * i);
    return v;
  }
  uint64_t at(const HCol& c, uint64_t i) const { return c.w ? c.base + le(c.at + i * c.w, c.w) : c.base; }
};
inline bool h_uints(const HBlock& S, uint64_t off, uint64_t rows, HCol* u, uint64_t* end) {
  *u = HCol{};
  u->at = off;
  if (rows == 0) {
    *end = off;
    return true;
  }
  if (off >= S.len) return false;
  const uint32_t e = S.p[off++], w = e & 0x7f;
  const bool delta = (e & 0x80) != 0;
  if (!(w == 0 || w == 1 || w == 2 || w == 4 || (w == 8 && !delta))) return false;
  if (delta) {
    if (off + 8 > S.len) return false;
    u->base = S.le(off, 8);
    off += 8;
  }
  if (w) off = (off + w - 1) / w * w;
  u->w = w;
  u->at = off;
  *end = off + rows * w;
  return true;
}
inline bool h_rawbytes(const HBlock& S, uint64_t off, uint64_t count, HCol* o, uint64_t* data, uint64_t* end) {
  *data = 0;
  if (count == 0) {
    *o = HCol{};
    o->at = off;
    *end = off;
    return true;
  }
  uint64_t dend;
  if (!h_uints(S, off, count + 1, o, &dend)) return false;
  if (o->base != 0 || o->w == 8 || dend > S.len) return false;
  *data = dend;
  *end = dend + (o->w ? S.le(o->at + count * o->w, o->w) : 0);
  return *end <= S.len;
}
inline bool h_column(const HBlock& S, uint32_t ncols, uint32_t c, uint32_t type, uint64_t* start, uint64_t* next) {
  if (c >= ncols) return false;
  const uint64_t h = kCustom + 7 + 5ull * c;
  if (h + 5 > S.len || S.p[h] != type) return false;
  *start = S.le(h + 1, 4);
  if (c + 1 >= ncols) *next = S.len - 1;
  else {
    if (h + 10 > S.len) return false;
    *next = S.le(h + 6, 4);
  }
  return *next <= S.len && *start <= *next;
}

struct HKv {
  uint32_t span, row;
};
struct HDesc {
  HCol boff, idx, trl, soff, voff;
  uint64_t bdata, sdata, vdata;
  uint32_t B, R;
};

// The walk: First(), Next()... collecting (span, key row) pairs; then what the
// reference finds lazily, for the whole block.
inline uint32_t host_walk(const HBlock& S, HDesc* D, std::vector<HKv>* kvs) {
  kvs->clear();
  if (S.len < kCustom + 7) return PBL_CORRUPT_COLBLK_HEADER;
  const uint32_t B = uint32_t(S.le(0, 4)), ncols = uint32_t(S.le(kCustom + 1, 2)), R = uint32_t(S.le(kCustom + 3, 4));
  if (ncols != kCols) return PBL_CORRUPT_COLBLK_HEADER;
  uint64_t s, nx, e;
  if (!h_column(S, ncols, 0, col::kDtBytes, &s, &nx) || !h_rawbytes(S, s, B, &D->boff, &D->bdata, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!h_column(S, ncols, 1, col::kDtUint, &s, &nx) || !h_uints(S, s, B, &D->idx, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!h_column(S, ncols, 2, col::kDtUint, &s, &nx) || !h_uints(S, s, R, &D->trl, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!h_column(S, ncols, 3, col::kDtBytes, &s, &nx) || !h_rawbytes(S, s, R, &D->soff, &D->sdata, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  if (!h_column(S, ncols, 4, col::kDtBytes, &s, &nx) || !h_rawbytes(S, s, R, &D->voff, &D->vdata, &e) || e != nx)
    return PBL_CORRUPT_COLBLK_HEADER;
  D->B = B;
  D->R = R;
  if (B < 2) return PBL_OK;
  if (B > S.len) return PBL_CORRUPT_BOUNDS;
  // the whole block: idx[] and the boundary offsets ascend, idx[B-1] <= R
  for (uint32_t i = 0; i + 1 < B; i++)
    if (S.at(D->idx, i) > S.at(D->idx, i + 1)) return PBL_CORRUPT_BOUNDS;
  const uint64_t iN = S.at(D->idx, B - 1);
  if (iN > R) return PBL_CORRUPT_BOUNDS;
  // (the columns' last offsets, those of row R, are inside: h_rawbytes)
  if (S.at(D->soff, iN) > S.at(D->soff, R) || S.at(D->voff, iN) > S.at(D->voff, R)) return PBL_CORRUPT_BOUNDS;
  for (uint32_t i = 0; i < B; i++)
    if (S.at(D->boff, i) > S.at(D->boff, i + 1)) return PBL_CORRUPT_BOUNDS;
  // gatherKeysForward from First()
  for (int64_t start = 0; start < int64_t(B) - 1; start++) {
    auto nonempty = [&](int64_t x) { return S.at(D->idx, uint64_t(x)) < S.at(D->idx, uint64_t(x) + 1); };
    if (!nonempty(start)) {
      if (start == int64_t(B) - 2) return PBL_CORRUPT_BOUNDS;  // "empty span at end"
      start++;
      if (!nonempty(start)) return PBL_CORRUPT_BOUNDS;  // "consecutive empty spans"
    }
    // materializeSpan
    for (uint64_t j = S.at(D->idx, uint64_t(start)); j < S.at(D->idx, uint64_t(start) + 1); j++) {
      if (S.at(D->soff, j) > S.at(D->soff, j + 1) || S.at(D->voff, j) > S.at(D->voff, j + 1)) return PBL_CORRUPT_BOUNDS;
      kvs->push_back(HKv{uint32_t(start), uint32_t(j)});
    }
  }
  return PBL_OK;
}

}  // namespace keyspan
}  // namespace pbl

extern "C" {

uint64_t pbl_keyspan_workspace_bytes(uint32_t n_blocks, uint64_t total_boundaries) {
  return pbl::keyspan::layout(n_blocks, total_boundaries).size;
}

int pbl_keyspan_size(const pbl_block_batch* batch, uint64_t total_boundaries, pbl_decode_out* out,
                     pbl_keyspan_extra* extra, void* workspace, uint64_t workspace_bytes, void* stream) {
  return pbl::keyspan::launch(batch, out, extra, workspace, workspace_bytes, total_boundaries, true, stream);
}

int pbl_keyspan_decode(const pbl_block_batch* batch, uint64_t total_boundaries, pbl_decode_out* out,
                       pbl_keyspan_extra* extra, void* workspace, uint64_t workspace_bytes, void* stream) {
  return pbl::keyspan::launch(batch, out, extra, workspace, workspace_bytes, total_boundaries, false, stream);
}

int pbl_keyspan_decode_host(const pbl_block_batch* batch, pbl_decode_out* out, pbl_keyspan_extra* extra) {
  namespace M = pbl::keyspan;
  if (!M::batch_ok(batch) || !out || !pbl::result::result_ok(*out, false) || !M::extra_ok(extra, !out->key_off))
    return PBL_INVALID_ARG;
  const pbl_decode_out& O = *out;
  const uint32_t nb = batch->n_blocks;
  std::vector<std::vector<M::HKv>> kvs(nb);
  std::vector<M::HDesc> desc(nb);
  std::vector<uint32_t> status(nb);
  std::vector<uint64_t> kb(nb, 0), vb(nb, 0), sb(nb, 0), xb(nb, 0);
  pbl_totals T{};
  for (uint32_t b = 0; b < nb; b++) {
    const M::HBlock S{batch->blocks + batch->block_off[b], batch->block_len[b]};
    M::HDesc& D = desc[b];
    status[b] = M::host_walk(S, &D, &kvs[b]);
    if (status[b] == PBL_OK) {
      for (const M::HKv& kv : kvs[b]) {
        kb[b] += S.at(D.boff, kv.span + 1) - S.at(D.boff, kv.span);
        vb[b] += S.at(D.boff, kv.span + 2) - S.at(D.boff, kv.span + 1);
        sb[b] += S.at(D.soff, kv.row + 1) - S.at(D.soff, kv.row);
        xb[b] += S.at(D.voff, kv.row + 1) - S.at(D.voff, kv.row);
      }
      if (kb[b] > M::kMaxBytes || vb[b] > M::kMaxBytes) status[b] = PBL_UNSUPPORTED;
    }
    if (status[b] != PBL_OK) {
      kvs[b].clear();
      kb[b] = vb[b] = sb[b] = xb[b] = 0;
      T.status_mask |= 1u << status[b];
      T.n_bad_blocks++;
    }
  }
  uint64_t nkv = 0, nk = 0, nv = 0, ns = 0, nx = 0;
  for (uint32_t b = 0; b <= nb; b++) {
    O.blk_kv_base[b] = nkv;
    O.blk_key_base[b] = nk;
    O.blk_val_base[b] = nv;
    if (O.blk_rst_base) O.blk_rst_base[b] = 0;
    if (extra) {
      extra->blk_suffix_base[b] = ns;
      extra->blk_value_base[b] = nx;
    }
    if (b == nb) break;
    O.blk_status[b] = status[b];
    nkv += kvs[b].size();
    nk += kb[b];
    nv += vb[b];
    ns += sb[b];
    nx += xb[b];
  }
  T.n_kv = nkv;
  T.key_bytes = nk;
  T.val_bytes = nv;
  const bool size_only = !O.key_off;
  const bool over = !size_only && (nkv > O.kv_cap || nk > O.key_cap || nv > O.val_cap ||
                                   (extra && (ns > extra->suffix_cap || nx > extra->value_cap)));
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *O.totals = T;
  if (over || size_only) return PBL_OK;
  for (uint32_t b = 0; b < nb; b++) {
    const M::HBlock S{batch->blocks + batch->block_off[b], batch->block_len[b]};
    const M::HDesc& D = desc[b];
    const uint64_t kv0 = O.blk_kv_base[b];
    uint32_t ko = 0, vo = 0, so = 0, xo = 0;
    for (size_t x = 0; x < kvs[b].size(); x++) {
      const M::HKv kv = kvs[b][x];
      const uint64_t i = kv0 + x, o = i + b;
      uint64_t tr = S.at(D.trl, kv.row);
      if (batch->synthetic_seq_num) tr = batch->synthetic_seq_num << 8 | (tr & 0xff);
      O.trailer[i] = tr;
      if (O.kv_flags) O.kv_flags[i] = 0;
      if (O.entry_off) O.entry_off[i] = kv.row;
      if (O.tiering_span_id) O.tiering_span_id[i] = O.tiering_attr[i] = 0;
      const uint64_t b0 = S.at(D.boff, kv.span), b1 = S.at(D.boff, kv.span + 1), b2 = S.at(D.boff, kv.span + 2);
      O.key_off[o] = ko;
      O.val_off[o] = vo;
      if (b1 > b0) memcpy(O.key_bytes + O.blk_key_base[b] + ko, S.p + D.bdata + b0, b1 - b0);
      if (b2 > b1) memcpy(O.val_bytes + O.blk_val_base[b] + vo, S.p + D.bdata + b1, b2 - b1);
      ko += uint32_t(b1 - b0);
      vo += uint32_t(b2 - b1);
      if (extra) {
        const uint64_t s0 = S.at(D.soff, kv.row), s1 = S.at(D.soff, kv.row + 1);
        const uint64_t x0 = S.at(D.voff, kv.row), x1 = S.at(D.voff, kv.row + 1);
        extra->span[i] = kv.span;
        extra->suffix_off[o] = so;
        extra->value_off[o] = xo;
        if (s1 > s0) memcpy(extra->suffix_bytes + extra->blk_suffix_base[b] + so, S.p + D.sdata + s0, s1 - s0);
        if (x1 > x0) memcpy(extra->value_bytes + extra->blk_value_base[b] + xo, S.p + D.vdata + x0, x1 - x0);
        so += uint32_t(s1 - s0);
        xo += uint32_t(x1 - x0);
      }
    }
    const uint64_t o = O.blk_kv_base[b + 1] + b;
    O.key_off[o] = ko;
    O.val_off[o] = vo;
    if (extra) {
      extra->suffix_off[o] = so;
      extra->value_off[o] = xo;
    }
  }
  return PBL_OK;
}

size_t pbl_keyspan_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {sizeof(pbl_keyspan_extra),
                        PBL_OFF(pbl_keyspan_extra, span),
                        PBL_OFF(pbl_keyspan_extra, suffix_off),
                        PBL_OFF(pbl_keyspan_extra, value_off),
                        PBL_OFF(pbl_keyspan_extra, suffix_bytes),
                        PBL_OFF(pbl_keyspan_extra, value_bytes),
                        PBL_OFF(pbl_keyspan_extra, blk_suffix_base),
                        PBL_OFF(pbl_keyspan_extra, blk_value_base),
                        PBL_OFF(pbl_keyspan_extra, suffix_cap),
                        PBL_OFF(pbl_keyspan_extra, value_cap)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
