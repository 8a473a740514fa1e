// merge.hip — batched k-way merge of sorted decoded batches, on the device
// (DESIGN.md §3.11): result block q is the sequence mergingIter.First();
// Next()... yields over block q of every run (merging_iter_heap.go:55-67,
// internal/base/internal.go:431-437: user key ascending under the comparer, then
// trailer descending; equal internal keys in run order), copied inside HBM into a
// result that has the layout of a decoded batch (include/pebble_amd.h).
//
//   merge_validate_kernel<comparer>  lane per source KV: compare with its
//       successor in the same block, flag the result block of a pair out of order
//   merge_persize_kernel  lane per result block: its status and its sizes, the
//       sums of the runs' base differences
//   merge_sum_kernel / merge_bases_kernel  the exclusive scan over result blocks
//       (result_core.hip.h's chunk_sums / bases): bases, statuses, totals, the
//       capacity check
//   merge_rank_kernel<comparer>  lane per source KV (run r, block q, index j): its
//       place in result block q is j + the KVs of the runs before r that are <=
//       it + the KVs of the runs after r that are < it (seek_core.hip.h's iupper /
//       ilower, K - 1 searches).  Writes (run, kv) and the KV's key and value
//       lengths at that place, in the workspace.
//   merge_tile_kernel / merge_tile_scan_kernel / merge_offsets_kernel  the
//       exclusive scan of the lengths in result order (tiles of 256 result KVs):
//       keys and values are contiguous in result order over the whole result, so
//       a block-relative offset is the global prefix minus the block's base
//   merge_emit_kernel  one wave per 64 result KVs: the per-KV arrays gathered
//       through (run, kv), keys lane per KV in 16-B chunks, values by
//       result_core.hip.h's copy_values.
//
// The tile scan, every block's last offset, the per-KV arrays and the value copy
// are result_core.hip.h's too; the kernels here are wrappers around them.
//
// The ranks are a bijection onto the block's places when every run's block is
// sorted, which the validation guarantees for every block that is merged; the
// emit nevertheless checks what it reads from the workspace against the runs
// and the result's sizes, so that no input leads outside the arrays.
//
// pbl_merge_batch_host is a different algorithm over the same ikey_cmp (a plain
// k-way merge that repeatedly takes the least head, lowest run first).
#include <algorithm>
#include <vector>

#include "result_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace merge {

constexpr uint32_t kMaxRuns = PBL_MERGE_MAX_RUNS;
constexpr uint64_t kHdr = 64;
constexpr uint32_t kTileShift = 8, kTile = 1u << kTileShift;  // result KVs per tile
constexpr int kMergeTPB = 256;
constexpr uint32_t kChunk = 256;      // result blocks per chunk of the scan over blocks
static_assert(kMergeTPB == result::kTPB && kChunk == uint32_t(result::kTPB), "result_core.hip.h's workgroup");
constexpr uint32_t kGrid = 2048;      // workgroups of a grid-striding kernel, at most (per run)
constexpr uint64_t kMaxBytes = 0xffffffffull;  // a block's key / value bytes (u32 offsets)
constexpr uint64_t kMaxKvs = 0xffffffffull;    // a block's KVs
constexpr int kRunShift = 56;                  // workspace src word: run << 56 | kv
constexpr uint64_t kKvMask = (1ull << kRunShift) - 1;
// header word (u32) 0: nonzero = sizes only (a capacity overflow, or runs that
// hold more KVs than the workspace was sized for)
enum { kHSkip = 0 };

struct Layout {
  uint64_t nt;  // tiles (n_kv / 256 + 1)
  uint64_t bad, qst, q64, csum, tsum, src, len, size;
  uint32_t n_chunks;
};
__host__ __device__ inline Layout layout(uint32_t nb, uint64_t n_kv) {
  Layout L;
  L.nt = (n_kv >> kTileShift) + 1;
  L.n_chunks = nb ? (nb + kChunk - 1) / kChunk : 1;
  uint64_t o = kHdr;
  L.bad = o;  o += 4ull * nb;
  L.qst = o;  o += 4ull * nb;
  o = (o + 15) & ~uint64_t(15);
  L.q64 = o;  o += 3ull * 8 * (uint64_t(nb) + 1);
  L.csum = o; o += 3ull * 8 * L.n_chunks;
  L.tsum = o; o += 2ull * 8 * L.nt;
  L.src = o;  o += 8ull * n_kv;
  L.len = o;  o += 8ull * n_kv;
  L.size = (o + 15) & ~uint64_t(15);
  return L;
}

// ---- device side ---------------------------------------------------------------
struct MergeArgs {
  pbl_decode_out run[kMaxRuns];
  pbl_merge_out out;
  uint32_t n_runs, n_blocks, comparer, size_only;
  uint64_t n_kv;  // the KVs of all runs, as the workspace was sized
  uint8_t* ws;
};

struct Ws {
  gptr<uint32_t> hdr, bad, qst;
  gptr<uint64_t> q64, csum, tsum[2], src;
  gptr<uint32_t> klen, vlen;
  uint64_t nt, qs;
  uint32_t n_chunks;
  __device__ Ws(uint8_t* ws, uint32_t nb, uint64_t n_kv) {
    const Layout L = layout(nb, n_kv);
    hdr = to_glb(reinterpret_cast<uint32_t*>(ws));
    bad = to_glb(reinterpret_cast<uint32_t*>(ws + L.bad));
    qst = to_glb(reinterpret_cast<uint32_t*>(ws + L.qst));
    q64 = to_glb(reinterpret_cast<uint64_t*>(ws + L.q64));
    csum = to_glb(reinterpret_cast<uint64_t*>(ws + L.csum));
    tsum[0] = to_glb(reinterpret_cast<uint64_t*>(ws + L.tsum));
    tsum[1] = tsum[0] + L.nt;
    src = to_glb(reinterpret_cast<uint64_t*>(ws + L.src));
    klen = to_glb(reinterpret_cast<uint32_t*>(ws + L.len));
    vlen = klen + n_kv;
    nt = L.nt;
    qs = uint64_t(nb) + 1;
    n_chunks = L.n_chunks;
  }
  __device__ gptr<uint64_t> q(int c) const { return q64 + uint64_t(c) * qs; }  // per-block KVs, key bytes, value bytes
  __device__ result::Sizes sizes() const { return result::Sizes{q64, csum, qst, qs, n_chunks}; }
};

__device__ inline uint64_t run_held(const MergeArgs& A, uint32_t r) {
  return A.n_blocks ? to_glb(A.run[r].blk_kv_base)[A.n_blocks] : 0;
}
// Whether the workspace describes the runs: they hold no more KVs than it was
// sized for.
__device__ inline bool described(const MergeArgs& A) {
  uint64_t t = 0;
  for (uint32_t r = 0; r < A.n_runs; r++) {
    const uint64_t h = run_held(A, r);
    if (h > A.n_kv) return false;
    t += h;
  }
  return t <= A.n_kv;
}

using result::block_excl_scan64;
using result::block_of;
using result::block_sum64;
using GR = seek::GlobalReader;

__device__ inline seek::View<GR> run_view(const MergeArgs& A, uint32_t r) {
  pbl_seek_queries sq{};
  return seek::View<GR>(A.run[r], A.n_blocks, sq, nullptr, 0);
}

// blockIdx.y = run.  A pair of neighbours out of order flags its result block.
template <uint32_t kCmp>
__global__ __launch_bounds__(kMergeTPB) void merge_validate_kernel(MergeArgs A) {
  if (!described(A)) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  const uint32_t r = blockIdx.y, nb = A.n_blocks;
  const uint64_t held = run_held(A, r);
  const seek::View<GR> V = run_view(A, r);
  const gptr<const uint64_t> tr = to_glb((const uint64_t*)A.run[r].trailer);
  for (uint64_t kv = uint64_t(blockIdx.x) * kMergeTPB + threadIdx.x; kv < held; kv += uint64_t(gridDim.x) * kMergeTPB) {
    const uint32_t q = block_of(V.blk_kv_base, nb, kv);
    if (V.blk_status[q] != PBL_OK) continue;
    const seek::Block<GR> B(V, q);
    if (kv < B.kv0 || kv - B.kv0 + 1 >= B.n) continue;
    const uint32_t j = uint32_t(kv - B.kv0);
    uint64_t al, bl;
    const cmp::kptr<GR> a = B.key(j, &al), b = B.key(j + 1, &bl);
    if (cmp::ikey_cmp<GR, kCmp>(a, al, tr[kv], b, bl, tr[kv + 1]) > 0) W.bad[q] = 1u;
  }
}

// Lane per result block: its status (the first non-OK status among the runs'
// blocks, in run order; an unsorted block; sizes past the u32 offsets) and sizes.
__global__ __launch_bounds__(kMergeTPB) void merge_persize_kernel(MergeArgs A) {
  const uint64_t q = uint64_t(blockIdx.x) * kMergeTPB + threadIdx.x;
  if (q >= A.n_blocks) return;
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  uint32_t st = described(A) ? uint32_t(PBL_OK) : uint32_t(PBL_INVALID_ARG);
  uint64_t n = 0, k = 0, v = 0;
  if (st == PBL_OK) {
    for (uint32_t r = 0; r < A.n_runs; r++) {
      const uint32_t s = to_glb(A.run[r].blk_status)[q];
      if (s != PBL_OK) {
        st = s;
        break;
      }
      n += to_glb(A.run[r].blk_kv_base)[q + 1] - to_glb(A.run[r].blk_kv_base)[q];
      k += to_glb(A.run[r].blk_key_base)[q + 1] - to_glb(A.run[r].blk_key_base)[q];
      v += to_glb(A.run[r].blk_val_base)[q + 1] - to_glb(A.run[r].blk_val_base)[q];
    }
  }
  if (st == PBL_OK && W.bad[q]) st = PBL_INVALID_ARG;
  if (st == PBL_OK && (n > kMaxKvs || k > kMaxBytes || v > kMaxBytes)) st = PBL_UNSUPPORTED;
  const bool some = st == PBL_OK;
  W.q(0)[q] = some ? n : 0;
  W.q(1)[q] = some ? k : 0;
  W.q(2)[q] = some ? v : 0;
  W.qst[q] = st;
}

// Per chunk of kChunk result blocks: the sums of {KVs, key bytes, value bytes}.
__global__ __launch_bounds__(kMergeTPB) void merge_sum_kernel(MergeArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  result::chunk_sums<3>(W.sizes(), A.n_blocks, lds);
}

// The result's bases, statuses and totals; the capacity check (the last chunk).
// Totals were zeroed by the entry point.
__global__ __launch_bounds__(kMergeTPB) void merge_bases_kernel(MergeArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  uint64_t ex[3], end[3];
  bool over;
  if (result::bases<3>(W.sizes(), A.out.result, A.n_blocks, A.size_only != 0, lds, ex, end, &over))
    W.hdr[kHSkip] = (over || end[0] > A.n_kv) ? 1u : 0u;
}

// blockIdx.y = run.  The place of every source KV in its result block.
template <uint32_t kCmp>
__global__ __launch_bounds__(kMergeTPB) void merge_rank_kernel(MergeArgs A) {
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;  // sizes only
  const uint32_t r = blockIdx.y, nb = A.n_blocks, nr = A.n_runs;
  const uint64_t held = run_held(A, r);
  const seek::View<GR> V = run_view(A, r);
  const gptr<const uint64_t> tr = to_glb((const uint64_t*)A.run[r].trailer);
  const gptr<const uint32_t> vo = to_glb((const uint32_t*)A.run[r].val_off);
  const gptr<const uint64_t> okvb = to_glb((const uint64_t*)A.out.result.blk_kv_base);
  const gptr<const uint32_t> ost = to_glb((const uint32_t*)A.out.result.blk_status);
  for (uint64_t kv = uint64_t(blockIdx.x) * kMergeTPB + threadIdx.x; kv < held; kv += uint64_t(gridDim.x) * kMergeTPB) {
    const uint32_t q = block_of(V.blk_kv_base, nb, kv);
    if (ost[q] != PBL_OK) continue;  // (an OK result block: every run's block is OK and sorted)
    const seek::Block<GR> B(V, q);
    if (kv < B.kv0 || kv - B.kv0 >= B.n) continue;
    const uint32_t j = uint32_t(kv - B.kv0);
    uint64_t kl;
    const cmp::kptr<GR> k = B.key(j, &kl);
    const uint64_t ktr = tr[kv];
    uint64_t pos = j;
    for (uint32_t s = 0; s < nr; s++) {
      if (s == r) continue;
      const seek::View<GR> Vs = run_view(A, s);
      const seek::Block<GR> Bs(Vs, q);
      const gptr<const uint64_t> trs = to_glb((const uint64_t*)A.run[s].trailer) + Bs.kv0;
      pos += s < r ? seek::iupper<GR, kCmp>(Bs, trs, k, kl, ktr) : seek::ilower<GR, kCmp>(Bs, trs, k, kl, ktr);
    }
    const uint64_t o0 = okvb[q];
    if (pos >= okvb[q + 1] - o0 || o0 + pos >= A.n_kv) continue;
    const uint64_t p = o0 + pos;
    W.src[p] = uint64_t(r) << kRunShift | kv;
    W.klen[p] = uint32_t(kl);
    W.vlen[p] = vo[kv + q + 1] - vo[kv + q];
  }
}

// Per tile of 256 result KVs: its key bytes and value bytes.
__global__ __launch_bounds__(kMergeTPB) void merge_tile_kernel(MergeArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;
  const uint64_t total = to_glb(A.out.result.blk_kv_base)[A.n_blocks];
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t p = (t << kTileShift) + threadIdx.x;
    const uint64_t k = block_sum64(p < total ? W.klen[p] : 0u, lds), x = block_sum64(p < total ? W.vlen[p] : 0u, lds);
    if (threadIdx.x == 0) {
      W.tsum[0][t] = k;
      W.tsum[1][t] = x;
    }
  }
}

// One workgroup: the exclusive scan over tiles, in place.
__global__ __launch_bounds__(kMergeTPB) void merge_tile_scan_kernel(MergeArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;
  result::tile_scan_inplace(W.tsum, W.nt, lds);
}

// key_off / val_off of the result: the prefix of the lengths in result order,
// relative to the block's first byte; every block's last offset.
__global__ __launch_bounds__(kMergeTPB) void merge_offsets_kernel(MergeArgs A) {
  __shared__ uint64_t lds[4];
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;
  const pbl_decode_out& O = A.out.result;
  const uint32_t nb = A.n_blocks;
  const gptr<const uint64_t> okvb = to_glb((const uint64_t*)O.blk_kv_base), okeyb = to_glb((const uint64_t*)O.blk_key_base),
                             ovalb = to_glb((const uint64_t*)O.blk_val_base);
  result::last_offsets(O, nb, ~0ull);
  const uint64_t total = okvb[nb];
  for (uint64_t t = blockIdx.x; t < W.nt; t += gridDim.x) {
    const uint64_t p = (t << kTileShift) + threadIdx.x;
    const bool in = p < total;
    uint64_t tot;
    const uint64_t kx = W.tsum[0][t] + block_excl_scan64(in ? W.klen[p] : 0u, lds, &tot);
    const uint64_t vx = W.tsum[1][t] + block_excl_scan64(in ? W.vlen[p] : 0u, lds, &tot);
    if (in) {
      const uint32_t q = block_of(okvb, nb, p);
      to_glb(O.key_off)[p + q] = uint32_t(kx - okeyb[q]);
      to_glb(O.val_off)[p + q] = uint32_t(vx - ovalb[q]);
    }
  }
}

#ifndef PBL_MERGE_EMIT_WAVES
#define PBL_MERGE_EMIT_WAVES 5  // as every caller of result::copy_values
#endif
__global__ void __launch_bounds__(kMergeTPB) __attribute__((amdgpu_waves_per_eu(PBL_MERGE_EMIT_WAVES)))
merge_emit_kernel(MergeArgs A) {
  const Ws W(A.ws, A.n_blocks, A.n_kv);
  if (W.hdr[kHSkip] != 0) return;  // sizes only
  const pbl_decode_out& O = A.out.result;
  const uint32_t nb = A.n_blocks, nr = A.n_runs;
  const uint32_t lane = lane_id();
  const gptr<const uint64_t> okvb = to_glb((const uint64_t*)O.blk_kv_base), okeyb = to_glb((const uint64_t*)O.blk_key_base),
                             ovalb = to_glb((const uint64_t*)O.blk_val_base);
  const uint64_t total = okvb[nb];
  const uint64_t n_items = (total + kWave - 1) / kWave;
  const uint32_t wpb = kMergeTPB / kWave;
  for (uint64_t item = uint64_t(blockIdx.x) * wpb + wave_id(); item < n_items; item += uint64_t(gridDim.x) * wpb) {
    const uint64_t p = item * kWave + lane;
    bool ok = p < total;
    uint32_t klen = 0, vlen = 0;
    gptr<const uint8_t> ksrc = nullptr, vsrc = nullptr;
    gptr<uint8_t> kdst = nullptr, vdst = nullptr;
    if (ok) {
      const uint32_t q = block_of(okvb, nb, p);
      const uint64_t s = W.src[p];
      const uint32_t r = uint32_t(s >> kRunShift);
      const uint64_t kv = s & kKvMask;
      klen = W.klen[p];
      vlen = W.vlen[p];
      const uint32_t ko = to_glb(O.key_off)[p + q], vo = to_glb(O.val_off)[p + q];
      ok = r < nr;
      const pbl_decode_out& I = A.run[ok ? r : 0u];
      // what the workspace names is checked against the run and the result's
      // sizes: a KV of the run's block q, with these lengths, inside the block
      ok = ok && kv >= to_glb(I.blk_kv_base)[q] && kv < to_glb(I.blk_kv_base)[q + 1];
      if (ok) {
        const uint32_t k0 = to_glb(I.key_off)[kv + q], k1 = to_glb(I.key_off)[kv + q + 1];
        const uint32_t v0 = to_glb(I.val_off)[kv + q], v1 = to_glb(I.val_off)[kv + q + 1];
        ok = k1 - k0 == klen && v1 - v0 == vlen && uint64_t(ko) + klen <= okeyb[q + 1] - okeyb[q] &&
             uint64_t(vo) + vlen <= ovalb[q + 1] - ovalb[q];
        ksrc = to_glb((const uint8_t*)I.key_bytes) + (to_glb(I.blk_key_base)[q] + k0);
        vsrc = to_glb((const uint8_t*)I.val_bytes) + (to_glb(I.blk_val_base)[q] + v0);
        kdst = to_glb(O.key_bytes) + (okeyb[q] + ko);
        vdst = to_glb(O.val_bytes) + (ovalb[q] + vo);
      }
      if (ok) {
        result::copy_kv_arrays(O, p, I, kv, 0xff, true);
        if (A.out.src_run) to_glb(A.out.src_run)[p] = uint8_t(r);
        if (A.out.src_kv) to_glb(A.out.src_kv)[p] = kv;
        copy_chunks(kdst, ksrc, klen);
      }
    }
    result::copy_values(ok, vlen, vsrc, vdst);
  }
}

// ---- host side -----------------------------------------------------------------
// Argument checks shared by the device and the host entry points.
inline bool args_ok(const pbl_merge_runs* in, const pbl_merge_out* out, bool size_only) {
  if (!in || !out || !in->runs) return false;
  if (in->n_runs == 0 || in->n_runs > kMaxRuns || in->comparer > PBL_CMP_CRDB) return false;
  for (uint32_t r = 0; r < in->n_runs; r++)
    if (!result::source_ok(&in->runs[r])) return false;
  return result::result_ok(out->result, size_only);
}
inline bool ws_ok(const void* ws, uint64_t bytes, uint32_t nb, uint64_t n_kv) {
  return result::ws_aligned(ws) && bytes >= layout(nb, n_kv).size;
}

inline int launch(const pbl_merge_runs* in, pbl_merge_out* out, void* ws, uint64_t ws_bytes, bool size_only, bool sized,
                  hipStream_t st) {
  if (!args_ok(in, out, size_only) || !ws_ok(ws, ws_bytes, in->n_blocks, in->n_kv_total)) return PBL_INVALID_ARG;
  const uint32_t nb = in->n_blocks, nr = in->n_runs;
  const uint64_t n_kv = in->n_kv_total;
  MergeArgs a{};
  for (uint32_t r = 0; r < nr; r++) a.run[r] = in->runs[r];
  a.out = *out;
  a.n_runs = nr;
  a.n_blocks = nb;
  a.comparer = in->comparer;
  a.size_only = size_only ? 1u : 0u;
  a.n_kv = n_kv;
  a.ws = static_cast<uint8_t*>(ws);
  const Layout L = layout(nb, n_kv);
  if (hipMemsetAsync(out->result.totals, 0, sizeof(pbl_totals), st) != hipSuccess) return PBL_DEVICE_ERROR;
  const uint32_t kv_grid = uint32_t(std::min<uint64_t>((n_kv + kMergeTPB - 1) / kMergeTPB, kGrid));
  const uint32_t q_grid = (nb + kMergeTPB - 1) / kMergeTPB;
  if (!sized) {
    // the header and the unsorted flags
    if (hipMemsetAsync(a.ws, 0, L.qst, st) != hipSuccess) return PBL_DEVICE_ERROR;
    if (nb && n_kv)
      seek::with_cmp(in->comparer, [&](auto c) {
        hipLaunchKernelGGL(merge_validate_kernel<decltype(c)::value>, dim3(kv_grid, nr), dim3(kMergeTPB), 0, st, a);
        return 0;
      });
    if (nb) {
      hipLaunchKernelGGL(merge_persize_kernel, dim3(q_grid), dim3(kMergeTPB), 0, st, a);
      hipLaunchKernelGGL(merge_sum_kernel, dim3(L.n_chunks), dim3(kMergeTPB), 0, st, a);
    }
  }
  hipLaunchKernelGGL(merge_bases_kernel, dim3(L.n_chunks), dim3(kMergeTPB), 0, st, a);
  if (!size_only && nb && n_kv && out->result.key_off) {
    // places nobody ranks name no run and hold no bytes
    if (hipMemsetAsync(a.ws + L.src, 0xff, 8ull * n_kv, st) != hipSuccess ||
        hipMemsetAsync(a.ws + L.len, 0, 8ull * n_kv, st) != hipSuccess)
      return PBL_DEVICE_ERROR;
    seek::with_cmp(in->comparer, [&](auto c) {
      hipLaunchKernelGGL(merge_rank_kernel<decltype(c)::value>, dim3(kv_grid, nr), dim3(kMergeTPB), 0, st, a);
      return 0;
    });
    const uint32_t t_grid = uint32_t(std::min<uint64_t>(L.nt, kGrid));
    hipLaunchKernelGGL(merge_tile_kernel, dim3(t_grid), dim3(kMergeTPB), 0, st, a);
    hipLaunchKernelGGL(merge_tile_scan_kernel, dim3(1), dim3(kMergeTPB), 0, st, a);
    hipLaunchKernelGGL(merge_offsets_kernel, dim3(std::max(t_grid, std::min(q_grid, kGrid))), dim3(kMergeTPB), 0, st, a);
    hipLaunchKernelGGL(merge_emit_kernel, dim3(t_grid), dim3(kMergeTPB), 0, st, a);
  } else if (!size_only && nb && out->result.key_off) {
    // no KVs at all: every block's only offset
    hipLaunchKernelGGL(merge_offsets_kernel, dim3(std::min(q_grid, kGrid)), dim3(kMergeTPB), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

// One run's block on the host.
struct HostBlock {
  seek::Block<cmp::HostReader> B;
  const uint64_t* tr;
};

}  // namespace merge
}  // namespace pbl

extern "C" {

uint64_t pbl_merge_workspace_bytes(uint32_t n_runs, uint32_t n_blocks, uint64_t n_kv_total) {
  (void)n_runs;  // nothing in the workspace scales with the number of runs
  return pbl::merge::layout(n_blocks, n_kv_total).size;
}

int pbl_merge_size(const pbl_merge_runs* runs, pbl_merge_out* out, void* workspace, uint64_t workspace_bytes,
                   void* stream) {
  return pbl::merge::launch(runs, out, workspace, workspace_bytes, true, false, reinterpret_cast<hipStream_t>(stream));
}

int pbl_merge_batch(const pbl_merge_runs* runs, pbl_merge_out* out, void* workspace, uint64_t workspace_bytes,
                    uint32_t flags, void* stream) {
  if (flags & ~uint32_t(PBL_MERGE_SIZED)) return PBL_INVALID_ARG;
  return pbl::merge::launch(runs, out, workspace, workspace_bytes, false, (flags & PBL_MERGE_SIZED) != 0,
                            reinterpret_cast<hipStream_t>(stream));
}

int pbl_merge_batch_host(const pbl_merge_runs* in, pbl_merge_out* out) {
  namespace M = pbl::merge;
  namespace K = pbl::seek;
  using R = pbl::cmp::HostReader;
  if (!M::args_ok(in, out, false)) return PBL_INVALID_ARG;
  const pbl_decode_out& O = out->result;
  const uint32_t nb = in->n_blocks, nr = in->n_runs;
  pbl_seek_queries sq{};
  std::vector<K::View<R>> V;
  for (uint32_t r = 0; r < nr; r++) V.emplace_back(in->runs[r], nb, sq, nullptr, 0);
  auto block = [&](uint32_t r, uint32_t q) { return M::HostBlock{K::Block<R>(V[r], q), in->runs[r].trailer + V[r].blk_kv_base[q]}; };

  // statuses and sizes
  std::vector<uint32_t> status(nb);
  pbl_totals T{};
  uint64_t kvb = 0, keyb = 0, valb = 0;
  K::with_cmp(in->comparer, [&](auto c) {
    constexpr uint32_t kCmp = decltype(c)::value;
    for (uint32_t q = 0; q < nb; q++) {
      uint32_t st = PBL_OK;
      uint64_t n = 0, k = 0, v = 0;
      for (uint32_t r = 0; r < nr && st == PBL_OK; r++) {
        const pbl_decode_out& D = in->runs[r];
        if (D.blk_status[q] != PBL_OK) {
          st = D.blk_status[q];
          break;
        }
        n += D.blk_kv_base[q + 1] - D.blk_kv_base[q];
        k += D.blk_key_base[q + 1] - D.blk_key_base[q];
        v += D.blk_val_base[q + 1] - D.blk_val_base[q];
      }
      for (uint32_t r = 0; r < nr && st == PBL_OK; r++) {  // sorted, non-strictly
        const M::HostBlock H = block(r, q);
        for (uint32_t j = 0; j + 1 < H.B.n; j++) {
          uint64_t al, bl;
          const uint8_t *a = H.B.key(j, &al), *b = H.B.key(j + 1, &bl);
          if (pbl::cmp::ikey_cmp<R, kCmp>(a, al, H.tr[j], b, bl, H.tr[j + 1]) > 0) {
            st = PBL_INVALID_ARG;
            break;
          }
        }
      }
      if (st == PBL_OK && (n > M::kMaxKvs || k > M::kMaxBytes || v > M::kMaxBytes)) st = PBL_UNSUPPORTED;
      if (st != PBL_OK) {
        n = k = v = 0;
        T.status_mask |= 1u << st;
        T.n_bad_blocks++;
      }
      status[q] = st;
      O.blk_kv_base[q] = kvb;
      O.blk_key_base[q] = keyb;
      O.blk_val_base[q] = valb;
      if (O.blk_rst_base) O.blk_rst_base[q] = 0;
      O.blk_status[q] = st;
      kvb += n;
      keyb += k;
      valb += v;
    }
    return 0;
  });
  O.blk_kv_base[nb] = kvb;
  O.blk_key_base[nb] = keyb;
  O.blk_val_base[nb] = valb;
  if (O.blk_rst_base) O.blk_rst_base[nb] = 0;
  T.n_kv = kvb;
  T.key_bytes = keyb;
  T.val_bytes = valb;
  const bool over = kvb > O.kv_cap || keyb > O.key_cap || valb > O.val_cap;
  if (over) T.status_mask |= 1u << PBL_OVERFLOW;
  *O.totals = T;
  if (over || !O.key_off) return PBL_OK;

  // the merge: repeatedly the least head, the lowest run among equals
  K::with_cmp(in->comparer, [&](auto c) {
    constexpr uint32_t kCmp = decltype(c)::value;
    std::vector<M::HostBlock> H;
    std::vector<uint32_t> head(nr);
    for (uint32_t q = 0; q < nb; q++) {
      uint64_t p = O.blk_kv_base[q];
      uint32_t ko = 0, vo = 0;
      if (status[q] == PBL_OK) {
        H.clear();
        for (uint32_t r = 0; r < nr; r++) H.push_back(block(r, q));
        std::fill(head.begin(), head.end(), 0u);
        for (;;) {
          uint32_t best = nr;
          const uint8_t* bk = nullptr;
          uint64_t bl = 0;
          for (uint32_t r = 0; r < nr; r++) {
            if (head[r] >= H[r].B.n) continue;
            uint64_t kl;
            const uint8_t* k = H[r].B.key(head[r], &kl);
            if (best == nr || pbl::cmp::ikey_cmp<R, kCmp>(k, kl, H[r].tr[head[r]], bk, bl, H[best].tr[head[best]]) < 0) {
              best = r;
              bk = k;
              bl = kl;
            }
          }
          if (best == nr) break;
          const pbl_decode_out& D = in->runs[best];
          const uint64_t kv = H[best].B.kv0 + head[best]++;
          const uint32_t v0 = D.val_off[kv + q], vl = D.val_off[kv + q + 1] - v0;
          O.trailer[p] = D.trailer[kv];
          if (O.kv_flags) O.kv_flags[p] = D.kv_flags ? D.kv_flags[kv] : uint8_t(0);
          if (O.entry_off) O.entry_off[p] = D.entry_off ? D.entry_off[kv] : 0u;
          if (O.tiering_span_id) {
            O.tiering_span_id[p] = D.tiering_span_id ? D.tiering_span_id[kv] : 0ull;
            O.tiering_attr[p] = D.tiering_attr ? D.tiering_attr[kv] : 0ull;
          }
          if (out->src_run) out->src_run[p] = uint8_t(best);
          if (out->src_kv) out->src_kv[p] = kv;
          O.key_off[p + q] = ko;
          O.val_off[p + q] = vo;
          if (bl) memcpy(O.key_bytes + O.blk_key_base[q] + ko, bk, bl);
          if (vl) memcpy(O.val_bytes + O.blk_val_base[q] + vo, D.val_bytes + D.blk_val_base[q] + v0, vl);
          ko += uint32_t(bl);
          vo += vl;
          p++;
        }
      }
      O.key_off[p + q] = ko;
      O.val_off[p + q] = vo;
    }
    return 0;
  });
  return PBL_OK;
}

size_t pbl_merge_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_merge_runs), PBL_OFF(pbl_merge_runs, runs), PBL_OFF(pbl_merge_runs, n_runs),
      PBL_OFF(pbl_merge_runs, n_blocks), PBL_OFF(pbl_merge_runs, comparer), PBL_OFF(pbl_merge_runs, reserved),
      PBL_OFF(pbl_merge_runs, n_kv_total),
      sizeof(pbl_merge_out), PBL_OFF(pbl_merge_out, result), PBL_OFF(pbl_merge_out, src_run),
      PBL_OFF(pbl_merge_out, src_kv)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
