// filter.hip — batched probes of table bloom filters on the device, and the
// host forms of probe and builder.
//
// Get and SeekPrefixGE ask a table's filter before they touch an index or data
// block (sstable/reader_iter_single_lvl.go:1037-1134); this is that question
// for a batch of keys against one or many filter blocks resident in HBM.
//
//   filter_probe_kernel<comparer, all_pairs>   lane per key: Split, the hash,
//       then per filter the trailer, the line h % nLines and its probed bytes.
//       The probe is a short arithmetic chain followed by one dependent access
//       to a random 64-byte line: latency, not bytes.  So the whole line is
//       loaded before any bit of it is tested, and in all-pairs mode a key is
//       hashed once and the loop over the filters holds no branch on a result.
//       The trailer is read through wave-uniform addresses (scalar loads) where
//       the whole wave asks one filter: always in all-pairs mode, and in named
//       mode when the wave's ids agree.
//
// Every rule (hash, parse, probe, set) is filter_core.hip.h's; the kernel
// instantiates it with seek_core.hip.h's GlobalReader, the host forms with
// cmp::HostReader.
#include <vector>

#include "filter_core.hip.h"
#include "seek_core.hip.h"

namespace pbl {
namespace filter {

using seek::GlobalReader;
constexpr int kTPB = 256;

struct ProbeArgs {
  pbl_filter_set set;
  pbl_filter_queries q;
  pbl_filter_out out;
};

// may bits of hash h in filter f (f < n_filters)
template <class R>
PBL_HD inline uint8_t may_of(typename R::template ptr<const uint8_t> bytes, typename R::template ptr<const uint64_t> off,
                             uint32_t f, uint32_t h) {
  const uint64_t o0 = off[f], o1 = off[f + 1];
  const Header H = bloom_parse<R>(bytes + o0, o1 > o0 ? o1 - o0 : 0);
  const bool may = bloom_may<R>(bytes + o0, H, h);
  return uint8_t((may ? PBL_FILTER_MAY : 0u) | (H.status != PBL_OK ? PBL_FILTER_BAD : 0u));
}

template <uint32_t kCmp, bool kAllPairs>
__global__ __launch_bounds__(kTPB) void filter_probe_kernel(ProbeArgs A) {
  using R = GlobalReader;
  const uint64_t i = uint64_t(blockIdx.x) * kTPB + threadIdx.x;
  const gptr<const uint8_t> fb = to_glb(A.set.bytes);
  const gptr<const uint64_t> fo = to_glb(A.set.off);
  if (A.out.flt_status) {
    const gptr<int32_t> st = to_glb(A.out.flt_status);
    for (uint64_t f = i; f < A.set.n_filters; f += uint64_t(gridDim.x) * kTPB) {
      const uint64_t o0 = fo[f], o1 = fo[f + 1];
      st[f] = bloom_parse<R>(fb + o0, o1 > o0 ? o1 - o0 : 0).status;
    }
  }
  const bool live = i < A.q.n;
  uint32_t h = 0;
  if (live) {
    const gptr<const uint64_t> ko = to_glb(A.q.key_off);
    const uint64_t k0 = ko[i];
    h = prefix_hash<R>(kCmp, to_glb(A.q.key_bytes) + k0, ko[i + 1] - k0);
    if (A.out.hash) to_glb(A.out.hash)[i] = h;
  }
  const gptr<uint8_t> may = to_glb(A.out.may);
  if (kAllPairs) {
    // f is wave-uniform: offsets and trailer come through scalar loads
    for (uint32_t f = 0; f < A.set.n_filters; f++) {
      const uint8_t m = may_of<R>(fb, fo, f, h);
      if (live) may[uint64_t(f) * A.q.n + i] = m;
    }
  } else if (live) {
    const uint32_t f = to_glb(A.q.filter)[i];
    const uint32_t f0 = __builtin_amdgcn_readfirstlane(f);
    uint8_t m = uint8_t(PBL_FILTER_MAY | PBL_FILTER_BAD);
    if (__builtin_amdgcn_ballot_w64(f != f0) == 0) {  // the wave asks one filter: its trailer is read once
      if (f0 < A.set.n_filters) m = may_of<R>(fb, fo, f0, h);
    } else if (f < A.set.n_filters) {
      m = may_of<R>(fb, fo, f, h);
    }
    may[i] = m;
  }
}

inline bool args_ok(const pbl_filter_set* set, const pbl_filter_queries* q, const pbl_filter_out* out) {
  if (!set || !q || !out) return false;
  if (!out->may || !q->key_off || q->comparer > PBL_CMP_CRDB) return false;
  return true;
}

}  // namespace filter
}  // namespace pbl

extern "C" {

int pbl_filter_probe(const pbl_filter_set* set, const pbl_filter_queries* q, pbl_filter_out* out, void* stream) {
  namespace F = pbl::filter;
  if (!F::args_ok(set, q, out)) return PBL_INVALID_ARG;
  if (q->n == 0 || set->n_filters == 0) return PBL_OK;
  if (!set->bytes || !set->off || !q->key_bytes) return PBL_INVALID_ARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  F::ProbeArgs a{*set, *q, *out};
  const uint32_t grid = uint32_t((uint64_t(q->n) + F::kTPB - 1) / F::kTPB);
  pbl::seek::with_cmp(q->comparer, [&](auto c) {
    constexpr uint32_t kc = decltype(c)::value;
    if (q->filter) hipLaunchKernelGGL((F::filter_probe_kernel<kc, false>), dim3(grid), dim3(F::kTPB), 0, st, a);
    else hipLaunchKernelGGL((F::filter_probe_kernel<kc, true>), dim3(grid), dim3(F::kTPB), 0, st, a);
    return 0;
  });
  return hipGetLastError() == hipSuccess ? PBL_OK : PBL_DEVICE_ERROR;
}

int pbl_filter_probe_host(const pbl_filter_set* set, const pbl_filter_queries* q, pbl_filter_out* out) {
  namespace F = pbl::filter;
  using R = pbl::cmp::HostReader;
  if (!F::args_ok(set, q, out)) return PBL_INVALID_ARG;
  if (q->n == 0 || set->n_filters == 0) return PBL_OK;
  if (!set->bytes || !set->off || !q->key_bytes) return PBL_INVALID_ARG;
  if (out->flt_status)
    for (uint32_t f = 0; f < set->n_filters; f++) {
      const uint64_t o0 = set->off[f], o1 = set->off[f + 1];
      out->flt_status[f] = F::bloom_parse<R>(set->bytes + o0, o1 > o0 ? o1 - o0 : 0).status;
    }
  for (uint64_t i = 0; i < q->n; i++) {
    const uint64_t k0 = q->key_off[i];
    const uint32_t h = F::prefix_hash<R>(q->comparer, q->key_bytes + k0, q->key_off[i + 1] - k0);
    if (out->hash) out->hash[i] = h;
    if (!q->filter) {
      for (uint32_t f = 0; f < set->n_filters; f++)
        out->may[uint64_t(f) * q->n + i] = F::may_of<R>(set->bytes, set->off, f, h);
    } else {
      const uint32_t f = q->filter[i];
      out->may[i] = f < set->n_filters ? F::may_of<R>(set->bytes, set->off, f, h)
                                       : uint8_t(PBL_FILTER_MAY | PBL_FILTER_BAD);
    }
  }
  return PBL_OK;
}

uint64_t pbl_bloom_build_bound(uint64_t n, uint32_t bits_per_key) {
  return n ? pbl::filter::lines_for(n, bits_per_key) * pbl::filter::kLine + pbl::filter::kTrailer : 0;
}

int pbl_bloom_build_host(const uint8_t* key_bytes, const uint64_t* key_off, uint64_t n, uint32_t comparer,
                         uint32_t bits_per_key, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  namespace F = pbl::filter;
  using R = pbl::cmp::HostReader;
  if (!key_off || !out_len || comparer > PBL_CMP_CRDB || bits_per_key == 0 || (n && !key_bytes))
    return PBL_INVALID_ARG;
  std::vector<uint32_t> hs;
  hs.reserve(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t h = F::prefix_hash<R>(comparer, key_bytes + key_off[i], key_off[i + 1] - key_off[i]);
    if (hs.empty() || h != hs.back()) hs.push_back(h);
  }
  if (hs.empty()) {
    *out_len = 0;
    return PBL_OK;
  }
  const uint64_t nl = F::lines_for(hs.size(), bits_per_key);
  if (nl > 0xffffffffull) return PBL_UNSUPPORTED;
  *out_len = nl * F::kLine + F::kTrailer;
  if (!out || cap < *out_len) return PBL_OVERFLOW;
  memset(out, 0, *out_len);
  const uint32_t np = F::probes_for(bits_per_key);
  for (uint32_t h : hs) F::bloom_set(out, uint32_t(nl), np, h);
  uint8_t* t = out + nl * F::kLine;
  t[0] = uint8_t(np);
  for (int b = 0; b < 4; b++) t[1 + b] = uint8_t(nl >> (8 * b));
  return PBL_OK;
}

size_t pbl_filter_struct_layout(uint64_t* out, size_t cap) {
#define PBL_OFF(T, f) uint64_t(offsetof(T, f))
  const uint64_t v[] = {
      sizeof(pbl_filter_set), PBL_OFF(pbl_filter_set, bytes), PBL_OFF(pbl_filter_set, off),
      PBL_OFF(pbl_filter_set, n_filters),
      sizeof(pbl_filter_queries), PBL_OFF(pbl_filter_queries, key_bytes), PBL_OFF(pbl_filter_queries, key_off),
      PBL_OFF(pbl_filter_queries, filter), PBL_OFF(pbl_filter_queries, n), PBL_OFF(pbl_filter_queries, comparer),
      sizeof(pbl_filter_out), PBL_OFF(pbl_filter_out, may), PBL_OFF(pbl_filter_out, hash),
      PBL_OFF(pbl_filter_out, flt_status)};
#undef PBL_OFF
  const size_t n = sizeof(v) / sizeof(v[0]);
  for (size_t i = 0; i < n && i < cap && out; i++) out[i] = v[i];
  return n;
}

}  // extern "C"
