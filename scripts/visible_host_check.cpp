// visible_host_check.cpp — pbl_visible_batch_host as a stand-alone host program
// for sanitizer runs (no GPU is touched): random blocks under all three
// comparers, sorted (by pbl_key_compare), unsorted, bad and unsupported blocks,
// random kinds, handle flags, snapshots and both modes, every buffer a heap
// allocation of exactly its size, so that a read or write past an end is seen.
// Checks that every result block holds visible KVs of value kinds only, with
// user keys strictly ascending when chains are folded, and that src_kv / n_src
// name KVs of the source block.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/visible.hip pebble_amd/csrc/data_iter.cpp scripts/visible_host_check.cpp \
//     -fsanitize=address,undefined -o visible_host_check && ./visible_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"
struct Batch {
  std::vector<uint64_t> trailer, kvb, keyb, valb; std::vector<uint8_t> flags, kbytes, vbytes;
  std::vector<uint32_t> koff, voff, status;
  pbl_decode_out c() { pbl_decode_out d{}; d.trailer = trailer.data(); d.kv_flags = flags.data(); d.key_off = koff.data(); d.val_off = voff.data();
    d.key_bytes = kbytes.data(); d.val_bytes = vbytes.data(); d.blk_kv_base = kvb.data(); d.blk_key_base = keyb.data(); d.blk_val_base = valb.data();
    d.blk_status = status.data(); return d; }
};
int main() {
  std::mt19937 rng(11);
  const uint32_t kinds[] = {0, 1, 2, 7, 18, 23, 2, 1, 2, 21};
  uint64_t results = 0, bad = 0;
  for (int iter = 0; iter < 400; iter++) {
    const uint32_t nb = 1 + rng() % 5, cmp = rng() % 3, flags = rng() % 2 ? PBL_VISIBLE_KEEP_OPERANDS : 0;
    const uint64_t snapshot = rng() % 4 == 0 ? PBL_SEQNUM_MAX : rng() % 60;
    Batch R;
    R.kvb.push_back(0); R.keyb.push_back(0); R.valb.push_back(0);
    for (uint32_t q = 0; q < nb; q++) {
      const uint32_t n = rng() % 4 == 0 ? 0 : rng() % 90;
      const bool odd_kinds = rng() % 8 == 0, handles = rng() % 6 == 0;
      std::vector<std::pair<std::string, uint64_t>> kv;
      for (uint32_t j = 0; j < n; j++) {
        std::string k(rng() % 6, 'a');
        for (auto& ch : k) ch = "ab@1\0\x09"[rng() % 6];
        kv.push_back({k, uint64_t(rng() % 50) << 8 | kinds[rng() % (odd_kinds ? 10 : 9)]});
      }
      if (rng() % 8)
        std::sort(kv.begin(), kv.end(), [&](auto& a, auto& b) {
          const int c = pbl_key_compare(cmp, (const uint8_t*)a.first.data(), a.first.size(), (const uint8_t*)b.first.data(), b.first.size());
          return c ? c < 0 : a.second > b.second; });
      size_t k0 = R.kbytes.size(), v0 = R.vbytes.size();
      for (auto& x : kv) {
        R.koff.push_back(uint32_t(R.kbytes.size() - k0)); R.voff.push_back(uint32_t(R.vbytes.size() - v0));
        R.kbytes.insert(R.kbytes.end(), x.first.begin(), x.first.end());
        R.vbytes.insert(R.vbytes.end(), rng() % 30, uint8_t('v'));
        R.trailer.push_back(x.second);
        R.flags.push_back(uint8_t((handles && rng() % 10 == 0 ? PBL_KV_VALBLK_HANDLE : 0) | (rng() % 3 == 0 ? PBL_KV_OBSOLETE : 0) |
                                  (odd_kinds && rng() % 40 == 0 ? PBL_KV_INVALID_KEY : 0)));
      }
      R.koff.push_back(uint32_t(R.kbytes.size() - k0)); R.voff.push_back(uint32_t(R.vbytes.size() - v0));
      R.status.push_back(rng() % 10 == 0 ? PBL_CORRUPT_BOUNDS : PBL_OK);
      R.kvb.push_back(R.trailer.size()); R.keyb.push_back(R.kbytes.size()); R.valb.push_back(R.vbytes.size());
    }
    // exact sizes: shrink so that ASan sees every byte past the end
    R.kbytes.shrink_to_fit(); R.vbytes.shrink_to_fit(); R.trailer.shrink_to_fit(); R.flags.shrink_to_fit(); R.koff.shrink_to_fit(); R.voff.shrink_to_fit();
    if (R.trailer.empty()) { R.trailer.reserve(1); R.flags.reserve(1); }
    if (R.kbytes.empty()) R.kbytes.reserve(1);
    if (R.vbytes.empty()) R.vbytes.reserve(1);
    pbl_visible_in in{R.c(), nb, cmp, 0, snapshot};
    std::vector<uint64_t> okv(nb + 1), okey(nb + 1), oval(nb + 1); std::vector<uint32_t> ost(nb);
    pbl_totals T{};
    pbl_visible_out out{}; out.result.blk_kv_base = okv.data(); out.result.blk_key_base = okey.data(); out.result.blk_val_base = oval.data();
    out.result.blk_status = ost.data(); out.result.totals = &T;
    if (pbl_visible_batch_host(&in, &out, flags) != PBL_OK) return 1;
    const uint64_t n = T.n_kv, kb = T.key_bytes, vb = T.val_bytes;
    uint64_t* tr = (uint64_t*)malloc(n * 8 + 1); uint8_t* fl = (uint8_t*)malloc(n + 1); uint32_t* ko = (uint32_t*)malloc((n + nb) * 4);
    uint32_t* vo = (uint32_t*)malloc((n + nb) * 4); uint8_t* kby = (uint8_t*)malloc(kb + 1); uint8_t* vby = (uint8_t*)malloc(vb + 1);
    uint64_t* sk = (uint64_t*)malloc(n * 8 + 1); uint32_t* ns = (uint32_t*)malloc(n * 4 + 1);
    out.result.trailer = tr; out.result.kv_flags = fl; out.result.key_off = ko; out.result.val_off = vo; out.result.key_bytes = kby;
    out.result.val_bytes = vby; out.result.kv_cap = n; out.result.key_cap = kb; out.result.val_cap = vb; out.src_kv = sk; out.n_src = ns;
    if (pbl_visible_batch_host(&in, &out, flags) != PBL_OK) return 2;
    if (T.n_kv != n || (T.status_mask & (1u << PBL_OVERFLOW))) return 3;
    for (uint32_t q = 0; q < nb; q++) {
      if (ost[q] != PBL_OK) { bad++; if (okv[q + 1] != okv[q]) return 4; continue; }
      if (vo[okv[q + 1] + q] != oval[q + 1] - oval[q] || ko[okv[q + 1] + q] != okey[q + 1] - okey[q]) return 5;
      for (uint64_t p = okv[q]; p < okv[q + 1]; p++, results++) {
        const uint32_t kind = uint32_t(tr[p] & 0xff);
        if (kind != 1 && kind != 2 && kind != 18) return 6;
        if (snapshot < PBL_SEQNUM_MAX && (tr[p] >> 8) >= snapshot) return 7;
        if (sk[p] < R.kvb[q] || sk[p] >= R.kvb[q + 1] || R.trailer[sk[p]] != tr[p] || sk[p] + ns[p] > R.kvb[q + 1]) return 8;
        if (fl[p] & ~(PBL_KV_VALBLK_HANDLE | PBL_KV_BLOB_HANDLE)) return 9;
        if (flags || p + 1 >= okv[q + 1]) continue;
        const uint8_t *a = kby + okey[q] + ko[p + q], *b = kby + okey[q] + ko[p + q + 1];
        if (pbl_key_compare(cmp, a, ko[p + q + 1] - ko[p + q], b, ko[p + q + 2] - ko[p + q + 1]) >= 0) { printf("keys not ascending, iter %d\n", iter); return 10; }
      }
    }
    free(tr); free(fl); free(ko); free(vo); free(kby); free(vby); free(sk); free(ns);
  }
  printf("ok (%llu result KVs, %llu blocks with a status)\n", (unsigned long long)results, (unsigned long long)bad);
  return 0;
}
