// merge_host_check.cpp — pbl_merge_batch_host as a stand-alone host program for
// sanitizer runs (no GPU is touched): random runs under all three comparers,
// sorted, unsorted and bad blocks, every buffer a heap allocation of exactly its
// size, so that a read or write past an end is seen.  Checks that every result
// block is in mergingIter order with ties in run order.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/merge.hip pebble_amd/csrc/data_iter.cpp scripts/merge_host_check.cpp \
//     -fsanitize=address,undefined -o merge_host_check && ./merge_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"
struct Run {
  std::vector<uint64_t> trailer, kvb, keyb, valb; std::vector<uint8_t> flags, kbytes, vbytes;
  std::vector<uint32_t> koff, voff, status;
  pbl_decode_out c() { pbl_decode_out d{}; d.trailer = trailer.data(); d.kv_flags = flags.data(); d.key_off = koff.data(); d.val_off = voff.data();
    d.key_bytes = kbytes.data(); d.val_bytes = vbytes.data(); d.blk_kv_base = kvb.data(); d.blk_key_base = keyb.data(); d.blk_val_base = valb.data();
    d.blk_status = status.data(); return d; }
};
int main() {
  std::mt19937 rng(7);
  for (int iter = 0; iter < 200; iter++) {
    const uint32_t K = 1 + rng() % 16, nb = 1 + rng() % 5, cmp = rng() % 3;
    std::vector<Run> runs(K);
    for (auto& R : runs) {
      R.kvb.push_back(0); R.keyb.push_back(0); R.valb.push_back(0);
      for (uint32_t q = 0; q < nb; q++) {
        const uint32_t n = rng() % 4 == 0 ? 0 : rng() % 70;
        std::vector<std::pair<std::string, uint64_t>> kv;
        for (uint32_t j = 0; j < n; j++) {
          std::string k(rng() % 20, 'a');
          for (auto& ch : k) ch = "ab@1\0\x09"[rng() % 6];
          kv.push_back({k, uint64_t(rng() % 50) << 8 | 1});
        }
        if (cmp == 0 && rng() % 8) std::sort(kv.begin(), kv.end(), [](auto& a, auto& b) { return a.first != b.first ? a.first < b.first : a.second > b.second; });
        size_t k0 = R.kbytes.size(), v0 = R.vbytes.size();
        for (auto& x : kv) {
          R.koff.push_back(uint32_t(R.kbytes.size() - k0)); R.voff.push_back(uint32_t(R.vbytes.size() - v0));
          R.kbytes.insert(R.kbytes.end(), x.first.begin(), x.first.end());
          R.vbytes.insert(R.vbytes.end(), rng() % 30, uint8_t('v'));
          R.trailer.push_back(x.second); R.flags.push_back(0);
        }
        R.koff.push_back(uint32_t(R.kbytes.size() - k0)); R.voff.push_back(uint32_t(R.vbytes.size() - v0));
        R.status.push_back(rng() % 10 == 0 ? PBL_CORRUPT_BOUNDS : PBL_OK);
        R.kvb.push_back(R.trailer.size()); R.keyb.push_back(R.kbytes.size()); R.valb.push_back(R.vbytes.size());
      }
      // exact sizes: shrink so that ASan sees every byte past the end
      R.kbytes.shrink_to_fit(); R.vbytes.shrink_to_fit();
      if (R.trailer.empty()) { R.trailer.reserve(1); R.flags.reserve(1); }
      if (R.kbytes.empty()) R.kbytes.reserve(1);
      if (R.vbytes.empty()) R.vbytes.reserve(1);
    }
    std::vector<pbl_decode_out> cs;
    for (auto& R : runs) cs.push_back(R.c());
    pbl_merge_runs in{cs.data(), K, nb, cmp, 0, 0};
    std::vector<uint64_t> okv(nb + 1), okey(nb + 1), oval(nb + 1); std::vector<uint32_t> ost(nb);
    pbl_totals T{};
    pbl_merge_out out{}; out.result.blk_kv_base = okv.data(); out.result.blk_key_base = okey.data(); out.result.blk_val_base = oval.data();
    out.result.blk_status = ost.data(); out.result.totals = &T;
    if (pbl_merge_batch_host(&in, &out) != PBL_OK) return 1;
    const uint64_t n = T.n_kv, kb = T.key_bytes, vb = T.val_bytes;
    uint64_t* tr = (uint64_t*)malloc(n * 8 + 1); uint8_t* fl = (uint8_t*)malloc(n + 1); uint32_t* ko = (uint32_t*)malloc((n + nb) * 4);
    uint32_t* vo = (uint32_t*)malloc((n + nb) * 4); uint8_t* kby = (uint8_t*)malloc(kb + 1); uint8_t* vby = (uint8_t*)malloc(vb + 1);
    uint8_t* sr = (uint8_t*)malloc(n + 1); uint64_t* sk = (uint64_t*)malloc(n * 8 + 1);
    out.result.trailer = tr; out.result.kv_flags = fl; out.result.key_off = ko; out.result.val_off = vo; out.result.key_bytes = kby;
    out.result.val_bytes = vby; out.result.kv_cap = n; out.result.key_cap = kb; out.result.val_cap = vb; out.src_run = sr; out.src_kv = sk;
    if (pbl_merge_batch_host(&in, &out) != PBL_OK) return 2;
    if (T.n_kv != n || (T.status_mask & (1u << PBL_OVERFLOW))) return 3;
    for (uint32_t q = 0; q < nb; q++)
      for (uint64_t p = okv[q]; p + 1 < okv[q + 1]; p++) {
        const uint8_t *a = kby + okey[q] + ko[p + q], *b = kby + okey[q] + ko[p + q + 1];
        const int c = pbl_key_compare(cmp, a, ko[p + q + 1] - ko[p + q], b, ko[p + q + 2] - ko[p + q + 1]);
        if (c > 0 || (c == 0 && tr[p] < tr[p + 1])) { printf("unsorted result iter %d\n", iter); return 4; }
        if (c == 0 && tr[p] == tr[p + 1] && sr[p] > sr[p + 1]) return 5;
      }
    free(tr); free(fl); free(ko); free(vo); free(kby); free(vby); free(sr); free(sk);
  }
  printf("ok\n");
  return 0;
}
