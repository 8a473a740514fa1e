// rangedel_host_check.cpp — pbl_rangedel_set_host, pbl_rangedel_cover_host and
// pbl_visible_batch_host_rd as a stand-alone host program for sanitizer runs (no
// GPU is touched): random runs under all three comparers, valid (fragmented by
// construction), and broken ones (unsorted, overlapping, inverted, another kind,
// a bad status), every buffer a heap allocation of exactly its size, so that a
// read or write past an end is seen.  Checks that the set's boundaries ascend
// strictly, that its last cover is 0, that the cover of a batch made of the
// boundaries equals the set's trailers (the two host functions share no
// code path past the validation), and that the view with that cover holds no KV
// under a newer tombstone.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/rangedel.hip pebble_amd/csrc/visible.hip pebble_amd/csrc/data_iter.cpp \
//     scripts/rangedel_host_check.cpp -fsanitize=address,undefined -o rangedel_host_check && ./rangedel_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"
struct Batch {  // one block
  std::vector<uint64_t> trailer, kvb, keyb, valb; std::vector<uint8_t> flags, kbytes, vbytes;
  std::vector<uint32_t> koff, voff, status;
  void add(const std::string& k, uint64_t tr, const std::string& v) {
    koff.push_back(uint32_t(kbytes.size())); voff.push_back(uint32_t(vbytes.size()));
    kbytes.insert(kbytes.end(), k.begin(), k.end()); vbytes.insert(vbytes.end(), v.begin(), v.end());
    trailer.push_back(tr); flags.push_back(0);
  }
  pbl_decode_out c(uint32_t st = PBL_OK) {
    koff.push_back(uint32_t(kbytes.size())); voff.push_back(uint32_t(vbytes.size()));
    kvb = {0, trailer.size()}; keyb = {0, kbytes.size()}; valb = {0, vbytes.size()}; status = {st};
    // exact sizes: shrink so that ASan sees every byte past the end
    kbytes.shrink_to_fit(); vbytes.shrink_to_fit(); trailer.shrink_to_fit(); flags.shrink_to_fit(); koff.shrink_to_fit(); voff.shrink_to_fit();
    if (trailer.empty()) { trailer.reserve(1); flags.reserve(1); }
    if (kbytes.empty()) kbytes.reserve(1);
    if (vbytes.empty()) vbytes.reserve(1);
    pbl_decode_out d{}; d.trailer = trailer.data(); d.kv_flags = flags.data(); d.key_off = koff.data(); d.val_off = voff.data();
    d.key_bytes = kbytes.data(); d.val_bytes = vbytes.data(); d.blk_kv_base = kvb.data(); d.blk_key_base = keyb.data(); d.blk_val_base = valb.data();
    d.blk_status = status.data(); return d; }
};
static int cmpk(uint32_t c, const std::string& a, const std::string& b) {
  return pbl_key_compare(c, (const uint8_t*)a.data(), a.size(), (const uint8_t*)b.data(), b.size());
}
int main() {
  std::mt19937 rng(29);
  uint64_t boundaries = 0, with_status = 0, deleted = 0;
  for (int iter = 0; iter < 600; iter++) {
    const uint32_t cmp = rng() % 3, nr = rng() % 5;
    const uint64_t snapshot = rng() % 4 == 0 ? PBL_SEQNUM_MAX : rng() % 60;
    const int breakage = rng() % 4 == 0 ? 1 + rng() % 5 : 0;
    std::vector<Batch> runs(nr);
    std::vector<pbl_decode_out> rc;
    std::vector<uint64_t> nkv;
    std::vector<std::string> pool;
    for (int i = 0; i < 40; i++) {
      std::string k(rng() % 6, 'a');
      for (auto& ch : k) ch = "ab@1\0\x09"[rng() % 6];
      pool.push_back(k);
    }
    std::sort(pool.begin(), pool.end(), [&](auto& a, auto& b) { return cmpk(cmp, a, b) < 0; });
    pool.erase(std::unique(pool.begin(), pool.end(), [&](auto& a, auto& b) { return cmpk(cmp, a, b) == 0; }), pool.end());
    if (pool.size() < 3) continue;
    for (uint32_t r = 0; r < nr; r++) {
      // disjoint fragments over the pool, some repeated with descending trailers
      for (size_t i = 0; i + 1 < pool.size() && rng() % 6;) {
        const size_t j = i + 1 + rng() % 2;
        if (j >= pool.size()) break;
        uint64_t seq = 10 + rng() % 50;
        for (int rep = 1 + rng() % 3; rep > 0 && seq > 0; rep--, seq -= 1 + rng() % 3) runs[r].add(pool[i], seq << 8 | 15, pool[j]);
        i = j + rng() % 2;
      }
      if (breakage == 1 && r == 0 && runs[r].trailer.size() > 1) std::swap(runs[r].trailer[0], runs[r].trailer.back()), runs[r].add(pool[0], 5 << 8 | 15, pool[1]);
      if (breakage == 2 && r == 0) runs[r].add(pool.back(), 5 << 8 | 15, pool[0]);
      if (breakage == 3 && r == 0) runs[r].add(pool[0], 5 << 8 | 1, pool.back());
      rc.push_back(runs[r].c(breakage == 4 && r == 0 ? PBL_CORRUPT_BOUNDS : PBL_OK));
      nkv.push_back(runs[r].trailer.size() - (breakage == 5 && r == 0 && !runs[r].trailer.empty() ? 1 : 0));
    }
    rc.shrink_to_fit(); nkv.shrink_to_fit();
    // levels for every other iteration (exact-size array)
    std::vector<uint8_t> lvl(nr);
    for (auto& x : lvl) x = uint8_t(rng() % 4);
    lvl.shrink_to_fit();
    const bool leveled = iter % 2 == 1 && nr > 0;
    pbl_rangedel_runs in{rc.data(), nkv.data(), nr, cmp, snapshot, leveled ? lvl.data() : nullptr};
    uint64_t T = 0, bytes = 0;
    for (uint32_t r = 0; r < nr; r++) { T += nkv[r]; bytes += runs[r].kbytes.size() + runs[r].vbytes.size(); }
    // the set, into buffers of exactly the documented bounds
    uint64_t okv[2], okey[2], oval[2]; uint32_t ost[1]; pbl_totals tot{};
    uint64_t* tr = (uint64_t*)malloc(2 * T * 8 + 1); uint8_t* fl = (uint8_t*)malloc(2 * T + 1); uint32_t* ko = (uint32_t*)malloc((2 * T + 1) * 4);
    uint32_t* vo = (uint32_t*)malloc((2 * T + 1) * 4); uint8_t* kby = (uint8_t*)malloc(bytes + 1); uint8_t* vby = (uint8_t*)malloc(1);
    pbl_decode_out set{}; set.trailer = tr; set.kv_flags = fl; set.key_off = ko; set.val_off = vo; set.key_bytes = kby; set.val_bytes = vby;
    set.blk_kv_base = okv; set.blk_key_base = okey; set.blk_val_base = oval; set.blk_status = ost; set.totals = &tot;
    set.kv_cap = 2 * T; set.key_cap = bytes; set.val_cap = 0;
    if (pbl_rangedel_set_host(&in, &set) != PBL_OK) return 1;
    if (tot.status_mask & (1u << PBL_OVERFLOW)) return 2;
    const uint64_t n = tot.n_kv;
    if (ost[0] != PBL_OK) { with_status++; if (n) return 3; }
    if (breakage >= 2 && breakage <= 4 && nr && ost[0] == PBL_OK) return 4;
    if (ko[n] != tot.key_bytes || vo[n] != 0 || okv[1] != n) return 5;
    for (uint64_t i = 0; i + 1 < n; i++)
      if (pbl_key_compare(cmp, kby + ko[i], ko[i + 1] - ko[i], kby + ko[i + 1], ko[i + 2] - ko[i + 1]) >= 0) return 6;
    if (n && (tr[n - 1] >> 8) != 0) return 7;
    boundaries += n;
    // a batch of the boundaries, two versions each: its cover by the runs equals the set's trailers
    Batch P;
    for (uint64_t i = 0; i < n; i++)
      for (int v = 0; v < 2; v++) P.add(std::string((const char*)kby + ko[i], ko[i + 1] - ko[i]), uint64_t(40 - 25 * v) << 8 | (rng() % 3 ? 1 : 2), "v");
    pbl_decode_out pc = P.c();
    uint64_t* cov = (uint64_t*)malloc(2 * n * 8 + 1);
    uint32_t st = 99;
    if (pbl_rangedel_cover_host(&in, &pc, 1, cov, &st) != PBL_OK || st != ost[0]) return 8;
    if (leveled) {  // the leveled cover is the plain one or PBL_RANGEDEL_ALL, and never less
      uint8_t* src = (uint8_t*)malloc(2 * n + 1);
      uint64_t* cl = (uint64_t*)malloc(2 * n * 8 + 1);
      uint8_t table[PBL_RANGEDEL_MAX_RUNS];
      for (auto& x : table) x = uint8_t(rng() % 4);
      for (uint64_t i = 0; i < 2 * n; i++) src[i] = uint8_t(rng() % PBL_RANGEDEL_MAX_RUNS);
      if (pbl_rangedel_cover_host_lv(&in, &pc, 1, src, table, cl, &st) != PBL_OK) return 14;
      for (uint64_t i = 0; i < 2 * n; i++)
        if (cl[i] != cov[i] && (cl[i] != PBL_RANGEDEL_ALL || cov[i] == 0)) return 15;
      free(src); free(cl);
    }
    for (uint64_t i = 0; i < 2 * n; i++)
      if (cov[i] != (tr[i / 2] >> 8)) { printf("cover %llu of boundary %llu, iter %d\n", (unsigned long long)cov[i], (unsigned long long)i / 2, iter); return 9; }
    // the view with that cover
    pbl_visible_in vin{pc, 1, cmp, 0, snapshot};
    uint64_t rkv[2], rkey[2], rval[2]; uint32_t rst[1]; pbl_totals rt{};
    pbl_visible_out out{}; out.result.blk_kv_base = rkv; out.result.blk_key_base = rkey; out.result.blk_val_base = rval;
    out.result.blk_status = rst; out.result.totals = &rt;
    const uint32_t flags = rng() % 2 ? PBL_VISIBLE_KEEP_OPERANDS : 0;
    if (pbl_visible_batch_host_rd(&vin, &out, flags, cov) != PBL_OK) return 10;
    const uint64_t m = rt.n_kv;
    uint64_t* rtr = (uint64_t*)malloc(m * 8 + 1); uint32_t* rko = (uint32_t*)malloc((m + 1) * 4); uint32_t* rvo = (uint32_t*)malloc((m + 1) * 4);
    uint8_t* rkb = (uint8_t*)malloc(rt.key_bytes + 1); uint8_t* rvb = (uint8_t*)malloc(rt.val_bytes + 1); uint64_t* sk = (uint64_t*)malloc(m * 8 + 1);
    out.result.trailer = rtr; out.result.key_off = rko; out.result.val_off = rvo; out.result.key_bytes = rkb; out.result.val_bytes = rvb;
    out.result.kv_cap = m; out.result.key_cap = rt.key_bytes; out.result.val_cap = rt.val_bytes; out.src_kv = sk;
    if (pbl_visible_batch_host_rd(&vin, &out, flags, cov) != PBL_OK || rt.n_kv != m || (rt.status_mask & (1u << PBL_OVERFLOW))) return 11;
    for (uint64_t p = 0; p < m; p++) {
      if (sk[p] >= 2 * n || cov[sk[p]] > (rtr[p] >> 8)) return 12;
      if (snapshot < PBL_SEQNUM_MAX && (rtr[p] >> 8) >= snapshot) return 13;
    }
    for (uint64_t i = 0; i < 2 * n; i++) deleted += cov[i] > (P.trailer[i] >> 8);
    free(tr); free(fl); free(ko); free(vo); free(kby); free(vby); free(cov); free(rtr); free(rko); free(rvo); free(rkb); free(rvb); free(sk);
  }
  printf("ok (%llu boundaries, %llu sets with a status, %llu deleted KVs)\n", (unsigned long long)boundaries, (unsigned long long)with_status,
         (unsigned long long)deleted);
  return 0;
}
