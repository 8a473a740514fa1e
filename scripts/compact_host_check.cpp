// compact_host_check.cpp — pbl_compact_batch_host as a stand-alone host program
// for sanitizer runs (no GPU is touched): random blocks under all three
// comparers, sorted (by pbl_key_compare, sequence numbers distinct per key),
// unsorted, bad and unsupported blocks, all six kinds, DELSIZED values that are
// the right size, a wrong one, empty or no uvarint, handle flags, random
// snapshot lists and both flags, every buffer a heap allocation of exactly its
// size, so that a read or write past an end is seen.  Checks that every result
// names a head of its source block with that head's key and sequence number
// (or 0 in the bottommost stripe), that the heads of one block ascend, that a
// block with a status reports no counts, and that an unsorted snapshot list is
// refused.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/compact.hip pebble_amd/csrc/data_iter.cpp scripts/compact_host_check.cpp \
//     -fsanitize=address,undefined -o compact_host_check && ./compact_host_check
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
struct Kv { std::string key; uint64_t trailer; };
int main() {
  std::mt19937 rng(17);
  const uint32_t kinds[] = {0, 1, 2, 7, 18, 23, 2, 7, 23, 1, 21};
  uint64_t results = 0, bad = 0, calls = 0;
  for (int iter = 0; iter < 600; iter++) {
    const uint32_t nb = 1 + rng() % 5, cmp = rng() % 3, flags = (rng() % 2 ? PBL_COMPACT_ELIDE_TOMBSTONES : 0) | (rng() % 2 ? PBL_COMPACT_BOTTOMMOST : 0);
    std::vector<uint64_t> snaps(rng() % 3 == 0 ? 0 : rng() % 9);
    for (auto& s : snaps) s = rng() % 70;
    std::sort(snaps.begin(), snaps.end());
    snaps.shrink_to_fit();
    Batch R;
    R.kvb.push_back(0); R.keyb.push_back(0); R.valb.push_back(0);
    for (uint32_t q = 0; q < nb; q++) {
      const uint32_t n = rng() % 4 == 0 ? 0 : rng() % 90;
      const bool odd_kinds = rng() % 8 == 0, handles = rng() % 6 == 0;
      std::vector<Kv> kv;
      for (uint32_t j = 0; j < n; j++) {
        std::string k(rng() % 4, 'a');
        for (auto& ch : k) ch = "ab@1\0\x09"[rng() % 6];
        kv.push_back({k, uint64_t(rng() % 64) << 8 | kinds[rng() % (odd_kinds ? 11 : 10)]});
      }
      if (rng() % 8) {
        std::sort(kv.begin(), kv.end(), [&](const Kv& a, const Kv& b) {
          const int c = pbl_key_compare(cmp, (const uint8_t*)a.key.data(), a.key.size(), (const uint8_t*)b.key.data(), b.key.size());
          return c ? c < 0 : a.trailer > b.trailer; });
        // one KV per (user key, sequence number), unless this block is to be refused
        if (rng() % 10)
          kv.erase(std::unique(kv.begin(), kv.end(), [&](const Kv& a, const Kv& b) {
            return (a.trailer >> 8) == (b.trailer >> 8) &&
                   pbl_key_compare(cmp, (const uint8_t*)a.key.data(), a.key.size(), (const uint8_t*)b.key.data(), b.key.size()) == 0; }), kv.end());
      }
      size_t k0 = R.kbytes.size(), v0 = R.vbytes.size();
      for (size_t j = 0; j < kv.size(); j++) {
        R.koff.push_back(uint32_t(R.kbytes.size() - k0)); R.voff.push_back(uint32_t(R.vbytes.size() - v0));
        R.kbytes.insert(R.kbytes.end(), kv[j].key.begin(), kv[j].key.end());
        const uint32_t kind = uint32_t(kv[j].trailer & 0xff);
        if (kind == 23) {  // a size near the next key's (values are 0..2 bytes), empty, large, or two uvarints
          const uint32_t c = rng() % 10;
          const size_t next = j + 1 < kv.size() ? kv[j + 1].key.size() : 0;
          if (c < 5) R.vbytes.push_back(uint8_t(next + rng() % 3));
          else if (c == 5) { R.vbytes.push_back(0x85); R.vbytes.push_back(0x01); }
          else if (c == 6) { R.vbytes.push_back(0x03); R.vbytes.push_back(0x04); }
          else if (c == 7) R.vbytes.insert(R.vbytes.end(), 11, uint8_t(0x80));
        } else if (kind != 0 && kind != 7) {
          R.vbytes.insert(R.vbytes.end(), rng() % 3, uint8_t('v'));
        }
        R.trailer.push_back(kv[j].trailer);
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
    pbl_compact_in in{R.c(), nb, cmp, 0, snaps.empty() ? nullptr : snaps.data(), snaps.size()};
    std::vector<uint64_t> okv(nb + 1), okey(nb + 1), oval(nb + 1); std::vector<uint32_t> ost(nb), c0(nb), c1(nb), c2(nb);
    pbl_totals T{};
    pbl_compact_out out{}; out.result.blk_kv_base = okv.data(); out.result.blk_key_base = okey.data(); out.result.blk_val_base = oval.data();
    out.result.blk_status = ost.data(); out.result.totals = &T; out.n_missized = c0.data(); out.n_ineffectual = c1.data(); out.n_nondeterministic = c2.data();
    if (pbl_compact_batch_host(&in, &out, flags) != PBL_OK) return 1;
    const uint64_t n = T.n_kv, kb = T.key_bytes, vb = T.val_bytes;
    uint64_t* tr = (uint64_t*)malloc(n * 8 + 1); uint8_t* fl = (uint8_t*)malloc(n + 1); uint32_t* ko = (uint32_t*)malloc((n + nb) * 4);
    uint32_t* vo = (uint32_t*)malloc((n + nb) * 4); uint8_t* kby = (uint8_t*)malloc(kb + 1); uint8_t* vby = (uint8_t*)malloc(vb + 1);
    uint64_t* sk = (uint64_t*)malloc(n * 8 + 1); uint32_t* ns = (uint32_t*)malloc(n * 4 + 1); uint8_t* pin = (uint8_t*)malloc(n + 1);
    out.result.trailer = tr; out.result.kv_flags = fl; out.result.key_off = ko; out.result.val_off = vo; out.result.key_bytes = kby;
    out.result.val_bytes = vby; out.result.kv_cap = n; out.result.key_cap = kb; out.result.val_cap = vb; out.src_kv = sk; out.n_src = ns; out.pinned = pin;
    if (pbl_compact_batch_host(&in, &out, flags) != PBL_OK) return 2;
    if (T.n_kv != n || (T.status_mask & (1u << PBL_OVERFLOW))) return 3;
    for (uint32_t q = 0; q < nb; q++) {
      if (ost[q] != PBL_OK) { bad++; if (okv[q + 1] != okv[q] || c0[q] || c1[q] || c2[q]) return 4; continue; }
      calls += c0[q] + c1[q] + c2[q];
      if (vo[okv[q + 1] + q] != oval[q + 1] - oval[q] || ko[okv[q + 1] + q] != okey[q + 1] - okey[q]) return 5;
      for (uint64_t p = okv[q]; p < okv[q + 1]; p++, results++) {
        const uint32_t kind = uint32_t(tr[p] & 0xff);
        if (kind != 0 && kind != 1 && kind != 2 && kind != 7 && kind != 18 && kind != 23) return 6;
        if (sk[p] < R.kvb[q] || sk[p] >= R.kvb[q + 1] || ns[p] < 1 || sk[p] + ns[p] > R.kvb[q + 1] || pin[p] > 1) return 7;
        const uint64_t hseq = R.trailer[sk[p]] >> 8;
        if ((tr[p] >> 8) != hseq && !((flags & PBL_COMPACT_BOTTOMMOST) && (tr[p] >> 8) == 0)) return 8;
        if (fl[p] & ~(PBL_KV_VALBLK_HANDLE | PBL_KV_BLOB_HANDLE)) return 9;
        const uint32_t hk0 = R.koff[sk[p] + q], hk1 = R.koff[sk[p] + q + 1];
        if (ko[p + q + 1] - ko[p + q] != hk1 - hk0 || memcmp(kby + okey[q] + ko[p + q], R.kbytes.data() + R.keyb[q] + hk0, hk1 - hk0)) return 10;
        if (p + 1 < okv[q + 1] && sk[p + 1] <= sk[p]) { printf("heads not ascending, iter %d\n", iter); return 11; }
      }
    }
    // an unsorted snapshot list is refused
    if (snaps.size() >= 2 && snaps.front() != snaps.back()) {
      std::reverse(snaps.begin(), snaps.end());
      if (pbl_compact_batch_host(&in, &out, flags) != PBL_INVALID_ARG) return 12;
    }
    free(tr); free(fl); free(ko); free(vo); free(kby); free(vby); free(sk); free(ns); free(pin);
  }
  printf("ok (%llu result KVs, %llu blocks with a status, %llu counted calls)\n", (unsigned long long)results, (unsigned long long)bad,
         (unsigned long long)calls);
  return 0;
}
