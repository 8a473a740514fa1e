// rangekey_host_check.cpp — pbl_rangekey_set_host, pbl_rangekey_clip_host,
// pbl_rangekey_mask_set_host and pbl_rangekey_mask_host as a stand-alone host
// program for sanitizer runs (no GPU is touched): random range-key runs under
// all three comparers, valid (fragmented by construction) and broken ones
// (unsorted, overlapping, another kind, a bad status), every buffer a heap
// allocation of exactly its size, so that a read or write past an end is seen.
// Checks that the set's spans ascend and do not overlap, that a span's suffixes
// ascend strictly under pbl_range_suffix_compare, that the sizes-only call and
// the full call agree, that the unbounded clip is the set, and that the mask
// through the set equals the mask through the runs (the two share no code path
// past the validation and the coalescing of one key list).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/rangekey.hip pebble_amd/csrc/data_iter.cpp scripts/rangekey_host_check.cpp \
//     -fsanitize=address,undefined -o rangekey_host_check && ./rangekey_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"

template <class T>
static T* exact(std::vector<T>& v) {  // a heap block of exactly the vector's size (at least one element)
  v.shrink_to_fit();
  if (v.empty()) v.reserve(1);
  return v.data();
}

struct Batch {  // one block, with extras
  std::vector<uint64_t> trailer, kvb, keyb, valb, sufb, xvb;
  std::vector<uint8_t> flags, kbytes, vbytes, sbytes, xbytes;
  std::vector<uint32_t> koff, voff, soff, xoff, span, status;
  void add(const std::string& k, uint64_t tr, const std::string& v, const std::string& sfx = "", const std::string& val = "") {
    koff.push_back(uint32_t(kbytes.size())); voff.push_back(uint32_t(vbytes.size()));
    soff.push_back(uint32_t(sbytes.size())); xoff.push_back(uint32_t(xbytes.size()));
    kbytes.insert(kbytes.end(), k.begin(), k.end()); vbytes.insert(vbytes.end(), v.begin(), v.end());
    sbytes.insert(sbytes.end(), sfx.begin(), sfx.end()); xbytes.insert(xbytes.end(), val.begin(), val.end());
    trailer.push_back(tr); flags.push_back(0); span.push_back(0);
  }
  pbl_decode_out c(uint32_t st = PBL_OK) {
    koff.push_back(uint32_t(kbytes.size())); voff.push_back(uint32_t(vbytes.size()));
    soff.push_back(uint32_t(sbytes.size())); xoff.push_back(uint32_t(xbytes.size()));
    kvb = {0, trailer.size()}; keyb = {0, kbytes.size()}; valb = {0, vbytes.size()}; status = {st};
    sufb = {0, sbytes.size()}; xvb = {0, xbytes.size()};
    pbl_decode_out d{};
    d.trailer = exact(trailer); d.kv_flags = exact(flags); d.key_off = exact(koff); d.val_off = exact(voff);
    d.key_bytes = exact(kbytes); d.val_bytes = exact(vbytes); d.blk_kv_base = kvb.data(); d.blk_key_base = keyb.data();
    d.blk_val_base = valb.data(); d.blk_status = status.data();
    return d;
  }
  pbl_keyspan_extra x() {
    pbl_keyspan_extra e{};
    e.span = exact(span); e.suffix_off = exact(soff); e.value_off = exact(xoff); e.suffix_bytes = exact(sbytes);
    e.value_bytes = exact(xbytes); e.blk_suffix_base = sufb.data(); e.blk_value_base = xvb.data();
    return e;
  }
};

struct Out {  // a result with extras, nb blocks, allocated exactly at the offered capacities
  std::vector<uint64_t> trailer, kvb, keyb, valb, rstb, sufb, xvb;
  std::vector<uint8_t> flags, kbytes, vbytes, sbytes, xbytes;
  std::vector<uint32_t> koff, voff, soff, xoff, span, entry, status;
  pbl_totals tot{};
  pbl_decode_out d{};
  pbl_keyspan_extra e{};
  Out(uint32_t nb, uint64_t kv, uint64_t kb, uint64_t vb, uint64_t sb, uint64_t xb, bool arrays) {
    kvb.assign(nb + 1, 0); keyb = valb = rstb = sufb = xvb = kvb; status.assign(nb ? nb : 1, 0);
    d.blk_kv_base = kvb.data(); d.blk_key_base = keyb.data(); d.blk_val_base = valb.data(); d.blk_rst_base = rstb.data();
    d.blk_status = status.data(); d.totals = &tot;
    e.blk_suffix_base = sufb.data(); e.blk_value_base = xvb.data();
    if (!arrays) return;
    trailer.assign(kv, 0); flags.assign(kv, 0); span.assign(kv, 0); entry.assign(kv, 0);
    koff.assign(kv + nb, 0); voff = soff = xoff = koff;
    kbytes.assign(kb, 0); vbytes.assign(vb, 0); sbytes.assign(sb, 0); xbytes.assign(xb, 0);
    d.trailer = exact(trailer); d.kv_flags = exact(flags); d.entry_off = exact(entry); d.key_off = exact(koff);
    d.val_off = exact(voff); d.key_bytes = exact(kbytes); d.val_bytes = exact(vbytes);
    d.kv_cap = kv; d.key_cap = kb; d.val_cap = vb;
    e.span = exact(span); e.suffix_off = exact(soff); e.value_off = exact(xoff); e.suffix_bytes = exact(sbytes);
    e.value_bytes = exact(xbytes); e.suffix_cap = sb; e.value_cap = xb;
  }
  std::string key(uint64_t i) const { return std::string((const char*)kbytes.data() + koff[i], koff[i + 1] - koff[i]); }
  std::string end(uint64_t i) const { return std::string((const char*)vbytes.data() + voff[i], voff[i + 1] - voff[i]); }
  std::string suffix(uint64_t i) const { return std::string((const char*)sbytes.data() + soff[i], soff[i + 1] - soff[i]); }
};

static int cmpk(uint32_t c, const std::string& a, const std::string& b) {
  return pbl_key_compare(c, (const uint8_t*)a.data(), a.size(), (const uint8_t*)b.data(), b.size());
}
static int cmps(uint32_t c, const std::string& a, const std::string& b) {
  return pbl_range_suffix_compare(c, (const uint8_t*)a.data(), a.size(), (const uint8_t*)b.data(), b.size());
}
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s (line %d, iteration %d)\n", #x, __LINE__, iter); return 1; } } while (0)

int main() {
  std::mt19937 rng(31);
  uint64_t spans = 0, with_status = 0, masked = 0, joined = 0;
  for (int iter = 0; iter < 600; iter++) {
    const uint32_t cmp = rng() % 3, nr = rng() % 5;
    const uint64_t snapshot = rng() % 4 == 0 ? PBL_SEQNUM_MAX : rng() % 60;
    const int breakage = rng() % 4 == 0 ? 1 + rng() % 4 : 0;
    auto suffix = [&](uint32_t i) -> std::string {
      if (i == 0) return "";
      if (cmp == PBL_CMP_TESTKEYS) return "@" + std::to_string(i) + (rng() % 8 == 0 ? "_synthetic" : "");
      if (cmp == PBL_CMP_CRDB) return std::string(7, '\0') + char(i) + "\x09";
      return "s" + std::to_string(i);
    };
    // boundary keys, ascending under the comparer, without suffixes
    std::vector<std::string> pool;
    for (int i = 0; i < 24; i++) pool.push_back(std::string(1, char('a' + i)) + (cmp == PBL_CMP_CRDB ? std::string(1, '\0') : ""));
    std::vector<Batch> runs(nr);
    std::vector<pbl_decode_out> rc;
    std::vector<pbl_keyspan_extra> rx;
    std::vector<uint64_t> nkv;
    for (uint32_t r = 0; r < nr; r++) {
      size_t at = rng() % 4;
      while (at + 1 < pool.size() && rng() % 9) {
        const size_t to = std::min(pool.size() - 1, at + 1 + rng() % 3);
        std::vector<uint64_t> trs;
        for (int k = 1 + rng() % 3; k > 0; k--) trs.push_back(uint64_t(1 + rng() % 50) << 8 | (19 + rng() % 3));
        std::sort(trs.rbegin(), trs.rend());
        const std::string end = rng() % 20 == 0 ? pool[at] : pool[to];  // (sometimes an empty fragment)
        for (uint64_t tr : trs)
          runs[r].add(pool[at], tr, end, (tr & 0xff) == 19 ? "" : suffix(rng() % 4),
                      (tr & 0xff) == 21 ? std::string(rng() % 3, 'v') : "");
        at = to + rng() % 2;
      }
    }
    if (breakage && nr) {
      Batch& b = runs[rng() % nr];
      if (b.trailer.empty()) b.add("a", 5 << 8 | 21, "b", "", "");
      if (breakage == 1) b.trailer[0] = (b.trailer[0] & ~0xffull) | 15;                  // another kind
      if (breakage == 2) { b.add("a", 5 << 8 | 21, "b"); b.add("a", 5 << 8 | 21, "c"); }  // unsorted or unequal ends
      if (breakage == 3) b.flags[0] = PBL_KV_INVALID_KEY;
    }
    for (uint32_t r = 0; r < nr; r++) {
      rc.push_back(runs[r].c(breakage == 4 && r == 0 ? PBL_CORRUPT_BOUNDS : PBL_OK));
      rx.push_back(runs[r].x());
      nkv.push_back(runs[r].trailer.size());
    }
    pbl_rangekey_runs in{rc.data(), rx.data(), nkv.data(), nr, cmp, snapshot};
    // sizes only, then exactly
    Out sz(1, 0, 0, 0, 0, 0, false);
    CHECK(pbl_rangekey_set_host(&in, &sz.d, &sz.e) == PBL_OK);
    Out set(1, sz.tot.n_kv, sz.tot.key_bytes, sz.tot.val_bytes, sz.sufb[1], sz.xvb[1], true);
    CHECK(pbl_rangekey_set_host(&in, &set.d, &set.e) == PBL_OK);
    CHECK(set.tot.n_kv == sz.tot.n_kv && set.tot.key_bytes == sz.tot.key_bytes && set.sufb[1] == sz.sufb[1]);
    CHECK(!(set.tot.status_mask & 1u << PBL_OVERFLOW));
    const uint64_t n = set.tot.n_kv;
    if (set.status[0] != PBL_OK) { with_status++; CHECK(n == 0); }
    if (n) {  // one capacity too small: sizes and no bytes
      Out small(1, n - 1, sz.tot.key_bytes, sz.tot.val_bytes, sz.sufb[1], sz.xvb[1], true);
      CHECK(pbl_rangekey_set_host(&in, &small.d, &small.e) == PBL_OK);
      CHECK((small.tot.status_mask & 1u << PBL_OVERFLOW) && small.tot.n_kv == n);
    }
    for (uint64_t i = 0; i < n; i++) {
      CHECK(cmpk(cmp, set.key(i), set.end(i)) < 0 && (set.trailer[i] & 0xff) == 21 && set.span[i] <= i);
      if (set.span[i] == i) spans++;
      if (i == 0) continue;
      if (set.span[i] == set.span[i - 1]) {  // the same span: suffixes ascend strictly
        CHECK(set.key(i) == set.key(i - 1) && set.end(i) == set.end(i - 1) && set.entry[i] == set.entry[i - 1]);
        CHECK(cmps(cmp, set.suffix(i - 1), set.suffix(i)) < 0);
      } else {
        CHECK(set.span[i] == i && set.entry[i] == set.entry[i - 1] + 1 && cmpk(cmp, set.end(i - 1), set.key(i)) <= 0);
      }
    }
    // the unbounded clip is the set; a range inside the keys truncates
    const std::string lo2 = pool[3], up2 = pool[15];
    std::vector<uint8_t> lob(lo2.begin(), lo2.end()), upb(up2.begin(), up2.end());
    const uint64_t lo_off[3] = {0, 0, lo2.size()}, up_off[3] = {0, 0, up2.size()};
    const uint8_t fl[2] = {PBL_SCAN_NO_UPPER, 0};
    pbl_scan_queries q{};
    q.lower_bytes = exact(lob); q.lower_off = lo_off; q.upper_bytes = exact(upb); q.upper_off = up_off; q.flags = fl;
    q.n = 2; q.comparer = cmp;
    Out csz(2, 0, 0, 0, 0, 0, false);
    CHECK(pbl_rangekey_clip_host(&set.d, &set.e, &q, &csz.d, &csz.e) == PBL_OK);
    Out clip(2, csz.tot.n_kv, csz.tot.key_bytes, csz.tot.val_bytes, csz.sufb[2], csz.xvb[2], true);
    CHECK(pbl_rangekey_clip_host(&set.d, &set.e, &q, &clip.d, &clip.e) == PBL_OK);
    CHECK(clip.kvb[1] == n && clip.keyb[1] == set.tot.key_bytes && clip.status[0] == set.status[0]);
    for (uint64_t i = 0; i < n; i++) CHECK(clip.trailer[i] == set.trailer[i] && clip.span[i] == set.span[i]);
    for (uint64_t i = clip.kvb[1]; i < clip.kvb[2]; i++) {
      const uint64_t o = i + 1;
      const std::string k((const char*)clip.kbytes.data() + clip.keyb[1] + clip.koff[o], clip.koff[o + 1] - clip.koff[o]);
      const std::string e((const char*)clip.vbytes.data() + clip.valb[1] + clip.voff[o], clip.voff[o + 1] - clip.voff[o]);
      CHECK(cmpk(cmp, lo2, k) <= 0 && cmpk(cmp, e, up2) <= 0 && cmpk(cmp, k, e) < 0);
    }
    // the mask: through the set, and through the runs
    Batch pts;
    for (int i = 0; i < 60; i++) {
      std::string k = pool[rng() % pool.size()];
      if (cmp == PBL_CMP_TESTKEYS && rng() % 5) k += "@" + std::to_string(rng() % 6);
      if (cmp == PBL_CMP_CRDB && rng() % 5) k += std::string(7, '\0') + char(rng() % 6) + "\x09";
      pts.add(k, 7 << 8 | 1, "v");
    }
    pbl_decode_out pc = pts.c();
    const std::string t = suffix(rng() % 4);
    std::vector<uint64_t> a(60, 3), b(60, 3);
    uint32_t st = 99;
    CHECK(pbl_rangekey_mask_host(&in, &pc, 1, (const uint8_t*)t.data(), t.size(), exact(a), &st) == PBL_OK);
    CHECK(st == set.status[0]);
    CHECK(pbl_rangekey_mask_set_host(&set.d, &set.e, &pc, 1, cmp, (const uint8_t*)t.data(), t.size(), exact(b)) == PBL_OK);
    for (int i = 0; i < 60; i++) {
      CHECK(a[i] == b[i] && (a[i] == 3 || a[i] == PBL_RANGEDEL_ALL));
      if (a[i] != 3) masked++;
    }
    for (uint64_t i = 1; i < n; i++)
      if (set.span[i] == i && set.end(i - 1) == set.key(i)) joined++;  // (abutting spans that did not join)
  }
  printf("rangekey host check: %llu spans, %llu abutting, %llu sets with a status, %llu masked points: OK\n",
         (unsigned long long)spans, (unsigned long long)joined, (unsigned long long)with_status, (unsigned long long)masked);
  return spans > 100 && with_status > 20 && masked > 100 ? 0 : 2;
}
