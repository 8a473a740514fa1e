// filter_host_check.cpp — pbl_bloom_build_host, pbl_filter_probe_host and
// pbl_seek_prefix_batch_host as a stand-alone host program for sanitizer runs
// (no GPU is touched): random key sets under all three comparers at 1 to 20
// bits per key, every buffer a heap allocation of exactly its size, so that a
// read past a key's or a filter's end or a write past an output is seen.
// Checks that no member is excluded (a bloom filter has no false negatives),
// that named mode equals the all-pairs row of the named filter, that empty,
// corrupt and out-of-range filters answer as include/pebble_amd.h says, that
// the builder's bound holds, and that the filtered seek equals the plain one
// wherever PBL_SEEK_FILTERED is clear and excludes no exact hit.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/filter.hip pebble_amd/csrc/seek.hip scripts/filter_host_check.cpp \
//     -fsanitize=address,undefined -o filter_host_check && ./filter_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

template <class T>
static T* exact(std::vector<T>& v) {  // a heap block of exactly the vector's size (at least one element)
  v.shrink_to_fit();
  if (v.empty()) v.reserve(1);
  return v.data();
}

struct Keys {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> off{0};
  void add(const std::string& k) {
    bytes.insert(bytes.end(), k.begin(), k.end());
    off.push_back(bytes.size());
  }
  uint64_t n() const { return off.size() - 1; }
};

static std::string make_key(std::mt19937& rng, uint32_t cmp, uint32_t i, bool member) {
  std::string k = (member ? "k" : "x") + std::to_string(i * 7919u % 100003u);
  if (rng() % 4 == 0) k.push_back(char(0x80 + rng() % 128));  // tail bytes that sign-extend
  k.resize(k.size() + rng() % 3, char(0xff));
  if (cmp == PBL_CMP_TESTKEYS && rng() % 2) k += "@" + std::to_string(rng() % 50);
  if (cmp == PBL_CMP_CRDB) {
    k.push_back('\0');
    if (rng() % 2) {
      for (int b = 0; b < 8; b++) k.push_back(char(rng()));
      k.push_back(char(9));
    }
  }
  return k;
}

static std::vector<uint8_t> build(Keys& ks, uint32_t cmp, uint32_t bpk) {
  const uint64_t cap = pbl_bloom_build_bound(ks.n(), bpk);
  std::vector<uint8_t> out(cap);
  uint64_t len = ~0ull;
  CHECK(pbl_bloom_build_host(exact(ks.bytes), exact(ks.off), ks.n(), cmp, bpk, exact(out), cap, &len) == PBL_OK);
  CHECK(len <= cap && (ks.n() == 0) == (len == 0));
  if (len > 5) {  // a smaller output is refused, and says what it needs
    std::vector<uint8_t> small(len - 1);
    uint64_t need = 0;
    CHECK(pbl_bloom_build_host(exact(ks.bytes), exact(ks.off), ks.n(), cmp, bpk, exact(small), len - 1, &need) ==
          PBL_OVERFLOW);
    CHECK(need == len);
  }
  out.resize(len);
  return out;
}

static void probes(std::mt19937& rng, uint32_t cmp) {
  const uint32_t bpks[] = {1, 5, 10, 20};
  std::vector<std::vector<uint8_t>> filters;
  std::vector<Keys> members(4);
  for (int f = 0; f < 4; f++) {
    const uint32_t n = f == 0 ? 1 : 1 + rng() % 600;
    for (uint32_t i = 0; i < n; i++) members[f].add(make_key(rng, cmp, f * 1000 + i, true));
    filters.push_back(build(members[f], cmp, bpks[f]));
  }
  filters.push_back({});                                     // holds nothing
  filters.push_back({6, 1, 0, 0, 0});                        // five bytes: holds nothing
  std::vector<uint8_t> bad = filters[2];
  bad[bad.size() - 4] ^= 2;                                  // nLines does not match the length
  filters.push_back(bad);
  bad = filters[1];
  memset(&bad[bad.size() - 4], 0, 4);                        // nLines == 0
  filters.push_back(bad);
  const uint32_t nf = uint32_t(filters.size());
  std::vector<uint8_t> fbytes;
  std::vector<uint64_t> foff{0};
  for (auto& f : filters) {
    fbytes.insert(fbytes.end(), f.begin(), f.end());
    foff.push_back(fbytes.size());
  }
  pbl_filter_set set{exact(fbytes), exact(foff), nf};

  for (int f = 0; f < 4; f++) {
    Keys q = members[f];
    const uint64_t nm = q.n();
    for (uint32_t i = 0; i < 200; i++) q.add(make_key(rng, cmp, i, false));
    q.add("");
    const uint64_t n = q.n();
    std::vector<uint8_t> may(nf * n), named(n);
    std::vector<uint32_t> hash(n), hash2(n), which(n);
    std::vector<int32_t> st(nf);
    pbl_filter_queries pq{exact(q.bytes), exact(q.off), nullptr, uint32_t(n), cmp};
    pbl_filter_out po{exact(may), exact(hash), exact(st)};
    CHECK(pbl_filter_probe_host(&set, &pq, &po) == PBL_OK);
    for (uint64_t i = 0; i < nm; i++) CHECK(may[f * n + i] == PBL_FILTER_MAY);  // no false negative
    for (uint64_t i = 0; i < n; i++) {
      CHECK(may[4 * n + i] == 0 && may[5 * n + i] == 0);
      CHECK(may[6 * n + i] == (PBL_FILTER_MAY | PBL_FILTER_BAD) && may[7 * n + i] == (PBL_FILTER_MAY | PBL_FILTER_BAD));
    }
    for (uint32_t g = 0; g < nf; g++) CHECK(st[g] == (g >= 6 ? PBL_CORRUPT_FILTER : PBL_OK));
    for (uint64_t i = 0; i < n; i++) which[i] = uint32_t(rng() % (nf + 2));
    pq.filter = exact(which);
    pbl_filter_out pn{exact(named), exact(hash2), nullptr};
    CHECK(pbl_filter_probe_host(&set, &pq, &pn) == PBL_OK);
    for (uint64_t i = 0; i < n; i++) {
      CHECK(hash2[i] == hash[i]);
      CHECK(named[i] == (which[i] < nf ? may[which[i] * n + i] : uint8_t(PBL_FILTER_MAY | PBL_FILTER_BAD)));
    }
  }
}

// One row block's worth of sorted keys as a decoded batch of two blocks.
static void seeks(std::mt19937& rng) {
  std::vector<std::string> ks;
  for (uint32_t i = 0; i < 300; i++) ks.push_back("key" + std::to_string(100000 + i * 13));
  std::sort(ks.begin(), ks.end());
  Keys members;
  for (auto& k : ks) members.add(k);
  std::vector<uint8_t> flt = build(members, PBL_CMP_DEFAULT, 10);
  std::vector<uint32_t> koff, status{PBL_OK, PBL_OK};
  std::vector<uint8_t> kbytes, flags(ks.size(), 0);
  std::vector<uint64_t> kvb{0, 150, 300}, keyb{0, 0, 0};
  for (int b = 0; b < 2; b++) {
    keyb[b] = kbytes.size();
    for (int j = 0; j < 150; j++) {
      koff.push_back(uint32_t(kbytes.size() - keyb[b]));
      kbytes.insert(kbytes.end(), ks[b * 150 + j].begin(), ks[b * 150 + j].end());
    }
    koff.push_back(uint32_t(kbytes.size() - keyb[b]));
  }
  keyb[2] = kbytes.size();
  pbl_decode_out d{};
  d.kv_flags = exact(flags); d.key_off = exact(koff); d.key_bytes = exact(kbytes);
  d.blk_kv_base = exact(kvb); d.blk_key_base = exact(keyb); d.blk_status = exact(status);
  Keys q;
  for (uint32_t i = 0; i < 300; i += 3) q.add(ks[i]);
  for (uint32_t i = 0; i < 400; i++) q.add("key" + std::to_string(100000 + rng() % 5000));
  q.add("");
  q.add("zzz");
  const uint32_t n = uint32_t(q.n());
  std::vector<uint64_t> kv(n), kv0(n);
  std::vector<uint32_t> blk(n), blk0(n);
  std::vector<uint8_t> fl(n), fl0(n);
  pbl_seek_queries sq{exact(q.bytes), exact(q.off), nullptr, n, PBL_CMP_DEFAULT, PBL_SEEK_GE, 0};
  pbl_seek_out so{exact(kv), exact(blk), exact(fl)}, so0{exact(kv0), exact(blk0), exact(fl0)};
  CHECK(pbl_seek_batch_host(&d, 2, &sq, &so0) == PBL_OK);
  CHECK(pbl_seek_prefix_batch_host(&d, 2, &sq, exact(flt), flt.size(), &so) == PBL_OK);
  uint32_t n_out = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (fl[i] & PBL_SEEK_FILTERED) {
      n_out++;
      CHECK(kv[i] == PBL_SEEK_NONE && blk[i] == 0 && fl[i] == PBL_SEEK_FILTERED);
      CHECK(!(fl0[i] & PBL_SEEK_EXACT));
    } else {
      CHECK(kv[i] == kv0[i] && blk[i] == blk0[i] && fl[i] == fl0[i]);
    }
  }
  CHECK(n_out > 100);
  flt[flt.size() - 4] ^= 2;  // corrupt: excludes nothing, marks every answer
  CHECK(pbl_seek_prefix_batch_host(&d, 2, &sq, exact(flt), flt.size(), &so) == PBL_OK);
  for (uint32_t i = 0; i < n; i++) CHECK(kv[i] == kv0[i] && blk[i] == blk0[i] && fl[i] == (fl0[i] | PBL_SEEK_BAD_BLOCK));
  sq.op = PBL_SEEK_LT;
  CHECK(pbl_seek_prefix_batch_host(&d, 2, &sq, exact(flt), flt.size(), &so) == PBL_INVALID_ARG);
}

int main() {
  std::mt19937 rng(20251);
  for (int round = 0; round < 8; round++)
    for (uint32_t cmp = 0; cmp <= PBL_CMP_CRDB; cmp++) probes(rng, cmp);
  seeks(rng);
  printf("filter_host_check: ok\n");
  return 0;
}
