// rowenc_host_check.cpp — pbl_rowenc_batch_host as a stand-alone host program for
// sanitizer runs (no GPU is touched): random streams under all three comparers,
// every flag combination, restart intervals from 1 up, targets from one byte to
// more than a stream, empty and bad streams, keys that share long prefixes,
// values of zero to a few hundred bytes, every buffer a heap allocation of
// exactly its size, so that a read or write past an end is seen.  Each batch
// is sized with zero capacities (which must report PBL_OVERFLOW and write no
// block), then encoded into exactly sized buffers.  Checks that the blocks
// tile their streams, that offsets are 16-byte aligned with zero padding, that
// every block's tail holds ceil(n / ri) restart words whose first is 0, and
// that walking the entries of every block by their varints ends exactly at the
// restart array with the block's KV count.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/rowenc.hip pebble_amd/csrc/rowblk_writer.cpp pebble_amd/csrc/data_iter.cpp \
//     scripts/rowenc_host_check.cpp \
//     -fsanitize=address,undefined -o rowenc_host_check && ./rowenc_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s (iter %d)\n", __FILE__, __LINE__, #c, iter); return 1; } } while (0)

struct Kv { std::string key; uint64_t trailer; std::string val; };

static uint32_t rd32(const uint8_t* p) { uint32_t x; std::memcpy(&x, p, 4); return x; }
static bool uvarint(const uint8_t* b, size_t n, size_t* at, uint32_t* v) {
  uint32_t x = 0;
  for (int s = 0; s < 35; s += 7) {
    if (*at >= n) return false;
    const uint8_t c = b[(*at)++];
    x |= uint32_t(c & 0x7f) << s;
    if (c < 0x80) { *v = x; return true; }
  }
  return false;
}

int main() {
  std::mt19937 rng(19);
  const uint32_t kinds[] = {0, 1, 1, 1, 2, 2, 7, 18, 23};
  uint64_t n_blocks = 0, n_kvs = 0;
  for (int iter = 0; iter < 500; iter++) {
    const uint32_t nb = rng() % 6, cmp = rng() % 3;
    pbl_rowenc_opts o{};
    o.restart_interval = 1 + rng() % (rng() % 2 ? 4 : 40);
    o.target_block_size = rng() % 4 == 0 ? 1 + rng() % 40 : 40 + rng() % 3000;
    o.block_size_threshold = rng() % 3 ? 90 : rng() % 130;
    o.comparer = cmp;
    const uint32_t fsel = rng() % 6;
    o.flags = fsel == 0 ? 0 : fsel == 1 ? PBL_ENC_LOWEST_LEVEL : PBL_ENC_VALUE_PREFIX | (fsel >= 3 ? PBL_ENC_OBSOLETE : 0) |
                                                             (fsel >= 5 ? PBL_ENC_LOWEST_LEVEL : 0);
    std::vector<uint64_t> trailer, kvb{0}, keyb{0}, valb{0};
    std::vector<uint8_t> flags, kbytes, vbytes;
    std::vector<uint32_t> koff, voff, status;
    for (uint32_t q = 0; q < nb; q++) {
      const uint32_t n = rng() % 4 == 0 ? 0 : rng() % 120;
      std::vector<Kv> kv;
      for (uint32_t j = 0; j < n; j++) {
        std::string k(rng() % 3 ? 2 + rng() % 4 : rng() % 30, 'a');
        for (auto& ch : k) ch = "ab@1\0\x09"[rng() % 6];
        kv.push_back({k, uint64_t(rng() % 64) << 8 | kinds[rng() % 9], std::string(rng() % 5 ? rng() % 12 : rng() % 300, 'v')});
      }
      std::sort(kv.begin(), kv.end(), [&](const Kv& a, const Kv& b) {
        const int c = pbl_key_compare(cmp, (const uint8_t*)a.key.data(), a.key.size(), (const uint8_t*)b.key.data(), b.key.size());
        return c ? c < 0 : a.trailer > b.trailer; });
      const size_t k0 = kbytes.size(), v0 = vbytes.size();
      for (const Kv& x : kv) {
        koff.push_back(uint32_t(kbytes.size() - k0)); voff.push_back(uint32_t(vbytes.size() - v0));
        kbytes.insert(kbytes.end(), x.key.begin(), x.key.end());
        vbytes.insert(vbytes.end(), x.val.begin(), x.val.end());
        trailer.push_back(x.trailer);
        flags.push_back(uint8_t(rng() % 9 == 0 ? PBL_KV_OBSOLETE : 0));
      }
      koff.push_back(uint32_t(kbytes.size() - k0)); voff.push_back(uint32_t(vbytes.size() - v0));
      status.push_back(rng() % 9 == 0 ? PBL_CORRUPT_BOUNDS : PBL_OK);
      kvb.push_back(trailer.size()); keyb.push_back(kbytes.size()); valb.push_back(vbytes.size());
    }
    for (auto* v : {&flags, &kbytes, &vbytes}) v->shrink_to_fit();
    trailer.shrink_to_fit(); koff.shrink_to_fit(); voff.shrink_to_fit(); status.shrink_to_fit();
    pbl_rowenc_in in{};
    in.batch.trailer = trailer.data(); in.batch.kv_flags = flags.data(); in.batch.key_off = koff.data();
    in.batch.val_off = voff.data(); in.batch.key_bytes = kbytes.data(); in.batch.val_bytes = vbytes.data();
    in.batch.blk_kv_base = kvb.data(); in.batch.blk_key_base = keyb.data(); in.batch.blk_val_base = valb.data();
    in.batch.blk_status = status.data();
    // (empty vectors hand over NULL, which the argument check refuses: give them one element)
    std::vector<uint64_t> one64(1); std::vector<uint8_t> one8(1); std::vector<uint32_t> one32(1);
    if (trailer.empty()) in.batch.trailer = one64.data();
    if (kbytes.empty()) in.batch.key_bytes = one8.data();
    if (vbytes.empty()) in.batch.val_bytes = one8.data();
    if (koff.empty()) { in.batch.key_off = one32.data(); in.batch.val_off = one32.data(); }
    if (status.empty()) in.batch.blk_status = one32.data();
    in.n_streams = nb;
    std::vector<uint64_t> sbb(nb + 1);
    std::vector<uint32_t> sst(std::max(nb, 1u));
    pbl_rowenc_totals t0{}, t{};
    pbl_rowenc_out out{};
    out.stream_block_base = sbb.data(); out.stream_status = sst.data(); out.totals = &t0;
    CHECK(pbl_rowenc_batch_host(&in, &o, &out) == PBL_OK);
    CHECK((t0.n_blocks == 0) == !(t0.status_mask & (1u << PBL_OVERFLOW)));
    std::vector<uint8_t> blocks(t0.block_bytes), obs(trailer.size());
    std::vector<uint64_t> off(t0.n_blocks), first(t0.n_blocks);
    std::vector<uint32_t> len(t0.n_blocks), bst(t0.n_blocks), nkv(t0.n_blocks);
    out.blocks = blocks.data(); out.block_off = off.data(); out.block_len = len.data(); out.block_stream = bst.data();
    out.block_first_kv = first.data(); out.block_n_kv = nkv.data(); out.obsolete = obs.empty() ? nullptr : obs.data();
    out.totals = &t; out.blocks_cap = blocks.size(); out.block_cap = off.size();
    CHECK(pbl_rowenc_batch_host(&in, &o, &out) == PBL_OK);
    CHECK(t.n_blocks == t0.n_blocks && t.block_bytes == t0.block_bytes && t.n_restarts == t0.n_restarts);
    CHECK(!(t.status_mask & (1u << PBL_OVERFLOW)));
    uint64_t b = 0, at = 0, restarts = 0;
    for (uint32_t q = 0; q < nb; q++) {
      CHECK(sbb[q] == b && sst[q] == status[q]);
      if (status[q] != PBL_OK) continue;
      uint64_t kv = kvb[q];
      while (kv < kvb[q + 1]) {
        CHECK(b < t.n_blocks && bst[b] == q && first[b] == kv && nkv[b] >= 1 && off[b] == at && off[b] % 16 == 0);
        const uint8_t* p = blocks.data() + off[b];
        const uint32_t nr = rd32(p + len[b] - 4);
        CHECK(nr == (nkv[b] - 1) / o.restart_interval + 1 && len[b] >= 4 * (nr + 1));
        const size_t ra = len[b] - 4 * (nr + 1);
        CHECK(rd32(p + ra) == 0);
        size_t e = 0;
        uint32_t entries = 0;
        while (e < ra) {
          uint32_t sh, un, vl;
          const size_t e0 = e;
          CHECK(uvarint(p, ra, &e, &sh) && uvarint(p, ra, &e, &un) && uvarint(p, ra, &e, &vl));
          if (entries % o.restart_interval == 0) CHECK(sh == 0 && (rd32(p + ra + 4 * (entries / o.restart_interval)) & 0x7fffffffu) == e0);
          e += size_t(un) + vl;
          entries++;
        }
        CHECK(e == ra && entries == nkv[b]);
        for (uint64_t z = len[b]; z < ((uint64_t(len[b]) + 15) & ~15ull); z++) CHECK(p[z] == 0);
        at += (uint64_t(len[b]) + 15) & ~15ull;
        restarts += nr;
        kv += nkv[b];
        b++;
      }
      CHECK(kv == kvb[q + 1]);
    }
    CHECK(sbb[nb] == b && b == t.n_blocks && at == t.block_bytes && restarts == t.n_restarts);
    n_blocks += b;
    n_kvs += trailer.size();
  }
  // refused arguments
  {
    int iter = -1;
    pbl_rowenc_opts o{16, 4096, 90, 0, 0, 0};
    CHECK(pbl_rowenc_batch_host(nullptr, &o, nullptr) == PBL_INVALID_ARG);
    o.flags = PBL_ENC_OBSOLETE;
    pbl_rowenc_in in{};
    pbl_rowenc_out out{};
    CHECK(pbl_rowenc_batch_host(&in, &o, &out) == PBL_INVALID_ARG);
  }
  std::printf("rowenc_host_check ok: %llu blocks from %llu KVs\n", (unsigned long long)n_blocks, (unsigned long long)n_kvs);
  return 0;
}
