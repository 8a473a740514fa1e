// keyspan_host_check.cpp — pbl_keyspan_decode_host as a stand-alone host program
// for sanitizer runs (no GPU is touched): random valid keyspan blocks (spans with
// gaps, RANGEDEL and range keys, every offset and value width) and broken ones
// (cut anywhere, bytes flipped), every buffer a heap allocation of exactly its
// size, so that a read or write past an end is seen.  A valid block must decode
// to the spans it was written from; a broken one must end with some status or
// decode within its bounds; the size call must equal the decode's totals.  Also
// blocks with rows that no span reaches, whose last output slice ends past its
// column while the column's own last offset is in place.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     pebble_amd/csrc/keyspan.hip scripts/keyspan_host_check.cpp -fsanitize=address,undefined \
//     -o keyspan_host_check && ./keyspan_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/pebble_amd.h"

struct Key { uint64_t trailer; std::string suffix, value; };
struct Span { std::string start, end; std::vector<Key> keys; };

static void put_uints(std::vector<uint8_t>& b, const std::vector<uint64_t>& v, uint32_t w, bool delta) {
  if (v.empty()) return;
  uint64_t lo = v[0];
  for (uint64_t x : v) lo = x < lo ? x : lo;
  b.push_back(uint8_t(w | (delta ? 0x80 : 0)));
  if (delta) for (int i = 0; i < 8; i++) b.push_back(uint8_t(lo >> (8 * i)));
  if (!w) return;
  while (b.size() % w) b.push_back(0);
  for (uint64_t x : v) { const uint64_t d = x - (delta ? lo : 0); for (uint32_t i = 0; i < w; i++) b.push_back(uint8_t(d >> (8 * i))); }
}
static uint32_t width_of(uint64_t span) { return span == 0 ? 0 : span < 256 ? 1 : span < 65536 ? 2 : span < (1ull << 32) ? 4 : 8; }
static void put_uints_auto(std::vector<uint8_t>& b, const std::vector<uint64_t>& v, bool want_delta) {
  if (v.empty()) return;
  uint64_t lo = v[0], hi = v[0];
  for (uint64_t x : v) { lo = x < lo ? x : lo; hi = x > hi ? x : hi; }
  const bool delta = want_delta && width_of(hi - lo) != 8;
  put_uints(b, v, width_of(delta ? hi - lo : hi), delta);
}
// `at`, `bad`: offset number `at` is written as `bad` (the column's last offset stays, so DecodeColumn passes)
static void put_bytes(std::vector<uint8_t>& b, const std::vector<std::string>& s, size_t at = 0, uint64_t bad = 0) {
  if (s.empty()) return;
  std::vector<uint64_t> off{0};
  for (auto& x : s) off.push_back(off.back() + x.size());
  const uint64_t last = off.back();
  if (bad) off[at] = bad;
  put_uints(b, off, width_of(bad > last ? bad : last), false);
  for (auto& x : s) b.insert(b.end(), x.begin(), x.end());
}
// `tail`: rows past idx[B-1], which no span reaches; `bad_col` (3 or 4), `bad`: that column's offset of row
// idx[B-1], the end of the last slice that is output, written as `bad`
static std::vector<uint8_t> encode(const std::vector<Span>& spans, bool delta, int tail = 0, int bad_col = 0, uint64_t bad = 0) {
  std::vector<std::string> bounds, suf, val;
  std::vector<uint64_t> idx, trl;
  for (auto& s : spans) {
    if (bounds.empty() || bounds.back() != s.start) { idx.push_back(trl.size()); bounds.push_back(s.start); }
    idx.push_back(trl.size() + s.keys.size()); bounds.push_back(s.end);
    for (auto& k : s.keys) { trl.push_back(k.trailer); suf.push_back(k.suffix); val.push_back(k.value); }
  }
  const size_t reach = trl.size();
  for (int i = 0; i < tail; i++) { trl.push_back(uint64_t(i + 1) << 8 | 15); suf.push_back("t"); val.push_back("u"); }
  std::vector<uint8_t> b;
  auto le = [&](uint64_t v, int n) { for (int i = 0; i < n; i++) b.push_back(uint8_t(v >> (8 * i))); };
  le(bounds.size(), 4); b.push_back(1); le(5, 2); le(trl.size(), 4);
  const size_t hdr = b.size();
  b.resize(hdr + 25);
  const uint8_t types[5] = {3, 2, 2, 3, 3};
  for (int c = 0; c < 5; c++) {
    b[hdr + 5 * c] = types[c];
    const uint32_t at = uint32_t(b.size());
    memcpy(&b[hdr + 5 * c + 1], &at, 4);
    if (c == 0) put_bytes(b, bounds); else if (c == 1) put_uints_auto(b, idx, delta); else if (c == 2) put_uints_auto(b, trl, delta);
    else put_bytes(b, c == 3 ? suf : val, reach, c == bad_col ? bad : 0);
  }
  b.push_back(0);
  return b;
}

// A decode into buffers of exactly the sizes the size call reported; returns the
// status mask, -1 on a mismatch.
struct Result { std::vector<uint64_t> trailer; std::vector<std::string> key, val, suf, xval; std::vector<uint32_t> span, row, status; };
static int decode(const std::vector<std::vector<uint8_t>>& blocks, uint64_t ssn, Result* R) {
  const uint32_t nb = uint32_t(blocks.size());
  size_t total = 0;
  for (auto& b : blocks) total += b.size();
  uint8_t* buf = (uint8_t*)malloc(total ? total : 1);
  uint64_t* off = (uint64_t*)malloc(8 * (nb ? nb : 1));
  uint32_t* len = (uint32_t*)malloc(4 * (nb ? nb : 1));
  size_t pos = 0;
  for (uint32_t i = 0; i < nb; i++) { if (!blocks[i].empty()) memcpy(buf + pos, blocks[i].data(), blocks[i].size()); off[i] = pos; len[i] = uint32_t(blocks[i].size()); pos += blocks[i].size(); }
  pbl_block_batch in{}; in.blocks = buf; in.block_off = off; in.block_len = len; in.n_blocks = nb; in.synthetic_seq_num = ssn;
  auto u64s = [](size_t n) { return (uint64_t*)malloc(8 * (n ? n : 1)); };
  auto u32s = [](size_t n) { return (uint32_t*)malloc(4 * (n ? n : 1)); };
  auto u8s = [](size_t n) { return (uint8_t*)malloc(n ? n : 1); };
  pbl_totals t0{}, t1{};
  pbl_decode_out sz{}; sz.blk_kv_base = u64s(nb + 1); sz.blk_key_base = u64s(nb + 1); sz.blk_val_base = u64s(nb + 1); sz.blk_status = u32s(nb); sz.totals = &t0;
  pbl_keyspan_extra sx{}; sx.blk_suffix_base = u64s(nb + 1); sx.blk_value_base = u64s(nb + 1);
  int rc = -1;
  if (pbl_keyspan_decode_host(&in, &sz, &sx) == PBL_OK) {
    const uint64_t n = t0.n_kv, ns = sx.blk_suffix_base[nb], nx = sx.blk_value_base[nb];
    pbl_decode_out o{}; o.blk_kv_base = u64s(nb + 1); o.blk_key_base = u64s(nb + 1); o.blk_val_base = u64s(nb + 1); o.blk_rst_base = u64s(nb + 1);
    o.blk_status = u32s(nb); o.totals = &t1; o.trailer = u64s(n); o.kv_flags = u8s(n); o.entry_off = u32s(n); o.key_off = u32s(n + nb); o.val_off = u32s(n + nb);
    o.key_bytes = u8s(t0.key_bytes); o.val_bytes = u8s(t0.val_bytes); o.kv_cap = n; o.key_cap = t0.key_bytes; o.val_cap = t0.val_bytes;
    pbl_keyspan_extra x{}; x.blk_suffix_base = u64s(nb + 1); x.blk_value_base = u64s(nb + 1); x.span = u32s(n); x.suffix_off = u32s(n + nb); x.value_off = u32s(n + nb);
    x.suffix_bytes = u8s(ns); x.value_bytes = u8s(nx); x.suffix_cap = ns; x.value_cap = nx;
    if (pbl_keyspan_decode_host(&in, &o, &x) == PBL_OK && !(t1.status_mask & (1u << PBL_OVERFLOW)) && t1.n_kv == n && t1.key_bytes == t0.key_bytes &&
        t1.val_bytes == t0.val_bytes && t1.status_mask == t0.status_mask && x.blk_suffix_base[nb] == ns && x.blk_value_base[nb] == nx) {
      rc = int(t1.status_mask);
      *R = Result{};
      for (uint32_t b = 0; b < nb; b++) {
        R->status.push_back(o.blk_status[b]);
        if (o.blk_rst_base[b] != 0 || o.blk_status[b] != sz.blk_status[b]) rc = -1;
        for (uint64_t i = o.blk_kv_base[b]; i < o.blk_kv_base[b + 1]; i++) {
          const uint64_t q = i + b;
          if (o.key_off[q] > o.key_off[q + 1] || o.val_off[q] > o.val_off[q + 1] || o.kv_flags[i] != 0) rc = -1;
          R->trailer.push_back(o.trailer[i]); R->span.push_back(x.span[i]); R->row.push_back(o.entry_off[i]);
          R->key.emplace_back((const char*)o.key_bytes + o.blk_key_base[b] + o.key_off[q], o.key_off[q + 1] - o.key_off[q]);
          R->val.emplace_back((const char*)o.val_bytes + o.blk_val_base[b] + o.val_off[q], o.val_off[q + 1] - o.val_off[q]);
          R->suf.emplace_back((const char*)x.suffix_bytes + x.blk_suffix_base[b] + x.suffix_off[q], x.suffix_off[q + 1] - x.suffix_off[q]);
          R->xval.emplace_back((const char*)x.value_bytes + x.blk_value_base[b] + x.value_off[q], x.value_off[q + 1] - x.value_off[q]);
        }
      }
    }
    // one KV short: sizes, no bytes (nothing is written, so a NULL-sized array would do)
    if (n) {
      pbl_totals t2{}; o.totals = &t2; o.kv_cap = n - 1;
      if (pbl_keyspan_decode_host(&in, &o, &x) != PBL_OK || !(t2.status_mask & (1u << PBL_OVERFLOW)) || t2.n_kv != n) rc = -1;
    }
    for (void* p : {(void*)o.blk_kv_base, (void*)o.blk_key_base, (void*)o.blk_val_base, (void*)o.blk_rst_base, (void*)o.blk_status, (void*)o.trailer, (void*)o.kv_flags,
                    (void*)o.entry_off, (void*)o.key_off, (void*)o.val_off, (void*)o.key_bytes, (void*)o.val_bytes, (void*)x.blk_suffix_base, (void*)x.blk_value_base,
                    (void*)x.span, (void*)x.suffix_off, (void*)x.value_off, (void*)x.suffix_bytes, (void*)x.value_bytes}) free(p);
  }
  for (void* p : {(void*)sz.blk_kv_base, (void*)sz.blk_key_base, (void*)sz.blk_val_base, (void*)sz.blk_status, (void*)sx.blk_suffix_base, (void*)sx.blk_value_base,
                  (void*)buf, (void*)off, (void*)len}) free(p);
  return rc;
}

int main() {
  std::mt19937_64 rng(31);
  uint64_t kvs = 0, with_status = 0;
  for (int iter = 0; iter < 1500; iter++) {
    // ascending keys; the first sometimes of 0 bytes, some long
    const int nsp = 1 + int(rng() % (iter % 50 == 0 ? 400 : 12));
    std::vector<std::string> keys;
    for (int i = 0; i < 2 * nsp + 2; i++) {
      char pre[8];
      snprintf(pre, sizeof pre, "%05d", i);
      std::string key = i == 0 && rng() % 4 == 0 ? "" : pre;
      if (!key.empty() && rng() % 3 == 0) key += std::string(rng() % (rng() % 40 == 0 ? 400 : 9), char('a' + rng() % 26));
      keys.push_back(key);
    }
    const uint64_t seq_hi = iter % 3 == 0 ? (1ull << 56) - 1 : iter % 3 == 1 ? 200 : 1ull << 20;
    std::vector<Span> spans;
    size_t k = 0;
    for (int s = 0; s < nsp; s++) {
      Span sp{keys[k], keys[k + 1], {}};
      for (int j = 1 + int(rng() % 3); j > 0; j--) {
        const bool rk = iter % 2 && rng() % 2;
        sp.keys.push_back(Key{(1 + rng() % seq_hi) << 8 | (rk ? 21 : 15), rk ? "@" + std::to_string(rng() % 50) : "", rk ? std::string(rng() % 30, 'v') : ""});
      }
      spans.push_back(sp);
      k += rng() % 4 ? 1 : 2;
    }
    const std::vector<uint8_t> good = encode(spans, rng() % 2);
    std::vector<uint8_t> bad = good;
    if (rng() % 3 == 0) bad.resize(rng() % bad.size());
    else for (int f = 1 + int(rng() % 2); f > 0; f--) bad[rng() % bad.size()] ^= uint8_t(1u << (rng() % 8));
    bad.shrink_to_fit();
    const uint64_t ssn = rng() % 3 ? 0 : 99;
    Result R;
    const int rc = decode({good, bad, good}, ssn, &R);
    if (rc < 0) { printf("mismatch, iter %d\n", iter); return 1; }
    if (R.status[0] != PBL_OK || R.status[2] != PBL_OK) { printf("a valid block has status %u, iter %d\n", R.status[0], iter); return 2; }
    with_status += R.status[1] != PBL_OK;
    // the first block's KVs are the spans it was written from
    size_t i = 0;
    for (auto& sp : spans)
      for (auto& key : sp.keys) {
        const uint64_t tr = ssn ? ssn << 8 | (key.trailer & 0xff) : key.trailer;
        if (i >= R.key.size() || R.key[i] != sp.start || R.val[i] != sp.end || R.trailer[i] != tr || R.suf[i] != key.suffix || R.xval[i] != key.value || R.row[i] != i) {
          printf("KV %zu differs, iter %d\n", i, iter);
          return 3;
        }
        i++;
      }
    kvs += i;
  }
  // rows that no span reaches, and the end of the last slice that is output past its column (whose own last
  // offset, the only one DecodeColumn bounds, is in place): a status, and no read past the block
  Result R;
  for (int iter = 0; iter < 200; iter++) {
    std::vector<Span> spans{{"a", "b", {{uint64_t(7) << 8 | 21, "@1", "v"}}}, {"b", "c", {{uint64_t(6) << 8 | 21, "@22", "ww"}}}};
    const int tail = 1 + int(rng() % 3), colm = 3 + int(rng() % 2);
    const uint64_t bad = iter % 4 == 0 ? (1ull << 31) + rng() % 1000 : iter % 4 == 1 ? 70000 + rng() % 1000 : 9 + rng() % 240;
    if (decode({encode(spans, false, tail)}, 0, &R) != 0 || R.key.size() != 2 || R.suf[1] != "@22") return 7;
    if (decode({encode(spans, false, tail, colm, bad)}, 0, &R) != (1 << PBL_CORRUPT_BOUNDS) || !R.key.empty()) { printf("offset %llu past column %d: no status\n", (unsigned long long)bad, colm); return 8; }
  }
  // B = 0, B = 1, and nothing at all
  if (decode({encode({}, false)}, 0, &R) != 0 || !R.key.empty()) return 4;
  if (decode({}, 0, &R) != 0) return 5;
  if (decode({std::vector<uint8_t>{}}, 0, &R) != (1 << PBL_CORRUPT_COLBLK_HEADER)) return 6;
  printf("ok (%llu KVs checked, %llu broken blocks with a status)\n", (unsigned long long)kvs, (unsigned long long)with_status);
  return 0;
}
