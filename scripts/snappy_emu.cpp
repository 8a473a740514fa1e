// Host emulation of the device snappy decoder (pebble_amd/csrc/snappy_dec.hip.h):
// 64 std::threads run the wave's code in lockstep at every wave primitive.
// Run by tests/test_snappy_emu.py and tests/test_snappy_forms.py; not part of the product.
//   /opt/rocm/lib/llvm/bin/clang++ -O1 -std=c++20 -pthread scripts/snappy_emu.cpp -o /tmp/snappy_emu
//   /tmp/snappy_emu in.bin out.bin   (in: a snappy block, uvarint length first)
//   /tmp/snappy_emu --routes pairs.txt   ("n D" lines: the route each takes)
// The block goes down the route the kernels give it -- snappy_walk_kernel's
// lane then sn4_decode, sn_decode, or snappy_wave on one lane -- and the first
// output line names it: "route walk|lds|global ok 0|1 D <decoded length>".
// Exit status: 0 decoded, 1 corrupt.
#include <algorithm>
#include <barrier>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define __device__
#define __forceinline__ inline
template <class T> using lptr = T*;
template <class T> using gptr = T*;
template <class T> T* to_lds_ptr(T* p) { return p; }
template <class T> T* to_glb(T* p) { return p; }
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct uint4 { uint32_t x, y, z, w; };
static uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
constexpr int kWave = 64;
static thread_local int g_lane;
static std::barrier<>* g_bar;
static uint64_t g_slot[64];
static int lane_id() { return g_lane; }
static void wave_sync() { g_bar->arrive_and_wait(); }
template <class T> static T exch(T v, int src) {
  g_bar->arrive_and_wait();
  uint64_t x = 0;
  std::memcpy(&x, &v, sizeof(T));
  g_slot[g_lane] = x;
  g_bar->arrive_and_wait();
  T r;
  uint64_t y = g_slot[src];
  std::memcpy(&r, &y, sizeof(T));
  g_bar->arrive_and_wait();
  return r;
}
template <class T> static T __shfl(T v, int src, int) { return exch(v, src); }
static uint64_t __ballot(int p) {
  g_bar->arrive_and_wait();
  g_slot[g_lane] = p != 0;
  g_bar->arrive_and_wait();
  uint64_t m = 0;
  for (int i = 0; i < 64; i++) m |= g_slot[i] << i;
  g_bar->arrive_and_wait();
  return m;
}
static int emu_readfirstlane(int v) { return exch(v, 0); }  // (int, as the builtin)
static uint32_t emu_alignbyte(uint32_t hi, uint32_t lo, uint32_t r) {
  return uint32_t(((uint64_t(hi) << 32) | lo) >> (8 * (r & 3)));
}
#define __builtin_amdgcn_readfirstlane(x) emu_readfirstlane(x)
#define __builtin_amdgcn_readlane(x, l) exch((x), (l))
#define SN_EMU_SCAN 1
#define __builtin_amdgcn_alignbyte(a, b, c) emu_alignbyte(a, b, c)
#define __builtin_amdgcn_fence(a, b) ((void)0)
#define __builtin_amdgcn_wave_barrier() g_bar->arrive_and_wait()
#define SN_LDS_OR(p, v) __atomic_fetch_or((p), (v), __ATOMIC_RELAXED)
#define SN_T(v)
#define SN_ACC(i, v)
using std::min;
namespace pbl {
namespace phys {
constexpr uint32_t kSnIn = 32768;
constexpr uint32_t kSnQ = 592;
#include "../pebble_amd/csrc/snappy_dec.hip.h"
}  // namespace phys
}  // namespace pbl

// physical.hip's uvarint32
static bool uvarint32(const uint8_t* p, uint64_t n, uint32_t* v, uint32_t* used) {
  uint64_t x = 0;
  for (uint32_t i = 0; i < n && i < 10; i++) {
    x |= uint64_t(p[i] & 0x7f) << (7 * i);
    if (p[i] < 0x80) {
      if (x > 0xffffffffull) return false;
      *v = uint32_t(x);
      *used = i + 1;
      return true;
    }
  }
  return false;
}

// The route snappy2_kernel / snappy4_kernel give a block of n compressed bytes
// decoding to D, by the compiled conditions.
static const char* route_of(uint32_t n, uint32_t D) {
  if (pbl::phys::sn4_walkable(n, D)) return "walk";
  return n <= pbl::phys::kSnIn && D <= 0xffffu ? "lds" : "global";
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (argc == 3 && !strcmp(argv[1], "--routes")) {  // a file of "n D" lines: a route per line
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned long long n, D;
    while (fscanf(f, "%llu %llu", &n, &D) == 2) puts(route_of(uint32_t(n), uint32_t(D)));
    fclose(f);
    return 0;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in(1 << 20);  // (zero past the block: the indicator byte's place)
  const size_t n = fread(in.data(), 1, in.size() - 64, f);
  fclose(f);
  uint32_t D = 0, used = 0;
  if (!uvarint32(in.data(), n, &D, &used)) {
    printf("route none ok 0 D 0\n");
    return 1;
  }
  if (D > (64u << 20)) return 3;
  const char* route = route_of(uint32_t(n), D);
  // EMU_NO_WALK: a walked block through snappy2's decoder instead
  if (!strcmp(route, "walk") && getenv("EMU_NO_WALK")) route = n <= pbl::phys::kSnIn ? "lds" : "global";
  const bool walked = !strcmp(route, "walk"), global = !strcmp(route, "global");
  static pbl::phys::Snap2Lds S;
  static pbl::phys::Snap4Lds S4;
  std::vector<uint8_t> out(size_t(D) + 64);
  bool res[64] = {false};
  if (global) {
    // snappy2_kernel's lane 0 alone: every wave primitive is a no-op
    std::barrier<> one(1);
    g_bar = &one;
    g_lane = 0;
    res[0] = pbl::phys::snappy_wave(pbl::phys::GlbBytes{in.data()}, uint32_t(n), pbl::phys::GlbBytesW{out.data()}, D, 0,
                                    1) != ~0u;
  } else {
    // snappy_walk_kernel's lane for this block, then snappy4's decode (or snappy2's)
    if (!walked) std::memcpy(S.in, in.data(), n);
    if (walked) pbl::phys::sn4_walk(in.data(), uint32_t(n), used, D, out.data());
    std::barrier<> bar(64);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (int l = 0; l < 64; l++)
      th.emplace_back([&, l] {
        g_lane = l;
        res[l] = walked ? pbl::phys::sn4_decode(S4, in.data(), uint32_t(n), D, out.data())
                        : pbl::phys::sn_decode(S, 0, uint32_t(n), used, D, out.data());
      });
    for (auto& t : th) t.join();
  }
  printf("route %s ok %d D %u\n", route, int(res[0]), D);
  if (argc > 2) {
    FILE* g = fopen(argv[2], "wb");
    fwrite(out.data(), 1, D, g);
    fclose(g);
  }
  return res[0] ? 0 : 1;
}
