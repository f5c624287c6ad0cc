// kfx_scanws.h: the count / scan / emit workspace of n units.
//
// For each n of argv (default 0 1 2 4095 4096 4097 2^28), without extra bytes
// and with the single-pass extraction's (the pool positions and wave list):
//   - counts | offsets | bsum | total | extra are disjoint, in this order, and
//     end inside the reported size; offsets, bsum and total are 8-byte aligned
//     (from a null base and from a 256-byte aligned one);
//   - bsum has room for scan_blocks(n) entries, total for kScanHeadWords;
//   - the size is not below what the five hand-written expressions the layout
//     replaced gave for that n;
//   - for n <= 2^16 the regions are filled through the returned pointers in a
//     heap block of exactly the reported size (a sanitizer build sees a byte
//     outside it), each with its own value, and read back unchanged.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kfx_scanws.h"

using kfx::ScanWs;

static long long bad = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond) && bad++ < 20) printf("n %zu extra %zu: failed %s\n", n, extra, #cond); \
  } while (0)

static size_t al8(size_t x) { return (x + 7) & ~(size_t)7; }
static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

static void check(size_t n, size_t extra, void *base) {
  const ScanWs w = kfx::scanws_layout(base, n, extra);
  const size_t nb = kfx::scan_blocks(n);
  const uintptr_t b = (uintptr_t)base, c = (uintptr_t)w.counts, o = (uintptr_t)w.offsets, s = (uintptr_t)w.bsum,
                  t = (uintptr_t)w.total, x = (uintptr_t)w.extra;
  CHECK(nb == (n + 4095) / 4096);
  CHECK(c == b);
  CHECK(c + n * 4 <= o);
  CHECK(o + n * 8 <= s);
  CHECK(s + nb * 8 <= t);
  CHECK(t + kfx::kScanHeadWords * 8 <= x);
  CHECK(x + extra == b + w.bytes);
  CHECK((o - b) % 8 == 0 && (s - b) % 8 == 0 && (t - b) % 8 == 0 && (x - b) % 8 == 0);
  CHECK(o % 8 == 0 && s % 8 == 0 && t % 8 == 0);
  CHECK(kfx::scanws_layout(nullptr, n, extra).bytes == w.bytes);  // the size does not depend on the base
  // the expressions the layout replaced
  const size_t two_pass = n * 4 + n * 8 + nb * 8 + 64;                // extract_items
  const size_t evict = al8(n * 4) + n * 8 + nb * 8 + 64;              // kfx_evict_points, kfx_evict_bricks, world_items
  const size_t pool = al256(n * 4) + al256(n * 8) + al256(nb * 8) + 256 + al256(n * 8) + al256(n * 4);  // extract_single_pass
  CHECK(w.bytes >= two_pass);
  CHECK(w.bytes >= evict);
  if (extra == al256(n * 8) + al256(n * 4)) CHECK(w.bytes >= pool);  // called with that path's extra bytes
}

int main(int argc, char **argv) {
  size_t ns[64] = {0, 1, 2, 4095, 4096, 4097, (size_t)1 << 28};
  int count = 7;
  if (argc > 1) {
    count = 0;
    for (int i = 1; i < argc && count < 64; ++i) ns[count++] = (size_t)strtoull(argv[i], nullptr, 10);
  }
  long long cases = 0, filled = 0;
  for (int i = 0; i < count; ++i) {
    const size_t n = ns[i];
    const size_t extras[2] = {0, kfx::scan_align(n * 8) + kfx::scan_align(n * 4)};
    for (size_t extra : extras) {
      check(n, extra, nullptr);
      check(n, extra, (void *)(uintptr_t)0x7f0000001000ull);  // never dereferenced
      cases += 2;
      if (n > ((size_t)1 << 16)) continue;
      const size_t bytes = kfx::scanws_layout(nullptr, n, extra).bytes;
      void *mem = aligned_alloc(256, bytes);  // (bytes is a multiple of 256 here: extra is)
      if (!mem) return 2;
      const ScanWs w = kfx::scanws_layout(mem, n, extra);
      const size_t nb = kfx::scan_blocks(n);
      check(n, extra, mem);
      memset(w.counts, 0x11, n * 4);
      for (size_t k = 0; k < n; ++k) w.offsets[k] = 0x2222222222222222ull;
      for (size_t k = 0; k < nb; ++k) w.bsum[k] = 0x3333333333333333ull;
      for (size_t k = 0; k < kfx::kScanHeadWords; ++k) w.total[k] = 0x4444444444444444ull;
      memset(w.extra, 0x55, extra);
      for (size_t k = 0; k < n; ++k) CHECK(w.counts[k] == 0x11111111u && w.offsets[k] == 0x2222222222222222ull);
      for (size_t k = 0; k < nb; ++k) CHECK(w.bsum[k] == 0x3333333333333333ull);
      for (size_t k = 0; k < kfx::kScanHeadWords; ++k) CHECK(w.total[k] == 0x4444444444444444ull);
      for (size_t k = 0; k < extra; ++k) CHECK((unsigned char)w.extra[k] == 0x55);
      free(mem);
      ++filled;
    }
  }
  printf("bad %lld cases %lld filled %lld\n", bad, cases, filled);
  return bad ? 1 : 0;
}
