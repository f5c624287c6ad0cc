// world_store_check — the brick store's part of the world map
// driven as a stand-alone program, so that it can run under ASan + UBSan
// without the library: kfx_brick_store_copy (order, nothing removed, the short
// buffer, the argument errors) and the merge kfx_world_bricks does with the
// window's bricks (kfx::brick_store_merge), against a restatement on std::map.
// Compiled together with the store's source; prints "world_store_check ok: ..."
// and returns 0, else the first failed check and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/kfx.h"

namespace kfx {
void set_error_text(const std::string &) {}  // the library's kfx_last_error text: not linked here
int64_t brick_store_merge(const kfx_brick_store *s, const kfx_brick *win, int64_t nw, kfx_brick *out);
}  // namespace kfx

#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::printf("world_store_check FAILED line %d: %s\n", __LINE__, #cond); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

namespace {

uint64_t rng_state = 0x2545f4914f6cdd1dull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

kfx_brick make(int x, int y, int z, uint32_t tag) {
  kfx_brick b;
  std::memset(&b, 0, sizeof b);
  b.b[0] = x, b.b[1] = y, b.b[2] = z;
  for (int i = 0; i < 512; ++i) {
    b.tsdf[i] = (int16_t)(tag * 31u + (uint32_t)i);
    b.weight[i] = (uint8_t)(tag + (uint32_t)i);
    b.rgb[i][0] = (uint8_t)(tag >> 3), b.rgb[i][1] = (uint8_t)i, b.rgb[i][2] = (uint8_t)(tag ^ (uint32_t)i);
  }
  return b;
}

using Key = std::tuple<int, int, int>;  // (b[2], b[1], b[0])
Key key_of(const kfx_brick &b) { return Key(b.b[2], b.b[1], b.b[0]); }

bool same(const std::vector<kfx_brick> &got, const std::map<Key, kfx_brick> &want) {
  if (got.size() != want.size()) return false;
  size_t i = 0;
  for (const auto &e : want)
    if (std::memcmp(&got[i++], &e.second, sizeof(kfx_brick))) return false;
  return true;
}

}  // namespace

int main() {
  long long copies = 0, merges = 0, won = 0;
  for (int round = 0; round < 40; ++round) {
    kfx_brick_store *st = nullptr;
    CHECK(kfx_brick_store_create(&st) == KFX_OK);
    std::map<Key, kfx_brick> held;
    const int span = 2 + (int)(rnd() % 4);
    const int nput = (int)(rnd() % 60);  // (round-dependent: some stores stay empty)
    for (int i = 0; i < nput; ++i) {
      const kfx_brick b = make((int)(rnd() % span) - 1, (int)(rnd() % span) - 2, (int)(rnd() % span) - 1, rnd());
      CHECK(kfx_brick_store_put(st, &b, 1) == KFX_OK);
      held[key_of(b)] = b;
    }
    // copy: everything, ascending, nothing removed
    int64_t n = -1;
    CHECK(kfx_brick_store_copy(st, nullptr, 0, &n) == KFX_OK && n == (int64_t)held.size());
    std::vector<kfx_brick> out((size_t)n + 1, make(99, 99, 99, 7u));
    CHECK(kfx_brick_store_copy(st, out.data(), n, &n) == KFX_OK && n == (int64_t)held.size());
    CHECK(std::memcmp(&out[(size_t)n], &out.back(), sizeof(kfx_brick)) == 0 && out.back().b[0] == 99);
    out.resize((size_t)n);
    CHECK(same(out, held));
    if (n > 0) {  // a short buffer: the count, nothing written
      std::vector<kfx_brick> small((size_t)n - 1 + 1, make(98, 98, 98, 5u));
      int64_t m = -1;
      CHECK(kfx_brick_store_copy(st, small.data(), n - 1, &m) == KFX_OK && m == n);
      for (const kfx_brick &b : small) CHECK(b.b[0] == 98);
    }
    int64_t cnt = -1;
    CHECK(kfx_brick_store_count(st, &cnt) == KFX_OK && cnt == n);
    ++copies;
    // merge with a window: ascending bricks, some on held coordinates (the window's win)
    std::map<Key, kfx_brick> winmap;
    const int nwin = (int)(rnd() % 30);
    for (int i = 0; i < nwin; ++i) {
      const kfx_brick b = make((int)(rnd() % span) - 1, (int)(rnd() % span) - 2, (int)(rnd() % span) - 1, rnd());
      winmap[key_of(b)] = b;
    }
    std::vector<kfx_brick> win;
    std::map<Key, kfx_brick> want = held;
    for (const auto &e : winmap) {
      win.push_back(e.second);
      won += want.count(e.first);
      want[e.first] = e.second;
    }
    const int64_t total = kfx::brick_store_merge(st, win.data(), (int64_t)win.size(), nullptr);
    CHECK(total == (int64_t)want.size());
    std::vector<kfx_brick> merged((size_t)total);
    CHECK(kfx::brick_store_merge(st, win.data(), (int64_t)win.size(), merged.data()) == total);
    CHECK(same(merged, want));
    // no store: the window alone
    std::vector<kfx_brick> alone(win.size());
    CHECK(kfx::brick_store_merge(nullptr, win.data(), (int64_t)win.size(), alone.data()) == (int64_t)win.size());
    CHECK(same(alone, winmap));
    // the store is unchanged
    CHECK(kfx_brick_store_copy(st, out.data(), n, &cnt) == KFX_OK && cnt == n && same(out, held));
    ++merges;
    // argument errors
    CHECK(kfx_brick_store_copy(nullptr, nullptr, 0, &n) == KFX_ERR_ARG);
    CHECK(kfx_brick_store_copy(st, nullptr, 0, nullptr) == KFX_ERR_ARG);
    CHECK(kfx_brick_store_copy(st, nullptr, 1, &n) == KFX_ERR_ARG);
    CHECK(kfx_brick_store_copy(st, out.data(), -1, &n) == KFX_ERR_ARG);
    CHECK(kfx_brick_store_destroy(st) == KFX_OK);
  }
  CHECK(won > 10);
  std::printf("world_store_check ok: %lld copies, %lld merges, %lld coordinates the window won\n", copies, merges, won);
  return 0;
}
