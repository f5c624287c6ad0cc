// store_check — the host-only brick store (csrc/kfx_brick_store.cpp) driven as
// a stand-alone program, so that it can run under ASan + UBSan without the
// library: put, replacement, the window take with its order, negative
// origins, dims that are no multiple of 8, the cap < n no-op and the argument
// errors, against a restatement on std::map.  Compiled together with the
// store's source; prints "store_check ok: ..." and returns 0, else the first
// failed check and 1.
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
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("store_check FAILED line %d: %s\n", __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
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

using Key = std::tuple<int, int, int>;  // (b2, b1, b0): the canonical order
int fdiv8(int a) { return a >= 0 ? a / 8 : -((-a + 7) / 8); }

}  // namespace

int main() {
  kfx_brick_store *s = nullptr;
  CHECK(kfx_brick_store_create(nullptr) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_create(&s) == KFX_OK && s);
  std::map<Key, kfx_brick> ref;
  int64_t n = -1;
  CHECK(kfx_brick_store_count(s, &n) == KFX_OK && n == 0);

  // argument errors change nothing
  const int o0[3] = {0, 0, 0}, d64[3] = {64, 64, 64};
  kfx_brick one = make(0, 0, 0, 1);
  CHECK(kfx_brick_store_put(nullptr, &one, 1) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_put(s, nullptr, 1) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_put(s, &one, -1) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_put(s, nullptr, 0) == KFX_OK);
  CHECK(kfx_brick_store_count(nullptr, &n) == KFX_ERR_ARG && kfx_brick_store_count(s, nullptr) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(nullptr, o0, d64, &one, 1, &n) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(s, nullptr, d64, &one, 1, &n) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(s, o0, nullptr, &one, 1, &n) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(s, o0, d64, &one, 1, nullptr) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(s, o0, d64, nullptr, 1, &n) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(s, o0, d64, &one, -1, &n) == KFX_ERR_ARG);
  const int o_bad[3] = {0, 4, 0}, d_bad[3] = {64, 0, 64};
  CHECK(kfx_brick_store_take_window(s, o_bad, d64, &one, 1, &n) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_take_window(s, o0, d_bad, &one, 1, &n) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_destroy(nullptr) == KFX_ERR_ARG);
  CHECK(kfx_brick_store_count(s, &n) == KFX_OK && n == 0);

  // puts in batches over coordinates -6..9 per axis, many of them repeated (replacement; the later
  // of two equal coordinates in one batch wins)
  int64_t puts = 0, taken = 0, windows = 0, refused = 0;
  for (int round = 0; round < 40; ++round) {
    std::vector<kfx_brick> batch;
    const int m = (int)(rnd() % 60);
    for (int i = 0; i < m; ++i) {
      const int x = (int)(rnd() % 16) - 6, y = (int)(rnd() % 16) - 6, z = (int)(rnd() % 16) - 6;
      batch.push_back(make(x, y, z, rnd()));
      ref[Key(z, y, x)] = batch.back();
    }
    CHECK(kfx_brick_store_put(s, batch.data(), (int64_t)batch.size()) == KFX_OK);
    puts += m;
    CHECK(kfx_brick_store_count(s, &n) == KFX_OK && n == (int64_t)ref.size());

    // a window at a (possibly negative) origin, dims no multiple of 8 on some rounds
    const int org[3] = {8 * ((int)(rnd() % 12) - 6), 8 * ((int)(rnd() % 12) - 6), 8 * ((int)(rnd() % 12) - 6)};
    const int dims[3] = {8 + (int)(rnd() % 40), 8 * (1 + (int)(rnd() % 5)), 1 + (int)(rnd() % 44)};
    std::vector<Key> want;
    for (const auto &kv : ref) {
      const int q[3] = {std::get<2>(kv.first), std::get<1>(kv.first), std::get<0>(kv.first)};
      bool in = true;
      for (int k = 0; k < 3; ++k) in = in && q[k] >= fdiv8(org[k]) && q[k] < fdiv8(org[k]) + (dims[k] + 7) / 8;
      if (in) want.push_back(kv.first);  // (map order = ascending (b2, b1, b0))
    }
    CHECK(kfx_brick_store_take_window(s, org, dims, nullptr, 0, &n) == KFX_OK && n == (int64_t)want.size());
    int64_t held = -1;
    CHECK(kfx_brick_store_count(s, &held) == KFX_OK && held == (int64_t)ref.size());  // a count takes nothing
    std::vector<kfx_brick> out(want.size() + 1);
    std::memset(out.data(), 0xab, out.size() * sizeof(kfx_brick));
    if (want.size() > 0) {  // cap < n: nothing removed, nothing written
      CHECK(kfx_brick_store_take_window(s, org, dims, out.data(), (int64_t)want.size() - 1, &n) == KFX_OK);
      CHECK(n == (int64_t)want.size());
      CHECK(kfx_brick_store_count(s, &held) == KFX_OK && held == (int64_t)ref.size());
      const unsigned char *raw = reinterpret_cast<const unsigned char *>(out.data());
      for (size_t i = 0; i < out.size() * sizeof(kfx_brick); ++i) CHECK(raw[i] == 0xab);
      ++refused;
    }
    CHECK(kfx_brick_store_take_window(s, org, dims, out.data(), (int64_t)want.size(), &n) == KFX_OK);
    CHECK(n == (int64_t)want.size());
    for (size_t i = 0; i < want.size(); ++i) {
      CHECK(std::memcmp(&out[i], &ref[want[i]], sizeof(kfx_brick)) == 0);
      ref.erase(want[i]);
    }
    const unsigned char *tail = reinterpret_cast<const unsigned char *>(&out[want.size()]);
    for (size_t i = 0; i < sizeof(kfx_brick); ++i) CHECK(tail[i] == 0xab);
    CHECK(kfx_brick_store_count(s, &held) == KFX_OK && held == (int64_t)ref.size());
    CHECK(kfx_brick_store_take_window(s, org, dims, nullptr, 0, &n) == KFX_OK && n == 0);  // taken means gone
    taken += (int64_t)want.size();
    windows += want.size() > 0;
  }
  CHECK(taken > 100 && windows > 10 && refused > 10 && !ref.empty());
  CHECK(kfx_brick_store_destroy(s) == KFX_OK);  // with bricks still held
  std::printf("store_check ok: %lld puts, %lld taken in %lld windows, %lld refused takes, %lld held at the end\n",
              (long long)puts, (long long)taken, (long long)windows, (long long)refused, (long long)ref.size());
  return 0;
}
