// reloc_check — csrc/kfx_reloc.h as its own program: the table generator, pack
// and unpack, code distances, the selection rule on crafted records (a tie at
// each level, zero denominators), the blob round trip and truncated and
// corrupted blobs.  Prints "bad <n> checks <m>"; exit status 1 when bad > 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kfx_reloc.h"

using namespace kfx;

static int bad = 0, checks = 0;
#define CHECK(x)                                          \
  do {                                                    \
    ++checks;                                             \
    if (!(x)) {                                           \
      ++bad;                                              \
      std::printf("line %d: %s\n", __LINE__, #x);         \
    }                                                     \
  } while (0)

static RelocCand cand(int64_t n0, int64_t den, int64_t r2, int match, int start) { return {n0, den, r2, match, start}; }

int main() {
  // splitmix64: the first outputs of seed 0 (the published test vector) and the table's draw order
  SplitMix64 r0{0};
  CHECK(r0.next() == 0xE220A8397B1DCDAFull);
  CHECK(r0.next() == 0x6E789E6AA1B965F4ull);
  const FernGrid g = fern_grid(320, 240, 3);
  CHECK(g.wL == 80 && g.hL == 60 && g.s == 4);
  for (int m : {16, 48, 512, 1024}) {
    const kfx_fern_params p = {m, 400u, 4000u, 2013ull};
    CHECK(fern_params_ok(p));
    std::vector<kfx_fern> t((size_t)m);
    fern_table(g, p, t.data());
    CHECK(fern_table_ok(g, t.data(), m));
    SplitMix64 r{2013};
    bool same = true;
    for (int f = 0; f < m; ++f) {
      const uint64_t x = r.next() % 80, y = r.next() % 60, b = r.next() % 256, gg = r.next() % 256, rr = r.next() % 256;
      const float td = (float)(400 + r.next() % 3601) / 1000.0f;
      same = same && t[f].x == (int)x && t[f].y == (int)y && t[f].tb == b && t[f].tg == gg && t[f].tr == rr &&
             t[f].td == td && t[f].pad == 0 && td >= 0.4f && td <= 4.0f;
    }
    CHECK(same);
  }
  for (int m : {0, 8, 17, 1040, -16}) CHECK(!fern_count_ok(m));
  CHECK(!fern_params_ok({512, 4000u, 400u, 1ull}));
  {  // a one-value depth range
    const kfx_fern_params p = {16, 1234u, 1234u, 5ull};
    kfx_fern t[16];
    fern_table(g, p, t);
    for (const kfx_fern &f : t) CHECK(f.td == 1234.0f / 1000.0f);
  }

  // pack / unpack and distances
  uint64_t a[kFernMaxWords] = {}, b[kFernMaxWords] = {};
  for (int f = 0; f < kFernMax; ++f) code_set(a, f, (unsigned)(f * 7 + 3));
  bool ok = true;
  for (int f = 0; f < kFernMax; ++f) ok = ok && code_get(a, f) == (unsigned)((f * 7 + 3) & 15);
  CHECK(ok);
  std::memcpy(b, a, sizeof(a));
  CHECK(code_distance(a, b, kFernMaxWords) == 0);
  for (int bit = 0; bit < 4; ++bit) {
    std::memcpy(b, a, sizeof(a));
    code_set(b, 37, code_get(a, 37) ^ (1u << bit));
    CHECK(code_distance(a, b, kFernMaxWords) == 1);
  }
  std::memcpy(b, a, sizeof(a));
  code_set(b, 1023, code_get(a, 1023) ^ 15u);
  code_set(b, 0, code_get(a, 0) ^ 5u);
  CHECK(code_distance(a, b, kFernMaxWords) == 2);
  for (int w = 0; w < kFernMaxWords; ++w) b[w] = ~a[w];
  CHECK(code_distance(a, b, kFernMaxWords) == kFernMax && code_distance(a, b, 1) == 16);
  CHECK(key_match(match_key(5, 9)).id == 9 && key_match(match_key(5, 9)).distance == 5);
  CHECK(key_match(kNoKey).id == -1 && key_match(kNoKey).distance == -1);
  CHECK(match_key(0, 7) < match_key(1, 0) && match_key(3, 4) < match_key(3, 5));

  // the chunk rule
  CHECK(search_chunk_rule(0, 1) == 1 && search_chunk_rule(4100, 300) == 9 && search_chunk_rule(65536, 256) == 16);
  CHECK(search_chunk_rule(1024, 256) == 2 && search_chunk_rule(1 << 20, 1) == 1);

  // selection: fitness, then error, then match, then start; zero denominators lose
  CHECK(reloc_better(cand(3, 4, 100, 5, 5), cand(2, 3, 1, 0, 0)));       // 3/4 > 2/3
  CHECK(!reloc_better(cand(2, 3, 1, 0, 0), cand(3, 4, 100, 5, 5)));
  CHECK(reloc_better(cand(2, 4, 10, 3, 0), cand(1, 2, 6, 0, 0)));        // 1/2 each; 10/2 < 6/1
  CHECK(!reloc_better(cand(1, 2, 6, 0, 0), cand(2, 4, 10, 3, 0)));
  CHECK(reloc_better(cand(2, 4, 10, 1, 7), cand(1, 2, 5, 2, 0)));        // equal error: the earlier match
  CHECK(reloc_better(cand(2, 4, 10, 1, 3), cand(1, 2, 5, 1, 4)));        // then the earlier start
  CHECK(!reloc_better(cand(1, 2, 5, 1, 4), cand(2, 4, 10, 1, 3)));
  CHECK(reloc_better(cand(0, 7, 0, 9, 9), cand(0, 0, 0, 0, 0)));         // a zero denominator loses to fitness 0
  CHECK(!reloc_better(cand(0, 0, 0, 0, 0), cand(0, 7, 0, 9, 9)));
  CHECK(reloc_better(cand(0, 0, 0, 0, 1), cand(0, 0, 0, 1, 0)) && !reloc_better(cand(0, 0, 0, 1, 0), cand(0, 0, 0, 0, 1)));
  {  // cross products past 64 bits
    const int64_t big = (int64_t)1 << 62;
    CHECK(reloc_better(cand(big, big + 1, 0, 1, 0), cand(big - 1, big, 0, 0, 0)));
    CHECK(reloc_better(cand(big, big, big - 1, 1, 0), cand(big, big, big, 0, 0)));
  }
  {
    const RelocCand c[] = {cand(0, 0, 0, 0, 0), cand(5, 10, 50, 0, 1), cand(1, 2, 9, 1, 0), cand(1, 2, 9, 1, 1)};
    CHECK(reloc_select(c, 4) == 2 && reloc_select(c, 2) == 1 && reloc_select(c, 1) == 0 && reloc_select(c, 0) == -1);
  }
  {
    kfx_icp_quality q = {};
    q.n[0] = 7, q.n[1] = 100, q.n[2] = 1, q.n[3] = 2, q.n[4] = 3, q.n[5] = 1000, q.sum_r2 = 11;
    const RelocCand c = reloc_cand(q, 2, 3);
    CHECK(c.n0 == 7 && c.den == 13 && c.sum_r2 == 11 && c.match == 2 && c.start == 3);
  }

  // the blob
  for (int m : {16, 512}) {
    KeyframeHost h;
    h.par = {m, 400u, 4000u, 77ull};
    h.grid = g;
    h.words = m / 16;
    h.table.resize((size_t)m);
    fern_table(g, h.par, h.table.data());
    for (int n = 0; n <= 5; n += 5) {
      for (int i = 0; (int)h.count() < n; ++i) {
        kfx_pose p = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {(float)i, 0.5f, -2.f}};
        uint64_t code[kFernMaxWords];
        for (int w = 0; w < h.words; ++w) code[w] = 0x0123456789ABCDEFull * (uint64_t)(i + 1) + (uint64_t)w;
        CHECK(h.put(p, code) == i);
      }
      std::vector<char> blob((size_t)blob_bytes(h));
      CHECK((int64_t)blob.size() == 48 + 16 * m + n * (48 + m / 2));
      blob_write(h, blob.data());
      KeyframeHost back;
      CHECK(blob_read(blob.data(), (int64_t)blob.size(), g, &back) == nullptr);
      CHECK(back.count() == n && back.words == h.words && back.par.seed == 77ull && back.par.n_ferns == m);
      CHECK(std::memcmp(back.table.data(), h.table.data(), (size_t)m * 16) == 0);
      CHECK(back.codes == h.codes);
      CHECK(n == 0 || std::memcmp(back.poses.data(), h.poses.data(), (size_t)n * 48) == 0);
      // refused: truncated at every length, a longer one, another grid, and each header field damaged
      KeyframeHost none;
      bool refused = true;
      for (size_t cut = 0; cut < blob.size(); cut += (cut < 64 ? 1 : 97))
        refused = refused && blob_read(blob.data(), (int64_t)cut, g, &none) != nullptr;
      CHECK(refused && none.count() == 0 && none.table.empty());
      std::vector<char> longer(blob);
      longer.push_back(0);
      CHECK(blob_read(longer.data(), (int64_t)longer.size(), g, &none) != nullptr);
      CHECK(blob_read(blob.data(), (int64_t)blob.size(), fern_grid(640, 480, 3), &none) != nullptr);
      CHECK(blob_read(blob.data(), (int64_t)blob.size(), fern_grid(320, 240, 2), &none) != nullptr);
      CHECK(blob_read(nullptr, 0, g, &none) != nullptr);
      for (size_t off : {0u, 4u, 8u, 12u, 16u, 20u, 40u, 44u}) {
        std::vector<char> dmg(blob);
        dmg[off] ^= 0x5A;
        CHECK(blob_read(dmg.data(), (int64_t)dmg.size(), g, &none) != nullptr);
      }
      {  // a fern moved off the grid; a pose entry that is no number
        std::vector<char> dmg(blob);
        const int32_t x = 80;
        std::memcpy(&dmg[48], &x, 4);
        CHECK(blob_read(dmg.data(), (int64_t)dmg.size(), g, &none) != nullptr);
        if (n) {
          std::vector<char> nanp(blob);
          const uint32_t nan = 0x7FC00000u;
          std::memcpy(&nanp[48 + 16 * (size_t)m + 4], &nan, 4);
          CHECK(blob_read(nanp.data(), (int64_t)nanp.size(), g, &none) != nullptr);
        }
      }
    }
  }
  std::printf("bad %d checks %d\n", bad, checks);
  return bad ? 1 : 0;
}
