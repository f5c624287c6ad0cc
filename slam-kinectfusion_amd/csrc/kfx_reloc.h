// kfx_reloc.h — the host-only side of relocalisation: the fern
// table generator, packed frame codes and their distance, the match order, the
// selection rule of kfx_relocalise, the keyframe store's host mirror and its
// blob, and the search's chunk rule.  Plain C++, no HIP:
// tests/reloc/reloc_check.cpp builds it alone.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/kfx.h"

namespace kfx {

constexpr int kFernMin = 16, kFernMax = 1024;  // ferns per table: a multiple of 16 in this range
constexpr int kFernMaxWords = kFernMax / 16;   // uint64 words of a packed code at the most
constexpr int kSearchBlockKeys = 256;          // keyframes one search block holds in registers (one per lane)
constexpr int kSearchMaxChunk = 16;            // queries one search block walks at the most
constexpr int kSearchFillBlocks = 512;         // the grid a search aims for: two blocks on each of 256 CUs
constexpr int kSearchMaxK = 16;
constexpr uint64_t kNoKey = ~(uint64_t)0;      // the key of an empty result slot (no real key: distance <= 1024)

inline bool fern_count_ok(int m) { return m >= kFernMin && m <= kFernMax && m % 16 == 0; }

struct SplitMix64 {
  uint64_t state;
  uint64_t next() {
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
};

// the fern grid of a width x height camera with L pyramid levels: level L - 1
struct FernGrid {
  int wL, hL, s;
};
inline FernGrid fern_grid(int width, int height, int L) { return {width >> (L - 1), height >> (L - 1), 1 << (L - 1)}; }

inline bool fern_params_ok(const kfx_fern_params &p) { return fern_count_ok(p.n_ferns) && p.depth_min_mm <= p.depth_max_mm; }

// the table of (seed, depth range) on grid g: per fern x, y, tb, tg, tr, td drawn in this order
inline void fern_table(const FernGrid &g, const kfx_fern_params &p, kfx_fern *out) {
  SplitMix64 rng{p.seed};
  const uint64_t span = (uint64_t)p.depth_max_mm - p.depth_min_mm + 1;
  for (int f = 0; f < p.n_ferns; ++f) {
    kfx_fern &o = out[f];
    o.x = (int32_t)(rng.next() % (uint64_t)g.wL);
    o.y = (int32_t)(rng.next() % (uint64_t)g.hL);
    o.tb = (uint8_t)(rng.next() % 256);
    o.tg = (uint8_t)(rng.next() % 256);
    o.tr = (uint8_t)(rng.next() % 256);
    o.pad = 0;
    o.td = (float)(p.depth_min_mm + rng.next() % span) / 1000.0f;
  }
}

inline bool fern_table_ok(const FernGrid &g, const kfx_fern *t, int m) {
  for (int f = 0; f < m; ++f)
    if (t[f].x < 0 || t[f].x >= g.wL || t[f].y < 0 || t[f].y >= g.hL || !std::isfinite(t[f].td)) return false;
  return true;
}

// packed codes: fern f's nibble in word f / 16, bits 4 * (f % 16) .. + 3
inline void code_set(uint64_t *code, int f, unsigned nibble) {
  const int sh = 4 * (f % 16);
  code[f / 16] = (code[f / 16] & ~((uint64_t)0xF << sh)) | ((uint64_t)(nibble & 0xF) << sh);
}
inline unsigned code_get(const uint64_t *code, int f) { return (unsigned)(code[f / 16] >> (4 * (f % 16))) & 0xF; }

// ferns whose nibbles differ: each nibble of the XOR folded to its low bit, then counted
inline int word_distance(uint64_t a, uint64_t b) {
  const uint64_t x = a ^ b;
  return __builtin_popcountll((x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x1111111111111111ull);
}
inline int code_distance(const uint64_t *a, const uint64_t *b, int words) {
  int d = 0;
  for (int w = 0; w < words; ++w) d += word_distance(a[w], b[w]);
  return d;
}

// the match order's key: ascending (distance, keyframe id)
inline uint64_t match_key(int distance, int id) { return ((uint64_t)(uint32_t)distance << 32) | (uint32_t)id; }
inline kfx_keyframe_match key_match(uint64_t key) {
  if (key == kNoKey) return {-1, -1};
  return {(int32_t)(uint32_t)key, (int32_t)(key >> 32)};
}

// Queries per block of a search of q >= 1 codes over n keyframes: the most, up to
// 16, that still leave a grid of 512 blocks (keyframe blocks x chunks), at least
// 1.  A block keeps its 256 keyframes' words in registers over its chunk, so a
// longer chunk saves their loads but leaves fewer blocks.
inline long long search_key_blocks(long long n) { return n < 1 ? 1 : (n + kSearchBlockKeys - 1) / kSearchBlockKeys; }
inline int search_chunk_rule(long long n, long long q) {
  const long long kb = search_key_blocks(n);
  const long long want = (kSearchFillBlocks + kb - 1) / kb;
  const long long c = q / want;
  return (int)(c < 1 ? 1 : (c > kSearchMaxChunk ? kSearchMaxChunk : c));
}

// ---- kfx_relocalise's selection -----------------------------------------------
// A candidate: a (match, start) pair whose loop converged, with its level-0 record.
struct RelocCand {
  int64_t n0, den, sum_r2;  // accepted pixels, n[0] + n[2] + n[3] + n[4], the fixed-point sum of r^2
  int32_t match, start;
};
inline RelocCand reloc_cand(const kfx_icp_quality &q, int match, int start) {
  return {q.n[0], q.n[0] + q.n[2] + q.n[3] + q.n[4], q.sum_r2, match, start};
}
// a beats b: the larger fitness n0 / den by integer cross-multiplication (a zero
// denominator loses), then the smaller sum_r2 / n0 by a 128-bit cross product,
// then the earlier match, then the earlier start
inline bool reloc_better(const RelocCand &a, const RelocCand &b) {
  if (a.den == 0 || b.den == 0) {
    if (a.den != 0) return true;
    if (b.den != 0) return false;
  } else {
    const __int128 l = (__int128)a.n0 * b.den, r = (__int128)b.n0 * a.den;
    if (l != r) return l > r;
    const __int128 ea = (__int128)a.sum_r2 * b.n0, eb = (__int128)b.sum_r2 * a.n0;
    if (ea != eb) return ea < eb;
  }
  if (a.match != b.match) return a.match < b.match;
  return a.start < b.start;
}
// index of the winner among n candidates, -1 when there is none
inline int reloc_select(const RelocCand *c, int n) {
  int best = -1;
  for (int i = 0; i < n; ++i)
    if (best < 0 || reloc_better(c[i], c[best])) best = i;
  return best;
}

// ---- the store's host mirror and its blob -------------------------------------
struct KeyframeHost {
  kfx_fern_params par{};
  FernGrid grid{};
  int words = 0;  // m / 16
  std::vector<kfx_fern> table;
  std::vector<kfx_pose> poses;
  std::vector<uint64_t> codes;  // keyframe-major: keyframe i's words at codes[i * words ..]
  int64_t count() const { return (int64_t)poses.size(); }
  int32_t put(const kfx_pose &pose, const uint64_t *code) {
    poses.push_back(pose);
    codes.insert(codes.end(), code, code + words);
    return (int32_t)poses.size() - 1;
  }
};

// the blob: this header, then the table (m ferns), the poses (n), the codes (n * m / 16 words)
constexpr uint32_t kBlobMagic = 0x4B58464Bu;  // "KFXK"
constexpr uint32_t kBlobVersion = 1;
struct BlobHeader {
  uint32_t magic, version;
  int32_t n_ferns, wL, hL, s;
  uint32_t depth_min_mm, depth_max_mm;
  uint64_t seed;
  int64_t n;
};
static_assert(sizeof(BlobHeader) == 48, "the blob's header is 48 bytes");
static_assert(sizeof(kfx_fern) == 16 && sizeof(kfx_pose) == 48, "the blob's records");

inline int64_t blob_bytes(int m, int64_t n) {
  return (int64_t)sizeof(BlobHeader) + (int64_t)m * 16 + n * 48 + n * (m / 16) * 8;
}
inline int64_t blob_bytes(const KeyframeHost &h) { return blob_bytes(h.par.n_ferns, h.count()); }

inline void blob_write(const KeyframeHost &h, void *blob) {
  char *p = static_cast<char *>(blob);
  const BlobHeader hd = {kBlobMagic,         kBlobVersion,       h.par.n_ferns, h.grid.wL, h.grid.hL, h.grid.s,
                         h.par.depth_min_mm, h.par.depth_max_mm, h.par.seed,    h.count()};
  std::memcpy(p, &hd, sizeof(hd));
  p += sizeof(hd);
  std::memcpy(p, h.table.data(), h.table.size() * sizeof(kfx_fern));
  p += h.table.size() * sizeof(kfx_fern);
  if (h.count()) {
    std::memcpy(p, h.poses.data(), h.poses.size() * sizeof(kfx_pose));
    p += h.poses.size() * sizeof(kfx_pose);
    std::memcpy(p, h.codes.data(), h.codes.size() * sizeof(uint64_t));
  }
}

// Parse a blob for a context whose fern grid is g.  Returns nullptr and fills
// *out, or the reason it is refused (nothing written then).
inline const char *blob_read(const void *blob, int64_t bytes, const FernGrid &g, KeyframeHost *out) {
  if (!blob || bytes < (int64_t)sizeof(BlobHeader)) return "blob shorter than its header";
  BlobHeader hd;
  std::memcpy(&hd, blob, sizeof(hd));
  if (hd.magic != kBlobMagic) return "not a keyframe blob (magic)";
  if (hd.version != kBlobVersion) return "unknown blob version";
  if (!fern_count_ok(hd.n_ferns) || hd.depth_min_mm > hd.depth_max_mm) return "bad fern parameters in the blob";
  if (hd.wL != g.wL || hd.hL != g.hL || hd.s != g.s) return "the blob's fern grid is not this context's";
  if (hd.n < 0 || hd.n > ((int64_t)1 << 31) - 1) return "bad keyframe count in the blob";
  if (blob_bytes(hd.n_ferns, hd.n) != bytes) return "the blob's size does not match its header";
  const char *p = static_cast<const char *>(blob) + sizeof(hd);
  std::vector<kfx_fern> table((size_t)hd.n_ferns);
  std::memcpy(table.data(), p, table.size() * sizeof(kfx_fern));
  p += table.size() * sizeof(kfx_fern);
  if (!fern_table_ok(g, table.data(), hd.n_ferns)) return "a fern of the blob lies outside the grid";
  KeyframeHost h;
  h.par = {hd.n_ferns, hd.depth_min_mm, hd.depth_max_mm, hd.seed};
  h.grid = g;
  h.words = hd.n_ferns / 16;
  h.table.swap(table);
  h.poses.resize((size_t)hd.n);
  h.codes.resize((size_t)hd.n * h.words);
  if (hd.n) {
    std::memcpy(h.poses.data(), p, h.poses.size() * sizeof(kfx_pose));
    p += h.poses.size() * sizeof(kfx_pose);
    std::memcpy(h.codes.data(), p, h.codes.size() * sizeof(uint64_t));
  }
  for (const kfx_pose &q : h.poses)
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(i < 9 ? q.R[i] : q.t[i - 9])) return "a non-finite pose entry in the blob";
  *out = std::move(h);
  return nullptr;
}

}  // namespace kfx
