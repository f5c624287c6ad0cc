// kfx_brick_store.cpp — the host-only brick store of the moving volume
// (DESIGN.md §21): where a caller keeps the bricks kfx_evict_bricks handed out
// until the window returns to them.  An ordered map from the world brick
// coordinate, compared as (b[2], b[1], b[0]), to the 3600-byte record, so a
// window's bricks come out in kfx_evict_bricks' own order.  Host code only: no
// context, no GPU, and it compiles without HIP.
#include <array>
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <new>
#include <string>

#include "../../include/kfx.h"

namespace kfx {
void set_error_text(const std::string &msg);  // kfx_api.hip: the text kfx_last_error returns
}

namespace {

int fail(int code, const std::string &msg) {
  kfx::set_error_text(msg);
  return code;
}

using Key = std::array<int32_t, 3>;  // {b[2], b[1], b[0]}: the lexicographic order is the canonical one

Key key_of(const kfx_brick &b) { return {b.b[2], b.b[1], b.b[0]}; }

}  // namespace

struct kfx_brick_store {
  std::map<Key, std::unique_ptr<kfx_brick>> bricks;
};

namespace kfx {

// the store's bricks (s may be null: none) merged with the nw ascending bricks
// `win` (kfx_world_bricks: the window's), ascending, `win` winning an equal
// coordinate; returns how many there are and writes them when out is not null
int64_t brick_store_merge(const kfx_brick_store *s, const kfx_brick *win, int64_t nw, kfx_brick *out) {
  static const std::map<Key, std::unique_ptr<kfx_brick>> none;
  const auto &held = s ? s->bricks : none;
  auto it = held.begin();
  int64_t i = 0, at = 0;
  while (it != held.end() || i < nw) {
    const kfx_brick *src;
    if (it == held.end() || (i < nw && !(it->first < key_of(win[i])))) {
      if (it != held.end() && it->first == key_of(win[i])) ++it;  // the window's brick wins
      src = &win[i++];
    } else {
      src = (it++)->second.get();
    }
    if (out) std::memcpy(&out[at], src, sizeof(kfx_brick));
    ++at;
  }
  return at;
}

}  // namespace kfx

extern "C" {

int kfx_brick_store_create(kfx_brick_store **out) {
  if (!out) return fail(KFX_ERR_ARG, "null out");
  *out = new (std::nothrow) kfx_brick_store();
  return *out ? KFX_OK : fail(KFX_ERR_OOM, "brick store: out of memory");
}

int kfx_brick_store_destroy(kfx_brick_store *s) {
  if (!s) return fail(KFX_ERR_ARG, "null store");
  delete s;
  return KFX_OK;
}

int kfx_brick_store_put(kfx_brick_store *s, const kfx_brick *in, int64_t n) {
  if (!s) return fail(KFX_ERR_ARG, "null store");
  if (n < 0 || (n > 0 && !in)) return fail(KFX_ERR_ARG, "bad brick list");
  try {
    for (int64_t i = 0; i < n; ++i) {
      std::unique_ptr<kfx_brick> &slot = s->bricks[key_of(in[i])];
      if (!slot) slot.reset(new kfx_brick);
      std::memcpy(slot.get(), &in[i], sizeof(kfx_brick));
    }
  } catch (const std::bad_alloc &) {
    for (auto it = s->bricks.begin(); it != s->bricks.end();)  // (a slot whose record could not be allocated)
      it = it->second ? std::next(it) : s->bricks.erase(it);
    return fail(KFX_ERR_OOM, "brick store: out of memory");
  }
  return KFX_OK;
}

int kfx_brick_store_count(const kfx_brick_store *s, int64_t *n) {
  if (!s || !n) return fail(KFX_ERR_ARG, "null argument");
  *n = (int64_t)s->bricks.size();
  return KFX_OK;
}

int kfx_brick_store_copy(const kfx_brick_store *s, kfx_brick *out, int64_t cap, int64_t *n) {
  if (!s || !n) return fail(KFX_ERR_ARG, "null argument");
  if (cap < 0 || (cap > 0 && !out)) return fail(KFX_ERR_ARG, "bad brick buffer");
  *n = (int64_t)s->bricks.size();
  if (cap < *n) return KFX_OK;  // nothing written: size the buffer and call again
  int64_t at = 0;
  for (const auto &e : s->bricks) std::memcpy(&out[at++], e.second.get(), sizeof(kfx_brick));
  return KFX_OK;
}

int kfx_brick_store_take_window(kfx_brick_store *s, const int origin[3], const int dims[3], kfx_brick *out,
                                int64_t cap, int64_t *n) {
  if (!s || !origin || !dims || !n) return fail(KFX_ERR_ARG, "null argument");
  if (cap < 0 || (cap > 0 && !out)) return fail(KFX_ERR_ARG, "bad brick buffer");
  int64_t lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    if (origin[k] % 8) return fail(KFX_ERR_ARG, "origin components must be multiples of 8 voxels");
    if (dims[k] < 1) return fail(KFX_ERR_ARG, "dims must be positive");
    lo[k] = origin[k] / 8;
    hi[k] = lo[k] + ((int64_t)dims[k] + 7) / 8;
  }
  auto inside = [&](const Key &q) { return q[1] >= lo[1] && q[1] < hi[1] && q[2] >= lo[0] && q[2] < hi[0]; };
  // the keys are ordered by b[2] first: the window's z range is one run of the map
  const int32_t z0 = (int32_t)lo[2];  // (|origin / 8| < 2^28)
  const auto first = s->bricks.lower_bound(Key{z0, INT32_MIN, INT32_MIN});
  int64_t total = 0;
  for (auto it = first; it != s->bricks.end() && it->first[0] < hi[2]; ++it) total += inside(it->first);
  *n = total;
  if (cap < total) return KFX_OK;  // nothing removed or written: size the buffer and call again
  int64_t at = 0;
  for (auto it = first; it != s->bricks.end() && it->first[0] < hi[2];) {
    if (inside(it->first)) {
      std::memcpy(&out[at++], it->second.get(), sizeof(kfx_brick));
      it = s->bricks.erase(it);
    } else {
      ++it;
    }
  }
  return KFX_OK;
}

}  // extern "C"
