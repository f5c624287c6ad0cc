// A chunk's brick masks from a round of certificates over a column tile's
// whole interval (integrate's tile kernel).
//
// An integrate wave that computes its own prologue gives lane k the brick
// gbs + k, gbs = za >> 3 the first brick of its chunk [za, zb], and derives
//   inside  = the chunk holds all of the brick
//   touched = the brick starts in [za & ~3, zb] (the loop's first batch .. the chunk's end)
//   isset   = the brick starts at or below zb and its settled byte is set
//   setm    = isset
//   freem   = touched, isset, inside and the free-space certificate holds
//   skipm   = freem, or touched and the hidden certificate holds
//   overm   = hidden and skipped, not inside (the debug overhang count)
// for its first 64 bricks only.  The tile kernel evaluates the certificates
// once per brick of the tile's interval, lane k <-> brick rb + k in rounds of
// 64 bricks, and turns each round's ballots into every chunk's masks with the
// functions below: the predicates above are ranges of bricks, so they become
// range masks in the chunk's own 64-brick window, and the round's ballots are
// shifted into that window (bricks outside it fall off: the first-64 rule).
// Host and device share this text (tests/tilemask/tilemask_check.cpp compares
// it with the per-lane formula).
#pragma once

#include "kfx_ffadd.h"  // KFX_HD

namespace kfx {

// bits of the bricks lo .. hi (inclusive) in the 64-brick window that starts at brick w0
KFX_HD inline unsigned long long brick_range(int lo, int hi, int w0) {
  lo = lo - w0 > 0 ? lo - w0 : 0;
  hi = hi - w0 < 63 ? hi - w0 : 63;
  if (hi < lo) return 0ull;
  const int n = hi - lo + 1;
  return (n >= 64 ? ~0ull : (1ull << n) - 1ull) << lo;
}

// a mask over the bricks from .. from+63 as a mask over the bricks to .. to+63
KFX_HD inline unsigned long long brick_window(unsigned long long m, int from, int to) {
  const int d = from - to;
  if (d >= 64 || d <= -64) return 0ull;
  return d >= 0 ? m << d : m >> -d;
}

// The bricks a wave of chunk [za, zb] evaluates (lane k < 64: brick (za >> 3) + k):
// does brick b start in the chunk's batches / lie wholly in the chunk?
KFX_HD inline bool brick_touched(int b, int za, int zb) {
  return b >= (za >> 3) && b - (za >> 3) < 64 && b * 8 >= (za & ~3) && b * 8 <= zb;
}
KFX_HD inline bool brick_inside(int b, int za, int zb) {
  return b >= (za >> 3) && b - (za >> 3) < 64 && b * 8 >= za && b * 8 + 7 <= zb;
}

struct ChunkMasks {
  unsigned long long skipm = 0ull, setm = 0ull, freem = 0ull, overm = 0ull;
};

// One round, bricks rb .. rb+63, into the masks of the chunk [za, zb] (za <= zb):
//   hid: the hidden certificate holds;
//   fre: the free-space certificate holds, evaluated where the byte is set and
//        some chunk of the tile holds all of the brick;
//   set: the settled byte is set.
KFX_HD inline void chunk_masks_round(int za, int zb, int rb, unsigned long long hid, unsigned long long fre,
                                     unsigned long long set, ChunkMasks &m) {
  const int gbs = za >> 3;
  const unsigned long long H = brick_window(hid, rb, gbs), F = brick_window(fre, rb, gbs), S = brick_window(set, rb, gbs);
  const unsigned long long inside = brick_range((za + 7) >> 3, ((zb + 1) >> 3) - 1, gbs);
  const unsigned long long touched = brick_range(((za & ~3) + 7) >> 3, zb >> 3, gbs);
  const unsigned long long seen = brick_range(gbs, zb >> 3, gbs);
  const unsigned long long fr = F & S & inside, hd = H & touched;
  m.setm |= S & seen;
  m.freem |= fr;
  m.skipm |= fr | hd;
  m.overm |= hd & ~inside;
}

}  // namespace kfx
