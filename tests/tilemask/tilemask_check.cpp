// kfx_tilemask.h against the per-lane formula of an integrate wave that
// computes its own prologue (k_integrate, the !kTab path).
//
// For every interval [wl, wh] inside [1, 600) (wl stepping by argv[1]), 1..8
// chunks and three kinds of monotone brick-rounded cuts (geometric, equal,
// random), with random certificate bits, settled bytes and dead chunks:
//   reference  each working chunk's wave: lane k <-> brick (za >> 3) + k,
//              inside / touched / isset / cert exactly as the kernel writes them;
//   under test the tile kernel's rounds of 64 bricks from wl >> 3 (lane k <->
//              brick rb + k, brick_touched / brick_inside over the working
//              chunks, one certificate per brick) through chunk_masks_round.
// skipm, setm, the free mask and the overhang mask of every working chunk must
// be equal, hence the three debug counts too.  argv[2] = "mut" leaves the
// chunk's own `inside` range out of the free mask (a brick certified free
// inside a neighbouring chunk then shows in this one's window): the check must fail.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>

#include "kfx_tilemask.h"

using u64 = unsigned long long;

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int brick_cut(int b, int wl, int wh) {  // int_chunk's rounding of an inner boundary
  int r = (b + 4) & ~7;
  r = r > wl ? r : wl;
  return r < wh + 1 ? r : wh + 1;
}

constexpr int kMaxBrick = 256;

int main(int argc, char **argv) {
  const int step = argc > 1 ? atoi(argv[1]) : 1;
  const bool mut = argc > 2 && !strcmp(argv[2], "mut");
  long long cases = 0, chunks = 0, bad = 0, deep = 0, overhang = 0, dropped = 0;
  for (int wl = 1; wl < 600; wl += step)
    for (int wh = wl; wh < 600; ++wh)
      for (int n = 1; n <= 8; ++n)
        for (int kind = 0; kind < 3; ++kind) {
          const int len = wh - wl + 1;
          int za[8], zb[8];
          int cut[9];
          cut[0] = wl, cut[n] = wh + 1;
          for (int c = 1; c < n; ++c) {
            int raw;
            if (kind == 0) {
              const float r = 0.65f, den = 1.f - powf(r, (float)n);
              raw = wl + (int)((float)len * ((1.f - powf(r, (float)c)) / den));
            } else if (kind == 1) {
              raw = wl + (int)((long long)len * c / n);
            } else {
              raw = wl + (int)(rnd() % (uint64_t)(len + 1));
            }
            cut[c] = brick_cut(raw, wl, wh);
            if (cut[c] < cut[c - 1]) cut[c] = cut[c - 1];  // monotone
          }
          bool work[8];
          for (int c = 0; c < n; ++c) {
            za[c] = cut[c], zb[c] = cut[c + 1] - 1;
            work[c] = za[c] <= zb[c] && (rnd() & 7) != 0;  // (a chunk none of whose lanes is live: its wave returns)
          }
          // per-brick inputs, at three densities
          bool hid[kMaxBrick], fg[kMaxBrick], set[kMaxBrick];
          const unsigned dens = (unsigned)(rnd() % 3);
          for (int b = 0; b < kMaxBrick; ++b) {
            const unsigned r = (unsigned)rnd();
            hid[b] = dens == 0 ? (r & 1) : dens == 1 ? (r & 7) == 0 : (r & 7) != 0;
            fg[b] = (r >> 8) & 1;
            set[b] = dens == 2 ? ((r >> 16) & 3) != 0 : (r >> 16) & 1;
          }
          // under test: the tile kernel's rounds
          kfx::ChunkMasks got[8];
          const int b1 = wh >> 3;
          for (int rb = wl >> 3; rb <= b1; rb += 64) {
            u64 H = 0, F = 0, S = 0;
            for (int lane = 0; lane < 64; ++lane) {
              const int b = rb + lane;
              bool touched = false, inside = false;
              for (int c = 0; c < n; ++c) {
                if (!work[c]) continue;
                touched = touched || kfx::brick_touched(b, za[c], zb[c]);
                inside = inside || kfx::brick_inside(b, za[c], zb[c]);
              }
              const bool isset = b <= b1 && set[b];
              const bool h = touched && hid[b], f = touched && isset && inside && fg[b];
              H |= (u64)h << lane, F |= (u64)f << lane, S |= (u64)isset << lane;
            }
            for (int c = 0; c < n; ++c) {
              if (!work[c]) continue;
              if (mut) {  // the free mask without the chunk's own `inside`
                const int gbs = za[c] >> 3;
                kfx::ChunkMasks t;
                kfx::chunk_masks_round(za[c], zb[c], rb, H, F, S, t);
                const unsigned long long fr = kfx::brick_window(F, rb, gbs) & kfx::brick_window(S, rb, gbs);
                got[c].setm |= t.setm, got[c].overm |= t.overm;
                got[c].freem |= fr, got[c].skipm |= t.skipm | fr;
              } else {
                kfx::chunk_masks_round(za[c], zb[c], rb, H, F, S, got[c]);
              }
            }
          }
          // reference: each working chunk's own wave
          for (int c = 0; c < n; ++c) {
            if (!work[c]) continue;
            u64 skipm = 0, setm = 0, freem = 0, overm = 0;
            for (int k = 0; k < 64; ++k) {
              const int gb = (za[c] >> 3) + k;
              const bool inside = gb * 8 >= za[c] && gb * 8 + 7 <= zb[c];
              const bool touched = gb * 8 >= (za[c] & ~3) && gb * 8 <= zb[c];
              const bool isset = gb * 8 <= zb[c] && set[gb];
              const bool certh = touched && hid[gb], certf = touched && isset && inside && fg[gb];
              setm |= (u64)isset << k;
              freem |= (u64)certf << k;
              skipm |= (u64)(certf || certh) << k;
              overm |= (u64)(certh && !inside) << k;
            }
            ++chunks;
            if ((zb[c] >> 3) - (za[c] >> 3) >= 64) ++deep;
            if (overm) ++overhang;
            if (got[c].skipm != skipm || got[c].setm != setm || got[c].freem != freem || got[c].overm != overm) {
              if (bad++ < 5)
                printf("wl %d wh %d n %d kind %d chunk %d [%d, %d]: skipm %016llx / %016llx setm %016llx / %016llx "
                       "freem %016llx / %016llx overm %016llx / %016llx\n",
                       wl, wh, n, kind, c, za[c], zb[c], got[c].skipm, skipm, got[c].setm, setm, got[c].freem, freem,
                       got[c].overm, overm);
            }
          }
          for (int c = 0; c < n; ++c) dropped += !work[c];
          ++cases;
        }
  printf("bad %lld cases %lld chunks %lld deep %lld overhang %lld dead %lld\n", bad, cases, chunks, deep, overhang, dropped);
  return bad ? 1 : 0;
}
