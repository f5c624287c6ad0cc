// kfx_scanws.h — the workspace of a count / scan / emit export, laid out in one
// place (host only, no HIP: tests/scanws/scanws_check.cpp builds it alone).
//
//   counts  n u32     what the count pass found per unit
//   offsets n u64     launch_scan's exclusive scan of counts
//   bsum    scan_blocks(n) u64   launch_scan's block sums
//   total   kScanHeadWords u64   [0] the sum; [1], [2] a count pass's own words
//                                (the single-pass extraction's pool counter and
//                                overflow flag), downloaded with it in one copy
//   extra   extra_bytes          what else the count pass needs, behind the rest
//
// Every region starts on a multiple of kScanAlign bytes from the base (a
// hipMalloc result is at least that aligned), so each is aligned for its type
// whatever n is.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kfx {

constexpr size_t kScanAlign = 256;
constexpr size_t kScanHeadWords = 3;

// bsum entries launch_scan needs (one per 4096 counts; <= 65536 for n <= 2^28)
inline size_t scan_blocks(size_t n) { return (n + 4095) / 4096; }
inline size_t scan_align(size_t bytes) { return (bytes + kScanAlign - 1) & ~(kScanAlign - 1); }

struct ScanWs {
  size_t bytes = 0;  // the allocation: every region and extra_bytes
  unsigned *counts = nullptr;
  unsigned long long *offsets = nullptr, *bsum = nullptr, *total = nullptr;
  char *extra = nullptr;
};

// base = null gives the size (and the regions as offsets) before allocating
inline ScanWs scanws_layout(void *base, size_t n, size_t extra_bytes = 0) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(base);
  const size_t o_off = scan_align(n * 4), o_bsum = o_off + scan_align(n * 8),
               o_total = o_bsum + scan_align(scan_blocks(n) * 8), o_extra = o_total + scan_align(kScanHeadWords * 8);
  ScanWs w;
  w.bytes = o_extra + extra_bytes;
  w.counts = reinterpret_cast<unsigned *>(b);
  w.offsets = reinterpret_cast<unsigned long long *>(b + o_off);
  w.bsum = reinterpret_cast<unsigned long long *>(b + o_bsum);
  w.total = reinterpret_cast<unsigned long long *>(b + o_total);
  w.extra = reinterpret_cast<char *>(b + o_extra);
  return w;
}

}  // namespace kfx
