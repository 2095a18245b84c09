// swz_unpackstage.h -- what the unpack kernels of the converter share (swz_binunpack.hip, swz_pntsunpack.hip).  One workgroup
// takes TILE consecutive output rows, whatever segments they belong to; a WINDOW in LDS lists the segments from the one that
// holds the tile's first row on (s_first: their first rows, 0xFFFFFFFF past the table).  Array by array, what the tile holds
// of the array in one segment is one RUN of bytes of the raw image: the aligned dwords that cover it go into a STAGE in LDS,
// consecutive lanes consecutive dwords, so the run lies in the stage with the residue it has in memory.  Run e of an array of
// width w begins at dword (w * rel_e) / 4 + 2 e of the stage (rel_e: its first row in the tile): a run of L bytes is covered
// by at most (L + 6) / 4 <= L / 4 + 2 dwords, so the runs do not meet; a stage holds w * TILE / 4 + 2 * TILE + 4 dwords (one
// spare for the shifts).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace swz {

// the four bytes at byte q of the stage
__device__ __forceinline__ uint32_t stage_word(const uint32_t* stage, uint32_t q) {
  const uint32_t w0 = stage[q >> 2], w1 = stage[(q >> 2) + 1u];
  return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * (q & 3u)));
}

// the aligned dword at `at`: one load where it lies wholly inside [raw_begin, raw_end), else -- the first or the last dword of
// the buffer -- put together from the bytes that do
__device__ __forceinline__ uint32_t stage_load(uintptr_t at, uintptr_t raw_begin, uintptr_t raw_end) {
  if (at >= raw_begin && at + 4u <= raw_end) return *reinterpret_cast<const uint32_t*>(at);
  uint32_t v = 0;
  for (uint32_t b = 0; b < 4u; ++b)
    if (at + b >= raw_begin && at + b < raw_end) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(at + b) << (8u * b);
  return v;
}

// the segment of row r0: the last one of the table that begins at or before it (segment 0 begins at row 0)
template <typename Seg>
__device__ __forceinline__ uint32_t unpack_first_segment(const Seg* segs, uint32_t num_segs, uint32_t r0) {
  uint32_t k0 = 0;
  for (uint32_t hi = num_segs; hi - k0 > 1;) {
    const uint32_t mid = k0 + (hi - k0) / 2;
    if (segs[mid].first_row <= r0) k0 = mid; else hi = mid;
  }
  return k0;
}

// the window entries that hold rows of the tile: those that begin in front of r1 (every segment holds a point)
template <uint32_t TILE>
__device__ __forceinline__ uint32_t unpack_window_size(const uint32_t* s_first, uint32_t r1) {
  uint32_t l = 0, h = TILE;
  while (l < h) {
    const uint32_t mid = (l + h) / 2;
    if (s_first[mid] < r1) l = mid + 1; else h = mid;
  }
  return l;
}

// the entry of row r, a row of the tile
__device__ __forceinline__ uint32_t unpack_row_entry(const uint32_t* s_first, uint32_t nwin, uint32_t r) {
  uint32_t my = 0;
  for (uint32_t hi = nwin; hi - my > 1;) {
    const uint32_t mid = my + (hi - my) / 2;
    if (s_first[mid] <= r) my = mid; else hi = mid;
  }
  return my;
}

// The covering dwords of every run of one array into the stage.  run(e, &lo, &len, &G, &S): entry e's run holds len rows
// (0: its segment lacks the array) of w bytes, lies at [G, G + w len) of memory and from dword S of the stage on.  The caller
// synchronises.
template <uint32_t TILE, typename Run>
__device__ __forceinline__ void stage_fill(uint32_t* s_stage, const uint32_t* s_first, uint32_t nwin, uint32_t w, uint32_t r0,
                                           uint32_t r1, uintptr_t raw_begin, uintptr_t raw_end, Run&& run) {
  const uint32_t span = ((w * (r1 - r0)) >> 2) + 2u * nwin + 2u;
  for (uint32_t x = threadIdx.x; x < span; x += TILE) {
    // the last entry whose run begins at or before stage dword x (entry 0's begins at 0)
    uint32_t e = 0;
    for (uint32_t hi = nwin; hi - e > 1;) {
      const uint32_t mid = e + (hi - e) / 2;
      if (((w * (max(s_first[mid], r0) - r0)) >> 2) + 2u * mid <= x) e = mid; else hi = mid;
    }
    uint32_t lo, len, S;
    uintptr_t G;
    run(e, &lo, &len, &G, &S);
    if (len == 0u) continue;
    const uintptr_t word0 = G & ~(uintptr_t)3;
    const uint32_t slots = (uint32_t)((((G + (uintptr_t)w * len + 3u) & ~(uintptr_t)3) - word0) >> 2);
    const uint32_t s = x - S;
    if (s >= slots) continue;
    s_stage[x] = stage_load(word0 + 4u * (uintptr_t)s, raw_begin, raw_end);
  }
}

}  // namespace swz
