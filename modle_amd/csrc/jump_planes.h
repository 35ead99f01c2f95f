// jump_planes.h -- layout of the GF(2) jump table in the GPU's LDS (host and device).
//
// modle_host::build_jump_table keeps the canonical layout [64 nibbles][16 values][4 words]: row v of
// a nibble's sub-table is 32 bytes at byte 32 v.  A wave reads one row per lane with two 128-bit LDS
// reads, and the LDS serves such a read sixteen lanes at a time from 64 banks of 4 bytes: the
// half-rows of v and v + 8 lie 256 bytes apart, on the same banks, and sixteen lanes with independent
// nibble values nearly always hold such a pair (two LDS cycles per sixteen lanes instead of one).
//
// In the LDS the 512 bytes of a nibble are therefore kept as two planes: the sixteen low half-rows
// (words 0 and 1 of every row) 16 bytes apart, then the sixteen high half-rows (words 2 and 3).  The
// sixteen half-rows of a plane cover 256 bytes, every bank exactly once, so the lanes of a group
// either read different banks or the very same address.
//
// This header is the one definition of that layout: the host permutes the table with it before the
// upload (modle_hip.hip), wave::lds_load_row (wave_hip.h) addresses the rows with it, and
// tests/jump_planes checks both against the canonical table.  The CPU back-ends of the wave
// vocabulary (tests/wave_emu, tests/protocol_model) read the canonical table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MODLE_JP_FN __host__ __device__ constexpr
#else
#define MODLE_JP_FN constexpr
#endif

namespace jump_planes {

constexpr uint32_t NIBBLES = 64, ROWS = 16, ROW_WORDS = 4;      // canonical [64][16][4] u64
constexpr uint32_t NIBBLE_WORDS = ROWS * ROW_WORDS;              // 64 u64 = 512 bytes per nibble
constexpr uint32_t TABLE_WORDS = NIBBLES * NIBBLE_WORDS;         // 4096 u64

// Index, in 16-byte units from the start of a nibble's sub-table, of half `half` (0: words 0-1,
// 1: words 2-3) of row `v`.
MODLE_JP_FN uint32_t half_row16(uint32_t v, uint32_t half) { return half * ROWS + v; }

// Position in the plane layout of the u64 word that the canonical table holds at index `c`.
MODLE_JP_FN uint32_t word(uint32_t c) {
  const uint32_t nib = c / NIBBLE_WORDS, v = (c / ROW_WORDS) % ROWS, k = c % ROW_WORDS;
  return nib * NIBBLE_WORDS + 2 * half_row16(v, k / 2) + k % 2;
}

// dst (plane layout) from src (canonical layout), TABLE_WORDS words each
inline void permute(const uint64_t* src, uint64_t* dst) {
  for (uint32_t c = 0; c < TABLE_WORDS; ++c) dst[word(c)] = src[c];
}

}  // namespace jump_planes
