// planes_check.cpp -- the plane layout of the jump table (modle_amd/csrc/jump_planes.h) against the
// canonical table and against the sequential generator.  A stand-alone host program, built with
// AddressSanitizer and UBSan by the Makefile next to it (tests/test_jump_table_planes.py runs it).
//
//   * jump_planes::word is a bijection on the 4 096 words of the table;
//   * the hop T^512 * state, read row by row through the plane addressing that wave::lds_load_row
//     uses on the GPU (two 16-byte reads at jump_planes::half_row16(v, 0 / 1)) from the permuted
//     table, and through the canonical addressing from the canonical table, equals 512 sequential
//     xoshiro_next steps -- for the 256 single-bit states, the all-ones state and 10 000 random ones.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_prng.hpp"
#include "jump_planes.h"

namespace {

constexpr uint64_t STRIDE = 512;

struct Row {
  uint64_t w[4];
};

// canonical: row v of a nibble's sub-table is 4 consecutive words
Row row_canonical(const uint64_t* nibble_table, uint32_t v) {
  Row r;
  std::memcpy(r.w, nibble_table + 4 * v, sizeof(r.w));
  return r;
}

// planes: the two 16-byte halves of row v, addressed in 16-byte units as on the GPU
Row row_planes(const uint64_t* nibble_table, uint32_t v) {
  const unsigned char* row16 = reinterpret_cast<const unsigned char*>(nibble_table);
  Row r;
  std::memcpy(r.w + 0, row16 + 16 * jump_planes::half_row16(v, 0), 16);
  std::memcpy(r.w + 2, row16 + 16 * jump_planes::half_row16(v, 1), 16);
  return r;
}

template <class LoadRow>
void hop(const uint64_t* table, const uint64_t s[4], uint64_t out[4], LoadRow load_row) {
  uint64_t acc[4] = {0, 0, 0, 0};
  for (uint32_t nib = 0; nib < jump_planes::NIBBLES; ++nib) {
    const uint32_t v = static_cast<uint32_t>(s[nib / 16] >> (4 * (nib % 16))) & 15u;
    const Row r = load_row(table + nib * jump_planes::NIBBLE_WORDS, v);
    for (int k = 0; k < 4; ++k) acc[k] ^= r.w[k];
  }
  std::memcpy(out, acc, sizeof(acc));
}

int failures = 0;

void check_state(const uint64_t* canonical, const uint64_t* planes, const uint64_t s[4], const char* what, int idx) {
  uint64_t seq[4] = {s[0], s[1], s[2], s[3]};
  for (uint64_t k = 0; k < STRIDE; ++k) modle_host::xoshiro_next(seq);
  uint64_t a[4], b[4];
  hop(canonical, s, a, row_canonical);
  hop(planes, s, b, row_planes);
  if (std::memcmp(a, seq, sizeof(seq)) != 0) {
    if (failures++ < 10) std::fprintf(stderr, "%s state %d: canonical hop differs from %llu steps\n", what, idx,
                                      static_cast<unsigned long long>(STRIDE));
  }
  if (std::memcmp(b, seq, sizeof(seq)) != 0) {
    if (failures++ < 10) std::fprintf(stderr, "%s state %d: plane hop differs from %llu steps\n", what, idx,
                                      static_cast<unsigned long long>(STRIDE));
  }
}

}  // namespace

int main() {
  const std::vector<uint64_t> canonical = modle_host::build_jump_table(STRIDE);
  if (canonical.size() != jump_planes::TABLE_WORDS) {
    std::fprintf(stderr, "table of %zu words, expected %u\n", canonical.size(), jump_planes::TABLE_WORDS);
    return 1;
  }

  // bijection on the word indices, and every nibble keeps its own 512 bytes
  std::vector<int> hit(jump_planes::TABLE_WORDS, 0);
  for (uint32_t c = 0; c < jump_planes::TABLE_WORDS; ++c) {
    const uint32_t p = jump_planes::word(c);
    if (p >= jump_planes::TABLE_WORDS) {
      std::fprintf(stderr, "word %u maps to %u: out of the table\n", c, p);
      return 1;
    }
    if (p / jump_planes::NIBBLE_WORDS != c / jump_planes::NIBBLE_WORDS) {
      std::fprintf(stderr, "word %u maps to %u: another nibble's sub-table\n", c, p);
      return 1;
    }
    ++hit[p];
  }
  for (uint32_t p = 0; p < jump_planes::TABLE_WORDS; ++p) {
    if (hit[p] != 1) {
      std::fprintf(stderr, "plane word %u is written %d times\n", p, hit[p]);
      return 1;
    }
  }
  // the sixteen half-rows of a plane are 16 bytes apart: 256 bytes, each of the 64 banks once
  for (uint32_t half = 0; half < 2; ++half) {
    for (uint32_t v = 0; v < jump_planes::ROWS; ++v) {
      if (jump_planes::half_row16(v, half) != half * 16 + v) {
        std::fprintf(stderr, "half-row (%u, %u) is not at 16-byte unit %u\n", v, half, half * 16 + v);
        return 1;
      }
    }
  }

  std::vector<uint64_t> planes(jump_planes::TABLE_WORDS, 0);
  jump_planes::permute(canonical.data(), planes.data());

  for (int bit = 0; bit < 256; ++bit) {
    uint64_t s[4] = {0, 0, 0, 0};
    s[bit / 64] = 1ULL << (bit % 64);
    check_state(canonical.data(), planes.data(), s, "single-bit", bit);
  }
  {
    const uint64_t s[4] = {~0ULL, ~0ULL, ~0ULL, ~0ULL};
    check_state(canonical.data(), planes.data(), s, "all-ones", 0);
  }
  uint64_t gen[4];
  modle_host::splitmix_seed(0x6a756d70706c6e73ULL, gen);
  for (int i = 0; i < 10000; ++i) {
    uint64_t s[4];
    for (int k = 0; k < 4; ++k) s[k] = modle_host::xoshiro_next(gen);
    check_state(canonical.data(), planes.data(), s, "random", i);
  }
  if (failures != 0) {
    std::fprintf(stderr, "%d mismatches\n", failures);
    return 1;
  }
  std::printf("planes: bijection on %u words; 10257 states: plane hop == canonical hop == %llu steps\n",
              jump_planes::TABLE_WORDS, static_cast<unsigned long long>(STRIDE));
  return 0;
}
