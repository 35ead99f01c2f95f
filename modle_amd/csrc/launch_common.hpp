// launch_common.hpp -- host-side glue shared by the HIP launcher (modle_hip.hip) and the CPU
// lane-emulator harness (tests/wave_emu): digests modle_hip_config into the device-side Params
// and converts between the ABI's 64-bit arrays and the device's 32-bit fields.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "modle_hip.h"
#include "sim_types.h"

namespace modle_host {

inline modle_dev::Params make_params(const modle_hip_config& c) {
  modle_dev::Params p;
  std::memset(&p, 0, sizeof(p));
  p.rev_speed = static_cast<double>(c.rev_extrusion_speed);
  p.fwd_speed = static_cast<double>(c.fwd_extrusion_speed);
  p.rev_speed_burnin = static_cast<double>(c.rev_extrusion_speed_burnin);
  p.fwd_speed_burnin = static_cast<double>(c.fwd_extrusion_speed_burnin);
  p.rev_std = c.rev_extrusion_speed_std;
  p.fwd_std = c.fwd_extrusion_speed_std;
  p.p_release = c.prob_of_lef_release;
  p.p_release_burnin = c.prob_of_lef_release_burnin;
  p.hard_stall_mult = c.hard_stall_lef_stability_multiplier;
  p.soft_stall_mult = c.soft_stall_lef_stability_multiplier;
  p.p_bypass = c.probability_of_extrusion_unit_bypass;
  p.pblock_major = c.lef_bar_major_collision_pblock;
  p.pblock_minor = c.lef_bar_minor_collision_pblock;
  p.tad_to_loop_ratio = c.tad_to_loop_contact_ratio;
  p.gev_mu = c.genextreme_mu;
  p.gev_sigma = c.genextreme_sigma;
  p.gev_xi = c.genextreme_xi;
  p.target_contact_density = c.target_contact_density;
  p.min_burnin_epochs = c.min_burnin_epochs;
  p.max_burnin_epochs = c.max_burnin_epochs;
  p.burnin_target_epochs_for_lef_activation = c.burnin_target_epochs_for_lef_activation;
  p.bin_size = static_cast<uint32_t>(c.bin_size);
  p.sampling_strategy = static_cast<uint32_t>(c.contact_sampling_strategy);
  p.skip_burnin = c.skip_burnin ? 1u : 0u;
  p.hist_len = static_cast<uint32_t>(c.burnin_history_length);
  p.window = static_cast<uint32_t>(c.burnin_smoothing_window_size);
  p.track_1d = c.track_1d_lef_position ? 1u : 0u;
  return p;
}

// checks that an interval / config can be represented by the device layout
inline const char* check_limits(const modle_hip_config& c, uint64_t start, uint64_t end,
                                uint64_t max_lefs, size_t n_barriers) {
  if (end <= start) return "empty interval";
  if (end >= 0xFFFFFFF0ull) return "interval end must be below 2^32 - 16 bp";
  if (c.bin_size == 0 || c.bin_size > 0xFFFFFFFFull) return "invalid bin_size";
  if (max_lefs == 0 || max_lefs >= (1u << 24)) return "number of LEFs must be in [1, 2^24)";
  if (n_barriers >= (1u << 24)) return "number of barriers must be below 2^24";
  if (c.burnin_history_length < c.burnin_smoothing_window_size + 2)
    return "burnin_history_length must exceed burnin_smoothing_window_size + 1";
  if (c.burnin_target_epochs_for_lef_activation == 0 && !c.skip_burnin)
    return "burnin_target_epochs_for_lef_activation must be positive";
  return nullptr;
}

// Size class a set-up NEEDS (sim_types.h; modle_hip_size_class adds the environment's override).
// NARROW (0): LEF ids and moves fit 16 bits.  Ids: fewer than 65 536 LEFs.  Moves: a draw is speed + std * z,
// z bounded at 40 here -- the stream cannot produce it (the ziggurat's tail would need a uniform below 2^-1000).
// Two things raise a move above its draw:
//  - the move adjustment (reference: simulation.cpp:350-407), by at most one per link of a chain of consecutive
//    units of the unit's direction, i.e. by less than the number of LEFs: speed + 40 std + LEFs + 2;
//  - the correction for a primary LEF-LEF collision whose other unit stays stalled by a barrier (reference:
//    simulation_correct_moves.cpp:83-96, 105-119): the unit is put next to the stalled one, whatever it drew
//    itself.  The pair was tested with the moves both units had then, distance < rev move + fwd move, so the new
//    move stays below the SUM of a rev and a fwd move: a rev unit drawn at 1 kb that meets a stalled fwd unit of
//    a 64.9 kb direction may move 65.8 kb.  The chains that raised the two adjusted moves are fwd units upstream
//    of the pair and rev units downstream of it, units of different LEFs (a LEF's rev unit is not downstream of
//    its fwd unit), so both raises together stay below the number of LEFs:
//    rev speed + fwd speed + 40 (rev std + fwd std) + LEFs.
// Clamping and every other collision pass only shorten moves.  The kernel ends a cell with ERR_MOVE_RANGE should
// a move ever exceed the limit, instead of truncating it.
inline int size_class_required(const modle_hip_config& c, uint64_t max_lefs) {
  if (max_lefs >= 65536) return 1;
  const double rev = static_cast<double>(std::max(c.rev_extrusion_speed, c.rev_extrusion_speed_burnin));
  const double fwd = static_cast<double>(std::max(c.fwd_extrusion_speed, c.fwd_extrusion_speed_burnin));
  const double rev_sd = std::fabs(c.rev_extrusion_speed_std), fwd_sd = std::fabs(c.fwd_extrusion_speed_std);
  const double lefs = static_cast<double>(max_lefs);
  const double own = std::max(rev, fwd) + 40.0 * std::max(rev_sd, fwd_sd) + lefs + 2.0;
  const double pair = rev + fwd + 40.0 * (rev_sd + fwd_sd) + lefs;
  return std::max(own, pair) <= 65533.0 ? 0 : 1;  // (MOVE_LIMIT of the NARROW class)
}

// ---- how a launch is laid out on the GPU: THE statement of the rule ----
// What the environment may force (tests, A/B measurements, diagnostics; modle_hip.hip reads it once per launch).
struct LaunchOverrides {
  int grid_cap = 0;              // MODLE_HIP_GRID >= 1: at most that many workgroups
  int waves = 0;                 // MODLE_HIP_WAVES: 8 or 12 (anything else: the rule decides)
  int paired = -1;               // MODLE_HIP_PAIRED: -1 unset or empty, 0 fixed roles off, 1 on
  bool no_tail_helpers = false;  // MODLE_HIP_TAIL_HELPERS=0
  int active_waves = 0;          // MODLE_HIP_ACTIVE_WAVES in [1, waves]: only that many waves pull tasks
  bool wide = false;             // MODLE_HIP_SIZE_CLASS=wide
};
// What a measurement or diagnostic build of the library forces (the default build: nothing).
struct LaunchBuild {
  bool eight_waves_only = false;  // the build has no 12-wave geometry on its host side
  bool no_helpers = false;        // neither fixed roles nor tail helpers
  bool no_prng_producer = false;  // the generator policy has no block producer
};
struct LaunchPlan {
  uint32_t grid = 1;          // persistent workgroups
  uint32_t waves = 8;         // per workgroup: which pair of kernels (sim_launch.h)
  uint32_t pair_mains = 0;    // != 0: fixed roles (sim_pair.h) with that many main waves per workgroup
  uint32_t tail_helpers = 0;  // waves that find the queue empty help a running cell of their workgroup
  uint32_t active_waves = 8;  // waves of a workgroup that pull tasks
  bool wide = false;          // size class (size_class_required)
  // modle_hip_launch_info's view of the same:
  uint32_t main_waves_per_workgroup = 8, helper_waves = 0, prng_producer_waves = 0;
};

// Pure: the same answer on the host of a launch, in the CPU tests (modle_hip_plan_launch) and on paper.
inline LaunchPlan plan_launch(uint64_t n_tasks, uint64_t num_cus, uint64_t max_lefs, const modle_hip_config& c,
                              const LaunchOverrides& o, const LaunchBuild& b = LaunchBuild{}) {
  LaunchPlan p;
  // Workgroups: one per CU even when there are fewer tasks than waves -- the waves that win a task are then spread
  // over all CUs instead of being packed 8 to a CU.  MODLE_HIP_GRID (diagnostic): fewer workgroups than CUs (what
  // do the waves of a CU share, what do the CUs share?)
  uint64_t grid = std::max<uint64_t>(1, std::min(num_cus, n_tasks));
  if (o.grid_cap >= 1) grid = std::min<uint64_t>(grid, static_cast<uint64_t>(o.grid_cap));
  p.grid = static_cast<uint32_t>(grid);
  // Waves per workgroup (round 5): 12 -- three per SIMD, 168 VGPRs, 256-output PRNG blocks, 256-key LDS buffers -- is
  // worth 1.2 % on a launch that fills the slots and whose epochs re-insert few units (the default parameters: 70 - 134
  // per epoch on chr1); a launch whose epochs re-insert more than the small buffers hold (BASELINE configs[4]: 600 - 800)
  // loses 17 % with them, and the fixed roles of a launch that leaves slots empty are laid out for 8.  Expected
  // re-insertions per epoch and direction ~ LEFs x release probability.  MODLE_HIP_WAVES=8 / 12 forces it; helper-wave
  // mode asked for by name (MODLE_HIP_PAIRED=1) means the kernels that have it.
  constexpr uint64_t kMaxMains = 4;  // (of the 8 waves of the kernels that know fixed roles)
  const bool leaves_slots_empty = n_tasks <= grid * kMaxMains;
  const double p_release = std::max(c.prob_of_lef_release, c.prob_of_lef_release_burnin);
  if (!leaves_slots_empty && n_tasks >= grid * 12 && static_cast<double>(max_lefs) * p_release < 170.0) p.waves = 12;
  if (o.waves == 8 || o.waves == 12) p.waves = static_cast<uint32_t>(o.waves);
  if (o.paired == 1 || b.eight_waves_only) p.waves = 8;
  // Fixed roles -- a helper wave per cell, and a PRNG producer per cell while there are waves to spare -- for launches
  // that leave at least half of the wave slots empty; MODLE_HIP_PAIRED=0 / 1 turns them off / on whatever the number
  // of tasks.  Every other launch: tail helpers.
  bool paired = p.waves == 8 && leaves_slots_empty;
  if (o.paired >= 0) paired = o.paired != 0;
  if (b.no_helpers) paired = false;
  if (paired && p.waves == 8) p.pair_mains = static_cast<uint32_t>(std::min(kMaxMains, (n_tasks + grid - 1) / grid));
  p.tail_helpers = (p.pair_mains == 0 && !o.no_tail_helpers && !b.no_helpers) ? 1u : 0u;
  // MODLE_HIP_ACTIVE_WAVES (diagnostic): how the kernel time scales with the waves in flight per CU
  p.active_waves = (o.active_waves >= 1 && static_cast<uint32_t>(o.active_waves) <= p.waves)
                       ? static_cast<uint32_t>(o.active_waves) : p.waves;
  p.wide = o.wide || size_class_required(c, max_lefs) != 0;
  p.main_waves_per_workgroup = p.pair_mains != 0 ? p.pair_mains : p.active_waves;
  p.helper_waves = p.pair_mains != 0 ? 1 : 0;
  p.prng_producer_waves = (p.pair_mains != 0 && p.pair_mains <= 2 && !b.no_prng_producer) ? 1 : 0;
  return p;
}

inline uint32_t pos_to_dev(uint64_t v) {
  return v == UINT64_MAX ? modle_dev::UNBOUND : static_cast<uint32_t>(v);
}
inline uint64_t pos_to_abi(uint32_t v) {
  return v == modle_dev::UNBOUND ? UINT64_MAX : static_cast<uint64_t>(v);
}
inline uint32_t coll_to_dev(uint64_t w) {
  return static_cast<uint32_t>(w & modle_dev::CW_INDEX_MASK) |
         (static_cast<uint32_t>(w >> 56) << modle_dev::CW_SHIFT);
}
inline uint64_t coll_to_abi(uint32_t w) {
  return static_cast<uint64_t>(w & modle_dev::CW_INDEX_MASK) |
         (static_cast<uint64_t>((w >> modle_dev::CW_SHIFT) & modle_dev::CW_EVENT_MASK) << 56);
}

inline uint32_t pow2_ceil(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// words of scratch one wave needs for `max_lefs` LEFs / `max_barriers` barriers
struct WorkspaceLayout {
  size_t u32_words;   // NUM_STATE_ARRAYS arrays of max_lefs
  size_t u64_words;   // sort keys
  size_t f64_words;   // burn-in history
  size_t u8_bytes;    // barrier states
  size_t hit_words;   // 4 lists of stalling barriers (u32)
  size_t total_bytes;
};

inline WorkspaceLayout workspace_layout(uint32_t max_lefs, uint32_t max_barriers,
                                        uint32_t hist_len) {
  WorkspaceLayout w;
  const size_t Lp = (static_cast<size_t>(max_lefs) + 63) & ~size_t(63);
  w.u32_words = modle_dev::NUM_STATE_ARRAYS * Lp;
  w.u64_words = pow2_ceil(max_lefs < 64 ? 64 : max_lefs);
  w.f64_words = 2 * static_cast<size_t>(hist_len);
  w.u8_bytes = (static_cast<size_t>(max_barriers) + 63) & ~size_t(63);
  w.hit_words = 4 * ((static_cast<size_t>(max_barriers) + 63) & ~size_t(63));
  w.total_bytes = w.u64_words * 8 + w.f64_words * 8 + w.u32_words * 4 + w.u8_bytes + w.hit_words * 4;
  w.total_bytes = (w.total_bytes + 255) & ~size_t(255);
  return w;
}

// carves a Workspace out of `base` (must be 8-byte aligned)
inline modle_dev::Workspace carve_workspace(void* base, uint32_t max_lefs, uint32_t max_barriers,
                                            uint32_t hist_len) {
  const WorkspaceLayout w = workspace_layout(max_lefs, max_barriers, hist_len);
  const size_t Lp = (static_cast<size_t>(max_lefs) + 63) & ~size_t(63);
  modle_dev::Workspace ws;
  char* p = static_cast<char*>(base);
  ws.sort_keys = reinterpret_cast<uint64_t*>(p);
  p += w.u64_words * 8;
  ws.hist = reinterpret_cast<double*>(p);
  p += w.f64_words * 8;
  uint32_t* q = reinterpret_cast<uint32_t*>(p);
  ws.r_pos = q + 0 * Lp;
  ws.r_id = reinterpret_cast<modle_dev::lefid_t*>(q + 1 * Lp);
  ws.r_move = reinterpret_cast<modle_dev::move_t*>(q + 2 * Lp);
  ws.r_coll = q + 3 * Lp;
  ws.f_pos = q + 4 * Lp;
  ws.f_id = reinterpret_cast<modle_dev::lefid_t*>(q + 5 * Lp);
  ws.f_move = reinterpret_cast<modle_dev::move_t*>(q + 6 * Lp);
  ws.f_coll = q + 7 * Lp;
  ws.epoch = q + 8 * Lp;
  ws.r_rank = q + 9 * Lp;
  ws.f_rank = q + 10 * Lp;
  ws.stall = q + 11 * Lp;
  for (uint32_t k = 0; k < modle_dev::NUM_TMP; ++k) ws.tmp[k] = q + (12 + static_cast<size_t>(k)) * Lp;
  for (uint32_t d = 0; d < 2; ++d) ws.by_id_pos[d] = q + (12 + modle_dev::NUM_TMP + static_cast<size_t>(d)) * Lp;
  p += w.u32_words * 4;
  ws.bar_active = reinterpret_cast<uint8_t*>(p);
  p += w.u8_bytes;
  uint32_t* hq = reinterpret_cast<uint32_t*>(p);
  const size_t Bp = w.hit_words / 4;
  ws.hit_pos[0] = hq;
  ws.hit_pos[1] = hq + Bp;
  ws.hit_idx[0] = hq + 2 * Bp;
  ws.hit_idx[1] = hq + 3 * Bp;
  ws.capacity_lefs = max_lefs;
  ws.capacity_barriers = max_barriers;
  return ws;
}

// Phase-level test entry point: the caller's arrays (reference layout, 64-bit) packed into nine
// consecutive u32 arrays of n entries (modle_dev::TestImage)
template <class Image>
inline void fill_test_image(uint32_t* base, size_t n, const uint64_t* rev_pos,
                            const uint64_t* fwd_pos, const uint64_t* epoch,
                            const uint64_t* rev_rank, const uint64_t* fwd_rank,
                            const uint64_t* rev_moves, const uint64_t* fwd_moves,
                            const uint64_t* rev_coll, const uint64_t* fwd_coll, Image& img) {
  img.rev_pos = base + 0 * n;
  img.fwd_pos = base + 1 * n;
  img.epoch = base + 2 * n;
  img.rev_rank = base + 3 * n;
  img.fwd_rank = base + 4 * n;
  img.rev_moves = base + 5 * n;
  img.fwd_moves = base + 6 * n;
  img.rev_coll = base + 7 * n;
  img.fwd_coll = base + 8 * n;
  for (size_t i = 0; i < n; ++i) {
    img.rev_pos[i] = pos_to_dev(rev_pos[i]);
    img.fwd_pos[i] = pos_to_dev(fwd_pos[i]);
    img.epoch[i] = pos_to_dev(epoch[i]);
    img.rev_rank[i] = static_cast<uint32_t>(rev_rank[i]);
    img.fwd_rank[i] = static_cast<uint32_t>(fwd_rank[i]);
    img.rev_moves[i] = static_cast<uint32_t>(rev_moves[i]);
    img.fwd_moves[i] = static_cast<uint32_t>(fwd_moves[i]);
    img.rev_coll[i] = coll_to_dev(rev_coll[i]);
    img.fwd_coll[i] = coll_to_dev(fwd_coll[i]);
  }
}

template <class Image>
inline void read_test_image(const Image& img, size_t n, uint64_t* rev_pos, uint64_t* fwd_pos,
                            uint64_t* epoch, uint64_t* rev_rank, uint64_t* fwd_rank,
                            uint64_t* rev_moves, uint64_t* fwd_moves, uint64_t* rev_coll,
                            uint64_t* fwd_coll) {
  for (size_t i = 0; i < n; ++i) {
    rev_pos[i] = pos_to_abi(img.rev_pos[i]);
    fwd_pos[i] = pos_to_abi(img.fwd_pos[i]);
    epoch[i] = pos_to_abi(img.epoch[i]);
    rev_rank[i] = img.rev_rank[i];
    fwd_rank[i] = img.fwd_rank[i];
    rev_moves[i] = img.rev_moves[i];
    fwd_moves[i] = img.fwd_moves[i];
    rev_coll[i] = coll_to_abi(img.rev_coll[i]);
    fwd_coll[i] = coll_to_abi(img.fwd_coll[i]);
  }
}

// bucket table for barrier lookups (see modle_dev::Interval::bar_bucket)
inline std::vector<uint32_t> build_barrier_buckets(uint64_t start, uint64_t end,
                                                   const std::vector<uint32_t>& bar_pos) {
  const uint32_t shift = modle_dev::BAR_BUCKET_SHIFT;
  const size_t n_buckets = static_cast<size_t>((end - start) >> shift) + 2;
  std::vector<uint32_t> table(n_buckets);
  size_t i = 0;
  for (size_t b = 0; b < n_buckets; ++b) {
    const uint64_t lo = start + (static_cast<uint64_t>(b) << shift);
    while (i < bar_pos.size() && bar_pos[i] < lo) ++i;
    table[b] = static_cast<uint32_t>(i);
  }
  return table;
}

}  // namespace modle_host
