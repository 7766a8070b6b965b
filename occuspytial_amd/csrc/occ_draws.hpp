// occ_draws.hpp -- the draws of a call, described once: the occupied sites per region (k_z_ob_occ, k_pb_z_occ), the posterior
// predictive check (k_z_ob_ppc) and the spatial residual check (occ_spatial.hpp).  Each records `width` integers per chain
// and kept draw of an occ_run, [C][keep][width] elements on the device, while the chain's switch is on; the rows name answers
// those of the last completed call.  Whatever the host does for them -- names, refusals, element types, what a rows name
// returns, opening, copying out and closing the record -- is read off this table (occ_gibbs.hip: DRAWS loops and get /
// set_draws_state); the kernels, and who holds the record's address, are the kinds' own.  Plain C++17, no HIP:
// tests/test_draws_cpu.py drives it through occ_plan_capi.cpp.  To add a draws output: DESIGN.md 7.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "occ_plan.hpp"  // (OUTPUTS: the bit, the switch's name and "the probit model has it" of an output of the z update)

namespace occ {

enum : int { DRW_REGION = 0, DRW_PPC = 1, DRW_MORAN = 2, N_DRAWS = 3 };
enum : int { DRW_NONE = -1, DRW_SWITCH = 0, DRW_ROWS = 1, DRW_INPUT = 2 };  // the fields of a kind's state names

struct Draws {
    const char *name[3];    // state names by field; input: what the handle must be given before the first switch-on (or none)
    int elem;               // bytes per element ...
    bool is_signed;         // ... and whether it is signed
    int width;              // elements per row; 0: set by the input
    int scaled;             // the leading columns that are fixed point: the rows name returns them times 2^-32
    uint32_t bit;           // the chain's switch: this bit of ChainScalars::site_on, or (0) a word of the handle (Switches)
    bool probit;            // the probit handle has the output
    // refusals, word for word.  Until the kind is ready -- its input is set; without an input, a switch has been written
    // once -- its names answer not_ready.  Only a kind with an input refuses the switch itself that way: any first valid
    // write of ppc_stats makes the PPC names answer, and moran_stats = 0 before the first switch-on is accepted and does
    // nothing (set_draws_state, moran_switch).  input_locked: the input is set only while every chain is off.
    const char *not_ready, *no_probit, *bad_switch, *read_only, *input_locked;
};
constexpr Draws DRAWS[N_DRAWS] = {
    // uint32 counts of occupied sites, one per region: G = max(region_id) + 1 columns
    {{output_of(OUT_REGION).sw, "region_draws", "region_id"}, 4, false, 0, 0, OUT_REGION, output_of(OUT_REGION).probit,
     "no regions have been set for this handle (set region_id first)", nullptr, "region_stats is 0 or 1", "region_draws is read-only",
     "region_id cannot be set while a chain has region_stats on"},
    // uint64 sums (occ_kernels.hpp: PPC_NCOL): T_obs and T_rep in 2^-32 quanta, then two whole counts
    {{output_of(OUT_PPC).sw, "ppc_draws", nullptr}, 8, false, 4, 2, OUT_PPC, output_of(OUT_PPC).probit,
     "the posterior predictive check has not been switched on for this handle (set ppc_stats first)",
     "posterior predictive checks are not available for the probit model", "ppc_stats is 0 or 1", "ppc_draws is read-only", nullptr},
    // int64 sums (occ_spatial.hpp: SP_NCOL), all in 2^-32 quanta
    {{"moran_stats", "moran_draws", nullptr}, 8, true, 8, 8, 0u, false,
     "the spatial residual check has not been switched on for this handle (set moran_stats first)",
     "the spatial residual check is not available for the probit model", "moran_stats is 0 or 1", "moran_draws is read-only", nullptr}};

// The kind and (*field) the field of a state name; -1 for a name that is none of theirs.
inline int draws_lookup(const char *name, int *field)
{
    for (int k = 0; k < N_DRAWS; ++k)
        for (int f = 0; f < 3; ++f)
            if (DRAWS[k].name[f] && !std::strcmp(name, DRAWS[k].name[f])) {
                *field = f;
                return k;
            }
    *field = DRW_NONE;
    return -1;
}

// What the rows name returns for the raw element at column `col`: exact for a count and for a sum below 2^53 quanta,
// otherwise rounded to nearest.
inline double draws_value(const Draws &d, const void *raw, size_t col)
{
    uint64_t w = 0;
    std::memcpy(&w, raw, (size_t)d.elem);  // (little endian: a 4-byte count fills the low half)
    const double x = d.is_signed ? (double)(int64_t)w : (double)w;
    return col < (size_t)d.scaled ? x * 0x1.0p-32 : x;
}

// The elements a name holds -- what a write must bring, what a read returns: the switch one, the input one per site, the
// rows `keep` of `width` (both 0 for a chain that has none).
constexpr size_t draws_length(int field, size_t n, size_t keep, size_t width) { return field == DRW_SWITCH ? 1 : field == DRW_INPUT ? n : keep * width; }

}  // namespace occ
