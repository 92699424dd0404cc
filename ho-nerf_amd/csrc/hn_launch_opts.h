// How options reach a field launch: one plain host struct, built where a C-ABI call starts and passed down
// by reference to every launcher.  No HIP header here: a host-only program can include this file (tests/san/launch_opts_san.cpp).
#pragma once
#include <stdlib.h>

namespace hn {

struct FieldLaunchOpts {
    const int* n_pts_dev = nullptr;   // device-side sample count of a compact list (hn_api.hip, CompactRec::n_dev)
    const int* orig_idx = nullptr;    // ordered -> dense index (compact list, live-first order)
    // The frame table of a FRAME-ALIGNED compact list (hn_api.hip, k_hand_compact_write: [first slot per frame, af + 1 | live samples per
    // frame, af]; n_pts_dev[2] = af), hand adjoint: k_pose_part_reduce takes a frame's rows from it.  NULL: a dense list, or the plain
    // compact layout of a one-frame launch.
    const int* frame_seg = nullptr;
    // object adjoint: g_rays_d is [n, 3], one row per SAMPLE, stored -- the caller sums the rows of a ray in a fixed order -- instead of
    // [n / spr, 3] accumulated with atomics
    bool dir_per_sample = false;
    // inside a render that keeps a TAPE (a backward pass follows) every launch of an HN_PREC_F16 field, the sdf-only ones of the
    // importance rounds included, takes the fp32-equivalent kernels: the differentiable render of such a field is the HN_PREC_F16X3
    // field's, bit for bit
    bool three_pass = false;
    // HONERF_UNIFORM_STASH (Hand2Args::ustash): 0 = every wave of the hand evaluation kernel moves its stash at full width; 2 = a wave
    // whose samples are all far keeps one column, in place; 1 = that column packed into whole cache lines (the same bits in all three)
    int uniform_stash = 1;
    // HONERF_FAR_TILES (Hand2Args::far_tiles): 0 = every tile of the hand evaluation kernel runs the general tile program; 1 = all-far
    // tiles run their own (the same bits)
    int far_tiles = 1;
    // HONERF_FAR_EPILOGUE (Hand2Args::far_epilogue) and HONERF_FAR_STREAM (Hand2Args::far_stream), both 1: a workgroup computes the far
    // result in its first all-far tile of a launch and its later all-far tiles reuse it (no weight chunk, no epilogue, the MFMAs on
    // held operands); either 0 = every all-far tile runs the all-far program that streams every chunk and computes (the same bits)
    int far_epilogue = 1;
    int far_stream = 1;
};

// unset or empty -> 1; first character '0' -> 0; '2' -> 2 where the switch has a third form; anything else -> 1
inline int env_switch(const char* e, bool has_two) {
    if (e == nullptr || e[0] == '\0') return 1;
    return e[0] == '0' ? 0 : ((has_two && e[0] == '2') ? 2 : 1);
}

// The five environment switches, read ONCE per C-ABI call, where that call builds its options (a setenv between two calls takes
// effect).  live_first (optional): HONERF_LIVE_FIRST, the single-field render's own switch: 0 = off; 1 = on for launches the field
// kernel treats as long; 2 = on at every size.
inline FieldLaunchOpts resolve_launch_opts(int* live_first = nullptr) {
    FieldLaunchOpts o;
    o.uniform_stash = env_switch(getenv("HONERF_UNIFORM_STASH"), true);
    o.far_tiles = env_switch(getenv("HONERF_FAR_TILES"), false);
    o.far_epilogue = env_switch(getenv("HONERF_FAR_EPILOGUE"), false);
    o.far_stream = env_switch(getenv("HONERF_FAR_STREAM"), false);
    if (live_first != nullptr) *live_first = env_switch(getenv("HONERF_LIVE_FIRST"), true);
    return o;
}

}  // namespace hn
