// Sanitizer harness (CPU): the options of a field launch (ho-nerf_amd/csrc/hn_launch_opts.h, host only, no HIP header), compiled
// with -fsanitize=address,undefined: the parse table of the three environment switches for unset, "", "0", "1", "2", "7", "off",
// and the default-constructed options.  TEST INFRASTRUCTURE (tests/san/Makefile, tests/test_abi.py).
#include <stdio.h>
#include <stdlib.h>

#include "hn_launch_opts.h"

struct Case {
    const char* value;   // NULL: unset
    int three_way;       // HONERF_LIVE_FIRST, HONERF_UNIFORM_STASH
    int two_way;         // HONERF_FAR_TILES
};

int main() {
    const Case cases[] = {{nullptr, 1, 1}, {"", 1, 1}, {"0", 0, 0}, {"1", 1, 1}, {"2", 2, 1}, {"7", 1, 1}, {"off", 1, 1}};
    const char* names[3] = {"HONERF_LIVE_FIRST", "HONERF_UNIFORM_STASH", "HONERF_FAR_TILES"};
    int bad = 0;
    for (int v = 0; v < 3; ++v) unsetenv(names[v]);
    // one variable at a time, the other two unset: each switch follows its own variable and no other
    for (int v = 0; v < 3; ++v) {
        for (const Case& c : cases) {
            if (c.value != nullptr)
                setenv(names[v], c.value, 1);
            else
                unsetenv(names[v]);
            int live_first = -1;
            const hn::FieldLaunchOpts o = hn::resolve_launch_opts(&live_first);
            const int got[3] = {live_first, o.uniform_stash, o.far_tiles};
            for (int w = 0; w < 3; ++w) {
                const int want = w != v ? 1 : (w == 2 ? c.two_way : c.three_way);
                if (got[w] != want) {
                    printf("%s=%s: %s resolved to %d, expected %d\n", names[v], c.value ? c.value : "(unset)", names[w], got[w], want);
                    ++bad;
                }
            }
            // the resolve leaves everything that is not an environment switch at its default, and works without the live-first slot
            const hn::FieldLaunchOpts p = hn::resolve_launch_opts();
            bad += o.n_pts_dev != nullptr || o.orig_idx != nullptr || o.frame_seg != nullptr || o.dir_per_sample || o.three_pass;
            bad += p.uniform_stash != o.uniform_stash || p.far_tiles != o.far_tiles;
        }
        unsetenv(names[v]);
    }
    const hn::FieldLaunchOpts d;
    if (d.n_pts_dev != nullptr || d.orig_idx != nullptr || d.frame_seg != nullptr || d.dir_per_sample || d.three_pass || d.uniform_stash != 1 ||
        d.far_tiles != 1) {
        printf("a default-constructed FieldLaunchOpts is not all-null / all-false / switches at 1\n");
        ++bad;
    }
    if (bad) {
        printf("FAILED\n");
        return 1;
    }
    printf("launch opts: ok\n");
    return 0;
}
