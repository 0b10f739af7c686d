// The launch geometry (csrc/nmpc_launch.h) compiled for the host: for every grid_cap given on the command line, both kernel families,
// ordering on and off, and the knob settings below, one line per batch size B = 0 .. 3 * grid_cap + 2:
//   grid_cap P use_order park_min sched_mode forced B : grid owners workgroups ordered pools pool_cap
// tests/test_launch_geometry.py compares the lines with a literal restatement of the rule.
#include <cstdio>
#include <cstdlib>

#include "nmpc_launch.h"

int main(int argc, char **argv)
{
    static const int knobs[][3] = {      // park_min, sched_mode, team_owners_forced: the handle's defaults first
        {500, 1, 0}, {0, 1, 0}, {500, 0, 0}, {0, 0, 0}, {500, 1, 1}, {500, 1, 2}, {500, 1, 3}, {500, 1, 4}};
    for (int i = 1; i < argc; ++i) {
        const int cap = std::atoi(argv[i]);
        for (int P = 20; P <= 40; P += 20)
            for (int order = 0; order < 2; ++order)
                for (const auto &k : knobs)
                    for (int B = 0; B <= 3 * cap + 2; ++B) {
                        const nmpc::LaunchGeometry g = nmpc::launch_geometry(B, cap, P, order != 0, k[0], k[1], k[2]);
                        std::printf("%d %d %d %d %d %d %d : %d %d %d %d %d %d\n", cap, P, order, k[0], k[1], k[2], B, g.grid, g.owners,
                                    g.workgroups, g.ordered, g.pools, g.pool_cap);
                    }
    }
    return 0;
}
