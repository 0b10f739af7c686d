// nmpc_launch.h -- the launch geometry of a batch solve: how many waves take instances, how they are grouped into teams, and whether the
// launch orders its instances and gives them pools to wait in.  Plain host arithmetic on integers, no HIP header: solve_launch
// (nmpc_kernels.hip) launches by it, nmpc_launch_geometry reports it, and tests/launch_geometry_main.cpp compiles it for the host under
// the sanitizers and prints it for every batch size (tests/test_launch_geometry.py holds the lines to the rule of DESIGN.md section 5.5).
#ifndef NMPC_LAUNCH_H
#define NMPC_LAUNCH_H

namespace nmpc {

constexpr int LAUNCH_TEAM_WAVES = 4;      // waves of a workgroup (nmpc_layout.h's TEAM_WAVES; nmpc_kernels.hip asserts that they agree)

struct LaunchGeometry {
    int grid;          // waves that take instances: min(B, grid_cap)
    int owners;        // waves per workgroup that take instances, 1..4; the others help
    int workgroups;    // workgroups launched, at most grid_cap / 4
    int ordered;       // the hard-looking instances are handed out first (classify + order kernels run)
    int pools;         // instances may leave their wave at outer-iteration boundaries (pools and their counters are cleared)
    int pool_cap;      // slots of each pool's ring in this launch: an instance waits in at most one slot at a time
};

// B instances on a handle sized for grid_cap resident waves (a positive multiple of four).  P: the kernel family, 20 = one stage per lane,
// 40 = two; use_order, park_min, sched_mode, team_owners_forced: the handle's fields of those names (the last 0 = automatic).
inline LaunchGeometry launch_geometry(int B, int grid_cap, int P, bool use_order, int park_min, int sched_mode, int team_owners_forced)
{
    LaunchGeometry g{};
    g.grid = B < grid_cap ? B : grid_cap;
    // more instances than resident waves: hand the hard-looking ones out first, and let instances leave their wave (the slot migration is
    // the one-stage kernel's: two waves per SIMD)
    const bool beyond = B > g.grid;
    g.ordered = beyond && use_order;
    g.pools = beyond && ((P == 20 && (park_min > 0 || sched_mode > 0)) || (P == 40 && sched_mode > 0));
    g.pool_cap = B;
    // teams of four waves.  With fewer instances than workgroups fit on the chip every instance gets a workgroup of its own (one wave
    // solves, three help from the first iteration on: the small-batch / latency mode); otherwise as many waves per workgroup take
    // instances as it needs for all of them to start at once, up to all four.
    int max_wgs = grid_cap / LAUNCH_TEAM_WAVES;
    if (max_wgs < 1) max_wgs = 1;                  // (no handle has fewer than four resident waves)
    int owners = (B + max_wgs - 1) / max_wgs;
    if (owners < 1) owners = 1;                    // (B = 0, which launches nothing)
    if (owners > LAUNCH_TEAM_WAVES) owners = LAUNCH_TEAM_WAVES;
    if (team_owners_forced > 0) owners = team_owners_forced;
    int wgs = (g.grid + owners - 1) / owners;
    if (wgs > max_wgs) wgs = max_wgs;
    g.owners = owners;
    g.workgroups = wgs;
    return g;
}

}  // namespace nmpc
#endif
