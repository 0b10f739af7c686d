// nmpc_loop_host.h -- host side of the receding-horizon loop on device (its kernels: nmpc_loop.h): struct nmpc_loop and the nmpc_loop_*
// entry points of include/nmpc_solver.h.  Part of the one translation unit: nmpc_kernels.hip includes it inside its extern "C" block,
// after the handle, fail, HIP_TRY and solve_launch.
//
// A loop is its view (nmpc::LoopView: the shape, the per-robot arrays and the active list, the same for every kernel), its base
// (assemble -> solve -> advance) and up to eleven stages, each a sub-struct with its device buffers and the argument block of its own
// kernels.  A setter makes its stage whole in a local and moves it into the loop, so a refused or failed call leaves the loop as it
// was, and a stage is on when it is made.  Setters come in any order but not after the first step, so step 0 finds the configuration
// final.  The loop keeps ONE counter, `steps`: nmpc_loop_step derives everything that changes per step from it and the active count
// (nmpc::LoopStep, on its stack), hands view, step and a stage's block to each kernel, and writes to no argument block.  It is ONE
// sequence of kernels in which a stage adds its own; the pointers that cross stages (the predicted poses, which peers and crowd share
// and the loop owns, for the compaction; retirement's retired_at for the monitor and the ensemble; the missions' leg for the log) are passed at the
// launch, from the stage that owns them.
#pragma once

// member lists of the groups 0 .. B - 1 (most of them empty), each group's robots in ascending index
struct LoopGroups {
    DevBuf<int> group_of, goff, gmem;      // [B], [B + 1], [B]
    nmpc::GroupLists lists() const { return {group_of, goff, gmem}; }
    // group_of NULL: everybody in group 0
    hipError_t upload(const int32_t *of, int B)
    {
        std::vector<int> gof(B, 0), off(B + 1, 0), mem(B);
        if (of) for (int b = 0; b < B; ++b) gof[b] = of[b];
        for (int b = 0; b < B; ++b) off[gof[b] + 1]++;
        for (int g = 0; g < B; ++g) off[g + 1] += off[g];
        {
            std::vector<int> at(off.begin(), off.end() - 1);
            for (int b = 0; b < B; ++b) mem[at[gof[b]]++] = b;
        }
        hipError_t e = group_of.upload(gof.data(), B);
        if (e == hipSuccess) e = goff.upload(off.data(), (size_t)B + 1);
        if (e == hipSuccess) e = gmem.upload(mem.data(), B);
        return e;
    }
};
struct LoopPeers {           // nmpc_loop_set_peers: two more kernels per step, between the assembly and the solve
    nmpc::PeerArgs a{};
    LoopGroups groups;
    // nmpc_loop_set_peers_grid: the candidates come from a grid, three kernels in the place of the all-pairs one
    nmpc::PeerGridArgs g{};
    DevBuf<double> box;              // [B][4]
    DevBuf<nmpc_peer_grid> hdr;      // [1]
    DevBuf<int> cell_of, cell_off, cell_cur, cell_mem;      // [B], [CAP * CAP + 1], [CAP * CAP], [B]
    bool made() const { return groups.group_of != nullptr; }
    bool grid() const { return box != nullptr; }
};
// nmpc_loop_set_crowd: one kernel per step that advances the world's table, one between the assembly and the solve; with the observer
// (nmpc_loop_set_crowd_monitor) one more after the advance
struct LoopCrowd {
    nmpc::CrowdArgs a{};
    DevBuf<double> obst, tab[2];     // [D][10], [D][N][5] twice
    DevBuf<int> seen;                // [B][M]
    DevBuf<nmpc_crowd_clearance> rec;    // [B]: the observer's
    // nmpc_loop_set_crowd_grid: the obstacles a robot measures come from a grid in space and stage, filed anew every step: five kernels
    // behind the table's advance, and nmpc_loop_crowd_grid_kernel in the place of nmpc_loop_crowd_kernel
    nmpc::CrowdGridArgs g{};
    nmpc_crowd_grid hdr{};               // (filed: read from the device when asked for)
    DevBuf<int> cell_of, cell_off, tile_sum, cell_cur, cell_mem, looked;      // [D][N], [cells + 1], [tiles], [cells], [D * N], [B]
    bool made() const { return obst != nullptr; }
    bool watched() const { return rec != nullptr; }
    bool grid() const { return cell_off != nullptr; }
};
// nmpc_loop_set_retire: robots at their goal leave the loop.  A step runs over the active list, the solve over gathered rows, and
// the host learns the list's length one step late (nmpc_loop.h)
struct LoopRetire {
    bool called = false;         // the setter has been taken, with on = 0 too
    nmpc::RetireArgs a{};
    DevBuf<int> act, nact, retired_at;
    DevBuf<double> sP, sU, sY;
    DevBuf<nmpc_status> sst;
    PinBuf h_nact;               // one int: the active robots after the last compaction whose event was waited for
    Event ev_nact;               // recorded behind the copy of the count
    bool nact_pending = false;   // a copy is under way: wait for ev_nact before h_nact is read
    bool made() const { return act != nullptr; }
};
struct LoopMonitor {         // nmpc_loop_set_monitor: one more kernel per step, after the advance
    nmpc::MonitorArgs a{};
    LoopGroups groups;
    DevBuf<nmpc_clearance> rec;      // [B]
    bool made() const { return rec != nullptr; }
};
// The walls grid on the device, for the two stages that find edges through it (nmpc_loop_set_walls_grid, nmpc_loop_set_map_monitor_grid):
// what WallGridHost::build made, uploaded, and the kernels' argument block
struct WallGridHost;
struct LoopWallGrid {
    nmpc::WallGridArgs g{};
    nmpc_wall_grid hdr{};
    DevBuf<int> cell_off, cell_edge, cell_tag, looked;     // [nx * ny + 1], [entries], [entries], [B]
    bool made() const { return cell_off != nullptr; }
    hipError_t upload(const WallGridHost &gh, double range, size_t B);
    // what nmpc_loop_wall_grid and nmpc_loop_map_grid copy out (NULL = skip)
    hipError_t read(nmpc_wall_grid *out, int32_t *off, int32_t *edge, int32_t *seen, size_t B) const
    {
        if (out) *out = hdr;
        hipError_t e = cell_off.read(off, (size_t)hdr.nx * hdr.ny + 1);
        if (e == hipSuccess) e = cell_edge.read(edge, (size_t)hdr.entries);
        if (e == hipSuccess) e = looked.read(seen, B);
        return e;
    }
};
struct LoopMap {             // nmpc_loop_set_map_monitor: one more kernel per step, after the advance and the clearance monitor
    nmpc::MapArgs a{};
    DevBuf<double> edge;             // [E][4]
    DevBuf<int> poly_off, edge_poly; // [n_poly + 1], [E]
    DevBuf<nmpc_map_clearance> rec;  // [B]
    LoopWallGrid grid;               // nmpc_loop_set_map_monitor_grid: nmpc_loop_map_grid_kernel in the place of nmpc_loop_map_kernel
    bool made() const { return rec != nullptr; }
};
// nmpc_loop_set_track_monitor: one more kernel per step, after the advance and the other monitors and before the log and the dispatch
struct LoopTrack {
    nmpc::TrackArgs a{};
    DevBuf<nmpc_tracking> rec;       // [B]
    bool made() const { return rec != nullptr; }
};
// nmpc_loop_set_missions: a robot at its goal takes up the next route of its mission; one more kernel per step, before the compaction
struct LoopMissions {
    nmpc::DispatchArgs a{};
    DevBuf<int> leg_off, leg_route, leg, leg_at;
    int n_legs = 0;                  // leg_off[B]
    bool made() const { return leg_off != nullptr; }
};
// nmpc_loop_set_log: two more kernels per step, after the advance and the monitors and before the dispatch
struct LoopLog {
    nmpc::LogArgs a{};
    DevBuf<double> ctrl;             // [max_steps * s][B][2]
    DevBuf<nmpc_step_record> rec;    // [max_steps][B]
    DevBuf<nmpc_drive_summary> sum;  // [B]
    DevBuf<nmpc_step_totals> tot;    // [max_steps]
    bool made() const { return sum != nullptr; }
};
// nmpc_loop_set_plant: the plant kernel in the place of the advance, and with measurement noise one more kernel in front of the assembly
struct LoopPlant {
    bool on = false;
    nmpc::PlantArgs a{};
    DevBuf<double> meas;             // [B][3]: the measured poses, the start states until a step measures
    DevBuf<unsigned> ids;            // [B], or none: robot b has id b
    DevBuf<double> applied;          // [max_steps * s][B][2] if kept
    bool made() const { return on; }
    bool measures() const { return a.meas[0] > 0.0 || a.meas[1] > 0.0 || a.meas[2] > 0.0; }
};
struct LoopWalls {           // nmpc_loop_set_walls: one more kernel per step, between the peers' kernels and the solve
    nmpc::WallArgs a{};
    DevBuf<double> edge;             // [E][4]
    DevBuf<int> wall_edge, wall_stage;   // [B][M] each
    // nmpc_loop_set_walls_grid: the edges a robot measures come from a grid built by the setter, nmpc_loop_walls_grid_kernel in the place
    // of nmpc_loop_walls_kernel
    LoopWallGrid grid;
    bool made() const { return edge != nullptr; }
};
struct LoopEnsemble {        // nmpc_loop_set_ensemble: one more kernel per step, the step's last
    nmpc::EnsembleArgs a{};
    DevBuf<int> goff, gmem;              // [G + 1], [B]: the groups' members, ascending inside a group
    DevBuf<nmpc_ensemble_stat> ens;      // [max_steps][G]
    bool made() const { return ens != nullptr; }
};

struct nmpc_loop {
    nmpc_handle *h = nullptr;
    nmpc::LoopView v{};          // what every kernel sees of the loop; act is the retirement setter's, the rest final at creation
    nmpc::AssembleArgs a{};
    int steps = 0, max_steps = 0;        // steps taken: the loop's one counter (nmpc::LoopStep::after)
    int R = 1;
    std::vector<int> h_route_of;         // [B] as given at creation
    std::vector<int> h_n_vert;           // [R]: every route's vertices, for the walls setter
    DevBuf<double> d_tab;        // every route's tables, one allocation
    DevBuf<nmpc::LoopRoute> d_routes;   // [R]
    DevBuf<int> d_route_of;      // [B]
    DevBuf<double> d_dynpar, d_state, d_last_u, d_dyn[2], d_P, d_U, d_Y, d_traj;
    DevBuf<int> d_idx;
    DevBuf<unsigned char> d_done;
    DevBuf<nmpc_status> d_st;
    DevBuf<double> d_pred;       // [B][N][3]: every robot's predicted poses, made by the first of the peers, crowd and walls setters
    LoopPeers peers;
    LoopCrowd crowd;
    LoopRetire retire;
    LoopMonitor monitor;
    LoopMap map;
    LoopTrack track;
    LoopMissions missions;
    LoopLog log;
    LoopPlant plant;
    LoopEnsemble ensemble;
    LoopWalls walls;
};

static bool route_ok(const nmpc_handle *h, const nmpc_route *r)
{
    return r->n_ref >= 1 && r->n_vert >= 0 && r->n_brake >= 1 && r->num_steps_taken >= 1 && r->num_steps_taken <= h->pb.N &&
           r->x_ref && r->y_ref && r->theta_ref && r->brake_vel && r->brake_dist && (r->n_vert == 0 || r->vert_xy);
}

void nmpc_loop_free(nmpc_loop *l)
{
    if (!l) return;
    (void)hipSetDevice(l->h->device);
    delete l;
}

int nmpc_loop_new_routes(nmpc_handle *h, const nmpc_route *routes, int R, const int32_t *route_of, int B, const double *starts,
                         const int32_t *idx0, int K, const double *dyn, int max_steps, nmpc_loop **out)
{
    if (!h || !routes || !out || !starts) return NMPC_ERR_BAD_ARG;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    if (B < 1 || B > h->max_batch || K < 0 || K > h->pb.ndyn || (K > 0 && !dyn) || max_steps < 0)
        return fail(h, NMPC_ERR_BAD_ARG, "bad loop arguments");
    if (R < 1) return fail(h, NMPC_ERR_BAD_ARG, "R < 1: no route");
    if (!route_of && R > 1) return fail(h, NMPC_ERR_BAD_ARG, "route_of == NULL with R > 1");
    if (route_of) for (int b = 0; b < B; ++b) if (route_of[b] < 0 || route_of[b] >= R) return fail(h, NMPC_ERR_BAD_ARG, "route_of out of range");
    size_t ntab = 0;
    for (int i = 0; i < R; ++i) {
        const nmpc_route *r = routes + i;
        if (!route_ok(h, r)) return fail(h, NMPC_ERR_BAD_ARG, R == 1 ? "bad route" : ("bad route " + std::to_string(i)).c_str());
        if (r->num_steps_taken != routes[0].num_steps_taken)
            return fail(h, NMPC_ERR_BAD_ARG, "routes differ in num_steps_taken (the fleet moves in lock step)");
        ntab += 3 * (size_t)r->n_ref + 2 * (size_t)r->n_vert + 2 * (size_t)r->n_brake;
    }
    if (ntab > 0x7fffffff) return fail(h, NMPC_ERR_BAD_ARG, "route tables too large");
    if (idx0) for (int b = 0; b < B; ++b) if (idx0[b] < 0 || idx0[b] >= routes[route_of ? route_of[b] : 0].n_ref) return fail(h, NMPC_ERR_BAD_ARG, "idx0 out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    // (a return below releases what the loop holds so far, on its device)
    std::unique_ptr<nmpc_loop, decltype(&nmpc_loop_free)> l(new nmpc_loop(), nmpc_loop_free);
    l->h = h;
    l->max_steps = max_steps;
    l->R = R;
    nmpc::LoopView &v = l->v;
    v.B = B; v.N = h->pb.N; v.nobs = h->pb.nobs; v.ndyn = h->pb.ndyn; v.K = K;
    v.n_p = nmpc_n_p(&h->pb); v.n_u = nmpc_n_u(&h->pb); v.n1 = nmpc_n1(&h->pb);
    v.s = routes[0].num_steps_taken;
    v.ts = h->pb.ts;
    const size_t ndynrow = (size_t)v.ndyn * v.N * 5;
    // route tables, route after route: x_ref | y_ref | theta_ref | vertices | brake velocities | brake distances
    std::vector<double> tab(ntab);
    std::vector<nmpc::LoopRoute> desc(R);
    size_t off = 0;
    for (int i = 0; i < R; ++i) {
        const nmpc_route *r = routes + i;
        nmpc::LoopRoute &d = desc[i];
        std::memset(&d, 0, sizeof(d));
        auto put = [&](const double *src, size_t n) { const int at = (int)off; if (n) std::memcpy(tab.data() + off, src, 8 * n); off += n; return at; };
        d.xr = put(r->x_ref, r->n_ref); d.yr = put(r->y_ref, r->n_ref); d.thr = put(r->theta_ref, r->n_ref);
        d.vert = put(r->vert_xy, 2 * (size_t)r->n_vert);
        d.bv = put(r->brake_vel, r->n_brake); d.bd = put(r->brake_dist, r->n_brake);
        d.n_ref = r->n_ref; d.n_vert = r->n_vert; d.n_brake = r->n_brake;
        for (int k = 0; k < 3; ++k) d.end[k] = r->end[k];
        d.base = r->base_speed; d.radius = r->radius; d.pad = r->dyn_pad;
        for (int k = 0; k < 10; ++k) d.w[k] = r->weights[k];
    }
    for (int i = 0; i < R; ++i) l->h_n_vert.push_back(routes[i].n_vert);
    l->h_route_of.assign(B, 0);
    if (route_of) l->h_route_of.assign(route_of, route_of + B);
    HIP_TRY(h, l->d_tab.upload(tab.data(), ntab));
    HIP_TRY(h, l->d_routes.upload(desc.data(), R));
    HIP_TRY(h, l->d_route_of.upload(l->h_route_of.data(), B));
    if (K) HIP_TRY(h, l->d_dynpar.upload(dyn, (size_t)B * K * 10));
    else HIP_TRY(h, l->d_dynpar.alloc(10 * (size_t)B));
    HIP_TRY(h, l->d_state.upload(starts, (size_t)B * 3));
    if (max_steps > 0) {
        HIP_TRY(h, l->d_traj.alloc(((size_t)max_steps * v.s + 1) * B * 3));
        HIP_TRY(h, hipMemcpy(l->d_traj, starts, (size_t)B * 3 * 8, hipMemcpyHostToDevice));
    }
    HIP_TRY(h, l->d_last_u.alloc_fill((size_t)B * 2, 0));
    HIP_TRY(h, l->d_P.alloc((size_t)B * v.n_p));
    HIP_TRY(h, l->d_U.alloc_fill((size_t)B * v.n_u, 0));
    HIP_TRY(h, l->d_Y.alloc_fill((size_t)B * v.n1, 0));
    if (idx0) HIP_TRY(h, l->d_idx.upload(idx0, B));
    else HIP_TRY(h, l->d_idx.alloc_fill(B, 0));
    HIP_TRY(h, l->d_done.alloc_fill(B, 0));
    HIP_TRY(h, l->d_st.alloc_fill(B, 0));
    {          // padding block: zeros with unit radii (path_generator.py:274-280)
        std::vector<double> pad(B * (ndynrow ? ndynrow : 1), 0.0);
        for (size_t i = 0; ndynrow && i < pad.size(); i += 5) { pad[i + 2] = 1.0; pad[i + 3] = 1.0; }
        HIP_TRY(h, l->d_dyn[0].upload(pad.data(), pad.size()));
        HIP_TRY(h, l->d_dyn[1].alloc(pad.size()));
    }
    v.state = l->d_state; v.last_u = l->d_last_u; v.idx = l->d_idx; v.done = l->d_done;
    v.P = l->d_P; v.U = l->d_U; v.Y = l->d_Y; v.st = l->d_st; v.route_of = l->d_route_of; v.traj = l->d_traj;
    nmpc::AssembleArgs &a = l->a;
    a.tab = l->d_tab; a.routes = l->d_routes; a.dynpar = l->d_dynpar; a.dyn[0] = l->d_dyn[0]; a.dyn[1] = l->d_dyn[1];
    *out = l.release();
    return NMPC_OK;
}

int nmpc_loop_new(nmpc_handle *h, const nmpc_route *r, int B, const double *starts, const int32_t *idx0, int K,
                  const double *dyn, int max_steps, nmpc_loop **out)
{
    return nmpc_loop_new_routes(h, r, 1, nullptr, B, starts, idx0, K, dyn, max_steps, out);
}

// what every setter checks first, l != NULL given: a live handle, a loop that has not taken its first step and does not have
// the setter's stage yet.  Leaves the loop's device current.
static int loop_setter(nmpc_loop *l, const char *fn, bool has, const char *already)
{
    nmpc_handle *h = l->h;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    if (has) return fail(h, NMPC_ERR_BAD_ARG, (std::string(fn) + ": " + already).c_str());
    if (l->steps > 0) return fail(h, NMPC_ERR_BAD_ARG, (std::string(fn) + ": after the loop's first step").c_str());
    HIP_TRY(h, hipSetDevice(h->device));
    return NMPC_OK;
}

// both peers setters: `cell` NULL = all pairs (nmpc_loop_set_peers), else the grid's edge
static int loop_set_peers(nmpc_loop *l, const char *fn, const int32_t *group_of, int M, double rx, double ry, double range, const double *cell)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, fn, l->peers.made(), "the loop has its peers already")) return rc;
    nmpc_handle *h = l->h;
    const nmpc::LoopView &v = l->v;
    const int B = v.B;
    const std::string who = std::string(fn) + ": ";
    if (M < 1) return fail(h, NMPC_ERR_BAD_ARG, (who + "M < 1").c_str());
    const int Mc = l->crowd.a.M;       // the crowd's slots come first (0 without a crowd)
    if (v.K + Mc + M > v.ndyn) return fail(h, NMPC_ERR_BAD_ARG, (who + (Mc ? "K + the crowd's M + M > Ndynobs, no free ellipse slot" : "K + M > Ndynobs, no free ellipse slot")).c_str());
    for (const double v : {rx, ry, range})
        if (!(v > 0.0) || v > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, (who + "rx, ry and range must be finite and positive").c_str());
    if (cell && (!(*cell > 0.0) || *cell > DBL_MAX)) return fail(h, NMPC_ERR_BAD_ARG, (who + "cell must be finite and positive").c_str());
    if (group_of) for (int b = 0; b < B; ++b) if (group_of[b] < 0 || group_of[b] >= B) return fail(h, NMPC_ERR_BAD_ARG, (who + "group_of out of range").c_str());
    LoopPeers st;
    DevBuf<double> pred;           // the loop's, unless the crowd has made it
    if (!l->d_pred) HIP_TRY(h, pred.alloc((size_t)B * v.N * 3));
    HIP_TRY(h, st.groups.upload(group_of, B));
    nmpc::PeerArgs &p = st.a;
    p.M = M; p.first = v.K + Mc; p.rx = rx; p.ry = ry; p.range2 = range * range;
    p.pred = l->d_pred.p ? l->d_pred.p : pred.p; p.grp = st.groups.lists();
    if (cell) {
        constexpr size_t cells = (size_t)nmpc::PEER_GRID_CAP * nmpc::PEER_GRID_CAP;
        HIP_TRY(h, st.box.alloc(4 * (size_t)B));
        HIP_TRY(h, st.hdr.alloc_fill(1, 0));
        HIP_TRY(h, st.cell_of.alloc_fill(B, 0xFF));
        HIP_TRY(h, st.cell_off.alloc_fill(cells + 1, 0));
        HIP_TRY(h, st.cell_cur.alloc_fill(cells, 0));
        HIP_TRY(h, st.cell_mem.alloc_fill(B, 0));
        nmpc::PeerGridArgs &g = st.g;
        g.range = range; g.cell = *cell;
        g.box = st.box; g.hdr = st.hdr;
        g.cell_of = st.cell_of; g.cell_off = st.cell_off; g.cell_cur = st.cell_cur; g.cell_mem = st.cell_mem;
    }
    l->peers = std::move(st);
    if (pred) l->d_pred = std::move(pred);
    return NMPC_OK;
}

static constexpr int CROWD_MAX = 16384;
static const nmpc_crowd_clearance CROWD_CLEARANCE_NONE = {__builtin_inf(), -1, -1};

// The geometry of nmpc_loop_set_crowd_grid, fixed by the setter (the rule: DESIGN.md section 5.9; trajectory.crowd_grid is its NumPy
// statement): over the end points of obst [D][10] whose two coordinates are finite, with the functions of nmpc_geom.h only.
static nmpc_crowd_grid crowd_grid_geometry(int D, const double *obst, double cell, int N)
{
    const double inf = __builtin_inf();
    double lx = inf, ly = inf, hx = -inf, hy = -inf;
    for (int d = 0; d < D; ++d) {
        const double *q = obst + 10 * (size_t)d;
        nmpc::box_fold(q[0], q[1], lx, ly, hx, hy);
        nmpc::box_fold(q[2], q[3], lx, ly, hx, hy);
    }
    nmpc_crowd_grid g{};
    g.nx = g.ny = 1; g.h[0] = g.h[1] = cell; g.layers = N;
    if (lx <= hx) {
        g.origin[0] = lx; g.origin[1] = ly;
        nmpc::grid_axis(hx - lx, cell, nmpc::CROWD_GRID_CAP, g.nx, g.h[0]);
        nmpc::grid_axis(hy - ly, cell, nmpc::CROWD_GRID_CAP, g.ny, g.h[1]);
    }
    return g;
}

// both crowd setters: `cell` NULL = every obstacle against every robot (nmpc_loop_set_crowd), else the grid's cell
static int loop_set_crowd(nmpc_loop *l, const char *name, int max_D, int D, const double *obst, double pad, int M, double range, const double *cell)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, name, l->crowd.made(), "the loop has its crowd already")) return rc;
    nmpc_handle *h = l->h;
    const nmpc::LoopView &v = l->v;
    const size_t B = (size_t)v.B;
    const std::string fn = std::string(name) + ": ";
    if (D < 1 || D > max_D) return fail(h, NMPC_ERR_BAD_ARG, (fn + "D outside 1 .. " + std::to_string(max_D)).c_str());
    if (!obst) return fail(h, NMPC_ERR_BAD_ARG, (fn + "obst is NULL").c_str());
    if (M < 1) return fail(h, NMPC_ERR_BAD_ARG, (fn + "M < 1").c_str());
    const int Mp = l->peers.made() ? l->peers.a.M : 0;
    if (v.K + M + Mp > v.ndyn)
        return fail(h, NMPC_ERR_BAD_ARG, (fn + (Mp ? "K + M + the peers' M > Ndynobs, no free ellipse slot" : "K + M > Ndynobs, no free ellipse slot")).c_str());
    if (!(pad >= -DBL_MAX && pad <= DBL_MAX)) return fail(h, NMPC_ERR_BAD_ARG, (fn + "pad must be finite").c_str());
    if (!(range > 0.0) || range > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, (fn + "range must be finite and positive").c_str());
    if (cell && (!(*cell > 0.0) || *cell > DBL_MAX)) return fail(h, NMPC_ERR_BAD_ARG, (fn + "cell must be finite and positive").c_str());
    LoopCrowd st;
    DevBuf<double> pred;           // the loop's, unless the peers have made it
    if (!l->d_pred) HIP_TRY(h, pred.alloc(B * v.N * 3));
    const size_t ntab = (size_t)D * v.N * 5;
    HIP_TRY(h, st.obst.upload(obst, (size_t)D * 10));
    HIP_TRY(h, st.tab[0].alloc_fill(ntab, 0));
    HIP_TRY(h, st.tab[1].alloc_fill(ntab, 0));
    HIP_TRY(h, st.seen.alloc_fill(B * M, 0xFF));                   // seen = -1
    nmpc::CrowdArgs &c = st.a;
    c.D = D; c.M = M; c.pad = pad; c.range2 = range * range;
    c.obst = st.obst; c.tab[0] = st.tab[0]; c.tab[1] = st.tab[1];
    c.pred = l->d_pred.p ? l->d_pred.p : pred.p; c.seen = st.seen; c.rec = nullptr;
    if (cell) {
        st.hdr = crowd_grid_geometry(D, obst, *cell, v.N);
        const size_t cells = (size_t)v.N * st.hdr.nx * st.hdr.ny, entries = (size_t)D * v.N;
        HIP_TRY(h, st.cell_of.alloc_fill(entries, 0xFF));          // -1
        HIP_TRY(h, st.cell_off.alloc_fill(cells + 1, 0));
        HIP_TRY(h, st.cell_cur.alloc_fill(cells, 0));
        HIP_TRY(h, st.tile_sum.alloc_fill((cells + nmpc::CROWD_GRID_TILE) / nmpc::CROWD_GRID_TILE, 0));
        HIP_TRY(h, st.cell_mem.alloc_fill(entries, 0));
        HIP_TRY(h, st.looked.alloc_fill(B, 0));
        nmpc::CrowdGridArgs &g = st.g;
        for (int ax = 0; ax < 2; ++ax) { g.origin[ax] = st.hdr.origin[ax]; g.h[ax] = st.hdr.h[ax]; }
        g.nx = st.hdr.nx; g.ny = st.hdr.ny; g.cells = (int)cells; g.range = range;
        g.cell_of = st.cell_of; g.cell_off = st.cell_off; g.tile_sum = st.tile_sum; g.cell_cur = st.cell_cur; g.cell_mem = st.cell_mem; g.looked = st.looked;
    }
    l->crowd = std::move(st);
    if (pred) l->d_pred = std::move(pred);
    if (l->peers.made()) l->peers.a.first = v.K + M;       // the peers' slots follow the crowd's
    return NMPC_OK;
}

int nmpc_loop_set_crowd(nmpc_loop *l, int D, const double *obst, double pad, int M, double range)
{
    return loop_set_crowd(l, "nmpc_loop_set_crowd", CROWD_MAX, D, obst, pad, M, range, nullptr);
}

int nmpc_loop_set_crowd_grid(nmpc_loop *l, int D, const double *obst, double pad, int M, double range, double cell)
{
    return loop_set_crowd(l, "nmpc_loop_set_crowd_grid", nmpc::CROWD_GRID_MAX, D, obst, pad, M, range, &cell);
}

int nmpc_loop_set_crowd_monitor(nmpc_loop *l)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_crowd_monitor", l->crowd.watched(), "the loop has its crowd observer already")) return rc;
    nmpc_handle *h = l->h;
    if (!l->crowd.made()) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_crowd_monitor: the loop has no crowd (nmpc_loop_set_crowd first)");
    if (!l->d_traj) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_crowd_monitor: the loop records no trajectory (max_steps == 0)");
    DevBuf<nmpc_crowd_clearance> rec;
    const std::vector<nmpc_crowd_clearance> none(l->v.B, CROWD_CLEARANCE_NONE);
    HIP_TRY(h, rec.upload(none.data(), none.size()));
    l->crowd.rec = std::move(rec);
    l->crowd.a.rec = l->crowd.rec;
    return NMPC_OK;
}

int nmpc_loop_set_peers(nmpc_loop *l, const int32_t *group_of, int M, double rx, double ry, double range)
{
    return loop_set_peers(l, "nmpc_loop_set_peers", group_of, M, rx, ry, range, nullptr);
}

int nmpc_loop_set_peers_grid(nmpc_loop *l, const int32_t *group_of, int M, double rx, double ry, double range, double cell)
{
    return loop_set_peers(l, "nmpc_loop_set_peers_grid", group_of, M, rx, ry, range, &cell);
}

int nmpc_loop_set_retire(nmpc_loop *l, int on)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_retire", l->retire.called, "called already")) return rc;
    nmpc_handle *h = l->h;
    const nmpc::LoopView &v = l->v;
    const size_t B = (size_t)v.B;
    LoopRetire st;
    st.called = true;
    if (on) {
        std::vector<int> all(B);
        for (size_t b = 0; b < B; ++b) all[b] = (int)b;
        HIP_TRY(h, st.act.upload(all.data(), B));                  // everybody is active at step 0
        HIP_TRY(h, st.nact.upload(&v.B, 1));
        HIP_TRY(h, st.retired_at.alloc_fill(B, 0xFF));             // retired_at = -1
        HIP_TRY(h, st.sP.alloc(B * v.n_p));
        HIP_TRY(h, st.sU.alloc(B * v.n_u));
        HIP_TRY(h, st.sY.alloc(B * v.n1));
        HIP_TRY(h, st.sst.alloc(B));
        HIP_TRY(h, st.h_nact.alloc(sizeof(int)));
        HIP_TRY(h, st.ev_nact.create(hipEventDisableTiming));
        *(int *)st.h_nact.p = v.B;
        nmpc::RetireArgs &r = st.a;
        r.retired_at = st.retired_at; r.list = st.act; r.count = st.nact;
        r.sP = st.sP; r.sU = st.sU; r.sY = st.sY; r.sst = st.sst;
    }
    l->retire = std::move(st);
    l->v.act = l->retire.act;      // the robots every kernel runs over from now on (NULL with on = 0: everybody)
    return NMPC_OK;
}

static const nmpc_clearance CLEARANCE_NONE = {__builtin_inf(), __builtin_inf(), __builtin_inf(), -1, -1, -1, -1};

int nmpc_loop_set_monitor(nmpc_loop *l, const int32_t *group_of)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_monitor", l->monitor.made(), "the loop has its monitor already")) return rc;
    nmpc_handle *h = l->h;
    const int B = l->v.B;
    if (!l->d_traj) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_monitor: the loop records no trajectory (max_steps == 0)");
    if (group_of) for (int b = 0; b < B; ++b) if (group_of[b] < 0 || group_of[b] >= B) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_monitor: group_of out of range");
    LoopMonitor st;
    const std::vector<nmpc_clearance> none(B, CLEARANCE_NONE);
    HIP_TRY(h, st.rec.upload(none.data(), B));
    HIP_TRY(h, st.groups.upload(group_of, B));
    st.a.grp = st.groups.lists(); st.a.rec = st.rec;
    l->monitor = std::move(st);
    return NMPC_OK;
}

// (the map monitor's setters stand behind the walls': they share the walls grid)

static_assert(sizeof(nmpc_tracking) == 64, "nmpc_tracking is 64 bytes");
static const nmpc_tracking TRACKING_NONE = {0.0, 0.0, 0.0, 0.0, 0, -1, -1, -1, -1, 0, -1, 0};

int nmpc_loop_set_track_monitor(nmpc_loop *l, double tol)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_track_monitor", l->track.made(), "the loop has its track monitor already")) return rc;
    nmpc_handle *h = l->h;
    const int B = l->v.B;
    if (!(tol >= 0.0) || tol > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_track_monitor: tol must be finite and not negative");
    if (!l->d_traj) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_track_monitor: the loop records no trajectory (max_steps == 0)");
    LoopTrack st;
    const std::vector<nmpc_tracking> none(B, TRACKING_NONE);
    HIP_TRY(h, st.rec.upload(none.data(), B));
    st.a.tol2 = tol * tol; st.a.rec = st.rec;
    l->track = std::move(st);
    return NMPC_OK;
}

int nmpc_loop_set_missions(nmpc_loop *l, const int32_t *leg_off, const int32_t *leg_route)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_missions", l->missions.made(), "the loop has its missions already")) return rc;
    nmpc_handle *h = l->h;
    const int B = l->v.B;
    if (!leg_off || !leg_route) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_missions: leg_off or leg_route is NULL");
    if (!l->retire.made()) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_missions: the loop does not retire its robots (nmpc_loop_set_retire first)");
    if (leg_off[0] != 0) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_missions: leg_off[0] != 0");
    for (int b = 0; b < B; ++b)
        if (leg_off[b + 1] <= leg_off[b]) return fail(h, NMPC_ERR_BAD_ARG, ("nmpc_loop_set_missions: robot " + std::to_string(b) + " has no leg").c_str());
    const int T = leg_off[B];
    for (int i = 0; i < T; ++i)
        if (leg_route[i] < 0 || leg_route[i] >= l->R) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_missions: leg_route out of range");
    for (int b = 0; b < B; ++b)
        if (leg_route[leg_off[b]] != l->h_route_of[b])
            return fail(h, NMPC_ERR_BAD_ARG, ("nmpc_loop_set_missions: the first leg of robot " + std::to_string(b) + " is not its route_of").c_str());
    LoopMissions st;
    HIP_TRY(h, st.leg_off.upload(leg_off, (size_t)B + 1));
    HIP_TRY(h, st.leg_route.upload(leg_route, T));
    HIP_TRY(h, st.leg.alloc_fill(B, 0));
    HIP_TRY(h, st.leg_at.alloc_fill(T, 0xFF));                     // leg_at = -1
    st.n_legs = T;
    nmpc::DispatchArgs &d = st.a;
    d.leg_off = st.leg_off; d.leg_route = st.leg_route; d.leg = st.leg; d.leg_at = st.leg_at;
    d.route_of = l->d_route_of;
    l->missions = std::move(st);
    return NMPC_OK;
}

static const nmpc_step_record STEP_RECORD_NONE = {-1, 0, 0, 0, 0.0, 0.0, 0.0};
static const nmpc_drive_summary DRIVE_SUMMARY_NONE = {0, 0, {0, 0, 0, 0, 0}, 0, 0, -1, -1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

int nmpc_loop_set_log(nmpc_loop *l)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_log", l->log.made(), "the loop has its log already")) return rc;
    nmpc_handle *h = l->h;
    const size_t B = (size_t)l->v.B, steps = (size_t)l->max_steps;
    if (!l->d_traj) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_log: the loop records no trajectory (max_steps == 0)");
    LoopLog st;
    HIP_TRY(h, st.ctrl.alloc_fill(steps * l->v.s * B * 2, 0));
    {
        const std::vector<nmpc_step_record> none(steps * B, STEP_RECORD_NONE);
        HIP_TRY(h, st.rec.upload(none.data(), none.size()));
    }
    const std::vector<nmpc_drive_summary> none(B, DRIVE_SUMMARY_NONE);
    HIP_TRY(h, st.sum.upload(none.data(), B));
    HIP_TRY(h, st.tot.alloc_fill(steps, 0));
    st.a.ctrl = st.ctrl; st.a.rec = st.rec; st.a.sum = st.sum; st.a.tot = st.tot;
    l->log = std::move(st);
    return NMPC_OK;
}

int nmpc_loop_set_plant(nmpc_loop *l, const nmpc_plant *plant, const uint32_t *ids)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_plant", l->plant.made(), "the loop has its plant already")) return rc;
    nmpc_handle *h = l->h;
    const nmpc::LoopView &v = l->v;
    const size_t B = (size_t)v.B;
    if (!plant) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_plant: plant is NULL");
    for (const double g : {plant->act_gain[0], plant->act_gain[1], plant->act_add[0], plant->act_add[1], plant->proc[0], plant->proc[1],
                           plant->proc[2], plant->meas[0], plant->meas[1], plant->meas[2]})
        if (!(g >= 0.0) || g > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_plant: every sigma must be finite and >= 0");
    if (plant->keep_applied && !l->d_traj)
        return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_plant: keep_applied on a loop that records no trajectory (max_steps == 0)");
    LoopPlant st;
    st.on = true;
    HIP_TRY(h, st.meas.alloc(B * 3));
    HIP_TRY(h, hipMemcpy(st.meas, l->d_state, B * 3 * sizeof(double), hipMemcpyDeviceToDevice));      // (no step yet: the start states)
    if (ids) HIP_TRY(h, st.ids.upload(ids, B));
    if (plant->keep_applied) HIP_TRY(h, st.applied.alloc_fill((size_t)l->max_steps * v.s * B * 2, 0));
    nmpc::PlantArgs &a = st.a;
    a.seed = plant->seed;
    for (int k = 0; k < 2; ++k) { a.act_gain[k] = plant->act_gain[k]; a.act_add[k] = plant->act_add[k]; }
    for (int k = 0; k < 3; ++k) { a.proc[k] = plant->proc[k]; a.meas[k] = plant->meas[k]; }
    a.ids = st.ids; a.meas_state = st.meas; a.applied = st.applied;
    l->plant = std::move(st);
    return NMPC_OK;
}

static constexpr int ENSEMBLE_MAX_GROUPS = 65536;

int nmpc_loop_set_ensemble(nmpc_loop *l, const int32_t *group_of, int G)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, "nmpc_loop_set_ensemble", l->ensemble.made(), "the loop has its ensemble already")) return rc;
    nmpc_handle *h = l->h;
    const int B = l->v.B;
    if (l->max_steps == 0) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_ensemble: the loop keeps no table per step (max_steps == 0)");
    if (G < 1 || G > ENSEMBLE_MAX_GROUPS) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_ensemble: G outside 1 .. 65536");
    if (!group_of && G != 1) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_ensemble: group_of == NULL with G != 1");
    if (group_of) for (int b = 0; b < B; ++b) if (group_of[b] < 0 || group_of[b] >= G) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_set_ensemble: group_of out of range");
    // the members group after group, each group's in ascending index (as LoopGroups::upload files its own)
    std::vector<int> off((size_t)G + 1, 0), mem(B);
    for (int b = 0; b < B; ++b) off[(group_of ? group_of[b] : 0) + 1]++;
    for (int g = 0; g < G; ++g) off[g + 1] += off[g];
    {
        std::vector<int> at(off.begin(), off.end() - 1);
        for (int b = 0; b < B; ++b) mem[at[group_of ? group_of[b] : 0]++] = b;
    }
    LoopEnsemble st;
    HIP_TRY(h, st.goff.upload(off.data(), off.size()));
    HIP_TRY(h, st.gmem.upload(mem.data(), B));
    HIP_TRY(h, st.ens.alloc_fill((size_t)l->max_steps * G, 0));
    st.a.G = G; st.a.goff = st.goff; st.a.gmem = st.gmem; st.a.ens = st.ens;
    l->ensemble = std::move(st);
    return NMPC_OK;
}

// The grid of nmpc_loop_set_walls_grid, built once on the host (the rule: DESIGN.md section 5.9; trajectory.wall_grid is its NumPy
// statement): the header, the CSR arrays and per filing its tag for nmpc_loop_walls_grid_kernel.  -> false if the filings exceed
// WALL_GRID_MAX_ENTRIES, with nothing allocated beyond the per-edge rectangles.
struct WallGridHost {
    nmpc_wall_grid hdr{};
    double amax = 0.0;
    std::vector<int> cell_off, cell_edge, cell_tag;
    bool build(int E, const double *edge, double cell)
    {
        double lo[2] = {edge[0], edge[1]}, hi[2] = {edge[0], edge[1]};
        for (int i = 0; i < 4 * E; ++i) {
            const double v = edge[i];
            lo[i & 1] = v < lo[i & 1] ? v : lo[i & 1];
            hi[i & 1] = v > hi[i & 1] ? v : hi[i & 1];
            amax = std::fabs(v) > amax ? std::fabs(v) : amax;
        }
        int n[2];
        for (int ax = 0; ax < 2; ++ax) {
            hdr.origin[ax] = lo[ax];
            nmpc::grid_axis(hi[ax] - lo[ax], cell, nmpc::WALL_GRID_CAP, n[ax], hdr.h[ax]);
        }
        hdr.nx = n[0]; hdr.ny = n[1];
        // every edge's rectangle of cells: c0, c1, r0, r1
        std::vector<int> rect(4 * (size_t)E);
        long long entries = 0;
        for (int e = 0; e < E; ++e) {
            const double *d = edge + 4 * (size_t)e;
            int *r = rect.data() + 4 * (size_t)e;
            r[0] = nmpc::cellof(d[0] < d[2] ? d[0] : d[2], lo[0], hdr.h[0], n[0]);
            r[1] = nmpc::cellof(d[0] < d[2] ? d[2] : d[0], lo[0], hdr.h[0], n[0]);
            r[2] = nmpc::cellof(d[1] < d[3] ? d[1] : d[3], lo[1], hdr.h[1], n[1]);
            r[3] = nmpc::cellof(d[1] < d[3] ? d[3] : d[1], lo[1], hdr.h[1], n[1]);
            entries += (long long)(r[1] - r[0] + 1) * (r[3] - r[2] + 1);
        }
        if (entries > nmpc::WALL_GRID_MAX_ENTRIES) return false;
        hdr.entries = (int)entries;
        const size_t cells = (size_t)n[0] * n[1];
        cell_off.assign(cells + 1, 0);
        for (int e = 0; e < E; ++e) {
            const int *r = rect.data() + 4 * (size_t)e;
            for (int j = r[2]; j <= r[3]; ++j)
                for (int i = r[0]; i <= r[1]; ++i) cell_off[(size_t)j * n[0] + i + 1]++;
        }
        for (size_t c = 0; c < cells; ++c) cell_off[c + 1] += cell_off[c];
        cell_edge.resize(entries); cell_tag.resize(entries);
        std::vector<int> at(cell_off.begin(), cell_off.end() - 1);
        for (int e = 0; e < E; ++e) {          // edges in ascending index: they ascend inside every cell
            const int *r = rect.data() + 4 * (size_t)e;
            for (int j = r[2]; j <= r[3]; ++j)
                for (int i = r[0]; i <= r[1]; ++i) {
                    const int k = at[(size_t)j * n[0] + i]++;
                    cell_edge[k] = e;
                    cell_tag[k] = (i - r[0]) | (j - r[2]) << 9 | r[0] << 18;
                }
        }
        return true;
    }
};

hipError_t LoopWallGrid::upload(const WallGridHost &gh, double range, size_t B)
{
    hipError_t e = cell_off.upload(gh.cell_off.data(), gh.cell_off.size());
    if (e == hipSuccess) e = cell_edge.upload(gh.cell_edge.data(), gh.cell_edge.size());
    if (e == hipSuccess) e = cell_tag.upload(gh.cell_tag.data(), gh.cell_tag.size());
    if (e == hipSuccess) e = looked.alloc_fill(B, 0);
    if (e != hipSuccess) return e;
    hdr = gh.hdr;
    for (int ax = 0; ax < 2; ++ax) { g.origin[ax] = gh.hdr.origin[ax]; g.h[ax] = gh.hdr.h[ax]; }
    g.nx = gh.hdr.nx; g.ny = gh.hdr.ny;
    g.range = range; g.slack = 0x1p-40 * (range + gh.amax) + 0x1p-500;
    g.cell_off = cell_off; g.cell_edge = cell_edge; g.cell_tag = cell_tag; g.looked = looked;
    return hipSuccess;
}

// both walls setters: `cell` NULL = every edge against every robot (nmpc_loop_set_walls), else the grid's cell
static int loop_set_walls(nmpc_loop *l, const char *name, int max_edge, int n_edge, const double *edge, int M, double radius, double range,
                          double spacing, const double *cell)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, name, l->walls.made(), "the loop has its walls already")) return rc;
    nmpc_handle *h = l->h;
    const nmpc::LoopView &v = l->v;
    const size_t B = (size_t)v.B;
    const std::string fn = std::string(name) + ": ";
    if (!edge) return fail(h, NMPC_ERR_BAD_ARG, (fn + "edge is NULL").c_str());
    if (n_edge < 1 || n_edge > max_edge) return fail(h, NMPC_ERR_BAD_ARG, (fn + "n_edge outside 1 .. " + std::to_string(max_edge)).c_str());
    for (int i = 0; i < 4 * n_edge; ++i)
        if (!(edge[i] >= -DBL_MAX && edge[i] <= DBL_MAX))
            return fail(h, NMPC_ERR_BAD_ARG, (fn + "a coordinate of edge " + std::to_string(i / 4) + " is not finite").c_str());
    if (M < 1) return fail(h, NMPC_ERR_BAD_ARG, (fn + "M < 1").c_str());
    if (M > v.nobs || M > nmpc::WALLS_MAX_SLOTS) return fail(h, NMPC_ERR_BAD_ARG, (fn + "M > Nobs, no such circle slot").c_str());
    for (int i = 0; i < l->R; ++i)
        if (l->h_n_vert[i] + M > v.nobs)
            return fail(h, NMPC_ERR_BAD_ARG, (fn + "route " + std::to_string(i) + " has " + std::to_string(l->h_n_vert[i]) +
                                              " vertices, n_vert + M > Nobs: its last M circle slots are not free").c_str());
    for (const double x : {radius, range})
        if (!(x > 0.0) || x > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, (fn + "radius and range must be finite and positive").c_str());
    if (!(spacing >= 0.0) || spacing > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, (fn + "spacing must be finite and not negative").c_str());
    WallGridHost gh;
    if (cell) {
        if (!(*cell > 0.0) || *cell > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, (fn + "cell must be finite and positive").c_str());
        if (!gh.build(n_edge, edge, *cell))
            return fail(h, NMPC_ERR_BAD_ARG, (fn + "the edges are filed in more than " + std::to_string(nmpc::WALL_GRID_MAX_ENTRIES) +
                                              " cells in all: use a larger cell or shorter edges").c_str());
    }
    LoopWalls st;
    DevBuf<double> pred;           // the loop's, unless the peers or the crowd have made it
    if (!l->d_pred) HIP_TRY(h, pred.alloc(B * v.N * 3));
    HIP_TRY(h, st.edge.upload(edge, 4 * (size_t)n_edge));
    HIP_TRY(h, st.wall_edge.alloc_fill(B * M, 0xFF));              // -1
    HIP_TRY(h, st.wall_stage.alloc_fill(B * M, 0xFF));
    nmpc::WallArgs &w = st.a;
    w.E = n_edge; w.M = M; w.radius = radius; w.range2 = range * range; w.spacing2 = spacing * spacing;
    w.edge = st.edge; w.pred = l->d_pred.p ? l->d_pred.p : pred.p; w.wall_edge = st.wall_edge; w.wall_stage = st.wall_stage;
    if (cell) HIP_TRY(h, st.grid.upload(gh, range, B));
    l->walls = std::move(st);
    if (pred) l->d_pred = std::move(pred);
    return NMPC_OK;
}

int nmpc_loop_set_walls(nmpc_loop *l, int n_edge, const double *edge, int M, double radius, double range, double spacing)
{
    return loop_set_walls(l, "nmpc_loop_set_walls", nmpc::WALLS_MAX_EDGES, n_edge, edge, M, radius, range, spacing, nullptr);
}

int nmpc_loop_set_walls_grid(nmpc_loop *l, int n_edge, const double *edge, int M, double radius, double range, double spacing, double cell)
{
    return loop_set_walls(l, "nmpc_loop_set_walls_grid", nmpc::WALL_GRID_MAX_EDGES, n_edge, edge, M, radius, range, spacing, &cell);
}

static const nmpc_map_clearance MAP_CLEARANCE_NONE = {__builtin_inf(), -1, -1, 0, -1, -1, 0};
static constexpr int MAP_MAX_EDGES = 1024;

// both map monitor setters: `grid` NULL = every edge against every robot (nmpc_loop_set_map_monitor), else {range, cell} of the walls
// grid the edges are found through
static int loop_set_map(nmpc_loop *l, const char *name, int max_edge, const nmpc_scene *map, const double *grid)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_setter(l, name, l->map.made(), "the loop has its map monitor already")) return rc;
    nmpc_handle *h = l->h;
    const int B = l->v.B;
    const std::string fn = std::string(name) + ": ";
    if (!map) return fail(h, NMPC_ERR_BAD_ARG, (fn + "map is NULL").c_str());
    if (!l->d_traj) return fail(h, NMPC_ERR_BAD_ARG, (fn + "the loop records no trajectory (max_steps == 0)").c_str());
    const int E = map->n_edge, np = map->n_poly;
    if (E < 3 || E > max_edge) return fail(h, NMPC_ERR_BAD_ARG, (fn + "n_edge outside 3 .. " + std::to_string(max_edge)).c_str());
    if (np < 1 || np > E / 3) return fail(h, NMPC_ERR_BAD_ARG, (fn + "n_poly outside 1 .. n_edge / 3").c_str());
    if (!map->edge || !map->poly_off) return fail(h, NMPC_ERR_BAD_ARG, (fn + "edge or poly_off is NULL").c_str());
    if (map->poly_off[0] != 0 || map->poly_off[np] != E) return fail(h, NMPC_ERR_BAD_ARG, (fn + "poly_off does not run from 0 to n_edge").c_str());
    for (int k = 0; k < np; ++k)
        if (map->poly_off[k + 1] > E || map->poly_off[k] < 0 || map->poly_off[k + 1] - map->poly_off[k] < 3)
            return fail(h, NMPC_ERR_BAD_ARG, (fn + "poly_off gives polygon " + std::to_string(k) + " fewer than three edges").c_str());
    for (int i = 0; i < 4 * E; ++i)
        if (!(map->edge[i] >= -DBL_MAX && map->edge[i] <= DBL_MAX))
            return fail(h, NMPC_ERR_BAD_ARG, (fn + "a coordinate of edge " + std::to_string(i / 4) + " is not finite").c_str());
    WallGridHost gh;
    if (grid) {
        for (int i = 0; i < 2; ++i)
            if (!(grid[i] > 0.0) || grid[i] > DBL_MAX) return fail(h, NMPC_ERR_BAD_ARG, (fn + "range and cell must be finite and positive").c_str());
        if (!gh.build(E, map->edge, grid[1]))
            return fail(h, NMPC_ERR_BAD_ARG, (fn + "the edges are filed in more than " + std::to_string(nmpc::WALL_GRID_MAX_ENTRIES) +
                                              " cells in all: use a larger cell or shorter edges").c_str());
    }
    std::vector<int> owner(E);
    for (int k = 0; k < np; ++k)
        for (int e = map->poly_off[k]; e < map->poly_off[k + 1]; ++e) owner[e] = k;
    LoopMap st;
    const std::vector<nmpc_map_clearance> none(B, MAP_CLEARANCE_NONE);
    HIP_TRY(h, st.rec.upload(none.data(), B));
    HIP_TRY(h, st.edge.upload(map->edge, 4 * (size_t)E));
    HIP_TRY(h, st.poly_off.upload(map->poly_off, (size_t)np + 1));
    HIP_TRY(h, st.edge_poly.upload(owner.data(), E));
    if (grid) HIP_TRY(h, st.grid.upload(gh, grid[0], B));
    nmpc::MapArgs &m = st.a;
    m.E = E; m.n_poly = np;
    m.edge = st.edge; m.poly_off = st.poly_off; m.edge_poly = st.edge_poly;
    m.rec = st.rec;
    l->map = std::move(st);
    return NMPC_OK;
}

int nmpc_loop_set_map_monitor(nmpc_loop *l, const nmpc_scene *map)
{
    return loop_set_map(l, "nmpc_loop_set_map_monitor", MAP_MAX_EDGES, map, nullptr);
}

int nmpc_loop_set_map_monitor_grid(nmpc_loop *l, const nmpc_scene *map, double range, double cell)
{
    const double grid[2] = {range, cell};
    return loop_set_map(l, "nmpc_loop_set_map_monitor_grid", nmpc::WALL_GRID_MAX_EDGES, map, grid);
}

// a retiring loop's active robots as the last step enqueued leaves them: waits for that step's count to arrive, not for the device
static int loop_nactive(nmpc_loop *l, int *n)
{
    LoopRetire &r = l->retire;
    if (r.nact_pending) {
        HIP_TRY(l->h, hipEventSynchronize(r.ev_nact));
        r.nact_pending = false;
    }
    *n = *(const int *)r.h_nact.p;
    return NMPC_OK;
}

// One step: assemble -> solve -> advance over the n robots still active, every stage's kernels where they belong.  Without retirement
// n = B and the host waits for nothing; with it the step waits for the count of the step before (an event), solves on gathered rows
// and rebuilds the active list behind the advance.
int nmpc_loop_step(nmpc_loop *l, void *stream)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    nmpc_handle *h = l->h;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    if (l->max_steps > 0 && l->steps >= l->max_steps) return fail(h, NMPC_ERR_BAD_ARG, "trajectory buffer is full");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(h, hipSetDevice(h->device));
    const nmpc::LoopView &v = l->v;
    LoopRetire &r = l->retire;
    const bool retiring = r.made();
    int n = v.B;
    if (retiring) {
        if (const int rc = loop_nactive(l, &n)) return rc;
        if (n < 0 || n > v.B) return fail(h, NMPC_ERR_HIP, "nmpc_loop_step: active count out of range");
    }
    const nmpc::LoopStep stp = nmpc::LoopStep::after(l->steps, v.s, n);
    const LoopCrowd &cr = l->crowd;
    const LoopPlant &pl = l->plant;
    // what the controller is told: with a plant that measures, the assembly and the prediction (and nobody else) see the measured poses
    nmpc::LoopView told = v;
    if (pl.made() && pl.measures()) told.state = pl.meas;
    // the crowd's table belongs to the world: it advances with nobody active too
    if (cr.made())
        hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_advance_kernel, dim3((cr.a.D * v.N * 5 + 255) / 256), dim3(256), 0, s, v, stp, cr.a);
    if (n > 0) {
        if (cr.grid()) {           // this step's table filed: zero, count, tile sums, scan, scatter
            const int entries = (cr.a.D * v.N + 255) / 256;
            hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_grid_zero_kernel, dim3((cr.g.cells + 256) / 256), dim3(256), 0, s, cr.g);
            hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_grid_count_kernel, dim3(entries), dim3(256), 0, s, v, stp, cr.a, cr.g);
            const int tiles = (cr.g.cells + nmpc::CROWD_GRID_TILE) / nmpc::CROWD_GRID_TILE;        // cells + 1 entries
            hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_grid_sum_kernel, dim3(tiles), dim3(256), 0, s, cr.g);
            hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_grid_scan_kernel, dim3(tiles), dim3(256), 0, s, cr.g);
            hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_grid_scatter_kernel, dim3(entries), dim3(256), 0, s, v, cr.a, cr.g);
        }
        if (pl.made() && pl.measures()) hipLaunchKernelGGL(nmpc::nmpc_loop_measure_kernel, dim3((n + 255) / 256), dim3(256), 0, s, v, stp, pl.a);
        hipLaunchKernelGGL(nmpc::nmpc_loop_assemble_kernel, dim3(n), dim3(64), 0, s, told, stp, l->a);
        if (l->d_pred) hipLaunchKernelGGL(nmpc::nmpc_loop_predict_kernel, dim3((n + 255) / 256), dim3(256), 0, s, told, stp, l->d_pred.p);
        if (cr.grid()) hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_grid_kernel, dim3(n), dim3(64), 0, s, v, stp, cr.a, cr.g);
        else if (cr.made()) hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_kernel, dim3(n), dim3(64), 0, s, v, stp, cr.a);
        if (l->peers.made()) {
            const nmpc::PeerArgs &p = l->peers.a;
            if (l->peers.grid()) {     // the boxes and the grid over all B: a retired robot stays filed
                const nmpc::PeerGridArgs &g = l->peers.g;
                hipLaunchKernelGGL(nmpc::nmpc_loop_peer_box_kernel, dim3((v.B + 255) / 256), dim3(256), 0, s, v, p, g);
                hipLaunchKernelGGL(nmpc::nmpc_loop_peer_grid_kernel, dim3(1), dim3(1024), 0, s, v, g);
                hipLaunchKernelGGL(nmpc::nmpc_loop_peers_grid_kernel, dim3(n), dim3(64), 0, s, v, p, g);
            } else {
                hipLaunchKernelGGL(nmpc::nmpc_loop_peers_kernel, dim3(n), dim3(64), 0, s, v, p);
            }
        }
        if (l->walls.grid.made())
            hipLaunchKernelGGL(nmpc::nmpc_loop_walls_grid_kernel, dim3(n), dim3(64), 0, s, v, l->walls.a, l->walls.grid.g);
        else if (l->walls.made())
            hipLaunchKernelGGL(nmpc::nmpc_loop_walls_kernel, dim3(n), dim3(64), nmpc::WallArgs::lds_bytes(l->walls.a.E), s, v, l->walls.a);
        if (retiring) hipLaunchKernelGGL(nmpc::nmpc_loop_gather_kernel, dim3(n), dim3(256), 0, s, v, r.a);
        HIP_TRY(h, hipGetLastError());
        // warm start: previous controls and multipliers, penalty back to its initial value (the server's behaviour).  The solve runs on
        // the loop's own rows, or on the gathered ones: rows 0 .. n - 1 are then the active robots
        double *P = v.P, *U = v.U, *Y = v.Y;
        nmpc_status *st = v.st;
        if (retiring) { P = r.a.sP; U = r.a.sU; Y = r.a.sY; st = r.a.sst; }
        // launch order: from the second step on, by the pass counts of these very robots' solves of the step before (read by the
        // classification kernel ahead of the solve, which then overwrites them); the first step has only the inputs to go by
        const nmpc_status *hint = (l->steps > 0 && h->loop_order_prev) ? st : nullptr;
        if (const int rc = solve_launch(h, n, P, U, Y, nullptr, Y, st, hint, stream)) return rc;
        if (retiring) hipLaunchKernelGGL(nmpc::nmpc_loop_scatter_kernel, dim3(n), dim3(256), 0, s, v, r.a);
        if (pl.made()) hipLaunchKernelGGL(nmpc::nmpc_loop_plant_kernel, dim3((n + 255) / 256), dim3(256), 0, s, v, stp, l->a, pl.a);
        else hipLaunchKernelGGL(nmpc::nmpc_loop_advance_kernel, dim3((n + 255) / 256), dim3(256), 0, s, v, stp, l->a);
        // the monitors and the dispatch run over the robots the advance ran over: the compaction comes after.  The monitor reads
        // retired_at as the step found it (NULL without retirement)
        if (l->monitor.made())
            hipLaunchKernelGGL(nmpc::nmpc_loop_monitor_kernel, dim3(n), dim3(64), 0, s, v, stp, l->monitor.a, r.retired_at);
        if (l->map.grid.made()) hipLaunchKernelGGL(nmpc::nmpc_loop_map_grid_kernel, dim3(n), dim3(64), 0, s, v, stp, l->map.a, l->map.grid.g);
        else if (l->map.made()) hipLaunchKernelGGL(nmpc::nmpc_loop_map_kernel, dim3(n), dim3(64), 0, s, v, stp, l->map.a);
        if (cr.watched()) hipLaunchKernelGGL(nmpc::nmpc_loop_crowd_monitor_kernel, dim3(n), dim3(64), 0, s, v, stp, cr.a);
        // the track monitor measures against the route the rows were driven on: the dispatch comes after
        if (l->track.made()) hipLaunchKernelGGL(nmpc::nmpc_loop_track_kernel, dim3(n), dim3(64), 0, s, v, stp, l->a, l->track.a);
        // the log sees the leg and the p the solve belonged to: the dispatch comes after (leg: the missions', NULL without them)
        if (l->log.made()) {
            hipLaunchKernelGGL(nmpc::nmpc_loop_log_kernel, dim3((n + 255) / 256), dim3(256), 0, s, v, stp, l->log.a, l->missions.leg.p);
            hipLaunchKernelGGL(nmpc::nmpc_loop_log_totals_kernel, dim3(1), dim3(1024), 0, s, v, stp, l->log.a);
        }
        if (l->missions.made()) hipLaunchKernelGGL(nmpc::nmpc_loop_dispatch_kernel, dim3(n), dim3(64), 0, s, v, stp, l->missions.a);
    } else if (l->log.made()) {    // nobody active: the step's totals are a row of zeros
        hipLaunchKernelGGL(nmpc::nmpc_loop_log_totals_kernel, dim3(1), dim3(1024), 0, s, v, stp, l->log.a);
    }
    // (with nobody active the step still counts: the clock advances and the trajectory rows repeat).  The compaction parks a retired
    // robot's predictions for the peers (NULL without them: the crowd reads the active robots' only)
    if (retiring) hipLaunchKernelGGL(nmpc::nmpc_loop_compact_kernel, dim3(1), dim3(1024), 0, s, v, stp, r.a, l->peers.made() ? l->d_pred.p : nullptr);
    // the ensemble sees the step as it ends: everybody's true pose, retired_at with this step's retirements (NULL without retirement)
    if (l->ensemble.made())
        hipLaunchKernelGGL(nmpc::nmpc_loop_ensemble_kernel, dim3(l->ensemble.a.G), dim3(256), 0, s, v, stp, l->ensemble.a, r.retired_at.p);
    HIP_TRY(h, hipGetLastError());
    if (retiring) {
        HIP_TRY(h, hipMemcpyAsync(r.h_nact.p, r.nact.p, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipEventRecord(r.ev_nact, s));
        r.nact_pending = true;
    }
    l->steps++;
    return NMPC_OK;
}

int nmpc_loop_run(nmpc_loop *l, int max_steps, void *stream)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    nmpc_handle *h = l->h;
    if (!h->alive) return NMPC_ERR_DEAD_HANDLE;
    if (!l->retire.made()) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_run: the loop does not retire its robots, it would never end");
    if (max_steps < 0) return fail(h, NMPC_ERR_BAD_ARG, "nmpc_loop_run: max_steps < 0");
    HIP_TRY(h, hipSetDevice(h->device));
    int taken = 0;
    while (taken < max_steps && !(l->max_steps > 0 && l->steps >= l->max_steps)) {
        int n = 0;
        if (const int rc = loop_nactive(l, &n)) return rc;
        if (n == 0) break;
        if (const int rc = nmpc_loop_step(l, stream)) return rc;
        ++taken;
    }
    return taken;
}

// what every reader does first: on the loop's device, after everything enqueued there has finished
static int loop_settle(nmpc_loop *l)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    HIP_TRY(l->h, hipSetDevice(l->h->device));
    HIP_TRY(l->h, hipDeviceSynchronize());
    return NMPC_OK;
}

int nmpc_loop_active(nmpc_loop *l, int32_t *n_active, int32_t *retired_at)
{
    if (const int rc = loop_settle(l)) return rc;
    const int B = l->v.B;
    if (!l->retire.made()) {
        if (n_active) *n_active = B;
        if (retired_at) for (int b = 0; b < B; ++b) retired_at[b] = -1;
        return NMPC_OK;
    }
    HIP_TRY(l->h, l->retire.nact.read(n_active, 1));
    HIP_TRY(l->h, l->retire.retired_at.read(retired_at, B));
    return NMPC_OK;
}

int nmpc_loop_legs(nmpc_loop *l, int32_t *leg, int32_t *route_of, int32_t *leg_at)
{
    if (const int rc = loop_settle(l)) return rc;
    const size_t B = (size_t)l->v.B;
    HIP_TRY(l->h, l->d_route_of.read(route_of, B));
    if (!l->missions.made()) {
        if (leg) for (size_t b = 0; b < B; ++b) leg[b] = 0;
        return NMPC_OK;
    }
    HIP_TRY(l->h, l->missions.leg.read(leg, B));
    HIP_TRY(l->h, l->missions.leg_at.read(leg_at, l->missions.n_legs));
    return NMPC_OK;
}

int nmpc_loop_clearance(nmpc_loop *l, nmpc_clearance *out)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    const int B = l->v.B;
    if (!l->monitor.made()) {
        for (int b = 0; b < B; ++b) out[b] = CLEARANCE_NONE;
        return NMPC_OK;
    }
    HIP_TRY(l->h, l->monitor.rec.read(out, B));
    return NMPC_OK;
}

int nmpc_loop_peer_grid(nmpc_loop *l, nmpc_peer_grid *out, int32_t *cell_of)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    if (!l->peers.grid()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_peer_grid: the loop has no peers grid (nmpc_loop_set_peers_grid)");
    if (l->steps == 0) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_peer_grid: before the loop's first step");
    HIP_TRY(l->h, l->peers.hdr.read(out, 1));
    HIP_TRY(l->h, l->peers.cell_of.read(cell_of, l->v.B));
    return NMPC_OK;
}

int nmpc_loop_crowd(nmpc_loop *l, double *table, int32_t *seen)
{
    if (const int rc = loop_settle(l)) return rc;
    const LoopCrowd &c = l->crowd;
    if (!c.made()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_crowd: the loop has no crowd (nmpc_loop_set_crowd, nmpc_loop_set_crowd_grid)");
    if (l->steps == 0) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_crowd: before the loop's first step");
    // step k (k = 0, 1, ...) wrote buffer (k & 1) ^ 1
    HIP_TRY(l->h, c.tab[((l->steps - 1) & 1) ^ 1].read(table, (size_t)c.a.D * l->v.N * 5));
    HIP_TRY(l->h, c.seen.read(seen, (size_t)l->v.B * c.a.M));
    return NMPC_OK;
}

int nmpc_loop_crowd_grid(nmpc_loop *l, nmpc_crowd_grid *out, int32_t *cell_of, int32_t *looked)
{
    if (const int rc = loop_settle(l)) return rc;
    const LoopCrowd &c = l->crowd;
    if (!c.grid()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_crowd_grid: the loop has no crowd grid (nmpc_loop_set_crowd_grid)");
    if ((cell_of || looked) && l->steps == 0) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_crowd_grid: cell_of and looked before the loop's first step");
    if (out) {
        *out = c.hdr;          // filed: the entry behind the last cell, as the last build's scan left it (0 before any build)
        HIP_TRY(l->h, hipMemcpy(&out->filed, c.cell_off.p + c.g.cells, sizeof(int), hipMemcpyDeviceToHost));
    }
    HIP_TRY(l->h, c.cell_of.read(cell_of, (size_t)c.a.D * l->v.N));
    HIP_TRY(l->h, c.looked.read(looked, (size_t)l->v.B));
    return NMPC_OK;
}

int nmpc_loop_walls(nmpc_loop *l, int32_t *wall_edge, int32_t *wall_stage)
{
    if (const int rc = loop_settle(l)) return rc;
    const LoopWalls &w = l->walls;
    if (!w.made()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_walls: the loop has no walls (nmpc_loop_set_walls, nmpc_loop_set_walls_grid)");
    if (l->steps == 0) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_walls: before the loop's first step");
    HIP_TRY(l->h, w.wall_edge.read(wall_edge, (size_t)l->v.B * w.a.M));
    HIP_TRY(l->h, w.wall_stage.read(wall_stage, (size_t)l->v.B * w.a.M));
    return NMPC_OK;
}

int nmpc_loop_wall_grid(nmpc_loop *l, nmpc_wall_grid *out, int32_t *cell_off, int32_t *cell_edge, int32_t *looked)
{
    if (const int rc = loop_settle(l)) return rc;
    const LoopWalls &w = l->walls;
    if (!w.grid.made()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_wall_grid: the loop has no walls grid (nmpc_loop_set_walls_grid)");
    if (looked && l->steps == 0) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_wall_grid: looked before the loop's first step");
    HIP_TRY(l->h, w.grid.read(out, cell_off, cell_edge, looked, (size_t)l->v.B));
    return NMPC_OK;
}

int nmpc_loop_map_grid(nmpc_loop *l, nmpc_wall_grid *out, int32_t *cell_off, int32_t *cell_edge, int32_t *looked)
{
    if (const int rc = loop_settle(l)) return rc;
    const LoopMap &m = l->map;
    if (!m.grid.made()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_map_grid: the loop has no map monitor grid (nmpc_loop_set_map_monitor_grid)");
    if (looked && l->steps == 0) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_map_grid: looked before the loop's first step");
    HIP_TRY(l->h, m.grid.read(out, cell_off, cell_edge, looked, (size_t)l->v.B));
    return NMPC_OK;
}

int nmpc_loop_crowd_clearance(nmpc_loop *l, nmpc_crowd_clearance *out)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    const int B = l->v.B;
    if (!l->crowd.watched()) {
        for (int b = 0; b < B; ++b) out[b] = CROWD_CLEARANCE_NONE;
        return NMPC_OK;
    }
    HIP_TRY(l->h, l->crowd.rec.read(out, B));
    return NMPC_OK;
}

int nmpc_loop_map_clearance(nmpc_loop *l, nmpc_map_clearance *out)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    const int B = l->v.B;
    if (!l->map.made()) {
        for (int b = 0; b < B; ++b) out[b] = MAP_CLEARANCE_NONE;
        return NMPC_OK;
    }
    HIP_TRY(l->h, l->map.rec.read(out, B));
    return NMPC_OK;
}

int nmpc_loop_tracking(nmpc_loop *l, nmpc_tracking *out)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    if (!l->track.made()) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_tracking: the loop has no track monitor (nmpc_loop_set_track_monitor)");
    HIP_TRY(l->h, l->track.rec.read(out, l->v.B));
    return NMPC_OK;
}

int nmpc_loop_log(nmpc_loop *l, double *ctrl, nmpc_step_record *rec, int max_steps)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (!l->log.made()) return 0;
    if (max_steps < l->steps) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_log: max_steps is smaller than the steps taken, the log does not fit");
    if (const int rc = loop_settle(l)) return rc;
    const size_t B = (size_t)l->v.B, steps = (size_t)l->steps;
    HIP_TRY(l->h, l->log.ctrl.read(ctrl, steps * l->v.s * B * 2));
    HIP_TRY(l->h, l->log.rec.read(rec, steps * B));
    return l->steps;
}

int nmpc_loop_drive_summary(nmpc_loop *l, nmpc_drive_summary *out)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    const int B = l->v.B;
    if (!l->log.made()) {
        for (int b = 0; b < B; ++b) out[b] = DRIVE_SUMMARY_NONE;
        return NMPC_OK;
    }
    HIP_TRY(l->h, l->log.sum.read(out, B));
    return NMPC_OK;
}

int nmpc_loop_step_totals(nmpc_loop *l, nmpc_step_totals *out, int max_steps)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (!l->log.made()) return 0;
    if (max_steps < l->steps) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_step_totals: max_steps is smaller than the steps taken, the totals do not fit");
    if (const int rc = loop_settle(l)) return rc;
    HIP_TRY(l->h, l->log.tot.read(out, (size_t)l->steps));
    return l->steps;
}

int nmpc_loop_ensemble(nmpc_loop *l, nmpc_ensemble_stat *out, int max_steps)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (!l->ensemble.made()) return 0;
    if (max_steps < l->steps) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_ensemble: max_steps is smaller than the steps taken, the records do not fit");
    if (const int rc = loop_settle(l)) return rc;
    HIP_TRY(l->h, l->ensemble.ens.read(out, (size_t)l->steps * l->ensemble.a.G));
    return l->steps;
}

int nmpc_loop_ensemble_groups(nmpc_loop *l)
{
    return l && l->ensemble.made() ? l->ensemble.a.G : 0;
}

int nmpc_loop_plant_applied(nmpc_loop *l, double *out, int rows)
{
    if (!l) return NMPC_ERR_BAD_ARG;
    if (!l->plant.applied) return 0;
    const int taken = l->steps * l->v.s;
    if (rows < taken) return fail(l->h, NMPC_ERR_BAD_ARG, "nmpc_loop_plant_applied: rows is smaller than the controls applied, they do not fit");
    if (const int rc = loop_settle(l)) return rc;
    HIP_TRY(l->h, l->plant.applied.read(out, (size_t)taken * l->v.B * 2));
    return taken;
}

int nmpc_loop_plant_measured(nmpc_loop *l, double *out)
{
    if (!out) return NMPC_ERR_BAD_ARG;
    if (const int rc = loop_settle(l)) return rc;
    nmpc_handle *h = l->h;
    const nmpc::LoopView &v = l->v;
    const size_t B = (size_t)v.B;
    // what the solves were given is p[0 .. 3): the measured poses where the plant measures, else the poses themselves
    if (l->plant.made() && l->plant.measures()) HIP_TRY(h, l->plant.meas.read(out, B * 3));
    else if (l->steps == 0) HIP_TRY(h, l->d_state.read(out, B * 3));
    else HIP_TRY(h, hipMemcpy2D(out, 3 * sizeof(double), v.P, (size_t)v.n_p * sizeof(double), 3 * sizeof(double), B, hipMemcpyDeviceToHost));
    return NMPC_OK;
}

int nmpc_loop_read(nmpc_loop *l, double *state, double *last_u, int32_t *idx, uint8_t *done, nmpc_status *status)
{
    if (const int rc = loop_settle(l)) return rc;
    nmpc_handle *h = l->h;
    const size_t B = (size_t)l->v.B;
    HIP_TRY(h, l->d_state.read(state, B * 3));
    HIP_TRY(h, l->d_last_u.read(last_u, B * 2));
    HIP_TRY(h, l->d_idx.read(idx, B));
    HIP_TRY(h, l->d_done.read(done, B));
    HIP_TRY(h, l->d_st.read(status, B));
    return NMPC_OK;
}

int nmpc_loop_params(nmpc_loop *l, double *p, double *u, double *y)
{
    if (const int rc = loop_settle(l)) return rc;
    nmpc_handle *h = l->h;
    const size_t B = (size_t)l->v.B;
    HIP_TRY(h, l->d_P.read(p, B * l->v.n_p));
    HIP_TRY(h, l->d_U.read(u, B * l->v.n_u));
    HIP_TRY(h, l->d_Y.read(y, B * l->v.n1));
    return NMPC_OK;
}

int nmpc_loop_trajectory(nmpc_loop *l, double *rows, int max_rows)
{
    if (!l || !rows) return NMPC_ERR_BAD_ARG;
    nmpc_handle *h = l->h;
    if (!l->d_traj) return fail(h, NMPC_ERR_BAD_ARG, "the loop was created without a trajectory buffer");
    const int nrows = l->steps * l->v.s + 1;
    if (max_rows < nrows) return fail(h, NMPC_ERR_BAD_ARG, "trajectory does not fit");
    if (const int rc = loop_settle(l)) return rc;
    HIP_TRY(h, l->d_traj.read(rows, (size_t)nrows * l->v.B * 3));
    return nrows;
}
