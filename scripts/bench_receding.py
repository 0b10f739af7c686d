#!/usr/bin/env python3
"""BASELINE config 4: smooth_velocity weights, per-robot randomised dynamic ellipses, B robots advanced
for K receding-horizon steps (num_steps_taken = 2), warm starts carried, p rebuilt every step.
Default: the whole loop on device (nmpc_loop_*: assembly, solve and state advance are kernels, nothing
crosses PCIe between steps), every robot on the scene's route; --routes R > 1: the robots follow R routes
planned between random start / goal points of the scene (frontend.random_fleet).  --peers G: the robots see each
other in groups of G consecutive robots; --peer-slots of the Ndynobs ellipse slots go to peers, the
rest stay scripted; with --peer-cell H the peers are found through a grid of H metres built on the device every step
(nmpc_loop_set_peers_grid: the same peers), and the result line gains peer_grid: the last step's cells, filed robots and largest cell.  --retire: robots that reach their goal leave the loop (nmpc_loop_set_retire); the run ends when nobody is
active or after --steps steps, and reports the steps and solves it took.  --back: how close to the route's end robots may start
(--routes 1); a small value gives a fleet whose robots arrive all through the run.  --monitor [G]: the clearance monitor (nmpc_loop_set_monitor,
DESIGN.md section 5.9) in groups of G consecutive robots, default the --peers groups or 32; the result line then has, from its records, the shares
of robots that were inside a circle, inside a padded ellipse and closer to a groupmate than two peer radii, and the fleet's smallest value of each.
--own-routes: every robot its own start and goal (workloads.own_route_fleet, seed 0), with --retire --legs L its own mission of L legs, each leg
from the goal of the one before; the routes are planned on the device (frontend.DevicePlanner), and the result line
gains plan_ms (the planner kernels' time over all batches, redraws included) and routes_planned.  --map [inflated]: the map monitor
(nmpc_loop_set_map_monitor) on the scene's original polygons, the true walls, or with "inflated" on the polygons the
planner plans on; the result line then has map_clearance: the share of robots with a hit, the rows hit and the fleet's smallest wall distance,
and (without --retire) the stage's time per step, from whole runs of the same fleet with and without it.  --map-pieces P cuts every edge into P
pieces (workloads.subdivided_map); --map-cell H [--map-range R] finds the edges through the walls grid (nmpc_loop_set_map_monitor_grid), which
lifts the limit of 1024 edges; map_clearance then has the grid and the edges looked at.
--track [TOL]: the track monitor (nmpc_loop_set_track_monitor): the result line then has tracking: the fleet's largest
and RMS cross-track error in metres, its largest and RMS heading error and the share of rows and of robots further than TOL (0.5 m) from the route.
--log: the drive log (nmpc_loop_set_log): the result line then has drive_log: the share of non-converged solves per exit
status, the worst step's slowest solve and the fleet's largest acceleration.  --crowd D: a crowd of D moving obstacles shared by the whole fleet
(nmpc_loop_set_crowd; workloads.crowd_ellipses, seed 2): --crowd-slots of the Ndynobs ellipse slots go to the closest
ones within --crowd-range metres, the result line gains crowd: the share of those slots filled at the last step (--crowd-cell H: the obstacles a
robot measures are found through a grid in space and stage of H-metre cells, nmpc_loop_set_crowd_grid, which lifts the limit of 16384 obstacles to
131072; crowd then also has the grid's cells, the entries filed, and the mean and the largest number of the table's entries a robot looked at at
the last step beside the D * N the all-obstacles selection looks at); with --crowd-watch also the
observer (nmpc_loop_set_crowd_monitor): the robots whose level against some obstacle fell below 1, and how many of those closest approaches
were to an obstacle the robot did not have in a slot at that step (found by an untimed second run that reads the slots after every step).
--plant-act G, --plant-proc P, --plant-meas M, --plant-seed S: a disturbed plant (nmpc_loop_set_plant): actuation noise of
relative sigma G on both controls, process noise of sigma P metres (and radians) per applied control, measurement noise of sigma M metres (and
radians), seed S; a robot's id is its index in the whole fleet, so --split does not change its disturbances.  --ensemble (--routes 1): B copies of
the fleet's robot 0, its start, reference sample and ellipses (workloads.ensemble_fleet), the Monte-Carlo study of one controller; the result line gains
plant: the sigmas, and with --ensemble the spread of the final poses.  --ensemble-stats [M]: the ensemble stage (nmpc_loop_set_ensemble, DESIGN.md
section 5.9): without M the whole fleet is one group (with --ensemble: the study's result, on the device); with M every robot of the fleet --routes
gives is repeated M times (workloads.grouped_ensemble: --batch x M robots, the copies of a robot one group, interleaved) and, under the plant, each
group is the Monte-Carlo study of one robot.  The result line gains ensemble: from the device's records of the last step, per group (the first 8)
the members, the mean pose, the standard deviations of x, y and the heading and the arrived count -- the records of the --split sub-fleets pooled
on the host -- and with --ensemble the largest relative difference of those standard deviations from the host-side spread beside them.
--walls M: the walls stage (nmpc_loop_set_walls): every step each robot's closest points on the scene's true walls
(frontend.map_edges, with --walls-pieces P every edge cut into P pieces by workloads.subdivided_map) within --walls-range metres of its predicted
path, no closer to each other than --walls-spacing, become circles of --walls-radius (default vehicle_width / 2 + vehicle_margin) in the last M
static-circle slots of its p (--walls-cell H: the edges a robot measures are found through a grid of H-metre cells, nmpc_loop_set_walls_grid, which
lifts the limit of 1024 edges; the result line then has the edges looked at and, from whole runs of the same fleet timed in this run, the time per step
under the grid's setter, under the all-edges one up to 1024 edges, and their difference: the two solve the same problems, so it is the stages'); the result line gains walls: the edges and the share of those slots filled at the last step, and with --map the
map_clearance beside it is the closest approach with the walls seen.  --host: parameter assembly on the host (NumPy-vectorised) around BatchSolver.solve.  Prints one JSON line."""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from mpc_trajectory_generator_amd import named_config                            # noqa: E402
from mpc_trajectory_generator_amd import harness                                 # noqa: E402
from mpc_trajectory_generator_amd.solver import BatchSolver                      # noqa: E402
from mpc_trajectory_generator_amd.trajectory import DriveLog, Ensemble, FleetRecedingHorizon, MapMonitor, Monitor, Peers, TrackMonitor, VectorizedRecedingHorizon   # noqa: E402
from mpc_trajectory_generator_amd.workloads import moving_ellipses, route_fleet   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--scene", type=int, default=11)
ap.add_argument("--host", action="store_true")
ap.add_argument("--routes", type=int, default=1,
                help="routes the fleet follows: 1 = every robot on the scene's own route; R > 1 = frontend.random_fleet(cfg, "
                     "scene, R, batch, seed=0), robots dealt evenly to R randomly planned routes")
ap.add_argument("--split", type=int, default=2,
                help="device loop only: split the fleet into this many sub-fleets, each with its own handle and HIP "
                     "stream, stepped alternately -- one sub-fleet's slow instances overlap the others' bulk")
ap.add_argument("--budget", type=int, default=0,
                help="max_total_inner per solve: the deterministic counterpart of the reference's 0.5 s max_duration "
                     "(src/mpc/mpc_generator.py:9,186); 0 = off")
ap.add_argument("--peers", type=int, default=0,
                help="G > 0: groups of G consecutive robots (of a sub-fleet, see --split) see each other; 0 = nobody sees anybody")
ap.add_argument("--peer-slots", type=int, default=2, help="with --peers: ellipse slots given to peers (the other Ndynobs - M stay scripted)")
ap.add_argument("--peer-range", type=float, default=10.0, help="with --peers: how far a robot sees, in metres")
ap.add_argument("--peer-cell", type=float, default=None, metavar="H",
                help="with --peers: find the peers through a grid with cells of H metres (device loop: nmpc_loop_set_peers_grid)")
ap.add_argument("--retire", action="store_true",
                help="device loop only: retire the robots that reach their goal; run until nobody is active, --steps at the most")
ap.add_argument("--legs", type=int, default=1, metavar="L",
                help="with --retire: every robot drives a mission of L legs (nmpc_loop_set_missions), its route and the same route "
                     "driven backwards in turn, and retires after the last; the result line gains legs_done")
ap.add_argument("--own-routes", action="store_true",
                help="device loop only: every robot its own start and goal (and, with --legs L, its own L legs), planned on the device; "
                     "takes the place of --routes")
ap.add_argument("--monitor", type=int, nargs="?", const=0, default=None, metavar="G",
                help="device loop only: keep every robot's closest approach to circles, scripted ellipses and the robots of its group of G "
                     "consecutive robots (of a sub-fleet) on the device, and report them; G defaults to the --peers groups, or 32")
ap.add_argument("--map", nargs="?", const="original", default=None, choices=("original", "inflated"), metavar="inflated",
                help="device loop only: keep every robot's closest approach to the scene's walls and its rows inside an obstacle, outside the "
                     "boundary or through an edge on the device, and report them; 'inflated': against the polygons the planner plans on")
ap.add_argument("--map-cell", type=float, default=None, metavar="H",
                help="with --map: find the edges a row is judged against through the walls grid of H-metre cells (nmpc_loop_set_map_monitor_grid), "
                     "which lifts the limit of 1024 edges; the result line gains the edges looked at and the stage's time per step")
ap.add_argument("--map-range", type=float, default=2.0, metavar="R", help="with --map-cell: walls further than R metres are not recorded")
ap.add_argument("--map-pieces", type=int, default=1, metavar="P",
                help="with --map: every edge of the map cut into P pieces (1024 edges at the most without --map-cell, 1048576 with it)")
ap.add_argument("--track", type=float, nargs="?", const=0.5, default=None, metavar="TOL",
                help="device loop only: the track monitor, rows further than TOL metres (default 0.5) from the route count as off it")
ap.add_argument("--log", action="store_true",
                help="device loop only: keep every robot's applied controls, a record of every solve, a summary per robot and the fleet's "
                     "totals per step on the device, and report from them")
ap.add_argument("--crowd", type=int, default=0, metavar="D",
                help="device loop only: D > 0 moving obstacles of the scene, shared by the whole fleet (every sub-fleet sees the same crowd)")
ap.add_argument("--crowd-slots", type=int, default=2, help="with --crowd: ellipse slots given to the crowd (the others stay scripted, or go to peers)")
ap.add_argument("--crowd-range", type=float, default=10.0, help="with --crowd: how far a robot sees an obstacle of the crowd, in metres")
ap.add_argument("--crowd-cell", type=float, default=None, metavar="H",
                help="with --crowd: the obstacles a robot measures are found through a grid in space and stage of H-metre cells "
                     "(nmpc_loop_set_crowd_grid: the same obstacles, D up to 131072 instead of 16384)")
ap.add_argument("--crowd-watch", action="store_true", help="with --crowd: keep every robot's closest approach to any obstacle of the crowd on the device")
ap.add_argument("--plant-act", type=float, default=0.0, metavar="G", help="device loop only: actuation noise, sigma = G * |control| on v and omega")
ap.add_argument("--plant-proc", type=float, default=0.0, metavar="P", help="device loop only: process noise on x, y (metres) and theta (radians) per applied control")
ap.add_argument("--plant-meas", type=float, default=0.0, metavar="M", help="device loop only: measurement noise on x, y (metres) and theta (radians)")
ap.add_argument("--plant-seed", type=int, default=0, metavar="S", help="the seed of the plant's disturbances")
ap.add_argument("--ensemble", action="store_true", help="--routes 1: B copies of the fleet's robot 0 (a Monte-Carlo study under the plant)")
ap.add_argument("--ensemble-stats", type=int, nargs="?", const=0, default=None, metavar="M",
                help="device loop only: per-group pose statistics after every step, kept on the device; without M one group of everybody, with M "
                     "every robot of the fleet M times (--batch x M robots), the copies of a robot one group")
ap.add_argument("--walls", type=int, default=0, metavar="M",
                help="device loop only: M > 0 of the static-circle slots go to the closest points on the scene's walls (every route must leave them free)")
ap.add_argument("--walls-range", type=float, default=2.0, metavar="R", help="with --walls: how far from its predicted path a robot sees a wall, in metres")
ap.add_argument("--walls-spacing", type=float, default=0.0, metavar="S", help="with --walls: no two wall circles of a robot closer than this, in metres")
ap.add_argument("--walls-radius", type=float, default=None, metavar="RC", help="with --walls: the circles' radius (default vehicle_width / 2 + vehicle_margin)")
ap.add_argument("--walls-pieces", type=int, default=1, metavar="P",
                help="with --walls: every edge of the map cut into P pieces (26 P edges; 1024 at the most without --walls-cell, 1048576 with it)")
ap.add_argument("--walls-cell", type=float, default=None, metavar="H",
                help="with --walls: find the edges a robot measures through a static grid of H-metre cells (nmpc_loop_set_walls_grid): the same "
                     "circles; the result line gains the edges looked at and, up to 1024 edges, the time per step under either setter and their difference")
ap.add_argument("--back", type=int, default=60, help="--routes 1: no robot starts within this many samples of the route's end")
ap.add_argument("--experiments", action="store_true", help="the experiments build of the library (reads the NMPC_* knobs: A/B runs only)")
args = ap.parse_args()
if args.monitor is not None:
    if args.host or args.steps < 1:
        ap.error("--monitor reads the trajectory the device loop records: it needs the device loop (no --host) and --steps >= 1")
    if args.monitor < 0:
        ap.error("--monitor G: G >= 1")
    args.monitor = args.monitor or args.peers or 32
if args.peer_cell is not None and not args.peers:
    ap.error("--peer-cell goes with --peers G")
if args.map and (args.host or args.steps < 1):
    ap.error("--map reads the trajectory the device loop records: it needs the device loop (no --host) and --steps >= 1")
if args.map_pieces < 1 or ((args.map_cell is not None or args.map_pieces > 1) and not args.map):
    ap.error("--map-cell H, --map-pieces P: go with --map, P >= 1")
if args.map_cell is not None and not (0 < args.map_cell < float("inf") and 0 < args.map_range < float("inf")):
    ap.error("--map-cell H, --map-range R: finite and positive")
if args.track is not None and (args.host or args.steps < 1 or not 0 <= args.track < float("inf")):
    ap.error("--track [TOL]: TOL >= 0 and finite, on the device loop (no --host) with --steps >= 1")
if args.log and (args.host or args.steps < 1):
    ap.error("--log is the device loop's, and its length is --steps: it needs the device loop (no --host) and --steps >= 1")
if args.legs < 1 or (args.legs > 1 and (not args.retire or args.host)):
    ap.error("--legs L: L >= 1, and L > 1 needs --retire on the device loop")
if args.own_routes and (args.host or args.routes != 1):
    ap.error("--own-routes: on the device loop, and in place of --routes")
if args.crowd and (args.host or args.steps < 1):
    ap.error("--crowd is the device loop's: it needs the device loop (no --host) and --steps >= 1")
if (args.crowd_watch or args.crowd < 0) and args.crowd < 1:
    ap.error("--crowd D: D >= 1, and --crowd-watch goes with it")
if args.crowd_cell is not None and not (args.crowd and 0 < args.crowd_cell < float("inf")):
    ap.error("--crowd-cell H: goes with --crowd, H finite and positive")
if args.walls < 0 or (args.walls and (args.host or args.steps < 1)) or args.walls_pieces < 1:
    ap.error("--walls M: M >= 1, on the device loop (no --host) with --steps >= 1; --walls-pieces P: P >= 1")
if args.walls_cell is not None and not (args.walls and 0 < args.walls_cell < float("inf")):
    ap.error("--walls-cell H: goes with --walls, H finite and positive")
planted = args.plant_act > 0 or args.plant_proc > 0 or args.plant_meas > 0
if min(args.plant_act, args.plant_proc, args.plant_meas) < 0 or (planted and args.host):
    ap.error("--plant-act, --plant-proc, --plant-meas: >= 0, on the device loop (no --host)")
if args.ensemble and (args.routes != 1 or args.own_routes or args.host):
    ap.error("--ensemble: copies of one robot on the scene's route, on the device loop")
if args.ensemble_stats is not None:
    if args.host or args.steps < 1 or args.ensemble_stats < 0:
        ap.error("--ensemble-stats [M]: M >= 1, on the device loop (no --host) with --steps >= 1")
    if args.ensemble_stats and (args.ensemble or args.own_routes or args.legs > 1 or args.peers):
        ap.error("--ensemble-stats M repeats the fleet --routes gives: not with --ensemble, --own-routes, --legs or --peers")
sopts = {"max_total_inner": args.budget} if args.budget > 0 else {}
if args.experiments:
    sopts["experiments"] = True
cfg = named_config("cfg4")
K = cfg.Ndynobs - (args.peer_slots if args.peers else 0) - (args.crowd_slots if args.crowd else 0)
if K < 0:
    ap.error(f"--peer-slots and --crowd-slots together take more than the {cfg.Ndynobs} ellipse slots")
B = args.batch
# a peer's ellipse: its half width, this robot's half width and the margin
peer_radius = cfg.vehicle_width + cfg.vehicle_margin


def peers_of(n):
    """groups of --peers consecutive robots among n"""
    return Peers(slots=args.peer_slots, rx=peer_radius, ry=peer_radius, range=args.peer_range,
                 group_of=(np.arange(n) // args.peers).astype(np.int32), cell=args.peer_cell) if args.peers else None


def monitor_of(n):
    """groups of --monitor consecutive robots among n"""
    return Monitor(group_of=(np.arange(n) // args.monitor).astype(np.int32)) if args.monitor else None


map_monitor = None
if args.map:
    from mpc_trajectory_generator_amd.frontend import map_edges, scene_planner
    from mpc_trajectory_generator_amd.workloads import subdivided_map
    map_monitor = MapMonitor(*subdivided_map(*map_edges(scene_planner(cfg, args.scene), inflated=args.map == "inflated"), args.map_pieces),
                             cell=args.map_cell, range=None if args.map_cell is None else args.map_range)

crowd = None
if args.crowd:
    from mpc_trajectory_generator_amd.trajectory import Crowd
    from mpc_trajectory_generator_amd.workloads import crowd_ellipses
    crowd = Crowd(crowd_ellipses(cfg, args.scene, args.crowd, 2), args.crowd_slots, args.crowd_range, watch=args.crowd_watch, cell=args.crowd_cell)

walls = None
if args.walls:
    from mpc_trajectory_generator_amd.frontend import map_edges, scene_planner
    from mpc_trajectory_generator_amd.trajectory import Walls
    from mpc_trajectory_generator_amd.workloads import subdivided_map
    walls = Walls(subdivided_map(*map_edges(scene_planner(cfg, args.scene)), args.walls_pieces)[0], args.walls,
                  cfg.vehicle_width / 2 + cfg.vehicle_margin if args.walls_radius is None else args.walls_radius, args.walls_range, args.walls_spacing,
                  cell=args.walls_cell)

planning = {}
legs_of = None
if args.own_routes:
    from mpc_trajectory_generator_amd.frontend import DevicePlanner, scene_planner
    from mpc_trajectory_generator_amd.workloads import fleet_ellipses, own_route_fleet
    dp = DevicePlanner(scene_planner(cfg, args.scene), max_batch=B)
    planning = {"plan_ms": 0.0, "routes_planned": 0}

    def plan(s, g):
        res = dp.plan(s, g)
        planning["plan_ms"] += dp.last_ms
        return res
    routes, route_of, starts, i0, legs_of = own_route_fleet(cfg, args.scene, B, 0, legs=args.legs, plan=plan)
    dp.close()
    planning["routes_planned"] = len(routes)
    dyn = fleet_ellipses(routes, route_of, i0, K, seed=1)      # ellipses crossing each robot's first route
elif args.routes == 1:
    route = harness.scene_route(cfg, args.scene)
    i0, starts, dyn = route_fleet(route, B, 0, K, back=args.back)
    if args.ensemble:      # everybody a copy of the fleet's robot 0: its start, its reference sample, its ellipses
        from mpc_trajectory_generator_amd.workloads import ensemble_fleet
        _, _, starts, i0 = ensemble_fleet(route, starts[0], B, i0[0])
        dyn = dyn and tuple(np.repeat(a[:1], B, axis=0) for a in dyn)
    routes, route_of = route, None
else:
    from mpc_trajectory_generator_amd.frontend import random_fleet
    routes, route_of, starts, i0 = random_fleet(cfg, args.scene, args.routes, B, seed=0)
    rng = np.random.Generator(np.random.PCG64(1))
    # ellipses crossing each robot's own route, 0..29 samples ahead of its start
    n = np.array([len(r.x_ref) for r in routes])[route_of]
    first = np.concatenate([[0], np.cumsum([len(r.x_ref) for r in routes])[:-1]])[route_of]
    xs, ys = np.concatenate([r.x_ref for r in routes]), np.concatenate([r.y_ref for r in routes])
    jj = first[:, None] + np.minimum(n[:, None] - 1, i0[:, None] + rng.integers(0, 30, (B, K)))
    dyn = moving_ellipses(np.stack([xs[jj], ys[jj]], axis=2), rng)
ens_group_of, ens_G = None, 0           # with --ensemble-stats: the group of every robot of the whole fleet, and their number
if args.ensemble_stats is not None:
    ens_group_of, ens_G = np.zeros(B, dtype=np.int32), 1
    if args.ensemble_stats:
        from mpc_trajectory_generator_amd.workloads import grouped_ensemble
        routes, route_of, starts, i0, ens_group_of = grouped_ensemble([routes] if route_of is None else routes,
                                                                     np.zeros(B, dtype=np.int32) if route_of is None else route_of,
                                                                     starts, i0, args.ensemble_stats)
        dyn = dyn and tuple(a[ens_group_of] for a in dyn)
        B, ens_G = len(starts), B
fleet = f", {args.routes} routes (frontend.random_fleet, seed 0)" if args.routes > 1 else ""
if args.own_routes:
    fleet = f", every robot its own start and goal (workloads.own_route_fleet, seed 0; {len(routes)} routes planned on the device)"
if args.ensemble:
    fleet += ", an ensemble: every robot a copy of the fleet's robot 0"
if args.ensemble_stats:
    fleet += f", every robot {args.ensemble_stats} times (workloads.grouped_ensemble: {ens_G} groups)"
if planted:
    fleet += (f", disturbed plant (actuation {args.plant_act}, process {args.plant_proc}, measurement {args.plant_meas}, seed {args.plant_seed})")
if args.peers:
    fleet += (f", {K} scripted ellipses and {args.peer_slots} peer slots per robot, groups of {args.peers} consecutive robots, "
              f"range {args.peer_range} m, radii {peer_radius} m"
              + (f", found through a grid of {args.peer_cell} m" if args.peer_cell is not None else ""))
if args.crowd:
    fleet += (f", a crowd of {args.crowd} moving obstacles (workloads.crowd_ellipses, seed 2), {args.crowd_slots} crowd slots per robot, "
              f"range {args.crowd_range} m" + (f", found through a grid of {args.crowd_cell} m" if args.crowd_cell is not None else "") +
              (", crowd observer" if args.crowd_watch else "") + ("" if args.peers else f", {K} scripted ellipses"))
if walls is not None:
    fleet += (f", {args.walls} wall slots per robot over {len(walls.edges)} edges, range {args.walls_range} m, spacing {args.walls_spacing} m, "
              f"radius {walls.radius} m" + (f", found through a grid of {args.walls_cell} m" if args.walls_cell is not None else ""))
solver = BatchSolver(cfg, max_batch=B, **sopts)
missions_of = lambda ids: None
routes_of = lambda ids: (routes, None if route_of is None else route_of[ids])
if args.own_routes:
    # a sub-fleet takes its own robots' routes only: robot b's are b * L .. b * L + L - 1, and the sub-fleets are runs of consecutive robots
    from mpc_trajectory_generator_amd.trajectory import Missions
    L = args.legs
    routes_of = lambda ids: (routes[ids[0] * L:(ids[-1] + 1) * L], route_of[ids] - ids[0] * L)
    if L > 1:
        missions_of = lambda ids: Missions([[r - ids[0] * L for r in legs_of[b]] for b in ids])
        fleet += f", missions of {L} legs"
elif args.legs > 1:
    # route r driven backwards is route R + r: the same waypoints and circles from the goal to the start
    from mpc_trajectory_generator_amd.trajectory import Missions
    fwd = [routes] if route_of is None else list(routes)
    # (like workloads.handmade_route: the start heading along the first segment, the end heading 0; a mission never reads a leg's start)
    import math
    routes = fwd + [harness.Route(cfg, (w[0][0], w[0][1], math.atan2(w[1][1] - w[0][1], w[1][0] - w[0][0])), (w[-1][0], w[-1][1], 0.0), w,
                                  list(r.vertices)) for r in fwd for w in [list(r.waypoints)[::-1]]]
    route_of = np.zeros(B, dtype=np.int32) if route_of is None else route_of
    missions_of = lambda ids: Missions([[int(route_of[b]) + len(fwd) * (k % 2) for k in range(args.legs)] for b in ids])
    fleet += f", missions of {args.legs} legs (the route and its reverse in turn)"
if not args.host:
    from mpc_trajectory_generator_amd.trajectory import DeviceRecedingHorizon
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    parts = np.array_split(np.arange(B), args.split)
    loops, streams = [], []

    def plant_of(ids):
        """the fleet's plant for the robots ``ids``: a robot keeps its id, its index in the whole fleet"""
        from mpc_trajectory_generator_amd.trajectory import Plant
        return Plant(seed=args.plant_seed, act_gain=(args.plant_act,) * 2, proc=(args.plant_proc,) * 3, meas=(args.plant_meas,) * 3,
                     ids=np.asarray(ids, dtype=np.uint32)) if planted else None

    def pooled(recs):
        """the sub-fleets' records of one step [G] each -> the whole fleet's (n, arrived, mean [G, 3], cov [G, 4]): counts add, means weigh by
        n, and a sub-fleet's second moments move from its own mean to the fleet's"""
        n, arrived = sum(r["n"] for r in recs), sum(r["arrived"] for r in recs)
        w = [r["n"] / np.maximum(n, 1) for r in recs]
        mean = sum(wi[:, None] * r["mean"] for wi, r in zip(w, recs))
        cov = 0.0
        for wi, r in zip(w, recs):
            d = r["mean"] - mean
            cov = cov + wi[:, None] * (r["cov"] + np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]], axis=1))
        return n, arrived, mean, cov

    def make_loop(sv, ids, walls=walls, map_monitor=map_monitor):
        sub_routes, sub_route_of = routes_of(ids)
        return DeviceRecedingHorizon(sv, sub_routes, starts[ids], dyn and tuple(a[ids] for a in dyn), max_steps=args.steps, idx0=i0[ids],
                                     route_of=sub_route_of, peers=peers_of(len(ids)), retire=args.retire, monitor=monitor_of(len(ids)),
                                     missions=missions_of(ids), map_monitor=map_monitor, log=DriveLog() if args.log else None, crowd=crowd,
                                     plant=plant_of(ids), ensemble=None if ens_group_of is None else Ensemble(ens_group_of[ids], groups=ens_G),
                                     walls=walls, track=None if args.track is None else TrackMonitor(args.track))

    for ids in parts:
        sv = solver if not loops else BatchSolver(cfg, max_batch=len(ids), **sopts)
        loops.append(make_loop(sv, ids))
        strm = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(strm)) == 0
        streams.append(strm)
    for rh, strm in zip(loops, streams):
        rh.step(strm)                           # step 0 = cold start; timed separately
    st0 = np.concatenate([rh.read()[4] for rh in loops])        # (synchronises)
    t0 = time.perf_counter()
    steps = args.steps
    if args.retire:
        # a sub-fleet's step waits for the count of its own step before, while the other sub-fleets' steps run on their streams
        while any([rh.steps < args.steps and rh.run(1, strm) for rh, strm in zip(loops, streams)]):
            pass
    else:
        for k in range(1, args.steps):
            for rh, strm in zip(loops, streams):
                rh.step(strm)
    outs = [rh.read() for rh in loops]          # synchronises
    total = time.perf_counter() - t0
    solves = B * (args.steps - 1)
    if args.retire:
        steps = max(rh.steps for rh in loops)
        # after the first step: a retired robot took retired_at solves, an active one as many as its sub-fleet took steps
        solves = int(sum(np.where(at < 0, rh.steps, at).sum() for rh in loops for at in [rh.active()[1]])) - B
    done = np.concatenate([o[3] for o in outs])
    st = np.concatenate([o[4] for o in outs])
    quality = {}
    if args.legs > 1:
        quality["legs_done"] = int(sum((rh.legs()[2] >= 0).sum() for rh in loops))
    if args.peers and args.peer_cell is not None and args.steps >= 1:
        grids = [rh.peer_grid() for rh in loops]                  # the last step's, per sub-fleet
        quality["peer_grid"] = {"cell_m": args.peer_cell, "cells": [[int(h["nx"]), int(h["ny"])] for h, _ in grids],
                                "edges_m": [h["h"].tolist() for h, _ in grids], "filed": int(sum(h["filed"] for h, _ in grids)),
                                "largest_cell": int(max(np.bincount(c[c >= 0]).max(initial=0) for _, c in grids))}
    if args.monitor:
        rec = np.concatenate([rh.clearance() for rh in loops])
        quality["clearance"] = {
            "groups_of": args.monitor, "inside_circle_frac": float((rec["circle"] < 0).mean()),
            "inside_ellipse_frac": float((rec["ellipse"] < 1).mean()),
            "closer_than_two_peer_radii_frac": float((rec["peer2"] < (2 * peer_radius) ** 2).mean()), "two_peer_radii_m": 2 * peer_radius,
            "min_circle_m": float(rec["circle"].min()), "min_ellipse_level": float(rec["ellipse"].min()),
            "min_peer_m": float(np.sqrt(rec["peer2"].min()))}
    if args.map:
        rec = np.concatenate([rh.map_clearance() for rh in loops])
        quality["map_clearance"] = {"polygons": args.map, "edges": len(map_monitor.edges), "robots_hit_frac": float((rec["hits"] > 0).mean()),
                                    "rows_hit": int(rec["hits"].sum()), "min_wall_m": float(np.sqrt(rec["wall2"].min())),
                                    "median_wall_m": float(np.sqrt(np.median(rec["wall2"])))}
        if args.map_cell is not None:
            grids = [rh.map_grid() for rh in loops]                       # the same grid in every sub-fleet; looked is the last step's
            looked = np.concatenate([g[3] for g in grids])
            hdr = grids[0][0]
            near = rec["wall2"][np.isfinite(rec["wall2"])]                # (walls beyond the range are not recorded)
            quality["map_clearance"].update({"robots_with_a_wall_frac": float(len(near) / len(rec)),
                                             "median_wall_m": float(np.sqrt(np.median(near))) if len(near) else None})
            quality["map_clearance"].update({"cell_m": args.map_cell, "range_m": args.map_range, "cells": [int(hdr["nx"]), int(hdr["ny"])],
                                             "filings": int(hdr["entries"]), "looked_mean": float(looked.mean()), "looked_max": int(looked.max())})
        if not args.retire:
            # the stage's time per step: whole runs of the same fleet, timed behind the first step, with the map monitor and without it.
            # The stage observes only, so the two solve the same problems bit for bit and the difference of their times is the stage's.
            # A kernel's own time needs a trace (rocprofv3 --kernel-trace --stats).
            def map_ms_per_step(mm):
                rhs = [make_loop(rh.solver, ids, map_monitor=mm) for rh, ids in zip(loops, parts)]
                for rh in rhs:
                    rh.step()
                    rh.read()
                t = time.perf_counter()
                for k in range(1, args.steps):
                    for rh in rhs:
                        rh.step()
                for rh in rhs:
                    rh.read()
                t = time.perf_counter() - t
                for rh in rhs:
                    rh.close()
                return 1e3 * t / max(args.steps - 1, 1)
            with_it, without = map_ms_per_step(map_monitor), map_ms_per_step(None)
            quality["map_clearance"]["stage"] = {"ms_per_step_with_map": with_it, "ms_per_step_without_map": without,
                                                 "map_stage_ms_per_step": with_it - without}
    if args.track is not None:
        from mpc_trajectory_generator_amd.report import tracking_summary
        quality["tracking"] = {"tol_m": args.track, **tracking_summary(np.concatenate([rh.tracking() for rh in loops]))}
    if walls is not None:
        edge = np.concatenate([rh.walls()[0] for rh in loops])            # the last step's
        quality["walls"] = {"edges": len(walls.edges), "slots": args.walls, "range_m": args.walls_range, "spacing_m": args.walls_spacing,
                            "radius_m": walls.radius, "slots_filled_frac": float((edge >= 0).mean()),
                            "robots_with_a_wall_frac": float((edge >= 0).any(axis=1).mean())}
        if args.walls_cell is not None:
            grids = [rh.wall_grid() for rh in loops]                      # the same grid in every sub-fleet; looked is the last step's
            looked = np.concatenate([g[3] for g in grids])
            hdr = grids[0][0]
            quality["walls"].update({"cell_m": args.walls_cell, "cells": [int(hdr["nx"]), int(hdr["ny"])], "filings": int(hdr["entries"]),
                                     "looked_mean": float(looked.mean()), "looked_max": int(looked.max())})
            # the stage's cost per step under either setter: whole runs of the same fleet on one stream, timed behind the first step, with
            # the grid's setter and (up to 1024 edges) the all-edges one.  The two solve the same problems bit for bit, so the difference of
            # their times is the difference of the two stages, nothing else.  The run without walls is there for scale only: it solves other
            # problems (no wall circles).  A kernel's own time needs a trace (rocprofv3 --kernel-trace --stats).
            import dataclasses

            def ms_per_step(w):
                rhs = [make_loop(rh.solver, ids, w) for rh, ids in zip(loops, parts)]
                for rh in rhs:
                    rh.step()
                    rh.read()
                t = time.perf_counter()
                for k in range(1, args.steps):
                    for rh in rhs:
                        rh.step()
                for rh in rhs:
                    rh.read()
                t = time.perf_counter() - t
                for rh in rhs:
                    rh.close()
                return 1e3 * t / max(args.steps - 1, 1)
            if not args.retire:
                stage = {"ms_per_step_without_walls": ms_per_step(None), "ms_per_step_grid": ms_per_step(walls)}
                if len(walls.edges) <= 1024:
                    stage["ms_per_step_all_edges"] = ms_per_step(dataclasses.replace(walls, cell=None))
                    stage["all_edges_minus_grid_ms_per_step"] = stage["ms_per_step_all_edges"] - stage["ms_per_step_grid"]
                quality["walls"]["stage"] = stage
    if args.crowd:
        seen = np.concatenate([rh.crowd_seen() for rh in loops])          # the last step's
        quality["crowd"] = {"obstacles": args.crowd, "slots": args.crowd_slots, "range_m": args.crowd_range,
                            "slots_filled_frac": float((seen >= 0).mean())}
        if args.crowd_cell is not None:                                   # what each robot looked at at its last step, beside all obstacles' D * N
            grids = [rh.crowd_grid() for rh in loops]
            hdr, looked = grids[0][0], np.concatenate([g[2] for g in grids])
            quality["crowd"].update({"cell_m": args.crowd_cell, "cells": [int(hdr["nx"]), int(hdr["ny"]), int(hdr["layers"])],
                                     "filed": int(hdr["filed"]), "looked_mean": float(looked.mean()), "looked_max": int(looked.max()),
                                     "all_obstacles_look_at": args.crowd * cfg.N_hor})
        if args.crowd_watch:
            # a second, untimed run of the same loops (bit for bit the same) that reads the slots after every step
            recs = [rh.crowd_clearance() for rh in loops]
            unseen = below = 0
            for first, ids, rec in zip(loops, parts, recs):
                rh, hist = make_loop(first.solver, ids), []
                for k in range(first.steps):
                    rh.step()
                    hist.append(rh.crowd_seen())
                assert rh.crowd_clearance().tobytes() == rec.tobytes(), "the second run is not the first"
                rh.close()
                hit = np.nonzero(rec["level"] < 1)[0]
                step = (rec["row"][hit] - 1) // cfg.num_steps_taken
                below += len(hit)
                unseen += sum(int(rec["obstacle"][b] not in hist[k][b]) for b, k in zip(hit, step))
            quality["crowd"].update({"robots_below_level_1": int(below), "of_those_obstacle_not_in_a_slot": int(unseen),
                                     "min_level": float(min(r["level"].min() for r in recs))})
    if planted or args.ensemble:
        quality["plant"] = {"act_gain": args.plant_act, "proc": args.plant_proc, "meas": args.plant_meas, "seed": args.plant_seed}
        if args.ensemble:
            pose = np.concatenate([o[0] for o in outs])
            quality["plant"].update({"final_pose_mean": pose.mean(axis=0).tolist(), "final_pose_std": pose.std(axis=0).tolist()})
    from mpc_trajectory_generator_amd import _lib
    if args.ensemble_stats is not None:
        n, arrived, mean, cov = pooled([rh.ensemble_stats()[-1] for rh in loops])         # every sub-fleet's last step
        std = np.sqrt(cov[:, [0, 2, 3]])
        quality["ensemble"] = {"groups": ens_G, "copies": args.ensemble_stats or B, "members": n[:8].tolist(), "arrived": arrived[:8].tolist(),
                               "mean": mean[:8].tolist(), "std": std[:8].tolist(),
                               "device_bytes": int(sum(rh.max_steps * ens_G * _lib.ENSEMBLE_DTYPE.itemsize + 4 * (ens_G + 1 + rh.B) for rh in loops))}
        if args.ensemble:
            host_std = np.array(quality["plant"]["final_pose_std"])
            quality["ensemble"]["std_rel_diff_from_host"] = float((np.abs(std[0] - host_std) / np.where(host_std > 0, host_std, 1.0)).max())
    if args.log:
        tot = [rh.step_totals() for rh in loops]
        summ = np.concatenate([rh.drive_summary() for rh in loops])
        exits = sum(t["exits"].sum(axis=0) for t in tot)
        worst = max(tot, key=lambda t: t["solve_ms_max"].max(initial=0.0))
        quality["drive_log"] = {
            "solves": int(exits.sum()),
            "not_converged_frac": {_lib.EXIT_STATUS[e]: float(exits[e] / max(exits.sum(), 1)) for e in range(1, 5)},
            "worst_step": int(np.argmax(worst["solve_ms_max"])) + 1 if len(worst) else 0,
            "worst_step_solve_ms_max": float(worst["solve_ms_max"].max(initial=0.0)),
            "max_acc_abs": float(summ["acc_abs_max"].max()), "max_wacc_abs": float(summ["wacc_abs_max"].max()),
            "device_bytes": int(sum(rh.max_steps * rh.B * (rh.cfg.num_steps_taken * 16 + _lib.STEP_RECORD_DTYPE.itemsize)
                                    + rh.B * _lib.DRIVE_SUMMARY_DTYPE.itemsize + rh.max_steps * _lib.STEP_TOTALS_DTYPE.itemsize for rh in loops))}
    if hasattr(_lib.load_library(), "nmpc_debug_win_stats"):        # instrumented build (-DNMPC_WIN_STATS, scripts/win_stats.py)
        buf = (ctypes.c_ulonglong * 2)()
        _lib.load_library().nmpc_debug_win_stats(buf, 0)
        print(f"windowed cross-track searches {buf[0]}, fell back {buf[1]} ({100.0 * buf[1] / max(buf[0], 1):.1f} %)", file=sys.stderr)
    print(json.dumps({
        "metric": "nmpc_receding_horizon_solves_per_sec", "value": solves / total, "unit": "solves/s",
        "config": {"workload": f"cfg4 smooth_velocity, scene {args.scene}{fleet}, B={B}, {args.steps} receding-horizon steps, "
                               "num_steps_taken=2, warm start (u, y carried; c reset), loop entirely on device"
                               + (f", robots start up to {args.back} samples before the route's end" if args.back != 60 else "")
                               + (", robots retire at their goals" if args.retire else "")
                               + (f", clearance monitor in groups of {args.monitor}" if args.monitor else "")
                               + (f", map monitor on the scene's {args.map} polygons" if args.map else "")
                               + (f" cut into {len(map_monitor.edges)} edges" if args.map and args.map_pieces > 1 else "")
                               + (f", found through a grid of {args.map_cell} m" if args.map_cell is not None else "")
                               + (f", track monitor with tol {args.track} m" if args.track is not None else "")
                               + (", drive log" if args.log else "")
                               + (f", ensemble statistics in {ens_G} group{'s' if ens_G > 1 else ''}" if args.ensemble_stats is not None else "")
                               + (f", at most {args.budget} PANOC iterations per solve (NotConvergedOutOfTime beyond)" if args.budget else "")
                               + (f", fleet split into {args.split} sub-fleets on {args.split} streams" if args.split > 1 else ""),
                   "kernel": solver.kernel_name},
        "steps": steps, "solves": solves + B, "seconds_after_first_step": total,
        "ms_per_step": 1e3 * total / max(steps - 1, 1), "mean_inner_iters_first_step": float(st0["num_inner_iterations"].mean()),
        "mean_inner_iters_last_step": float(st["num_inner_iterations"].mean()),
        "converged_frac_last_step": float((st["exit_status"] == 0).mean()),
        "out_of_time_frac_last_step": float((st["exit_status"] == 2).mean()), "robots_at_goal": int(done.sum()), **quality, **planning}))
    sys.exit(0)
if route_of is None and not args.peers:
    rh = VectorizedRecedingHorizon(routes, starts, dyn, idx0=i0)
elif route_of is None:
    rh = FleetRecedingHorizon([routes], np.zeros(B, dtype=np.int32), starts, dyn, idx0=i0, peers=peers_of(B))
else:
    rh = FleetRecedingHorizon(routes, route_of, starts, dyn, idx0=i0, peers=peers_of(B))
t_solve, t_asm, iters, conv = [], [], [], []


def solve(P, U, Y):
    t = time.perf_counter()
    out = solver.solve(P, u0=U, y0=Y)
    t_solve.append(time.perf_counter() - t)
    return out


t0 = time.perf_counter()
for k in range(args.steps):
    t = time.perf_counter()
    P = rh.assemble()
    t_asm.append(time.perf_counter() - t)
    U, Y, st = solve(P, rh.U, rh.Y)
    rh.U, rh.Y = U, Y
    rh.advance(U)
    iters.append(float(st["num_inner_iterations"].mean()))
    conv.append(float((st["exit_status"] == 0).mean()))
total = time.perf_counter() - t0
print(json.dumps({
    "metric": "nmpc_receding_horizon_solves_per_sec", "value": B * args.steps / total, "unit": "solves/s",
    "config": {"workload": f"cfg4 smooth_velocity, scene {args.scene}{fleet}, B={B}, {args.steps} receding-horizon steps, "
                           "num_steps_taken=2, warm start (u, y carried; c reset), host-side vectorised p assembly"},
    "solver_only_solves_per_sec": B * args.steps / sum(t_solve), "ms_per_step_total": 1e3 * total / args.steps,
    "ms_per_step_solve_incl_pcie": 1e3 * float(np.mean(t_solve)), "ms_per_step_assembly": 1e3 * float(np.mean(t_asm)),
    "mean_inner_iters_first_step": iters[0], "mean_inner_iters_steady": float(np.mean(iters[5:])),
    "converged_frac_steady": float(np.mean(conv[5:])), "robots_at_goal": int(rh.done.sum())}))
