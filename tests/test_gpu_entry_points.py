"""GPU: what carries a batch to and from the solve and eval kernels -- the host half of csrc/nmpc_kernels.hip and the device entry points --
at the batch sizes where the launch geometry changes regime and where the host staging changes path.  The kernels' arithmetic is held to
the oracle elsewhere; here the oracle says which row belongs where.

* the launch geometry (``BatchSolver.launch_geometry``, csrc/nmpc_launch.h; its rule: tests/test_launch_geometry.py) on a real handle, and
  every regime it has -- one to four owners per workgroup, with and without launch order and pools, below and above the kernel's
  first-round hold -- solved through the device path for the prefixes of one batch, for one handle per kernel family row;
* the device entry points as include/nmpc_solver.h documents them: everything on the caller's stream, every optional operand given or NULL,
  launches back to back, in place, on two handles at once, and the on-device loop on a caller's stream;
* the host staging: one to four chunks per array, a row across a chunk boundary, the small-batch arena against the staged path, and
  operands a previous call left behind.

Device outputs are pre-filled with 0xFF bytes (a NaN as float64) between two guard rows (``entry_cases.Guarded``): a row nobody wrote keeps
the sentinel, and a write outside rows 0 .. B - 1 lands in a guard row.  (u is the initial guess as well: its rows start as zeros, which no
solution equals.)

The oracle runs once per family, on its longest batch (2561, 2561 and 1281 rows on an MI355X); the measured times are in ``case``."""
import ctypes as C
import functools
import itertools
import time
import types

import numpy as np
import pytest

from conftest import oracle_for
from entry_cases import DeviceSolve, Delay, Guarded, family, literal_geometry, sweep_sizes, timed_ms, to_device
from mpc_trajectory_generator_amd import _lib, harness, named_config
from mpc_trajectory_generator_amd.config import load_config
from mpc_trajectory_generator_amd.workloads import LOG_CLOCK_FIELDS, PARITY_FIELDS, crowd_ellipses, differing, fleet_ellipses

pytestmark = pytest.mark.gpu
THREADS = 16
GEOMETRY = ("grid", "owners", "workgroups", "ordered", "pools", "pool_cap")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> one handle of the family row ``name`` with room for W + W / 4 + 1 instances, that batch, and the oracle's solve of it (the one
    oracle run of the family: instances are independent, so a prefix's answer is the prefix of the answers).

    Measured oracle times, 16 threads on 8 cores: cfg1, 2561 rows, default options (mean 1285 inner iterations, 1056 instances with three
    or more outer iterations) 5.7 s -- once for the eight tests that use the handle; n17, 2561 rows, max_inner 100 / max_outer 5 (1116
    instances with three or more outer iterations) 0.94 s; cfg2, 1281 rows, max_inner 60 / max_outer 4 (502 such instances) 0.56 s.
    On an MI355X host with 16 cores the three runs took 1.09, 0.17 and 0.10 s.  (cfg1 with max_inner 100 / max_outer 5 would cost 1.1 s on the 8 cores, but then no test would run the headline kernel's full-length solves through
    these launch regimes.)"""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg, kernel, opts, per_cu, batch = family(name)
    probe = BatchSolver(cfg, max_batch=1, **opts)
    W = probe.launch_geometry(1)["resident_waves"]
    probe.close()
    Bmax = W + W // 4 + 1
    s = BatchSolver(cfg, max_batch=Bmax, **opts)
    P = batch(Bmax, 20241)
    t0 = time.perf_counter()
    ref = oracle_for(cfg, **opts).solve_batch(P, threads=THREADS)
    print(f"{name}: oracle on {Bmax} rows in {time.perf_counter() - t0:.2f} s; exit statuses {np.bincount(ref[2]['exit_status'], minlength=5).tolist()}, "
          f"outer iterations up to {int(ref[2]['num_outer_iterations'].max())}")
    assert int(ref[2]["num_outer_iterations"].max()) >= 3, "no instance reaches a third outer iteration: nothing would park"
    _OPEN.append(s)
    return types.SimpleNamespace(name=name, cfg=cfg, kernel=kernel, opts=opts, per_cu=per_cu, s=s, W=W, G=W // 4, Bmax=Bmax, P=P, ref=ref,
                                 family=20 if cfg.N_hor <= 20 else 40)


_OPEN = []


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    while _OPEN:
        _OPEN.pop().close()
    case.cache_clear()


def rows_of(ref, rows):
    return tuple(x[rows] for x in ref)


def given_differing(got, want):
    """``differing`` over the outputs that were asked for: (u, y or None, status or None) against the oracle's triple"""
    bad = [] if np.array_equal(got[0], want[0]) else ["u"]
    if got[1] is not None and not np.array_equal(got[1], want[1]):
        bad.append("y")
    if got[2] is not None:
        bad += [f for f in PARITY_FIELDS if not np.array_equal(got[2][f], want[2][f])]
    return bad


def sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. the getter on a real handle
@pytest.mark.parametrize("name", ["cfg1", "n17", "cfg2"])
def test_resident_waves_and_getter(name):
    """W is the device's CU count times 8 (one stage per lane, two teams per CU) or 4 (two stages per lane), as nmpc_new documents; the
    getter gives the literal rule for every batch size around the boundaries, and refuses sizes outside 0 .. max_batch."""
    import torch
    from mpc_trajectory_generator_amd.solver import SolverError
    c = case(name)
    assert c.s.kernel_name == c.kernel
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert c.W == cus * c.per_cu and c.W % 4 == 0, (c.W, cus)
    for B in sorted(set(sweep_sizes(c.W) + [0, 2, 3, c.Bmax])):
        g = c.s.launch_geometry(B)
        assert tuple(g[k] for k in GEOMETRY) == literal_geometry(B, c.W, c.family), (B, g)
        assert g["resident_waves"] == c.W and g["staging_chunk_bytes"] > 0 and g["staging_chunk_bytes"] % 8 == 0
    for B in (-1, c.Bmax + 1):
        with pytest.raises(SolverError):
            c.s.launch_geometry(B)
    assert c.s.lib.nmpc_launch_geometry(None, 1, C.byref(_lib.NmpcLaunchInfo())) == -3
    assert c.s.lib.nmpc_launch_geometry(c.s._h, 1, None) == -3


# ------------------------------------------------------------------------------------------------ 2. every launch regime at its boundaries
@pytest.mark.parametrize("name", ["cfg1", "n17", "cfg2"])
def test_every_launch_regime_at_its_boundaries(name):
    """The prefixes P[:B] of one batch at B = 1, G - 1, G, G + 1, 2G - 1, 2G, 2G + 1, 3G, 3G + 1, W - 1, W, W + 1, W + 2 and the three
    sizes around W + W / 4, through the device path into guarded, sentinel-filled outputs: rows 0 .. B - 1 are the oracle's, bit for bit, no
    sentinel survives in them, and both guard rows of u, y_out and status keep their bytes."""
    c = case(name)
    W, G = c.W, c.G
    sizes = sweep_sizes(W)
    assert sizes == sorted(set(sizes)) and sizes[0] == 1 and sizes[-1] == c.Bmax, sizes
    geo = {B: c.s.launch_geometry(B) for B in sizes}
    # the sweep reaches every regime (a handle whose geometry left one out would fail here, not skip it)
    assert {g["owners"] for g in geo.values()} == {1, 2, 3, 4}, geo
    assert {g["ordered"] for g in geo.values()} == {0, 1} and {g["pools"] for g in geo.values()} == {0, 1}, geo
    assert all((g["ordered"], g["pools"]) == ((1, 1) if B > W else (0, 0)) for B, g in geo.items())
    assert [geo[B]["owners"] for B in (1, G, G + 1, 2 * G, 2 * G + 1, 3 * G, 3 * G + 1, W)] == [1, 1, 2, 2, 3, 3, 4, 4]
    hold = W + W // 4                                  # the kernel's first-round hold: B >= n_waves + n_waves / 4
    assert [B for B in sizes if W < B < hold] and [B for B in sizes if B >= hold] == [hold, hold + 1]
    d_P = to_device(c.P)
    launched = []
    for B in sizes:
        run = DeviceSolve(c.s, B)
        run.launch(d_P[:B])
        sync()
        bad = differing(run.result(), rows_of(c.ref, slice(0, B)))
        assert not bad, f"B = {B} ({geo[B]}): {bad}"
        launched.append((B, geo[B]["owners"], geo[B]["ordered"], geo[B]["pools"], int(B >= hold)))
    print(name, "W", W, "launched (B, owners, ordered, pools, held):", launched)


# ------------------------------------------------------------------------------------------------ 3. the device entry points as documented
def _measured_delay(stream, enqueue_alone, what):
    """-> a ``Delay`` at least twice as long as ``enqueue_alone`` takes on ``stream``, both timed with events; prints both"""
    timed_ms(stream, enqueue_alone)                    # (a first run: allocations, code loading)
    alone_ms = timed_ms(stream, enqueue_alone)
    delay = Delay().sized_for(alone_ms, stream)
    delay_ms = delay.measure(stream)
    print(f"{what}: alone {alone_ms:.3f} ms, the delay in front of it {delay_ms:.3f} ms ({delay.rounds} products)")
    assert delay_ms >= 2.0 * alone_ms, (delay_ms, alone_ms)
    return delay


def test_solve_on_the_callers_stream():
    """On a non-default (non-blocking) stream: a delay, the copies that fill two NaN parameter arrays, then two solves of B = W + 50, nothing
    synchronised in between.  Classify, order, the clearing of queue, pools and counters and the solve itself must all wait for the copies:
    whatever went to another stream runs before its producer (a classify that reads NaN; a queue cleared before the first solve has used
    it, which leaves the second solve nothing to fetch).  Both results are the oracle's."""
    import torch
    c = case("cfg1")
    s, B = c.s, c.W + 50
    g = s.launch_geometry(B)
    assert g["ordered"] == 1 and g["pools"] == 1
    stream = torch.cuda.Stream()
    rows = (slice(0, B), slice(c.Bmax - B, c.Bmax))
    src = [to_device(c.P[r]) for r in rows]
    d_p = [torch.full((B, s.n_p), float("nan"), dtype=torch.float64, device="cuda") for _ in rows]
    sync()
    # (fresh outputs for every timed run: a second solve into the same u would start from the first one's solution)
    delay = _measured_delay(stream, lambda: DeviceSolve(s, B).launch(src[0], stream=stream), f"solve of {B} on its own stream")
    runs = [DeviceSolve(s, B) for _ in rows]
    sync()
    with torch.cuda.stream(stream):
        delay.enqueue()
        for dst, a in zip(d_p, src):
            dst.copy_(a, non_blocking=True)
        for run, p in zip(runs, d_p):
            run.launch(p, stream=stream)
    sync()
    for k, (run, r) in enumerate(zip(runs, rows)):
        bad = differing(run.result(), rows_of(c.ref, r))
        assert not bad, f"solve {k}: {bad}"


def oracle_eval(o, P, U, c, y):
    """-> psi [B], grad [B, n_u], F1 [B, n1], F2 [B, n2] of the oracle, row by row (c, y: arrays or None)"""
    out = [o.eval(P[i], U[i], 0.0 if c is None else float(c[i]), None if y is None else y[i]) for i in range(len(P))]
    return tuple(np.array([r[k] for r in out]).reshape(len(P), -1) for k in range(4))


def eval_device(s, B, d_p, d_u, d_c, d_y, outs, stream=None):
    """nmpc_eval_batch_device through ctypes; outs: four ``Guarded`` or None (psi, grad, F1, F2)"""
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    s._check(s.lib.nmpc_eval_batch_device(s._h, B, ptr(d_p), ptr(d_u), ptr(d_c), ptr(d_y), *[None if g is None else g.ptr for g in outs],
                                          None if stream is None else C.c_void_p(stream.cuda_stream)))


def eval_outputs(s, B, which=(1, 1, 1, 1)):
    cols = (1, s.n_u, s.n1, s.n2)
    return [Guarded(B, 8 * n) if w else None for n, w in zip(cols, which)]


def eval_differing(outs, want):
    """(after a synchronisation) the names of the outputs given that are not the oracle's bits or still hold a sentinel; guards asserted"""
    bad = []
    for name, g, w in zip(("psi", "grad", "F1", "F2"), outs, want):
        if g is not None and (g.sentinels().size or g.host().tobytes() != np.ascontiguousarray(w).tobytes()):
            bad.append(name)
    return bad


def eval_points(c, B, seed):
    """-> (P, U, c, y): B rows of the family's batch with controls inside the bounds, penalties and multipliers drawn from ``seed``"""
    rng = np.random.default_rng(seed)
    n_u, n1 = c.s.n_u, c.s.n1
    U = np.stack([rng.uniform(0.0, c.cfg.lin_vel_max, (B, n_u // 2)), rng.uniform(-0.5, 0.5, (B, n_u // 2))], axis=2).reshape(B, n_u)
    return c.P[:B], U, rng.uniform(1.0, 50.0, B), rng.normal(0.0, 0.3, (B, n1))


@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_eval_on_the_callers_stream(name):
    import torch
    c = case(name)
    s, B = c.s, 50
    P, U, cc, yy = eval_points(c, B, 5)
    want = oracle_eval(oracle_for(c.cfg, **c.opts), P, U, cc, yy)
    stream = torch.cuda.Stream()
    src_p, d_u, d_c, d_y = to_device(P), to_device(U), to_device(cc), to_device(yy)
    d_p = torch.full((B, s.n_p), float("nan"), dtype=torch.float64, device="cuda")
    warm = eval_outputs(s, B)
    sync()
    delay = _measured_delay(stream, lambda: eval_device(s, B, src_p, d_u, d_c, d_y, warm, stream), f"{name}: eval of {B} on its own stream")
    outs = eval_outputs(s, B)
    sync()
    with torch.cuda.stream(stream):
        delay.enqueue()
        d_p.copy_(src_p, non_blocking=True)
        eval_device(s, B, d_p, d_u, d_c, d_y, outs, stream)
    sync()
    assert not eval_differing(outs, want)


def test_solve_optional_operands():
    """d_y0, d_c0, d_y_out and d_status each given or NULL, all sixteen ways: u is the oracle's for those initial multipliers and penalties,
    and so are y_out and status wherever they were asked for."""
    c = case("cfg1")
    s, B = c.s, 24
    rng = np.random.default_rng(11)
    P, y0, c0 = c.P[:B], rng.normal(0.0, 0.2, (B, s.n1)), rng.uniform(2.0, 30.0, B)
    o = oracle_for(c.cfg, **c.opts)
    want = {(hy, hc): o.solve_batch(P, y0=y0 if hy else None, c0=c0 if hc else None, threads=THREADS) for hy in (0, 1) for hc in (0, 1)}
    assert not differing(want[0, 0], rows_of(c.ref, slice(0, B)))
    for a, b in itertools.combinations(want, 2):
        assert "u" in differing(want[a], want[b]), "the operands make no difference: the test would not see one that was dropped"
    d_P, d_y0, d_c0 = to_device(P), to_device(y0), to_device(c0)
    for hy, hc, wy, ws in itertools.product((0, 1), repeat=4):
        run = DeviceSolve(s, B, y_out=bool(wy), status=bool(ws))
        run.launch(d_P, d_y0 if hy else None, d_c0 if hc else None)
        sync()
        got = run.result()
        assert (got[1] is not None, got[2] is not None) == (bool(wy), bool(ws))
        bad = given_differing(got, want[hy, hc])
        assert not bad, f"y0 {hy} c0 {hc} y_out {wy} status {ws}: {bad}"


EVAL_OUTPUTS = [(1, 1, 1, 1)] + [tuple(int(i != k) for i in range(4)) for k in range(4)] + [tuple(int(i == k) for i in range(4)) for k in range(4)]


@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_eval_optional_operands_and_guard_rows(name):
    """nmpc_eval_batch_device at B = 1 .. 5 (an eval wave holds three instances: one wave, a partly filled one, two): all four outputs,
    each NULL in turn, all NULL but one, with c and y each NULL or given.  What was asked for is the oracle's, bit for bit, without a
    sentinel left, and the guard rows around psi, grad, F1 and F2 keep their bytes."""
    c = case(name)
    s = c.s
    o = oracle_for(c.cfg, **c.opts)
    P, U, cc, yy = eval_points(c, 5, 6)
    d_P, d_U, d_c, d_y = to_device(P), to_device(U), to_device(cc), to_device(yy)
    want = {(hc, hy): oracle_eval(o, P, U, cc if hc else None, yy if hy else None) for hc in (0, 1) for hy in (0, 1)}
    # (c and y both matter: psi differs with c, and with y once c is given; y alone, at c = 0, leaves plain f)
    assert not np.array_equal(want[1, 1][0], want[0, 0][0]) and not np.array_equal(want[1, 1][0], want[1, 0][0])
    for B in (1, 2, 3, 4, 5):
        for (hc, hy), which in itertools.product(want, EVAL_OUTPUTS):
            outs = eval_outputs(s, B, which)
            eval_device(s, B, d_P[:B], d_U[:B], d_c[:B] if hc else None, d_y[:B] if hy else None, outs)
            sync()
            bad = eval_differing(outs, [w[:B] for w in want[hc, hy]])
            assert not bad, f"B = {B}, c {hc}, y {hy}, outputs {which}: {bad}"


def test_back_to_back_without_synchronising():
    """One handle, one stream: launches of W + 50, 5, W + 50 and 17 instances on buffers of their own and different inputs, one
    synchronisation at the end, each result its own oracle rows; then a warm chain of three launches in place -- d_u input and output,
    d_y_out the very tensor d_y0 is -- which must be the oracle's warm chain."""
    import torch
    c = case("cfg1")
    s, big = c.s, c.W + 50
    rows = [slice(0, big), slice(100, 105), slice(c.Bmax - big, c.Bmax), slice(200, 217)]
    d_p = [to_device(c.P[r]) for r in rows]
    runs = [DeviceSolve(s, r.stop - r.start) for r in rows]
    stream = torch.cuda.Stream()
    sync()
    for run, p in zip(runs, d_p):
        run.launch(p, stream=stream)
    sync()
    for run, r in zip(runs, rows):
        bad = differing(run.result(), rows_of(c.ref, r))
        assert not bad, f"rows {r}: {bad}"
    # the warm chain
    B = 96
    links = [c.P[k * B:(k + 1) * B] for k in range(3)]
    d_links = [to_device(p) for p in links]
    u, y, st = Guarded(B, 8 * s.n_u, fill=np.zeros((B, s.n_u))), Guarded(B, 8 * s.n1, fill=np.zeros((B, s.n1))), Guarded(B, _lib.STATUS_DTYPE.itemsize)
    sync()
    for p in d_links:
        s.solve_device(p, u.f64(), y.f64(), None, y.f64(), st.u8(), stream=stream)
    sync()
    o = oracle_for(c.cfg, **c.opts)
    U, Y = np.zeros((B, s.n_u)), np.zeros((B, s.n1))
    for p in links:
        U, Y, S = o.solve_batch(p, u0=U, y0=Y, threads=THREADS)
    assert not st.sentinels().size
    bad = differing((u.host(), y.host(), st.host(_lib.STATUS_DTYPE).reshape(B)), (U, Y, S))
    assert not bad, bad
    assert "u" in differing((U, Y, S), rows_of(c.ref, slice(2 * B, 3 * B))), "the chain's last link equals a cold solve"


def test_two_handles_two_streams():
    """A one-stage and a two-stage handle, 64 and 48 instances, launched together on two streams: both grids are resident at once, and each
    handle's result is what it gives alone (and the oracle's)."""
    import torch
    a, b = case("cfg1"), case("cfg2")
    pairs = [(a, 64, torch.cuda.Stream()), (b, 48, torch.cuda.Stream())]
    d_p = [to_device(c.P[:B]) for c, B, _ in pairs]
    alone = []
    for (c, B, stream), p in zip(pairs, d_p):
        run = DeviceSolve(c.s, B)
        sync()
        run.launch(p, stream=stream)
        sync()
        alone.append(run.result())
    runs = [DeviceSolve(c.s, B) for c, B, _ in pairs]
    sync()
    for (c, B, stream), p, run in zip(pairs, d_p, runs):
        run.launch(p, stream=stream)
    sync()
    for (c, B, _), run, single in zip(pairs, runs, alone):
        got = run.result()
        assert not differing(got, single), c.name
        assert not differing(got, rows_of(c.ref, slice(0, B))), c.name


def _loop_readouts(dev):
    """-> {name: bytes} of everything the all-stages loop can be asked for, the clocks aside"""
    sync()
    out = dict(zip(("P", "U", "Y"), dev.params()))
    state, last_u, idx, done, st = dev.read()
    out.update(state=state, last_u=last_u, idx=idx, done=done, trajectory=dev.trajectory(), clearance=dev.clearance(),
               map_clearance=dev.map_clearance(), tracking=dev.tracking(), crowd_clearance=dev.crowd_clearance(), crowd_seen=dev.crowd_seen(),
               crowd_table=dev.crowd_table(), controls=dev.controls(), drive_summary=dev.drive_summary())
    out["wall_edge"], out["wall_stage"] = dev.walls()
    out["peer_grid"], out["cell_of"] = dev.peer_grid()
    for f in PARITY_FIELDS:
        out["status." + f] = st[f]
    for name, rec in (("step_records", dev.step_records()), ("step_totals", dev.step_totals())):
        for f in rec.dtype.names:
            if f not in LOG_CLOCK_FIELDS:
                out[f"{name}.{f}"] = rec[f]
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


def test_the_loop_on_a_callers_stream():
    """The all-stages fleet of tests/test_gpu_track_loop.py (watched crowd, grid peers, walls, both monitors, log, track) for three steps on
    a non-default stream behind a measured delay, nothing synchronised in between, against the same loop on the null stream: state,
    trajectory, P, U, Y and every stage's readout are equal bit for bit."""
    import torch
    from mpc_trajectory_generator_amd.solver import BatchSolver
    from mpc_trajectory_generator_amd.trajectory import Crowd, DeviceRecedingHorizon, DriveLog, MapMonitor, Monitor, Peers, TrackMonitor
    from test_walls_mirror import fleet24, scene_map, walls_of
    cfg = named_config("cfg4")
    routes, route_of, starts, i0 = fleet24(cfg)
    dyn = fleet_ellipses(routes, route_of, i0, 1, 9)

    def make(s):
        kw = dict(idx0=i0, crowd=Crowd(crowd_ellipses(cfg, 11, 70, 23), 1, 1e3, watch=True),
                  peers=Peers(slots=1, rx=0.37, ry=0.53, range=1e3, cell=1.0), walls=walls_of(cfg, pieces=4, spacing=1.0), monitor=Monitor(),
                  map_monitor=MapMonitor(*scene_map(cfg, 4)), log=DriveLog(), track=TrackMonitor(0.05))
        return DeviceRecedingHorizon(s, routes, starts, dyn, max_steps=3, route_of=route_of, **kw)

    s = BatchSolver(cfg, max_batch=32)
    stream = torch.cuda.Stream()
    dev = None
    try:
        dev = make(s)
        sync()

        def three_steps(loop, where):
            for _ in range(3):
                loop.step(where)

        loop_ms = timed_ms(torch.cuda.default_stream(), lambda: three_steps(dev, None))
        want = _loop_readouts(dev)
        dev.close()
        dev = make(s)
        delay = Delay().sized_for(loop_ms, stream)
        delay_ms = delay.measure(stream)
        print(f"three steps of the loop on the null stream {loop_ms:.3f} ms, the delay in front of them {delay_ms:.3f} ms ({delay.rounds} products)")
        assert delay_ms >= 2.0 * loop_ms
        sync()
        with torch.cuda.stream(stream):
            delay.enqueue()
            three_steps(dev, C.c_void_p(stream.cuda_stream))
        got = _loop_readouts(dev)
        assert sorted(got) == sorted(want)
        bad = [k for k in want if got[k] != want[k]]
        assert not bad, bad
        assert np.frombuffer(want["tracking"], dtype=_lib.TRACKING_DTYPE)["rows"].min() == 6       # (the yardstick drove: two rows a step)
    finally:
        if dev is not None:
            dev.close()
        s.close()


# ------------------------------------------------------------------------------------------------ 4. the host staging at its boundaries
STAGING_OPTS = dict(max_inner=2, max_outer=1)          # every solve short: the data path is under test, not convergence


def tiled_batch(cfg, B, seed=3, base=64):
    """-> P [B, n_p]: ``base`` instances of ``synthetic_batch`` repeated to B rows, each row's start pose moved by an offset of its own"""
    P = harness.synthetic_batch(cfg, 11, base, seed)[np.arange(B) % base]
    P[:, 0] += 1e-6 * np.arange(B)
    P[:, 1] -= 2e-6 * np.arange(B)
    return np.ascontiguousarray(P)


def boundary_rows(B, row_bytes, chunk, total=64, seed=0):
    """-> ``total`` sorted rows of 0 .. B - 1: the first, the last, the rows on either side of every chunk boundary of an array of
    ``row_bytes`` rows (the row a boundary cuts and both of its neighbours), the rest drawn from ``seed``"""
    rows = {0, B - 1}
    for off in range(chunk, B * row_bytes, chunk):
        r = off // row_bytes                           # the row byte `off` belongs to: it begins a chunk, or straddles the boundary
        rows |= {r - 2, r - 1, r, r + 1}
    rows = {r for r in rows if 0 <= r < B}
    rng = np.random.default_rng(seed)
    while len(rows) < min(total, B):
        rows.add(int(rng.integers(0, B)))
    return np.array(sorted(rows))


@pytest.mark.parametrize("N,B,chunks", [(32, 8192, 1), (32, 8193, 2), (32, 16384, 2), (32, 16385, 3), (32, 24577, 4), (20, 13200, 2)])
def test_host_staging_chunks(N, B, chunks):
    """The host path against the device path (operands moved by torch, not by the staging code) over all rows, and against the oracle
    on 64 rows that include the first, the last and those on either side of every chunk boundary.  N = 32: rows of u and y_out are 512
    bytes, so 8192 rows are exactly one chunk; 16385 rows are three chunks, the first reuse of a pinned buffer, 24577 four: both buffers
    reused.  N = 20 at 13200 rows: rows of 320 bytes, of which row 13107 lies across the boundary."""
    from mpc_trajectory_generator_amd.solver import BatchSolver
    cfg = load_config(N_hor=N)
    P = tiled_batch(cfg, B)
    s = BatchSolver(cfg, max_batch=B, **STAGING_OPTS)
    try:
        chunk = s.launch_geometry(B)["staging_chunk_bytes"]
        row = 8 * s.n_u
        assert s.n1 == s.n_u and -(-B * row // chunk) == chunks, (B * row, chunk)
        if N == 32:
            assert chunk % row == 0 and chunk // row == 8192
        else:
            assert chunk % row != 0 and B * row > chunk
        run = DeviceSolve(s, B)
        run.launch(to_device(P))
        sync()
        want = run.result()
        assert (want[0][1:] != want[0][:-1]).any(axis=1).all(), "two neighbouring rows of u are equal: a misplaced row could pass"
        per_chunk = -(-chunk // row)
        if B > per_chunk:                              # ... nor may the rows one chunk apart (copies of one base instance for N = 32)
            assert (want[0][per_chunk:] != want[0][:-per_chunk]).any(axis=1).all(), "two rows a chunk apart are equal"
        got = s.solve(P)
        bad = differing(got, want)
        if bad:
            wrong = np.nonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]).any(axis=1))[0]
            raise AssertionError(f"{bad}; first wrong rows of u / y: {wrong[:10]} of {wrong.size}")
        rows = boundary_rows(B, row, chunk)
        assert len(rows) == 64 and rows[0] == 0 and rows[-1] == B - 1
        for k in range(1, chunks):
            r = k * chunk // row
            assert {r - 1, r, min(r + 1, B - 1)} <= set(rows.tolist())      # (at B = 8193, 16385, 24577 row r is the last one)
        ref = oracle_for(cfg, **STAGING_OPTS).solve_batch(P[rows], threads=THREADS)
        assert not differing(got, ref, rows)
    finally:
        s.close()


def test_arena_and_staged_path_alternate():
    """One handle, B = 17, 16, 17, 1, 16 in a row with different P: the staged path and the small-batch arena take turns, each result the
    oracle's.  (The arena and the staging buffers keep the previous call's bytes.)"""
    c = case("cfg1")
    at = 300
    for B in (17, 16, 17, 1, 16):
        r = slice(at, at + B)
        at += B
        bad = differing(c.s.solve(c.P[r]), rows_of(c.ref, r))
        assert not bad, f"B = {B}: {bad}"


@pytest.mark.parametrize("B", [8, 40])
def test_stale_warm_start_operands(B):
    """On the arena (B = 8) and on the staged path (B = 40): a solve with y0 and c0, then one with neither on the same P.  The second is
    the oracle's cold-multiplier solve, although the handle's buffers still hold the first call's y0 and c0."""
    c = case("cfg1")
    rng = np.random.default_rng(B)
    r = slice(500, 500 + B)
    P, y0, c0 = c.P[r], rng.normal(0.0, 0.2, (B, c.s.n1)), rng.uniform(2.0, 30.0, B)
    warm = oracle_for(c.cfg, **c.opts).solve_batch(P, y0=y0, c0=c0, threads=THREADS)
    cold = rows_of(c.ref, r)
    assert "u" in differing(warm, cold)
    assert not differing(c.s.solve(P, y0=y0, c0=c0), warm)
    assert not differing(c.s.solve(P), cold)
    assert not differing(c.s.solve(P, y0=y0), oracle_for(c.cfg, **c.opts).solve_batch(P, y0=y0, threads=THREADS))
    assert not differing(c.s.solve(P, c0=c0), oracle_for(c.cfg, **c.opts).solve_batch(P, c0=c0, threads=THREADS))


@pytest.mark.parametrize("name", ["cfg1", "cfg2"])
def test_eval_host_path_forgets_c_and_y(name):
    """``evaluate`` with c and y, then without them: the second call gives plain f, although the staging buffers still hold c and y."""
    c = case(name)
    o = oracle_for(c.cfg, **c.opts)
    P, U, cc, yy = eval_points(c, 5, 7)
    for hc, hy in ((1, 1), (0, 0), (0, 1), (0, 0), (1, 0), (0, 0)):
        got = c.s.evaluate(P, U, cc if hc else None, yy if hy else None)
        want = oracle_eval(o, P, U, cc if hc else None, yy if hy else None)
        bad = [n for n, x, w in zip(("psi", "grad", "F1", "F2"), got, want) if np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(w).tobytes()]
        assert not bad, (hc, hy, bad)
