"""What the entry-point tests share (tests/test_launch_geometry.py, tests/test_gpu_entry_points.py): the launch geometry's rule restated
literally, the kernel-family rows under test, device buffers with guard rows, and a delay of measured length on a stream."""
import ctypes as C

import numpy as np

from mpc_trajectory_generator_amd import _lib, harness, named_config
from mpc_trajectory_generator_amd.config import load_config

TEAM_WAVES = 4


def literal_geometry(B, grid_cap, P, use_order=True, park_min=500, sched_mode=1, forced=0):
    """-> (grid, owners, workgroups, ordered, pools, pool_cap): the rule of DESIGN.md section 5.5 and of solve_launch's comments.

    A persistent grid of min(B, resident waves) waves takes the instances, in teams of four.  With no more instances than workgroups fit
    on the chip (a quarter of the resident waves) every instance gets a workgroup of its own; otherwise as many waves per workgroup take
    instances as it needs for all of them to start at once, up to all four.  A launch with more instances than resident waves hands the
    hard-looking ones out first (unless ordering is switched off) and lets instances leave their wave: the one-stage family if slot
    migration or step-aside scheduling is on, the two-stage family if step-aside scheduling is on.  Each pool's ring has B slots."""
    grid = min(B, grid_cap)
    fit = grid_cap // TEAM_WAVES                       # workgroups the chip holds
    owners = next((k for k in range(1, TEAM_WAVES + 1) if k * fit >= B), TEAM_WAVES)
    if forced:
        owners = forced
    workgroups = min(fit, -(-grid // owners))         # the fewest workgroups whose owners cover the grid, at most what fits
    beyond = B > grid_cap
    leaves = (park_min > 0 or sched_mode > 0) if P == 20 else sched_mode > 0
    return grid, owners, workgroups, int(beyond and bool(use_order)), int(beyond and leaves), B


# one handle per kernel family row: name -> (config, the kernel it must launch, synthetic_batch flags, solver options, resident waves per CU)
FAMILIES = {
    "cfg1": (lambda: named_config("cfg1"), "nmpc_solve_hyb_kernel<ShapeDefault>", {}, {}, 8),
    # cfg1 keeps the default options, the headline path; the other two rows cap the iterations, which keeps their one oracle run under a
    # second and leaves four or five outer iterations (instances leave their wave at outer-iteration boundaries)
    "n17": (lambda: load_config(N_hor=17, Nobs=4, Ndynobs=1), "nmpc_solve_hyb_kernel<ShapeAny>", dict(random_dyn=True),
            dict(max_inner=100, max_outer=5), 8),
    "cfg2": (lambda: named_config("cfg2"), "nmpc_solve_hyb2_kernel<ShapeN40>", {}, dict(max_inner=60, max_outer=4), 4),
}


def family(name):
    """-> (cfg, kernel name, solver / oracle options, resident waves per CU, batch(B, seed))"""
    make, kernel, flags, opts, per_cu = FAMILIES[name]
    cfg = make()
    return cfg, kernel, opts, per_cu, lambda B, seed: harness.synthetic_batch(cfg, 11, B, seed, **flags)


def sweep_sizes(W):
    """the batch sizes on both sides of every launch regime of a handle with W resident waves, G = W / 4 workgroups: one owner up to G,
    two, three and four beyond; order and pools beyond W; the kernel's first-round hold from W + W / 4 on"""
    G = W // 4
    return [1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G, 3 * G + 1, W - 1, W, W + 1, W + 2, W + W // 4 - 1, W + W // 4, W + W // 4 + 1]


SENTINEL = 0xFF                                        # every byte of it: a float64 of these bytes is a NaN, an int32 is -1
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


class Guarded:
    """A device array [B] of rows of ``row_bytes`` bytes with one guard row before row 0 and one after row B - 1, every byte SENTINEL
    (``fill``: the rows' own initial bytes, an array of B rows, e.g. an initial guess)."""

    def __init__(self, B, row_bytes, fill=None):
        import torch
        assert row_bytes % 8 == 0
        self.B, self.row_bytes = B, row_bytes
        self.raw = torch.full(((B + 2) * row_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.rows = self.raw[row_bytes:(B + 1) * row_bytes]
        if fill is not None:
            host = np.ascontiguousarray(fill)
            assert host.nbytes == B * row_bytes
            self.rows.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1)))

    def f64(self):
        """the rows as a float64 tensor [B, row_bytes / 8]"""
        import torch
        return self.rows.view(torch.float64).view(self.B, self.row_bytes // 8)

    def u8(self):
        """the rows as a uint8 tensor [B, row_bytes] (status)"""
        return self.rows.view(self.B, self.row_bytes)

    @property
    def ptr(self):
        return C.c_void_p(self.rows.data_ptr())

    def host(self, dtype=np.float64):
        """(after a synchronisation) -> the rows on the host as ``dtype``; asserts that both guard rows kept their bytes"""
        raw = self.raw.cpu().numpy()
        n = self.row_bytes
        assert (raw[:n] == SENTINEL).all(), "the guard row before row 0 was written"
        assert (raw[-n:] == SENTINEL).all(), f"the guard row after row {self.B - 1} was written"
        body = raw[n:-n].copy()
        if np.dtype(dtype).names:
            return body.view(dtype)
        return body.view(dtype).reshape(self.B, -1)

    def sentinels(self):
        """(after a synchronisation) -> the rows that still hold an 8-byte word of SENTINEL bytes"""
        words = self.raw.cpu().numpy()[self.row_bytes:-self.row_bytes].view(np.uint64).reshape(self.B, -1)
        return np.nonzero((words == ALL_ONES).any(axis=1))[0]


class DeviceSolve:
    """The operands of one nmpc_solve_batch_device launch in device memory, the outputs guarded: u (initial guess ``u0``, zeros by default),
    y_out and status pre-filled with SENTINEL unless not asked for."""

    def __init__(self, solver, B, u0=None, y_out=True, status=True):
        self.s, self.B = solver, B
        self.u = Guarded(B, solver.n_u * 8, fill=np.zeros((B, solver.n_u)) if u0 is None else np.asarray(u0, dtype=np.float64))
        self.y = Guarded(B, solver.n1 * 8) if y_out else None
        self.st = Guarded(B, _lib.STATUS_DTYPE.itemsize) if status else None

    def launch(self, d_p, d_y0=None, d_c0=None, stream=None):
        self.s.solve_device(d_p, self.u.f64(), d_y0, d_c0, None if self.y is None else self.y.f64(), None if self.st is None else self.st.u8(),
                            stream=stream)

    def result(self):
        """(after a synchronisation) -> (u, y or None, status or None); asserts the guard rows, and that no row of an output that was
        asked for still holds the sentinel"""
        u = self.u.host()
        assert self.u.sentinels().size == 0, f"u rows {self.u.sentinels()[:8]} hold the sentinel"
        y = st = None
        if self.y is not None:
            y = self.y.host()
            assert self.y.sentinels().size == 0, f"y_out rows {self.y.sentinels()[:8]} were never written"
        if self.st is not None:
            st = self.st.host(_lib.STATUS_DTYPE).reshape(self.B)
            assert self.st.sentinels().size == 0, f"status rows {self.st.sentinels()[:8]} were never written"
        return u, y, st


def to_device(a):
    """a host array -> a contiguous device tensor, moved by torch"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Delay:
    """A long torch operation on a stream: ``rounds`` products of two n x n float32 matrices.  ``sized_for(ms, stream)`` chooses the rounds so
    that it runs about three times ``ms``; ``measure(stream)`` times it with events, as the solve it is compared with is timed."""

    def __init__(self, n=4096):
        import torch
        self.a = torch.randn(n, n, device="cuda", dtype=torch.float32) * (1.0 / n ** 0.5)
        self.b = self.a.clone()
        self.rounds = 1

    def enqueue(self):
        import torch
        for _ in range(self.rounds):
            self.b = torch.mm(self.a, self.b)

    def measure(self, stream):
        return timed_ms(stream, self.enqueue)

    def sized_for(self, ms, stream):
        self.rounds = 8
        self.measure(stream)                           # (the first products also load the library's kernels)
        per_round = self.measure(stream) / self.rounds
        self.rounds = max(8, int(3.0 * ms / per_round) + 1)
        return self


def timed_ms(stream, enqueue):
    """-> the ms between two events around ``enqueue()`` on ``stream``, which is made current for it; synchronises the stream"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        enqueue()
        e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1)
