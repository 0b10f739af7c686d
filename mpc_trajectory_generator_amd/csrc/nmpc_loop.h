// nmpc_loop.h -- the receding-horizon loop on device: B robots following R routes in lock step.
//
// Counterpart of the body of the reference's `PathGenerator.run` loop (src/path_generator.py:290-403:
// closest reference sample in the sliding window :320-325, horizon padded with the end pose :326-341,
// braking `vel_ref` :343-361, dynamic block rotated left and refreshed :306-316, `last_u` :371-374,
// parameter concatenation :378-379, terminal test :397), of the closed-form obstacle predictor
// (src/visibility/visibility.py:156-166,199-216) and of `MpcModule.run`'s Euler state advance
// (src/mpc/mpc_generator.py:223-235).  One step = assemble p -> batched solve (warm start from the
// previous controls and multipliers) -> advance; nothing crosses PCIe between steps.
//
// Routes: robot b follows routes[route_of[b]]; a route's tables live in one packed table at the offsets of
// its descriptor.  One route (nmpc_loop_new) is the case R = 1 of the same kernels.
//
// Arithmetic: index selections (window arg-min, vertex window, braking-table filter) use the same
// unfused IEEE operations as the host mirror (`trajectory.VectorizedRecedingHorizon`), so they are
// bit-identical to it; sin / cos are the kernels' own sincos_cw (the mirror takes it as a hook).  What several kernels must compute
// operation for operation is one function: the geometry that the host shares in nmpc_geom.h (included before this file), the rest here.
//
// Retirement (nmpc_loop_set_retire; the rule is DESIGN.md section 5.9): a robot whose terminal test holds after an advance leaves the
// loop for good, as the reference's `while not terminal` ends.  The kernels of a step then run over the list of the robots still
// active, `act[0 .. nact)` (ascending robot index; NULL = everybody, row i is robot i): the same arithmetic on the same per-robot
// arrays through one more indirection.  nmpc_loop_compact_kernel rebuilds the list after every advance, and a gather / scatter pair
// moves the active robots' rows through contiguous buffers, so that the solve sees a batch of nact instances and nothing else.
// The host sizes a step's launches by nact, which it learns one step late: the count is copied to pinned memory behind an event, and
// the next nmpc_loop_step waits for THAT event (not for the device: a loop on another stream keeps running).  This coupling of the
// host to the step before exists only with retirement on; without it a step enqueues what it always did and waits for nothing.
//
// Arguments: every kernel takes (LoopView, LoopStep, the arguments of its stage), or fewer where it needs fewer.  LoopView is what the
// loop is -- its shape, its per-robot arrays, its active list -- fixed once the loop is configured and the same for every kernel;
// LoopStep is what changes from step to step, all of it derived from the step count and the active count.  A stage's struct holds
// what is the stage's own and nothing of those two.  The one place where two kernels of a step see different views: with a plant that
// measures (nmpc_loop_set_plant, meas > 0) the assembly and nmpc_loop_predict_kernel get a copy of the view whose `state` is the measured
// poses, built by nmpc_loop_step on its stack; every other kernel of the step keeps the true `state`.
#pragma once

namespace nmpc {

constexpr int LOOP_NONE = 0x7fffffff;       // no candidate, no row, no polygon: the index behind every real one

struct LoopView {
    int B, N, nobs, ndyn, K, n_p, n_u, n1, s;
    double ts;
    double *state;            // [B][3]
    double *last_u;           // [B][2]
    int *idx;                 // [B]
    unsigned char *done;      // [B]
    double *P, *U, *Y;        // [B][n_p], [B][n_u], [B][n1]
    nmpc_status *st;          // [B]
    const int *route_of;      // [B] (written by nmpc_loop_dispatch_kernel, through its own pointer, and by nobody else)
    double *traj;             // [(steps * s + 1)][B][3] or NULL
    const int *act;           // the robots a step runs over, ascending; NULL: all B (no retirement), row i is robot i

    __device__ int robot(int i) const { return act ? act[i] : i; }
    __device__ double *row(int r, int b) const { return traj + ((size_t)r * B + b) * 3; }      // trajectory row r of robot b
    // where the blocks of a parameter vector start: head [NZ] | vel_ref [N] | circles [nobs][3] | ellipses [ndyn][N][5] | references [N][3]
    __device__ int p_vel() const { return NZ; }
    __device__ int p_circ() const { return NZ + N; }
    __device__ int p_dyn() const { return NZ + N + 3 * nobs; }
    __device__ int p_ref() const { return NZ + N + 3 * nobs + 5 * ndyn * N; }
};

struct LoopStep {
    int t;                    // controls applied before this step
    int traj_row;             // the first of this step's s trajectory rows (>= 1: row 0 is the start)
    int step;                 // steps taken, this one included: what retired_at and leg_at take
    int nact;                 // the robots this step runs over (B without retirement)
    int cur;                  // which of the two carried dynamic blocks is read; the other is written

    // the step that follows `steps` others of s controls each, over n robots
    static LoopStep after(int steps, int s, int n) { return {steps * s, steps * s + 1, steps + 1, n, steps & 1}; }
};

// one route: where its tables sit in AssembleArgs::tab (in doubles) and its constants (nmpc_route)
struct LoopRoute {
    int xr, yr, thr, vert, bv, bd;          // x_ref | y_ref | theta_ref [n_ref], vertices [n_vert][2], brake vel / dist [n_brake]
    int n_ref, n_vert, n_brake;
    double end[3];
    double base, radius, pad;
    double w[10];
};

struct AssembleArgs {         // (the advance reads a route's goal pose through it)
    const double *tab;        // every route's tables, packed
    const LoopRoute *routes;  // [R]
    const double *dynpar;     // [B][K][10]: p1x p1y p2x p2y freq rx ry angle | sinusoidal law (0 / 1) | atan2(p2 - p1)
    double *dyn[2];           // [B][ndyn][N][5]: the carried dynamic block, read and written in turn
};

// thread t of a workgroup owns the entries [lo, hi) of n: chunks of ceil(n / threads), the last ones short or empty
__device__ __forceinline__ void block_chunk(int n, int &lo, int &hi)
{
    const int t = threadIdx.x, nt = blockDim.x;
    const int chunk = (n + nt - 1) / nt;
    lo = t * chunk < n ? t * chunk : n;
    hi = lo + chunk < n ? lo + chunk : n;
}

// inclusive scan over the workgroup's threads of one value each, through cnt [threads] in LDS; the last thread's result is the total
__device__ __forceinline__ int block_scan(int *cnt, int c)
{
    const int t = threadIdx.x, nt = blockDim.x;
    cnt[t] = c;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {
        const int v = t >= off ? cnt[t - off] : 0;
        __syncthreads();
        cnt[t] += v;
        __syncthreads();
    }
    return cnt[t];
}

// (d, j) lexicographic minimum over the wave, result in every lane: the FIRST minimal index, like np.argmin
__device__ __forceinline__ void wave_argmin(double &d, int &j)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(d, off);
        const int oj = __shfl_xor(j, off);
        if (od < d || (od == d && oj < j)) { d = od; j = oj; }
    }
}

// (v, r, j) lexicographic minimum over the wave, result in every lane
__device__ __forceinline__ void wave_argmin3(double &d, int &r, int &j)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double od = __shfl_xor(d, off);
        const int orow = __shfl_xor(r, off);
        const int oj = __shfl_xor(j, off);
        if (od < d || (od == d && (orow < r || (orow == r && oj < j)))) { d = od; r = orow; j = oj; }
    }
}

// minimum / maximum over the wave, result in every lane (the order of the reduction does not show)
template <class T>
__device__ __forceinline__ T wave_min(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

template <class T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const T o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// What the one-wave-per-robot kernels stage in `own` (LDS), barrier included.
// Robot b's N predicted positions, own[2 k] = x, own[2 k + 1] = y of stage k; each(x, y) sees every position its lane loads.
template <class Each>
__device__ __forceinline__ void stage_pred(double *own, const double *pred, int b, int N, Each each)
{
    for (int k = threadIdx.x; k < N; k += 64) {
        const double x = pred[((size_t)b * N + k) * 3], y = pred[((size_t)b * N + k) * 3 + 1];
        own[2 * k] = x;
        own[2 * k + 1] = y;
        each(x, y);
    }
    __syncthreads();
}

__device__ __forceinline__ void stage_pred(double *own, const double *pred, int b, int N)
{
    stage_pred(own, pred, b, N, [](double, double) {});
}

// the first C components of robot b's trajectory rows row0 .. row0 + n - 1, own[C i + c] = component c of row row0 + i
template <int C>
__device__ __forceinline__ void stage_rows(double *own, const LoopView &L, int b, int row0, int n)
{
    for (int i = threadIdx.x; i < n; i += 64) {
        const double *row = L.row(row0 + i, b);
#pragma unroll
        for (int c = 0; c < C; ++c) own[C * i + c] = row[c];
    }
    __syncthreads();
}

// One Euler step of the unicycle under the control (v, w) (mpc_generator.py:225-235): the advance's, the predictions' and the plant's.
__device__ __forceinline__ void unicycle_step(double &x, double &y, double &th, double v, double w, double ts)
{
    double sn, cs;
    sincos_cw(th, sn, cs);
    x = x + ts * (v * cs);
    y = y + ts * (v * sn);
    th = th + ts * w;
}

// the level of the ellipse q = (x, y, rx, ry, theta) at the position (x, y): the cost's (a/rx)^2 + (c/ry)^2, below 1 inside
__device__ __forceinline__ double ellipse_level(double x, double y, const double *q)
{
    const double dx = x - q[0], dy = y - q[1];
    double sn, cs;
    sincos_cw(q[4], sn, cs);
    const double al = dx * cs + dy * sn, ac = dx * sn - dy * cs;
    return (al * al) / (q[2] * q[2]) + (ac * ac) / (q[3] * q[3]);
}

// times = numpy.linspace(t0, t0 + H * ts, H)[i]   (visibility.py:204)
__device__ __forceinline__ double linspace_at(double t0, double ts, int H, int i)
{
    const double stop = t0 + (double)H * ts;
    if (H == 1) return t0;
    if (i == H - 1) return stop;
    const double step = (stop - t0) / (double)(H - 1);
    return (double)i * step + t0;
}

// Field f of stage st of a scripted ellipse q [10] (AssembleArgs::dynpar) where the step computes it anew: every stage at t == 0, the
// last s stages afterwards (visibility.py:156-166,199-216).  The assembly's carried block and the crowd's table share it.
__device__ __forceinline__ double ellipse_fresh(const double *q, double pad, int f, int st, int t, int N, int s, double ts)
{
    if (f >= 2) return f == 2 ? q[5] + pad : (f == 3 ? q[6] + pad : q[7]);
    const int H = t == 0 ? N : s, i = t == 0 ? st : st - (N - s);
    const double t0 = t == 0 ? 0.0 : (double)(t + N - s) * ts;
    const double tm = linspace_at(t0, ts, H, i);
    double sn, cs;
    sincos_cw(q[4] * tm, sn, cs);
    const double w = fabs(sn);
    double v = w * q[f] + (1.0 - w) * q[2 + f];
    if (q[8] != 0.0) {
        // sinusoidal law (visibility.py:177-196): offset across the p1 -> p2 line, amplitude 1.5
        const double p3x = w * q[0] + (1.0 - w) * q[2], p3y = w * q[1] + (1.0 - w) * q[3];
        double s10, c10, sa_, ca_;
        sincos_cw((10.0 * q[4]) * tm, s10, c10);
        sincos_cw(q[9], sa_, ca_);
        const double add = 1.5 * c10;
        const double dx = p3x - q[0], dy = p3y - q[1];
        const double rx = ca_ * dx - sa_ * dy;
        double ry = sa_ * dx + ca_ * dy;
        ry = ry + add;
        const double qx = ca_ * rx - (-sa_) * ry, qy = (-sa_) * rx + ca_ * ry;      // rotate back by -angle
        v = f == 0 ? qx + q[0] : qy + q[1];
    }
    return v;
}

// one wave per robot: fills p[b] and the rotated dynamic block
__global__ __launch_bounds__(64) void nmpc_loop_assemble_kernel(LoopView L, LoopStep stp, AssembleArgs g)
{
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    // the robot's route: the same for the whole wave (read before any store, so that the loads can be scalar)
    const LoopRoute &rt = g.routes[L.route_of[b]];
    const double *xr = g.tab + rt.xr, *yr = g.tab + rt.yr, *thr = g.tab + rt.thr, *vert = g.tab + rt.vert;
    const double *bv = g.tab + rt.bv, *bd = g.tab + rt.bd;
    const int N = L.N, n = rt.n_ref, s = L.s, t = stp.t, n_vert = rt.n_vert, n_brake = rt.n_brake;
    const double base = rt.base, radius = rt.radius, pad = rt.pad, ex = rt.end[0], ey = rt.end[1], eth = rt.end[2];
    const double x = L.state[3 * b], y = L.state[3 * b + 1], th = L.state[3 * b + 2];
    double *p = L.P + (size_t)b * L.n_p;

    // ---- static circles (path_generator.py:295-304 + visibility.py:141-148, look-back 0)
    {
        double *pc = p + L.p_circ();
        const int nv = n_vert;
        int lb = 0, ub = nv;
        if (nv > L.nobs) {
            double best = __builtin_inf();
            int bj = LOOP_NONE;
            for (int j = lane; j < nv; j += 64) {
                const double dx = vert[2 * j] - x, dy = vert[2 * j + 1] - y;
                double d = sqrt(dx * dx + dy * dy);
                if (d != d) d = -__builtin_inf();
                if (d < best) { best = d; bj = j; }
            }
            wave_argmin(best, bj);
            lb = bj;
            ub = L.nobs;          // (sic: the reference's window is [lb, min(nv, Nobs)) )
        }
        for (int k = lane; k < L.nobs; k += 64) {
            const int j = lb + k;
            const bool ok = nv > 0 && j < ub;
            const int jj = j < nv ? j : (nv > 0 ? nv - 1 : 0);
            pc[3 * k] = ok ? vert[2 * jj] : 0.0;
            pc[3 * k + 1] = ok ? vert[2 * jj + 1] : 0.0;
            pc[3 * k + 2] = ok ? radius : 0.0;
        }
    }
    // ---- dynamic ellipses (path_generator.py:306-316; visibility.py:156-166,199-216)
    {
        const int per = N * 5, tot = L.ndyn * per;
        const double *din = g.dyn[stp.cur] + (size_t)b * tot;
        double *dout = g.dyn[stp.cur ^ 1] + (size_t)b * tot;
        double *pd = p + L.p_dyn();
        for (int e = lane; e < tot; e += 64) {
            const int k = e / per, r = e - k * per, st = r / 5, f = r - st * 5;
            double v;
            const bool fresh = k < L.K && (t == 0 || st >= N - s);
            if (fresh) {
                v = ellipse_fresh(g.dynpar + ((size_t)b * L.K + k) * 10, pad, f, st, t, N, s, L.ts);
            } else if (t == 0) {
                v = din[e];                                    // padding block as initialised
            } else {
                // the reference rotates the WHOLE flat list left by 5 s entries (path_generator.py:312): a shift by s
                // stages inside a block, and a block's last s stages take the next block's first s (the last block's
                // take block 0's, so a padding slot can inherit stale ellipses of obstacle 0 when 0 < K < Ndynobs)
                const int src = e + 5 * s;
                v = din[src < tot ? src : src - tot];
            }
            dout[e] = v;
            pd[e] = v;
        }
    }
    // ---- closest reference sample in the sliding window (:320-325)
    int idx;
    {
        const int i0 = L.idx[b];
        const int lb = i0 - s > 0 ? i0 - s : 0, ub = i0 + 5 * s < n ? i0 + 5 * s : n;
        double best = __builtin_inf();
        int bj = LOOP_NONE;
        for (int j = lb + lane; j < ub; j += 64) {
            const double dx = xr[j] - x, dy = yr[j] - y;
            double d = sqrt(dx * dx + dy * dy);
            if (d != d) d = -__builtin_inf();
            if (d < best) { best = d; bj = j; }
        }
        wave_argmin(best, bj);
        idx = bj;
        if (lane == 0) L.idx[b] = idx;
    }
    // ---- head: state, last_u, target, last_u again, weights (:378-379)
    {
        const bool far = idx + N < n;
        const int jf = far ? idx + N : n - 1;
        if (lane < 3) p[lane] = lane == 0 ? x : (lane == 1 ? y : th);
        if (lane >= 3 && lane < 5) p[lane] = L.last_u[2 * b + lane - 3];
        if (lane >= 5 && lane < 8) {
            const int f = lane - 5;
            p[lane] = far ? (f == 0 ? xr[jf] : (f == 1 ? yr[jf] : thr[jf])) : (f == 0 ? ex : (f == 1 ? ey : eth));
        }
        if (lane >= 8 && lane < 10) p[lane] = L.last_u[2 * b + lane - 8];
        if (lane >= 10 && lane < 20) p[lane] = rt.w[lane - 10];
    }
    // ---- horizon references (:326-341) and velocity reference with the braking profile (:343-361)
    {
        double *pv = p + L.p_vel(), *pr = p + L.p_ref();
        const bool brake = (double)(idx + N) >= (double)n - bd[0] / base;
        const int nbase = n - idx - 1 < N ? n - idx - 1 : N;
        const double ddx = x - ex, ddy = y - ey;
        const double dist_to_goal = sqrt(ddx * ddx + ddy * ddy);
        for (int k = lane; k < N; k += 64) {
            const int j = idx + k;
            const bool ok = j < n;
            const int jj = ok ? j : n - 1;
            pr[3 * k] = ok ? xr[jj] : ex;
            pr[3 * k + 1] = ok ? yr[jj] : ey;
            pr[3 * k + 2] = ok ? thr[jj] : eth;
            double v = base;
            if (brake) {
                if (nbase == 0) {
                    // inside the last sample: the k-th braking entry whose distance is within reach (:347-351)
                    v = 0.0;
                    int cnt = 0;
                    for (int i = 0; i < n_brake; ++i) {
                        if (bd[i] <= dist_to_goal) {
                            if (cnt == k) { v = bv[i]; break; }
                            ++cnt;
                        }
                    }
                } else if (k >= nbase) {
                    v = k - nbase < n_brake ? bv[k - nbase] : 0.0;
                }
            }
            pv[k] = v;
        }
    }
}

// the terminal test (path_generator.py:397): within GOAL_POS_TOL of the goal on both axes, the last commanded speed below GOAL_VEL_TOL
constexpr double GOAL_POS_TOL = 0.05, GOAL_VEL_TOL = 0.005;

// the pose after a control into the robot's trajectory row r, if the loop keeps a trajectory
__device__ __forceinline__ void drive_row(const LoopView &L, int r, int b, double x, double y, double th)
{
    if (L.traj) {
        double *row = L.row(r, b);
        row[0] = x; row[1] = y; row[2] = th;
    }
}

// the end of a drive over the controls u: the true pose into `state`, the last COMMANDED control into last_u, the terminal test on both
__device__ __forceinline__ void drive_end(const LoopView &L, const AssembleArgs &g, int b, const double *u, double x, double y, double th)
{
    L.state[3 * b] = x; L.state[3 * b + 1] = y; L.state[3 * b + 2] = th;
    const double lv = u[2 * (L.s - 1)], lw = u[2 * (L.s - 1) + 1];
    L.last_u[2 * b] = lv; L.last_u[2 * b + 1] = lw;
    const double *end = g.routes[L.route_of[b]].end;
    L.done[b] = (fabs(x - end[0]) <= GOAL_POS_TOL && fabs(y - end[1]) <= GOAL_POS_TOL && fabs(lv) < GOAL_VEL_TOL) ? 1 : 0;
}

// one thread per robot: Euler advance over the steps taken (mpc_generator.py:225-235), terminal test (:397)
__global__ void nmpc_loop_advance_kernel(LoopView L, LoopStep stp, AssembleArgs g)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stp.nact) return;
    const int b = L.robot(i);
    const double *u = L.U + (size_t)b * L.n_u;
    double x = L.state[3 * b], y = L.state[3 * b + 1], th = L.state[3 * b + 2];
    for (int i = 0; i < L.s; ++i) {
        unicycle_step(x, y, th, u[2 * i], u[2 * i + 1], L.ts);
        drive_row(L, stp.traj_row + i, b, x, y, th);
    }
    drive_end(L, g, b, u, x, y, th);
}

// ---- peers: the robots of a group see each other (nmpc_loop_set_peers; the rule is DESIGN.md section 5.9) ----
// Two kernels between the assembly and the solve: every robot's predicted poses over the horizon, then per robot the M closest
// peers of its group written into the ellipse slots [first, first + M) of p, first = K + the crowd's slots.  The carried block
// (dyn_in / dyn_out) never sees them.
struct GroupLists {          // the groups 0 .. B - 1 (most of them empty)
    const int *group_of;      // [B]
    const int *goff;          // [groups + 1]: a group's members are gmem[goff[g] .. goff[g + 1])
    const int *gmem;          // [B], ascending robot index inside a group
};

struct PeerArgs {
    int M, first;             // the peers' ellipse slots: [first, first + M)
    double rx, ry, range2;
    double *pred;             // [B][N][3]: the loop's predicted poses (nmpc_loop_predict_kernel)
    GroupLists grp;
};

// one thread per robot: pred[b][k] = the pose after k + 1 Euler steps (unicycle_step, as nmpc_loop_advance_kernel takes them) under the
// previous plan shifted by the s controls already applied, its last control held beyond the plan's end
// (a retired robot's row is not computed here: nmpc_loop_compact_kernel parked it)
__global__ void nmpc_loop_predict_kernel(LoopView L, LoopStep stp, double *pred)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stp.nact) return;
    const int b = L.robot(i);
    const double *u = L.U + (size_t)b * L.n_u;      // the previous plan
    double *out = pred + (size_t)b * L.N * 3;
    double x = L.state[3 * b], y = L.state[3 * b + 1], th = L.state[3 * b + 2];
    for (int k = 0; k < L.N; ++k) {
        const int c = L.s + k < L.N ? L.s + k : L.N - 1;
        unicycle_step(x, y, th, u[2 * c], u[2 * c + 1], L.ts);
        out[3 * k] = x; out[3 * k + 1] = y; out[3 * k + 2] = th;
    }
}

// What the peers kernels and the crowd's share: a lane's list of its best NDYN_MAX candidates, sorted by (D, j) and held in registers
// (static indices); no candidate = (inf, LOOP_NONE), behind every real one

// D(b, j) = min_k |pred[b][k] - pj[k]|^2, b's positions in `own` (LDS), j's positions stage by stage in `pj`, `stride` doubles apart
// (3: a row of pred, 5: a row of the crowd's table)
__device__ __forceinline__ double peer_closeness(const double *own, const double *pj, int N, int stride)
{
    double D = __builtin_inf();
    for (int k = 0; k < N; ++k) {
        const double dx = own[2 * k] - pj[stride * k], dy = own[2 * k + 1] - pj[stride * k + 1];
        const double d = dx * dx + dy * dy;
        if (d < D) D = d;
    }
    return D;
}

// the list without a candidate
__device__ __forceinline__ void peer_none(double (&bd)[NDYN_MAX], int (&bj)[NDYN_MAX])
{
#pragma unroll
    for (int q = 0; q < NDYN_MAX; ++q) { bd[q] = __builtin_inf(); bj[q] = LOOP_NONE; }
}

// candidate (cd, cj) into the lane's sorted list
__device__ __forceinline__ void peer_keep(double (&bd)[NDYN_MAX], int (&bj)[NDYN_MAX], double cd, int cj)
{
#pragma unroll
    for (int q = 0; q < NDYN_MAX; ++q) {
        if (cd < bd[q] || (cd == bd[q] && cj < bj[q])) {
            const double td = bd[q]; const int tj = bj[q];
            bd[q] = cd; bj[q] = cj;
            cd = td; cj = tj;
        }
    }
}

// M rounds: the wave's (D, j) minimum over the lanes' heads, written over ellipse slot first + m of p[b]; the lane that held it moves
// on to its next.  entry(j, e) = entry e of candidate j's ellipse row [N][5]; seen [M] (NULL: nobody asks) gets j, or -1 where no
// candidate was left
template <class Entry>
__device__ __forceinline__ void peer_overlay(const LoopView &L, int b, int lane, double (&bd)[NDYN_MAX], int (&bj)[NDYN_MAX], int first, int M,
                                             int *seen, Entry entry)
{
    double *pd = L.P + (size_t)b * L.n_p + L.p_dyn();
    const int per = 5 * L.N;
    int m = 0;
    for (; m < M; ++m) {
        double d = bd[0];
        int j = bj[0];
        wave_argmin(d, j);
        if (j == LOOP_NONE) break;            // (wave-uniform) no candidate left: the remaining slots keep what they hold
        if (bj[0] == j) {
#pragma unroll
            for (int q = 0; q + 1 < NDYN_MAX; ++q) { bd[q] = bd[q + 1]; bj[q] = bj[q + 1]; }
            bd[NDYN_MAX - 1] = __builtin_inf(); bj[NDYN_MAX - 1] = LOOP_NONE;
        }
        double *slot = pd + (size_t)(first + m) * per;
        for (int e = lane; e < per; e += 64) slot[e] = entry(j, e);
        if (seen && lane == 0) seen[m] = j;
    }
    if (seen) for (int q = m + lane; q < M; q += 64) seen[q] = -1;
}

// a peer's ellipse row: its predicted poses as (x, y, rx, ry, theta)
__device__ __forceinline__ void peers_overlay(const LoopView &L, const PeerArgs &a, int b, int lane, double (&bd)[NDYN_MAX], int (&bj)[NDYN_MAX])
{
    const int N = L.N;
    peer_overlay(L, b, lane, bd, bj, a.first, a.M, nullptr, [&](int j, int e) {
        const double *pj = a.pred + (size_t)j * N * 3;
        const int st = e / 5, f = e - st * 5;
        return f == 0 ? pj[3 * st] : (f == 1 ? pj[3 * st + 1] : (f == 2 ? a.rx : (f == 3 ? a.ry : pj[3 * st + 2])));
    });
}

// one wave per robot: D(b, j) = min_k |pred[b][k] - pred[j][k]|^2 over the members j != b of b's group (lanes stride over them),
// the first M of the candidates D < range^2 in (D, j) order, each written over one ellipse slot of p[b]
__global__ __launch_bounds__(64) void nmpc_loop_peers_kernel(LoopView L, PeerArgs a)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int N = L.N;
    // the group's member range: the same for the whole wave
    const int g = a.grp.group_of[b];
    const int lo = a.grp.goff[g], hi = a.grp.goff[g + 1];
    stage_pred(own, a.pred, b, N);
    double bd[NDYN_MAX];
    int bj[NDYN_MAX];
    peer_none(bd, bj);
    for (int i = lo + lane; i < hi; i += 64) {
        const int j = a.grp.gmem[i];
        const double D = peer_closeness(own, a.pred + (size_t)j * N * 3, N, 3);
        if (j != b && D < a.range2) peer_keep(bd, bj, D, j);
    }
    peers_overlay(L, a, b, lane, bd, bj);
}

// ---- peers through a grid (nmpc_loop_set_peers_grid; the rule, and why it misses nobody: DESIGN.md section 5.9) ----
// The same selection over fewer candidates.  Three kernels take the place of nmpc_loop_peers_kernel: every robot's box over its
// predicted positions, a uniform grid in which each robot is filed once, under the cell of its box's lower corner, and per robot the
// rule of the all-pairs kernel over the robots filed in the cells its range can reach.
constexpr int PEER_GRID_CAP = 128;      // cells per axis at the most: 16 384 cells, two per robot of the largest fleet run (8192)

struct PeerGridArgs {
    double range, cell;
    double *box;              // [B][4]: lo.x, lo.y, hi.x, hi.y over the finite stages; (inf, inf, -inf, -inf) = unfiled
    nmpc_peer_grid *hdr;      // [1]: this step's grid
    int *cell_of;             // [B]: the robot's cell (row-major, y * nx + x), -1 = unfiled
    int *cell_off;            // [CAP * CAP + 1]: cell c holds cell_mem[cell_off[c] .. cell_off[c + 1])
    int *cell_cur;            // [CAP * CAP]: the scatter's cursors
    int *cell_mem;            // [B]
};

// (the cell of a coordinate and the rule for an axis, over the extent of the lower corners: cellof and grid_axis of nmpc_geom.h)

// a box's extent rounded up: never below the real hi - lo
__device__ __forceinline__ double peer_extent_up(double hi, double lo)
{
    const double w = hi - lo;
    return w < __builtin_inf() ? __longlong_as_double(__double_as_longlong(w) + 1) : w;
}

// one thread per robot, all B (a retired robot stands parked in pred): the box of its predicted positions
__global__ void nmpc_loop_peer_box_kernel(LoopView L, PeerArgs a, PeerGridArgs g)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= L.B) return;
    const double *p = a.pred + (size_t)b * L.N * 3;
    const double inf = __builtin_inf();
    double lx = inf, ly = inf, hx = -inf, hy = -inf;
    for (int k = 0; k < L.N; ++k) box_fold(p[3 * k], p[3 * k + 1], lx, ly, hx, hy);
    double *out = g.box + 4 * (size_t)b;
    out[0] = lx; out[1] = ly; out[2] = hx; out[3] = hy;
}

// One workgroup, thread t over its chunk of the robots (block_chunk) as in nmpc_loop_compact_kernel: the grid's header (minima and
// maxima: the order of a reduction does not show), every robot's cell, the cells' populations counted with integer atomics in global
// memory (cell_off: 64 KB at CAP = 128, more than a workgroup's static LDS), their exclusive scan, and the scatter into cell_mem.
// The order inside a cell is the atomics' and differs from run to run; no result depends on it.  Stores, atomics and loads of the
// same words are ordered by the device-scope fences in front of the barriers.
__global__ __launch_bounds__(1024) void nmpc_loop_peer_grid_kernel(LoopView L, PeerGridArgs g)
{
    __shared__ double red[16][6];
    __shared__ int redn[16];
    __shared__ int cnt[1024];
    const int t = threadIdx.x, nt = blockDim.x;
    int lo, hi;
    block_chunk(L.B, lo, hi);
    const double inf = __builtin_inf();
    double v[6] = {inf, inf, -inf, -inf, 0.0, 0.0};       // min lo.x, min lo.y, max lo.x, max lo.y, max extent x, max extent y
    int nf = 0;
    for (int b = lo; b < hi; ++b) {
        const double *bx = g.box + 4 * (size_t)b;
        if (bx[0] <= bx[2]) {
            const double wx = peer_extent_up(bx[2], bx[0]), wy = peer_extent_up(bx[3], bx[1]);
            v[0] = bx[0] < v[0] ? bx[0] : v[0]; v[1] = bx[1] < v[1] ? bx[1] : v[1];
            v[2] = bx[0] > v[2] ? bx[0] : v[2]; v[3] = bx[1] > v[3] ? bx[1] : v[3];
            v[4] = wx > v[4] ? wx : v[4]; v[5] = wy > v[5] ? wy : v[5];
            ++nf;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = q < 2 ? wave_min(v[q]) : wave_max(v[q]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nf += __shfl_xor(nf, off);
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) red[t >> 6][q] = v[q];
        redn[t >> 6] = nf;
    }
    __syncthreads();
    nf = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = q < 2 ? inf : (q < 4 ? -inf : 0.0);
    for (int w = 0; w < nt / 64; ++w) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double o = red[w][q];
            v[q] = q < 2 ? (o < v[q] ? o : v[q]) : (o > v[q] ? o : v[q]);
        }
        nf += redn[w];
    }
    // the grid: the same in every thread
    int nx = 1, ny = 1;
    double hx = g.cell, hy = g.cell;
    if (nf == 0) { v[0] = 0.0; v[1] = 0.0; }
    else {
        grid_axis(v[2] - v[0], g.cell, PEER_GRID_CAP, nx, hx);
        grid_axis(v[3] - v[1], g.cell, PEER_GRID_CAP, ny, hy);
    }
    const int cells = nx * ny;
    if (t == 0) {
        nmpc_peer_grid *h = g.hdr;
        h->origin[0] = v[0]; h->origin[1] = v[1]; h->h[0] = hx; h->h[1] = hy; h->W[0] = v[4]; h->W[1] = v[5];
        h->nx = nx; h->ny = ny; h->filed = nf; h->reserved = 0;
    }
    for (int c = t; c <= cells; c += nt) g.cell_off[c] = 0;
    __threadfence();
    __syncthreads();
    for (int b = lo; b < hi; ++b) {
        const double *bx = g.box + 4 * (size_t)b;
        int c = -1;
        if (bx[0] <= bx[2]) {
            c = cellof(bx[1], v[1], hy, ny) * nx + cellof(bx[0], v[0], hx, nx);
            atomicAdd(g.cell_off + c, 1);
        }
        g.cell_of[b] = c;
    }
    __threadfence();
    __syncthreads();
    // exclusive scan of the populations: thread t over its chunk of the entries, the one behind the last cell included
    int clo, chi;
    block_chunk(cells + 1, clo, chi);
    int sum = 0;
    for (int c = clo; c < chi; ++c) sum += g.cell_off[c];
    int run = block_scan(cnt, sum) - sum;
    for (int c = clo; c < chi; ++c) {
        const int n = g.cell_off[c];
        g.cell_off[c] = run;
        if (c < cells) g.cell_cur[c] = run;
        run += n;
    }
    __threadfence();
    __syncthreads();
    for (int b = lo; b < hi; ++b) {
        const int c = g.cell_of[b];                     // (the thread's own store above)
        if (c >= 0) g.cell_mem[atomicAdd(g.cell_cur + c, 1)] = b;
    }
}

// one wave per active robot: the rule of nmpc_loop_peers_kernel over the robots filed in the cells of b's window, row after row (a
// row's cells cx0 .. cx1 are one range of cell_mem, and the lanes stride over it).  Every loop's bounds are read before it starts.
__global__ __launch_bounds__(64) void nmpc_loop_peers_grid_kernel(LoopView L, PeerArgs a, PeerGridArgs g)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int N = L.N;
    stage_pred(own, a.pred, b, N);
    double bd[NDYN_MAX];
    int bj[NDYN_MAX];
    peer_none(bd, bj);
    // the box, the grid and the window: the same for the whole wave
    const double *bx = g.box + 4 * (size_t)b;
    const nmpc_peer_grid *h = g.hdr;
    if (bx[0] <= bx[2]) {                               // an unfiled robot finds nobody
        const int nx = h->nx, ny = h->ny, grp = a.grp.group_of[b];
        const int cx0 = cellof((bx[0] - g.range) - h->W[0], h->origin[0], h->h[0], nx);
        const int cy0 = cellof((bx[1] - g.range) - h->W[1], h->origin[1], h->h[1], ny);
        const int cx1 = cellof(bx[2] + g.range, h->origin[0], h->h[0], nx);
        const int cy1 = cellof(bx[3] + g.range, h->origin[1], h->h[1], ny);
        for (int row = cy0; row <= cy1; ++row) {
            const int i0 = g.cell_off[row * nx + cx0], i1 = g.cell_off[row * nx + cx1 + 1];
            for (int i = i0 + lane; i < i1; i += 64) {
                const int j = g.cell_mem[i];
                if (j != b && a.grp.group_of[j] == grp) {
                    const double D = peer_closeness(own, a.pred + (size_t)j * N * 3, N, 3);
                    if (D < a.range2) peer_keep(bd, bj, D, j);
                }
            }
        }
    }
    peers_overlay(L, a, b, lane, bd, bj);
}

// ---- crowd: D moving obstacles of the world, shared by the fleet (nmpc_loop_set_crowd; the rule is DESIGN.md section 5.9) ----
// One table of every obstacle's ellipses over the horizon, advanced once per step whoever is active; between the assembly and the solve
// each active robot's M closest obstacles are written into the ellipse slots [K, K + M) of p.  The carried block never sees them.  An
// optional observer keeps each robot's closest approach to any obstacle of the crowd.
struct CrowdArgs {
    int D, M;
    double pad, range2;
    const double *obst;       // [D][10]: the fields of AssembleArgs::dynpar
    double *tab[2];           // [D][N][5]: read and written in turn with LoopStep::cur, as AssembleArgs::dyn
    const double *pred;       // [B][N][3]: the loop's predicted poses (nmpc_loop_predict_kernel)
    int *seen;                // [B][M]: the obstacle in slot K + m of p[b], -1 = none
    nmpc_crowd_clearance *rec;    // [B], NULL without the observer
};

// One thread per entry (d, stage, field) of the table: what the assembly does to a scripted slot, obstacle by obstacle.  A stage that is
// not fresh takes stage st + s of the SAME obstacle (st + s < N): the assembly's flat rotation carries a neighbour's stages only into
// stages that a scripted obstacle then refreshes.
__global__ __launch_bounds__(256) void nmpc_loop_crowd_advance_kernel(LoopView L, LoopStep stp, CrowdArgs c)
{
    const int per = L.N * 5, tot = c.D * per;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tot) return;
    const int d = e / per, r = e - d * per, st = r / 5, f = r - st * 5;
    const bool fresh = stp.t == 0 || st >= L.N - L.s;
    c.tab[stp.cur ^ 1][e] = fresh ? ellipse_fresh(c.obst + (size_t)d * 10, c.pad, f, st, stp.t, L.N, L.s, L.ts) : c.tab[stp.cur][e + 5 * L.s];
}

// one wave per active robot: C(b, d) = min_k |pred[b][k] - tab[d][k]|^2 over the table as this step wrote it (lanes stride over d, each
// reading its obstacle's row through the cache), the first M of the candidates C < range^2 in (C, d) order, each obstacle's row copied
// over one ellipse slot of p[b].  No loop's bounds depend on the table's values.
__global__ __launch_bounds__(64) void nmpc_loop_crowd_kernel(LoopView L, LoopStep stp, CrowdArgs c)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int N = L.N, per = 5 * N;
    const double *tab = c.tab[stp.cur ^ 1];
    stage_pred(own, c.pred, b, N);
    double bd[NDYN_MAX];
    int bj[NDYN_MAX];
    peer_none(bd, bj);
    for (int d = lane; d < c.D; d += 64) {
        const double C = peer_closeness(own, tab + (size_t)d * per, N, 5);
        if (C < c.range2) peer_keep(bd, bj, C, d);
    }
    peer_overlay(L, b, lane, bd, bj, L.K, c.M, c.seen + (size_t)b * c.M, [&](int d, int e) { return tab[(size_t)d * per + e]; });
}

// One wave per robot the step drove, after the advance: the robot's s new poses go to LDS; row by row, lanes stride over ALL D obstacles,
// the pose of row traj_row + i against entry i of the obstacle's row of this step's table (the pairing of nmpc_loop_monitor_kernel's
// scripted ellipses, and its level).  A lane's rows and obstacles ascend, so among equal values its first stays; one wave reduction, and
// lane 0 folds the lexicographic minimum of (level, row, d) into the record.  It observes: the record is the only thing it writes.
__global__ __launch_bounds__(64) void nmpc_loop_crowd_monitor_kernel(LoopView L, LoopStep stp, CrowdArgs c)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int s = L.s, N = L.N, row0 = stp.traj_row;
    const double *tab = c.tab[stp.cur ^ 1];
    stage_rows<2>(own, L, b, row0, s);
    double bv = __builtin_inf();
    int br = LOOP_NONE, bo = LOOP_NONE;
    for (int i = 0; i < s; ++i) {
        const double x = own[2 * i], y = own[2 * i + 1];
        for (int d = lane; d < c.D; d += 64) {
            const double v = ellipse_level(x, y, tab + ((size_t)d * N + i) * 5);
            if (v < bv) { bv = v; br = row0 + i; bo = d; }
        }
    }
    wave_argmin3(bv, br, bo);
    if (lane == 0) {
        nmpc_crowd_clearance r = c.rec[b];
        if (bv < r.level || (bv == r.level && (br < r.row || (br == r.row && bo < r.obstacle)))) { r.level = bv; r.row = br; r.obstacle = bo; }
        c.rec[b] = r;
    }
}

// ---- the crowd through a grid in space and stage (nmpc_loop_set_crowd_grid; the rule, and why it misses nobody: DESIGN.md section 5.9) ----
// The same selection over fewer obstacles.  The closeness rule pairs robot and obstacle stage by stage, so entry (d, k) of the table is
// filed under the cell of its position in layer k of a grid the setter fixed (host, nmpc_geom.h), every step anew: a counting sort over
// five kernels (zero, count, tile sums, scan, scatter), whose boundaries order its phases.  A robot then looks, per stage, only at the
// entries filed within `range` of its own position at that stage, and an obstacle is kept at the first stage that finds it in range.
constexpr int CROWD_GRID_CAP = 128;                 // cells per axis at the most
constexpr int CROWD_GRID_MAX = 131072;              // D at the most: 5.2 M entries at N = 40

struct CrowdGridArgs {
    double origin[2], h[2];
    int nx, ny, cells;        // cells = N * nx * ny: layer k holds the cells k * nx * ny + y * nx + x
    double range;
    int *cell_of;             // [D][N]: the entry's cell, -1 = unfiled (a coordinate that is not finite)
    int *cell_off;            // [cells + 1]: cell c holds cell_mem[cell_off[c] .. cell_off[c + 1]); cell_off[cells] = the entries filed
    int *tile_sum;            // [tiles]: the scan's sums per CROWD_GRID_TILE cells
    int *cell_cur;            // [cells]: the scatter's cursors
    int *cell_mem;            // [D * N]: the obstacle d of each filed entry (its stage is its cell's layer)
    int *looked;              // [B]: the filed entries in the robot's windows at its last step
};

// one thread per cell, the one behind the last included: the populations start at zero
__global__ __launch_bounds__(256) void nmpc_loop_crowd_grid_zero_kernel(CrowdGridArgs g)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= g.cells) g.cell_off[c] = 0;
}

// one thread per entry (d, k) of this step's table: its cell into cell_of, and the cell's population counted (integer atomics)
__global__ __launch_bounds__(256) void nmpc_loop_crowd_grid_count_kernel(LoopView L, LoopStep stp, CrowdArgs c, CrowdGridArgs g)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.D * L.N) return;
    const int k = e % L.N;
    const double *q = c.tab[stp.cur ^ 1] + (size_t)e * 5;
    const double x = q[0], y = q[1], inf = __builtin_inf();
    int key = -1;
    if (fabs(x) < inf && fabs(y) < inf) {
        key = (k * g.ny + cellof(y, g.origin[1], g.h[1], g.ny)) * g.nx + cellof(x, g.origin[0], g.h[0], g.nx);
        atomicAdd(g.cell_off + key, 1);
    }
    g.cell_of[e] = key;
}

// The exclusive scan of the populations, the entry behind the last cell included, over tiles of CROWD_GRID_TILE cells, one workgroup
// per tile and four consecutive cells per thread (block_scan over the threads' sums).  First every tile's sum; then each tile adds up
// the sums of the tiles in front of it and scans its own cells in place, and sets the scatter's cursors.  (One workgroup over all
// cells in chunks, as nmpc_loop_peer_grid_kernel scans its 16 384, took 135 us for the 64 980 cells of a 57 x 57 x 20 grid.)
constexpr int CROWD_GRID_TILE = 1024;

__global__ __launch_bounds__(256) void nmpc_loop_crowd_grid_sum_kernel(CrowdGridArgs g)
{
    __shared__ int cnt[256];
    const int c0 = blockIdx.x * CROWD_GRID_TILE + 4 * threadIdx.x;
    int sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) sum += c0 + q <= g.cells ? g.cell_off[c0 + q] : 0;
    const int all = block_scan(cnt, sum);
    if (threadIdx.x == 255) g.tile_sum[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void nmpc_loop_crowd_grid_scan_kernel(CrowdGridArgs g)
{
    __shared__ int cnt[256];
    __shared__ int before;
    const int t = threadIdx.x, tile = blockIdx.x;
    int sum = 0;
    for (int i = t; i < tile; i += 256) sum += g.tile_sum[i];
    const int all = block_scan(cnt, sum);
    if (t == 255) before = all;
    __syncthreads();
    const int c0 = tile * CROWD_GRID_TILE + 4 * t;
    int n[4];
    sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { n[q] = c0 + q <= g.cells ? g.cell_off[c0 + q] : 0; sum += n[q]; }
    int run = before + block_scan(cnt, sum) - sum;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + q;
        if (c <= g.cells) g.cell_off[c] = run;
        if (c < g.cells) g.cell_cur[c] = run;
        run += n[q];
    }
}

// one thread per entry: a filed entry's obstacle into its cell's next place.  The order inside a cell is the atomics' and differs from
// run to run; no result depends on it.
__global__ __launch_bounds__(256) void nmpc_loop_crowd_grid_scatter_kernel(LoopView L, CrowdArgs c, CrowdGridArgs g)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.D * L.N) return;
    const int key = g.cell_of[e];
    if (key >= 0) g.cell_mem[atomicAdd(g.cell_cur + key, 1)] = e / L.N;
}

// One wave per active robot: the rule of nmpc_loop_crowd_kernel over the entries filed in the robot's windows.  Lane k forms the window
// of stage k (none at a stage that is not finite: its d_k is never < range^2); the windows' rows, stage after stage, count as one list,
// and each row of it is one run of cell_mem.  The list is taken 64 rows at a time: the lanes read the rows' bounds, a wave scan lays
// the runs end to end, and the lanes stride over the entries of all 64 rows together (six halvings name an entry's row).  Entry (d, k)
// keeps d if d_k < range^2 and no earlier stage has d_j < range^2 (ascending, four at a time, left at the first four with one): its
// first stage in range alone, so one lane keeps d once, with the C of peer_closeness.  Every loop's bounds are read before it starts,
// and no buffer's size depends on a population: a window of any number of rows and a row of any length take more rounds.
__global__ __launch_bounds__(64) void nmpc_loop_crowd_grid_kernel(LoopView L, LoopStep stp, CrowdArgs c, CrowdGridArgs g)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    __shared__ int wx0[NMPC_MAX_HORIZON], wx1[NMPC_MAX_HORIZON], wy0[NMPC_MAX_HORIZON], wpre[NMPC_MAX_HORIZON];
    __shared__ int rbeg[64], rstage[64], rpre[64];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int N = L.N, per = 5 * N, nx = g.nx, ny = g.ny;
    const double *tab = c.tab[stp.cur ^ 1];
    const double inf = __builtin_inf();
    stage_pred(own, c.pred, b, N);
    // the windows: wpre = the exclusive prefix sums of the stages' rows
    int rows = 0;
    for (int k0 = 0; k0 < N; k0 += 64) {
        const int k = k0 + lane;
        int n = 0;
        if (k < N) {
            const double x = own[2 * k], y = own[2 * k + 1];
            int cx0 = 0, cx1 = 0, cy0 = 0;
            if (fabs(x) < inf && fabs(y) < inf) {
                cx0 = cellof(x - g.range, g.origin[0], g.h[0], nx);
                cx1 = cellof(x + g.range, g.origin[0], g.h[0], nx);
                cy0 = cellof(y - g.range, g.origin[1], g.h[1], ny);
                n = cellof(y + g.range, g.origin[1], g.h[1], ny) - cy0 + 1;
            }
            wx0[k] = cx0; wx1[k] = cx1; wy0[k] = cy0;
        }
        int sum = n;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(sum, off);
            if (lane >= off) sum += o;
        }
        if (k < N) wpre[k] = rows + sum - n;
        rows += __shfl(sum, 63);
    }
    __syncthreads();
    double bd[NDYN_MAX];
    int bj[NDYN_MAX];
    peer_none(bd, bj);
    int looked = 0;
    for (int q0 = 0; q0 < rows; q0 += 64) {
        // row q of the list: the last stage k with wpre[k] <= q holds it (stages without a window are passed)
        const int q = q0 + lane;
        int i0 = 0, len = 0, k = 0;
        if (q < rows) {
            int lo = 0, hi = N - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (wpre[mid] <= q) lo = mid; else hi = mid - 1;
            }
            k = lo;
            const int at = (k * ny + wy0[k] + (q - wpre[k])) * nx;
            i0 = g.cell_off[at + wx0[k]];
            len = g.cell_off[at + wx1[k] + 1] - i0;
        }
        int sum = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(sum, off);
            if (lane >= off) sum += o;
        }
        const int total = __shfl(sum, 63);
        rbeg[lane] = i0; rstage[lane] = k; rpre[lane] = sum - len;
        __syncthreads();
        for (int idx = lane; idx < total; idx += 64) {
            int lo = 0, hi = 63;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (rpre[mid] <= idx) lo = mid; else hi = mid - 1;
            }
            const int kk = rstage[lo], d = g.cell_mem[rbeg[lo] + (idx - rpre[lo])];
            const double *pj = tab + (size_t)d * per;
            const double dx = own[2 * kk] - pj[5 * kk], dy = own[2 * kk + 1] - pj[5 * kk + 1];
            if (dx * dx + dy * dy < c.range2) {
                bool first = true;
                for (int j0 = 0; j0 < kk && first; j0 += 4) {         // four stages at a time: their loads are in flight together
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const bool in = j0 + u < kk;
                        const int j = in ? j0 + u : 0;
                        const double ex = own[2 * j] - pj[5 * j], ey = own[2 * j + 1] - pj[5 * j + 1];
                        if (in && ex * ex + ey * ey < c.range2) first = false;
                    }
                }
                if (first) peer_keep(bd, bj, peer_closeness(own, pj, N, 5), d);
            }
        }
        looked += total;
        __syncthreads();                      // the rows' bounds are read before the next 64 take their place
    }
    peer_overlay(L, b, lane, bd, bj, L.K, c.M, c.seen + (size_t)b * c.M, [&](int d, int e) { return tab[(size_t)d * per + e]; });
    if (lane == 0) g.looked[b] = looked;
}

// ---- walls: each robot's closest points on the map's wall segments as circles (nmpc_loop_set_walls; the rule is DESIGN.md section 5.9) ----
// One kernel between the peers' and the solve: per active robot and edge the smallest wall distance (that of nmpc_loop_map_kernel) over its
// predicted positions, the first M of the edges with D < range^2 in (D, e) order that keep `spacing` from the ones taken before them, each
// one's closest point written over one of the LAST M circle slots of p.  The setter has made sure the assembly leaves those slots zero.
constexpr int WALLS_MAX_EDGES = 1024;       // 16 edges per lane
constexpr int WALLS_MAX_SLOTS = 64;         // M <= nobs <= 64 (nmpc_new)

struct WallArgs {
    int E, M;
    double radius, range2, spacing2;
    const double *edge;       // [E][4] x1 y1 x2 y2
    const double *pred;       // [B][N][3]: the loop's predicted poses (nmpc_loop_predict_kernel)
    int *wall_edge;           // [B][M]: the edge in circle slot nobs - M + m of p[b], -1 = none
    int *wall_stage;          // [B][M]: the stage at which it came closest

    static size_t lds_bytes(int E) { return (size_t)E * (3 * sizeof(double) + sizeof(int)); }
};

// D(e) of the edge ed = (x1, y1, x2, y2) against the N positions in `own` (LDS): the smallest wall distance (segment_closest, that of
// nmpc_loop_map_kernel) over the stages in ascending order, with its closest point and stage k*.  A strict <: the first of equal
// stages stays, a NaN lowers nothing (D = inf, k* = -1 if every stage is one).
__device__ __forceinline__ void wall_closest(const double *own, int N, const double *ed, double &D, double &bx, double &by, int &bk)
{
    const double x1 = ed[0], y1 = ed[1], x2 = ed[2], y2 = ed[3];
    D = __builtin_inf(); bx = 0.0; by = 0.0; bk = -1;
    for (int k = 0; k < N; ++k) {
        double cx, cy;
        const double v = segment_closest(own[2 * k], own[2 * k + 1], x1, y1, x2, y2, true, cx, cy);
        if (v < D) { D = v; bx = cx; by = cy; bk = k; }
    }
}

// The walk of the walls rule, for both walls kernels.  Every round each lane offers the smallest (D, e) of its candidates that lies
// behind the last one considered, (ld, le), with its centre and stage: offer(ld, le, d, j, ox, oy, ok), which leaves (inf, LOOP_NONE)
// where the lane has none.  wave_argmin names the wave's, the one lane that offered it hands over its centre and stage, and lanes
// 0 .. m - 1 test the centre against the m taken before; a centre that keeps `spacing` from all of them takes circle slot nobs - M + m
// of p[b].  A round considers one candidate, so the walk ends after `rounds` rounds at the most (the caller's count of the edges it
// measured), with M taken or with no candidate left, whichever comes first: no loop's bounds depend on a pose.
template <class Offer>
__device__ __forceinline__ void walls_walk(const LoopView &L, const WallArgs &w, int b, int rounds, Offer offer)
{
    __shared__ double tx[WALLS_MAX_SLOTS], ty[WALLS_MAX_SLOTS];      // the centres taken
    const int lane = threadIdx.x, M = w.M;
    double *pc = L.P + (size_t)b * L.n_p + L.p_circ() + 3 * (size_t)(L.nobs - M);
    int *we = w.wall_edge + (size_t)b * M, *ws = w.wall_stage + (size_t)b * M;
    double ld = -1.0;         // the last candidate considered: behind it comes every real one (D >= 0)
    int le = -1;
    int m = 0;
    for (int round = 0; round < rounds && m < M; ++round) {
        double d = __builtin_inf(), ox = 0.0, oy = 0.0;
        int j = LOOP_NONE, ok = -1;
        offer(ld, le, d, j, ox, oy, ok);
        double dd = d;
        int jj = j;
        wave_argmin(dd, jj);
        if (jj == LOOP_NONE) break;           // (wave-uniform) no candidate left: the remaining slots keep the assembly's zeros
        ld = dd; le = jj;
        const int src = __ffsll((long long)__ballot(j == jj)) - 1;      // the one lane that measured edge jj
        const double cx = __shfl(ox, src), cy = __shfl(oy, src);
        const int ck = __shfl(ok, src);
        bool close = false;
        if (lane < m) {
            const double ddx = cx - tx[lane], ddy = cy - ty[lane];
            close = ddx * ddx + ddy * ddy < w.spacing2;
        }
        if (__any(close)) continue;           // (wave-uniform)
        if (lane == 0) {
            tx[m] = cx; ty[m] = cy;
            pc[3 * m] = cx; pc[3 * m + 1] = cy; pc[3 * m + 2] = w.radius;
            we[m] = jj; ws[m] = ck;
        }
        ++m;
        __syncthreads();                      // lane 0's stores of tx, ty before the next round's loads
    }
    for (int q = m + lane; q < M; q += 64) { we[q] = -1; ws[q] = -1; }
}

// One wave per active robot, WallArgs::lds_bytes(E) of dynamic LDS: D | cx | cy [E] doubles and k* [E] ints.  The predicted positions
// go to LDS; lanes stride over the edges (wall_closest) and park (D, cx, cy, k*) in LDS.  Then the walk, a lane's candidates being its
// edges of the table with D < range2: E rounds at the most.
__global__ __launch_bounds__(64) void nmpc_loop_walls_kernel(LoopView L, WallArgs w)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    extern __shared__ double wall_lds[];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int N = L.N, E = w.E;
    double *sD = wall_lds, *sx = sD + E, *sy = sx + E;
    int *sk = (int *)(sy + E);
    stage_pred(own, w.pred, b, N);
    for (int e = lane; e < E; e += 64) {
        double D, bx, by;
        int bk;
        wall_closest(own, N, w.edge + 4 * (size_t)e, D, bx, by, bk);
        sD[e] = D; sx[e] = bx; sy[e] = by; sk[e] = bk;
    }
    __syncthreads();
    walls_walk(L, w, b, E, [&](double ld, int le, double &d, int &j, double &ox, double &oy, int &ok) {
        for (int e = lane; e < E; e += 64) {
            const double c = sD[e];
            if (c < w.range2 && (c > ld || (c == ld && e > le)) && c < d) { d = c; j = e; }      // (a lane's edges ascend: of equal D the first stays)
        }
        if (j != LOOP_NONE) { ox = sx[j]; oy = sy[j]; ok = sk[j]; }
    });
}

// ---- walls through a grid (nmpc_loop_set_walls_grid; the rule, and why it hides no edge: DESIGN.md section 5.9) ----
// The same rule over fewer edges.  The edges never move, so the setter builds the grid once, on the host: every edge is filed in every
// cell of the rectangle of cells its box covers (CSR: cell_off, cell_edge, the edges ascending inside a cell), and a robot measures the
// edges filed in the cells its predicted positions can reach.  Every D is formed by wall_closest, as in nmpc_loop_walls_kernel, and tested
// against the same range2, so a window wider than needed changes no result.
constexpr int WALL_GRID_CAP = 512;                  // cells per axis at the most
constexpr int WALL_GRID_MAX_EDGES = 1 << 20;
constexpr int WALL_GRID_MAX_ENTRIES = 1 << 23;      // filings at the most (cell_edge and cell_tag: 32 MB each)
constexpr int WALL_GRID_LIST = 256;                 // candidates the LDS list holds; more take the exact rounds

struct WallGridArgs {
    double origin[2], h[2];
    int nx, ny;
    double range, slack;      // the window's margin: slack = 2^-40 (range + the largest |coordinate| of an edge) + 2^-500
    const int *cell_off;      // [nx * ny + 1]: cell c (row-major, y * nx + x) holds cell_edge[cell_off[c] .. cell_off[c + 1])
    const int *cell_edge;     // [entries]
    const int *cell_tag;      // [entries]: di | dj << 9 | col0 << 18, the filing's place in its edge's rectangle and the rectangle's first column
    int *looked;              // [B]: the distinct edges the last step measured
};

// One wave per active robot.  The predicted positions go to LDS and their box over the finite stages (a wave reduction of minima and
// maxima) gives the window cx0 .. cx1 x cy0 .. cy1 (cellof of nmpc_geom.h, the function of the setter's filing); a robot without a
// finite stage looks at nothing.  A row of the window is one run of cell_edge; the rows' runs are laid end to end and the lanes
// stride over them in steps of 64, all lanes together.  An edge filed in
// several cells of the window is measured in one of them only, the first of its rectangle that lies in the window (di == max(0, cx0 -
// col0), the same in j), so `looked` counts distinct edges.  A candidate (D < range2) is appended to an LDS list at the place a ballot
// gives it.  Then the walk (walls_walk).  With WALL_GRID_LIST candidates or fewer a lane's candidates are its entries of the list; with
// more the list is dropped and every round measures the window again, which needs no memory and gives the same (D, e) sequence.  The
// walk ends after `seen` rounds at the most, seen <= E the window's distinct edges.  No loop's bounds depend on a pose other than
// through the window, which is clamped to the grid.
__global__ __launch_bounds__(64) void nmpc_loop_walls_grid_kernel(LoopView L, WallArgs w, WallGridArgs g)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    __shared__ double lD[WALL_GRID_LIST], lx[WALL_GRID_LIST], ly[WALL_GRID_LIST];
    __shared__ int lE[WALL_GRID_LIST], lk[WALL_GRID_LIST];
    __shared__ int rbeg[WALL_GRID_CAP], rpre[WALL_GRID_CAP + 1];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int N = L.N;
    const double inf = __builtin_inf();
    double lox = inf, loy = inf, hix = -inf, hiy = -inf;
    stage_pred(own, w.pred, b, N, [&](double x, double y) { box_fold(x, y, lox, loy, hix, hiy); });
    lox = wave_min(lox); loy = wave_min(loy); hix = wave_max(hix); hiy = wave_max(hiy);
    // the window: the same in every lane; cy1 < cy0 for a robot that looks at nothing
    const int nx = g.nx;
    int cx0 = 0, cx1 = 0, cy0 = 0, cy1 = -1;
    if (lox <= hix) {
        const double tm = 0x1p-40;
        cx0 = cellof((lox - g.range) - (g.slack + tm * fabs(lox)), g.origin[0], g.h[0], nx);
        cx1 = cellof((hix + g.range) + (g.slack + tm * fabs(hix)), g.origin[0], g.h[0], nx);
        cy0 = cellof((loy - g.range) - (g.slack + tm * fabs(loy)), g.origin[1], g.h[1], g.ny);
        cy1 = cellof((hiy + g.range) + (g.slack + tm * fabs(hiy)), g.origin[1], g.h[1], g.ny);
    }
    // the window's rows: row r is the run cell_edge[rbeg[r] .. ) of rpre[r + 1] - rpre[r] filings, rpre the exclusive prefix sums (a wave scan
    // per 64 rows).  The filings of all rows then count as ONE list of `total`, over which the lanes stride: a window of several short rows
    // costs one pass, not one per row.
    const int R = cy1 - cy0 + 1;
    int total = 0;
    for (int r0 = 0; r0 < R; r0 += 64) {
        const int r = r0 + lane;
        int i0 = 0, len = 0;
        if (r < R) {
            i0 = g.cell_off[(cy0 + r) * nx + cx0];
            len = g.cell_off[(cy0 + r) * nx + cx1 + 1] - i0;
        }
        int sum = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(sum, off);
            if (lane >= off) sum += o;
        }
        if (r < R) { rbeg[r] = i0; rpre[r] = total + sum - len; }
        total += __shfl(sum, 63);
    }
    if (lane == 0) rpre[R > 0 ? R : 0] = total;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    // place idx < total of that list: its filing's place i in cell_edge and, from the filing's tag, whether this is the cell at which its
    // edge is measured (at most nine halvings over the rows; the last row r with rpre[r] <= idx holds idx, rows without filings are passed)
    auto mine = [&](int idx, int &i) {
        int lo = 0, hi = R - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rpre[mid] <= idx) lo = mid; else hi = mid - 1;
        }
        i = rbeg[lo] + (idx - rpre[lo]);
        const int tag = g.cell_tag[i];
        const int di = tag & 511, dj = (tag >> 9) & 511, col0 = tag >> 18, row0 = cy0 + lo - dj;
        return di == (cx0 > col0 ? cx0 - col0 : 0) && dj == (cy0 > row0 ? cy0 - row0 : 0);
    };
    int seen = 0, cnt = 0;
    for (int base = 0; base < total; base += 64) {
        const int idx = base + lane;
        bool cand = false;
        double D = inf, bx = 0.0, by = 0.0;
        int bk = -1, e = LOOP_NONE, i = 0;
        const bool meas = idx < total && mine(idx, i);
        if (meas) {
            e = g.cell_edge[i];
            wall_closest(own, N, w.edge + 4 * (size_t)e, D, bx, by, bk);
            cand = D < w.range2;
        }
        seen += __popcll(__ballot(meas));
        const unsigned long long cm = __ballot(cand);
        const int at = cnt + __popcll(cm & below);
        if (cand && at < WALL_GRID_LIST) { lD[at] = D; lx[at] = bx; ly[at] = by; lE[at] = e; lk[at] = bk; }
        cnt += __popcll(cm);
    }
    __syncthreads();
    const bool listed = cnt <= WALL_GRID_LIST;        // (wave-uniform)
    // a lane's offer: among equal D the smaller edge index is kept
    walls_walk(L, w, b, seen, [&](double ld, int le, double &d, int &j, double &ox, double &oy, int &ok) {
        if (listed) {
            for (int q = lane; q < cnt; q += 64) {
                const double c = lD[q];
                const int e = lE[q];
                if ((c > ld || (c == ld && e > le)) && (c < d || (c == d && e < j))) { d = c; j = e; ox = lx[q]; oy = ly[q]; ok = lk[q]; }
            }
        } else {
            for (int idx = lane; idx < total; idx += 64) {
                int i;
                if (!mine(idx, i)) continue;
                const int e = g.cell_edge[i];
                double c, bx, by;
                int bk;
                wall_closest(own, N, w.edge + 4 * (size_t)e, c, bx, by, bk);
                if (c < w.range2 && (c > ld || (c == ld && e > le)) && (c < d || (c == d && e < j))) { d = c; j = e; ox = bx; oy = by; ok = bk; }
            }
        }
    });
    if (lane == 0) g.looked[b] = seen;
}

// ---- retirement: robots that reached their goal leave the loop (nmpc_loop_set_retire; the rule is DESIGN.md section 5.9) ----
struct RetireArgs {
    int *retired_at;          // [B]: -1 = active
    int *list;                // [B]: LoopView::act as the compaction writes it, the robots still active in ascending index
    int *count;               // [1]: their number
    double *sP, *sU, *sY;     // [count][n_p], [count][n_u], [count][n1]: the rows the solve reads and writes, row i = robot act[i]
    nmpc_status *sst;         // [count]
};

// One workgroup, after the advance: thread t takes its chunk of the robots (block_chunk), so that an exclusive scan of the threads'
// counts gives each its place in the ascending list.  An active robot that is done (done[b] is of this step's advance for the robots
// it ran over, 1 for every robot retired before) is retired at this step: retired_at latches, and with peers (pred, theirs, else NULL)
// its row of pred becomes its final pose at every stage, a copy, for as long as the others look at it.  A robot retired earlier
// repeats its final pose in this step's trajectory rows.
__global__ __launch_bounds__(1024) void nmpc_loop_compact_kernel(LoopView L, LoopStep stp, RetireArgs r, double *pred)
{
    __shared__ int cnt[1024];
    int lo, hi;
    block_chunk(L.B, lo, hi);
    int c = 0;
    for (int b = lo; b < hi; ++b) {
        const double x = L.state[3 * b], y = L.state[3 * b + 1], th = L.state[3 * b + 2];
        if (r.retired_at[b] >= 0) {
            if (L.traj) {
                for (int i = 0; i < L.s; ++i) {
                    double *row = L.row(stp.traj_row + i, b);
                    row[0] = x; row[1] = y; row[2] = th;
                }
            }
        } else if (L.done[b]) {
            r.retired_at[b] = stp.step;
            if (pred) {
                double *out = pred + (size_t)b * L.N * 3;
                for (int k = 0; k < L.N; ++k) { out[3 * k] = x; out[3 * k + 1] = y; out[3 * k + 2] = th; }
            }
        } else {
            ++c;
        }
    }
    const int end = block_scan(cnt, c);
    int pos = end - c;
    for (int b = lo; b < hi; ++b)
        if (r.retired_at[b] < 0) r.list[pos++] = b;     // (the thread's own stores above)
    if (threadIdx.x == blockDim.x - 1) *r.count = end;
}

__device__ __forceinline__ void copy_row(double *dst, const double *src, int n)
{
    for (int e = threadIdx.x; e < n; e += blockDim.x) dst[e] = src[e];
}

// one workgroup per active robot.  The status row goes along: it is the launch-order hint of the solve (the same robot's previous pass count)
__global__ __launch_bounds__(256) void nmpc_loop_gather_kernel(LoopView L, RetireArgs r)
{
    const size_t i = blockIdx.x, b = (size_t)L.act[blockIdx.x];
    copy_row(r.sP + i * L.n_p, L.P + b * L.n_p, L.n_p);
    copy_row(r.sU + i * L.n_u, L.U + b * L.n_u, L.n_u);
    copy_row(r.sY + i * L.n1, L.Y + b * L.n1, L.n1);
    if (threadIdx.x == 0) r.sst[i] = L.st[b];
}

__global__ __launch_bounds__(256) void nmpc_loop_scatter_kernel(LoopView L, RetireArgs r)
{
    const size_t i = blockIdx.x, b = (size_t)L.act[blockIdx.x];
    copy_row(L.U + b * L.n_u, r.sU + i * L.n_u, L.n_u);
    copy_row(L.Y + b * L.n1, r.sY + i * L.n1, L.n1);
    if (threadIdx.x == 0) L.st[b] = r.sst[i];
}

// ---- clearance monitor: each robot's closest approach to circles, scripted ellipses and groupmates (nmpc_loop_set_monitor; the
// rule is DESIGN.md section 5.9).  It observes: the record is the only thing it writes.
struct MonitorArgs {
    GroupLists grp;           // the monitor's own groups
    nmpc_clearance *rec;      // [B]
};

// One wave per robot the step drove, after the advance: the robot's s new poses go to LDS; lanes stride over the (pose, circle slot)
// and (pose, scripted ellipse) pairs of its p, then over the members of its group, each lane walking the s rows of its member (a
// robot retired earlier stands at its state: the compaction writes its rows later); every lane keeps its lexicographic minimum, three
// wave reductions follow, and lane 0 folds them into the record.  A lane that saw nothing holds (inf, LOOP_NONE): behind every value.
// P is this step's parameter vectors as the solve read them; retired_at is retirement's (NULL: nobody retires), as the step found it.
__global__ __launch_bounds__(64) void nmpc_loop_monitor_kernel(LoopView L, LoopStep stp, MonitorArgs m, const int *retired_at)
{
    __shared__ double own[2 * NMPC_MAX_HORIZON];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int s = L.s, N = L.N, nobs = L.nobs, K = L.K, row0 = stp.traj_row;
    const int g = m.grp.group_of[b];
    const int lo = m.grp.goff[g], hi = m.grp.goff[g + 1];
    stage_rows<2>(own, L, b, row0, s);
    const double *p = L.P + (size_t)b * L.n_p;
    // ---- static circles: sqrt(dx^2 + dy^2) - r over the slots with r > 0
    double cv = __builtin_inf();
    int cr = LOOP_NONE;
    {
        const double *pc = p + L.p_circ();
        const int tot = s * nobs;
        for (int e = lane; e < tot; e += 64) {
            const int i = e / nobs, c = e - i * nobs;
            const double rc = pc[3 * c + 2];
            if (rc > 0.0) {
                const double dx = own[2 * i] - pc[3 * c], dy = own[2 * i + 1] - pc[3 * c + 1];
                const double v = sqrt(dx * dx + dy * dy) - rc;
                const int r = row0 + i;
                if (v < cv || (v == cv && r < cr)) { cv = v; cr = r; }
            }
        }
        wave_argmin(cv, cr);
    }
    // ---- scripted ellipses: the cost's level (a/rx)^2 + (c/ry)^2 at entry i of slot k, for the pose after control i
    double ev = __builtin_inf();
    int er = LOOP_NONE;
    {
        const double *pd = p + L.p_dyn();
        const int tot = s * K;
        for (int e = lane; e < tot; e += 64) {
            const int i = e / K, k = e - i * K;
            const double v = ellipse_level(own[2 * i], own[2 * i + 1], pd + ((size_t)k * N + i) * 5);
            const int r = row0 + i;
            if (v < ev || (v == ev && r < er)) { ev = v; er = r; }
        }
        wave_argmin(ev, er);
    }
    // ---- groupmates: squared distance between centres, in the same row
    double pv = __builtin_inf();
    int pr = LOOP_NONE, pj = LOOP_NONE;
    for (int at = lo + lane; at < hi; at += 64) {
        const int j = m.grp.gmem[at];
        if (j == b) continue;
        const bool parked = retired_at && retired_at[j] >= 0;
        for (int i = 0; i < s; ++i) {
            const double *q = parked ? L.state + 3 * (size_t)j : L.row(row0 + i, j);
            const double dx = own[2 * i] - q[0], dy = own[2 * i + 1] - q[1];
            const double v = dx * dx + dy * dy;
            const int r = row0 + i;
            if (v < pv || (v == pv && (r < pr || (r == pr && j < pj)))) { pv = v; pr = r; pj = j; }
        }
    }
    wave_argmin3(pv, pr, pj);
    if (lane == 0) {
        nmpc_clearance c = m.rec[b];
        if (cv < c.circle || (cv == c.circle && cr < c.circle_row)) { c.circle = cv; c.circle_row = cr; }
        if (ev < c.ellipse || (ev == c.ellipse && er < c.ellipse_row)) { c.ellipse = ev; c.ellipse_row = er; }
        if (pv < c.peer2 || (pv == c.peer2 && (pr < c.peer_row || (pr == c.peer_row && pj < c.peer)))) {
            c.peer2 = pv; c.peer_row = pr; c.peer = pj;
        }
        m.rec[b] = c;
    }
}

// ---- map monitor: each robot's closest approach to the walls of a polygon map, and the rows at which it was inside an obstacle, outside
// the boundary or went through an edge (nmpc_loop_set_map_monitor; the rule is DESIGN.md section 5.9).  It observes: the record is the
// only thing it writes.  For the pose (x, y) of row r and (ax, ay) of row r - 1, unfused f64 in the order written, no sqrt:
//   wall      per edge (x1, y1, x2, y2): ex = x2 - x1, ey = y2 - y1, L2 = ex*ex + ey*ey; t = 0 unless L2 > 0, then t = ((x - x1)*ex +
//             (y - y1)*ey)/L2 clamped by `if (t < 0) t = 0; if (t > 1) t = 1`; dx = x - (x1 + t*ex), dy = y - (y1 + t*ey), v = dx*dx + dy*dy
//   inside    polygon k, even-odd: an edge with (y1 > y) != (y2 > y) is a crossing if x1 + ((y - y1)*(x2 - x1))/(y2 - y1) > x; an obstacle
//             fails on an odd count, the boundary (the last polygon) on an even one
//   crossing  edge (c, d) is crossed if o1*o2 < -1e-9 && o3*o4 < -1e-9 (the planner's segment test, nmpc_plan.h); its polygon fails
// A row is a hit if any polygon fails.  The record keeps the lexicographic minimum of (v, r, e), the number of hits, the first hit's row
// and the smallest failing polygon of that row; a comparison that is false (a NaN) keeps what it would have replaced.
struct MapArgs {
    int E, n_poly;
    const double *edge;       // [E][4] x1 y1 x2 y2, polygon by polygon: the obstacles first, the boundary last
    const int *poly_off;      // [n_poly + 1]
    const int *edge_poly;     // [E]: the polygon that owns the edge
    nmpc_map_clearance *rec;  // [B]
};

// One wave per robot the step drove, after the advance (and the clearance monitor): the robot's s + 1 poses, from the row before the
// step's first on, go to LDS.  Row by row, lanes stride over the edges (wall distance, crossing test: consecutive lanes read consecutive
// edges, 32 bytes apart, through the cache: the table is the same for every robot), then over the polygons, each lane walking the edges
// of its polygon for the parity; a wave minimum of the failing polygon index is the row's verdict.  Every lane keeps its lexicographic
// minimum of (v, r, e); one wave reduction follows the rows, and lane 0 folds everything into the record.  Every loop is bounded by s, E
// or n_poly (poly_off was checked by the setter).
__global__ __launch_bounds__(64) void nmpc_loop_map_kernel(LoopView L, LoopStep stp, MapArgs m)
{
    __shared__ double own[2 * (NMPC_MAX_HORIZON + 1)];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int s = L.s, E = m.E, n_poly = m.n_poly, row0 = stp.traj_row;      // (row0 >= 1: the row before it is there)
    stage_rows<2>(own, L, b, row0 - 1, s + 1);
    double wv = __builtin_inf();
    int wr = LOOP_NONE, we = LOOP_NONE;
    int hits = 0, hit_row = LOOP_NONE, hit_poly = LOOP_NONE;        // the same in every lane
    for (int i = 0; i < s; ++i) {
        const double ax = own[2 * i], ay = own[2 * i + 1], x = own[2 * i + 2], y = own[2 * i + 3];
        const double ux = x - ax, uy = y - ay;
        const int r = row0 + i;
        int fail = LOOP_NONE;
        for (int e = lane; e < E; e += 64) {
            const double x1 = m.edge[4 * e], y1 = m.edge[4 * e + 1], x2 = m.edge[4 * e + 2], y2 = m.edge[4 * e + 3];
            double cx, cy;
            const double v = segment_closest(x, y, x1, y1, x2, y2, true, cx, cy);
            if (v < wv) { wv = v; wr = r; we = e; }       // (rows and a lane's edges ascend: among equal values the first stays)
            const double ex = x2 - x1, ey = y2 - y1;
            const double o1 = ux * (y1 - ay) - uy * (x1 - ax);
            const double o2 = ux * (y2 - ay) - uy * (x2 - ax);
            const double o3 = ex * (ay - y1) - ey * (ax - x1);
            const double o4 = ex * (y - y1) - ey * (x - x1);
            if (o1 * o2 < -1e-9 && o3 * o4 < -1e-9) {
                const int k = m.edge_poly[e];
                if (k < fail) fail = k;
            }
        }
        for (int k = lane; k < n_poly; k += 64) {
            const int lo = m.poly_off[k], hi = m.poly_off[k + 1];
            bool odd = false;
            for (int e = lo; e < hi; ++e) {
                const double y1 = m.edge[4 * e + 1], y2 = m.edge[4 * e + 3];
                if ((y1 > y) != (y2 > y)) {
                    const double x1 = m.edge[4 * e], x2 = m.edge[4 * e + 2];
                    const double xi = x1 + ((y - y1) * (x2 - x1)) / (y2 - y1);
                    if (xi > x) odd = !odd;
                }
            }
            const bool bad = k == n_poly - 1 ? !odd : odd;
            if (bad && k < fail) fail = k;
        }
        fail = wave_min(fail);
        if (fail != LOOP_NONE) {
            if (hits == 0) { hit_row = r; hit_poly = fail; }
            ++hits;
        }
    }
    wave_argmin3(wv, wr, we);
    if (lane == 0) {
        nmpc_map_clearance c = m.rec[b];
        if (wv < c.wall2 || (wv == c.wall2 && (wr < c.wall_row || (wr == c.wall_row && we < c.wall_edge)))) {
            c.wall2 = wv; c.wall_row = wr; c.wall_edge = we;
        }
        if (hits > 0) {
            if (c.hits == 0) { c.hit_row = hit_row; c.hit_poly = hit_poly; }
            c.hits += hits;
        }
        m.rec[b] = c;
    }
}

// ---- map monitor through a grid (nmpc_loop_set_map_monitor_grid; the rule, and why it is the all-edges rule's result: DESIGN.md
// section 5.9) ----
// The same three tests over fewer edges.  The grid is the walls grid (WallGridArgs, built by the setter's WallGridHost::build): a row
// measures the distinct edges filed in the window of its two poses padded by `range` for the wall distance (only v < range^2 is a
// candidate) and the crossing, and the distinct edges filed in the grid row of y, from the column of x - m(x) to the last, for the
// containment.  A row with a coordinate that is not finite is judged against every edge, as nmpc_loop_map_kernel judges it.
constexpr int MAP_GRID_HITS = 512;          // ray hits on obstacle edges the LDS list holds; a pose with more takes the exact rounds

// the sum over the wave, result in every lane
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The two steps below are nmpc_loop_walls_grid_kernel's, statement for statement; that kernel keeps them in its body, as built and measured.
// The rows cy0 .. cy0 + R - 1 of a window over the columns cx0 .. cx1, for a wave: row r is the run cell_edge[rbeg[r] .. ) of rpre[r + 1] -
// rpre[r] filings, rpre the exclusive prefix sums (a wave scan per 64 rows), -> their total.  The filings of all rows then count as ONE
// list, over which the lanes stride: a window of several short rows costs one pass, not one per row.  Barrier included.
__device__ __forceinline__ int window_rows(const WallGridArgs &g, int cx0, int cx1, int cy0, int R, int *rbeg, int *rpre)
{
    const int lane = threadIdx.x, nx = g.nx;
    int total = 0;
    for (int r0 = 0; r0 < R; r0 += 64) {
        const int r = r0 + lane;
        int i0 = 0, len = 0;
        if (r < R) {
            i0 = g.cell_off[(cy0 + r) * nx + cx0];
            len = g.cell_off[(cy0 + r) * nx + cx1 + 1] - i0;
        }
        int sum = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(sum, off);
            if (lane >= off) sum += o;
        }
        if (r < R) { rbeg[r] = i0; rpre[r] = total + sum - len; }
        total += __shfl(sum, 63);
    }
    if (lane == 0) rpre[R > 0 ? R : 0] = total;
    __syncthreads();
    return total;
}

// place idx < total of that list: its filing's place i in cell_edge and, from the filing's tag, whether this is the cell at which its
// edge is measured (at most nine halvings over the rows; the last row r with rpre[r] <= idx holds idx, rows without filings are passed)
__device__ __forceinline__ bool window_filing(const WallGridArgs &g, int cx0, int cy0, int R, const int *rbeg, const int *rpre, int idx, int &i)
{
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rpre[mid] <= idx) lo = mid; else hi = mid - 1;
    }
    i = rbeg[lo] + (idx - rpre[lo]);
    const int tag = g.cell_tag[i];
    const int di = tag & 511, dj = (tag >> 9) & 511, col0 = tag >> 18, row0 = cy0 + lo - dj;
    return di == (cx0 > col0 ? cx0 - col0 : 0) && dj == (cy0 > row0 ? cy0 - row0 : 0);
}

// One wave per robot the step drove, in nmpc_loop_map_kernel's place: the robot's s + 1 poses go to LDS.  Row by row:
//   window       its rows are runs of cell_edge laid end to end (window_rows, window_filing: nmpc_loop_walls_grid_kernel's); the lanes stride
//                over the filings, an edge filed in several cells of the window is taken in the first cell of its rectangle that lies in
//                the window (the filing's tag), so `looked` counts distinct edges.  Wall distance and crossing test per edge, as in nmpc_loop_map_kernel.
//   containment  one run of cell_edge; an edge is taken in the first column of its rectangle at or behind the ray's first.  A hit on the
//                boundary is counted, a hit on an obstacle appends its polygon to an LDS list at the place a ballot gives it.  Then rounds:
//                each names the smallest polygon behind the last one named and counts its hits (a lane keeps the smallest of its
//                entries and how often it saw it; a wave minimum and a wave sum follow); an odd count fails it and ends the rounds, as
//                does a polygon that is not below what has failed already.  With more hits than the list holds a round walks the run
//                again, which needs no memory and names the same polygons.  There are no more rounds than hits.
// Every loop is bounded by s, E, n_poly or the grid's size: the window and the ray are clamped to the grid.
__global__ __launch_bounds__(64) void nmpc_loop_map_grid_kernel(LoopView L, LoopStep stp, MapArgs m, WallGridArgs g)
{
    __shared__ double own[2 * (NMPC_MAX_HORIZON + 1)];
    __shared__ int rbeg[WALL_GRID_CAP], rpre[WALL_GRID_CAP + 1];
    __shared__ int hk[MAP_GRID_HITS];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    const int s = L.s, E = m.E, n_poly = m.n_poly, row0 = stp.traj_row, nx = g.nx;
    const double inf = __builtin_inf(), tm = 0x1p-40, range2 = g.range * g.range;
    const unsigned long long below = (1ull << lane) - 1ull;
    stage_rows<2>(own, L, b, row0 - 1, s + 1);
    double wv = inf;
    int wr = LOOP_NONE, we = LOOP_NONE;
    int hits = 0, hit_row = LOOP_NONE, hit_poly = LOOP_NONE, looked = 0;      // the same in every lane
    // wall distance and crossing test of edge e for the row's poses
    auto measure = [&](int e, int r, double ax, double ay, double x, double y, int &fail) {
        const double x1 = m.edge[4 * (size_t)e], y1 = m.edge[4 * (size_t)e + 1], x2 = m.edge[4 * (size_t)e + 2], y2 = m.edge[4 * (size_t)e + 3];
        double cx, cy;
        const double v = segment_closest(x, y, x1, y1, x2, y2, true, cx, cy);
        if (v < range2 && (v < wv || (v == wv && (r < wr || (r == wr && e < we))))) { wv = v; wr = r; we = e; }
        const double ux = x - ax, uy = y - ay, ex = x2 - x1, ey = y2 - y1;
        const double o1 = ux * (y1 - ay) - uy * (x1 - ax);
        const double o2 = ux * (y2 - ay) - uy * (x2 - ax);
        const double o3 = ex * (ay - y1) - ey * (ax - x1);
        const double o4 = ex * (y - y1) - ey * (x - x1);
        if (o1 * o2 < -1e-9 && o3 * o4 < -1e-9) {
            const int k = m.edge_poly[e];
            if (k < fail) fail = k;
        }
    };
    // whether the ray from (x, y) to the right meets edge e by the containment's predicate
    auto meets = [&](int e, double x, double y) {
        const double y1 = m.edge[4 * (size_t)e + 1], y2 = m.edge[4 * (size_t)e + 3];
        if ((y1 > y) == (y2 > y)) return false;
        const double x1 = m.edge[4 * (size_t)e], x2 = m.edge[4 * (size_t)e + 2];
        return x1 + ((y - y1) * (x2 - x1)) / (y2 - y1) > x;
    };
    for (int i = 0; i < s; ++i) {
        const double ax = own[2 * i], ay = own[2 * i + 1], x = own[2 * i + 2], y = own[2 * i + 3];
        const int r = row0 + i;
        int fail = LOOP_NONE;
        if (!(fabs(x) < inf && fabs(y) < inf && fabs(ax) < inf && fabs(ay) < inf)) {      // (wave-uniform) every edge, polygon by polygon
            for (int e = lane; e < E; e += 64) measure(e, r, ax, ay, x, y, fail);
            for (int k = lane; k < n_poly; k += 64) {
                bool odd = false;
                for (int e = m.poly_off[k]; e < m.poly_off[k + 1]; ++e)
                    if (meets(e, x, y)) odd = !odd;
                if ((k == n_poly - 1 ? !odd : odd) && k < fail) fail = k;
            }
            fail = wave_min(fail);
            looked += E;
        } else {
            // ---- the window of the two poses
            const double lox = x < ax ? x : ax, hix = x < ax ? ax : x, loy = y < ay ? y : ay, hiy = y < ay ? ay : y;
            const int cx0 = cellof((lox - g.range) - (g.slack + tm * fabs(lox)), g.origin[0], g.h[0], nx);
            const int cx1 = cellof((hix + g.range) + (g.slack + tm * fabs(hix)), g.origin[0], g.h[0], nx);
            const int cy0 = cellof((loy - g.range) - (g.slack + tm * fabs(loy)), g.origin[1], g.h[1], g.ny);
            const int cy1 = cellof((hiy + g.range) + (g.slack + tm * fabs(hiy)), g.origin[1], g.h[1], g.ny);
            const int R = cy1 - cy0 + 1;          // >= 1: cellof is monotone
            const int total = window_rows(g, cx0, cx1, cy0, R, rbeg, rpre);
            for (int base = 0; base < total; base += 64) {
                const int idx = base + lane;
                int at;
                const bool meas = idx < total && window_filing(g, cx0, cy0, R, rbeg, rpre, idx, at);
                if (meas) measure(g.cell_edge[at], r, ax, ay, x, y, fail);
                looked += __popcll(__ballot(meas));
            }
            fail = wave_min(fail);
            // ---- the ray: grid row cellof(y), from the column of x - m(x) to the last
            const int c0 = cellof(x - (g.slack + tm * fabs(x)), g.origin[0], g.h[0], nx);
            const int cy = cellof(y, g.origin[1], g.h[1], g.ny);
            const int i0 = g.cell_off[cy * nx + c0], i1 = g.cell_off[cy * nx + nx];
            // the edge a filing of the run stands for, LOOP_NONE where another filing of the run does
            auto taken = [&](int at) {
                const int tag = g.cell_tag[at];
                const int col0 = tag >> 18;
                return (tag & 511) == (c0 > col0 ? c0 - col0 : 0) ? g.cell_edge[at] : LOOP_NONE;
            };
            int nb = 0, cnt = 0;
            for (int base = i0; base < i1; base += 64) {
                const int at = base + lane;
                int k = LOOP_NONE;
                if (at < i1) {
                    const int e = taken(at);
                    if (e != LOOP_NONE && meets(e, x, y)) k = m.edge_poly[e];
                }
                if (k == n_poly - 1) { ++nb; k = LOOP_NONE; }
                const unsigned long long hm = __ballot(k != LOOP_NONE);
                const int to = cnt + __popcll(hm & below);
                if (k != LOOP_NONE && to < MAP_GRID_HITS) hk[to] = k;
                cnt += __popcll(hm);
            }
            __syncthreads();
            const bool listed = cnt <= MAP_GRID_HITS;       // (wave-uniform)
            int last = -1;
            for (int round = 0; round < cnt; ++round) {
                int km = LOOP_NONE, c = 0;
                auto offer = [&](int k) {
                    if (k > last && k <= km) { c = k < km ? 1 : c + 1; km = k; }
                };
                if (listed) {
                    for (int q = lane; q < cnt; q += 64) offer(hk[q]);
                } else {
                    for (int at = i0 + lane; at < i1; at += 64) {
                        const int e = taken(at);
                        if (e == LOOP_NONE || !meets(e, x, y)) continue;
                        const int k = m.edge_poly[e];
                        if (k != n_poly - 1) offer(k);
                    }
                }
                const int kk = wave_min(km);
                if (kk >= fail) break;            // (wave-uniform) nothing left below what has failed
                if (wave_sum(km == kk ? c : 0) & 1) { fail = kk; break; }
                last = kk;
            }
            if (!(wave_sum(nb) & 1) && n_poly - 1 < fail) fail = n_poly - 1;
            __syncthreads();                      // this row's loads of rbeg, rpre and hk before the next row's stores
        }
        if (fail != LOOP_NONE) {
            if (hits == 0) { hit_row = r; hit_poly = fail; }
            ++hits;
        }
    }
    wave_argmin3(wv, wr, we);
    if (lane == 0) {
        nmpc_map_clearance c = m.rec[b];
        if (wv < c.wall2 || (wv == c.wall2 && (wr < c.wall_row || (wr == c.wall_row && we < c.wall_edge)))) {
            c.wall2 = wv; c.wall_row = wr; c.wall_edge = we;
        }
        if (hits > 0) {
            if (c.hits == 0) { c.hit_row = hit_row; c.hit_poly = hit_poly; }
            c.hits += hits;
        }
        m.rec[b] = c;
        g.looked[b] = looked;
    }
}

// ---- track monitor: how far each robot was from the route it was asked to follow (nmpc_loop_set_track_monitor; the rule is DESIGN.md
// section 5.9).  It observes: the record is the only thing it writes.  The route is routes[route_of[b]] as the step found it (the dispatch
// comes after), its polyline Q_j = (x_ref[j], y_ref[j]), n_seg = max(n_ref - 1, 1) segments, segment j from Q_j to Q_e, e = min(j + 1,
// n_ref - 1).  For the pose (x, y, th) of row r, unfused f64 in the order written, no sqrt:
//   segment j   ex = x2 - x1, ey = y2 - y1, L2 = ex*ex + ey*ey; t = 0 unless L2 > 0, then t = ((x - x1)*ex + (y - y1)*ey)/L2;
//               `if (t < 0 && j > 0) t = 0; if (t > 1) t = 1` (segment 0 runs on backwards: the table begins one sample after the start);
//               dx = x - (x1 + t*ex), dy = y - (y1 + t*ey), v = dx*dx + dy*dy
//   row         (v*, j*) = the first smallest v over the segments, from (+inf, -1) by a strict <: a NaN is passed over.  j* = -1: the row
//               counts in `rows` and nowhere else.  Otherwise d = th - theta_ref[e*], e* = min(j* + 1, n_ref - 1), a = |d|, not wrapped
//               (the cost does not wrap either), and the record takes: rows += 1; cte2_sum += v*; dth2_sum += d*d; a strictly larger v*
//               (cte2_max, cte_row, cte_seg); a strictly larger a (dth_max, dth_row); last_seg = j*; if v* > tol*tol: off_rows += 1 and
//               off_row = r if it was -1
struct TrackArgs {
    double tol2;              // tol * tol
    nmpc_tracking *rec;       // [B]
};

// One wave per robot the step drove, after the advance (or the plant: the true poses) and the other monitors, before the dispatch: the
// robot's s new poses go to LDS.  Row by row, lanes stride over the segments (consecutive lanes read consecutive samples of x_ref and
// y_ref through the cache), each lane keeps the first minimum of its own ascending segments, wave_argmin names the row's, and lane 0
// folds the row into the record, which it holds in registers from before the first row to after the last.  Every loop is bounded by s
// or n_seg.
__global__ __launch_bounds__(64) void nmpc_loop_track_kernel(LoopView L, LoopStep stp, AssembleArgs g, TrackArgs k)
{
    __shared__ double own[3 * NMPC_MAX_HORIZON];
    const int b = L.robot(blockIdx.x), lane = threadIdx.x;
    // the robot's route: the same for the whole wave (read before any store, so that the loads can be scalar)
    const LoopRoute &rt = g.routes[L.route_of[b]];
    const double *xr = g.tab + rt.xr, *yr = g.tab + rt.yr, *thr = g.tab + rt.thr;
    const int n = rt.n_ref, n_seg = n > 1 ? n - 1 : 1, s = L.s, row0 = stp.traj_row;
    stage_rows<3>(own, L, b, row0, s);
    nmpc_tracking c = k.rec[b];
    for (int i = 0; i < s; ++i) {
        const double x = own[3 * i], y = own[3 * i + 1], th = own[3 * i + 2];
        const int r = row0 + i;
        double bv = __builtin_inf();
        int bj = LOOP_NONE;
        for (int j = lane; j < n_seg; j += 64) {
            const int e = j + 1 < n ? j + 1 : n - 1;
            double cx, cy;
            const double v = segment_closest(x, y, xr[j], yr[j], xr[e], yr[e], j > 0, cx, cy);      // (segment 0 runs on backwards)
            if (v < bv) { bv = v; bj = j; }               // (a lane's segments ascend: among equal values the first stays)
        }
        wave_argmin(bv, bj);
        if (lane == 0) {
            c.rows += 1;
            if (bj != LOOP_NONE) {
                const int e = bj + 1 < n ? bj + 1 : n - 1;
                const double d = th - thr[e];
                const double a = d < 0.0 ? -d : d;
                c.cte2_sum = c.cte2_sum + bv;
                c.dth2_sum = c.dth2_sum + d * d;
                if (bv > c.cte2_max) { c.cte2_max = bv; c.cte_row = r; c.cte_seg = bj; }
                if (a > c.dth_max) { c.dth_max = a; c.dth_row = r; }
                c.last_seg = bj;
                if (bv > k.tol2) {
                    c.off_rows += 1;
                    if (c.off_row == -1) c.off_row = r;
                }
            }
        }
    }
    if (lane == 0) k.rec[b] = c;
}

// ---- drive log: each robot's applied controls and solve outcomes (nmpc_loop_set_log; the rule is DESIGN.md section 5.9).  It observes:
// its four tables are the only things it writes.
struct LogArgs {
    double *ctrl;             // [max_steps * s][B][2]
    nmpc_step_record *rec;    // [max_steps][B]
    nmpc_drive_summary *sum;  // [B]
    nmpc_step_totals *tot;    // [max_steps]
};

// One thread per robot the step drove, after the advance and the monitors and before the dispatch: U is what the advance applied, st the
// step's statuses (scattered), P the parameter vectors as the solve read them (p[3], p[4]: the controls before this step's first) and
// `leg` the missions' array as the solve found it (NULL: no missions).  The thread copies the s control pairs and the record, walks the
// step's s + 1 trajectory rows for the length and folds everything into the robot's summary, field by field in global memory (exits is
// indexed by the status).  Unfused f64; a comparison that is false keeps a maximum.  With a plant (below) the controls logged stay the
// COMMANDED ones, U as the solve returned it (what acted is the plant's `applied`), and the length walks the true rows.
__global__ __launch_bounds__(256) void nmpc_loop_log_kernel(LoopView L, LoopStep stp, LogArgs g, const int *leg)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stp.nact) return;
    const int b = L.robot(i), s = L.s;
    const double *u = L.U + (size_t)b * L.n_u, *p = L.P + (size_t)b * L.n_p;
    const nmpc_status st = L.st[b];
    nmpc_step_record r;
    r.exit_status = st.exit_status; r.leg = leg ? leg[b] : 0;
    r.num_inner_iterations = st.num_inner_iterations; r.num_outer_iterations = st.num_outer_iterations;
    r.cost = st.cost; r.f2_norm = st.f2_norm; r.solve_time_ms = st.solve_time_ms;
    g.rec[(size_t)(stp.step - 1) * L.B + b] = r;
    nmpc_drive_summary *m = g.sum + b;
    m->steps = m->steps + 1;
    m->rows = m->rows + s;
    if ((unsigned)st.exit_status < 5u) m->exits[st.exit_status] += 1u;
    m->inner_total = m->inner_total + st.num_inner_iterations;
    if (st.num_inner_iterations > m->inner_max) { m->inner_max = st.num_inner_iterations; m->inner_max_step = stp.step; }
    if (st.f2_norm > m->f2_max) { m->f2_max = st.f2_norm; m->f2_max_step = stp.step; }
    double len = m->length, vm = m->v_abs_max, wm = m->w_abs_max;
    double am = m->acc_abs_max, wam = m->wacc_abs_max, as = m->acc_sq_sum, was = m->wacc_sq_sum;
    double vp = p[3], wp = p[4];
    const double *at = L.row(stp.traj_row - 1, b);           // (traj_row >= 1: the row before the step's first is there)
    double ax = at[0], ay = at[1];
    for (int c = 0; c < s; ++c) {
        const double v = u[2 * c], w = u[2 * c + 1];
        double *out = g.ctrl + ((size_t)(stp.t + c) * L.B + b) * 2;
        out[0] = v; out[1] = w;
        const double *row = L.row(stp.traj_row + c, b);
        const double x = row[0], y = row[1];
        const double dx = x - ax, dy = y - ay;
        len = len + sqrt(dx * dx + dy * dy);
        ax = x; ay = y;
        const double fv = fabs(v), fw = fabs(w);
        if (fv > vm) vm = fv;
        if (fw > wm) wm = fw;
        const double a = (v - vp) / L.ts, wa = (w - wp) / L.ts;
        const double fa = fabs(a), fwa = fabs(wa);
        if (fa > am) am = fa;
        if (fwa > wam) wam = fwa;
        as = as + a * a;
        was = was + wa * wa;
        vp = v; wp = w;
    }
    m->length = len; m->v_abs_max = vm; m->w_abs_max = wm;
    m->acc_abs_max = am; m->wacc_abs_max = wam; m->acc_sq_sum = as; m->wacc_sq_sum = was;
}

// One workgroup, behind nmpc_loop_log_kernel: thread t strides over the rows of the step's active list; a wave reduction, then the
// waves' results through LDS, and thread 0 writes the step's totals.  Every field is independent of the order: integer sums, one
// maximum over the key (inner << 32) | (0xffffffff - b) -- the largest count, and among equals the smallest robot -- and a maximum of
// non-negative finite times.  With nobody active (nact == 0) the row is written as zeros.
__global__ __launch_bounds__(1024) void nmpc_loop_log_totals_kernel(LoopView L, LoopStep stp, LogArgs g)
{
    __shared__ unsigned long long rkey[16], rsum[16];
    __shared__ double rms[16];
    __shared__ unsigned rex[16][5];
    const int t = threadIdx.x, nt = blockDim.x;
    unsigned e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;
    unsigned long long key = 0, sum = 0;
    double ms = 0.0;
    for (int i = t; i < stp.nact; i += nt) {
        const int b = L.robot(i);
        const nmpc_status *st = L.st + b;
        const int e = st->exit_status;
        const unsigned inner = st->num_inner_iterations;
        const double tm = st->solve_time_ms;
        e0 += e == 0; e1 += e == 1; e2 += e == 2; e3 += e == 3; e4 += e == 4;
        sum += inner;
        const unsigned long long k = ((unsigned long long)inner << 32) | (0xffffffffu - (unsigned)b);
        if (k > key) key = k;
        if (tm > ms) ms = tm;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        e0 += __shfl_xor(e0, off); e1 += __shfl_xor(e1, off); e2 += __shfl_xor(e2, off);
        e3 += __shfl_xor(e3, off); e4 += __shfl_xor(e4, off);
        sum += __shfl_xor(sum, off);
        const unsigned long long ok = __shfl_xor(key, off);
        if (ok > key) key = ok;
        const double om = __shfl_xor(ms, off);
        if (om > ms) ms = om;
    }
    if ((t & 63) == 0) {
        const int w = t >> 6;
        rkey[w] = key; rsum[w] = sum; rms[w] = ms;
        rex[w][0] = e0; rex[w][1] = e1; rex[w][2] = e2; rex[w][3] = e3; rex[w][4] = e4;
    }
    __syncthreads();
    if (t == 0) {
        nmpc_step_totals o;
        o.solved = stp.nact;
#pragma unroll
        for (int q = 0; q < 5; ++q) o.exits[q] = 0;
        key = 0; sum = 0; ms = 0.0;
        for (int w = 0; w < nt / 64; ++w) {
#pragma unroll
            for (int q = 0; q < 5; ++q) o.exits[q] += rex[w][q];
            sum += rsum[w];
            if (rkey[w] > key) key = rkey[w];
            if (rms[w] > ms) ms = rms[w];
        }
        o.inner_max = (unsigned)(key >> 32);
        o.inner_max_robot = stp.nact > 0 ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffu)) : 0;
        o.inner_total = sum;
        o.solve_ms_max = ms;
        g.tot[stp.step - 1] = o;
    }
}

// ---- plant: the world does not do what the model says (nmpc_loop_set_plant; the rule is DESIGN.md section 5.9) ----
// Seeded disturbances on what the robot does (actuation), on where that takes it (process) and on what the controller is told
// (measurement).  xi(id, r, c) = nmpc::plant_xi(seed, id, r, c) (nmpc_rng.h): a robot's draws depend on (seed, its id, the trajectory
// row, the channel) and on nothing else.  Unfused f64, the statements in the order written:
//   measurement, at the start of a step, m = traj_row - 1 (the row of the pose being measured; row 0 is the start):
//     meas_x = x + meas[0]*xi(id, m, 5), y and theta likewise with channels 6 and 7; a channel whose sigma is 0 copies the value and
//     draws nothing.  The assembly and nmpc_loop_predict_kernel read the measured pose (a view whose `state` is `meas_state`), nothing
//     else does.
//   plant, in the place of the advance, for control i of the step, r = traj_row + i, (v, w) the commanded pair:
//     t = act_gain[0]*v;  t = t + act_add[0];  va = v + t*xi(id, r, 0)        (skipped, va = v, if act_gain[0] == 0 and act_add[0] == 0)
//     wa likewise with index 1 and channel 1
//     sincos_cw(th)
//     x  = x + ts*(va*cs);  x  = x  + proc[0]*xi(id, r, 2)                    (the second statement skipped if proc[0] == 0)
//     y  = y + ts*(va*sn);  y  = y  + proc[1]*xi(id, r, 3)
//     th = th + ts*wa;      th = th + proc[2]*xi(id, r, 4)
// The trajectory row and `state` are the true pose; last_u is the COMMANDED last control, what the controller knows it sent; the
// terminal test is the advance's, on the true pose and the commanded v; (va, wa) go to applied[t + i][b] if kept.  The sigmas are
// kernel arguments, so a skip is uniform over the launch, and a plant of zeros executes the advance's operations and no others.
struct PlantArgs {
    unsigned long long seed;
    double act_gain[2], act_add[2];       // for v and w
    double proc[3], meas[3];              // x, y, theta
    const unsigned *ids;      // [B]; NULL: robot b has id b
    double *meas_state;       // [B][3]: the measured poses, what the last step's solves were given
    double *applied;          // [max_steps * s][B][2]: the controls that acted, or NULL

    __device__ unsigned id(int b) const { return ids ? ids[b] : (unsigned)b; }
};

// value + sigma * xi, or the value itself where the sigma is 0
__device__ __forceinline__ double plant_add(double value, double sigma, const PlantArgs &p, unsigned id, unsigned row, unsigned channel)
{
    return sigma != 0.0 ? value + sigma * plant_xi(p.seed, id, row, channel) : value;
}

// one thread per active robot, in front of the assembly (launched only if some meas > 0): the pose as the controller is told it
__global__ __launch_bounds__(256) void nmpc_loop_measure_kernel(LoopView L, LoopStep stp, PlantArgs p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stp.nact) return;
    const int b = L.robot(i);
    const unsigned id = p.id(b), m = (unsigned)(stp.traj_row - 1);
    const double x = L.state[3 * b], y = L.state[3 * b + 1], th = L.state[3 * b + 2];
    double *out = p.meas_state + 3 * (size_t)b;
    out[0] = plant_add(x, p.meas[0], p, id, m, 5u);
    out[1] = plant_add(y, p.meas[1], p, id, m, 6u);
    out[2] = plant_add(th, p.meas[2], p, id, m, 7u);
}

// one thread per active robot, in the place of nmpc_loop_advance_kernel: its shape, its terminal test, the rule above
__global__ __launch_bounds__(256) void nmpc_loop_plant_kernel(LoopView L, LoopStep stp, AssembleArgs g, PlantArgs p)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stp.nact) return;
    const int b = L.robot(i);
    const unsigned id = p.id(b);
    const bool act_v = p.act_gain[0] != 0.0 || p.act_add[0] != 0.0, act_w = p.act_gain[1] != 0.0 || p.act_add[1] != 0.0;
    const double *u = L.U + (size_t)b * L.n_u;
    double x = L.state[3 * b], y = L.state[3 * b + 1], th = L.state[3 * b + 2];
    for (int i = 0; i < L.s; ++i) {
        const unsigned r = (unsigned)(stp.traj_row + i);
        const double v = u[2 * i], w = u[2 * i + 1];
        double va = v, wa = w;
        if (act_v) {
            double t = p.act_gain[0] * v;
            t = t + p.act_add[0];
            va = v + t * plant_xi(p.seed, id, r, 0u);
        }
        if (act_w) {
            double t = p.act_gain[1] * w;
            t = t + p.act_add[1];
            wa = w + t * plant_xi(p.seed, id, r, 1u);
        }
        // (a draw goes to its own coordinate only, and the step has read th already: after the three updates is between them)
        unicycle_step(x, y, th, va, wa, L.ts);
        x = plant_add(x, p.proc[0], p, id, r, 2u);
        y = plant_add(y, p.proc[1], p, id, r, 3u);
        th = plant_add(th, p.proc[2], p, id, r, 4u);
        drive_row(L, stp.traj_row + i, b, x, y, th);
        if (p.applied) {
            double *out = p.applied + ((size_t)(stp.t + i) * L.B + b) * 2;
            out[0] = va; out[1] = wa;
        }
    }
    drive_end(L, g, b, u, x, y, th);
}

// ---- missions: a robot at its goal takes up its next route (nmpc_loop_set_missions; the rule is DESIGN.md section 5.9) ----
struct DispatchArgs {
    const int *leg_off;       // [B + 1]: robot b drives the routes leg_route[leg_off[b] .. leg_off[b + 1]) in turn
    const int *leg_route;     // [leg_off[B]]
    int *leg;                 // [B]: the leg a robot is on, counted inside its mission
    int *leg_at;              // [leg_off[B]]: the steps at which each leg ended, -1 = not yet
    int *route_of;            // [B]: LoopView::route_of, written here and nowhere else
};

// One wave per robot the step drove, after the advance (and the monitor) and before the compaction.  A robot whose terminal test holds
// ends its leg at this step; if its mission has another leg it starts that route as a loop started anew from where it stands: window
// search from sample 0, no previous control, a cold solve (the scatter has run: U and Y are the loop's), and done[b] cleared, so that
// the compaction keeps it.  Its state, carried dynamic block, p, status and clearance record stay.  The list is there: missions need
// retirement.
__global__ __launch_bounds__(64) void nmpc_loop_dispatch_kernel(LoopView L, LoopStep stp, DispatchArgs d)
{
    const int b = L.act[blockIdx.x], lane = threadIdx.x;
    // the same for the whole wave (read before any store, so that the loads can be scalar)
    const int fin = L.done[b], leg = d.leg[b], lo = d.leg_off[b], hi = d.leg_off[b + 1];
    if (!fin) return;
    const bool more = lo + leg + 1 < hi;
    const int next = more ? d.leg_route[lo + leg + 1] : 0;
    if (lane == 0) d.leg_at[lo + leg] = stp.step;
    if (!more) return;                        // the last leg: the compaction retires the robot
    double *u = L.U + (size_t)b * L.n_u, *y = L.Y + (size_t)b * L.n1;
    for (int e = lane; e < L.n_u; e += 64) u[e] = 0.0;
    for (int e = lane; e < L.n1; e += 64) y[e] = 0.0;
    if (lane == 0) {
        d.leg[b] = leg + 1;
        d.route_of[b] = next;
        L.idx[b] = 0;
        L.last_u[2 * b] = 0.0; L.last_u[2 * b + 1] = 0.0;
        L.done[b] = 0;
    }
}

// ---- ensemble: per-group pose statistics after every step (nmpc_loop_set_ensemble; the rule is DESIGN.md section 5.9).  It observes:
// its table is the only thing it writes.
// Group g's members m_0 < ... < m_{n-1} are gmem[goff[g] .. goff[g + 1]); every member counts, whoever is active.  Unfused f64:
//   SUM(v): slot t of 256 starts at +0.0 and takes acc = acc + v[m_i] for i = t, t + 256, ... ascending; within each block of 64 slots
//           a[l] = a[l] + a[l + off] for l < off, off = 32, 16, 8, 4, 2, 1 (an xor butterfly leaves that in every lane: IEEE addition
//           commutes); the four block sums give ((w0 + w1) + w2) + w3
//   mean = (SUM x, SUM y, SUM theta) / double(n), one division each
//   dx = x - mean_x, dy, dth likewise; cov = (SUM dx*dx, SUM dx*dy, SUM dy*dy, SUM dth*dth) / double(n), each product rounded first
//   (far2, far_robot): the extreme of (r2, b), r2 = dx*dx + dy*dy, by `r2 > far2 || (r2 == far2 && b < far_robot)` from (-1.0, -1)
//   arrived: retired_at[b] >= 0 on a retiring loop, else done[b] != 0
//   an empty group: zeros, far2 = -1.0, far_robot = -1
struct EnsembleArgs {
    int G;
    const int *goff;          // [G + 1]
    const int *gmem;          // [B]: the groups' members, group after group, ascending inside a group
    nmpc_ensemble_stat *ens;  // [max_steps][G]
};

// the tree's halving inside a block of 64 slots, result in every lane
__device__ __forceinline__ double wave_sum(double a)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off);
    return a;
}

// One workgroup per group, the step's last kernel: behind the log, the dispatch and the compaction (retired_at: the retirement's, this
// step's retirements in it; NULL without retirement).  Thread t is slot t.  Two passes over the members' true poses, the second from
// the cache; each a wave reduction, the four waves' results through LDS, combined by thread 0, which hands the mean back through LDS
// and writes the record.  No group is staged: its size is bounded by B only.
__global__ __launch_bounds__(256) void nmpc_loop_ensemble_kernel(LoopView L, LoopStep stp, EnsembleArgs e, const int *retired_at)
{
    __shared__ double red[4][5], mean[3];
    __shared__ int rint[4];
    const int g = blockIdx.x, t = threadIdx.x, w = t >> 6;
    const int lo = e.goff[g], n = e.goff[g + 1] - lo;
    const int *mem = e.gmem + lo;
    nmpc_ensemble_stat *out = e.ens + (size_t)(stp.step - 1) * e.G + g;
    if (n == 0) {              // (the same for the whole workgroup)
        if (t == 0) {
            nmpc_ensemble_stat o;
            o.n = 0; o.arrived = 0; o.far_robot = -1; o.reserved = 0;
            o.mean[0] = o.mean[1] = o.mean[2] = 0.0;
            o.cov[0] = o.cov[1] = o.cov[2] = o.cov[3] = 0.0;
            o.far2 = -1.0;
            *out = o;
        }
        return;
    }
    const double dn = (double)n;
    double sx = 0.0, sy = 0.0, sth = 0.0;
    int arrived = 0;
    for (int i = t; i < n; i += 256) {
        const int b = mem[i];
        const double *p = L.state + 3 * (size_t)b;
        sx = sx + p[0]; sy = sy + p[1]; sth = sth + p[2];
        arrived += retired_at ? retired_at[b] >= 0 : L.done[b] != 0;
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sth = wave_sum(sth);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) arrived += __shfl_xor(arrived, off);
    if ((t & 63) == 0) { red[w][0] = sx; red[w][1] = sy; red[w][2] = sth; rint[w] = arrived; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) mean[q] = (((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]) / dn;
        arrived = ((rint[0] + rint[1]) + rint[2]) + rint[3];
    }
    __syncthreads();
    const double mx = mean[0], my = mean[1], mth = mean[2];
    double cxx = 0.0, cxy = 0.0, cyy = 0.0, ctt = 0.0, far2 = -1.0;
    int far = -1;
    for (int i = t; i < n; i += 256) {
        const int b = mem[i];
        const double *p = L.state + 3 * (size_t)b;
        const double dx = p[0] - mx, dy = p[1] - my, dth = p[2] - mth;
        const double xx = dx * dx, xy = dx * dy, yy = dy * dy, tt = dth * dth;
        cxx = cxx + xx; cxy = cxy + xy; cyy = cyy + yy; ctt = ctt + tt;
        const double r2 = xx + yy;
        if (r2 > far2 || (r2 == far2 && b < far)) { far2 = r2; far = b; }
    }
    cxx = wave_sum(cxx); cxy = wave_sum(cxy); cyy = wave_sum(cyy); ctt = wave_sum(ctt);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o2 = __shfl_xor(far2, off);
        const int ob = __shfl_xor(far, off);
        if (o2 > far2 || (o2 == far2 && ob < far)) { far2 = o2; far = ob; }
    }
    // (red and rint are free again: thread 0 read them in front of the barrier that published the mean)
    if ((t & 63) == 0) { red[w][0] = cxx; red[w][1] = cxy; red[w][2] = cyy; red[w][3] = ctt; red[w][4] = far2; rint[w] = far; }
    __syncthreads();
    if (t == 0) {
        nmpc_ensemble_stat o;
        o.n = n; o.arrived = arrived; o.reserved = 0;
        o.mean[0] = mx; o.mean[1] = my; o.mean[2] = mth;
#pragma unroll
        for (int q = 0; q < 4; ++q) o.cov[q] = (((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]) / dn;
        far2 = -1.0; far = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (red[k][4] > far2 || (red[k][4] == far2 && rint[k] < far)) { far2 = red[k][4]; far = rint[k]; }
        o.far2 = far2; o.far_robot = far;
        *out = o;
    }
}

}  // namespace nmpc
