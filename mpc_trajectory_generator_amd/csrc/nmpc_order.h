// nmpc_order.h -- the launch order of a batch: hardness levels from the inputs or the previous solve, a stable partition by level.
#pragma once

// ---------------------------------------------------------------------------------------------
// launch-order heuristic.  Iteration counts are heavy-tailed and a batch ends when its slowest
// instance does, so instances that LOOK hard are handed out first (list scheduling, longest expected
// first).  "Looks hard" uses the inputs only: the reference samples of the horizon pass within
// SCHED_CLEARANCE of a circle / ellipse, or the reference bends by more than SCHED_BEND inside
// the horizon.  Only the order of processing changes; every instance's result is independent of it.
// ---------------------------------------------------------------------------------------------
namespace nmpc {
constexpr double SCHED_CLEARANCE = 0.6;    // m
constexpr double SCHED_GRAZE = 0.05;       // m: the reference itself touches an obstacle's edge -- its penalty will be active
constexpr double SCHED_BEND = 0.05;        // rad, summed |heading change| of the reference samples
constexpr double SCHED_SPEED_GAP = 1.0;    // m/s between the last applied and the first reference speed: the
                                           // acceleration bounds stay active for several stages (many outer iterations)
constexpr int SCHED_LEVELS = 13;           // hardness level = 4 x (grazes) + 4 x (grazes within the first half of the horizon) + other criteria met

__global__ void nmpc_classify_kernel(KArgs a, unsigned char *cls)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const int N = a.pb.N, nobs = a.pb.nobs, ndyn = a.pb.ndyn;
    const double *p = a.p + (size_t)b * a.n_p;
    const double *ps = p + NZ + N, *pd = ps + 3 * nobs, *pr = pd + 5 * ndyn * N;
    bool hard = false, graze = false, early = false;
    double bend = 0.0;
    for (int t = 0; t < N; ++t) {
        const double rx = pr[3 * t], ry = pr[3 * t + 1];
        if (t > 0) {
            double d = pr[3 * t + 2] - pr[3 * t - 1];
            d = d - 6.283185307179586 * rint(d * 0.15915494309189535);
            bend += fabs(d);
        }
        for (int k = 0; k < nobs; ++k) {
            const double r = ps[3 * k + 2];
            if (r > 0.0) {
                const double dx = rx - ps[3 * k], dy = ry - ps[3 * k + 1], lim = r + SCHED_CLEARANCE, lim0 = r + SCHED_GRAZE;
                hard |= dx * dx + dy * dy < lim * lim;
                graze |= dx * dx + dy * dy < lim0 * lim0;
                early |= 2 * t < N && dx * dx + dy * dy < lim0 * lim0;      // the sooner the robot meets the obstacle, the longer the solve
            }
        }
        for (int k = 0; k < ndyn; ++k) {
            const double *e = pd + (k * N + t) * 5;
            const double dx = rx - e[0], dy = ry - e[1], lim = fmax(e[2], e[3]) + SCHED_CLEARANCE, lim0 = fmin(e[2], e[3]) + SCHED_GRAZE;
            hard |= dx * dx + dy * dy < lim * lim;
            graze |= dx * dx + dy * dy < lim0 * lim0;
        }
    }
    const bool gap = fabs(p[NZ] - p[3]) > SCHED_SPEED_GAP;
    // the horizon reaches the goal: the reference is padded with the end pose (degenerate segments, braking profile)
    const bool goal = pr[3 * (N - 1)] == pr[3 * (N - 2)] && pr[3 * (N - 1) + 1] == pr[3 * (N - 2) + 1];
    cls[b] = (unsigned char)((graze ? 4 : 0) + (early ? 4 : 0) + (hard ? 1 : 0) + (bend > SCHED_BEND ? 1 : 0) + (gap ? 1 : 0) + (goal ? 1 : 0));
}

// The same levels from what a receding-horizon loop already knows: the evaluation passes each instance's solve took one step earlier
// (nmpc_status.reserved).  Consecutive solves of one robot are alike -- the previous count is a far better predictor of the next than anything the
// inputs show -- so the closed loop hands out its instances longest-last-time first (nmpc_loop_step); level = position of the count's top bit.
__global__ void nmpc_classify_prev_kernel(int B, const nmpc_status *prev, unsigned char *cls)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned n = prev[b].reserved;
    const int lvl = n < 32u ? 0 : (31 - __clz((int)n)) - 4;      // 32..63 passes -> 1, 64..127 -> 2, ...
    cls[b] = (unsigned char)(lvl > SCHED_LEVELS - 1 ? SCHED_LEVELS - 1 : lvl);
}

// stable partition of 0..B-1 by level (highest first); one block, deterministic
__global__ void nmpc_order_kernel(int B, const unsigned char *cls, int *order)
{
    __shared__ int cnt[SCHED_LEVELS][1024];
    const int t = threadIdx.x, nt = blockDim.x;
    const int chunk = (B + nt - 1) / nt;
    const int lo = t * chunk < B ? t * chunk : B, hi = lo + chunk < B ? lo + chunk : B;
    int c[SCHED_LEVELS];
#pragma unroll
    for (int k = 0; k < SCHED_LEVELS; ++k) c[k] = 0;
    for (int i = lo; i < hi; ++i) {
#pragma unroll
        for (int k = 0; k < SCHED_LEVELS; ++k) c[k] += cls[i] == k;
    }
#pragma unroll
    for (int k = 0; k < SCHED_LEVELS; ++k) cnt[k][t] = c[k];
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {            // inclusive scans, one per level
        int v[SCHED_LEVELS];
#pragma unroll
        for (int k = 0; k < SCHED_LEVELS; ++k) v[k] = t >= off ? cnt[k][t - off] : 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SCHED_LEVELS; ++k) cnt[k][t] += v[k];
        __syncthreads();
    }
    int pos[SCHED_LEVELS], base = 0;                    // write cursor of this chunk inside each level's segment
#pragma unroll
    for (int k = SCHED_LEVELS - 1; k >= 0; --k) {
        pos[k] = base + cnt[k][t] - c[k];
        base += cnt[k][nt - 1];
    }
    for (int i = lo; i < hi; ++i) {
        const int k = cls[i];
#pragma unroll
        for (int j = 0; j < SCHED_LEVELS; ++j) if (k == j) order[pos[j]++] = i;
    }
}
}  // namespace nmpc
