// nmpc_plan.h -- a route per robot, planned on device: batched shortest paths over the visibility graph of a scene.
//
// Counterpart of the reference's front-end for one query (src/visibility/visibility.py:69-88: extremitypathfinder's visibility graph over the
// inflated polygons and its shortest path between start and goal), restated as this project's own planner states it
// (`frontend.VisibilityPlanner._free` / `shortest_path`) and widened to a batch: every robot of a fleet its own start and goal, as the
// reference's user calls `PathGenerator.run(graph_map, start, end)` per robot (src/path_generator.py:197-251).  The rule is DESIGN.md
// section 5.11; `frontend.plan_batch_mirror` is its NumPy statement, and the kernels give its bits.
//
// Arithmetic: unfused IEEE f64 + - * / and sqrt in the order the mirror writes them (the library is built with -ffp-contract=off), every
// comparison in the sense the literal code has it, so that one that is false because of a NaN has the same consequence: the segment is
// blocked.  A visibility is a boolean: order of evaluation and early exits are free, and the kernels take none that would diverge a wave.
//
// Bounds: the rounds of the search and the walk back along `prev` are counted loops of at most n = V + 2 passes.  No loop waits on data.
#pragma once

namespace nmpc {

constexpr int PLAN_MAX_NODES = 254;                        // V: a query's n = V + 2 points are strided over 64 lanes, four per lane
constexpr int PLAN_MAX_EDGES = 1024;                       // E: 32 B each in LDS
constexpr int PLAN_MAX_POLYS = PLAN_MAX_EDGES / 3;         // a polygon has three edges at least
constexpr int PLAN_MAX_POINTS = PLAN_MAX_NODES + 2;
constexpr int PLAN_PER_LANE = PLAN_MAX_POINTS / 64;
constexpr int PLAN_VIS_BLOCK = 256;

struct PlanVisArgs {
    int V, E, n_poly;
    int n_seg;                    // segments this launch judges
    int queries;                  // 0: segment s = (node s / V, node s % V); 1: segment s = number s % (2V + 1) of query s / (2V + 1)
    const double *node;           // [V][2]
    const double *edge;           // [E][4] x1 y1 x2 y2: the obstacles' polygons, then the boundary's
    const int *poly_off;          // [n_poly + 1]
    const double *start, *goal;   // [B][2] (queries)
    unsigned char *out;           // [n_seg]: 1 = free
};

// One thread per segment a -> b: is the open segment free (`_free`)?  Blocked if it properly crosses an edge
// (`_seg_intersect_strict`), or if one of its five interior samples lies strictly inside an obstacle or not inside the boundary, whose
// edges count as inside (`_point_in_polygon`: the on-edge test over all the polygon's edges first, then the even-odd crossing count).
// The workgroup stages the edges, each edge's on-edge tolerance and the polygon offsets in LDS; every thread then walks all polygons and
// all edges (LDS reads at one address per wave: broadcasts), keeping for the polygon at hand one on-edge bit and one parity bit per
// sample.  A thread past the end of the list judges the last segment again and stores nothing.
__global__ __launch_bounds__(PLAN_VIS_BLOCK) void nmpc_plan_visible_kernel(PlanVisArgs a)
{
    __shared__ double ed[PLAN_MAX_EDGES][4];
    __shared__ double etol[PLAN_MAX_EDGES];
    __shared__ int poff[PLAN_MAX_POLYS + 1];
    const int V = a.V, E = a.E, n_poly = a.n_poly;
    for (int e = threadIdx.x; e < E; e += PLAN_VIS_BLOCK) {
        const double x1 = a.edge[4 * e], y1 = a.edge[4 * e + 1], x2 = a.edge[4 * e + 2], y2 = a.edge[4 * e + 3];
        ed[e][0] = x1; ed[e][1] = y1; ed[e][2] = x2; ed[e][3] = y2;
        const double ex = x2 - x1, ey = y2 - y1;
        const double h = sqrt(ex * ex + ey * ey);
        etol[e] = 1e-9 * (h > 1.0 ? h : 1.0);
    }
    for (int k = threadIdx.x; k <= n_poly; k += PLAN_VIS_BLOCK) poff[k] = a.poly_off[k];
    __syncthreads();
    const int s_own = blockIdx.x * PLAN_VIS_BLOCK + threadIdx.x;
    const int s = s_own < a.n_seg ? s_own : a.n_seg - 1;
    double ax, ay, bx, by;
    if (a.queries) {
        const int per = 2 * V + 1;
        const int q = s / per, k = s - q * per;
        const double *pa = k >= V && k < 2 * V ? a.goal + 2 * (size_t)q : a.start + 2 * (size_t)q;
        const double *pb = k < V ? a.node + 2 * k : (k < 2 * V ? a.node + 2 * (k - V) : a.goal + 2 * (size_t)q);
        ax = pa[0]; ay = pa[1]; bx = pb[0]; by = pb[1];
    } else {
        const int i = s / V, j = s - i * V;
        ax = a.node[2 * i]; ay = a.node[2 * i + 1]; bx = a.node[2 * j]; by = a.node[2 * j + 1];
    }
    const double lx = ax - bx, ly = ay - by;
    const bool coincide = sqrt(lx * lx + ly * ly) < 1e-12;
    const double ux = bx - ax, uy = by - ay;
    constexpr int NS = 5;
    const double at[NS] = {0.5, 0.25, 0.75, 0.0625, 0.9375};
    double sx[NS], sy[NS];
#pragma unroll
    for (int m = 0; m < NS; ++m) { sx[m] = ax + at[m] * ux; sy[m] = ay + at[m] * uy; }
    bool blocked = false;
    for (int k = 0; k < n_poly; ++k) {
        const int lo = poff[k], hi = poff[k + 1];
        unsigned on = 0, in = 0;                   // per sample: on an edge of this polygon / inside by the crossing count
        for (int e = lo; e < hi; ++e) {
            const double x1 = ed[e][0], y1 = ed[e][1], x2 = ed[e][2], y2 = ed[e][3], tol = etol[e];
            const double ex = x2 - x1, ey = y2 - y1;
            const double o1 = ux * (y1 - ay) - uy * (x1 - ax);
            const double o2 = ux * (y2 - ay) - uy * (x2 - ax);
            const double o3 = ex * (ay - y1) - ey * (ax - x1);
            const double o4 = ex * (by - y1) - ey * (bx - x1);
            if (o1 * o2 < -1e-9 && o3 * o4 < -1e-9) blocked = true;
            const double xlo = (x2 < x1 ? x2 : x1) - 1e-9, xhi = (x2 > x1 ? x2 : x1) + 1e-9;
            const double ylo = (y2 < y1 ? y2 : y1) - 1e-9, yhi = (y2 > y1 ? y2 : y1) + 1e-9;
#pragma unroll
            for (int m = 0; m < NS; ++m) {
                const double x = sx[m], y = sy[m];
                const double cross = ex * (y - y1) - ey * (x - x1);
                if (fabs(cross) <= tol && xlo <= x && x <= xhi && ylo <= y && y <= yhi) on |= 1u << m;
                if ((y1 > y) != (y2 > y)) {
                    const double xi = x1 + ((y - y1) * ex) / ey;
                    if (xi > x) in ^= 1u << m;
                }
            }
        }
        constexpr unsigned ALL = (1u << NS) - 1;
        if (k < n_poly - 1) blocked = blocked || (~on & in & ALL) != 0;      // an obstacle: a sample strictly inside
        else blocked = blocked || (~(on | in) & ALL) != 0;                   // the boundary: a sample not inside
    }
    if (s_own < a.n_seg) a.out[s_own] = coincide || !blocked ? 1 : 0;
}

struct PlanPathArgs {
    int V;
    const double *node;           // [V][2]
    const unsigned char *nn;      // [V][V] node-node visibility; a pair is read at (lower, higher) index, as `shortest_path` judges it
    const double *start, *goal;   // [B][2]
    const unsigned char *qvis;    // [B][2V + 1]: (start, node k), (goal, node k), (start, goal)
    int *n_wp;                    // [B]: waypoints of the path, 0 = none
    int *wp;                      // [B][V + 2]: their point indices from 0 (start) to 1 (goal), -1 behind them
    double *length;               // [B]: dist[1], +inf without a path
};

// One wave per query: Dijkstra over the points [start, goal] + nodes with the tie rule of the mirror.  Point j belongs to lane j % 64,
// which keeps dist and the settled flag of its up to four points in registers; coordinates, prev and the query's own visibility bytes
// are in LDS.  A round settles the unsettled point with the smallest (dist, index) -- every lane's first minimum, then wave_argmin --
// stops if that distance is not finite (nothing reachable is left) or the point is the goal, and relaxes the unsettled points it sees
// on the strict d < dist[j].  Then lane 0 walks prev back from the goal, n steps at the most, and the wave writes wp in forward order.
__global__ __launch_bounds__(64) void nmpc_plan_path_kernel(PlanPathArgs a)
{
    __shared__ double px[PLAN_MAX_POINTS], py[PLAN_MAX_POINTS];
    __shared__ int prev[PLAN_MAX_POINTS], back[PLAN_MAX_POINTS];
    __shared__ unsigned char qv[2 * PLAN_MAX_NODES + 4];
    __shared__ int count;
    const int q = blockIdx.x, lane = threadIdx.x, V = a.V, n = V + 2;
    for (int j = lane; j < n; j += 64) {
        const double *p = j == 0 ? a.start + 2 * (size_t)q : (j == 1 ? a.goal + 2 * (size_t)q : a.node + 2 * (j - 2));
        px[j] = p[0]; py[j] = p[1];
        prev[j] = -1;
    }
    for (int k = lane; k < 2 * V + 1; k += 64) qv[k] = a.qvis[(size_t)q * (2 * V + 1) + k];
    __syncthreads();
    constexpr int NONE = 0x7fffffff;
    double dist[PLAN_PER_LANE];
    bool settled[PLAN_PER_LANE];
#pragma unroll
    for (int k = 0; k < PLAN_PER_LANE; ++k) {
        dist[k] = lane + 64 * k == 0 ? 0.0 : __builtin_inf();
        settled[k] = lane + 64 * k >= n;          // a slot beyond the query's points is never picked and never relaxed
    }
    bool reached = false;
    for (int r = 0; r < n; ++r) {
        double d = __builtin_inf();
        int i = NONE;
#pragma unroll
        for (int k = 0; k < PLAN_PER_LANE; ++k)
            if (!settled[k] && dist[k] < d) { d = dist[k]; i = lane + 64 * k; }
        wave_argmin(d, i);
        if (!(d < __builtin_inf())) break;        // (wave-uniform, like every exit of this loop)
#pragma unroll
        for (int k = 0; k < PLAN_PER_LANE; ++k)
            if (lane + 64 * k == i) settled[k] = true;
        if (i == 1) { reached = true; break; }
        const double xi = px[i], yi = py[i];
#pragma unroll
        for (int k = 0; k < PLAN_PER_LANE; ++k) {
            const int j = lane + 64 * k;
            if (settled[k]) continue;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            const unsigned char v = lo == 0 ? (hi == 1 ? qv[2 * V] : qv[hi - 2])
                                            : (lo == 1 ? qv[V + hi - 2] : a.nn[(lo - 2) * V + (hi - 2)]);
            if (v) {
                const double dx = xi - px[j], dy = yi - py[j];
                const double c = d + sqrt(dx * dx + dy * dy);
                if (c < dist[k]) { dist[k] = c; prev[j] = i; }
            }
        }
    }
    const double len = __shfl(dist[0], 1);        // dist[1]
    __syncthreads();
    if (lane == 0) {
        int cnt = 0;
        if (reached) {
            int j = 1;
            back[0] = 1;
            cnt = 1;
            for (int step = 0; step < n && j != 0; ++step) {
                j = prev[j];
                if (j < 0 || j >= n || cnt >= n) { j = -1; break; }      // not a path: a corrupt prev ends here, not in a cycle
                back[cnt++] = j;
            }
            if (j != 0) cnt = 0;
        }
        count = cnt;
        a.n_wp[q] = cnt;
        a.length[q] = len;
    }
    __syncthreads();
    const int cnt = count;
    for (int j = lane; j < n; j += 64) a.wp[(size_t)q * n + j] = j < cnt ? back[cnt - 1 - j] : -1;
}

}  // namespace nmpc
